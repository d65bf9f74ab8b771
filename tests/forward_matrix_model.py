"""Plain float64 references and case tables of the forward MATRIX kernels of libos2d_hip.so (include/os2d_hip.h): the three
correlation entry points and the inference convolutions of the TransformNet, fp32 and split-fp16.  Test infrastructure, CPU only;
tests/test_forward_matrix_model.py holds the models to their own conditions, tests/test_forward_matrix_gpu.py compares the
kernels with them.

Inputs are the float32 values the kernels read, converted to float64; everything downstream is float64.  The convolution model
is the UNFOLDED layer as the reference writes it (conv, eval-mode BatchNorm, ReLU), so that a GPU test checks the packing (fold
and re-layout) together with the kernel.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import backward_model as M
import train_forward_f16x3_model as SHB
import util
from oracle import head_oracle as O
from os2d_amd.utils import synthetic

T = O.TEMPLATE
K = T * T
F64 = torch.float64
U32 = 2.0 ** -24                     # unit round-off of fp32
SPLIT_EXP = 12                       # both correlation operands and the normalised tensor are stored times 2^12


# ---------------------------------------------------------------------------------------------------------- correlation
# (A, B, C, H, W), the smallest shapes at which the three kernels can still go wrong:
#   C     1, 7, 16, 17, 33, 67: either side of the 16-channel K chunk of corr_mfma.hip and of the 32-channel chunk (four
#         8-channel groups) of corr_f16x3.hip, and inside a zero-padded 8-channel group
#   H*W   1, 15, 128, 129, 256, 257, 258, 260: below, on and one past the position tiles (128 for fp32, 128 / 256 for f16x3); 15,
#         129, 257 and 258 are no multiple of 4 (scalar loads and stores)
#   B     9 at a small map: 9 * 228 stacked rows over 256-row tiles, a work-group of the packed form crosses class boundaries
#   B     97 at 258 / 260 positions: more than 256 work-groups of 128 positions in BOTH forms (97 * 3 padded, ceil(97 * 228 /
#         256) * 3 = 261 packed), where os2d_launch_corr_f16x3 switches to the 256-position tile
CORR_CASES = [(3, 2, 1, 1, 1), (1, 2, 7, 3, 5), (2, 3, 16, 8, 16), (1, 2, 17, 3, 43), (1, 1, 33, 16, 16), (1, 2, 67, 1, 257),
              (1, 9, 7, 3, 5), (1, 97, 17, 6, 43), (1, 97, 16, 13, 20)]


MIN_LIVE_NORM = 0.5                  # see corr_inputs


def corr_case_id(case):
    return "A{}_B{}_C{}_{}x{}".format(*case)


def corr_zero_at(case):
    """(image, position) whose feature vector is exactly zero: the last position of image 0."""
    A, B, C, H, W = case
    return 0, H * W - 1


def corr_dead_at(case):
    """(image, class, position) whose 225 correlation values are all < 0: position 0 of the last class; of the last image, and
    with a single position (where image 0 is the zero vector) of image 1 - the last image stays alive."""
    A, B, C, H, W = case
    if H * W == 1:
        assert A >= 3
        return 1, B - 1, 0
    return A - 1, B - 1, 0


@functools.lru_cache(maxsize=None)
def corr_inputs(case):
    """fm [A,C,H,W] float32, non-negative as backbone features are, and q_hat [B,C,15,15] float32 of both signs (about half of the
    correlation values are negative: the ReLU works), L2-normalised over the channels as os2d_class_prepare leaves it (|q| <= 1:
    the split operand is q * 2^12 in fp16).  The last class is non-negative and the feature vector at the dead position
    non-positive: every one of its 225 correlation values there is negative.

    Conditioning: the normalised tensor is relu(corr) / (norm + 1e-6), so to first order its error is the correlation's error
    divided by the norm of the column.  The project's 2e-6 holds for both tensors on backbone-like features, whose columns have
    norms of order 1; a column that is dead but for a few tiny values (norm 1e-3: sign-mixed features give some) amplifies the
    correlation's 2e-7 to 1e-4 for ANY fp32 correlation, a property of that input and not of a kernel.  MIN_LIVE_NORM is the
    condition the inputs keep (tests/test_forward_matrix_model.py): a column is dead (norm 0) or has a norm of at least 0.5."""
    A, B, C, H, W = case
    g = torch.Generator().manual_seed(8000 + 131 * C + 7 * H * W + A + B)
    fm = torch.randn(A, C, H * W, generator=g).abs()
    q = torch.randn(B, C, T, T, generator=g)
    q[B - 1] = q[B - 1].abs() + 0.05
    q_hat = O.l2_normalize_channels(q.double(), 1e-5).float()
    a0, n0 = corr_zero_at(case)
    fm[a0, :, n0] = 0.0
    a1, _, n1 = corr_dead_at(case)
    fm[a1, :, n1] = -fm[a1, :, n1].abs() - 0.05
    if H * W == 1:
        fm[A - 1, :, 0] = fm[A - 1, :, 0].abs() + 0.05            # the one position of the last image: alive for every class
    return fm.reshape(A, C, H, W).contiguous(), q_hat.contiguous()


def corr_model(fm, q_hat):
    """fm [A,C,H,W], q_hat [B,C,15,15] -> float64
      corr      [A*B,225,H*W]  sum_c q_hat[b,c,i,j] f[a,c,n] / (||f[a,:,n]|| + 1e-5) at k = j*15 + i (reference head.py:339-350)
      rnorm     [A*B,225,H*W]  relu, then L2 over the 225 channels with eps 1e-6 (head.py:650)
      inv_norm  [A*B,H*W]      1 / (norm + 1e-6)"""
    fm, q_hat = fm.to(F64), q_hat.to(F64)
    A, C, H, W = fm.shape
    B = q_hat.size(0)
    f = fm.reshape(A, C, H * W)
    f_hat = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-5)
    qk = q_hat.permute(0, 3, 2, 1).reshape(B, K, C)               # [b, j*15 + i, c]
    corr = torch.einsum("bkc,acn->abkn", qk, f_hat).reshape(A * B, K, H * W)
    r = corr.clamp(min=0)
    norm = r.pow(2).sum(1).sqrt()
    inv = 1.0 / (norm + 1e-6)
    return corr, r * inv.unsqueeze(1), inv


@functools.lru_cache(maxsize=None)
def corr_reference(case):
    """(corr, rnorm, inv_norm) of a case: computed once, shared by every test of the case, never written to."""
    return corr_model(*corr_inputs(case))


def split_groups(C):
    """8-channel groups of the split correlation operands: ceil(C / 8) padded to a multiple of 4."""
    return -(-(-(-C // 8)) // 4) * 4


def class_split_encode(qp):
    """qp [B,C,256] float32 -> the operand os2d_class_split writes, built on the host: bytes of [B, G, hi|lo, 256, 8] halves,
    hi = rn16(v * 2^12), lo = rn16(v * 2^12 - hi) (the difference is exact in fp32); zero pad channels and groups."""
    B, C, _ = qp.shape
    G = split_groups(C)
    full = np.zeros((B, G * 8, 256), dtype=np.float32)
    full[:, :C] = qp.detach().to(torch.float32).numpy() * np.float32(2.0 ** SPLIT_EXP)
    hi, lo = SHB.split(full)
    units = np.stack([hi, lo], 1).reshape(B, 2, G, 8, 256).transpose(0, 2, 1, 4, 3)       # [B, G, 2, 256, 8]
    return torch.from_numpy(np.ascontiguousarray(units).view(np.uint8).reshape(-1))


# ---------------------------------------------------------------------------------------------------------- convolutions
# (H, W); Ws = W + 3 cells per plane row, tiles of 256 cells (fp32, the standard f16x3 shape) or 128 (the fine f16x3 shape)
#   1x1, 2x2   smallest maps          9x13   one tile           8x13   H * Ws = 128 exactly (the fine shape's tile)
#   16x13      H * Ws = 256 exactly   17x13  one row into the next tile
#   1x209      the widest direct 7x7 map, one row
#   3x316, 3x317 (layers 2 and 3)     the last linear slab and the first column strips
CONV_SHAPES = [(1, 1), (2, 2), (9, 13), (8, 13), (16, 13), (17, 13), (1, 209)]
CONV_SHAPES_5X5 = CONV_SHAPES + [(3, 316), (3, 317)]
CONV_NB = 3                          # every case is computed for NB = 3; the NB = 1 calls are its slices
STATES = ("edited", "adversarial")
LAYER_CHANNELS = {1: (K, 128), 2: (128, 64)}
LAYER_KEYS = {1: ("conv.0", "conv.1"), 2: ("conv.3", "conv.4"), 3: ("linear", None)}
# BatchNorm channels of the edited state (both BatchNorm layers)
GAMMA_ZERO, GAMMA_NEGATIVE, VAR_ZERO = 5, 9, 12


def shape_id(shape):
    return "{}x{}".format(*shape)


@functools.lru_cache(maxsize=None)
def conv_state(kind, P):
    """"edited": synthetic.make_transform_net_state with gamma = 0, gamma < 0 and running_var = 0 planted in both BatchNorm
    layers; "adversarial": util.adversarial_transform_net_state (channel scales over nine decades)."""
    if kind == "adversarial":
        return util.adversarial_transform_net_state(P, seed=11)
    st = {k: v.clone() for k, v in synthetic.make_transform_net_state(P, seed=5).items()}
    for bn in ("conv.1", "conv.4"):
        st[bn + ".weight"][GAMMA_ZERO] = 0.0
        st[bn + ".weight"][GAMMA_NEGATIVE] = -st[bn + ".weight"][GAMMA_NEGATIVE].abs()
        # (gamma compensated as util.adversarial_transform_net_state does: the folded scale gamma / sqrt(var + eps) stays what it was)
        st[bn + ".weight"][VAR_ZERO] *= torch.sqrt(O.BN_EPS / (st[bn + ".running_var"][VAR_ZERO] + O.BN_EPS))
        st[bn + ".running_var"][VAR_ZERO] = 0.0
    return st


@functools.lru_cache(maxsize=None)
def conv_net(kind, P):
    """The state in a CPU TransformationNet: ``_folded`` and ``range_plan`` of the product's host code."""
    from os2d_amd.modeling.head import TransformationNet
    net = TransformationNet(output_dim=P, use_cuda=False)
    net.load_state_dict(conv_state(kind, P))
    return net.eval()


def conv_layer_model(layer, x, state, P):
    """One TransformNet layer as the reference writes it (head.py:619-629), float64: x [NB,Cin,H,W] -> conv, eval-mode BatchNorm
    with the running statistics and ReLU for layers 1 and 2; the convolution alone for layer 3 ([NB,P,H,W])."""
    conv, bn = LAYER_KEYS[layer]
    w, b = state[conv + ".weight"].to(F64), state[conv + ".bias"].to(F64)
    assert layer != 3 or w.size(0) == P
    y = F.conv2d(x.to(F64), w, b, padding=w.size(-1) // 2)
    if bn is None:
        return y
    y = F.batch_norm(y, state[bn + ".running_mean"].to(F64), state[bn + ".running_var"].to(F64), state[bn + ".weight"].to(F64),
                     state[bn + ".bias"].to(F64), training=False, eps=O.BN_EPS)
    return F.relu(y)


@functools.lru_cache(maxsize=None)
def typical_activations(kind):
    """(h1 [128], h2 [64]): the largest activation of every channel when the float64 model runs the state's first two layers
    on a 6x7 map of two random pairs - the magnitudes a layer's input really has under this state (0 for a dead channel)."""
    g = torch.Generator().manual_seed(77)
    x = O.l2_normalize_channels(torch.randn(2, K, 6, 7, generator=g, dtype=F64).clamp(min=0), 1e-6)
    h1 = conv_layer_model(1, x, conv_state(kind, 6), 6)
    h2 = conv_layer_model(2, h1, conv_state(kind, 6), 6)
    return h1.amax(dim=(0, 2, 3)), h2.amax(dim=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def conv_input(layer, kind, shape):
    """The layer's input [3,Cin,H,W] float32, built on the host - no kernel's and no other layer's output.
      layer 1     relu of a Gaussian tensor, L2-normalised over the 225 channels (what head.py:650 hands the layer: the range plan
                  of the split-fp16 path rests on norms <= 1); one location of the last pair is the zero vector
      layer 2, 3  non-negative and half zeros, as ReLU outputs are: channel c is typical[c] / 3 * relu(Gaussian) with the
                  channel's magnitude of ``typical_activations``, capped at the channel's bound of ``range_plan`` (which a constant
                  channel - gamma = 0 - sits on): the magnitudes follow the channel scales of the state (nine decades in the
                  adversarial one), a dead channel is all zero, and the layer-3 outputs stay O(1) as transform parameters are."""
    H, W = shape
    g = torch.Generator().manual_seed(9000 + 1000 * layer + 17 * H + W + (0 if kind == "edited" else 500))
    cin = {1: K, 2: 128, 3: 64}[layer]
    x = torch.randn(CONV_NB, cin, H, W, generator=g, dtype=F64).clamp(min=0)
    if layer == 1:
        x = O.l2_normalize_channels(x, 1e-6)
        x[CONV_NB - 1, :, H - 1, W // 2] = 0.0
    else:
        bound = conv_net(kind, 6).range_plan()["bounds"][layer - 2]
        x = torch.minimum(x * (typical_activations(kind)[layer - 2] / 3.0).view(1, -1, 1, 1), bound.view(1, -1, 1, 1))
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def conv_reference(layer, kind, shape, P=6):
    """The model's output for ``conv_input``: computed once per case, never written to."""
    return conv_layer_model(layer, conv_input(layer, kind, shape), conv_state(kind, P), P)


def conv_error_ceiling(layer, kind, shape, mode="f32"):
    """The bound of |got - ref|_max / |ref|_max for layers 1 and 2, from the float64 model of the case.

    An fp32 accumulation of K products, in any order, is off by at most (K - 1) u sum_k |w_k x_k| to first order, u = 2^-24;
    the kernels fold BatchNorm in fp32 first (w * (gamma / sqrtf(var + eps)): four roundings per weight) and add the folded bias
    (three roundings) - 8 more units, also on S below, which includes |b|:
        S = max over outputs and cells of sum_k |w_k x_k| + |b|           (folded weights, float64)
        f32    (K + 8) u S / |ref|_max                                    K = 225 * 49 = 11025 or 128 * 25 = 3200
    Split fp16 (tests/f16x3_model.py): an operand is hi + lo with |x - hi - lo| <= 2^-22 |x| (two roundings to 11 bits), for both
    operands, and the product lo * lo (<= 2^-22 |w x|) is dropped: 3 * 2^-22 S; the output is stored as hi + lo again: 2^-22 of
    the value itself, at most of |ref|_max:
        f16x3  f32 + (3 * 2^-22 S) / |ref|_max + 2^-22
        f16x2  the weights are their fp16 roundings only, 2^-11 |w| each: f16x3 + 2^-11 S / |ref|_max"""
    net = conv_net(kind, 6)
    w, b = net._folded()[layer - 1]
    x = conv_input(layer, kind, shape).to(F64)
    S = float((F.conv2d(x.abs(), w.abs(), None, padding=w.size(-1) // 2) + b.abs().view(1, -1, 1, 1)).max())
    ref_max = float(conv_reference(layer, kind, shape).abs().max())
    k = w[0].numel()
    assert k == {1: 11025, 2: 3200}[layer]
    bound = (k + 8) * U32 * S / ref_max
    if mode in ("f16x3", "f16x2"):
        bound += 3 * 2.0 ** -22 * S / ref_max + 2.0 ** -22
    if mode == "f16x2":
        bound += 2.0 ** -11 * S / ref_max
    return bound


def pack_planes_input(layer, x):
    """x [NB,Cin,H,W] float32 -> the fp32 kernels' input [NB,CinP,PLANE]: zero-bordered planes; layer 1 has the 226th, all-zero
    plane of rnorm (the kernel consumes channel pairs)."""
    p = M.pack_planes(x)
    if layer == 1:
        p = torch.cat([p, torch.zeros_like(p[:, :1])], dim=1)
    return p.contiguous()


def shb_input(x, exp):
    """x [NB,Cin,H,W] float32, exp [Cin] int -> the split-half blocked buffer of the f16x3 kernels as bytes."""
    return torch.from_numpy(SHB.pack(x.numpy(), exp.numpy()).view(np.uint8).reshape(-1))


def shb_output(buf, exp, channels, H, W):
    """Bytes of an SHB buffer -> (values [NB,channels,H,W] float64 with the channel scales undone, the [NB,G,2,PLANE,8] halves)."""
    G, PL = SHB.groups(channels), SHB.plane(H, W)
    halves = buf.cpu().numpy().view(np.float16).reshape(-1, G, 2, PL, 8)
    return torch.from_numpy(SHB.unpack_interior(halves, exp.numpy(), channels, H, W)), halves
