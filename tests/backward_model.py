"""Plain float64 references of the nine backward entry points of libos2d_train.so (include/os2d_train.h), one per entry point.

Each model restates the FORWARD stage in float64 with stock torch operators on the CPU (the oracle's own functions where it has
one) and lets ``torch.autograd.grad`` differentiate it: no gradient formula of the kernels is written down here.  The models
take and return the tensors in the layouts of the C ABI (zero-bordered planes, x-major class operand), so that chaining them in
the order of ``_HeadFunction.backward`` (tests/test_backward_model.py) also checks the layout helpers and the channel orders.

Inputs are the float32 values the kernels read, converted to float64; everything downstream is float64.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import head_oracle as O

T = O.TEMPLATE
K = T * T
F64 = torch.float64
SENTINEL = 1e30                      # plane 225 of layer 1's input: nothing may read it
EPS32 = float(np.float32(1e-5))      # the BatchNorm epsilon as the C ABI receives it (a float)
U32 = 2.0 ** -24                     # unit round-off of fp32


# ---------------------------------------------------------------------------------------------------------- plane layout
def round_up(x, m):
    return (x + m - 1) // m * m


def plane_geometry(H, W):
    """(ws, base, PLANE) of the zero-bordered plane layout: cell (h, w) at base + h*ws + w."""
    ws = W + 3
    base = round_up(3 * ws + 3, 4)
    return ws, base, round_up(base + (H + 3) * ws + 3, 64)


def plane_index(H, W):
    """Flat plane offsets of the H*W data cells, row-major."""
    ws, base, _ = plane_geometry(H, W)
    return (base + torch.arange(H).view(H, 1) * ws + torch.arange(W).view(1, W)).reshape(-1)


def interior_mask(H, W):
    m = torch.zeros(plane_geometry(H, W)[2], dtype=torch.bool)
    m[plane_index(H, W)] = True
    return m


def pack_planes(x):
    """[N,C,H,W] -> [N,C,PLANE], zeros at the pad cells."""
    N, C, H, W = x.shape
    out = torch.zeros(N, C, plane_geometry(H, W)[2], dtype=x.dtype)
    out[:, :, plane_index(H, W)] = x.reshape(N, C, H * W)
    return out


def unpack_planes(p, H, W):
    """[N,C,PLANE] -> [N,C,H,W] (the data cells)."""
    return p[:, :, plane_index(H, W)].reshape(p.size(0), p.size(1), H, W)


def pack_layer1_input(x):
    """[NB,225,H,W] -> [NB,226,PLANE] as the forward leaves rnorm: 225 planes and a 226th nothing reads (SENTINEL)."""
    p = pack_planes(x)
    return torch.cat([p, torch.full_like(p[:, :1], SENTINEL)], dim=1)


def class_operand(q_hat):
    """Normalised class maps [B,C,15,15] -> qp [B,C,256] of os2d_class_prepare_batch: x-major (m = x*15 + y), rows 225..255 zero."""
    B, C = q_hat.shape[:2]
    qp = torch.zeros(B, C, 256, dtype=q_hat.dtype)
    qp[:, :, :K] = q_hat.permute(0, 1, 3, 2).reshape(B, C, K)
    return qp


def from_xmajor(dq):
    """[B,C,225] x-major -> [B,C,15,15] (row y, column x)."""
    return dq.reshape(dq.size(0), dq.size(1), T, T).permute(0, 1, 3, 2)


def to_xmajor(g):
    return g.permute(0, 1, 3, 2).reshape(g.size(0), g.size(1), K)


def _leaf(t):
    return t.detach().to(F64).clone().requires_grad_(True)


def _grad(out, leaves, upstream):
    gs = torch.autograd.grad(out, leaves, upstream.to(F64), allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves)]


# ---------------------------------------------------------------------------------------------------------- decode backward
def template_coords(fp32=True):
    """The 15 template coordinates.  fp32=True: torch.linspace(-1, 1, 15) in float32 (the constants the kernels use: the
    middle element is -4.47e-8, not 0) as float64 values; fp32=False: the float64 linspace of F.affine_grid."""
    return torch.linspace(-1, 1, T, dtype=torch.float32).to(F64) if fp32 else torch.linspace(-1, 1, T, dtype=F64)


def pool_mask64():
    m = O.pool_mask().to(F64)
    return (m > 0).to(F64) / float((m > 0).sum())


def theta_regularised(params, inverse):
    """oracle.params_to_theta, with the inverse taken of the matrix regularised as os2d_theta (csrc/sample_decode.h) does it:
    where the 2x2 determinant is exactly 0, 1e-5 is added (in fp32) to the three diagonal elements of the homogeneous matrix."""
    theta = O.params_to_theta(params, False)
    if not inverse:
        return theta
    n = theta.size(0)
    last = torch.zeros(n, 1, 3, dtype=theta.dtype)
    last[:, :, 2] = 1
    M = torch.cat([theta, last], dim=1)
    th = theta.detach()
    singular = (th[:, 0, 0] * th[:, 1, 1] - th[:, 0, 1] * th[:, 1, 0]) == 0
    if singular.any():
        t32 = th.float()
        reg = torch.zeros(n, 3, 3, dtype=theta.dtype)
        reg[:, 0, 0] = (t32[:, 0, 0] + 1e-5).to(F64) - th[:, 0, 0]
        reg[:, 1, 1] = (t32[:, 1, 1] + 1e-5).to(F64) - th[:, 1, 1]
        reg[:, 2, 2] = float(np.float32(1) + np.float32(1e-5)) - 1.0
        M = M + reg * singular.view(-1, 1, 1).to(theta.dtype)
    return torch.inverse(M)[:, :2, :]


def decode_forward(corr, params, inverse, stride, rec_field, coords=None, mask=None):
    """(loc [NB,4,H,W], cls [NB,1,H,W], aux) from corr [NB,225,H,W] and params [NB,P,H,W]: the oracle's stages after the
    TransformNet (head_oracle.head_forward), with the base grid of F.affine_grid written out so that its 15 coordinates can be
    the kernels' fp32 constants."""
    NB, _, H, W = corr.shape
    coords = template_coords(True) if coords is None else coords
    mask = pool_mask64() if mask is None else mask
    theta = theta_regularised(params, inverse)
    one = torch.ones(T, T, dtype=F64)
    base = torch.stack([coords.view(1, T) * one, coords.view(T, 1) * one, one], dim=-1)     # [row i, col j] -> (x_j, y_i, 1)
    grids = torch.einsum("ijk,nck->nijc", base, theta).view(NB, 1, H, W, T, T, 2)           # = F.affine_grid(theta, ..)
    g_fm = O.local_to_global(grids, O.anchor_grid(H, W, float(T), 1.0).to(F64).view(1, 1, H, W, 4))
    g_unit = torch.stack([g_fm[..., 0] / (W - 1) * 2 - 1, g_fm[..., 1] / (H - 1) * 2 - 1], dim=-1).clamp(-1, 1)
    cls = O.resample_and_pool(corr.view(NB, 1, K, H, W), g_unit, mask).view(NB, 1, H, W)
    anchors = O.anchor_grid(H, W, float(stride * (T - 1) + rec_field), float(stride)).to(F64)
    g_img = O.local_to_global(grids, anchors.view(1, 1, H, W, 4))
    gx, gy = g_img[..., 0].reshape(-1, K), g_img[..., 1].reshape(-1, K)
    boxes = torch.stack([gx.min(1)[0], gy.min(1)[0], gx.max(1)[0], gy.max(1)[0]], dim=1)
    loc = O.encode_boxes(O.clip_to_min_size(boxes), O.clip_to_min_size(anchors.repeat(NB, 1)))
    loc = loc.view(NB, H, W, 4).permute(0, 3, 1, 2)
    return loc, cls, dict(theta=theta, g_fm=g_fm, g_img=g_img)


def fragility(aux, P, H, W, stride, rec_field):
    """[NB,HW]: the smallest distance of a location to a point where the gradient of the decode stage jumps, in units of the
    rounding error delta the kernel's fp32 chain can have there.  A location is FRAGILE when the value is below 1.

    The jumps: a pooled sample coordinate crossing a cell edge of the bilinear interpolation (an integer in [0, W-1] or
    [0, H-1]; the two clamp bounds are such integers), the arg-min or arg-max over the corners changing hands (the gap between
    the two smallest / two largest corner U's and V's) and clip_to_min_size switching (|x2 - x1 - 1|, |y2 - y1 - 1|).

    delta: the kernel rounds theta to fp32, evaluates g = t00*xj + t01*yi + t02 (two multiplications, two additions), then
    X = g*7.5 + cx (a multiplication, an addition): with the rounding of theta's three elements about 8 roundings, each at most
    2^-24 of the magnitude it works at, which |t00 xj| + |t01 yi| + |t02| (times 7.5, plus cx) bounds.  With a factor 2 for the
    float64 model's own path through normalised coordinates and for the products of such terms:
        delta = 16 * 2^-24 * (7.5 * (|t00 xj| + |t01 yi| + |t02|) + cx)
    per sample coordinate, and the same with half_box for 7.5, the image-level centre ecx for cx and xj, yi = +-1 for the corners.
    """
    theta = aux["theta"].detach()
    N = theta.size(0)
    NB = N // (H * W)
    xs = template_coords(True)[O.POOL_BORDER:T - O.POOL_BORDER]
    g_fm = aux["g_fm"].detach().reshape(N, T, T, 2)[:, O.POOL_BORDER:T - O.POOL_BORDER, O.POOL_BORDER:T - O.POOL_BORDER]
    hh = torch.arange(H, dtype=F64).view(H, 1).expand(H, W).reshape(-1).repeat(NB)
    ww = torch.arange(W, dtype=F64).view(1, W).expand(H, W).reshape(-1).repeat(NB)
    ratio = torch.full((N,), float("inf"), dtype=F64)
    half_box = 0.5 * (stride * (T - 1) + rec_field)
    g_img = aux["g_img"].detach().reshape(N, T, T, 2)
    for axis, size, centre in ((0, W, ww + 0.5), (1, H, hh + 0.5)):
        t0, t1, t2 = theta[:, axis, 0].abs(), theta[:, axis, 1].abs(), theta[:, axis, 2].abs()
        X = g_fm[..., axis]                                                                 # [N, i, j]
        dist = (X - X.round().clamp(0, size - 1)).abs()
        mag = t0.view(N, 1, 1) * xs.abs().view(1, 1, -1) + t1.view(N, 1, 1) * xs.abs().view(1, -1, 1) + t2.view(N, 1, 1)
        delta = 16 * U32 * (0.5 * T * mag + centre.view(N, 1, 1))
        ratio = torch.minimum(ratio, (dist / delta).reshape(N, -1).min(1)[0])
        U = g_img[:, [0, 0, T - 1, T - 1], [0, T - 1, 0, T - 1], axis].sort(dim=1)[0]       # the four corners
        delta_c = 16 * U32 * (half_box * (t0 + t1 + t2) + stride * centre)
        # P = 4: t01 = t10 = 0, the corners coincide in pairs by construction and either of a pair gives the same gradient
        gaps = [U[:, 2] - U[:, 1]] if P == 4 else [U[:, 1] - U[:, 0], U[:, 3] - U[:, 2]]
        gaps.append((U[:, 3] - U[:, 0] - 1).abs())
        for gap in gaps:
            ratio = torch.minimum(ratio, gap / delta_c)
    return ratio.view(NB, H * W)


def decode_backward_model(corr, params, dcls, dcls_det, dloc, inverse, stride, rec_field, fp32_coords=True, mask=None):
    """os2d_train_decode_backward: corr [NB,225,H,W], params [NB,P,H,W]; upstream dcls / dcls_det [NB,H,W], dloc [NB,4,H,W]
    (None = zero).  Returns (the amount ADDED to dcorr [NB,225,HW], dparams [NB,P,HW], fragility [NB,HW]).  cls_det is the
    same resampling on a grid built from DETACHED parameters (reference head.py:396-402)."""
    NB, _, H, W = corr.shape
    P = params.size(1)
    c, p = _leaf(corr), _leaf(params)
    coords = template_coords(fp32_coords)
    loc, cls, aux = decode_forward(c, p, inverse, stride, rec_field, coords, mask)
    _, cls_det, _ = decode_forward(c, p.detach(), inverse, stride, rec_field, coords, mask)
    loss = (loc * 0).sum()
    if dloc is not None:
        loss = loss + (loc * dloc.to(F64).view(NB, 4, H, W)).sum()
    if dcls is not None:
        loss = loss + (cls * dcls.to(F64).view(NB, 1, H, W)).sum()
    if dcls_det is not None:
        loss = loss + (cls_det * dcls_det.to(F64).view(NB, 1, H, W)).sum()
    dc, dp = _grad(loss, [c, p], torch.ones((), dtype=F64))
    return dc.reshape(NB, K, H * W), dp.reshape(NB, P, H * W), fragility(aux, P, H, W, stride, rec_field)


# ---------------------------------------------------------------------------------------------------------- TransformNet
LAYERS = {1: (128, K, 7), 2: (64, 128, 5)}


def layer_shape(layer, P):
    """(Cout, Cin, k) of TransformNet layer 1, 2 or 3."""
    return LAYERS[layer] if layer in LAYERS else (P, 64, 5)


def params_backward_model(dparams, H, W):
    """os2d_train_params_backward: dparams [NB,P,HW] -> (dy [NB,P,PLANE], dbias [P]); forward: params = y + bias."""
    NB, P, _ = dparams.shape
    y, b = _leaf(torch.zeros(NB, P, H, W)), _leaf(torch.zeros(P))
    dy, db = _grad(y + b.view(1, P, 1, 1), [y, b], dparams.reshape(NB, P, H, W))
    return pack_planes(dy), db


def conv_backward_model(x_planes, w, dy_planes, H, W):
    """os2d_train_conv_backward_data / _weight: the layer's input [NB,>=Cin,PLANE] (only the first Cin planes are read), raw
    weights [Cout,Cin,k,k], dy [NB,Cout,PLANE] -> (dx [NB,Cin,PLANE], dw).  Forward: F.conv2d with zero padding k // 2."""
    cin, k = w.size(1), w.size(2)
    x, wl = _leaf(unpack_planes(x_planes[:, :cin], H, W)), _leaf(w)
    dx, dw = _grad(F.conv2d(x, wl, padding=k // 2), [x, wl], unpack_planes(dy_planes, H, W))
    return pack_planes(dx), dw


def bn_relu_forward(z, gamma, beta, mean, var, eps=EPS32):
    """h = relu(BatchNorm_eval(z)), z [NB,C,H,W] = the convolution's output (bias included)."""
    return F.relu(F.batch_norm(z, mean, var, gamma, beta, training=False, eps=eps))


def bn_relu_backward_model(dh_planes, z, gamma, beta, mean, var, H, W, eps=EPS32):
    """os2d_train_bn_relu_backward: dh [NB,C,PLANE], z the pre-BatchNorm activation [NB,C,H,W] (the kernel sees only
    h = bn_relu_forward(z, ..)) -> (dy [NB,C,PLANE], dgamma, dbeta, dbias [C]); dbias = gradient of the convolution's bias."""
    C = z.size(1)
    zl, g, b, cb = _leaf(z), _leaf(gamma), _leaf(beta), _leaf(torch.zeros(C))
    h = bn_relu_forward(zl + cb.view(1, C, 1, 1), g, b, mean.to(F64), var.to(F64), eps)
    dz, dg, db, dcb = _grad(h, [zl, g, b, cb], unpack_planes(dh_planes, H, W))
    return pack_planes(dz), dg, db, dcb


def norm225_backward_model(corr, dxn_planes):
    """os2d_train_norm225_backward: corr [NB,225,H,W], dxn [NB,225,PLANE] -> the amount ADDED to dcorr [NB,225,HW]."""
    NB, _, H, W = corr.shape
    c = _leaf(corr)
    (dc,) = _grad(O.l2_normalize_channels(F.relu(c), 1e-6), [c], unpack_planes(dxn_planes, H, W))
    return dc.reshape(NB, K, H * W)


# ---------------------------------------------------------------------------------------------------------- correlation, class maps
def corr_backward_model(fm, qp, dcorr):
    """os2d_train_corr_backward: fm [A,C,H,W], qp [B,C,256], dcorr [A*B,225,HW] -> (dfm [A,C,H,W], dq [B,C,225] x-major)."""
    A, C, H, W = fm.shape
    B = qp.size(0)
    f, q = _leaf(fm), _leaf(from_xmajor(qp[:, :, :K]))
    dfm, dq = _grad(O.correlation(q, f), [f, q], dcorr.reshape(A * B, K, H, W))
    return dfm, to_xmajor(dq)


def class_backward_model(raws, dq):
    """os2d_train_class_backward: raw class maps [1,C,h_b,w_b], dq [B,C,225] x-major -> gradients of the raw maps."""
    leaves = [_leaf(r) for r in raws]
    return _grad(O.prepare_class_maps(leaves), leaves, from_xmajor(dq))


def rel_err(got, ref):
    """|got - ref|_max / |ref|_max."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------- decode backward inputs
# name: (P, inverse, stride, rec_field, NB, H, W, seed).  Every map with both P, the inverse on and off and both anchor geometries.
DECODE_CASES = {}
for _tag, _nb, _h, _w in (("2x2", 3, 2, 2), ("9x13", 3, 9, 13), ("17x19", 3, 17, 19), ("38x38", 2, 38, 38)):
    for _k, (_p, _inv, _s, _rf) in enumerate(((6, True, 16, 16), (6, False, 8, 32), (4, True, 8, 32), (4, False, 16, 16))):
        DECODE_CASES["{}_p{}_{}_s{}".format(_tag, _p, "inv" if _inv else "fwd", _s)] = (_p, _inv, _s, _rf, _nb, _h, _w, 100 + _k)


def decode_inputs(name):
    """Float32 inputs of a DECODE_CASES entry: corr, params (an identity-like map plus 0.3 randn: samples land inside, on the edge
    and outside the map), the three upstream gradients and the pattern dcorr is pre-filled with."""
    P, inverse, stride, rec_field, NB, H, W, seed = DECODE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    ident = torch.tensor([1.0, 0, 0, 0, 1, 0] if P == 6 else [1.0, 0, 1, 0]).view(1, P, 1, 1)
    return dict(corr=0.3 * torch.randn(NB, K, H, W, generator=g), params=ident + 0.3 * torch.randn(NB, P, H, W, generator=g),
                dcls=torch.randn(NB, H, W, generator=g), dcls_det=torch.randn(NB, H, W, generator=g),
                dloc=torch.randn(NB, 4, H, W, generator=g), prefill=0.01 * torch.randn(NB, K, H * W, generator=g))


# Hand-placed locations of one 3x3 map (P = 6), as the 2x3 matrix theta the sampling uses; None = the parameters are given
# directly (singular matrices).  Margins to every jump are far above delta (see fragility), except the exact ties of the
# all-zero matrix, where kernel and reference both take the first corner.
HAND_THETA = [
    None,                                                   # all-zero parameters: exactly singular
    None,                                                   # a = b = c = d = 1: exactly singular, translated
    [[1e-3, 2e-4, 0.01], [-3e-4, 1e-3, -0.02]],             # both clips of clip_to_min_size active
    [[1e-3, 2e-4, 0.01], [0.1, 0.9, 0.05]],                 # only the x clip active
    [[1.0, 0.1, 5.0], [-0.1, 1.0, -5.0]],                   # all 121 points clamped: the dcls part of dparams is 0
    [[0.9, 0.12, 0.031], [-0.07, 1.1, -0.043]],
    [[1.2, -0.21, -0.11], [0.17, 0.8, 0.093]],
    [[0.7, 0.05, 0.21], [0.03, 0.75, -0.17]],
    [[1.05, 0.3, -0.07], [-0.25, 0.95, 0.13]],
]
HAND_SINGULAR = {0: [0.0] * 6, 1: [1.0, 1.0, 3.0, 1.0, 1.0, 0.0]}


def hand_inputs(inverse):
    """Inputs of the hand-placed 3x3 map (NB = 1, P = 6).  With the inverse on, the parameters are the inverse of HAND_THETA."""
    g = torch.Generator().manual_seed(77)
    params = torch.zeros(1, 6, 9)
    for n, th in enumerate(HAND_THETA):
        if th is None:
            params[0, :, n] = torch.tensor(HAND_SINGULAR[n])
            continue
        m = torch.tensor(th + [[0.0, 0.0, 1.0]], dtype=F64)
        params[0, :, n] = (torch.inverse(m) if inverse else m)[:2].reshape(6).float()
    return dict(corr=0.3 * torch.randn(1, K, 3, 3, generator=g), params=params.view(1, 6, 3, 3),
                dcls=torch.randn(1, 3, 3, generator=g), dcls_det=torch.randn(1, 3, 3, generator=g),
                dloc=torch.randn(1, 4, 3, 3, generator=g), prefill=0.01 * torch.randn(1, K, 9, generator=g))
