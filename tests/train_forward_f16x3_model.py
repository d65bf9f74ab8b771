"""numpy model of the split-half blocked ("SHB") activation layout of the f16x3 kernels and of os2d_train_planes_from_shb
(include/os2d_train.h), written from the layout text of include/os2d_hip.h and os2d_amd/csrc/os2d_common.h - test infrastructure,
no GPU needed.

Plane geometry (os2d_common.h): a map H x W is stored as rows of WS = W + 3 cells, cell (h, w) at BASE + h * WS + w with
BASE = round_up(3 * WS + 3, 4); PLANE = round_up(BASE + (H + 3) * WS + 3, 64) cells per channel; every cell that is not a
data cell is a pad cell.
SHB: [NB][G = ceil(channels / 8)][hi | lo][PLANE] units of 8 halves (16 bytes): unit (nb, g, part, n) holds channels 8g .. 8g+7
of plane cell n, channel c as x * 2^exp[c] split into hi = rn16(x 2^exp), lo = rn16(x 2^exp - hi)."""
import numpy as np

PAD = 3


def round_up(x, m):
    return (x + m - 1) // m * m


def ws(W):                      # os2d_ws
    return W + PAD


def base(W):                    # os2d_base
    return round_up(PAD * ws(W) + PAD, 4)


def plane(H, W):                # os2d_plane = os2d_plane_floats
    return round_up(base(W) + (H + PAD) * ws(W) + PAD, 64)


def interior(n, H, W):          # os2d_interior, operation for operation
    r = n - base(W)
    return r >= 0 and r < H * ws(W) and (r % ws(W)) < W


def plane_index(H, W):
    """Flat plane offsets of the H x W data cells, row-major: cell(h, w) = BASE + h * WS + w."""
    return (base(W) + np.arange(H)[:, None] * ws(W) + np.arange(W)[None, :]).reshape(-1)


def interior_mask(H, W):
    m = np.zeros(plane(H, W), dtype=bool)
    m[plane_index(H, W)] = True
    return m


def groups(channels):
    return (channels + 7) // 8


def split(v):
    """fp32 -> (hi, lo) fp16: hi = rn16(v), lo = rn16(v - hi) (the subtraction in fp32, where it is exact)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def pack(x, exp):
    """x [NB, channels, H, W] fp32, exp [channels] int -> SHB as float16 [NB, G, 2, PLANE, 8]; pad cells and the unused channels
    of the last group are zero."""
    x = np.asarray(x, dtype=np.float32)
    NB, C, H, W = x.shape
    hi, lo = split(np.ldexp(x, np.asarray(exp, dtype=np.int32).reshape(1, C, 1, 1)).astype(np.float32))
    out = np.zeros((NB, groups(C), 2, plane(H, W), 8), dtype=np.float16)
    idx = plane_index(H, W)
    for c in range(C):
        out[:, c // 8, 0, idx, c % 8] = hi[:, c].reshape(NB, H * W)
        out[:, c // 8, 1, idx, c % 8] = lo[:, c].reshape(NB, H * W)
    return out


def unpack(shb, exp, channels, out_channels, H, W, dtype=np.float32):
    """os2d_train_planes_from_shb: SHB float16 [NB, G, 2, PLANE, 8] -> planes [NB, out_channels, PLANE] of ``dtype``:
    (hi + lo) * 2^-exp[c] at data cells - the sum and the scaling in ``dtype`` (float32: the kernel's own arithmetic; float64:
    exact for every pair of halves) - and +0 at pad cells, whatever shb holds there, and in planes channels .. out_channels-1."""
    NB, G, _, PL, _ = shb.shape
    assert G == groups(channels) and PL == plane(H, W) and out_channels >= channels
    out = np.zeros((NB, out_channels, PL), dtype=dtype)
    idx = plane_index(H, W)
    exp = np.asarray(exp, dtype=np.int32)
    for c in range(channels):
        hi = shb[:, c // 8, 0, idx, c % 8].astype(dtype)
        lo = shb[:, c // 8, 1, idx, c % 8].astype(dtype)
        out[:, c, idx] = np.ldexp(hi + lo, -exp[c]).astype(dtype)
    return out


def unpack_interior(shb, exp, channels, H, W, dtype=np.float64):
    """The data cells of ``unpack`` as [NB, channels, H, W]."""
    p = unpack(shb, exp, channels, channels, H, W, dtype)
    return p[:, :, plane_index(H, W)].reshape(p.shape[0], channels, H, W)
