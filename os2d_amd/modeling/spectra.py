"""Transform plans and weight spectra of the frequency-domain layers, on the host: the only Python wrapper of the library's
planners, the only twiddle table, the two operand builders, and the caches the operands live in.  ``TransformationNet.spectra`` /
``spectra2`` (head.py) are a few lines around these; a new weight layout or cached operand is added here."""
import collections
import ctypes
import functools
import itertools
import os

import torch

from .. import _lib
from .._native import STREAM


@functools.lru_cache(maxsize=None)
def transform_sizes(H, W, split):
    """Transform plan of an H x W map, (P, Q, nbins, tiles), or None when the library has none: os2d_dft_sizes for ``split``
    (precision "fftx3"; tiles = TY, TX, TH, TW, window rows, window columns), else os2d_fft_sizes + os2d_fft_tiles ("fft" /
    "fft32"; tiles = TY, TX, TH, TW).  Memoised: a pure function of the map size, which the library caches the same way."""
    lib = _lib.load()
    out = [ctypes.c_int() for _ in range(7)]
    ref = [ctypes.byref(x) for x in out]
    if split:
        tiles = (ctypes.c_int * 6)()
        rc = lib.os2d_dft_sizes(H, W, *ref[:3], tiles)
    else:
        rc = lib.os2d_fft_sizes(H, W, *ref[:3]) or lib.os2d_fft_tiles(H, W, *ref[3:])
        tiles = [x.value for x in out[3:]]
    return tuple(x.value for x in out[:3]) + (tuple(tiles),) if rc == 0 else None


def twiddles64(n, device):
    """exp(-2 pi i m / n) as a float64 [n, 2] table.  The fp32 tables of the in-LDS FFTs are its ``.float()``: for every size their
    planner returns (2^a 3^b, 42, 84) that equals the rounding of -2 pi m / n, their first form (tests/test_host_logic.py)."""
    m = torch.arange(n, dtype=torch.float64)
    ang = m * (-2.0 * torch.pi / n)
    return torch.stack([torch.cos(ang), torch.sin(ang)], 1).to(device).contiguous()


def build_dft_matrices(P, Q, device):
    """The four operand matrices of the P x Q matrix-product transforms (os2d_dft_matrices_build), on the current stream."""
    lib = _lib.load()
    tp64, tq64 = twiddles64(P, device), twiddles64(Q, device)
    mats = torch.empty(lib.os2d_dft_matrices_bytes(P, Q), dtype=torch.uint8, device=device)
    _lib.call("os2d_dft_matrices_build", tp64, tq64, P, Q, mats, STREAM)
    cur = torch.cuda.current_stream(device)
    tp64.record_stream(cur), tq64.record_stream(cur)
    return mats


def build_weight_spectra(wfold, C, Cout, P, Q, nbins, split, device):
    """Spectra of the float64 filters ``wfold`` [Cout, C, 7, 7] centred on the origin of the P x Q grid (tap (t, s) at ((3 - t) mod
    P, (3 - s) mod Q): the circular convolution then IS the zero-padded correlation of head.py:619 for the first H x W samples), one
    7-term float64 DFT per axis on the device (spectra_pack.hip): complex64 (os2d_spectral_gemm) or ``split`` fp16 hi + lo."""
    lib = _lib.load()
    wfold = wfold.to(device).contiguous()
    tp64, tq64 = twiddles64(P, device), twiddles64(Q, device)
    scratch = torch.empty(1024, dtype=torch.uint8, device=device)
    args = (wfold, tp64, tq64, C, Cout, P, Q, nbins)
    if split:
        wspec = torch.empty(lib.os2d_spectral_weight16_bytes(C, nbins), dtype=torch.uint8, device=device)
        _lib.call("os2d_spectral_weights_build_dft", *args, wspec, scratch, STREAM)
    else:
        wspec = torch.empty(lib.os2d_spectral_weight_bytes(C, Cout, nbins) // 4, dtype=torch.float32, device=device)
        _lib.call("os2d_spectral_weights_build", *args, 0, wspec, scratch, STREAM)
    cur = torch.cuda.current_stream(device)
    for t in (wfold, tp64, tq64, scratch):
        t.record_stream(cur)
    return wspec


class _StreamOrdered(object):
    """A cached device operand together with the event that marks the end of the kernels that produced it.  Consumers on
    OTHER streams (the per-level streams of the pyramid runner) wait for that event before their kernels read the
    buffers; on the producing stream plain stream order is enough."""

    def __init__(self, key, value, device):
        self.key, self.value = key, value
        stream = torch.cuda.current_stream(device)
        self._stream = stream.cuda_stream
        self._event = torch.cuda.Event()
        self._event.record(stream)

    def get(self, device):
        stream = torch.cuda.current_stream(device)
        if stream.cuda_stream != self._stream:
            stream.wait_event(self._event)
            for t in self._tensors():     # the cache may drop the operand while this stream's kernels still read it
                t.record_stream(stream)
        return self.value

    def _tensors(self):
        values = self.value if isinstance(self.value, (tuple, list)) else (self.value,)
        return [t for t in values if isinstance(t, torch.Tensor)]

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._tensors())


def spectra_cache_cap_bytes(split=True):
    """Upper bound for the cached weight spectra of one arithmetic FAMILY of the frequency-domain modes on ONE DEVICE - over all
    transform sizes and all TransformationNets of the process (least recently used entries are dropped first; 654 MB for the
    64 x 84 transform of a 60 x 80 map).  $OS2D_FFT_CACHE_BYTES overrides both families.
      split = True  ("fftx3", the default precision): every map is planned on six canonical transform sizes (overlap-save tiles;
                    os2d_amd/csrc/dft_mfma.h): 2.4 GB in total, whatever the dataset - an eighth of the device's memory, at
                    most 8 GiB;
      split = False ("fft" / "fft32"): one set of spectra per FFT-friendly transform size - 52 sizes = 35.6 GB for a dataset fed
                    at its own aspect ratios and 7 pyramid scales (reference os2d/data/dataloader.py:326;
                    tools/bench_size_churn.py) - a quarter of the device's memory, at most 64 GiB (under the 8 GiB
                    cap of round 4 an LRU cache missed on EVERY call of such a cyclic access pattern)."""
    env = os.environ.get("OS2D_FFT_CACHE_BYTES")
    if env:
        return int(env)
    total = 64 << 30
    if torch.cuda.is_available():
        total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory
    return int(min(8 << 30, total // 8)) if split else int(min(64 << 30, total // 4))


class _SpectraStore(object):
    """The cached weight spectra of one device, shared by every TransformationNet of the process (a per-net cap let N
    nets pin N times the cap, invisibly to the caching allocator's out-of-memory retry).  Entries are keyed by (net id, slot),
    least recently used first; a net that goes away takes its entries with it."""
    _stores = {}

    @classmethod
    def of(cls, device):
        index = device.index if device.index is not None else torch.cuda.current_device()
        store = cls._stores.get(index)
        if store is None:
            store = cls._stores[index] = cls()
        return store

    def __init__(self):
        self.entries = collections.OrderedDict()

    def get(self, net_id, slot, key):
        entry = self.entries.get((net_id, slot))
        if entry is None or entry.key != key:
            return None
        self.entries.move_to_end((net_id, slot))
        return entry

    def drop_stale(self, net_id, key):
        for k in [k for k, e in self.entries.items() if k[0] == net_id and e.key != key]:
            del self.entries[k]

    def drop_net(self, net_id):
        for k in [k for k in self.entries if k[0] == net_id]:
            del self.entries[k]

    def put(self, net_id, slot, entry):
        family = bool(slot[2])                                 # slot = (P, Q, split): the two families have caps of their own
        cap, used = spectra_cache_cap_bytes(family), entry.nbytes()
        for k in list(self.entries):                          # oldest first, whichever net it belongs to
            if used + sum(e.nbytes() for kk, e in self.entries.items() if bool(kk[1][2]) == family) <= cap:
                break
            if bool(k[1][2]) == family:
                del self.entries[k]
        self.entries[(net_id, slot)] = entry

    def slots_of(self, net_id):
        return [k[1] for k in self.entries if k[0] == net_id]

    def nbytes(self):
        return sum(e.nbytes() for e in self.entries.values())


def split_rows_f16(T):
    """(float64 MODEL of what spectra_pack.hip does on the device; used by tests/test_range_plan.py.)
    fp16 hi + lo split of a float64 tensor whose leading dimension indexes rows that get their own power-of-two scale
    (precision "fftx3": the weight spectra; one row per output channel): row r is multiplied by 2^wexp[r], the largest
    power of two that keeps its largest |entry| <= 32768 (< 65504: no overflow, also not through rounding), then
    hi = rn16(v), lo = rn16(v - hi): hi + lo carries 22 bits of v wherever |v| >= 2^-3 and an absolute 2^-25 below (fp16
    subnormal spacing).  Returns (hi, lo, wexp); works in place on T (which holds the residual afterwards)."""
    dims = tuple(range(1, T.dim()))
    amax = T.abs().amax(dim=dims).clamp_min(1e-300)
    wexp = torch.floor(torch.log2(32768.0 / amax)).clamp(-100, 100)
    T *= torch.exp2(wexp).view(-1, *([1] * (T.dim() - 1)))
    hi = T.to(torch.float16)
    T -= hi.double()
    lo = T.to(torch.float16)
    return hi, lo, wexp



_NET_IDS = itertools.count(1)


class _SpectraView(object):
    """dict-like access to ONE net's entries of a device store (tests / tools: len, in, clear, values)."""

    def __init__(self, store, net_id):
        self.store, self.net_id = store, net_id

    def __len__(self):
        return len(self.store.slots_of(self.net_id))

    def __contains__(self, slot):
        return (self.net_id, slot) in self.store.entries

    def __iter__(self):
        return iter(self.store.slots_of(self.net_id))

    def values(self):
        return [e for k, e in self.store.entries.items() if k[0] == self.net_id]

    def clear(self):
        self.store.drop_net(self.net_id)


def _drop_spectra_of(net_id):
    for store in _SpectraStore._stores.values():
        store.drop_net(net_id)

