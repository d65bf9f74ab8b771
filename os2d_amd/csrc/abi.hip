// C ABI of libos2d_hip.so (include/os2d_hip.h): argument checking, workspace carving, stage sequencing.
#include <stdio.h>

#include "../../include/os2d_hip.h"
#include "os2d_common.h"
#include "detect_common.h"
#include <atomic>
#include <mutex>
#include <random>
#include <vector>

namespace {
struct ConvShape {
  int cout, cin, ks, mt;
};
bool conv_shape(int layer, int P, ConvShape* s) {
  switch (layer) {
    case 1: *s = {128, OS2D_K, 7, 128}; return true;
    case 2: *s = {64, 128, 5, 64}; return true;
    case 3: *s = {P, 64, 5, 32}; return true;
    default: return false;
  }
}
size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// k-steps of one channel group of the packed 7x7 weights (49 taps in pairs), = 5 LDS stages of 5 in conv_f16x3.hip
int os2d_conv1_steps_padded() { return 25; }

// ---- the head call.  What does not depend on the class chunk is decided once (head_route) and kept in a HeadRoute: the size
// entry points and os2d_head_forward_ex2 carve the workspace from the same record, the stage functions branch on its fields.
enum Transform7 { T7_NONE, T7_FFT, T7_DFT };  // 7x7 layer: direct kernels | in-LDS FFTs (fft.hip) | transforms as matrix products (dft_mfma.hip)
struct HeadRoute {
  int precision;
  bool f16;                 // split-fp16 operands: qs is required and the range words are live (false: fp32 MFMA correlation / 5x5 layers)
  Transform7 transform;
  bool conv2_freq;          // the 5x5 layer 128 -> 64 in the frequency domain as well (T7_DFT with the layer's weight spectra)
  bool borders_in_inverse;  // T7_DFT: the layer-1 inverse transform writes the zero borders of the planes it fills
  bool fused_tail_allowed;  // the last layer and the alignment epilogue in ONE launch (conv3_f16x3.hip, FUSE)
  int terms1;               // 7x7 layer, direct split-fp16 kernel: 3, or 2 = the weights as fp16 roundings only (f16x2)
  int layout;               // of the output spectra (include/os2d_hip.h): the split-half GEMM writes them in quads of bins
  int bins, tiles[6], T;    // transform plan: bins of a window (0: T7_NONE), TY, TX, TH, TW, window rows / columns, T = TY * TX
  int xch;                  // channel stride of the input spectra
};

// workspace carve for a chunk of Bc classes
struct Carve {
  size_t flags, sumsq, fs, corr, rpad, h1, h2, params, invn, sumfx, xspec, yspec, total;
};
Carve carve(const HeadRoute& r, int A, int Bc, int C, int H, int W, int P) {
  const size_t HW = (size_t)H * W, PL = os2d_plane(H, W), NB = (size_t)A * Bc;
  Carve c;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off = align_up(off + floats * sizeof(float), 256);
    return o;
  };
  c.flags = take((size_t)A + 1);           // range words of the call: one per image + one for the whole call (Os2dRangeFlag); FIRST
  c.sumsq = take((size_t)A * HW);
  c.fs = take((size_t)A * os2d_corr_groups(C) * 2 * HW * 4);  // f16x3: split image features, 16 B per (group, part, cell)
  c.corr = take(NB * OS2D_K * HW);
  // fp32: 226 planes; f16x3: 29 groups x (hi|lo) x 16 B = 232 floats; not needed by the frequency-domain 7x7 layer
  c.rpad = take(r.bins > 0 ? 0 : NB * (OS2D_G * 2 * 4) * PL);
  c.h1 = take(NB * 128 * PL);
  c.h2 = take(NB * 64 * PL);
  c.params = take(NB * P * HW);
  c.invn = c.sumfx = c.xspec = c.yspec = 0;
  if (r.bins > 0) {  // frequency-domain 7x7 layer: inverse norms, input / output spectra (complex64)
    c.invn = take(NB * HW);
    c.sumfx = take(NB * HW * 2);           // 64-bit fixed-point sums of the packed correlation kernel (corr_f16x3.hip, STACK)
    c.xspec = take(NB * r.T * r.xch * (size_t)r.bins * 2);     // a tile of a tiled map is one more "pair" (fft.hip)
    c.yspec = take(NB * r.T * 128 * (size_t)r.bins * 2);
  }
  c.total = off;
  return c;
}

// ---- debugging aid (tools/diag_pyramid_dump.py): copies of intermediate buffers of os2d_head_forward_ex, per stream.
// Compiled only into DIAGNOSTIC builds (python -m os2d_amd.build --variant dump, with the macro below defined): a registered destination
// is a raw pointer nobody can unregister safely once its tensor is freed, and the table would be consulted by every
// production call.  In the product library os2d_debug_set_dump only reports that it does nothing.
#ifdef OS2D_DIAG_DUMP
struct DumpEntry {
  void* stream;
  int slot;
  void* dst;
  size_t bytes;
};
std::vector<DumpEntry> g_dumps;
std::mutex g_dumps_mutex;               // ctypes releases the GIL: callers may race on the table
bool dumps_active() {
  std::lock_guard<std::mutex> lock(g_dumps_mutex);
  return !g_dumps.empty();
}
void dump_slot(void* stream, int slot, const void* src, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_dumps_mutex);
  for (const DumpEntry& e : g_dumps)
    if (e.stream == stream && e.slot == slot && e.dst)
      (void)hipMemcpyAsync(e.dst, src, bytes < e.bytes ? bytes : e.bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
}
#else
inline bool dumps_active() { return false; }
inline void dump_slot(void*, int, const void*, size_t) {}
#endif

bool head_args_ok(int A, int B, int C, int H, int W, int P) {
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1 || (P != 6 && P != 4)) {
    os2d_set_error("bad head shape A=%d B=%d C=%d H=%d W=%d P=%d (need A,B,C,H,W>=1, P in {6,4})", A, B, C, H,
                   W, P);
    return false;
  }
  if (W > OS2D_MAX_W) {
    os2d_set_error("feature map width %d > %d: beyond what the transform planner of the 7x7 layer tiles (images wider than %d px "
                   "at stride 16 are not supported)", W, OS2D_MAX_W, OS2D_MAX_W * 16);
    return false;
  }
  if (H > OS2D_MAX_H) {
    os2d_set_error("feature map height %d > %d: beyond what the transform planner of the 7x7 layer tiles (images taller than %d px "
                   "at stride 16 are not supported)", H, OS2D_MAX_H, OS2D_MAX_H * 16);
    return false;
  }
  return true;
}
// The epoch of a head call: what its kernels store into the range words of the workspace (os2d_common.h: Os2dRangeFlag).  Unique per
// call of the process, never 0 (a zero-filled workspace) and never OS2D_STATUS_F16_RANGE; the base is random so that the stale
// content of a workspace that was NOT zero-filled matches a call's epoch with probability 2^-32.
int next_epoch() {
  static std::atomic<unsigned> counter{[] {
    std::random_device rd;
    return (unsigned)rd() | 0x100u;
  }()};
  unsigned e;
  do e = counter.fetch_add(1u, std::memory_order_relaxed) + 1u;
  while (e < 2u);
  return (int)e;
}
bool is_freq(int precision) {
  return precision == OS2D_PRECISION_FFT || precision == OS2D_PRECISION_FFTX3 || precision == OS2D_PRECISION_FFT32;
}
// The measurement switches of the head call, read once per process; each is on unless its variable starts with '0':
// OS2D_CONV2_FREQ=0 the direct kernel for the 5x5 layer 128 -> 64, OS2D_BORDERS_IN_INVERSE=0 the zero borders of the layer-1 planes
// in a launch of their own, OS2D_FUSED_TAIL=0 the last layer and the resampler as two launches (same bits)
struct HeadSwitches {
  bool conv2_freq, borders_in_inverse, fused_tail;
};
bool env_on(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
const HeadSwitches& head_switches() {
  static const HeadSwitches s = {env_on("OS2D_CONV2_FREQ"), env_on("OS2D_BORDERS_IN_INVERSE"), env_on("OS2D_FUSED_TAIL")};
  return s;
}
// The route of a call in `precision` on an H x W map; 0, or the error text is set (`who`: the entry point) and -1 for an unknown
// precision or a map too wide for the direct 7x7 kernels, -3 when the transforms have no plan.  launch = false (the size entry
// points, which launch nothing): those two -1 cases get the footprint of the direct routes, as they always did.
int head_route(const char* who, int precision, int H, int W, bool have_wspec2, bool launch, HeadRoute* r) {
  *r = HeadRoute{precision, false, T7_NONE, false, false, false, 3, OS2D_SPECTRA_ROWS, 0, {1, 1, 0, 0, 0, 0}, 1, OS2D_K};
  switch (precision) {
    case OS2D_PRECISION_F32: break;
    case OS2D_PRECISION_F16X3: r->f16 = true; break;
    case OS2D_PRECISION_F16X2: r->f16 = true, r->terms1 = 2; break;
    case OS2D_PRECISION_FFT32: r->transform = T7_FFT; break;
    case OS2D_PRECISION_FFT: r->f16 = true, r->transform = T7_FFT; break;
    case OS2D_PRECISION_FFTX3: r->f16 = true, r->transform = T7_DFT, r->layout = OS2D_SPECTRA_QUADS, r->xch = OS2D_XSPEC_CPAD; break;
    default:
      if (!launch) break;
      os2d_set_error("%s: unknown precision %d", who, precision);
      return -1;
  }
  if (r->transform == T7_NONE) {
    if (launch && W > OS2D_MAX_W_DIRECT7) {
      os2d_set_error("feature map width %d > %d: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a "
                     "frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to %d", W, OS2D_MAX_W_DIRECT7, OS2D_MAX_W);
      return -1;
    }
  } else if (!(r->transform == T7_DFT ? os2d_dft_plan : os2d_fft_plan)(H, W, nullptr, nullptr, &r->bins, r->tiles)) {
    os2d_set_error("%s: no transform plan for a %dx%d map", who, H, W);
    return -3;
  }
  r->T = r->tiles[0] * r->tiles[1];
  // layer 2 on the transform route: the layer-1 inverse writes fp32 planes scaled to <= 1, a forward transform of those 128 channels,
  // the per-bin GEMM 128 -> 64 and the inverse with the layer-2 bias and scales follow
  r->conv2_freq = r->transform == T7_DFT && have_wspec2 && head_switches().conv2_freq;
  r->borders_in_inverse = r->transform == T7_DFT && head_switches().borders_in_inverse;
  r->fused_tail_allowed = r->f16 && head_switches().fused_tail && !dumps_active();     // (diagnostic dumps of the parameters need the separate launches)
  return 0;
}
int head_workspace_bytes(const char* who, int A, int B, int C, int H, int W, int P, int precision, size_t* bytes) {
  if (!bytes) {
    os2d_set_error("%s: null output", who);
    return -1;
  }
  if (!head_args_ok(A, B, C, H, W, P)) return -1;
  HeadRoute r;
  if (const int rc = head_route(who, precision, H, W, false, false, &r)) return rc;
  *bytes = carve(r, A, B, C, H, W, P).total;
  return 0;
}
// largest class chunk that fits the workspace (the footprint is affine in Bc); 0: not even one class fits
int largest_chunk(const HeadRoute& r, int A, int B, int C, int H, int W, int P, size_t workspace_bytes) {
  const size_t one = carve(r, A, 1, C, H, W, P).total;
  if (workspace_bytes < one) return 0;
  int Bc = B;
  while (Bc > 1 && carve(r, A, Bc, C, H, W, P).total > workspace_bytes) {
    const size_t per = carve(r, A, 2, C, H, W, P).total - one;
    int guess = per ? (int)((workspace_bytes - one) / per) + 1 : 1;
    if (guess >= Bc) guess = Bc - 1;
    if (guess < 1) guess = 1;
    Bc = guess;
  }
  return Bc;
}

// One os2d_head_forward_ex2 call: the caller's arguments, then what the call made of them (buffers a route does not use: NULL)
struct HeadCall {
  const float *fm, *qp, *b1, *b2, *b3, *wspec, *twQ, *twP;
  const void *w1, *w2, *w3, *qs, *wspec2;
  int A, B, C, H, W, P, inverse, stride, rec_field;
  float *loc, *cls, *corners;
  int* status;
  void** events;
  hipStream_t st;
  float *sumsq, *corr, *rpad, *h1, *h2, *params, *invn, *xspec, *yspec;
  void *fsplit, *sumfx;     // sumfx != NULL: the packed form of the half-precision correlation
  // range words (one per image, one for the whole call) and the value this call's kernels store there; the last kernel of every class
  // chunk - the resampler - turns a raised word into NaN outputs and raises the caller's sticky host word
  int* flags;
  int epoch;
  Os2dRangeFlag per_image, whole_call;
};
// optional per-stage events (first class chunk only): events[2*s] / [2*s+1] bracket stage s, [10] .. [12] lie inside stage 1
void mark(const HeadCall& x, int b0, int idx) {
  if (x.events && b0 == 0 && x.events[idx]) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(x.events[idx]), x.st);
}
// diagnostic builds: a copy of a buffer of the first class chunk; slots: 0 corr, 1 inverse norms, 2 input spectra, 3 output spectra,
// 4 h1, 5 h2, 6 params
void dump(const HeadCall& x, int b0, int slot, const void* src, size_t bytes) {
  if (b0 == 0 && dumps_active()) dump_slot(x.st, slot, src, bytes);
}

// ---- the five stages of the class chunk [b0, b0 + bc), called in this order by the chunk loop of os2d_head_forward_ex2
int stage_corr(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  int rc;
  // the frequency-domain 7x7 layer takes corr + invn; the split / blocked copy of the normalised maps is not written
  if (!r.bins && (rc = r.f16 ? os2d_launch_border_zero_shb(x.rpad, NB, x.H, x.W, x.st) : os2d_launch_border_zero(x.rpad, NB * OS2D_KP, x.H, x.W, x.st)))
    return rc;
  if (!r.f16) return os2d_launch_corr(x.fm, x.qp + (size_t)b0 * x.C * OS2D_QROWS, x.sumsq, x.corr, x.rpad, x.invn, x.A, bc, x.C, x.H, x.W, 0, x.st);
  const char* qsb = static_cast<const char*>(x.qs) + (size_t)b0 * os2d_corr_groups(x.C) * 2 * 256 * 16;
  // packed form: the sums become inverse norms in the border launch of stage_conv1 (before the forward transform reads them)
  return os2d_launch_corr_f16x3(x.fsplit, qsb, x.corr, x.rpad, x.invn, x.sumfx, 1, x.A, bc, x.C, x.H, x.W, x.st);
}
// direct fp32 | direct split-fp16 | the layer in the frequency domain (fft.hip / dft_mfma.hip, spectral*.hip): transform of
// relu(corr) / norm -> one complex GEMM per bin -> inverse transform + bias + ReLU into the activation buffer of the 5x5 layer
int stage_conv1(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc, H = x.H, W = x.W;
  int rc;
  if (r.transform == T7_NONE)
    return r.f16 ? os2d_launch_conv_f16x3(1, x.rpad, x.w1, x.b1, x.whole_call, x.h1, NB, x.P, H, W, r.terms1, x.st)
                 : os2d_launch_conv(1, x.rpad, static_cast<const float*>(x.w1), x.b1, x.h1, NB, x.P, H, W, x.st);
  if (r.f16) {
    // what is left of the border launch when the inverse transform writes the borders (or fp32 planes, which have none) is the
    // norms pass of the packed correlation (none for the padded form: no launch at all)
    const int planes = (r.borders_in_inverse || r.conv2_freq) ? 0 : NB * 16 * 2;
    if ((planes || x.sumfx) && (rc = os2d_launch_border_zero_shb_planes_norms(x.h1, planes, H, W, x.sumfx, x.invn, (size_t)NB * H * W, x.st)))
      return rc;
  } else if ((rc = os2d_launch_border_zero(x.h1, NB * 128, H, W, x.st))) {     // all-fp32 mode: fp32 planes for the fp32 5x5 kernel
    return rc;
  }
  mark(x, b0, 10);
  if (r.transform == T7_FFT) {
    if ((rc = os2d_launch_fft_forward(x.corr, x.invn, x.xspec, x.twQ, x.twP, NB, OS2D_K, H, W, x.st))) return rc;
    mark(x, b0, 11);
    if ((rc = os2d_launch_spectral_gemm(x.wspec, x.xspec, x.yspec, NB * r.T, OS2D_K, 128, r.bins, x.st))) return rc;
    mark(x, b0, 12);
    return os2d_launch_fft_inverse(x.yspec, x.b1, 128, x.h1, x.twQ, x.twP, NB, 128, H, W, x.whole_call, r.layout, r.f16 ? 0 : 1, x.st);
  }
  // the transforms as matrix products on the half-precision matrix cores (twQ = the matrices), spectra in quads of bins on both
  // sides of the per-bin GEMM; |X| <= number of samples of a window (every sample of the normalised maps is <= 1)
  if ((rc = os2d_launch_dft_forward(x.corr, x.invn, x.xspec, x.twQ, NB, OS2D_K, r.xch, H, W, x.st))) return rc;
  mark(x, b0, 11);
  if ((rc = os2d_launch_spectral_gemm_f16(x.wspec, x.xspec, x.yspec, NB * r.T, OS2D_K, 128, r.bins, os2d_spectral_xscale_for(r.tiles[4], r.tiles[5]), 1, r.xch, x.st)))
    return rc;
  mark(x, b0, 12);
  return os2d_launch_dft_inverse(x.yspec, x.b1, 128, x.h1, x.twQ, NB, 128, H, W, x.whole_call,
                                 r.conv2_freq ? OS2D_DFT_OUT_PLANES : r.borders_in_inverse ? OS2D_DFT_OUT_SHB_BORDERS : OS2D_DFT_OUT_SHB, x.st);
}
int stage_conv2(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc, H = x.H, W = x.W;
  int rc;
  dump(x, b0, 0, x.corr, (size_t)NB * OS2D_K * H * W * 4);
  if (r.bins) {
    dump(x, b0, 1, x.invn, (size_t)NB * H * W * 4);
    dump(x, b0, 2, x.xspec, (size_t)NB * r.T * OS2D_K * r.bins * 8);
    dump(x, b0, 3, x.yspec, (size_t)NB * r.T * 128 * r.bins * 8);
  }
  dump(x, b0, 4, x.h1, (size_t)NB * 128 * (r.conv2_freq ? (size_t)H * W : (size_t)os2d_plane(H, W)) * 4);  // (fp32 planes on the transform route of layer 2)
  if (!r.conv2_freq)
    return r.f16 ? os2d_launch_conv_f16x3(2, x.h1, x.w2, x.b2, x.whole_call, x.h2, NB, x.P, H, W, 3, x.st)
                 : os2d_launch_conv(2, x.h1, static_cast<const float*>(x.w2), x.b2, x.h2, NB, x.P, H, W, x.st);
  // h1: fp32 planes [pair][128][H * W], every sample in [0, 1] - unit norms, and the ReLU of the forward kernel changes nothing;
  // both spectra buffers are reused (128 channels fit the input stride, 64 the output buffer)
  if ((rc = os2d_launch_dft_forward(x.h1, nullptr, x.xspec, x.twQ, NB, 128, 128, H, W, x.st))) return rc;
  if ((rc = os2d_launch_spectral_gemm_f16(x.wspec2, x.xspec, x.yspec, NB * r.T, 128, 64, r.bins, os2d_spectral_xscale_for(r.tiles[4], r.tiles[5]), 1, 128, x.st)))
    return rc;
  return os2d_launch_dft_inverse(x.yspec, x.b2, 64, x.h2, x.twQ, NB, 64, H, W, x.whole_call, OS2D_DFT_OUT_SHB_BORDERS, x.st);
}
// fused tail: ONE launch for the last layer and the alignment epilogue (conv3_f16x3.hip, FUSE: the parameters go from the accumulators
// through LDS to the resampler, never to HBM), and stage_sample has nothing left to do
int stage_conv3(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  dump(x, b0, 5, x.h2, (size_t)NB * 64 * os2d_plane(x.H, x.W) * 4);
  if (r.fused_tail_allowed)
    return os2d_launch_conv3_sample_decode(x.h2, x.w3, x.b3, x.corr, NB, x.H, x.W, x.P, x.inverse, x.stride, x.rec_field, bc, x.B, b0, x.loc, x.cls,
                                           x.corners, x.flags, x.epoch, x.status, x.st);
  return r.f16 ? os2d_launch_conv_f16x3(3, x.h2, x.w3, x.b3, x.whole_call, x.params, NB, x.P, x.H, x.W, 3, x.st)
               : os2d_launch_conv(3, x.h2, static_cast<const float*>(x.w3), x.b3, x.params, NB, x.P, x.H, x.W, x.st);
}
int stage_sample(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  if (r.fused_tail_allowed) return 0;
  dump(x, b0, 6, x.params, (size_t)NB * x.P * x.H * x.W * 4);
  return os2d_launch_sample_decode(x.corr, x.params, NB, x.H, x.W, x.P, x.inverse, x.stride, x.rec_field, bc, x.B, b0, x.loc, x.cls, x.corners,
                                   x.flags, x.epoch, x.status, x.st);
}

// shared prologue of os2d_corr_f16x3 / os2d_corr_f16x3_packed: their workspace starts with sumsq | split image features
// (os2d_corr_f16x3_workspace_bytes); both are filled
int corr_f16x3_prologue(const float* fm, void* workspace, int A, int C, int H, int W, hipStream_t st, void** fs) {
  float* sumsq = static_cast<float*>(workspace);
  *fs = static_cast<char*>(workspace) + align_up((size_t)A * H * W * sizeof(float), 256);
  const int rc = os2d_launch_fm_sumsq(fm, sumsq, A, C, H * W, st);
  return rc ? rc : os2d_launch_split_fm(fm, sumsq, *fs, A, C, H * W, nullptr, 0, Os2dRangeFlag{nullptr, 0}, st);
}
// BatchNorm folding takes all four of weight / bias / running_mean / running_var, or none
bool bn_all_or_none(const float* weight, const float* bias, const float* mean, const float* var) {
  return (weight && bias && mean && var) || !(weight || bias || mean || var);
}
// argument and alignment checks of the per-bin GEMM entry points (`hint`: what the entry point's text adds to the shape)
bool spectral_gemm_args_ok(const char* who, const char* hint, const void* w, const float* X, const float* Y, int NB, int C, int Cout, int nbins,
                           float xscale) {
  if (!w || !X || !Y || NB < 1 || C < 1 || Cout < 1 || Cout > 128 || nbins < 8 || (nbins & 7) || !(xscale > 0.f)) {
    os2d_set_error("%s: bad arguments (NB=%d C=%d Cout=%d nbins=%d%s)", who, NB, C, Cout, nbins, hint);
    return false;
  }
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) {
    os2d_set_error("%s: buffers must be 16-byte aligned", who);
    return false;
  }
  return true;
}
// the same for the two weight-spectra builders; P != NULL: the matrix-product family, whose transform length is a multiple of 4
bool spectra_build_args_ok(const char* who, const double* wfold, const double* twP64, const double* twQ64, const void* out,
                           const void* workspace, bool need_workspace, int C, int Cout, int nbins, const int* P) {
  if (!wfold || !twP64 || !twQ64 || !out || (need_workspace && !workspace) || C < 1 || Cout < 1 || Cout > 128 || nbins < 8 || (nbins & 7) ||
      (P && (*P & 3))) {
    if (P) os2d_set_error("%s: bad arguments (C=%d Cout=%d P=%d nbins=%d)", who, C, Cout, *P, nbins);
    else os2d_set_error("%s: bad arguments (C=%d Cout=%d nbins=%d)", who, C, Cout, nbins);
    return false;
  }
  if ((reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
    os2d_set_error("%s: out must be 16-byte, workspace 8-byte aligned", who);
    return false;
  }
  return true;
}
}  // namespace

void os2d_debug_set_dump(void* stream, int slot, void* dst, size_t bytes) {
#ifdef OS2D_DIAG_DUMP
  std::lock_guard<std::mutex> lock(g_dumps_mutex);
  for (size_t i = 0; i < g_dumps.size(); ++i)
    if (g_dumps[i].stream == stream && g_dumps[i].slot == slot) {
      if (dst) {
        g_dumps[i].dst = dst;
        g_dumps[i].bytes = bytes;
      } else {
        g_dumps.erase(g_dumps.begin() + i);          // dst == NULL unregisters the slot
      }
      return;
    }
  if (dst) g_dumps.push_back(DumpEntry{stream, slot, dst, bytes});
#else
  (void)stream, (void)slot, (void)dst, (void)bytes;
  os2d_set_error("os2d_debug_set_dump: this library was built without -DOS2D_DIAG_DUMP (diagnostic builds only)");
#endif
}

extern "C" {

int os2d_abi_version(void) { return OS2D_ABI_VERSION; }
const char* os2d_last_error(void) { return os2d_error_text; }

size_t os2d_packed_conv_floats(int layer) {
  ConvShape s;
  if (!conv_shape(layer, 6, &s)) return 0;
  return (size_t)((s.cin + 1) / 2) * s.ks * s.ks * 2 * s.mt;
}
size_t os2d_packed_bias_floats(int layer) {
  ConvShape s;
  if (!conv_shape(layer, 6, &s)) return 0;
  return (size_t)3 * s.mt;  // folded bias | per-row 2^-weight_exp | per-row 2^out_exp (f16x3 packing; fp32: first third)
}

int os2d_pack_conv(int layer, int P, const float* w, const float* b, const float* bn_weight, const float* bn_bias,
                   const float* bn_running_mean, const float* bn_running_var, float bn_eps, float* packed_w,
                   float* packed_b, void* stream) {
  ConvShape s;
  if (!conv_shape(layer, P, &s) || (layer == 3 && P != 6 && P != 4)) {
    os2d_set_error("os2d_pack_conv: bad layer %d / P %d", layer, P);
    return -1;
  }
  if (!w || !b || !packed_w || !packed_b) return os2d_refuse("os2d_pack_conv: null pointer");
  if (!bn_all_or_none(bn_weight, bn_bias, bn_running_mean, bn_running_var))
    return os2d_refuse("os2d_pack_conv: BatchNorm needs all four of weight/bias/running_mean/running_var");
  return os2d_launch_pack_conv(w, b, bn_weight, bn_bias, bn_running_mean, bn_running_var, bn_eps, s.cout, s.cin, s.ks,
                               s.mt, packed_w, packed_b, os2d_stream(stream));
}

int os2d_class_prepare(const float* src, int C, int h, int w, int normalize, float* q15, float* qp, void* stream) {
  if (!src || !q15 || !qp || C < 1 || h < 1 || w < 1) {
    os2d_set_error("os2d_class_prepare: bad arguments (C=%d h=%d w=%d)", C, h, w);
    return -1;
  }
  return os2d_launch_class_prepare(src, C, h, w, normalize, q15, qp, os2d_stream(stream));
}

size_t os2d_class_prepare_workspace_floats(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)os2d_class_prepare_partial_floats(B, C);
}

int os2d_class_prepare_batch(const float* const* srcs, const int* sizes, int B, int C, int normalize, float* q15,
                             float* qp, float* workspace, void* stream) {
  if (!srcs || !sizes || !q15 || !qp || !workspace || B < 1 || C < 1 || B > 65535) {
    os2d_set_error("os2d_class_prepare_batch: bad arguments (B=%d C=%d; at most 65535 classes per call)", B, C);
    return -1;
  }
  return os2d_launch_class_prepare_batch(srcs, sizes, B, C, normalize, q15, qp, workspace, os2d_stream(stream));
}

size_t os2d_plane_floats(int H, int W) { return (size_t)os2d_plane(H, W); }

size_t os2d_shb_bytes(int channels, int H, int W) {
  if (channels < 1 || H < 1 || W < 1) return 0;
  return (size_t)((channels + 7) / 8) * 2 * os2d_plane(H, W) * 16;
}

int os2d_head_workspace_bytes(int A, int B, int C, int H, int W, int P, size_t* bytes) {
  return head_workspace_bytes("os2d_head_workspace_bytes", A, B, C, H, W, P, OS2D_PRECISION_F32, bytes);
}

int os2d_head_workspace_bytes_ex(int A, int B, int C, int H, int W, int P, int precision, size_t* bytes) {
  return head_workspace_bytes("os2d_head_workspace_bytes_ex", A, B, C, H, W, P, precision, bytes);
}

int os2d_fm_sumsq(const float* fm, float* sumsq, int A, int C, int H, int W, void* stream) {
  if (!fm || !sumsq || A < 1 || C < 1 || H < 1 || W < 1) {
    os2d_set_error("os2d_fm_sumsq: bad arguments");
    return -1;
  }
  return os2d_launch_fm_sumsq(fm, sumsq, A, C, H * W, os2d_stream(stream));
}

int os2d_corr(const float* fm, const float* qp, const float* sumsq, float* corr, float* rnorm, int A, int B, int C,
              int H, int W, void* stream) {
  if (!fm || !qp || !sumsq || !corr || !rnorm) {
    os2d_set_error("os2d_corr: null pointer");
    return -1;
  }
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  int rc = os2d_launch_border_zero(rnorm, A * B * OS2D_KP, H, W, os2d_stream(stream));
  if (rc) return rc;
  return os2d_launch_corr(fm, qp, sumsq, corr, rnorm, nullptr, A, B, C, H, W, 0, os2d_stream(stream));
}

size_t os2d_corr_f16x3_workspace_bytes(int A, int C, int H, int W) {
  if (A < 1 || C < 1 || H < 1 || W < 1) return 0;
  return align_up((size_t)A * H * W * sizeof(float), 256) + (size_t)A * os2d_corr_groups(C) * 2 * H * W * 16;
}

int os2d_corr_f16x3(const float* fm, const void* qs, float* corr, void* rshb, int A, int B, int C, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!fm || !qs || !corr || !rshb || !workspace) return os2d_refuse("os2d_corr_f16x3: null pointer");
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  if (workspace_bytes < os2d_corr_f16x3_workspace_bytes(A, C, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
    os2d_set_error("os2d_corr_f16x3: workspace too small or not 256-byte aligned");
    return -2;
  }
  void* fs;
  int rc = corr_f16x3_prologue(fm, workspace, A, C, H, W, os2d_stream(stream), &fs);
  if (!rc) rc = os2d_launch_border_zero_shb(rshb, A * B, H, W, os2d_stream(stream));
  if (!rc) rc = os2d_launch_corr_f16x3(fs, qs, corr, rshb, nullptr, nullptr, 0, A, B, C, H, W, os2d_stream(stream));
  return rc;
}

size_t os2d_corr_f16x3_packed_workspace_bytes(int A, int B, int C, int H, int W) {
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return align_up(os2d_corr_f16x3_workspace_bytes(A, C, H, W), 256) + (size_t)A * B * H * W * sizeof(unsigned long long);
}

int os2d_corr_f16x3_packed(const float* fm, const void* qs, float* corr, float* inv_norm, int A, int B, int C, int H, int W,
                           int form, void* workspace, size_t workspace_bytes, void* stream) {
  if (!fm || !qs || !corr || !inv_norm || !workspace) return os2d_refuse("os2d_corr_f16x3_packed: null pointer");
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  if (form < -1 || form > 7 || (form >= 0 && (form & 3) > 1)) {
    os2d_set_error("os2d_corr_f16x3_packed: form %d (0 padded | 1 packed | -1 the head's choice; + 4: no half tiles at the tail)", form);
    return -1;
  }
  if (workspace_bytes < os2d_corr_f16x3_packed_workspace_bytes(A, B, C, H, W) || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
    os2d_set_error("os2d_corr_f16x3_packed: workspace too small or not 256-byte aligned");
    return -2;
  }
  void *fs, *sumfx = static_cast<char*>(workspace) + align_up(os2d_corr_f16x3_workspace_bytes(A, C, H, W), 256);
  int rc = corr_f16x3_prologue(fm, workspace, A, C, H, W, os2d_stream(stream), &fs);
  const bool packed = form < 0 ? os2d_corr_f16x3_use_packed(A, B, H, W) != 0 : (form & 1) != 0;
  if (!rc && packed) rc = os2d_launch_corr_sums_clear(sumfx, A, B, H, W, os2d_stream(stream));
  if (!rc) rc = os2d_launch_corr_f16x3(fs, qs, corr, nullptr, inv_norm, packed ? sumfx : nullptr, (form >= 0 && (form & 4)) ? 2 : 0, A, B, C, H, W, os2d_stream(stream));
  return rc;
}

int os2d_corr_normalize(const float* corr, float* rnorm, int NB, int H, int W, void* stream) {
  if (!corr || !rnorm || NB < 1 || H < 1 || W < 1) {
    os2d_set_error("os2d_corr_normalize: bad arguments");
    return -1;
  }
  return os2d_launch_corr_normalize(corr, rnorm, NB, H, W, os2d_stream(stream));
}

int os2d_transform_conv(int layer, const float* in, const float* packed_w, const float* packed_b, float* out, int NB,
                        int P, int H, int W, void* stream) {
  if (!in || !packed_w || !packed_b || !out || NB < 1 || H < 1 || W < 1 || (layer == 3 && P != 6 && P != 4)) {
    os2d_set_error("os2d_transform_conv: bad arguments (layer=%d NB=%d P=%d)", layer, NB, P);
    return -1;
  }
  return os2d_launch_conv(layer, in, packed_w, packed_b, out, NB, P, H, W, os2d_stream(stream));
}

int os2d_sample_decode(const float* corr, const float* params, int NB, int H, int W, int P, int inverse, int stride,
                       int rec_field, float* loc, float* cls, float* corners, void* stream) {
  if (!corr || !params || !loc || !cls || !corners || NB < 1 || H < 1 || W < 1 || (P != 6 && P != 4)) {
    os2d_set_error("os2d_sample_decode: bad arguments");
    return -1;
  }
  return os2d_launch_sample_decode(corr, params, NB, H, W, P, inverse, stride, rec_field, NB, NB, 0, loc, cls,
                                   corners, nullptr, 0, nullptr, os2d_stream(stream));
}

int os2d_decode_boxes(const float* loc, int NB, int H, int W, int stride, int rec_field, float img_w, float img_h,
                      float* boxes, void* stream) {
  if (!loc || !boxes || NB < 1 || H < 1 || W < 1) {
    os2d_set_error("os2d_decode_boxes: bad arguments");
    return -1;
  }
  return os2d_launch_decode_boxes(loc, NB, H, W, stride, rec_field, img_w, img_h, boxes, os2d_stream(stream));
}

int os2d_detect_level_supported(int H, int W) { return os2d_detect_level_lds_bytes(H, W) != 0 ? 1 : 0; }

int os2d_detect_level(const float* loc, const float* cls, int B, int H, int W, int stride, int rec_field, float img_w,
                      float img_h, float scale_x, float scale_y, float score_threshold, float iou_threshold,
                      float* out_boxes, float* out_scores, int* out_index, int* out_count, void* stream) {
  if (!loc || !cls || !out_boxes || !out_scores || !out_index || !out_count || B < 1 || H < 1 || W < 1 || stride < 1 ||
      rec_field < 1) {
    os2d_set_error("os2d_detect_level: bad arguments");
    return -1;
  }
  return os2d_launch_detect_level(loc, cls, B, H, W, stride, rec_field, img_w, img_h, os2d_box_ops_scale<OS2D_BOX_MAX_OPS>(scale_x, scale_y),
                                  score_threshold, iou_threshold, out_boxes, out_scores, out_index, out_count, os2d_stream(stream));
}

int os2d_detect_level_ops(const float* loc, const float* cls, int B, int H, int W, int stride, int rec_field, float img_w,
                          float img_h, int op_count, const int* op_kinds, const float* op_args, float score_threshold,
                          float iou_threshold, float* out_boxes, float* out_scores, int* out_index, int* out_count,
                          void* stream) {
  if (!loc || !cls || !out_boxes || !out_scores || !out_index || !out_count || B < 1 || H < 1 || W < 1 || stride < 1 ||
      rec_field < 1) {
    os2d_set_error("os2d_detect_level_ops: bad arguments");
    return -1;
  }
  Os2dBoxOps ops;
  if (!os2d_box_ops_from(op_kinds, op_args, op_count, &ops)) {
    os2d_set_error("os2d_detect_level_ops: bad transform chain (at most %d ops of kind 1..4)", OS2D_BOX_MAX_OPS);
    return -1;
  }
  return os2d_launch_detect_level(loc, cls, B, H, W, stride, rec_field, img_w, img_h, ops, score_threshold, iou_threshold,
                                  out_boxes, out_scores, out_index, out_count, os2d_stream(stream));
}

int os2d_nms_workspace_bytes(int NC, int N, size_t* bytes) {
  if (!bytes || NC < 1 || N < 1) {
    os2d_set_error("os2d_nms_workspace_bytes: bad arguments");
    return -1;
  }
  *bytes = (size_t)NC * N * 4 * sizeof(float);
  return 0;
}

int os2d_nms(const float* boxes, const int* counts, int NC, int N, float iou_threshold, unsigned char* keep,
             int* num_keep, void* workspace, size_t workspace_bytes, void* stream) {
  if (!boxes || !counts || !keep || !num_keep || !workspace || NC < 1 || N < 1) {
    os2d_set_error("os2d_nms: bad arguments");
    return -1;
  }
  if ((reinterpret_cast<uintptr_t>(boxes) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    os2d_set_error("os2d_nms: boxes and workspace must be 16-byte aligned");
    return -1;
  }
  if (workspace_bytes < (size_t)NC * N * 4 * sizeof(float)) {
    os2d_set_error("os2d_nms: workspace too small");
    return -2;
  }
  return os2d_launch_nms(boxes, counts, NC, N, iou_threshold, keep, num_keep, workspace, os2d_stream(stream));
}

int os2d_head_forward_ex2(const float* fm, const float* qp, const void* w1, const float* b1, const void* w2,
                          const float* b2, const void* w3, const float* b3, int A, int B, int C, int H, int W, int P,
                          int inverse, int stride, int rec_field, float* loc, float* cls, float* corners,
                          void* workspace, size_t workspace_bytes, void* stream, int precision, const void* qs,
                          void** stage_events, int* chunk_classes, int* status, const float* wspec, const float* twQ,
                          const float* twP, const void* wspec2) {
  if (!fm || !qp || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !loc || !cls || !corners || !workspace) return os2d_refuse("os2d_head_forward: null pointer");
  if (is_freq(precision) && (!wspec || !twQ || (precision != OS2D_PRECISION_FFTX3 && !twP)))
    return os2d_refuse("os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables "
                       "(fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)");
  HeadRoute route;
  int rc = head_route("os2d_head_forward", precision, H, W, wspec2 != nullptr, true, &route);
  if (rc) return rc;
  if (route.f16 && !qs) return os2d_refuse("os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)");
  if (!head_args_ok(A, B, C, H, W, P)) return -1;
  if (stride < 1 || rec_field < 1) {
    os2d_set_error("os2d_head_forward: bad stride/rec_field %d/%d", stride, rec_field);
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return os2d_refuse("os2d_head_forward: workspace must be 256-byte aligned");
  const int Bc = largest_chunk(route, A, B, C, H, W, P, workspace_bytes);
  if (!Bc) {
    os2d_set_error("os2d_head_forward: workspace too small (%zu B, need >= %zu B for one class)", workspace_bytes,
                   carve(route, A, 1, C, H, W, P).total);
    return -2;
  }
  if (chunk_classes) *chunk_classes = Bc;
  HeadCall x = {fm, qp, b1, b2, b3, wspec, twQ, twP, w1, w2, w3, qs, wspec2, A, B, C, H, W, P, inverse, stride, rec_field, loc, cls, corners,
                status, stage_events, os2d_stream(stream)};
  const Carve c = carve(route, A, Bc, C, H, W, P);
  char* ws = static_cast<char*>(workspace);
  auto floats = [&](size_t offset) { return reinterpret_cast<float*>(ws + offset); };
  x.sumsq = floats(c.sumsq);
  x.fsplit = ws + c.fs;
  x.corr = floats(c.corr);
  x.rpad = route.bins ? nullptr : floats(c.rpad);
  x.h1 = floats(c.h1);
  x.h2 = floats(c.h2);
  x.params = floats(c.params);
  x.invn = route.bins ? floats(c.invn) : nullptr;
  x.xspec = route.bins ? floats(c.xspec) : nullptr;
  x.yspec = route.bins ? floats(c.yspec) : nullptr;
  // half-precision correlation on the frequency-domain route: classes packed along M (no padded rows 225 .. 255 per class)
  // - when that saves a round of the chip (os2d_corr_f16x3_use_packed: both forms give the same bits; decided on the chunk size
  // so that every chunk but a shorter last one takes the same form)
  x.sumfx = (route.bins && route.f16 && os2d_corr_f16x3_use_packed(A, Bc, H, W)) ? ws + c.sumfx : nullptr;
  x.flags = route.f16 ? reinterpret_cast<int*>(ws + c.flags) : nullptr;
  x.epoch = next_epoch();
  x.per_image = {x.flags, x.epoch};
  x.whole_call = {route.f16 ? x.flags + A : nullptr, x.epoch};

  if ((rc = os2d_launch_fm_sumsq(fm, x.sumsq, A, C, H * W, x.st))) return rc;
  // (the packed correlation kernel's sums are cleared by the same launch; every chunk's norms pass leaves them cleared again)
  if (route.f16 && (rc = os2d_launch_split_fm(fm, x.sumsq, x.fsplit, A, C, H * W, x.sumfx, x.sumfx ? (size_t)A * Bc * H * W : 0, x.per_image, x.st)))
    return rc;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int bc = (B - b0 < Bc) ? (B - b0) : Bc;
    mark(x, b0, 0);
    if ((rc = stage_corr(route, x, b0, bc))) return rc;
    mark(x, b0, 1);
    mark(x, b0, 2);
    if ((rc = stage_conv1(route, x, b0, bc))) return rc;
    mark(x, b0, 3);
    mark(x, b0, 4);
    if ((rc = stage_conv2(route, x, b0, bc))) return rc;
    mark(x, b0, 5);
    mark(x, b0, 6);
    if ((rc = stage_conv3(route, x, b0, bc))) return rc;      // (the fused tail: events 7, 8 and 9 follow its one launch)
    mark(x, b0, 7);
    mark(x, b0, 8);
    if ((rc = stage_sample(route, x, b0, bc))) return rc;
    mark(x, b0, 9);
  }
  return 0;
}

int os2d_head_forward_ex(const float* fm, const float* qp, const void* w1, const float* b1, const void* w2,
                         const float* b2, const void* w3, const float* b3, int A, int B, int C, int H, int W, int P,
                         int inverse, int stride, int rec_field, float* loc, float* cls, float* corners,
                         void* workspace, size_t workspace_bytes, void* stream, int precision, const void* qs,
                         void** stage_events, int* chunk_classes, int* status, const float* wspec, const float* twQ,
                         const float* twP) {
  return os2d_head_forward_ex2(fm, qp, w1, b1, w2, b2, w3, b3, A, B, C, H, W, P, inverse, stride, rec_field, loc, cls, corners, workspace,
                               workspace_bytes, stream, precision, qs, stage_events, chunk_classes, status, wspec, twQ, twP, nullptr);
}

int os2d_head_forward(const float* fm, const float* qp, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, int A, int B, int C, int H, int W, int P,
                      int inverse, int stride, int rec_field, float* loc, float* cls, float* corners, void* workspace,
                      size_t workspace_bytes, void* stream) {
  return os2d_head_forward_ex(fm, qp, w1, b1, w2, b2, w3, b3, A, B, C, H, W, P, inverse, stride, rec_field, loc, cls,
                              corners, workspace, workspace_bytes, stream, OS2D_PRECISION_F32, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr);
}

size_t os2d_class_split_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * os2d_corr_groups(C) * 2 * 256 * 16;
}

int os2d_class_split(const float* qp, void* qs, int B, int C, void* stream) {
  if (!qp || !qs || B < 1 || C < 1) {
    os2d_set_error("os2d_class_split: bad arguments");
    return -1;
  }
  return os2d_launch_split_qp(qp, qs, B, C, os2d_stream(stream));
}

size_t os2d_packed_conv_bytes(int layer, int precision) {
  if (precision == OS2D_PRECISION_F32) return os2d_packed_conv_floats(layer) * sizeof(float);
  if (precision != OS2D_PRECISION_F16X3 && precision != OS2D_PRECISION_F16X2) return 0;
  // [G][steps padded to whole stages][2][2][MT] units of 16 B (conv_f16x3.hip: layer 1 SS=5, layer 2 SS=7)
  if (layer == 1) return (size_t)OS2D_G * os2d_conv1_steps_padded() * 4 * 128 * 16;
  if (layer == 2) return (size_t)16 * 14 * 4 * 64 * 16;
  if (layer == 3) return (size_t)8 * 14 * 4 * 32 * 16;
  return 0;
}

int os2d_pack_conv_f16x3(int layer, int P, const float* w, const float* b, const float* bn_weight, const float* bn_bias,
                         const float* bn_running_mean, const float* bn_running_var, float bn_eps, const int* weight_exp,
                         const int* in_exp, const int* out_exp, void* packed_w, float* packed_b, void* stream) {
  if (layer < 1 || layer > 3 || !w || !b || !packed_w || !packed_b || !weight_exp || !in_exp ||
      (layer != 3 && !out_exp) || !bn_all_or_none(bn_weight, bn_bias, bn_running_mean, bn_running_var) ||
      (layer == 3 && P != 6 && P != 4)) {
    os2d_set_error("os2d_pack_conv_f16x3: bad arguments (layer %d, P %d)", layer, P);
    return -1;
  }
  ConvShape s;
  conv_shape(layer, P, &s);
  return os2d_launch_pack_conv_f16(w, b, bn_weight, bn_bias, bn_running_mean, bn_running_var, bn_eps, s.cout, s.cin, s.ks, s.mt,
                                   layer == 1 ? os2d_conv1_steps_padded() : 14, weight_exp, in_exp, layer == 3 ? nullptr : out_exp, packed_w,
                                   packed_b, os2d_stream(stream));
}

int os2d_rnorm_exp(void) { return OS2D_RNORM_EXP; }

int os2d_corr_normalize_f16x3(const float* corr, void* rshb, int NB, int H, int W, void* stream) {
  if (!corr || !rshb || NB < 1 || H < 1 || W < 1) {
    os2d_set_error("os2d_corr_normalize_f16x3: bad arguments");
    return -1;
  }
  return os2d_launch_corr_normalize_shb(corr, rshb, NB, H, W, os2d_stream(stream));
}

int os2d_transform_conv_f16x3(int layer, const void* in, const void* packed_w, const float* packed_b, void* out, int NB,
                              int P, int H, int W, int terms, int* status, void* stream) {
  if (!in || !packed_w || !packed_b || !out || NB < 1 || H < 1 || W < 1 || layer < 1 || layer > 3 ||
      (layer == 3 && P != 6 && P != 4) || (terms != 3 && !(terms == 2 && layer == 1))) {
    os2d_set_error("os2d_transform_conv_f16x3: bad arguments (layer=%d NB=%d P=%d terms=%d)", layer, NB, P, terms);
    return -1;
  }
  if (W > (layer == 1 ? OS2D_MAX_W_DIRECT7 : OS2D_MAX_W)) {
    os2d_set_error("os2d_transform_conv_f16x3: feature map width %d > %d", W, layer == 1 ? OS2D_MAX_W_DIRECT7 : OS2D_MAX_W);
    return -1;
  }
  return os2d_launch_conv_f16x3(layer, in, packed_w, packed_b, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE}, out, NB, P, H, W, terms, os2d_stream(stream));
}

int os2d_fft_sizes(int H, int W, int* P, int* Q, int* nbins) {
  if (!P || !Q || !nbins) {
    os2d_set_error("os2d_fft_sizes: null output");
    return -1;
  }
  if (!os2d_fft_plan(H, W, P, Q, nbins, nullptr)) {
    os2d_set_error("os2d_fft_sizes: no transform plan for a %dx%d map", H, W);
    return -3;
  }
  return 0;
}

int os2d_fft_tiles(int H, int W, int* tiles_y, int* tiles_x, int* tile_h, int* tile_w) {
  int t[6];
  if (!tiles_y || !tiles_x || !tile_h || !tile_w) {
    os2d_set_error("os2d_fft_tiles: null output");
    return -1;
  }
  if (!os2d_fft_plan(H, W, nullptr, nullptr, nullptr, t)) {
    os2d_set_error("os2d_fft_tiles: no transform plan for a %dx%d map", H, W);
    return -3;
  }
  *tiles_y = t[0];
  *tiles_x = t[1];
  *tile_h = t[2];
  *tile_w = t[3];
  return 0;
}

int os2d_fft_forward(const float* corr, const float* inv_norm, float* X, const float* twQ, const float* twP, int NB, int C,
                     int H, int W, void* stream) {
  if (!corr || !inv_norm || !X || !twQ || !twP || NB < 1 || C < 1 || H < 1 || W < 1) {
    os2d_set_error("os2d_fft_forward: bad arguments");
    return -1;
  }
  return os2d_launch_fft_forward(corr, inv_norm, X, twQ, twP, NB, C, H, W, os2d_stream(stream));
}

int os2d_fft_inverse_ex(const float* Y, const float* packed_b, void* out, const float* twQ, const float* twP, int NB, int Cout,
                        int H, int W, int* status, int layout, void* stream) {
  if (!Y || !packed_b || !out || !twQ || !twP || NB < 1 || Cout != 128 || H < 1 || W < 1 ||
      (layout != OS2D_SPECTRA_ROWS && layout != OS2D_SPECTRA_QUADS)) {
    os2d_set_error("os2d_fft_inverse: bad arguments (Cout must be 128: the 7x7 layer)");
    return -1;
  }
  int rc = os2d_launch_border_zero_shb_planes(out, NB * (Cout / 8) * 2, H, W, os2d_stream(stream));
  if (rc) return rc;
  return os2d_launch_fft_inverse(Y, packed_b, 128, out, twQ, twP, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE}, layout, 0, os2d_stream(stream));
}

int os2d_fft_inverse(const float* Y, const float* packed_b, void* out, const float* twQ, const float* twP, int NB, int Cout,
                     int H, int W, int* status, void* stream) {
  return os2d_fft_inverse_ex(Y, packed_b, out, twQ, twP, NB, Cout, H, W, status, OS2D_SPECTRA_ROWS, stream);
}

size_t os2d_spectral_weight_bytes(int C, int Cout, int nbins) {
  if (C < 1 || Cout < 1 || Cout > 128 || nbins < 8 || (nbins & 7)) return 0;
  return os2d_spectral_weight_floats(C, Cout, nbins) * sizeof(float);
}

int os2d_spectral_gemm(const float* wspec, const float* X, float* Y, int NB, int C, int Cout, int nbins, void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm", "; nbins must be a multiple of 8", wspec, X, Y, NB, C, Cout, nbins, 1.f)) return -1;
  return os2d_launch_spectral_gemm(wspec, X, Y, NB, C, Cout, nbins, os2d_stream(stream));
}

int os2d_spectral_weights_build(const double* wfold, const double* twP64, const double* twQ64, int C, int Cout, int P, int Q,
                                int nbins, int split, void* out, void* workspace, void* stream) {
  if (!spectra_build_args_ok("os2d_spectral_weights_build", wfold, twP64, twQ64, out, workspace, split != 0, C, Cout, nbins, nullptr)) return -1;
  return os2d_launch_spectra_pack(wfold, twP64, twQ64, C, Cout, P, Q, nbins, split, 0, out, workspace, os2d_stream(stream));
}

size_t os2d_spectral_weight16_bytes(int C, int nbins) {
  if (C < 1 || nbins < 8 || (nbins & 7)) return 0;
  return os2d_spectral_weight16_size(C, nbins);
}

float os2d_spectral_xscale(int H, int W) {
  int t[6];
  if (H < 1 || W < 1 || !os2d_fft_plan(H, W, nullptr, nullptr, nullptr, t)) return 0.f;
  return os2d_spectral_xscale_for(t[4], t[5]);      // samples of one transform window (the whole map, or a tile + its halo)
}

int os2d_spectral_gemm_f16(const void* w16, const float* X, float* Y, int NB, int C, int Cout, int nbins, float xscale,
                           void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm_f16", "; nbins must be a multiple of 8", w16, X, Y, NB, C, Cout, nbins, xscale)) return -1;
  return os2d_launch_spectral_gemm_f16(w16, X, Y, NB, C, Cout, nbins, xscale, 0, 0, os2d_stream(stream));
}

/* ---- the transforms of the frequency-domain 7x7 layer as matrix products (dft_mfma.hip; OS2D_PRECISION_FFTX3) */
int os2d_dft_sizes(int H, int W, int* P, int* Q, int* nbins, int* tiles) {
  if (!P || !Q || !nbins) {
    os2d_set_error("os2d_dft_sizes: null output");
    return -1;
  }
  if (!os2d_dft_plan(H, W, P, Q, nbins, tiles)) {
    os2d_set_error("os2d_dft_sizes: no transform plan for a %dx%d map", H, W);
    return -3;
  }
  return 0;
}

int os2d_dft_channel_stride(int C) { return C == OS2D_K ? OS2D_XSPEC_CPAD : (C + 7) / 8 * 8; }

size_t os2d_dft_matrices_bytes(int P, int Q) {
  if (P < 4 || (P & 3) || Q < 2 || (Q & 1)) return 0;
  return os2d_dft_matrices_size(P, Q);
}

int os2d_dft_matrices_build(const double* twP64, const double* twQ64, int P, int Q, void* out, void* stream) {
  if (!twP64 || !twQ64 || !out || (reinterpret_cast<uintptr_t>(out) & 15)) {
    os2d_set_error("os2d_dft_matrices_build: bad arguments (out must be 16-byte aligned)");
    return -1;
  }
  return os2d_launch_dft_matrices(twP64, twQ64, P, Q, out, os2d_stream(stream));
}

int os2d_dft_forward(const float* corr, const float* inv_norm, float* X, const void* matrices, int NB, int C, int H, int W,
                     void* stream) {
  if (!corr || !X || !matrices || NB < 1 || C < 1 || H < 1 || W < 1) {      // inv_norm == NULL: unit norms
    os2d_set_error("os2d_dft_forward: bad arguments");
    return -1;
  }
  return os2d_launch_dft_forward(corr, inv_norm, X, matrices, NB, C, os2d_dft_channel_stride(C), H, W, os2d_stream(stream));
}

int os2d_dft_inverse(const float* Y, const float* packed_b, void* out, const void* matrices, int NB, int Cout, int H, int W,
                     int* status, void* stream) {
  if (!Y || !packed_b || !out || !matrices || NB < 1 || (Cout != 128 && Cout != 64) || H < 1 || W < 1) {
    os2d_set_error("os2d_dft_inverse: bad arguments (Cout must be 128 or 64: the 7x7 layer / the 5x5 layer 128 -> 64)");
    return -1;
  }
  return os2d_launch_dft_inverse(Y, packed_b, Cout, out, matrices, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE},
                                 OS2D_DFT_OUT_SHB_BORDERS, os2d_stream(stream));
}

int os2d_dft_inverse_planes(const float* Y, const float* packed_b, float* out, const void* matrices, int NB, int Cout, int H, int W,
                            int* status, void* stream) {
  if (!Y || !packed_b || !out || !matrices || NB < 1 || (Cout != 128 && Cout != 64) || H < 1 || W < 1) {
    os2d_set_error("os2d_dft_inverse_planes: bad arguments (Cout must be 128 or 64)");
    return -1;
  }
  return os2d_launch_dft_inverse(Y, packed_b, Cout, out, matrices, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE},
                                 OS2D_DFT_OUT_PLANES, os2d_stream(stream));
}

int os2d_spectral_weights_build_dft(const double* wfold, const double* twP64, const double* twQ64, int C, int Cout, int P, int Q,
                                    int nbins, void* out, void* workspace, void* stream) {
  if (!spectra_build_args_ok("os2d_spectral_weights_build_dft", wfold, twP64, twQ64, out, workspace, true, C, Cout, nbins, &P)) return -1;
  return os2d_launch_spectra_pack(wfold, twP64, twQ64, C, Cout, P, Q, nbins, 1, 1, out, workspace, os2d_stream(stream));
}

int os2d_spectral_gemm_f16_quads(const void* w16, const float* X, float* Y, int NB, int C, int Cout, int nbins, float xscale,
                                 void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm_f16_quads", "", w16, X, Y, NB, C, Cout, nbins, xscale)) return -1;
  return os2d_launch_spectral_gemm_f16(w16, X, Y, NB, C, Cout, nbins, xscale, 1, os2d_dft_channel_stride(C), os2d_stream(stream));
}

float os2d_dft_xscale(int H, int W) {
  int t[6];
  if (H < 1 || W < 1 || !os2d_dft_plan(H, W, nullptr, nullptr, nullptr, t)) return 0.f;
  return os2d_spectral_xscale_for(t[4], t[5]);
}

int os2d_alignment_grids(const float* params, int NB, int H, int W, int P, int inverse, float* theta, float* grids,
                         void* stream) {
  if (!params || (!theta && !grids) || NB < 1 || H < 1 || W < 1 || (P != 6 && P != 4)) {
    os2d_set_error("os2d_alignment_grids: bad arguments");
    return -1;
  }
  return os2d_launch_alignment_grids(params, NB, H, W, P, inverse, theta, grids, os2d_stream(stream));
}

int os2d_prof_event_create(void** ev) {
  hipEvent_t e;
  hipError_t rc = hipEventCreate(&e);
  if (rc != hipSuccess || !ev) {
    os2d_set_error("hipEventCreate: %s", hipGetErrorString(rc));
    return -4;
  }
  *ev = e;
  return 0;
}
int os2d_prof_event_destroy(void* ev) { return hipEventDestroy(reinterpret_cast<hipEvent_t>(ev)) == hipSuccess ? 0 : -4; }
int os2d_prof_event_elapsed_ms(void* a, void* b, float* ms) {
  hipError_t rc = hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(a), reinterpret_cast<hipEvent_t>(b));
  if (rc != hipSuccess) {
    os2d_set_error("hipEventElapsedTime: %s", hipGetErrorString(rc));
    return -4;
  }
  return 0;
}

}  // extern "C"
