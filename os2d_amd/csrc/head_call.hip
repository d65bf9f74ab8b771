// The head call of libos2d_hip.so (include/os2d_hip.h: os2d_head_forward*, os2d_head_workspace_bytes*): the route of a precision,
// the workspace carve, the five stages of a class chunk and the diagnostic dump aid.  Host code only; the per-stage entry points
// are abi.hip's.
#include "../../include/os2d_hip.h"
#include "abi_sizes.h"
#include <atomic>
#include <mutex>
#include <random>
#include <vector>

namespace {
constexpr Os2dLayer L1 = os2d_layer(1), L2 = os2d_layer(2);

// ---- What does not depend on the class chunk is decided once (head_route) and kept in a HeadRoute: the size entry points and
// os2d_head_forward_ex2 carve the workspace from the same record, the stage functions branch on its fields.
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

// workspace carve for a chunk of Bc classes: byte offset and byte size of every buffer (a buffer the route does not use: 0 bytes)
struct Span {
  size_t at, bytes;
};
struct Carve {
  Span flags, sumsq, fs, corr, rpad, h1, h2, params, invn, sumfx, xspec, yspec;
  size_t total;
};
Carve carve(const HeadRoute& r, int A, int Bc, int C, int H, int W, int P) {
  const size_t HW = (size_t)H * W, NB = (size_t)A * Bc, F = sizeof(float);
  Carve c = {};
  auto take = [&](size_t bytes) {
    const Span s = {c.total, bytes};
    c.total = align_up(c.total + bytes, 256);
    return s;
  };
  c.flags = take(((size_t)A + 1) * F);     // range words of the call: one per image + one for the whole call (Os2dRangeFlag); FIRST
  c.sumsq = take((size_t)A * HW * F);
  c.fs = take(fm_split_bytes(A, C, HW));   // f16x3
  c.corr = take(NB * L1.cin * HW * F);
  // fp32: 226 planes; f16x3: 29 groups x (hi|lo) x 16 B = 232 floats; not needed by the frequency-domain 7x7 layer
  c.rpad = take(r.bins > 0 ? 0 : NB * shb_bytes(L1.cin, H, W));
  c.h1 = take(NB * L1.cout * os2d_plane(H, W) * F);
  c.h2 = take(NB * L2.cout * os2d_plane(H, W) * F);
  c.params = take(NB * P * HW * F);
  if (r.bins > 0) {  // frequency-domain 7x7 layer: inverse norms, input / output spectra (complex64)
    c.invn = take(NB * HW * F);
    c.sumfx = take(NB * HW * sizeof(unsigned long long));      // 64-bit fixed-point sums of the packed correlation kernel (corr_f16x3.hip, STACK)
    c.xspec = take(NB * r.T * r.xch * (size_t)r.bins * 2 * F);     // a tile of a tiled map is one more "pair" (fft.hip)
    c.yspec = take(NB * r.T * L1.cout * (size_t)r.bins * 2 * F);
  }
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
// What the precision alone decides (no plan yet); false for an unknown precision, which gets the record of the fp32 route
bool precision_route(int precision, HeadRoute* r) {
  *r = HeadRoute{precision, false, T7_NONE, false, false, false, 3, OS2D_SPECTRA_ROWS, 0, {1, 1, 0, 0, 0, 0}, 1, L1.cin};
  switch (precision) {
    case OS2D_PRECISION_F32: return true;
    case OS2D_PRECISION_F16X3: r->f16 = true; return true;
    case OS2D_PRECISION_F16X2: r->f16 = true, r->terms1 = 2; return true;
    case OS2D_PRECISION_FFT32: r->transform = T7_FFT; return true;
    case OS2D_PRECISION_FFT: r->f16 = true, r->transform = T7_FFT; return true;
    case OS2D_PRECISION_FFTX3: r->f16 = true, r->transform = T7_DFT, r->layout = OS2D_SPECTRA_QUADS, r->xch = OS2D_XSPEC_CPAD; return true;
    default: return false;
  }
}
// The route of a call in `precision` on an H x W map; 0, or the error text is set (`who`: the entry point) and -1 for an unknown
// precision or a map too wide for the direct 7x7 kernels, -3 when the transforms have no plan.  launch = false (the size entry
// points, which launch nothing): those two -1 cases get the footprint of the direct routes, as they always did.
int head_route(const char* who, int precision, int H, int W, bool have_wspec2, bool launch, HeadRoute* r) {
  if (!precision_route(precision, r) && launch) return OS2D_REFUSE(-1, "%s: unknown precision %d", who, precision);
  if (r->transform == T7_NONE) {
    if (launch && W > OS2D_MAX_W_DIRECT7)
      return OS2D_REFUSE(-1, "feature map width %d > %d: the direct 7x7 kernels keep 3 halo rows of their input in LDS - wider maps need a "
                         "frequency-domain precision (fftx3 / fft / fft32), which tiles any width up to %d", W, OS2D_MAX_W_DIRECT7, OS2D_MAX_W);
  } else if (!(r->transform == T7_DFT ? os2d_dft_plan : os2d_fft_plan)(H, W, nullptr, nullptr, &r->bins, r->tiles)) {
    return OS2D_REFUSE(-3, "%s: no transform plan for a %dx%d map", who, H, W);
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
  if (!bytes) return OS2D_REFUSE(-1, "%s: null output", who);
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
  Carve layout;             // of the class chunk: where the buffers below lie and how many bytes each holds
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
// diagnostic builds: a copy of a buffer of the first class chunk (which is as long as the carve's: `bytes` is a Carve size or a part of
// one); slots: 0 corr, 1 inverse norms, 2 input spectra, 3 output spectra, 4 h1, 5 h2, 6 params
void dump(const HeadCall& x, int b0, int slot, const void* src, size_t bytes) {
  if (b0 == 0 && dumps_active()) dump_slot(x.st, slot, src, bytes);
}

// ---- the five stages of the class chunk [b0, b0 + bc), called in this order by the chunk loop of os2d_head_forward_ex2
int stage_corr(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  int rc;
  // the frequency-domain 7x7 layer takes corr + invn; the split / blocked copy of the normalised maps is not written
  if (!r.bins && (rc = r.f16 ? os2d_launch_border_zero_shb(x.rpad, NB, x.H, x.W, x.st) : os2d_launch_border_zero(x.rpad, NB * L1.planes(), x.H, x.W, x.st)))
    return rc;
  if (!r.f16) return os2d_launch_corr(x.fm, x.qp + (size_t)b0 * x.C * OS2D_QROWS, x.sumsq, x.corr, x.rpad, x.invn, x.A, bc, x.C, x.H, x.W, 0, x.st);
  const char* qsb = static_cast<const char*>(x.qs) + (size_t)b0 * class_split_bytes(x.C);
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
    const int planes = (r.borders_in_inverse || r.conv2_freq) ? 0 : NB * L2.groups * 2;
    if ((planes || x.sumfx) && (rc = os2d_launch_border_zero_shb_planes_norms(x.h1, planes, H, W, x.sumfx, x.invn, (size_t)NB * H * W, x.st)))
      return rc;
  } else if ((rc = os2d_launch_border_zero(x.h1, NB * L1.cout, H, W, x.st))) {     // all-fp32 mode: fp32 planes for the fp32 5x5 kernel
    return rc;
  }
  mark(x, b0, 10);
  if (r.transform == T7_FFT) {
    if ((rc = os2d_launch_fft_forward(x.corr, x.invn, x.xspec, x.twQ, x.twP, NB, L1.cin, H, W, x.st))) return rc;
    mark(x, b0, 11);
    if ((rc = os2d_launch_spectral_gemm(x.wspec, x.xspec, x.yspec, NB * r.T, L1.cin, L1.cout, r.bins, x.st))) return rc;
    mark(x, b0, 12);
    return os2d_launch_fft_inverse(x.yspec, x.b1, L1.rows, x.h1, x.twQ, x.twP, NB, L1.cout, H, W, x.whole_call, r.layout, r.f16 ? 0 : 1, x.st);
  }
  // the transforms as matrix products on the half-precision matrix cores (twQ = the matrices), spectra in quads of bins on both
  // sides of the per-bin GEMM; |X| <= number of samples of a window (every sample of the normalised maps is <= 1)
  if ((rc = os2d_launch_dft_forward(x.corr, x.invn, x.xspec, x.twQ, NB, L1.cin, r.xch, H, W, x.st))) return rc;
  mark(x, b0, 11);
  if ((rc = os2d_launch_spectral_gemm_f16(x.wspec, x.xspec, x.yspec, NB * r.T, L1.cin, L1.cout, r.bins, os2d_spectral_xscale_for(r.tiles[4], r.tiles[5]), 1, r.xch, x.st)))
    return rc;
  mark(x, b0, 12);
  return os2d_launch_dft_inverse(x.yspec, x.b1, L1.rows, x.h1, x.twQ, NB, L1.cout, H, W, x.whole_call,
                                 r.conv2_freq ? OS2D_DFT_OUT_PLANES : r.borders_in_inverse ? OS2D_DFT_OUT_SHB_BORDERS : OS2D_DFT_OUT_SHB, x.st);
}
int stage_conv2(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc, H = x.H, W = x.W;
  const Carve& c = x.layout;
  int rc;
  dump(x, b0, 0, x.corr, c.corr.bytes);
  if (r.bins) {
    dump(x, b0, 1, x.invn, c.invn.bytes);
    // The input spectra are dumped with the layer's 225 channels although the buffer's channel stride is r.xch (232 on the fftx3
    // route), i.e. 225 / 232 of the buffer: the byte count of a diagnostic build is kept as it was; correcting it is a change of its own.
    dump(x, b0, 2, x.xspec, c.xspec.bytes / r.xch * L1.cin);
    dump(x, b0, 3, x.yspec, c.yspec.bytes);
  }
  // (fp32 planes without borders on the transform route of layer 2: H * W of the PLANE cells of every channel)
  dump(x, b0, 4, x.h1, r.conv2_freq ? c.h1.bytes / os2d_plane(H, W) * ((size_t)H * W) : c.h1.bytes);
  if (!r.conv2_freq)
    return r.f16 ? os2d_launch_conv_f16x3(2, x.h1, x.w2, x.b2, x.whole_call, x.h2, NB, x.P, H, W, 3, x.st)
                 : os2d_launch_conv(2, x.h1, static_cast<const float*>(x.w2), x.b2, x.h2, NB, x.P, H, W, x.st);
  // h1: fp32 planes [pair][128][H * W], every sample in [0, 1] - unit norms, and the ReLU of the forward kernel changes nothing;
  // both spectra buffers are reused (128 channels fit the input stride, 64 the output buffer)
  if ((rc = os2d_launch_dft_forward(x.h1, nullptr, x.xspec, x.twQ, NB, L2.cin, L2.cin, H, W, x.st))) return rc;
  if ((rc = os2d_launch_spectral_gemm_f16(x.wspec2, x.xspec, x.yspec, NB * r.T, L2.cin, L2.cout, r.bins, os2d_spectral_xscale_for(r.tiles[4], r.tiles[5]), 1, L2.cin, x.st)))
    return rc;
  return os2d_launch_dft_inverse(x.yspec, x.b2, L2.rows, x.h2, x.twQ, NB, L2.cout, H, W, x.whole_call, OS2D_DFT_OUT_SHB_BORDERS, x.st);
}
// fused tail: ONE launch for the last layer and the alignment epilogue (conv3_f16x3.hip, FUSE: the parameters go from the accumulators
// through LDS to the resampler, never to HBM), and stage_sample has nothing left to do
int stage_conv3(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  dump(x, b0, 5, x.h2, x.layout.h2.bytes);
  if (r.fused_tail_allowed)
    return os2d_launch_conv3_sample_decode(x.h2, x.w3, x.b3, x.corr, NB, x.H, x.W, x.P, x.inverse, x.stride, x.rec_field, bc, x.B, b0, x.loc, x.cls,
                                           x.corners, x.flags, x.epoch, x.status, x.st);
  return r.f16 ? os2d_launch_conv_f16x3(3, x.h2, x.w3, x.b3, x.whole_call, x.params, NB, x.P, x.H, x.W, 3, x.st)
               : os2d_launch_conv(3, x.h2, static_cast<const float*>(x.w3), x.b3, x.params, NB, x.P, x.H, x.W, x.st);
}
int stage_sample(const HeadRoute& r, const HeadCall& x, int b0, int bc) {
  const int NB = x.A * bc;
  if (r.fused_tail_allowed) return 0;
  dump(x, b0, 6, x.params, x.layout.params.bytes);
  return os2d_launch_sample_decode(x.corr, x.params, NB, x.H, x.W, x.P, x.inverse, x.stride, x.rec_field, bc, x.B, b0, x.loc, x.cls, x.corners,
                                   x.flags, x.epoch, x.status, x.st);
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

int os2d_head_workspace_bytes(int A, int B, int C, int H, int W, int P, size_t* bytes) {
  return head_workspace_bytes("os2d_head_workspace_bytes", A, B, C, H, W, P, OS2D_PRECISION_F32, bytes);
}

int os2d_head_workspace_bytes_ex(int A, int B, int C, int H, int W, int P, int precision, size_t* bytes) {
  return head_workspace_bytes("os2d_head_workspace_bytes_ex", A, B, C, H, W, P, precision, bytes);
}

int os2d_head_forward_ex2(const float* fm, const float* qp, const void* w1, const float* b1, const void* w2,
                          const float* b2, const void* w3, const float* b3, int A, int B, int C, int H, int W, int P,
                          int inverse, int stride, int rec_field, float* loc, float* cls, float* corners,
                          void* workspace, size_t workspace_bytes, void* stream, int precision, const void* qs,
                          void** stage_events, int* chunk_classes, int* status, const float* wspec, const float* twQ,
                          const float* twP, const void* wspec2) {
  if (!fm || !qp || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !loc || !cls || !corners || !workspace) return OS2D_REFUSE(-1, "os2d_head_forward: null pointer");
  HeadRoute route;
  precision_route(precision, &route);      // (an unknown precision is head_route's to refuse, after the tables)
  if (route.transform != T7_NONE && (!wspec || !twQ || (route.transform != T7_DFT && !twP)))
    return OS2D_REFUSE(-1, "os2d_head_forward: the frequency-domain modes need the weight spectra and the transform tables "
                       "(fft / fft32: twQ, twP; fftx3: the matrices of os2d_dft_matrices_build as twQ)");
  int rc = head_route("os2d_head_forward", precision, H, W, wspec2 != nullptr, true, &route);
  if (rc) return rc;
  if (route.f16 && !qs) return OS2D_REFUSE(-1, "os2d_head_forward: precision f16x3 / f16x2 needs the split class operand (os2d_class_split)");
  if (!head_args_ok(A, B, C, H, W, P)) return -1;
  if (stride < 1 || rec_field < 1) return OS2D_REFUSE(-1, "os2d_head_forward: bad stride/rec_field %d/%d", stride, rec_field);
  if (!aligned_to(256, workspace)) return OS2D_REFUSE(-1, "os2d_head_forward: workspace must be 256-byte aligned");
  const int Bc = largest_chunk(route, A, B, C, H, W, P, workspace_bytes);
  if (!Bc)
    return OS2D_REFUSE(-2, "os2d_head_forward: workspace too small (%zu B, need >= %zu B for one class)", workspace_bytes,
                       carve(route, A, 1, C, H, W, P).total);
  if (chunk_classes) *chunk_classes = Bc;
  HeadCall x = {fm, qp, b1, b2, b3, wspec, twQ, twP, w1, w2, w3, qs, wspec2, A, B, C, H, W, P, inverse, stride, rec_field, loc, cls, corners,
                status, stage_events, os2d_stream(stream), carve(route, A, Bc, C, H, W, P)};
  const Carve& c = x.layout;
  char* ws = static_cast<char*>(workspace);
  auto floats = [&](const Span& s) { return reinterpret_cast<float*>(ws + s.at); };
  x.sumsq = floats(c.sumsq);
  x.fsplit = ws + c.fs.at;
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
  x.sumfx = (route.bins && route.f16 && os2d_corr_f16x3_use_packed(A, Bc, H, W)) ? ws + c.sumfx.at : nullptr;
  x.flags = route.f16 ? reinterpret_cast<int*>(ws + c.flags.at) : nullptr;
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

}  // extern "C"
