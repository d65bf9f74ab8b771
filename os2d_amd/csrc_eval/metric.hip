// VOC evaluation, step 3 (gfx950): precision / recall curves, their running maximum and the average precision of every class
// (reference os2d/data/voc_eval.py:150-253), over ONE sorted array of all D detections whose segments are the classes - or one
// segment of D positions for the joint class, so no segment may be tied to a work-group.
//
// All three array steps are segmented inclusive scans, device-wide in three launches each:
//   scan_partials_kernel  (value, "a segment starts in here") of every tile of EVAL_TILE positions
//   scan_carries_kernel   exclusive scan of those pairs by one work-group: what flows into every tile
//   scan_apply_kernel     the tile's scan again, started from its carry, and the step's stores
// with the steps
//   PrecRec   forward, integer (tp << 32 | fp) sums of match == 1 / match == 0 -> prec = tp / (tp + fp), rec = tp / n_pos (fp64,
//             one IEEE division each), the last recall of every segment
//   RunMax    backward, max of nan_to_num(prec): mpre
//   ApSum     forward, fp64 sum of (rec[i] - rec[i-1]) * mpre[i] where rec changes; the last position of a segment stores it
// ap11_kernel is the 11-point form (no sum: each of the 11 recall levels has one first position that reaches it) and
// finalise_kernel turns the per-class numbers into ap / recall arrays and the four scalars.
// The order of every sum is fixed by the tile geometry; there is no floating-point atomic.
#include "../../include/os2d_eval.h"
#include "eval_common.h"

namespace {

template <typename T>
struct Seg {
  T v;
  int f;   // a segment starts at or before the last element this value covers
};

template <class P>
__device__ __forceinline__ Seg<typename P::T> combine(Seg<typename P::T> a, Seg<typename P::T> b) {
  Seg<typename P::T> r;
  r.v = b.f ? b.v : P::op(a.v, b.v);
  r.f = a.f | b.f;
  return r;
}

// Exclusive scan of one Seg per thread over the work-group, started from `start`; *total = start combined with all of them.
template <class P>
__device__ __forceinline__ Seg<typename P::T> block_exclusive(Seg<typename P::T> mine, Seg<typename P::T> start, Seg<typename P::T>* total) {
  typedef typename P::T T;
  __shared__ T agg_v[EVAL_THREADS / 64];
  __shared__ int agg_f[EVAL_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  Seg<T> incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    Seg<T> o;
    o.v = __shfl_up(incl.v, off);
    o.f = __shfl_up(incl.f, off);
    if (lane >= off) incl = combine<P>(o, incl);
  }
  __syncthreads();   // the previous use of agg_* is over
  if (lane == 63) {
    agg_v[wv] = incl.v;
    agg_f[wv] = incl.f;
  }
  __syncthreads();
  Seg<T> ex = start, all = start;
#pragma unroll
  for (int w = 0; w < EVAL_THREADS / 64; ++w) {
    Seg<T> a;
    a.v = agg_v[w];
    a.f = agg_f[w];
    if (w < wv) ex = combine<P>(ex, a);
    all = combine<P>(all, a);
  }
  Seg<T> prev;
  prev.v = __shfl_up(incl.v, 1);
  prev.f = __shfl_up(incl.f, 1);
  if (lane > 0) ex = combine<P>(ex, prev);
  *total = all;
  return ex;
}

// The scan of one tile.  Logical position i runs forward; the array position is D-1-i for a backward step.
template <class P, bool STORE>
__device__ __forceinline__ Seg<typename P::T> tile_scan(const P& p, int D, typename P::T carry) {
  typedef typename P::T T;
  const long long first = (long long)blockIdx.x * EVAL_TILE + (long long)threadIdx.x * EVAL_ITEMS;
  // segment of the positions first-1 .. first+EVAL_ITEMS.  Outside the array the value is a filler that decides nothing: the
  // first position is a head and the last a tail by their index, so a segment may carry any label, -1 included.
  int s[EVAL_ITEMS + 2];
#pragma unroll
  for (int k = 0; k < EVAL_ITEMS + 2; ++k) {
    const long long i = first - 1 + k;
    s[k] = (i < 0 || i >= D) ? -1 : (p.seg ? p.seg[P::REV ? D - 1 - i : i] : 0);
  }
  T v[EVAL_ITEMS];
  bool own[EVAL_ITEMS];   // a segment started inside this thread's run, at or before the position
  Seg<T> run;
  run.v = P::identity();
  run.f = 0;
#pragma unroll
  for (int k = 0; k < EVAL_ITEMS; ++k) {
    const long long i = first + k;
    if (i < D) {
      const bool head = i == 0 || s[k + 1] != s[k];
      const T x = p.load((int)(P::REV ? D - 1 - i : i), head);
      run.v = head ? x : P::op(run.v, x);
      run.f |= head ? 1 : 0;
    }
    v[k] = run.v;
    own[k] = run.f != 0;
  }
  Seg<T> start, total;
  start.v = carry;
  start.f = 0;
  const Seg<T> ex = block_exclusive<P>(run, start, &total);
  if (STORE) {
#pragma unroll
    for (int k = 0; k < EVAL_ITEMS; ++k) {
      const long long i = first + k;
      if (i < D) p.store((int)(P::REV ? D - 1 - i : i), own[k] ? v[k] : P::op(ex.v, v[k]), i == D - 1 || s[k + 2] != s[k + 1], s[k + 1]);
    }
  }
  return total;
}

template <class P>
__global__ __launch_bounds__(EVAL_THREADS) void scan_partials_kernel(P p, int D, typename P::T* __restrict__ part_v, int* __restrict__ part_f) {
  const Seg<typename P::T> total = tile_scan<P, false>(p, D, P::identity());
  if (threadIdx.x == 0) {
    part_v[blockIdx.x] = total.v;
    part_f[blockIdx.x] = total.f;
  }
}

template <class P>
__global__ __launch_bounds__(EVAL_THREADS) void scan_carries_kernel(const typename P::T* __restrict__ part_v, const int* __restrict__ part_f, int n,
                                                                     typename P::T* __restrict__ carry) {
  typedef typename P::T T;
  Seg<T> c;
  c.v = P::identity();
  c.f = 0;
  for (int base = 0; base < n; base += EVAL_THREADS) {
    const int b = base + threadIdx.x;
    Seg<T> x;
    x.v = b < n ? part_v[b] : P::identity();
    x.f = b < n ? part_f[b] : 0;
    Seg<T> total;
    const Seg<T> ex = block_exclusive<P>(x, c, &total);
    if (b < n) carry[b] = ex.v;
    c = total;
  }
}

template <class P>
__global__ __launch_bounds__(EVAL_THREADS) void scan_apply_kernel(P p, int D, const typename P::T* __restrict__ carry) {
  tile_scan<P, true>(p, D, carry[blockIdx.x]);
}

struct PrecRec {
  typedef u64 T;
  static const bool REV = false;
  const signed char* match;
  const u32* perm;
  const int* seg;
  const int* n_pos;
  int L;
  u64* tpfp;
  double *prec, *rec, *rec_last;
  static __device__ __forceinline__ T identity() { return 0ull; }
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
  __device__ __forceinline__ T load(int j, bool) const {
    const int m = match[perm[j]];
    return ((u64)(m == 1) << 32) | (u64)(m == 0);
  }
  __device__ __forceinline__ void store(int j, T v, bool tail, int s) const {
    const u32 tp = (u32)(v >> 32), fp = (u32)v;
    const bool known = (unsigned)s < (unsigned)L;   // a label outside [0, L) has no n_pos
    const int np = known ? n_pos[s] : 0;
    const double r = (double)tp / (double)np;
    prec[j] = (double)tp / (double)(tp + fp);
    rec[j] = r;
    if (tpfp) tpfp[j] = v;
    if (tail && np > 0) rec_last[s] = r;
  }
};

struct RunMax {
  typedef double T;
  static const bool REV = true;
  const double* prec;
  const int* seg;
  double* mpre;
  static __device__ __forceinline__ T identity() { return 0.0; }
  static __device__ __forceinline__ T op(T a, T b) { return a > b ? a : b; }
  __device__ __forceinline__ T load(int j, bool) const {
    const double x = prec[j];
    return x != x ? 0.0 : x;
  }
  __device__ __forceinline__ void store(int j, T v, bool, int) const { mpre[j] = v; }
};

struct ApSum {
  typedef double T;
  static const bool REV = false;
  const double *rec, *mpre;
  const int* seg;
  int L;
  double* acc;
  static __device__ __forceinline__ T identity() { return 0.0; }
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
  __device__ __forceinline__ T load(int j, bool head) const {
    const double r = rec[j], before = head ? 0.0 : rec[j - 1];
    return r != before ? (r - before) * mpre[j] : 0.0;
  }
  __device__ __forceinline__ void store(int, T v, bool tail, int s) const {
    if (tail && (unsigned)s < (unsigned)L) acc[(size_t)s * 11] = v;
  }
};

// 11-point form: acc[s][t] = mpre at the first position of segment s whose recall reaches t / 10 (0.1 * t in fp64, the
// values of numpy.arange(0, 1.1, 0.1)); rec never decreases, so that is max(prec[rec >= t])
__global__ __launch_bounds__(EVAL_THREADS) void ap11_kernel(const double* __restrict__ rec, const double* __restrict__ mpre, const int* __restrict__ seg,
                                                             int L, int D, double* __restrict__ acc) {
  const int i = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (i >= D) return;
  const int s = seg ? seg[i] : 0;
  if ((unsigned)s >= (unsigned)L) return;
  const bool head = i == 0 || (seg && seg[i - 1] != s);
  const double r = rec[i], before = head ? 0.0 : rec[i - 1];
  const double m = mpre[i];
#pragma unroll
  for (int t = 0; t < 11; ++t) {
    const double level = 0.1 * (double)t;
    if (r >= level && (head || !(before >= level))) acc[(size_t)s * 11 + t] = m;
  }
}

__device__ __forceinline__ double class_ap(const double* __restrict__ acc, int l, int use_07) {
  if (!use_07) return acc[(size_t)l * 11];
  double ap = 0.0;
  for (int t = 0; t < 11; ++t) ap += acc[(size_t)l * 11 + t] / 11.0;
  return ap;
}

// one work-group: thread t takes the classes t, t + 256, ..; the four sums are reduced over the threads in a fixed tree
__global__ __launch_bounds__(EVAL_THREADS) void finalise_kernel(const double* __restrict__ acc, const double* __restrict__ rec_last,
                                                                 const int* __restrict__ n_pos, int L, int use_07, double* __restrict__ ap_out,
                                                                 double* __restrict__ recall_out, double* __restrict__ n_pos_out,
                                                                 double* __restrict__ scalars) {
  __shared__ double red[4][EVAL_THREADS];
  const int tid = threadIdx.x;
  const double nan = __builtin_nan("");
  const double total = (double)n_pos[L];
  double ap_sum = 0.0, ap_cnt = 0.0, ap_w = 0.0, good = 0.0;
  for (int l = tid; l < L; l += EVAL_THREADS) {
    const int np = n_pos[l];
    double ap = nan, rc = nan;
    if (np > 0) {
      ap = class_ap(acc, l, use_07);
      rc = rec_last[l];
      ap_sum += ap;
      ap_cnt += 1.0;
      ap_w += ap * (double)np / total;
      good += (double)np * rc;
    }
    ap_out[l] = ap;
    recall_out[l] = rc;
    n_pos_out[l] = (double)np;
  }
  red[0][tid] = ap_sum;
  red[1][tid] = ap_cnt;
  red[2][tid] = ap_w;
  red[3][tid] = good;
  __syncthreads();
  for (int half = EVAL_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    scalars[0] = red[0][0] / red[1][0];                       // nanmean: NaN when no class has positives
    scalars[1] = red[2][0];                                   // nansum(ap * n_pos / n_pos.sum())
    scalars[2] = total > 0.0 ? red[3][0] / total : nan;
    scalars[3] = total > 0.0 ? class_ap(acc, L, use_07) : nan;
  }
}

struct ScanWorkspace {
  void* part_v;
  int* part_f;
  void* carry;
};

bool carve(void* workspace, size_t bytes, int D, ScanWorkspace* w) {
  if (!workspace || bytes < os2d_eval_scan_workspace_bytes(D)) return false;
  const size_t each = align256(8 * (size_t)tiles(D));
  char* base = static_cast<char*>(workspace);
  w->part_v = base;
  w->part_f = reinterpret_cast<int*>(base + each);
  w->carry = base + 2 * each;
  return true;
}

template <class P>
int device_scan(const P& p, int D, const ScanWorkspace& w, hipStream_t st, const char* what) {
  typedef typename P::T T;
  const int nt = tiles(D);
  hipLaunchKernelGGL(scan_partials_kernel<P>, dim3(nt), dim3(EVAL_THREADS), 0, st, p, D, static_cast<T*>(w.part_v), w.part_f);
  if (int rc = os2d_launched(what)) return rc;
  hipLaunchKernelGGL(scan_carries_kernel<P>, dim3(1), dim3(EVAL_THREADS), 0, st, static_cast<const T*>(w.part_v), w.part_f, nt,
                     static_cast<T*>(w.carry));
  if (int rc = os2d_launched(what)) return rc;
  hipLaunchKernelGGL(scan_apply_kernel<P>, dim3(nt), dim3(EVAL_THREADS), 0, st, p, D, static_cast<const T*>(w.carry));
  return os2d_launched(what);
}

}  // namespace

extern "C" {

size_t os2d_eval_scan_workspace_bytes(int D) { return D <= 0 ? 0 : 3 * align256(8 * (size_t)tiles(D)); }

int os2d_eval_prec_rec(const signed char* match, const unsigned int* perm, const int* seg, const int* n_pos, int L, int D,
                       unsigned long long* tpfp, double* prec, double* rec, double* rec_last, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (D < 0 || L < 1) return os2d_refuse("prec_rec: bad shape (D >= 0, L >= 1)");
  if (D == 0) return 0;
  if (!match || !perm || !n_pos || !prec || !rec || !rec_last) return os2d_refuse("prec_rec: null pointer");
  ScanWorkspace w;
  if (!carve(workspace, workspace_bytes, D, &w)) {
    os2d_set_error("prec_rec: workspace too small");
    return -2;
  }
  PrecRec p;
  p.match = match;
  p.perm = perm;
  p.seg = seg;
  p.n_pos = n_pos;
  p.L = L;
  p.tpfp = tpfp;
  p.prec = prec;
  p.rec = rec;
  p.rec_last = rec_last;
  return device_scan(p, D, w, os2d_stream(stream), "prec_rec scan");
}

int os2d_eval_ap(const double* prec, const double* rec, const int* seg, int L, int D, int use_07_metric, double* mpre, double* acc,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (D < 0 || L < 1) return os2d_refuse("ap: bad shape (D >= 0, L >= 1)");
  if (D == 0) return 0;
  if (!prec || !rec || !mpre || !acc) return os2d_refuse("ap: null pointer");
  ScanWorkspace w;
  if (!carve(workspace, workspace_bytes, D, &w)) {
    os2d_set_error("ap: workspace too small");
    return -2;
  }
  RunMax m;
  m.prec = prec;
  m.seg = seg;
  m.mpre = mpre;
  if (int rc = device_scan(m, D, w, os2d_stream(stream), "running maximum scan")) return rc;
  if (use_07_metric) {
    hipLaunchKernelGGL(ap11_kernel, dim3((D + EVAL_THREADS - 1) / EVAL_THREADS), dim3(EVAL_THREADS), 0, os2d_stream(stream), rec, mpre, seg, L, D, acc);
    return os2d_launched("ap11_kernel");
  }
  ApSum a;
  a.rec = rec;
  a.mpre = mpre;
  a.seg = seg;
  a.L = L;
  a.acc = acc;
  return device_scan(a, D, w, os2d_stream(stream), "average precision scan");
}

int os2d_eval_finalise(const double* acc, const double* rec_last, const int* n_pos, int L, int use_07_metric, double* ap_per_class,
                       double* recall_per_class, double* n_pos_out, double* scalars, void* stream) {
  if (L < 1) return os2d_refuse("finalise: bad shape (L >= 1)");
  if (!acc || !rec_last || !n_pos || !ap_per_class || !recall_per_class || !n_pos_out || !scalars) return os2d_refuse("finalise: null pointer");
  hipLaunchKernelGGL(finalise_kernel, dim3(1), dim3(EVAL_THREADS), 0, os2d_stream(stream), acc, rec_last, n_pos, L, use_07_metric, ap_per_class,
                     recall_per_class, n_pos_out, scalars);
  return os2d_launched("finalise_kernel");
}

}  // extern "C"
