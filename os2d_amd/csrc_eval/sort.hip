// VOC evaluation, step 2 (gfx950): a stable LSD radix sort of (key, index) pairs with 8-bit digits, over all D detections.
//
// Four passes over os2d_score_key give the joint-classes order (descending score), further passes over the label key give the
// per-class order; equal keys keep increasing index (image order, then index within the image) because every pass is stable.
// Neither order depends on an IoU threshold.  The label key of a label outside [0, L) is L: such rows sort behind every
// class, in descending score, so the passes cover the bits of L (and label_bits, if the caller asks for more).
//
// One pass = radix_hist_kernel (digit histogram of a tile of EVAL_TILE keys in LDS, stored digit-major), radix_scan_kernel
// (exclusive scan of the 256 x tiles counts: one work-group, 4096 counts per round) and radix_scatter_kernel.  In the scatter
// a wave owns EVAL_ITEMS consecutive runs of 64 keys; the rank of a key among the equal digits of its run comes from ballots
// over the eight digit bits, the ranks of earlier runs and earlier waves from ordered per-wave counts in LDS.
#include "../../include/os2d_eval.h"
#include "../csrc/detect_common.h"
#include "eval_common.h"

namespace {

#define SCAN_THREADS 1024

__global__ __launch_bounds__(EVAL_THREADS) void sort_init_kernel(const float* __restrict__ scores, int D, u32* __restrict__ keys, u32* __restrict__ idx) {
  const int i = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (i >= D) return;
  keys[i] = os2d_score_key(scores[i]);
  idx[i] = (u32)i;
}

// label key: the label, or L for a label outside [0, L) - low digits alone would file label 256 among those of label 0
__global__ __launch_bounds__(EVAL_THREADS) void gather_labels_kernel(const int* __restrict__ labels, const u32* __restrict__ perm, int D, int L,
                                                                      u32* __restrict__ keys) {
  const int i = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (i >= D) return;
  const u32 l = (u32)labels[perm[i]];
  keys[i] = l < (u32)L ? l : (u32)L;
}

__global__ __launch_bounds__(EVAL_THREADS) void radix_hist_kernel(const u32* __restrict__ keys, int D, int shift, u32* __restrict__ hist, int ntiles) {
  __shared__ u32 h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * EVAL_TILE;
#pragma unroll
  for (int k = 0; k < EVAL_ITEMS; ++k) {
    const long long i = base + k * EVAL_THREADS + tid;
    if (i < D) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)tid * ntiles + blockIdx.x] = h[tid];
}

// exclusive scan of counts[n] in place by ONE work-group: rounds of 4 counts per thread, a wave scan by shuffles, the wave
// totals through LDS, the total of the round carried into the next
__global__ __launch_bounds__(SCAN_THREADS) void radix_scan_kernel(u32* __restrict__ counts, int n) {
  __shared__ u32 wsum[SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  u32 carry = 0;
  for (int base = 0; base < n; base += 4 * SCAN_THREADS) {
    const int i = base + 4 * tid;
    u32 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? counts[i + k] : 0u;
    const u32 mine = v[0] + v[1] + v[2] + v[3];
    u32 incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    u32 before = carry, total = 0;
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      if (w < wv) before += wsum[w];
      total += wsum[w];
    }
    u32 run = before + incl - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < n) counts[i + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(EVAL_THREADS) void radix_scatter_kernel(const u32* __restrict__ keys_in, const u32* __restrict__ idx_in,
                                                                      u32* __restrict__ keys_out, u32* __restrict__ idx_out, int D, int shift,
                                                                      const u32* __restrict__ offs, int ntiles) {
  __shared__ volatile u32 wcnt[EVAL_THREADS / 64][256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int w = 0; w < EVAL_THREADS / 64; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * EVAL_TILE + wv * (64 * EVAL_ITEMS);
  const u64 below = (1ull << lane) - 1ull;
  u32 key[EVAL_ITEMS], idx[EVAL_ITEMS], rank[EVAL_ITEMS];
#pragma unroll
  for (int k = 0; k < EVAL_ITEMS; ++k) {
    const long long i = base + k * 64 + lane;
    const bool valid = i < D;
    key[k] = valid ? keys_in[i] : 0u;
    idx[k] = valid ? idx_in[i] : 0u;
    const u32 dg = (key[k] >> shift) & 255u;
    u64 same = __ballot(valid);   // lanes of this run with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg >> b) & 1u;
      const u64 vote = __ballot(bit);
      same &= bit ? vote : ~vote;
    }
    const u32 r = (u32)__popcll(same & below);
    const u32 seen = wcnt[wv][dg];        // equal digits in the earlier runs of this wave
    rank[k] = seen + r;
    __builtin_amdgcn_wave_barrier();
    if (valid && r == 0) wcnt[wv][dg] = seen + (u32)__popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {   // thread = digit: the counts of the waves become their first output positions
    u32 run = offs[(size_t)tid * ntiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < EVAL_THREADS / 64; ++w) {
      const u32 c = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EVAL_ITEMS; ++k) {
    const long long i = base + k * 64 + lane;
    if (i < D) {
      const u32 pos = wcnt[wv][(key[k] >> shift) & 255u] + rank[k];
      keys_out[pos] = key[k];
      idx_out[pos] = idx[k];
    }
  }
}

// class_offsets[l] = first position with sorted label >= l (l = 0 .. L)
__global__ __launch_bounds__(EVAL_THREADS) void class_offsets_kernel(const int* __restrict__ sorted_labels, int D, int L, int* __restrict__ offsets) {
  const int l = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (l > L) return;
  int lo = 0, hi = D;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted_labels[mid] < l) lo = mid + 1;
    else hi = mid;
  }
  offsets[l] = lo;
}

struct SortBuffers {
  u32 *key_a, *key_b, *idx_a, *idx_b, *hist;
};

int radix_pass(const u32* kin, const u32* iin, u32* kout, u32* iout, int D, int shift, u32* hist, hipStream_t st) {
  const int nt = tiles(D);
  hipLaunchKernelGGL(radix_hist_kernel, dim3(nt), dim3(EVAL_THREADS), 0, st, kin, D, shift, hist, nt);
  if (int rc = os2d_launched("radix_hist_kernel")) return rc;
  hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, hist, 256 * nt);
  if (int rc = os2d_launched("radix_scan_kernel")) return rc;
  hipLaunchKernelGGL(radix_scatter_kernel, dim3(nt), dim3(EVAL_THREADS), 0, st, kin, iin, kout, iout, D, shift, hist, nt);
  return os2d_launched("radix_scatter_kernel");
}

}  // namespace

extern "C" {

size_t os2d_eval_sort_workspace_bytes(int D) {
  if (D <= 0) return 0;
  return 4 * align256(sizeof(u32) * (size_t)D) + align256(sizeof(u32) * 256 * (size_t)tiles(D));
}

int os2d_eval_sort(const float* det_scores, const int* det_labels, int D, int L, int label_bits, unsigned int* perm_joint,
                   unsigned int* perm_class, int* sorted_labels, int* class_offsets, void* workspace, size_t workspace_bytes, void* stream) {
  if (D < 0 || L < 1 || label_bits < 0 || label_bits > 31 || ((L - 1) >> label_bits) != 0)
    return os2d_refuse("sort: bad shape (D >= 0, L >= 1, L <= 2^label_bits)");
  if (!class_offsets) return os2d_refuse("sort: null pointer (class_offsets)");
  hipStream_t st = os2d_stream(stream);
  if (D == 0) {
    if (hipMemsetAsync(class_offsets, 0, sizeof(int) * ((size_t)L + 1), st) != hipSuccess) return os2d_launched("sort: memset");
    return 0;
  }
  if (!det_scores || !det_labels || !perm_joint || !perm_class || !sorted_labels || !workspace) return os2d_refuse("sort: null pointer");
  if (workspace_bytes < os2d_eval_sort_workspace_bytes(D)) {
    os2d_set_error("sort: workspace too small");
    return -2;
  }
  char* w = static_cast<char*>(workspace);
  const size_t each = align256(sizeof(u32) * (size_t)D);
  u32* key_a = reinterpret_cast<u32*>(w);
  u32* key_b = reinterpret_cast<u32*>(w + each);
  u32* idx_a = reinterpret_cast<u32*>(w + 2 * each);
  u32* idx_b = reinterpret_cast<u32*>(w + 3 * each);
  u32* hist = reinterpret_cast<u32*>(w + 4 * each);
  const dim3 flat((D + EVAL_THREADS - 1) / EVAL_THREADS);
  hipLaunchKernelGGL(sort_init_kernel, flat, dim3(EVAL_THREADS), 0, st, det_scores, D, key_a, idx_a);
  if (int rc = os2d_launched("sort_init_kernel")) return rc;
  // score key: a -> b -> a -> b -> (a, perm_joint)
  if (int rc = radix_pass(key_a, idx_a, key_b, idx_b, D, 0, hist, st)) return rc;
  if (int rc = radix_pass(key_b, idx_b, key_a, idx_a, D, 8, hist, st)) return rc;
  if (int rc = radix_pass(key_a, idx_a, key_b, idx_b, D, 16, hist, st)) return rc;
  if (int rc = radix_pass(key_b, idx_b, key_a, perm_joint, D, 24, hist, st)) return rc;
  // label: starts from the joint order, so equal labels stay in descending score
  hipLaunchKernelGGL(gather_labels_kernel, flat, dim3(EVAL_THREADS), 0, st, det_labels, perm_joint, D, L, key_a);
  if (int rc = os2d_launched("gather_labels_kernel")) return rc;
  int key_bits = label_bits;   // the largest key is L, not L - 1
  while (key_bits < 31 && ((u32)L >> key_bits) != 0) ++key_bits;
  const int passes = key_bits <= 8 ? 1 : (key_bits + 7) / 8;
  const u32* kin = key_a;
  const u32* iin = perm_joint;
  for (int p = 0; p < passes; ++p) {
    const bool last = p == passes - 1;
    u32* kout = last ? reinterpret_cast<u32*>(sorted_labels) : (kin == key_a ? key_b : key_a);
    u32* iout = last ? perm_class : (iin == idx_b ? idx_a : idx_b);
    if (int rc = radix_pass(kin, iin, kout, iout, D, 8 * p, hist, st)) return rc;
    kin = kout;
    iin = iout;
  }
  hipLaunchKernelGGL(class_offsets_kernel, dim3((L + 1 + EVAL_THREADS - 1) / EVAL_THREADS), dim3(EVAL_THREADS), 0, st, sorted_labels, D, L,
                     class_offsets);
  return os2d_launched("class_offsets_kernel");
}

}  // extern "C"
