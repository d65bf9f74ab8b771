// VOC evaluation, step 1 (gfx950): every detection against the ground truth of its image (the per-image, per-label loop of
// reference os2d/data/voc_eval.py:81-140, restated order-free).
//
//   count_gt_kernel   n_pos[l] = ground-truth boxes of label l that are not difficult (slot L: all labels), gt_count[l] = all
//   match_kernel      one thread per detection: IoU with every ground-truth box of its label in its image (+1 on xmax / ymax of
//                     both, fp32, every operation rounded on its own: the unit is compiled with -ffp-contract=off), FIRST
//                     argmax, -1 below the threshold; then a 64-bit atomicMin of (score key << 32 | index in image) into the
//                     word of that box: the minimum is the detection the reference's in-order loop reaches first
//   resolve_kernel    match = -1 (difficult box), 1 (the winner of its box), 0 (a later one, or no box)
//
// Only integer atomics: two runs give the same bits.
#include "../../include/os2d_eval.h"
#include "../csrc/detect_common.h"
#include "eval_common.h"

namespace {

__global__ __launch_bounds__(EVAL_THREADS) void count_gt_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ difficult,
                                                                 int G, int L, int* __restrict__ n_pos, int* __restrict__ gt_count) {
  const int g = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (g >= G) return;
  const int l = labels[g];
  if ((unsigned)l >= (unsigned)L) return;
  atomicAdd(&gt_count[l], 1);
  if (!difficult[g]) {
    atomicAdd(&n_pos[l], 1);
    atomicAdd(&n_pos[L], 1);
  }
}

// image of packed row d: the n < N with offsets[n] <= d < offsets[n + 1] (images without rows repeat an offset)
__device__ __forceinline__ int image_of(const int* __restrict__ offsets, int N, int d) {
  int lo = 0, hi = N;   // first n in [0, N] with offsets[n] > d, minus one
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] > d) hi = mid;
    else lo = mid + 1;
  }
  return lo > 0 ? lo - 1 : 0;
}

__device__ __forceinline__ u64 winner_key(float score, int index_in_image) {
  return ((u64)os2d_score_key(score) << 32) | (u64)(u32)index_in_image;
}

__global__ __launch_bounds__(EVAL_THREADS) void match_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                              const int* __restrict__ labels, const int* __restrict__ det_offsets, int D,
                                                              int N, const float4* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                              const int* __restrict__ gt_offsets, float thr, int* __restrict__ gt_index,
                                                              u64* __restrict__ winner) {
  const int d = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (d >= D) return;
  const int img = image_of(det_offsets, N, d);
  const int label = labels[d];
  float4 a = boxes[d];
  a.z = a.z + 1.f;
  a.w = a.w + 1.f;
  const float area_a = (a.z - a.x) * (a.w - a.y);
  float best = -1.f;
  int arg = -1;
  const int g1 = gt_offsets[img + 1];
  for (int g = gt_offsets[img]; g < g1; ++g) {
    if (gt_labels[g] != label) continue;
    float4 b = gt_boxes[g];
    b.z = b.z + 1.f;
    b.w = b.w + 1.f;
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
    const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = w * h;
    const float iou = inter / (area_a + area_b - inter);
    if (iou > best) {   // strict: the first of equal maxima stays
      best = iou;
      arg = g;
    }
  }
  if (best < thr) arg = -1;
  gt_index[d] = arg;
  if (arg >= 0) atomicMin(&winner[arg], winner_key(scores[d], d - det_offsets[img]));
}

__global__ __launch_bounds__(EVAL_THREADS) void resolve_kernel(const float* __restrict__ scores, const int* __restrict__ det_offsets, int D, int N,
                                                                const unsigned char* __restrict__ difficult, const int* __restrict__ gt_index,
                                                                const u64* __restrict__ winner, signed char* __restrict__ match) {
  const int d = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (d >= D) return;
  const int g = gt_index[d];
  signed char m = 0;
  if (g >= 0) {
    if (difficult[g]) m = -1;
    else m = winner[g] == winner_key(scores[d], d - det_offsets[image_of(det_offsets, N, d)]) ? 1 : 0;
  }
  match[d] = m;
}

}  // namespace

extern "C" {

int os2d_eval_abi_version(void) { return OS2D_EVAL_ABI_VERSION; }
const char* os2d_eval_last_error(void) { return os2d_error_text; }

int os2d_eval_count_gt(const int* gt_labels, const unsigned char* gt_difficult, int G, int L, int* n_pos, int* gt_count, void* stream) {
  if (G < 0 || L < 1) return os2d_refuse("count_gt: bad shape (G >= 0, L >= 1)");
  if (!n_pos || !gt_count || (G > 0 && (!gt_labels || !gt_difficult))) return os2d_refuse("count_gt: null pointer");
  if (hipMemsetAsync(n_pos, 0, sizeof(int) * ((size_t)L + 1), os2d_stream(stream)) != hipSuccess ||
      hipMemsetAsync(gt_count, 0, sizeof(int) * (size_t)L, os2d_stream(stream)) != hipSuccess)
    return os2d_launched("count_gt: memset");
  if (G == 0) return 0;
  hipLaunchKernelGGL(count_gt_kernel, dim3((G + EVAL_THREADS - 1) / EVAL_THREADS), dim3(EVAL_THREADS), 0, os2d_stream(stream), gt_labels, gt_difficult,
                     G, L, n_pos, gt_count);
  return os2d_launched("count_gt_kernel");
}

int os2d_eval_match(const float* det_boxes, const float* det_scores, const int* det_labels, const int* det_offsets, int D, int N,
                    const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult, const int* gt_offsets, int G,
                    float iou_thresh, int* gt_index, unsigned long long* winner, signed char* match, void* stream) {
  if (D < 0 || G < 0 || N < 1) return os2d_refuse("match: bad shape (D >= 0, G >= 0, N >= 1)");
  if (!det_offsets || !gt_offsets) return os2d_refuse("match: null pointer (offsets)");
  if (D == 0) return 0;
  if (!det_boxes || !det_scores || !det_labels || !gt_index || !match) return os2d_refuse("match: null pointer (detections)");
  if (G > 0 && (!gt_boxes || !gt_labels || !gt_difficult || !winner)) return os2d_refuse("match: null pointer (ground truth)");
  if (((size_t)det_boxes | (size_t)gt_boxes) & 15) return os2d_refuse("match: boxes must be 16-byte aligned");
  if (G > 0 && hipMemsetAsync(winner, 0xff, sizeof(u64) * (size_t)G, os2d_stream(stream)) != hipSuccess) return os2d_launched("match: memset");
  const dim3 grid((D + EVAL_THREADS - 1) / EVAL_THREADS);
  hipLaunchKernelGGL(match_kernel, grid, dim3(EVAL_THREADS), 0, os2d_stream(stream), reinterpret_cast<const float4*>(det_boxes), det_scores, det_labels,
                     det_offsets, D, N, reinterpret_cast<const float4*>(gt_boxes), gt_labels, gt_offsets, iou_thresh, gt_index, winner);
  if (int rc = os2d_launched("match_kernel")) return rc;
  hipLaunchKernelGGL(resolve_kernel, grid, dim3(EVAL_THREADS), 0, os2d_stream(stream), det_scores, det_offsets, D, N, gt_difficult, gt_index, winner,
                     match);
  return os2d_launched("resolve_kernel");
}

}  // extern "C"
