// libos2d_train.so (include/os2d_train.h): target assignment and the OS2D training objective on gfx950, fp32.
//
//   os2d_train_assign_targets      reference box_coder.py encode (mode 0) / remap_anchor_targets (mode 1): one thread per
//                                  (image, label, anchor) walks the boxes of its image that carry its label.
//   os2d_train_assign_targets_ops  the same kernel body with a box transform chain on the anchors (hard-patch mining).
//   os2d_train_objective_forward   reference objective.py:141-277 as a short chain of launches (see the ABI function).
//   os2d_train_objective_backward  one kernel: d loc_preds, d cls_preds, d cls_preds_for_neg.
//
// Every launch uses the same decomposition: grid (chunks, A*B), 256 threads, one element per thread, so a work-group belongs to
// one (image, label) pair and element i = ab*HW + chunk*256 + tid.  Float sums are block partials (wave shuffles, then the four
// wave sums added in order) combined by ONE work-group in a fixed order; counts, histograms and per-label maxima are integer
// atomics, whose result does not depend on the order.  Two runs on the same input give the same bits.
//
// This unit is compiled with -ffp-contract=off (os2d_amd/build.py): the IoU and the box encoding are the reference's
// expressions operation for operation, and a fused multiply-add would round differently from the CPU reference.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "../../include/os2d_train.h"
#include "../csrc/detect_common.h"
#include "../csrc_shared/abi_common.h"

namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_WAVES = OBJ_THREADS / 64;

// flags byte of one element
constexpr unsigned char F_POS = 1;      // positive of the class loss (remapped targets when given)
constexpr unsigned char F_NEG = 2;      // negative that enters the class loss (after mining)
constexpr unsigned char F_POSREG = 4;   // positive of the localisation loss (original targets)
constexpr unsigned char F_CAND = 8;     // neither positive nor ignored: candidate negative
constexpr unsigned char F_HINGE = 16;   // the argument of the element's own clamp is >= 0: where torch's clamp passes the gradient

// workspace layout, in 4-byte words
constexpr int W_CNT = 0;      // unsigned counters: 0 num_pos, 1 num_pos_for_regression, 2 non-trivial positives, 3 candidates
constexpr int W_STATE = 16;   // floats: 0 max(num_pos,1), 1 max(num_pos_for_regression,1), 2 RLL positive scale
constexpr int W_HIST = 32;    // unsigned [4][256]: radix-select histograms, most significant byte first
constexpr int W_LABEL = W_HIST + 4 * 256;   // unsigned labelmax[B] (float bits), float labelnorm[B], then per-block arrays

struct Layout {
  int chunks, nblk;
  size_t lmax, lnorm, part, wpart, tie, total;
};
Layout layout(int A, int B, int HW) {
  Layout l;
  l.chunks = (HW + OBJ_THREADS - 1) / OBJ_THREADS;
  l.nblk = A * B * l.chunks;
  l.lmax = W_LABEL;
  l.lnorm = l.lmax + B;
  l.part = l.lnorm + B;                        // float [nblk][3]: loc, positive class, negative class sums
  l.wpart = l.part + (size_t)3 * l.nblk;       // float [nblk]: RLL weight sums
  l.tie = l.wpart + l.nblk;                    // unsigned [nblk]: elements equal to the mining threshold (then their prefix)
  l.total = l.tie + l.nblk;
  return l;
}

struct ObjParams {
  int kind, patch, B, HW, chunks, nblk;
  float margin, margin_pos, negw, locw, ratio, neglog;
  unsigned lmax, lnorm, part, wpart, tie;   // word offsets into the workspace
};

// ------------------------------------------------------------------------------------------------ block helpers
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// sum over the work-group, valid in thread 0; fixed order
template <class T>
__device__ __forceinline__ T block_sum(T v, T* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = sm[0];
#pragma unroll
  for (int w = 1; w < OBJ_WAVES; ++w) r += sm[w];
  return r;
}

// number of negatives the mining keeps: the reference's (neg_to_pos_ratio * num_pos).long() with the device's saturation
__device__ __forceinline__ long long mined_count(float ratio, unsigned num_pos) {
  const float kf = ratio * (float)num_pos;
  if (!(kf > 0.f)) return 0;   // also NaN = inf * 0
  if (kf >= 9.0e18f) return LLONG_MAX;
  return (long long)kf;
}

// Radix select state after `npass` histogram passes, by the whole work-group.  mode 0: no negative is taken, 1: every
// candidate, 2: the `krem` largest among the candidates whose top npass bytes equal `prefix` plus everything above them.
struct Select {
  int mode;
  unsigned prefix, krem;
};
__device__ Select resolve(const unsigned* ws, float ratio, int npass, unsigned* sm /* 256 + 3 */) {
  const long long k = mined_count(ratio, ws[W_CNT + 0]);
  const unsigned total = ws[W_CNT + 3];
  Select s;
  s.prefix = 0;
  s.krem = 0;
  s.mode = k <= 0 ? 0 : (k >= (long long)total ? 1 : 2);
  if (s.mode != 2) return s;
  unsigned krem = (unsigned)k, prefix = 0;
  for (int q = 0; q < npass; ++q) {
    __syncthreads();
    sm[threadIdx.x] = ws[W_HIST + q * 256 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned cum = 0;
      int b = 255;
      for (; b > 0; --b) {
        const unsigned c = sm[b];
        if (cum + c >= krem) break;
        cum += c;
      }
      sm[256] = krem - cum;
      sm[257] = (prefix << 8) | (unsigned)b;
    }
    __syncthreads();
    krem = sm[256];
    prefix = sm[257];
  }
  s.krem = krem;
  s.prefix = prefix;
  return s;
}

__device__ __forceinline__ float smooth_l1(float a, float b) {
  const float z = fabsf(a - b);
  return z < 1.f ? 0.5f * z * z : z - 0.5f;
}

// ------------------------------------------------------------------------------------------------ target assignment
__device__ __forceinline__ float box_iou(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1, float bx2,
                                         float by2, float area_b) {
  const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
  const float h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = w * h;
  return inter / (area_a + area_b - inter);
}

// torchvision's Matcher without low-quality matches, then the difficult flag
__device__ __forceinline__ int match_index(float best, int best_i, bool difficult, float high, float low) {
  int idx = best_i;
  if (best < low)
    idx = -1;
  else if (best < high)
    idx = -2;
  if (idx >= 0 && difficult) idx = -2;
  return idx;
}

// OPS: the anchor (mode 0), or the decoded box and the anchor (mode 1), go through the box-op chain `ops` before anything is
// compared (os2d_train_assign_targets_ops); without it the chain is never touched and the code is what it was.
template <bool OPS>
__global__ __launch_bounds__(OBJ_THREADS) void assign_targets_kernel(int mode, const float* __restrict__ gt_boxes,
                                                                    const int* __restrict__ gt_labels,
                                                                    const unsigned char* __restrict__ gt_difficult,
                                                                    const int* __restrict__ image_offsets, int num_boxes,
                                                                    const float* __restrict__ loc_scores, int B, int H, int W, float stride,
                                                                    float box_size, float high, float low, float* __restrict__ loc_targets,
                                                                    long long* __restrict__ cls_targets, float* __restrict__ ious_anchor,
                                                                    float* __restrict__ ious_corrected, Os2dBoxOps ops) {
  const int HW = H * W;
  const int p = blockIdx.x * OBJ_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int ab = blockIdx.y, a = ab / B, label = ab - a * B;
  const size_t i = (size_t)ab * HW + p;
  const size_t l0 = ((size_t)ab * 4) * HW + p;
  // the anchor, closed form (row-major cells, centre (x+0.5)*stride)
  const float cx = ((float)(p % W) + 0.5f) * stride, cy = ((float)(p / W) + 0.5f) * stride;
  float ax1 = cx - 0.5f * box_size, ay1 = cy - 0.5f * box_size, ax2 = cx + 0.5f * box_size, ay2 = cy + 0.5f * box_size;
  if constexpr (OPS) {
    if (mode == 0) {   // reference box_coder.py:352-354: the transformed anchors are matched, clipped and encoded
      const float4 t = os2d_apply_box_ops(make_float4(ax1, ay1, ax2, ay2), ops);
      ax1 = t.x, ay1 = t.y, ax2 = t.z, ay2 = t.w;
    }
  }
  float dx1 = 0.f, dy1 = 0.f, dx2 = 0.f, dy2 = 0.f, area_dec = 0.f;
  if (mode == 1) {   // BoxCoder.decode_single, weights (10, 10, 5, 5)
    const float clipv = 4.135166556742356f;   // log(1000 / 16)
    const float w = ax2 - ax1, h = ay2 - ay1;
    const float ccx = ax1 + 0.5f * w, ccy = ay1 + 0.5f * h;
    const float ddx = loc_scores[l0] / 10.f, ddy = loc_scores[l0 + HW] / 10.f;
    const float ddw = fminf(loc_scores[l0 + 2 * (size_t)HW] / 5.f, clipv), ddh = fminf(loc_scores[l0 + 3 * (size_t)HW] / 5.f, clipv);
    const float pcx = ddx * w + ccx, pcy = ddy * h + ccy;
    const float pw = expf(ddw) * w, ph = expf(ddh) * h;
    dx1 = pcx - 0.5f * pw;
    dy1 = pcy - 0.5f * ph;
    dx2 = pcx + 0.5f * pw;
    dy2 = pcy + 0.5f * ph;
    if constexpr (OPS) {   // reference box_coder.py:250-254: decoded against the plain anchor, then both through the chain
      const float4 d = os2d_apply_box_ops(make_float4(dx1, dy1, dx2, dy2), ops);
      dx1 = d.x, dy1 = d.y, dx2 = d.z, dy2 = d.w;
      const float4 t = os2d_apply_box_ops(make_float4(ax1, ay1, ax2, ay2), ops);
      ax1 = t.x, ay1 = t.y, ax2 = t.z, ay2 = t.w;
    }
    area_dec = (dx2 - dx1) * (dy2 - dy1);
  }
  const float area_anchor = (ax2 - ax1) * (ay2 - ay1);
  int lo = image_offsets[a], hi = image_offsets[a + 1];
  lo = max(0, min(lo, num_boxes));
  hi = max(lo, min(hi, num_boxes));
  float best_a = -1.f, best_d = -1.f;
  int bi_a = -1, bi_d = -1, first = -1;
  for (int j = lo; j < hi; ++j) {
    if (gt_labels[j] != label) continue;
    if (first < 0) first = j;
    const float gx1 = gt_boxes[4 * j], gy1 = gt_boxes[4 * j + 1], gx2 = gt_boxes[4 * j + 2], gy2 = gt_boxes[4 * j + 3];
    const float area_g = (gx2 - gx1) * (gy2 - gy1);
    const float ia = box_iou(gx1, gy1, gx2, gy2, area_g, ax1, ay1, ax2, ay2, area_anchor);
    if (ia > best_a || bi_a < 0) {   // first maximum
      best_a = ia;
      bi_a = j;
    }
    if (mode == 1) {
      const float id = box_iou(gx1, gy1, gx2, gy2, area_g, dx1, dy1, dx2, dy2, area_dec);
      if (id > best_d || bi_d < 0) {
        best_d = id;
        bi_d = j;
      }
    }
  }
  if (first < 0) {   // no box of this label in this image
    cls_targets[i] = 0;
    if (mode == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) loc_targets[l0 + (size_t)c * HW] = 0.f;
    } else {
      ious_anchor[i] = 0.f;
      ious_corrected[i] = 0.f;
    }
    return;
  }
  if (mode == 1) {
    const int idx = match_index(best_d, bi_d - first, gt_difficult[bi_d] != 0, high, low);
    cls_targets[i] = 1 + max(-2, min(idx, 0));
    ious_anchor[i] = best_a;
    ious_corrected[i] = best_d;
    return;
  }
  const int idx = match_index(best_a, bi_a, gt_difficult[bi_a] != 0, high, low);
  cls_targets[i] = 1 + max(-2, min(idx, 0));
  const int j = idx >= 0 ? idx : first;   // index.clamp(min=0): an unmatched anchor is encoded against the label's first box
  // clip_to_min_size(1) on both boxes, then encode_boxes with weights (10, 10, 5, 5)
  float gx1 = gt_boxes[4 * j], gy1 = gt_boxes[4 * j + 1], gx2 = gt_boxes[4 * j + 2], gy2 = gt_boxes[4 * j + 3];
  if (gx1 + 1.f > gx2) gx2 = gx1 + 1.f;
  if (gy1 + 1.f > gy2) gy2 = gy1 + 1.f;
  float px1 = ax1, py1 = ay1, px2 = ax2, py2 = ay2;
  if (px1 + 1.f > px2) px2 = px1 + 1.f;
  if (py1 + 1.f > py2) py2 = py1 + 1.f;
  const float ew = px2 - px1, eh = py2 - py1;
  const float ecx = px1 + 0.5f * ew, ecy = py1 + 0.5f * eh;
  const float gw = gx2 - gx1, gh = gy2 - gy1;
  const float gcx = gx1 + 0.5f * gw, gcy = gy1 + 0.5f * gh;
  loc_targets[l0] = 10.f * (gcx - ecx) / ew;
  loc_targets[l0 + HW] = 10.f * (gcy - ecy) / eh;
  loc_targets[l0 + 2 * (size_t)HW] = 5.f * logf(gw / ew);
  loc_targets[l0 + 3 * (size_t)HW] = 5.f * logf(gh / eh);
}

// ------------------------------------------------------------------------------------------------ objective forward
// Pass 1 over the elements: masks, half-margins, the localisation loss, counts, per-label maxima (RLL), the first radix
// histogram (contrastive).  What does not depend on a global quantity is final here.
__global__ __launch_bounds__(OBJ_THREADS) void objective_elements_kernel(ObjParams P, const float* __restrict__ loc_preds,
                                                                        const float* __restrict__ loc_targets,
                                                                        const float* __restrict__ cls_preds,
                                                                        const long long* __restrict__ cls_targets,
                                                                        const long long* __restrict__ cls_targets_remapped,
                                                                        const float* __restrict__ cls_preds_for_neg,
                                                                        float* __restrict__ cls_loss, float* __restrict__ loc_loss,
                                                                        unsigned char* __restrict__ flags, float* __restrict__ coef,
                                                                        unsigned* __restrict__ ws) {
  __shared__ unsigned hist[256];
  __shared__ float smf[OBJ_WAVES];
  __shared__ unsigned smu[OBJ_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid, ab = blockIdx.y;
  const int blk = ab * P.chunks + blockIdx.x;
  const bool valid = p < P.HW;
  const bool mining = P.kind == 0 && !P.patch;
  const bool rll_norm = P.kind == 1 && !P.patch;
  if (mining) hist[tid] = 0;
  unsigned npos = 0, nreg = 0, nnt = 0, ncand = 0;
  float locv = 0.f, posv = 0.f, negv = 0.f;
  if (mining) __syncthreads();
  if (valid) {
    const size_t i = (size_t)ab * P.HW + p;
    const long long t0 = cls_targets[i];
    const long long tr = cls_targets_remapped ? cls_targets_remapped[i] : t0;
    const bool preg = t0 > 0, pos = tr > 0, cand = !(pos || tr == -1);
    float x = cls_preds[i];
    if (cls_preds_for_neg) x = pos ? x : (cand ? cls_preds_for_neg[i] : 0.f);
    const float lneg = cand ? 0.5f * fmaxf(x - P.margin, 0.f) : 0.f;
    const float lpos = pos ? 0.5f * fmaxf(P.margin_pos - x, 0.f) : 0.f;
    // the reference's clamp(min=0) passes the gradient where its argument is exactly 0 as well: the RLL coefficients go by the
    // argument (>= 0), the count of non-trivial positives by the loss (> 0), as objective.py has them
    const bool hinge = pos ? P.margin_pos - x >= 0.f : (cand && x - P.margin >= 0.f);
    if (preg) {
      const size_t l0 = ((size_t)ab * 4) * P.HW + p;
      float s = smooth_l1(loc_preds[l0], loc_targets[l0]);
      s += smooth_l1(loc_preds[l0 + P.HW], loc_targets[l0 + P.HW]);
      s += smooth_l1(loc_preds[l0 + 2 * (size_t)P.HW], loc_targets[l0 + 2 * (size_t)P.HW]);
      s += smooth_l1(loc_preds[l0 + 3 * (size_t)P.HW], loc_targets[l0 + 3 * (size_t)P.HW]);
      locv = s;
    }
    if (loc_loss) loc_loss[i] = locv;
    unsigned char f = (pos ? F_POS : 0) | (preg ? F_POSREG : 0) | (cand ? F_CAND : 0) | (hinge ? F_HINGE : 0);
    npos = pos;
    nreg = preg;
    ncand = cand;
    if (rll_norm) {   // the per-element loss needs the per-label maxima: keep the half-margins for the later passes
      cls_loss[i] = lneg;
      coef[i] = lpos;
      nnt = pos && lpos > 0.f;
      if (lneg > 0.f) atomicMax(&ws[P.lmax + ab % P.B], __float_as_uint(lneg));
    } else {
      float cl, c;
      if (P.kind == 0) {
        cl = lneg * lneg + lpos * lpos;
        c = pos ? -lpos : lneg;
      } else {
        cl = lneg + lpos;
        c = hinge ? (pos ? -0.5f : 0.5f) : 0.f;
      }
      cls_loss[i] = cl;
      coef[i] = c;
      posv = pos ? cl : 0.f;
      if (P.patch) {
        if (cand) f |= F_NEG;
        negv = cand ? cl : 0.f;
      } else if (cand) {
        atomicAdd(&hist[__float_as_uint(cl) >> 24], 1u);
      }
    }
    flags[i] = f;
  }
  npos = block_sum(npos, smu);
  nreg = block_sum(nreg, smu);
  ncand = block_sum(ncand, smu);
  locv = block_sum(locv, smf);
  if (tid == 0) {
    if (npos) atomicAdd(&ws[W_CNT + 0], npos);
    if (nreg) atomicAdd(&ws[W_CNT + 1], nreg);
    if (ncand) atomicAdd(&ws[W_CNT + 3], ncand);
    reinterpret_cast<float*>(ws)[P.part + 3 * (size_t)blk] = locv;
  }
  if (rll_norm) {
    nnt = block_sum(nnt, smu);
    if (tid == 0 && nnt) atomicAdd(&ws[W_CNT + 2], nnt);
  } else {
    posv = block_sum(posv, smf);
    if (tid == 0) reinterpret_cast<float*>(ws)[P.part + 3 * (size_t)blk + 1] = posv;
    if (P.patch) {
      negv = block_sum(negv, smf);
      if (tid == 0) reinterpret_cast<float*>(ws)[P.part + 3 * (size_t)blk + 2] = negv;
    }
  }
  if (mining) {
    __syncthreads();
    if (hist[tid]) atomicAdd(&ws[W_HIST + tid], hist[tid]);
  }
}

// Radix-select pass 1..3: histogram of the next byte among the candidates that match the prefix found so far.
__global__ __launch_bounds__(OBJ_THREADS) void mining_histogram_kernel(ObjParams P, int pass, const float* __restrict__ cls_loss,
                                                                      const unsigned char* __restrict__ flags,
                                                                      unsigned* __restrict__ ws) {
  __shared__ unsigned sm[258];
  __shared__ unsigned hist[256];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid;
  const Select s = resolve(ws, P.ratio, pass, sm);
  if (s.mode != 2) return;
  hist[tid] = 0;
  __syncthreads();
  if (p < P.HW) {
    const size_t i = (size_t)blockIdx.y * P.HW + p;
    if (flags[i] & F_CAND) {
      const unsigned key = __float_as_uint(cls_loss[i]);
      if ((key >> (32 - 8 * pass)) == s.prefix) atomicAdd(&hist[(key >> (24 - 8 * pass)) & 255u], 1u);
    }
  }
  __syncthreads();
  if (hist[tid]) atomicAdd(&ws[W_HIST + pass * 256 + tid], hist[tid]);
}

// Elements of each work-group that EQUAL the k-th largest loss: they are taken in increasing flat index.
__global__ __launch_bounds__(OBJ_THREADS) void mining_ties_kernel(ObjParams P, const float* __restrict__ cls_loss,
                                                                 const unsigned char* __restrict__ flags, unsigned* __restrict__ ws) {
  __shared__ unsigned sm[258];
  __shared__ unsigned smu[OBJ_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid;
  const int blk = blockIdx.y * P.chunks + blockIdx.x;
  const Select s = resolve(ws, P.ratio, 4, sm);
  unsigned tie = 0;
  if (s.mode == 2 && p < P.HW) {
    const size_t i = (size_t)blockIdx.y * P.HW + p;
    tie = (flags[i] & F_CAND) && __float_as_uint(cls_loss[i]) == s.prefix;
  }
  tie = block_sum(tie, smu);
  if (tid == 0) ws[P.tie + blk] = tie;
}

// Exclusive prefix sum of the per-work-group tie counts, in place, by one work-group.
__global__ __launch_bounds__(OBJ_THREADS) void mining_scan_kernel(ObjParams P, unsigned* __restrict__ ws) {
  __shared__ unsigned sums[OBJ_THREADS];
  const int tid = threadIdx.x;
  const int per = (P.nblk + OBJ_THREADS - 1) / OBJ_THREADS;
  const int b0 = min(tid * per, P.nblk), b1 = min(b0 + per, P.nblk);
  unsigned* tie = ws + P.tie;
  unsigned s = 0;
  for (int b = b0; b < b1; ++b) s += tie[b];
  sums[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned run = 0;
    for (int t = 0; t < OBJ_THREADS; ++t) {
      const unsigned v = sums[t];
      sums[t] = run;
      run += v;
    }
  }
  __syncthreads();
  unsigned run = sums[tid];
  for (int b = b0; b < b1; ++b) {
    const unsigned v = tie[b];
    tie[b] = run;
    run += v;
  }
}

// The mined negatives: everything above the k-th largest loss, and the first `krem` elements equal to it.
__global__ __launch_bounds__(OBJ_THREADS) void mining_select_kernel(ObjParams P, const float* __restrict__ cls_loss,
                                                                   unsigned char* __restrict__ flags, unsigned* __restrict__ ws) {
  __shared__ unsigned sm[258];
  __shared__ unsigned wcount[OBJ_WAVES];
  __shared__ float smf[OBJ_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid;
  const int blk = blockIdx.y * P.chunks + blockIdx.x;
  const Select s = resolve(ws, P.ratio, 4, sm);
  const bool valid = p < P.HW;
  const size_t i = (size_t)blockIdx.y * P.HW + p;
  unsigned char f = valid ? flags[i] : 0;
  const float cl = valid ? cls_loss[i] : 0.f;
  const bool cand = (f & F_CAND) != 0;
  bool sel = false;
  if (s.mode == 1) sel = cand;
  if (s.mode == 2) {   // uniform branch: the barriers below are reached by the whole work-group
    const unsigned key = __float_as_uint(cl);
    const bool tie = cand && key == s.prefix;
    const unsigned long long ballot = __ballot(tie);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wcount[wv] = (unsigned)__popcll(ballot);
    __syncthreads();
    unsigned rank = ws[P.tie + blk] + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) rank += wcount[w];
    sel = cand && (key > s.prefix || (tie && rank < s.krem));
  }
  if (valid && sel) flags[i] = f | F_NEG;
  const float negv = block_sum(sel ? cl : 0.f, smf);
  if (tid == 0) reinterpret_cast<float*>(ws)[P.part + 3 * (size_t)blk + 2] = negv;
}

// RLL: the unnormalised weight exp((l - max_l) * T) of one negative, T = -log(ratio) / max_l of its label
__device__ __forceinline__ float rll_weight(float lneg, float maxl, float neglog) {
  const float T = neglog / maxl;
  return expf((lneg - maxl) * T);
}

__global__ __launch_bounds__(OBJ_THREADS) void rll_weight_sums_kernel(ObjParams P, const float* __restrict__ cls_loss,
                                                                     const unsigned char* __restrict__ flags,
                                                                     unsigned* __restrict__ ws) {
  __shared__ float smf[OBJ_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid, ab = blockIdx.y;
  const int blk = ab * P.chunks + blockIdx.x;
  const float maxl = __uint_as_float(ws[P.lmax + ab % P.B]);
  float w = 0.f;
  if (p < P.HW && maxl > 1e-5f) {
    const size_t i = (size_t)ab * P.HW + p;
    const float lneg = cls_loss[i];
    if ((flags[i] & F_CAND) && lneg > 0.f) w = rll_weight(lneg, maxl, P.neglog);
  }
  w = block_sum(w, smf);
  if (tid == 0) reinterpret_cast<float*>(ws)[P.wpart + blk] = w;
}

// One work-group: per-label normalisation of the RLL weights and the scale of the positives.
__global__ __launch_bounds__(OBJ_THREADS) void rll_normalise_kernel(ObjParams P, int A, unsigned* __restrict__ ws) {
  __shared__ unsigned smu[OBJ_WAVES];
  __shared__ unsigned nlab_s;
  const int tid = threadIdx.x;
  float* wsf = reinterpret_cast<float*>(ws);
  unsigned mine = 0;
  for (int b = tid; b < P.B; b += OBJ_THREADS) mine += __uint_as_float(ws[P.lmax + b]) > 1e-5f;
  mine = block_sum(mine, smu);
  if (tid == 0) nlab_s = mine;
  __syncthreads();
  const float nlab = (float)nlab_s;
  for (int b = tid; b < P.B; b += OBJ_THREADS) {
    float sum = 0.f;
    for (int a = 0; a < A; ++a)
      for (int c = 0; c < P.chunks; ++c) sum += wsf[P.wpart + ((size_t)a * P.B + b) * P.chunks + c];
    float norm = 1.f / (sum * nlab);
    if (norm <= 1e-8f || !(__uint_as_float(ws[P.lmax + b]) > 1e-5f)) norm = 0.f;
    wsf[P.lnorm + b] = norm;
  }
  if (tid == 0) {
    const unsigned np = ws[W_CNT + 0], nnt = ws[W_CNT + 2];
    wsf[W_STATE + 2] = nnt > 0 ? (float)np / (float)nnt : 0.f;
  }
}

__global__ __launch_bounds__(OBJ_THREADS) void rll_elements_kernel(ObjParams P, float* __restrict__ cls_loss,
                                                                  unsigned char* __restrict__ flags, float* __restrict__ coef,
                                                                  unsigned* __restrict__ ws) {
  __shared__ float smf[OBJ_WAVES];
  const int tid = threadIdx.x, p = blockIdx.x * OBJ_THREADS + tid, ab = blockIdx.y;
  const int blk = ab * P.chunks + blockIdx.x;
  float* wsf = reinterpret_cast<float*>(ws);
  const unsigned np = ws[W_CNT + 0];
  const float np1 = (float)(np > 0 ? np : 1u);
  const bool take_negs = mined_count(P.ratio, np) > 0;   // RLL does not mine: all negatives, or none without a positive
  const float pos_scale = wsf[W_STATE + 2];
  const float maxl = __uint_as_float(ws[P.lmax + ab % P.B]);
  const float norm = wsf[P.lnorm + ab % P.B];
  float posv = 0.f, negv = 0.f;
  if (p < P.HW) {
    const size_t i = (size_t)ab * P.HW + p;
    const float lneg = cls_loss[i], lpos = coef[i];
    unsigned char f = flags[i];
    const bool pos = (f & F_POS) != 0, cand = (f & F_CAND) != 0;
    float w = 0.f;
    if (cand && lneg > 0.f && maxl > 1e-5f) w = rll_weight(lneg, maxl, P.neglog) * norm;
    w = w * np1;
    const bool wm = w > 1e-8f;
    const float ln = (wm ? lneg : 0.f) * w;
    const float lp = lpos * pos_scale;
    const float cl = (cand ? ln : 0.f) + (pos ? lp : 0.f);
    cls_loss[i] = cl;
    coef[i] = pos ? ((f & F_HINGE) ? -0.5f * pos_scale : 0.f) : (wm ? 0.5f * w : 0.f);
    if (cand && take_negs) {
      f |= F_NEG;
      negv = cl;
    }
    flags[i] = f;
    posv = pos ? cl : 0.f;
  }
  posv = block_sum(posv, smf);
  negv = block_sum(negv, smf);
  if (tid == 0) {
    wsf[P.part + 3 * (size_t)blk + 1] = posv;
    wsf[P.part + 3 * (size_t)blk + 2] = negv;
  }
}

// One work-group: the block partials in a fixed order, then the five scalars.
__global__ __launch_bounds__(OBJ_THREADS) void objective_finalise_kernel(ObjParams P, float* __restrict__ losses,
                                                                        unsigned* __restrict__ ws) {
  __shared__ float smf[OBJ_WAVES];
  const int tid = threadIdx.x;
  float* wsf = reinterpret_cast<float*>(ws);
  float sums[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float s = 0.f;
    for (int b = tid; b < P.nblk; b += OBJ_THREADS) s += wsf[P.part + 3 * (size_t)b + q];
    sums[q] = block_sum(s, smf);
  }
  if (tid == 0) {
    const unsigned np = ws[W_CNT + 0], npr = ws[W_CNT + 1];
    const float np1 = (float)(np > 0 ? np : 1u), npr1 = (float)(npr > 0 ? npr : 1u);
    const float loc = sums[0] / npr1, cls_pos = sums[1] / np1, cls_neg = sums[2] / np1;
    const float cls = cls_pos + cls_neg * P.negw;
    losses[0] = cls + loc * P.locw;
    losses[1] = loc;
    losses[2] = cls;
    losses[3] = cls_pos;
    losses[4] = cls_neg;
    wsf[W_STATE + 0] = np1;
    wsf[W_STATE + 1] = npr1;
  }
}

// ------------------------------------------------------------------------------------------------ objective backward
__global__ __launch_bounds__(OBJ_THREADS) void objective_backward_kernel(const float* __restrict__ grad_loss,
                                                                        const float* __restrict__ loc_preds,
                                                                        const float* __restrict__ loc_targets,
                                                                        const unsigned char* __restrict__ flags,
                                                                        const float* __restrict__ coef, const float* __restrict__ wsf,
                                                                        int HW, float negw, float locw, float* __restrict__ dloc,
                                                                        float* __restrict__ dcls, float* __restrict__ dcls_neg) {
  const int p = blockIdx.x * OBJ_THREADS + threadIdx.x, ab = blockIdx.y;
  if (p >= HW) return;
  const size_t i = (size_t)ab * HW + p;
  const float g = grad_loss[0];
  const float np1 = wsf[W_STATE + 0], npr1 = wsf[W_STATE + 1];
  const unsigned char f = flags[i];
  if (dloc) {
    const size_t l0 = ((size_t)ab * 4) * HW + p;
    const float scale = g * locw / npr1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t l = l0 + (size_t)c * HW;
      float d = 0.f;
      if (f & F_POSREG) d = scale * fminf(fmaxf(loc_preds[l] - loc_targets[l], -1.f), 1.f);
      dloc[l] = d;
    }
  }
  const float c = coef[i];
  const float dpos = (f & F_POS) ? g * c / np1 : 0.f;
  const float dneg = (f & F_NEG) ? g * negw * c / np1 : 0.f;
  if (dcls_neg) {
    dcls_neg[i] = dneg;
    if (dcls) dcls[i] = dpos;
  } else if (dcls) {
    dcls[i] = dpos + dneg;   // an element is never both
  }
}

bool dims_ok(int A, int B, int HW) {
  return A >= 1 && B >= 1 && HW >= 1 && (long long)A * B <= 65535 && (long long)A * B * HW <= (1ll << 28);
}

// both entry points: `ops` NULL = the plain anchors (os2d_train_assign_targets)
int assign_targets(const char* what, int mode, const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult,
                   const int* image_offsets, int num_boxes, const float* loc_scores, int A, int B, int H, int W, int stride, int rec_field,
                   float iou_high, float iou_low, const Os2dBoxOps* ops, float* loc_targets, long long* cls_targets, float* ious_anchor,
                   float* ious_anchor_corrected, void* stream) {
  if (mode != 0 && mode != 1) {
    os2d_set_error("%s: unknown mode %d (0 = encode, 1 = remap)", what, mode);
    return -1;
  }
  if (H < 1 || W < 1 || (long long)H * W > (1ll << 28) || !dims_ok(A, B, H * W)) {
    os2d_set_error("%s: bad shape A=%d B=%d H=%d W=%d", what, A, B, H, W);
    return -1;
  }
  if (stride < 1 || rec_field + 14 * stride < 1 || num_boxes < 0) {
    os2d_set_error("%s: bad stride=%d rec_field=%d num_boxes=%d", what, stride, rec_field, num_boxes);
    return -1;
  }
  if (!image_offsets || !cls_targets || (num_boxes > 0 && (!gt_boxes || !gt_labels || !gt_difficult))) {
    os2d_set_error("%s: null pointer", what);
    return -1;
  }
  if (mode == 0 ? !loc_targets : (!loc_scores || !ious_anchor || !ious_anchor_corrected)) {
    os2d_set_error("%s: null pointer for mode %d", what, mode);
    return -1;
  }
  const int HW = H * W;
  const dim3 grid((HW + OBJ_THREADS - 1) / OBJ_THREADS, A * B);
  const float fs = (float)stride, box = (float)(rec_field + 14 * stride);
  if (ops)
    assign_targets_kernel<true><<<grid, OBJ_THREADS, 0, os2d_stream(stream)>>>(mode, gt_boxes, gt_labels, gt_difficult, image_offsets, num_boxes,
                                                                    loc_scores, B, H, W, fs, box, iou_high, iou_low, loc_targets,
                                                                    cls_targets, ious_anchor, ious_anchor_corrected, *ops);
  else
    assign_targets_kernel<false><<<grid, OBJ_THREADS, 0, os2d_stream(stream)>>>(mode, gt_boxes, gt_labels, gt_difficult, image_offsets, num_boxes,
                                                                     loc_scores, B, H, W, fs, box, iou_high, iou_low, loc_targets,
                                                                     cls_targets, ious_anchor, ious_anchor_corrected, Os2dBoxOps{});
  return os2d_launched(what);
}
}  // namespace

extern "C" {

int os2d_train_assign_targets(int mode, const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult,
                              const int* image_offsets, int num_boxes, const float* loc_scores, int A, int B, int H, int W, int stride,
                              int rec_field, float iou_high, float iou_low, float* loc_targets, long long* cls_targets,
                              float* ious_anchor, float* ious_anchor_corrected, void* stream) {
  return assign_targets("os2d_train_assign_targets", mode, gt_boxes, gt_labels, gt_difficult, image_offsets, num_boxes, loc_scores, A, B, H, W,
                        stride, rec_field, iou_high, iou_low, nullptr, loc_targets, cls_targets, ious_anchor, ious_anchor_corrected, stream);
}

int os2d_train_assign_targets_ops(int mode, const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult,
                                  const int* image_offsets, int num_boxes, const float* loc_scores, int A, int B, int H, int W, int stride,
                                  int rec_field, float iou_high, float iou_low, int nops, const int* op_kinds, const float* op_args,
                                  float* loc_targets, long long* cls_targets, float* ious_anchor, float* ious_anchor_corrected,
                                  void* stream) {
  Os2dBoxOps ops;
  if (!os2d_box_ops_from(op_kinds, op_args, nops, &ops)) {
    os2d_set_error("os2d_train_assign_targets_ops: bad box-op chain (nops=%d, at most %d ops of kind 1..4)", nops, OS2D_BOX_MAX_OPS);
    return -1;
  }
  return assign_targets("os2d_train_assign_targets_ops", mode, gt_boxes, gt_labels, gt_difficult, image_offsets, num_boxes, loc_scores, A, B, H,
                        W, stride, rec_field, iou_high, iou_low, &ops, loc_targets, cls_targets, ious_anchor, ious_anchor_corrected, stream);
}

size_t os2d_train_objective_workspace_floats(int A, int B, int HW) {
  if (!dims_ok(A, B, HW)) return 0;
  return layout(A, B, HW).total;
}

int os2d_train_objective_forward(int class_loss, int patch_mining_mode, const float* loc_preds, const float* loc_targets,
                                 const float* cls_preds, const long long* cls_targets, const long long* cls_targets_remapped,
                                 const float* cls_preds_for_neg, int A, int B, int HW, float margin, float margin_pos,
                                 float class_loss_neg_weight, float localization_weight, float neg_to_pos_ratio,
                                 double rll_neg_weight_ratio, float* losses, float* cls_loss, float* loc_loss, unsigned char* flags,
                                 float* coef, float* workspace, size_t workspace_floats, void* stream) {
  if (class_loss != 0 && class_loss != 1) {
    os2d_set_error("os2d_train_objective_forward: unknown class loss %d (0 = ContrastiveLoss, 1 = RLL)", class_loss);
    return -1;
  }
  if (!dims_ok(A, B, HW)) {
    os2d_set_error("os2d_train_objective_forward: bad shape A=%d B=%d HW=%d", A, B, HW);
    return -1;
  }
  if (!loc_preds || !loc_targets || !cls_preds || !cls_targets || !losses || !cls_loss || !flags || !coef || !workspace) {
    os2d_set_error("os2d_train_objective_forward: null pointer");
    return -1;
  }
  if (class_loss == 1 && !(rll_neg_weight_ratio > 0.0)) {
    os2d_set_error("os2d_train_objective_forward: rll_neg_weight_ratio must be positive");
    return -1;
  }
  if (!(neg_to_pos_ratio >= 0.f)) {
    os2d_set_error("os2d_train_objective_forward: neg_to_pos_ratio must not be negative");
    return -1;
  }
  const Layout l = layout(A, B, HW);
  if (workspace_floats < l.total) {
    os2d_set_error("os2d_train_objective_forward: workspace of %zu floats, %zu needed", workspace_floats, l.total);
    return -2;
  }
  ObjParams P;
  P.kind = class_loss;
  P.patch = patch_mining_mode ? 1 : 0;
  P.B = B;
  P.HW = HW;
  P.chunks = l.chunks;
  P.nblk = l.nblk;
  P.margin = margin;
  P.margin_pos = margin_pos;
  P.negw = class_loss_neg_weight;
  P.locw = localization_weight;
  P.ratio = neg_to_pos_ratio;
  P.neglog = class_loss == 1 ? (float)(-log(rll_neg_weight_ratio)) : 0.f;
  P.lmax = (unsigned)l.lmax;
  P.lnorm = (unsigned)l.lnorm;
  P.part = (unsigned)l.part;
  P.wpart = (unsigned)l.wpart;
  P.tie = (unsigned)l.tie;
  hipStream_t s = os2d_stream(stream);
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  const dim3 grid(l.chunks, A * B);
  if (hipMemsetAsync(ws, 0, l.part * sizeof(unsigned), s) != hipSuccess) return os2d_launched("os2d_train_objective_forward: memset");
  objective_elements_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, loc_preds, loc_targets, cls_preds, cls_targets, cls_targets_remapped,
                                                        cls_preds_for_neg, cls_loss, loc_loss, flags, coef, ws);
  if (!P.patch && P.kind == 0) {
    for (int pass = 1; pass < 4; ++pass) mining_histogram_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, pass, cls_loss, flags, ws);
    mining_ties_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, cls_loss, flags, ws);
    mining_scan_kernel<<<1, OBJ_THREADS, 0, s>>>(P, ws);
    mining_select_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, cls_loss, flags, ws);
  } else if (!P.patch) {
    rll_weight_sums_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, cls_loss, flags, ws);
    rll_normalise_kernel<<<1, OBJ_THREADS, 0, s>>>(P, A, ws);
    rll_elements_kernel<<<grid, OBJ_THREADS, 0, s>>>(P, cls_loss, flags, coef, ws);
  }
  objective_finalise_kernel<<<1, OBJ_THREADS, 0, s>>>(P, losses, ws);
  return os2d_launched("os2d_train_objective_forward");
}

int os2d_train_objective_backward(const float* grad_loss, const float* loc_preds, const float* loc_targets, const unsigned char* flags,
                                  const float* coef, const float* workspace, int A, int B, int HW, float class_loss_neg_weight,
                                  float localization_weight, float* dloc_preds, float* dcls_preds, float* dcls_preds_for_neg,
                                  void* stream) {
  if (!dims_ok(A, B, HW)) {
    os2d_set_error("os2d_train_objective_backward: bad shape A=%d B=%d HW=%d", A, B, HW);
    return -1;
  }
  if (!grad_loss || !flags || !coef || !workspace || (dloc_preds && (!loc_preds || !loc_targets))) {
    os2d_set_error("os2d_train_objective_backward: null pointer");
    return -1;
  }
  if (!dloc_preds && !dcls_preds && !dcls_preds_for_neg) {
    os2d_set_error("os2d_train_objective_backward: null pointer for every gradient");
    return -1;
  }
  const dim3 grid((HW + OBJ_THREADS - 1) / OBJ_THREADS, A * B);
  objective_backward_kernel<<<grid, OBJ_THREADS, 0, os2d_stream(stream)>>>(grad_loss, loc_preds, loc_targets, flags, coef, workspace, HW,
                                                                class_loss_neg_weight, localization_weight, dloc_preds, dcls_preds,
                                                                dcls_preds_for_neg);
  return os2d_launched("os2d_train_objective_backward");
}

}  // extern "C"
