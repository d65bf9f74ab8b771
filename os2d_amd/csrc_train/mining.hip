// libos2d_train.so (include/os2d_train.h): hard-patch mining on gfx950 (reference os2d/engine/train.py:240-325).
//
//   os2d_train_crop_boxes    reference box_coder.py:78-166 for one level: the crop window and the anchor box of every anchor.
//   os2d_train_mine_select   per (image, role) the first K survivors of a greedy NMS over the crop windows of the flagged
//                            (level, label, anchor) candidates, in order of decreasing score.
//
// Greedy NMS emits its survivors in score order, so "NMS, sort, take K" is K rounds of "take the best candidate still alive,
// kill what overlaps it": O(N * K), no sort, no N x N mask.  One work-group of 1024 threads owns one (image, role).  Its slice
// of the workspace holds one dead byte per candidate and the crop window of every anchor of every level (a table of sum HW_l
// boxes, not of N = B * sum HW_l: the window is a closed form of (level, anchor), mining_crop.h).  Round r kills against the
// box kept in round r - 1 and reduces the arg-max of what is alive: a 64-bit key (score key, flat index) is min-reduced in
// the waves (shuffles) and across them (LDS), so equal scores (-0 == +0 included) go to the smaller flat index - the
// (level, label, anchor) order in which the reference concatenates its candidates.  A thread reads only the dead bytes it
// wrote itself.  No atomics, no cooperative launch; two runs give the same bits.
//
// Candidates whose score is not finite are never selected (the reference's behaviour there is not defined: its NMS keeps
// +inf, drops -inf and NaN, and sorts NaN wherever the sort leaves it).
//
// Decisions are made with os2d_apply_box_ops, os2d_box_area and os2d_iou_gt of csrc/detect_common.h (contraction off): they
// have the bits of the reference's tensor expressions.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/os2d_train.h"
#include "../csrc_shared/abi_common.h"
#include "mining_crop.h"

namespace {

constexpr int MINE_THREADS = 1024;
constexpr int MINE_WAVES = MINE_THREADS / 64;
constexpr int MINE_INDEX = 3;     // ints of a record: level, label, anchor
constexpr int MINE_VALUES = 19;   // floats of a record: crop 4, anchor 4, corners 8, cls_loss, loc_loss, cls_pred
constexpr unsigned long long NONE = ~0ull;

struct MineLevel {
  const float* cls_loss;
  const float* loc_loss;
  const unsigned char* flags;
  const float* cls_preds;
  const float* corners;   // may be null
  int HW, row_stride;     // anchors; elements between two (image, label) rows of cls_loss / loc_loss / flags
  int cand_offset;        // flat index of (label 0, anchor 0) of this level
  int table_offset;       // first box of this level in the crop table
  Os2dCropGeometry geom;
  Os2dBoxOps ops;
};

struct MineParams {
  MineLevel lv[OS2D_MINE_MAX_LEVELS];
  int L, B, K, N;
  float iou_thr;
  size_t table_bytes_offset, slice_bytes;   // workspace slice of one work-group: dead [N], then the crop table
};

__global__ __launch_bounds__(256) void crop_boxes_kernel(int HW, Os2dCropGeometry g, Os2dBoxOps ops, float4* __restrict__ crops,
                                                         float4* __restrict__ anchors) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float4 c, a;
  os2d_mine_crop_box(p, g, ops, &c, &a);
  crops[p] = c;
  anchors[p] = a;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    v = other < v ? other : v;
  }
  return v;
}

__global__ __launch_bounds__(MINE_THREADS) void mine_select_kernel(MineParams P, int* __restrict__ out_count, int* __restrict__ out_index,
                                                                  float* __restrict__ out_values, unsigned char* __restrict__ ws) {
  const int tid = threadIdx.x;
  const int a = blockIdx.x / 3, role = blockIdx.x - a * 3;
  const unsigned char want = role == 0 ? 2 : (role == 1 ? 1 : 4);   // neg, pos, pos_loc: flags of os2d_train_objective_forward
  unsigned char* dead = ws + (size_t)blockIdx.x * P.slice_bytes;
  float4* table = reinterpret_cast<float4*>(dead + P.table_bytes_offset);
  __shared__ unsigned long long s_wave[MINE_WAVES];

  for (int l = 0; l < P.L; ++l) {
    const MineLevel& lv = P.lv[l];
    for (int p = tid; p < lv.HW; p += MINE_THREADS) {
      float4 c, anchor;
      os2d_mine_crop_box(p, lv.geom, lv.ops, &c, &anchor);
      table[lv.table_offset + p] = c;
    }
  }
  __syncthreads();

  int* my_index = out_index + (size_t)blockIdx.x * P.K * MINE_INDEX;
  float* my_values = out_values + (size_t)blockIdx.x * P.K * MINE_VALUES;
  float4 kept = make_float4(0.f, 0.f, 0.f, 0.f);
  float kept_area = 0.f;
  int kept_flat = -1, count = 0;
  for (int r = 0; r < P.K; ++r) {
    unsigned long long best = NONE;
    for (int l = 0; l < P.L; ++l) {
      const MineLevel& lv = P.lv[l];
      const float* __restrict__ score = role == 2 ? lv.loc_loss : lv.cls_loss;
      const int n = P.B * lv.HW;
      for (int idx = tid; idx < n; idx += MINE_THREADS) {
        const int flat = lv.cand_offset + idx;
        const int label = idx / lv.HW, p = idx - label * lv.HW;
        const size_t e = ((size_t)a * P.B + label) * lv.row_stride + p;
        bool alive;
        float s = 0.f;
        if (r == 0) {
          alive = (lv.flags[e] & want) != 0;
          if (alive) {
            s = score[e];
            alive = isfinite(s);
          }
          dead[flat] = alive ? 0 : 1;
        } else {
          alive = dead[flat] == 0;
          if (alive) {
            const float4 c = table[lv.table_offset + p];
            if (flat == kept_flat || os2d_iou_gt(kept, kept_area, c, os2d_box_area(c), P.iou_thr)) {
              alive = false;
              dead[flat] = 1;
            } else {
              s = score[e];
            }
          }
        }
        if (alive) {
          const unsigned long long key = ((unsigned long long)os2d_score_key(s) << 32) | (unsigned)flat;
          best = key < best ? key : best;
        }
      }
    }
    best = wave_min(best);
    __syncthreads();   // the previous round's reads of s_wave are done
    if ((tid & 63) == 0) s_wave[tid >> 6] = best;
    __syncthreads();
    best = s_wave[0];
#pragma unroll
    for (int w = 1; w < MINE_WAVES; ++w) best = s_wave[w] < best ? s_wave[w] : best;
    if (best == NONE) break;   // nothing alive: the same in every thread
    kept_flat = (int)(unsigned)(best & 0xffffffffull);
    int l = 0;
    while (l + 1 < P.L && kept_flat >= P.lv[l + 1].cand_offset) ++l;
    const MineLevel& lv = P.lv[l];
    const int idx = kept_flat - lv.cand_offset;
    const int label = idx / lv.HW, p = idx - label * lv.HW;
    kept = table[lv.table_offset + p];
    kept_area = os2d_box_area(kept);
    if (tid == 0) {
      float4 c, anchor;
      os2d_mine_crop_box(p, lv.geom, lv.ops, &c, &anchor);
      const size_t row = (size_t)a * P.B + label;
      const size_t e = row * lv.row_stride + p, d = row * lv.HW + p;
      float4 k0 = make_float4(0.f, 0.f, 0.f, 0.f), k1 = k0;
      if (lv.corners) {   // the 8 corner values as two boxes through the level's chain (reference box_coder.py:440-446)
        const float* q = lv.corners + row * 8 * lv.HW + p;
        k0 = os2d_apply_box_ops(make_float4(q[0], q[lv.HW], q[2 * (size_t)lv.HW], q[3 * (size_t)lv.HW]), lv.ops);
        k1 = os2d_apply_box_ops(make_float4(q[4 * (size_t)lv.HW], q[5 * (size_t)lv.HW], q[6 * (size_t)lv.HW], q[7 * (size_t)lv.HW]), lv.ops);
      }
      int* oi = my_index + r * MINE_INDEX;
      oi[0] = l, oi[1] = label, oi[2] = p;
      float* ov = my_values + r * MINE_VALUES;
      ov[0] = c.x, ov[1] = c.y, ov[2] = c.z, ov[3] = c.w;
      ov[4] = anchor.x, ov[5] = anchor.y, ov[6] = anchor.z, ov[7] = anchor.w;
      ov[8] = k0.x, ov[9] = k0.y, ov[10] = k0.z, ov[11] = k0.w;
      ov[12] = k1.x, ov[13] = k1.y, ov[14] = k1.z, ov[15] = k1.w;
      ov[16] = lv.cls_loss[e];
      ov[17] = lv.loc_loss[e];
      ov[18] = lv.cls_preds[d];
    }
    ++count;
  }
  // records that were not filled read as level -1 and zeros
  for (int i = count * MINE_INDEX + tid; i < P.K * MINE_INDEX; i += MINE_THREADS) my_index[i] = -1;
  for (int i = count * MINE_VALUES + tid; i < P.K * MINE_VALUES; i += MINE_THREADS) my_values[i] = 0.f;
  if (tid == 0) out_count[blockIdx.x] = count;
}

bool geometry_ok(int H, int W, int stride, int box_size, int img_w, int img_h, int crop_w, int crop_h) {
  return H >= 1 && W >= 1 && (long long)H * W <= (1ll << 24) && stride >= 1 && box_size >= 1 && img_w >= 1 && img_h >= 1 &&
         crop_w >= 1 && crop_h >= 1;
}

Os2dCropGeometry geometry(int W, int stride, int box_size, int img_w, int img_h, int crop_w, int crop_h) {
  Os2dCropGeometry g;
  g.W = W;
  g.stride = (float)stride;
  g.box_size = (float)box_size;
  g.img_w = (float)img_w;
  g.img_h = (float)img_h;
  g.crop_w = (float)crop_w;
  g.crop_h = (float)crop_h;
  return g;
}

// candidates and table boxes of a pyramid; false when a level or the total is out of range
bool pyramid_sizes(int A, int B, int L, const int* level_hw, long long* N, long long* HWsum) {
  if (A < 1 || B < 1 || L < 1 || L > OS2D_MINE_MAX_LEVELS || !level_hw || (long long)A * 3 > 65535) return false;
  *N = 0;
  *HWsum = 0;
  for (int l = 0; l < L; ++l) {
    const long long H = level_hw[2 * l], W = level_hw[2 * l + 1];
    if (H < 1 || W < 1 || H * W > (1ll << 24)) return false;
    *HWsum += H * W;
    *N += (long long)B * H * W;
  }
  return *N <= (1ll << 28);
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int os2d_train_crop_boxes(int H, int W, int stride, int box_size, int img_w, int img_h, int crop_w, int crop_h, int nops,
                          const int* op_kinds, const float* op_args, float* crop_boxes, float* anchor_boxes, void* stream) {
  if (!geometry_ok(H, W, stride, box_size, img_w, img_h, crop_w, crop_h)) {
    os2d_set_error("os2d_train_crop_boxes: bad geometry H=%d W=%d stride=%d box_size=%d image %dx%d crop %dx%d", H, W, stride, box_size,
                   img_w, img_h, crop_w, crop_h);
    return -1;
  }
  Os2dBoxOps ops;
  if (!os2d_box_ops_from(op_kinds, op_args, nops, &ops)) {
    os2d_set_error("os2d_train_crop_boxes: bad box-op chain (nops=%d, at most %d ops of kind 1..4)", nops, OS2D_BOX_MAX_OPS);
    return -1;
  }
  if (!crop_boxes || !anchor_boxes) return os2d_refuse("os2d_train_crop_boxes: null pointer");
  const int HW = H * W;
  crop_boxes_kernel<<<(HW + 255) / 256, 256, 0, os2d_stream(stream)>>>(HW, geometry(W, stride, box_size, img_w, img_h, crop_w, crop_h), ops,
                                                                       reinterpret_cast<float4*>(crop_boxes),
                                                                       reinterpret_cast<float4*>(anchor_boxes));
  return os2d_launched("os2d_train_crop_boxes");
}

size_t os2d_train_mine_select_workspace_bytes(int A, int B, int L, const int* level_hw) {
  long long N, HWsum;
  if (!pyramid_sizes(A, B, L, level_hw, &N, &HWsum)) return 0;
  return (size_t)A * 3 * (align16((size_t)N) + (size_t)HWsum * sizeof(float4));
}

int os2d_train_mine_select(int A, int B, int L, const int* level_hw, const int* level_img, const int* level_row_stride, int stride,
                           int box_size, const int* op_counts, const int* op_kinds, const float* op_args, const float* const* cls_loss,
                           const float* const* loc_loss, const unsigned char* const* flags, const float* const* cls_preds,
                           const float* const* corners, int crop_w, int crop_h, float iou_thr, int K, int* out_count, int* out_index,
                           float* out_values, void* workspace, size_t workspace_bytes, void* stream) {
  long long N, HWsum;
  if (!pyramid_sizes(A, B, L, level_hw, &N, &HWsum)) {
    os2d_set_error("os2d_train_mine_select: bad shape A=%d B=%d levels=%d (1..%d levels, at most 2^28 candidates per image)", A, B, L,
                   OS2D_MINE_MAX_LEVELS);
    return -1;
  }
  if (K < 1 || K > OS2D_MINE_MAX_K) {
    os2d_set_error("os2d_train_mine_select: K=%d is not in 1..%d", K, OS2D_MINE_MAX_K);
    return -1;
  }
  if (!(iou_thr >= 0.f)) {
    os2d_set_error("os2d_train_mine_select: bad iou_thr=%g", (double)iou_thr);
    return -1;
  }
  if (!level_img || !level_row_stride || !op_counts || !cls_loss || !loc_loss || !flags || !cls_preds || !out_count || !out_index ||
      !out_values || !workspace)
    return os2d_refuse("os2d_train_mine_select: null pointer");
  if (reinterpret_cast<size_t>(workspace) & 15) return os2d_refuse("os2d_train_mine_select: the workspace must be 16-byte aligned");
  MineParams P = {};
  P.L = L, P.B = B, P.K = K, P.N = (int)N;
  P.iou_thr = iou_thr;
  P.table_bytes_offset = align16((size_t)N);
  P.slice_bytes = P.table_bytes_offset + (size_t)HWsum * sizeof(float4);
  int cand = 0, table = 0;
  for (int l = 0; l < L; ++l) {
    MineLevel& lv = P.lv[l];
    const int H = level_hw[2 * l], W = level_hw[2 * l + 1];
    if (!geometry_ok(H, W, stride, box_size, level_img[2 * l], level_img[2 * l + 1], crop_w, crop_h)) {
      os2d_set_error("os2d_train_mine_select: bad geometry at level %d: stride=%d box_size=%d image %dx%d crop %dx%d", l, stride, box_size,
                     level_img[2 * l], level_img[2 * l + 1], crop_w, crop_h);
      return -1;
    }
    if (!os2d_box_ops_from(op_kinds ? op_kinds + l * OS2D_BOX_MAX_OPS : nullptr, op_args ? op_args + l * OS2D_BOX_MAX_OPS * 2 : nullptr,
                           op_counts[l], &lv.ops)) {
      os2d_set_error("os2d_train_mine_select: bad box-op chain at level %d (nops=%d, at most %d ops of kind 1..4)", l, op_counts[l],
                     OS2D_BOX_MAX_OPS);
      return -1;
    }
    if (!cls_loss[l] || !loc_loss[l] || !flags[l] || !cls_preds[l]) {
      os2d_set_error("os2d_train_mine_select: null pointer at level %d", l);
      return -1;
    }
    if (level_row_stride[l] < H * W) {
      os2d_set_error("os2d_train_mine_select: row stride %d of level %d is below its %d anchors", level_row_stride[l], l, H * W);
      return -1;
    }
    lv.cls_loss = cls_loss[l], lv.loc_loss = loc_loss[l], lv.flags = flags[l], lv.cls_preds = cls_preds[l];
    lv.corners = corners ? corners[l] : nullptr;
    lv.HW = H * W, lv.row_stride = level_row_stride[l];
    lv.cand_offset = cand, lv.table_offset = table;
    lv.geom = geometry(W, stride, box_size, level_img[2 * l], level_img[2 * l + 1], crop_w, crop_h);
    cand += B * H * W;
    table += H * W;
  }
  if (workspace_bytes < (size_t)A * 3 * P.slice_bytes) {
    os2d_set_error("os2d_train_mine_select: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)A * 3 * P.slice_bytes);
    return -2;
  }
  mine_select_kernel<<<A * 3, MINE_THREADS, 0, os2d_stream(stream)>>>(P, out_count, out_index, out_values,
                                                                      static_cast<unsigned char*>(workspace));
  return os2d_launched("os2d_train_mine_select");
}

}  // extern "C"
