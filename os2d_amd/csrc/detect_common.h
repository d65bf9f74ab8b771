// What the detection stage shares (gfx950): box decode and the level -> image transform chains, the IoU test, the score
// sort key, the bitonic sort of a class's (key, index) arrays in LDS and the in-order greedy-NMS resolve of 64 candidates in a
// wave - once each, for nms.hip, detect.hip, detect_pyramid.hip, sample_decode.hip (decode_boxes_kernel) and abi.hip.  The
// fused kernels must stay bit-identical to the generic chain (tests/test_decode_gpu.py), which they are by construction when
// all of them call the same functions.
//
// The same source is compiled for the host by tests/host/detect_check.cpp (-DOS2D_HOST_EMU, SPMD emulator of
// tests/host/spmd_emu.h): the includer then supplies float4 / make_float4 and the hardware hooks DET_*.
#pragma once
#ifdef OS2D_HOST_EMU
#ifndef DET_DEV
#error "the includer defines float4, make_float4, DET_DEV, DET_BARRIER, DET_BALLOT, DET_READLANE"
#endif
#else
#include "os2d_common.h"
#define DET_DEV __device__ __forceinline__
#define DET_BARRIER() __syncthreads()
#define DET_BALLOT(p) __builtin_amdgcn_ballot_w64(p)
#define DET_READLANE(v, lane) __builtin_amdgcn_readlane(v, lane) /* int value of lane `lane` (wave-uniform index) */
#endif

// Box decode of ONE location (reference os2d/modeling/box_coder.py:319-330 = torchvision BoxCoder.decode_single with
// weights (10,10,5,5) and the dw/dh clamp log(1000/16), then clip_boxes_to_image): shared by decode_boxes_kernel and
// detect_level_kernel so both produce bit-identical boxes.  ``l`` points at loc[nb][0][n]; channel stride HW.
DET_DEV float4 os2d_decode_box(const float* __restrict__ l, int HW, int n, int W, float stride, float half_box, float img_w,
                               float img_h) {
  const int h = n / W, w = n - h * W;
  const float ecx = stride * ((float)w + 0.5f), ecy = stride * ((float)h + 0.5f);
  const float ax1 = ecx - half_box, ay1 = ecy - half_box;
  const float aw = (ecx + half_box) - ax1, ah = (ecy + half_box) - ay1;
  const float acx = ax1 + 0.5f * aw, acy = ay1 + 0.5f * ah;
  const float clipv = 4.135166556742356f;  // log(1000/16): torchvision BoxCoder.bbox_xform_clip
  const float dx = l[0] / 10.0f, dy = l[HW] / 10.0f;
  const float dw = fminf(l[2 * (size_t)HW] / 5.0f, clipv), dh = fminf(l[3 * (size_t)HW] / 5.0f, clipv);
  const float pcx = dx * aw + acx, pcy = dy * ah + acy;
  const float pw = expf(dw) * aw, ph = expf(dh) * ah;
  float4 o = make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph);
  if (img_w > 0.f && img_h > 0.f) {  // clip_boxes_to_image; a non-positive size means "leave unclipped"
    o.x = fminf(fmaxf(o.x, 0.f), img_w);
    o.y = fminf(fmaxf(o.y, 0.f), img_h);
    o.z = fminf(fmaxf(o.z, 0.f), img_w);
    o.w = fminf(fmaxf(o.w, 0.f), img_h);
  }
  return o;
}

// Chain of axis-aligned box transforms that maps a level's boxes into the output image: what the reference's per-level
// ``TransformList`` of closures amounts to (os2d/structures/transforms.py:12-27, built by os2d/data/dataloader.py:286-336 from
// BoxList.resize / transpose / crop, os2d/structures/bounding_box.py:138-226), applied op by op with the reference's
// roundings - every product / difference rounded on its own (no contraction into fused multiply-adds), so the fused decode
// equals the generic chain (which calls the closures on a BoxList) bit for bit.  Kinds: OS2D_BOX_OP_* of include/os2d_hip.h.
#define OS2D_BOX_MAX_OPS 6
#define OS2D_BOX_MAX_DEFAULT_OPS 12
template <int N>
struct Os2dBoxOpsN {
  int n;
  unsigned char kind[N];
  float ax[N], ay[N];
};
typedef Os2dBoxOpsN<OS2D_BOX_MAX_OPS> Os2dBoxOps;
// the anchors ("default_boxes") go through a chain of their own: in the reference they ride along as a BoxList FIELD of the
// boxes - BoxList.transpose / crop also transform such fields, resize does not (bounding_box.py:162,196-199,222-225) - and the
// level's transform is then applied to the field once more (box_coder.py:515-516); the caller records that whole sequence
typedef Os2dBoxOpsN<OS2D_BOX_MAX_DEFAULT_OPS> Os2dDefaultBoxOps;
template <int N>
DET_DEV float4 os2d_apply_box_ops(float4 b, const Os2dBoxOpsN<N>& t) {
#pragma clang fp contract(off)
  for (int k = 0; k < t.n; ++k) {
    const float ax = t.ax[k], ay = t.ay[k];
    switch (t.kind[k]) {
      case 1:   // SCALE: BoxList.resize
        b.x = b.x * ax;
        b.y = b.y * ay;
        b.z = b.z * ax;
        b.w = b.w * ay;
        break;
      case 2: { // HFLIP about the image width ax: (xmin, xmax) = (W - xmax, W - xmin)
        const float lo = ax - b.z, hi = ax - b.x;
        b.x = lo;
        b.z = hi;
        break;
      }
      case 3: { // VFLIP about the image height ay
        const float lo = ay - b.w, hi = ay - b.y;
        b.y = lo;
        b.w = hi;
        break;
      }
      case 4:   // SHIFT: BoxList.crop (x - left, y - top)
        b.x = b.x - ax;
        b.y = b.y - ay;
        b.z = b.z - ax;
        b.w = b.w - ay;
        break;
      default:
        break;
    }
  }
  return b;
}
template <int N>
static inline Os2dBoxOpsN<N> os2d_box_ops_scale(float sx, float sy) {
  Os2dBoxOpsN<N> t = {};
  t.n = 1;
  t.kind[0] = 1;
  t.ax[0] = sx;
  t.ay[0] = sy;
  return t;
}
// ops from the ABI arrays (kinds [nops], args [nops][2]); false on a bad chain
template <int N>
static inline bool os2d_box_ops_from(const int* kinds, const float* args, int nops, Os2dBoxOpsN<N>* t) {
  *t = Os2dBoxOpsN<N>{};
  if (nops < 0 || nops > N || (nops > 0 && (!kinds || !args))) return false;
  t->n = nops;
  for (int k = 0; k < nops; ++k) {
    if (kinds[k] < 1 || kinds[k] > 4) return false;
    t->kind[k] = (unsigned char)kinds[k];
    t->ax[k] = args[2 * k];
    t->ay[k] = args[2 * k + 1];
  }
  return true;
}

// IoU(a, b) > thr with torchvision's arithmetic (inter / (area_a + area_b - inter) in fp32, reference
// os2d/structures/bounding_box.py:367 -> torchvision.ops.nms).  The IEEE division (a dozen VALU instructions) is only
// executed when some lane of the wave is within 1e-5 (relative) of the threshold - everywhere else comparing inter with
// thr * union gives the same answer as the rounded quotient.  The vote makes the branch wave-uniform, so it is a real
// branch and not an if-converted select.
// Every product and sum below is rounded on its own, like the reference's tensor expressions: the compiler must NOT contract
// them into fused multiply-adds (hipcc's default for device code is -ffp-contract=fast, and HIP's __fmul_rn / __fadd_rn are
// plain operators that it fuses just the same: area_a + area_b - w * h became two v_fma_f32).  Whether it did depended on
// unrelated code generation choices - the decisions at the threshold flipped when the library was first built without
// packed-FP32 instructions (tests/test_decode_gpu.py::test_nms_decisions_at_the_iou_threshold).
DET_DEV float os2d_box_area(float4 b) {
#pragma clang fp contract(off)
  const float bw = b.z - b.x, bh = b.w - b.y;
  return bw * bh;
}

DET_DEV bool os2d_iou_gt(float4 a, float area_a, float4 b, float area_b, float thr) {
#pragma clang fp contract(off)
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = w * h;
  const float sum = area_a + area_b;
  const float uni = sum - inter;
  const float tu = thr * uni;
  bool res = inter > tu;
  const bool near = !(uni > 0.f && fabsf(inter - tu) > 1e-5f * fabsf(tu));
  if (DET_BALLOT(near) != 0ull) {
    if (near) res = inter / uni > thr;
  }
  return res;
}

// Sort key of a score: ascending unsigned key = descending score; equal scores (-0 == +0 included) get equal keys, so a sort
// by (key, index) is a STABLE descending sort by score.  A valid key is never 0xffffffff (that would be score -NaN): the
// kernels give that key to invalid entries, which sort to the end.
DET_DEV unsigned int os2d_score_key(float s) {
  unsigned int u = (s == 0.f) ? 0u : __builtin_bit_cast(unsigned int, s);  // -0 and +0 tie in a comparison sort
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                         // monotone map float -> uint (ascending)
  return ~u;                                                              // ascending key = descending score
}

// sort size of v entries: the next power of two, at least 8 (keeps the LDS sub-arrays of the kernels 16-byte aligned)
static inline int os2d_next_pow2(int v) {
  int p = 8;
  while (p < v) p <<= 1;
  return p;
}

// Bitonic sort of key[NP2] / idx[NP2] in LDS, ascending in (key, idx), by a work-group of NTHR threads; NP2 a power of two.
// Stage k = 2^m needs the compare-exchange levels j = 2^(m-1) .. 1; they are taken NB <= 3 at a time: a thread loads the
// 2^NB elements whose indices differ in bits lo .. lo+NB-1, exchanges them in registers and stores them back - 35 LDS round
// trips instead of 91 passes at 8192 keys.  Every round trip ends with a work-group barrier; the caller supplies the one
// between filling the arrays and the sort.
template <int NTHR, int NB>
DET_DEV void os2d_bitonic_levels(unsigned int* key, unsigned short* idx, int NP2, int tid, int k, int lo) {
  const int groups = NP2 >> NB;
  for (int g = tid; g < groups; g += NTHR) {
    const int base = ((g >> lo) << (lo + NB)) | (g & ((1 << lo) - 1));
    const bool up = (base & k) == 0;
    unsigned int kk[1 << NB];
    unsigned short ii[1 << NB];
#pragma unroll
    for (int e = 0; e < (1 << NB); ++e) {
      kk[e] = key[base | (e << lo)];
      ii[e] = idx[base | (e << lo)];
    }
#pragma unroll
    for (int b = NB - 1; b >= 0; --b) {
#pragma unroll
      for (int e = 0; e < (1 << NB); ++e) {
        if ((e >> b) & 1) continue;
        const int f = e | (1 << b);
        const bool gt = kk[e] > kk[f] || (kk[e] == kk[f] && ii[e] > ii[f]);
        if (gt == up) {
          const unsigned int tk = kk[e];
          kk[e] = kk[f];
          kk[f] = tk;
          const unsigned short ti = ii[e];
          ii[e] = ii[f];
          ii[f] = ti;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < (1 << NB); ++e) {
      key[base | (e << lo)] = kk[e];
      idx[base | (e << lo)] = ii[e];
    }
  }
  DET_BARRIER();
}

template <int NTHR>
DET_DEV void os2d_bitonic_sort(unsigned int* key, unsigned short* idx, int NP2, int tid) {
  for (int m = 1; (1 << m) <= NP2; ++m) {
    const int k = 1 << m;
    for (int hi = m - 1; hi >= 0; hi -= 3) {  // levels hi .. max(hi-2, 0)
      const int nb = hi + 1 < 3 ? hi + 1 : 3;
      const int lo = hi - nb + 1;
      if (nb == 3) os2d_bitonic_levels<NTHR, 3>(key, idx, NP2, tid, k, lo);
      else if (nb == 2) os2d_bitonic_levels<NTHR, 2>(key, idx, NP2, tid, k, lo);
      else os2d_bitonic_levels<NTHR, 1>(key, idx, NP2, tid, k, lo);
    }
  }
}

DET_DEV float4 os2d_readlane4(float4 v, int lane) {
  float4 r;
  r.x = __builtin_bit_cast(float, DET_READLANE(__builtin_bit_cast(int, v.x), lane));
  r.y = __builtin_bit_cast(float, DET_READLANE(__builtin_bit_cast(int, v.y), lane));
  r.z = __builtin_bit_cast(float, DET_READLANE(__builtin_bit_cast(int, v.z), lane));
  r.w = __builtin_bit_cast(float, DET_READLANE(__builtin_bit_cast(int, v.w), lane));
  return r;
}

// In-order greedy resolve of the 64 candidates of a wave (lane = rank by score; every lane of the wave calls it): the best
// candidate still alive is kept, every later alive candidate whose IoU with it exceeds thr dies (one IoU test over the 64
// lanes per box kept), and so on.  `alive`: candidates not yet suppressed (wave-uniform mask); returns the mask of kept lanes.
DET_DEV unsigned long long os2d_nms_resolve(float4 me, float my_area, unsigned long long alive, float thr) {
  unsigned long long kbits = 0ull;
  while (alive) {
    const int i = __builtin_ctzll(alive);  // best-scoring candidate still alive: kept
    kbits |= 1ull << i;
    const float4 kb = os2d_readlane4(me, i);
    const bool hit = os2d_iou_gt(kb, os2d_box_area(kb), me, my_area, thr);
    alive &= ~(DET_BALLOT(hit) | ((2ull << i) - 1ull));  // drop lanes 0..i and everything the new box suppresses
  }
  return kbits;
}

// detect.hip (the launcher takes a transform chain, so it is declared here and not with the others in os2d_common.h)
#ifndef OS2D_HOST_EMU
size_t os2d_detect_level_lds_bytes(int H, int W);
int os2d_launch_detect_level(const float* loc, const float* cls, int B, int H, int W, int stride, int rec_field,
                             float img_w, float img_h, const Os2dBoxOps& ops, float score_thr, float iou_thr,
                             float* out_boxes, float* out_scores, int* out_index, int* out_count, hipStream_t stream);
#endif
