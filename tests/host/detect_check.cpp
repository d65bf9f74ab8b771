// Host check of os2d_amd/csrc/detect_common.h on the SPMD emulator (spmd_emu.h) - the same source the GPU runs:
//   the bitonic sort with a 1024-thread work-group (what detect.hip / detect_pyramid.hip launch) against std::stable_sort by
//   descending score, on keys made by os2d_score_key;
//   the in-order resolve of 64 candidates + os2d_iou_gt against a scalar greedy NMS with the rounded quotient inter / union > thr.
// Built and run by tests/test_detect_host.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "spmd_emu.h"

struct float4 {
  float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

#define OS2D_HOST_EMU 1
#define DET_DEV static inline
#define DET_BARRIER() emu::group_barrier()
#define DET_BALLOT(p) emu::ballot(p)
#define DET_READLANE(v, lane) emu::readlane(v, lane)
#include "detect_common.h"

static unsigned rnd(unsigned& s) {
  s = s * 1664525u + 1013904223u;
  return s >> 8;
}
static float frand(unsigned& s) { return (rnd(s) & 0xffffff) / float(1 << 24); }

// ---------------------------------------------------------------- sort
constexpr int NTHR = 1024;

struct SortCase {
  int NP2;
  std::vector<float> score;     // [NP2]
  std::vector<char> valid;      // [NP2]
  std::vector<unsigned> key;    // out
  std::vector<unsigned short> idx;
};

static SortCase make_sort_case(int NP2, int flavour, unsigned seed) {
  SortCase c;
  c.NP2 = NP2;
  c.score.resize(NP2);
  c.valid.resize(NP2);
  c.key.assign(NP2, 0);
  c.idx.assign(NP2, 0);
  const float few[8] = {-2.5f, -0.0f, 0.0f, 1.5f, -1e-40f, 1e-40f, 0.25f, -std::numeric_limits<float>::infinity()};
  const int n = flavour == 2 ? NP2 - NP2 / 3 : NP2;      // flavour 2: the tail past the valid count is invalid, as in the kernels
  for (int i = 0; i < NP2; ++i) {
    if (flavour == 0) c.score[i] = few[rnd(seed) % 8];                       // many equal scores, +0 / -0, denormals, -inf
    else if (flavour == 1) c.score[i] = std::floor(frand(seed) * 16.f) - 8.f;   // 16 values around zero
    else c.score[i] = (frand(seed) - 0.5f) * std::ldexp(1.f, (int)(rnd(seed) % 40) - 20);
    c.valid[i] = i < n && rnd(seed) % 10 != 0;
  }
  return c;
}

static int check_sort(const SortCase& c) {
  std::vector<int> ref;
  for (int i = 0; i < c.NP2; ++i)
    if (c.valid[i]) ref.push_back(i);
  std::stable_sort(ref.begin(), ref.end(), [&](int a, int b) { return c.score[a] > c.score[b]; });
  for (int i = 0; i < c.NP2; ++i)
    if (!c.valid[i]) ref.push_back(i);                   // invalid entries: at the end, in index order
  for (int i = 0; i < c.NP2; ++i) {
    const unsigned want = c.valid[ref[i]] ? os2d_score_key(c.score[ref[i]]) : 0xffffffffu;
    if (c.idx[i] != ref[i] || c.key[i] != want) {
      std::printf("sort NP2=%d: position %d holds index %d key %08x, expected index %d key %08x\n", c.NP2, i, (int)c.idx[i],
                  c.key[i], ref[i], want);
      return 1;
    }
  }
  return 0;
}

static int run_sorts() {
  std::vector<SortCase> cases;
  const int sizes[4] = {8, 64, 512, 8192};
  for (int s = 0; s < 4; ++s)
    for (int f = 0; f < 3; ++f) cases.push_back(make_sort_case(sizes[s], f, 77u + 13u * s + f));
  emu::launch(1, NTHR, (size_t)8192 * 6, [&] {
    const int tid = emu::tid();
    for (SortCase& c : cases) {
      unsigned int* skey = reinterpret_cast<unsigned int*>(emu::lds());
      unsigned short* sidx = reinterpret_cast<unsigned short*>(emu::lds() + (size_t)c.NP2 * 4);
      for (int i = tid; i < c.NP2; i += NTHR) {
        skey[i] = c.valid[i] ? os2d_score_key(c.score[i]) : 0xffffffffu;
        sidx[i] = (unsigned short)i;
      }
      emu::group_barrier();
      os2d_bitonic_sort<NTHR>(skey, sidx, c.NP2, tid);
      for (int i = tid; i < c.NP2; i += NTHR) {
        c.key[i] = skey[i];
        c.idx[i] = sidx[i];
      }
      emu::group_barrier();
    }
  });
  int bad = 0;
  for (const SortCase& c : cases) bad += check_sort(c);
  std::printf("sort: %d cases, %d failed\n", (int)cases.size(), bad);
  return bad;
}

// ---------------------------------------------------------------- resolve
static float ref_area(const float4& b) { return (b.z - b.x) * (b.w - b.y); }
static bool ref_iou_gt(const float4& a, const float4& b, float thr) {      // torchvision: the rounded quotient
  const float w = std::max(std::min(a.z, b.z) - std::max(a.x, b.x), 0.f);
  const float h = std::max(std::min(a.w, b.w) - std::max(a.y, b.y), 0.f);
  const float inter = w * h;
  const float uni = ref_area(a) + ref_area(b) - inter;
  return inter / uni > thr;
}
static unsigned long long ref_resolve(const float4* box, unsigned long long alive, float thr) {
  unsigned long long kept = 0ull;
  for (int i = 0; i < 64; ++i) {
    if (!((alive >> i) & 1ull)) continue;
    kept |= 1ull << i;
    for (int j = i + 1; j < 64; ++j)
      if (((alive >> j) & 1ull) && ref_iou_gt(box[i], box[j], thr)) alive &= ~(1ull << j);
  }
  return kept;
}

struct Batch {
  float4 box[64];
  unsigned long long alive;
  float thr;
  unsigned long long kbits[64];      // out, per lane
};

static int run_resolve() {
  std::vector<Batch> batches;
  unsigned seed = 4242u;
  // clustered random boxes (many overlaps, some duplicates and empty boxes), random / all-dead / all-alive masks
  for (int t = 0; t < 40; ++t) {
    Batch b;
    for (int i = 0; i < 64; ++i) {
      const float cx = 30.f * (float)(rnd(seed) % 4) + 6.f * frand(seed), cy = 30.f * (float)(rnd(seed) % 3) + 6.f * frand(seed);
      const float w = 4.f + 12.f * frand(seed), h = 4.f + 12.f * frand(seed);
      b.box[i] = make_float4(cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h);
      if (i > 0 && rnd(seed) % 16 == 0) b.box[i] = b.box[rnd(seed) % i];                 // duplicate: IoU exactly 1
      if (rnd(seed) % 32 == 0) b.box[i].z = b.box[i].x;                                  // empty: union can be 0 (0 / 0)
    }
    b.alive = t == 0 ? 0ull : t < 4 ? ~0ull : ((unsigned long long)rnd(seed) << 40) ^ ((unsigned long long)rnd(seed) << 20) ^ rnd(seed);
    b.thr = t % 5 == 4 ? 0.5f : 0.3f;
    batches.push_back(b);
  }
  // pairs at the threshold, the construction of tests/test_decode_gpu.py::test_nms_decisions_at_the_iou_threshold: a square of
  // side 10 s and a box of the same width and height 3 s +- 0..3 ulps - IoU = 0.3 within a few ulps.  32 pairs per batch, apart
  // in x by multiples of 1024; s is a multiple of 1/8, so the shifted coordinates and the widths are exact.
  int near = 0, suppressed = 0, pairs = 0;
  for (int t = 0; t < 40; ++t) {
    Batch b;
    for (int p = 0; p < 32; ++p) {
      const float s = (float)(4 + rnd(seed) % 316) / 8.f, ox = 1024.f * (float)p;
      float y = 3.f * s;
      const int k = t * 32 + p, ulps = k % 7 ? (int)(rnd(seed) % 4) : 0;
      for (int u = 0; u < ulps; ++u) y = std::nextafter(y, k % 2 ? INFINITY : -INFINITY);
      b.box[2 * p] = make_float4(ox, 0.f, ox + 10.f * s, 10.f * s);
      b.box[2 * p + 1] = make_float4(ox, 0.f, ox + 10.f * s, y);
      near += std::fabs(y / (10.f * s) - 0.3f) < 1e-6f;
      suppressed += ref_iou_gt(b.box[2 * p], b.box[2 * p + 1], 0.3f);
      ++pairs;
    }
    b.alive = ~0ull;
    b.thr = 0.3f;
    batches.push_back(b);
  }
  if (near < pairs * 9 / 10 || suppressed < pairs / 10 || suppressed > pairs * 9 / 10) {
    std::printf("resolve: the threshold pairs do not sit at the threshold (%d near, %d suppressed of %d)\n", near, suppressed, pairs);
    return 1;
  }
  emu::launch(1, 64, 0, [&] {
    const int lane = emu::tid();
    for (Batch& b : batches) {
      const float4 me = b.box[lane];
      b.kbits[lane] = os2d_nms_resolve(me, os2d_box_area(me), b.alive, b.thr);
    }
  });
  int bad = 0;
  for (size_t t = 0; t < batches.size(); ++t) {
    const Batch& b = batches[t];
    const unsigned long long want = ref_resolve(b.box, b.alive, b.thr);
    for (int l = 0; l < 64; ++l)
      if (b.kbits[l] != want) {
        std::printf("resolve batch %d lane %d: kept %016llx, expected %016llx (alive %016llx)\n", (int)t, l, b.kbits[l], want, b.alive);
        ++bad;
        break;
      }
  }
  std::printf("resolve: %d batches (%d threshold pairs, %d suppressed), %d failed\n", (int)batches.size(), pairs, suppressed, bad);
  return bad;
}

int main() {
  if (os2d_next_pow2(1) != 8 || os2d_next_pow2(8) != 8 || os2d_next_pow2(9) != 16 || os2d_next_pow2(4800) != 8192) {
    std::printf("os2d_next_pow2 is wrong\n");
    return 1;
  }
  if (os2d_score_key(0.f) != os2d_score_key(-0.f) || !(os2d_score_key(1.f) < os2d_score_key(0.5f)) ||
      !(os2d_score_key(-1.f) > os2d_score_key(-0.5f)) || !(os2d_score_key(-1e-40f) > os2d_score_key(0.f))) {
    std::printf("os2d_score_key is not a descending map\n");
    return 1;
  }
  const int bad = run_sorts() + run_resolve();
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
