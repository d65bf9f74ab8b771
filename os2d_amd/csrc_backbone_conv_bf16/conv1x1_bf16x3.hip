// libos2d_backbone_conv_bf16.so: the 1x1 convolutions of a frozen-BatchNorm ResNet in split-bf16 arithmetic - every fp32 operand as
// three bf16 parts, six products on v_mfma_f32_32x32x16_bf16, fp32 accumulation - with the folded BatchNorm, the residual add and the
// ReLU as the epilogue (include/os2d_backbone_conv_bf16.h).
//
//   pack_kernel                    w [Cout][Cin] -> wp[part][Kp / 8][Cout][8]: once per weight, the A operand as the kernel reads it.
//   conv1x1_bf16x3_kernel<WAVES_M, VEC>
//                                  Y[Cout][pixels] = W . X in the tiling of csrc_backbone/conv1x1_common.h: a work-group of 4 waves owns
//                                  TM = 64 * WAVES_M output channels x TN = 64 * (4 / WAVES_M) pixels (128 x 128, or 64 x 256 for layers
//                                  of at most 64 outputs).
//                                  Per step of TILE_K = 32 input channels:
//                                    - the step's slice of wp, 3 * 4 * TM units of 16 bytes, is copied to LDS as it is;
//                                    - a thread loads 2 neighbouring pixels of 8 consecutive input channels of x (a wave: 512-byte runs
//                                      of 8 rows), splits the 16 values in registers and writes per (part, pixel) ONE 16-byte unit of 8
//                                      bf16: the transpose from "contiguous along pixels" to "8 consecutive k per lane" is the choice
//                                      of which two values share a v_cvt_pk_bf16_f32;
//                                    - both LDS images are [part][k / 8][row or pixel] units, so the 32 lanes of a half-wave read
//                                      consecutive units as their MFMA fragments (lane l: row / pixel l & 31, k = 8 * (l >> 5) ... + 7).
//                                  The NEXT step's global loads are issued before this step's products and land in registers while they
//                                  run; one LDS image, two barriers per step, two work-groups per CU fill each other's gaps.
//                                  VEC: the two pixels are one 8-byte load (stride 1, H * W even, x 8-byte aligned: a pair never leaves
//                                  its image); otherwise element by element, which also serves the stride-2 gather.
//                                  Everything outside the tensors - k >= Cin, m >= Cout, pixel >= pixels - is 0 in BOTH operands.
// W stays the A operand, for the accumulator layout of conv1x1_common.h, whose stores are 32 consecutive floats of one output row.  With
// the roles swapped a lane would hold 4 consecutive pixels of one channel, a 16-byte store, but the 32 lanes of a store would hit 32
// different rows: 16-byte pieces instead of 128-byte runs.
// The order of the products of an output is fixed (the header), whatever tile shape or load path runs.  No atomics, no inline assembly.
// The epilogue, the argument checks and the capped grid are those of conv1x1_common.h, shared with the fp32 library.
#include "../csrc_backbone/conv1x1_common.h"
#include "../../include/os2d_backbone_conv_bf16.h"
#include "bf16x3_split.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_TK = OS2D_BACKBONE_CONV_BF16_TILE_K;
constexpr int CB_KO = CB_TK / 8;                      // 16-byte units of k per step
constexpr int CB_PARTS = 3;
constexpr ConvTiles CB_TILES = {OS2D_BACKBONE_CONV_BF16_TILE_M, OS2D_BACKBONE_CONV_BF16_TILE_N, OS2D_BACKBONE_CONV_BF16_SMALL_TILE_M,
                                OS2D_BACKBONE_CONV_BF16_SMALL_TILE_N, CB_TK, OS2D_BACKBONE_CONV_BF16_MAX_GROUPS};

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Conv : ConvCall {
  const uint4* wp;
  int kunits;              // Kp / 8, Kp = TILE_K * ksteps
};

// 8 consecutive k of one pixel -> its three 16-byte units.  The common case is branch-free, two values per conversion; a value at the top
// of the range (NaN, Inf, or one that rounds to bf16's infinity) sends the 8 of them through the scalar rules of bf16x3_split_x, which
// give the same parts for every other value.
__device__ __forceinline__ void split_octet(const float (&v)[8], uint4& o0, uint4& o1, uint4& o2) {
  bool special = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) special |= bf16x3_special(v[j]);
  uint32_t p[CB_PARTS][4];
  if (!special) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float a = v[2 * q], b = v[2 * q + 1];
      const uint32_t u0 = bf16x3_round_pair(a, b);
      const float a1 = a - bf16x3_float(u0 << 16), b1 = b - bf16x3_float(u0 & 0xFFFF0000u);
      const uint32_t u1 = bf16x3_round_pair(a1, b1);
      const float a2 = a1 - bf16x3_float(u1 << 16), b2 = b1 - bf16x3_float(u1 & 0xFFFF0000u);
      p[0][q] = u0;
      p[1][q] = u1;
      p[2][q] = bf16x3_round_pair(a2, b2);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint16_t lo[CB_PARTS], hi[CB_PARTS];
      bf16x3_split_x(v[2 * q], &lo[0], &lo[1], &lo[2]);
      bf16x3_split_x(v[2 * q + 1], &hi[0], &hi[1], &hi[2]);
#pragma unroll
      for (int i = 0; i < CB_PARTS; ++i) p[i][q] = (uint32_t)lo[i] | ((uint32_t)hi[i] << 16);
    }
  }
  o0 = make_uint4(p[0][0], p[0][1], p[0][2], p[0][3]);
  o1 = make_uint4(p[1][0], p[1][1], p[1][2], p[1][3]);
  o2 = make_uint4(p[2][0], p[2][1], p[2][2], p[2][3]);
}

__device__ __forceinline__ f32x16 mfma(const uint4& a, const uint4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int WAVES_M, bool VEC>
__global__ __launch_bounds__(CB_THREADS, 2) void conv1x1_bf16x3_kernel(const Conv p) {
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = 64 * WAVES_M, TN = 64 * WAVES_N;
  constexpr int AQ = CB_PARTS * CB_KO * TM / CB_THREADS;      // 16-byte units of wp per thread and step
  constexpr int BI = TN / 128;                                // (pixel pair, 8 k) items of x per thread and step
  __shared__ uint4 sA[CB_PARTS][CB_KO][TM];
  __shared__ uint4 sB[CB_PARTS][CB_KO][TN];
  static_assert(AQ * CB_THREADS == CB_PARTS * CB_KO * TM && BI * 128 == TN, "every unit of a step has one thread");

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // the wave's index as a scalar
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int l32 = lane & 31, half = lane >> 5;
  const int b_ko = wave;                                      // item i of x: k = 8 * b_ko ... + 7 of the step, pixels 2 * (lane + 64 * i), + 1
  const long long plane = (long long)p.HW;

  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int m0 = (int)(tile % p.mtiles) * TM;
    const long long n0 = (tile / p.mtiles) * TN;

    // where this thread's pixels start in x (channel 0 of their image)
    long long xoff[BI][2];
    bool xok[BI][2];
#pragma unroll
    for (int i = 0; i < BI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) xok[i][j] = conv_source(p, n0 + 2 * (lane + 64 * i) + j, xoff[i][j]);

    uint4 ra[AQ];
    float2 rb[BI][8];
    // every load is from a clamped, always valid address and has no branch around it: what lies outside the tensors becomes 0 afterwards
    auto load = [&](int kt) {
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        // unit u = tid + 256 * i of the step's image [part][unit of k][TM]: its row is the thread's, the rest is the wave's
        const int m = m0 + (lane + 64 * wave) % TM, c = (CB_THREADS * i + 64 * wave) / TM;
        const uint4* units = p.wp + ((long long)(c / CB_KO) * p.kunits + kt * CB_KO + c % CB_KO) * p.Cout;
        const uint4 v = units[m < p.Cout ? m : p.Cout - 1];
        ra[i] = m < p.Cout ? v : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int i = 0; i < BI; ++i)
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const int k = kt * CB_TK + 8 * b_ko + kk;
          const bool k_ok = k < p.Cin;
          const float* row = p.x + (k_ok ? k : p.Cin - 1) * plane;
          float2 v;
          if (VEC) {
            v = *reinterpret_cast<const float2*>(row + xoff[i][0]);
          } else {
            v.x = row[xoff[i][0]];
            v.y = row[xoff[i][1]];
          }
          rb[i][kk].x = k_ok && xok[i][0] ? v.x : 0.0f;
          rb[i][kk].y = k_ok && xok[i][1] ? v.y : 0.0f;
        }
    };
    auto store = [&]() {
      uint4* a = &sA[0][0][0];
#pragma unroll
      for (int i = 0; i < AQ; ++i) a[tid + CB_THREADS * i] = ra[i];
#pragma unroll
      for (int i = 0; i < BI; ++i) {
        float lo[8], hi[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          lo[kk] = rb[i][kk].x;
          hi[kk] = rb[i][kk].y;
        }
        const int px = 2 * (lane + 64 * i);
        split_octet(lo, sB[0][b_ko][px], sB[1][b_ko][px], sB[2][b_ko][px]);
        split_octet(hi, sB[0][b_ko][px + 1], sB[1][b_ko][px + 1], sB[2][b_ko][px + 1]);
      }
    };

    f32x16 acc[2][2];
    conv_clear(acc);

    load(0);
    for (int kt = 0; kt < p.ksteps; ++kt) {
      store();
      __syncthreads();
      if (kt + 1 < p.ksteps) load(kt + 1);
#pragma unroll
      for (int kb = 0; kb < CB_TK / 16; ++kb) {
        uint4 fa[CB_PARTS][2], fb[CB_PARTS][2];
#pragma unroll
        for (int i = 0; i < CB_PARTS; ++i)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            fa[i][h] = sA[i][2 * kb + half][wm * 64 + 32 * h + l32];
            fb[i][h] = sB[i][2 * kb + half][wn * 64 + 32 * h + l32];
          }
        // the six products of the block, smallest first: (part of x, part of w)
        constexpr int XI[6] = {2, 1, 0, 1, 0, 0}, WI[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int g = 0; g < 6; ++g)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = mfma(fa[WI[g]][a], fb[XI[g]][b], acc[a][b]);
      }
      __syncthreads();                   // every wave has read its fragments: the image may be overwritten
    }

    conv_finish(p, acc, m0 + wm * 64, n0 + wn * 64, half, l32);
  }
}

__global__ __launch_bounds__(CB_THREADS) void pack_kernel(const float* w, unsigned short* wp, int Cout, int Cin, int Kp) {
  const long long total = (long long)Cout * Kp;
  for (long long i = (long long)blockIdx.x * CB_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * CB_THREADS) {
    const int co = (int)(i / Kp), k = (int)(i % Kp);
    uint16_t b[CB_PARTS];
    bf16x3_split(k < Cin ? w[(long long)co * Cin + k] : 0.0f, &b[0], &b[1], &b[2]);
#pragma unroll
    for (int part = 0; part < CB_PARTS; ++part) wp[(((long long)part * (Kp / 8) + k / 8) * Cout + co) * 8 + k % 8] = b[part];
  }
}

long long padded_k(int Cin) { return ((long long)Cin + CB_TK - 1) / CB_TK * CB_TK; }

}  // namespace

extern "C" {

int os2d_backbone_conv_bf16_abi_version(void) { return OS2D_BACKBONE_CONV_BF16_ABI_VERSION; }
const char* os2d_backbone_conv_bf16_last_error(void) { return os2d_error_text; }

size_t os2d_backbone_conv_bf16_packed_elems(int Cout, int Cin) {
  if (!conv_channels_ok(Cout) || !conv_channels_ok(Cin)) return 0;
  return (size_t)CB_PARTS * (size_t)padded_k(Cin) * (size_t)Cout;
}

int os2d_backbone_conv_bf16_pack_weights(const float* w, unsigned short* wp, int Cout, int Cin, void* stream) {
  if (!w || !wp) return os2d_refuse("pack_weights: null pointer");
  if (bb_misaligned(w, 4)) return os2d_refuse("pack_weights: w not aligned (4 bytes)");
  if (bb_misaligned(wp, 16)) return os2d_refuse("pack_weights: wp not aligned (16 bytes)");
  if (Cout < 1 || Cin < 1) return os2d_refuse("pack_weights: bad shape (every size >= 1)");
  if (!conv_channels_ok(Cout) || !conv_channels_ok(Cin)) return os2d_refuse("pack_weights: too large (Cin, Cout <= 2^20)");
  if (bb_bytes_meet(w, (size_t)Cout * Cin * sizeof(float), wp, os2d_backbone_conv_bf16_packed_elems(Cout, Cin) * sizeof(unsigned short)))
    return os2d_refuse("pack_weights: wp overlaps w");
  const long long Kp = padded_k(Cin), blocks = ((long long)Cout * Kp + CB_THREADS - 1) / CB_THREADS;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(CB_THREADS);
  hipLaunchKernelGGL(pack_kernel, grid, block, 0, os2d_stream(stream), w, wp, Cout, Cin, (int)Kp);
  return os2d_launched("pack_kernel");
}

int os2d_backbone_conv1x1_bf16x3(const float* x, const unsigned short* wp, const float* s, const float* t, const float* r, const float* sr,
                                 const float* tr, float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu, void* stream) {
  Conv p;
  const ConvWeights weights = {wp, "wp", 16, os2d_backbone_conv_bf16_packed_elems(Cout, Cin) * sizeof(unsigned short)};
  if (const int rc = conv_check("conv1x1_bf16x3", p, weights, x, s, t, r, sr, tr, y, N, Cin, Cout, H, W, stride, relu)) return rc;
  p.wp = reinterpret_cast<const uint4*>(wp);
  bool small;
  const dim3 grid(conv_plan(p, CB_TILES, small)), block(CB_THREADS);
  p.kunits = p.ksteps * CB_KO;
  const bool vec = stride == 1 && p.HW % 2 == 0 && !bb_misaligned(x, 8);
  const auto kernel = small ? (vec ? conv1x1_bf16x3_kernel<1, true> : conv1x1_bf16x3_kernel<1, false>)
                            : (vec ? conv1x1_bf16x3_kernel<2, true> : conv1x1_bf16x3_kernel<2, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, os2d_stream(stream), p);
  return os2d_launched("conv1x1_bf16x3_kernel");
}

}  // extern "C"
