// libos2d_backbone_conv.so: the 1x1 convolutions of a frozen-BatchNorm ResNet as fp32 GEMMs on v_mfma_f32_32x32x2_f32 with the folded
// BatchNorm, the residual add and the ReLU as the epilogue (include/os2d_backbone_conv.h).
//
//   conv1x1_kernel<WAVES_M, VEC>   Y[Cout][pixels] = W[Cout][Cin] . X[Cin][pixels] in the tiling of csrc_backbone/conv1x1_common.h: a
//                                  work-group of 4 waves owns TM = 64 * WAVES_M output channels x TN = 64 * (4 / WAVES_M) pixels (128 x 128,
//                                  or 64 x 256 for layers of at most 64 outputs).  Per step of TILE_K input channels the tile's slices of
//                                  W and X go from global memory to registers (the NEXT step's, while this step's products run) and
//                                  from there to one of two LDS images, [k][m] and [k][pixel]: lane l of a wave reads its MFMA operands
//                                  A[m = l & 31][k = l >> 5], B[k = l >> 5][pixel = l & 31] as consecutive floats.
//                                  VEC: a row of X is read as 16-byte units (stride 1, H * W a multiple of 4, x 16-byte aligned: a unit
//                                  never leaves its image); otherwise element by element, which also serves the stride-2 gather.
//                                  Everything outside the tensors - k >= Cin, m >= Cout, pixel >= pixels - is written to LDS as 0.0f in
//                                  BOTH operands.
// The k order of every output is ascending and one chain (the MFMA is a k-ordered fmaf chain), whatever tile shape or load path runs.
// No atomics.  The epilogue, the argument checks and the capped grid are those of conv1x1_common.h, shared with the bf16x3 library.
#include "../csrc_backbone/conv1x1_common.h"
#include "../../include/os2d_backbone_conv.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_TK = OS2D_BACKBONE_CONV_TILE_K;
constexpr int CV_PAD = 4;                             // floats between LDS rows: the transposing stores of W spread over the banks
constexpr ConvTiles CV_TILES = {OS2D_BACKBONE_CONV_TILE_M, OS2D_BACKBONE_CONV_TILE_N, OS2D_BACKBONE_CONV_SMALL_TILE_M, OS2D_BACKBONE_CONV_SMALL_TILE_N,
                                CV_TK, OS2D_BACKBONE_CONV_MAX_GROUPS};

struct Conv : ConvCall {
  const float* w;
  int wvec;                // rows of w are read as 16-byte units
};

template <int WAVES_M, bool VEC>
__global__ __launch_bounds__(CV_THREADS, 2) void conv1x1_kernel(const Conv p) {
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int TM = 64 * WAVES_M, TN = 64 * WAVES_N;
  constexpr int SA = TM + CV_PAD, SB = TN + CV_PAD;
  constexpr int AQ = TM * CV_TK / 4 / CV_THREADS;      // 4-float slots of W per thread and step
  constexpr int BQ = TN * CV_TK / 4 / CV_THREADS;      // of X
  constexpr int NQ = TN / 4;                           // pixel quads of a tile
  constexpr int KB = CV_THREADS / NQ;                  // k rows of X that the work-group loads at once
  constexpr int XO = VEC ? 1 : 4;
  __shared__ __attribute__((aligned(16))) float sA[2][CV_TK][SA];
  __shared__ __attribute__((aligned(16))) float sB[2][CV_TK][SB];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int l32 = lane & 31, half = lane >> 5;
  const int a_kq = tid & 3, a_m = tid >> 2;            // slot i of W: channel a_m + 64 * i, k = 4 * a_kq ... + 3
  const int b_nq = tid % NQ, b_k = tid / NQ;           // slot i of X: k = b_k + KB * i, pixels 4 * b_nq ... + 3
  const long long plane = (long long)p.HW;

  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int m0 = (int)(tile % p.mtiles) * TM;
    const long long n0 = (tile / p.mtiles) * TN;

    // where this thread's pixels start in x (channel 0 of their image)
    long long xoff[XO];
    bool xok[XO];
#pragma unroll
    for (int j = 0; j < XO; ++j) xok[j] = conv_source(p, n0 + 4 * b_nq + j, xoff[j]);

    float4 ra[AQ], rb[BQ];
    auto load = [&](int kt) {
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        const int m = m0 + a_m + 64 * i, k = kt * CV_TK + 4 * a_kq;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m < p.Cout && k < p.Cin) {
          const float* row = p.w + (long long)m * p.Cin + k;
          if (p.wvec) {
            v = *reinterpret_cast<const float4*>(row);
          } else {
            v.x = row[0];
            if (k + 1 < p.Cin) v.y = row[1];
            if (k + 2 < p.Cin) v.z = row[2];
            if (k + 3 < p.Cin) v.w = row[3];
          }
        }
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < BQ; ++i) {
        const int k = kt * CV_TK + b_k + KB * i;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < p.Cin) {
          const float* row = p.x + k * plane;
          if (VEC) {
            if (xok[0]) v = *reinterpret_cast<const float4*>(row + xoff[0]);
          } else {
            if (xok[0]) v.x = row[xoff[0]];
            if (xok[XO > 1 ? 1 : 0]) v.y = row[xoff[XO > 1 ? 1 : 0]];
            if (xok[XO > 2 ? 2 : 0]) v.z = row[xoff[XO > 2 ? 2 : 0]];
            if (xok[XO > 3 ? 3 : 0]) v.w = row[xoff[XO > 3 ? 3 : 0]];
          }
        }
        rb[i] = v;
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        const int m = a_m + 64 * i;
        sA[buf][4 * a_kq + 0][m] = ra[i].x;
        sA[buf][4 * a_kq + 1][m] = ra[i].y;
        sA[buf][4 * a_kq + 2][m] = ra[i].z;
        sA[buf][4 * a_kq + 3][m] = ra[i].w;
      }
#pragma unroll
      for (int i = 0; i < BQ; ++i) *reinterpret_cast<float4*>(&sB[buf][b_k + KB * i][4 * b_nq]) = rb[i];
    };

    f32x16 acc[2][2];
    conv_clear(acc);

    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < p.ksteps; ++kt) {
      const int buf = kt & 1;
      const bool more = kt + 1 < p.ksteps;
      if (more) load(kt + 1);
#pragma unroll
      for (int ks = 0; ks < CV_TK / 2; ++ks) {
        const int kk = 2 * ks + half;
        const float a0 = sA[buf][kk][wm * 64 + l32], a1 = sA[buf][kk][wm * 64 + 32 + l32];
        const float b0 = sB[buf][kk][wn * 64 + l32], b1 = sB[buf][kk][wn * 64 + 32 + l32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if (more) store(buf ^ 1);          // last read in step kt - 1, which every wave left at that step's barrier
      __syncthreads();
    }

    conv_finish(p, acc, m0 + wm * 64, n0 + wn * 64, half, l32);
  }
}

}  // namespace

extern "C" {

int os2d_backbone_conv_abi_version(void) { return OS2D_BACKBONE_CONV_ABI_VERSION; }
const char* os2d_backbone_conv_last_error(void) { return os2d_error_text; }

int os2d_backbone_conv1x1(const float* x, const float* w, const float* s, const float* t, const float* r, const float* sr, const float* tr,
                          float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu, void* stream) {
  Conv p;
  const ConvWeights weights = {w, "w", 4, (size_t)Cout * Cin * sizeof(float)};
  if (const int rc = conv_check("conv1x1", p, weights, x, s, t, r, sr, tr, y, N, Cin, Cout, H, W, stride, relu)) return rc;
  p.w = w;
  p.wvec = Cin % 4 == 0 && !bb_misaligned(w, 16);
  bool small;
  const dim3 grid(conv_plan(p, CV_TILES, small)), block(CV_THREADS);
  const bool vec = stride == 1 && p.HW % 4 == 0 && !bb_misaligned(x, 16);
  const auto kernel = small ? (vec ? conv1x1_kernel<1, true> : conv1x1_kernel<1, false>) : (vec ? conv1x1_kernel<2, true> : conv1x1_kernel<2, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, os2d_stream(stream), p);
  return os2d_launched("conv1x1_kernel");
}

}  // extern "C"
