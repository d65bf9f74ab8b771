// libos2d_backbone_conv.so: the 1x1 convolutions of a frozen-BatchNorm ResNet as fp32 GEMMs on v_mfma_f32_32x32x2_f32 with the folded
// BatchNorm, the residual add and the ReLU as the epilogue (include/os2d_backbone_conv.h).
//
//   conv1x1_kernel<WAVES_M, VEC>   Y[Cout][pixels] = W[Cout][Cin] . X[Cin][pixels], pixels = N * Ho * Wo: the batch index is folded into
//                                  the pixel dimension, a tile may span images.  A work-group of 4 waves owns a tile of TM = 64 * WAVES_M
//                                  output channels x TN = 64 * (4 / WAVES_M) pixels (128 x 128, or 64 x 256 for layers of at most 64
//                                  outputs); a wave owns 64 x 64 of it as 2 x 2 accumulators of 32 x 32.  Per step of TILE_K input
//                                  channels the tile's slices of W and X go from global memory to registers (the NEXT step's, while this
//                                  step's products run) and from there to one of two LDS images, [k][m] and [k][pixel]: lane l of a wave
//                                  reads its MFMA operands A[m = l & 31][k = l >> 5], B[k = l >> 5][pixel = l & 31] as consecutive floats.
//                                  VEC: a row of X is read as 16-byte units (stride 1, H * W a multiple of 4, x 16-byte aligned: a unit
//                                  never leaves its image); otherwise element by element, which also serves the stride-2 gather.
//                                  Everything outside the tensors - k >= Cin, m >= Cout, pixel >= pixels - is written to LDS as 0.0f in
//                                  BOTH operands.  The accumulator layout (pixel = lane & 31, channel = (reg & 3) + 8 * (reg >> 2) +
//                                  4 * (lane >> 5)) makes every store of the epilogue 32 consecutive floats of one output row.
// The k order of every output is ascending and one chain (the MFMA is a k-ordered fmaf chain), whatever tile shape or load path runs.
// No atomics; the grid is capped at OS2D_BACKBONE_CONV_MAX_GROUPS work-groups that stride over the tiles, output-channel tiles of one
// pixel tile next to each other, so that its slice of X is read from HBM once.
#include "../csrc_backbone/backbone_common.h"
#include "../../include/os2d_backbone_conv.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_TK = OS2D_BACKBONE_CONV_TILE_K;
constexpr int CV_PAD = 4;                             // floats between LDS rows: the transposing stores of W spread over the banks
constexpr long long CV_MAX_CHANNELS = 1ll << 20;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Conv {
  const float *x, *w, *s, *t, *r, *sr, *tr;
  float* y;
  int Cin, Cout, W, Wo, HWo, HW, stride, relu;
  int wvec;                // rows of w are read as 16-byte units
  int ksteps;              // ceil(Cin / TILE_K)
  int mtiles;
  long long pixels;        // N * Ho * Wo
  long long tiles;
};

// MODE 0: the fold alone, 1: + r, 2: + the fold of r
template <int MODE>
__device__ __forceinline__ float conv_out(float acc, float s, float t, float r, float sr, float tr, bool relu) {
#pragma clang fp contract(off)
  float v = bb_bn(acc, s, t);
  if (MODE) {
    const float d = MODE == 2 ? bb_bn(r, sr, tr) : r;
    v = v + d;
  }
  return relu ? bb_relu_nan(v) : v;
}

// The epilogue of one wave's 64 x 64 outputs from its accumulators: register q of accumulator [a][b] is channel cbase + 32 * a +
// (q & 3) + 8 * (q >> 2) at pixel pbase + 32 * b.  Every load is from a clamped, always valid address and has no branch around it, so
// that the 16 loads of a group are in flight together; only the stores are predicated.
template <int MODE>
__device__ __forceinline__ void conv_epilogue(const Conv& p, const f32x16 (&acc)[2][2], int cbase, long long pbase) {
  const bool relu = p.relu != 0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float s[16], t[16], sr[16], tr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
      const int cc = co < p.Cout ? co : p.Cout - 1;
      s[q] = p.s[cc];
      t[q] = p.t[cc];
      sr[q] = MODE == 2 ? p.sr[cc] : 0.0f;
      tr[q] = MODE == 2 ? p.tr[cc] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const long long pix = pbase + b * 32;
      const bool pix_ok = pix < p.pixels;
      const long long pc = pix_ok ? pix : p.pixels - 1;
      const long long img = pc / p.HWo;
      const long long at = img * p.Cout * p.HWo + (pc - img * p.HWo);
      float r[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
        const int cc = co < p.Cout ? co : p.Cout - 1;
        r[q] = MODE ? p.r[at + (long long)cc * p.HWo] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
        const float out = conv_out<MODE>(acc[a][b][q], s[q], t[q], r[q], sr[q], tr[q], relu);
        if (pix_ok && co < p.Cout) p.y[at + (long long)co * p.HWo] = out;
      }
    }
  }
}

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
    for (int j = 0; j < XO; ++j) {
      const long long pix = n0 + 4 * b_nq + j;
      xok[j] = pix < p.pixels;
      xoff[j] = 0;
      if (xok[j]) {
        const long long img = pix / p.HWo;
        const int i = (int)(pix - img * p.HWo);
        const int src = p.stride == 1 ? i : (i / p.Wo) * 2 * p.W + (i % p.Wo) * 2;
        xoff[j] = img * p.Cin * plane + src;
      }
    }

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
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.0f;

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

    const int mode = p.r == nullptr ? 0 : (p.sr == nullptr ? 1 : 2);
    const int cbase = m0 + wm * 64 + 4 * half;
    const long long pbase = n0 + wn * 64 + l32;
    if (mode == 0)
      conv_epilogue<0>(p, acc, cbase, pbase);
    else if (mode == 1)
      conv_epilogue<1>(p, acc, cbase, pbase);
    else
      conv_epilogue<2>(p, acc, cbase, pbase);
  }
}

// the limits of include/os2d_backbone.h on one tensor of N x C x plane
bool too_large(int N, int C, long long plane) {
  return (long long)N * C > BB_MAX_ROWS || plane > BB_MAX_PLANE || (long long)N * C * plane > BB_MAX_ELEMENTS;
}

}  // namespace

extern "C" {

int os2d_backbone_conv_abi_version(void) { return OS2D_BACKBONE_CONV_ABI_VERSION; }
const char* os2d_backbone_conv_last_error(void) { return os2d_error_text; }

int os2d_backbone_conv1x1(const float* x, const float* w, const float* s, const float* t, const float* r, const float* sr, const float* tr,
                          float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu, void* stream) {
  if (!x || !w || !s || !t || !y) return os2d_refuse("conv1x1: null pointer");
  if ((sr == nullptr) != (tr == nullptr)) return os2d_refuse("conv1x1: sr and tr are both given or both NULL");
  if (sr && !r) return os2d_refuse("conv1x1: sr and tr come only together with r");
  if (bb_misaligned(x, 4) || bb_misaligned(w, 4) || bb_misaligned(s, 4) || bb_misaligned(t, 4) || bb_misaligned(r, 4) || bb_misaligned(sr, 4) ||
      bb_misaligned(tr, 4) || bb_misaligned(y, 4))
    return os2d_refuse("conv1x1: pointer not aligned (4 bytes)");
  if (N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return os2d_refuse("conv1x1: bad shape (every size >= 1)");
  if (stride != 1 && stride != 2) return os2d_refuse("conv1x1: stride is 1 or 2");
  if (relu != 0 && relu != 1) return os2d_refuse("conv1x1: relu is 0 or 1");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const long long HW = (long long)H * W, HWo = (long long)Ho * Wo;
  if (Cin > CV_MAX_CHANNELS || Cout > CV_MAX_CHANNELS || too_large(N, Cin, HW) || too_large(N, Cout, HWo))
    return os2d_refuse("conv1x1: too large (Cin, Cout <= 2^20; for x and y: N * C < 2^31, H * W <= 2^30, N * C * H * W <= 2^40)");
  const long long ny = (long long)N * Cout * HWo;
  const size_t py = reinterpret_cast<size_t>(y), ybytes = (size_t)ny * sizeof(float);
  const auto y_meets = [&](const float* q, long long n) {
    const size_t pq = reinterpret_cast<size_t>(q);
    return py < pq + (size_t)n * sizeof(float) && pq < py + ybytes;
  };
  if (y_meets(x, (long long)N * Cin * HW)) return os2d_refuse("conv1x1: y overlaps x");
  if (y_meets(w, (long long)Cout * Cin)) return os2d_refuse("conv1x1: y overlaps w");
  if (r && bb_overlap(r, y, ny)) return os2d_refuse("conv1x1: y overlaps r");

  Conv p;
  p.x = x; p.w = w; p.s = s; p.t = t; p.r = r; p.sr = sr; p.tr = tr; p.y = y;
  p.Cin = Cin; p.Cout = Cout; p.W = W; p.Wo = Wo; p.HWo = (int)HWo; p.HW = (int)HW; p.stride = stride; p.relu = relu;
  p.wvec = Cin % 4 == 0 && !bb_misaligned(w, 16);
  p.ksteps = (Cin + CV_TK - 1) / CV_TK;
  p.pixels = (long long)N * HWo;
  const bool small = Cout <= OS2D_BACKBONE_CONV_SMALL_TILE_M;
  const int tm = small ? OS2D_BACKBONE_CONV_SMALL_TILE_M : OS2D_BACKBONE_CONV_TILE_M;
  const int tn = small ? OS2D_BACKBONE_CONV_SMALL_TILE_N : OS2D_BACKBONE_CONV_TILE_N;
  p.mtiles = (Cout + tm - 1) / tm;
  p.tiles = p.mtiles * ((p.pixels + tn - 1) / tn);
  const bool vec = stride == 1 && HW % 4 == 0 && !bb_misaligned(x, 16);
  const dim3 grid((unsigned)(p.tiles < OS2D_BACKBONE_CONV_MAX_GROUPS ? p.tiles : OS2D_BACKBONE_CONV_MAX_GROUPS)), block(CV_THREADS);
  if (small) {
    if (vec)
      hipLaunchKernelGGL((conv1x1_kernel<1, true>), grid, block, 0, os2d_stream(stream), p);
    else
      hipLaunchKernelGGL((conv1x1_kernel<1, false>), grid, block, 0, os2d_stream(stream), p);
  } else {
    if (vec)
      hipLaunchKernelGGL((conv1x1_kernel<2, true>), grid, block, 0, os2d_stream(stream), p);
    else
      hipLaunchKernelGGL((conv1x1_kernel<2, false>), grid, block, 0, os2d_stream(stream), p);
  }
  return os2d_launched("conv1x1_kernel");
}

}  // extern "C"
