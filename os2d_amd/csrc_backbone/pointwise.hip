// libos2d_backbone.so: everything between the convolutions of a frozen-BatchNorm ResNet (include/os2d_backbone.h).
//
//   bn_act_kernel<MODE>      y = relu(bn(x)) (MODE 0), relu(bn(x) + r) (1), relu(bn(x) + bn'(r)) (2).  A tensor is N * C channel rows
//                            of HW floats, and HW is odd at many level sizes: a row starts at any multiple of 4 bytes.  Each row is
//                            cut into 16-byte units counted from the 16-byte boundary at or below its first element; a lane owns
//                            one unit per tile: the inner units go as one float4, the (at most two) units that straddle the row's
//                            ends element by element.  A row whose x, y and r do not share their position inside a unit goes
//                            element by element throughout.  2^lanes_log2 lanes of a work-group share a row, so that the short rows
//                            of the deep layers still fill a work-group.
//   bn_relu_maxpool_kernel   a lane owns 4 adjacent outputs of one output row: 3 x 9 inputs, each normalised once, one float4 store
//                            where the address allows.  Out-of-image taps count as 0, which never wins: every value is >= 0 or NaN.
// No LDS, no atomics; the grid is capped at OS2D_BACKBONE_MAX_GROUPS work-groups that stride over the tiles.
#include "backbone_common.h"

namespace {

struct Pointwise {
  const float *x, *s, *t, *r, *sr, *tr;
  float* y;
  int rows, C, HW;
  int lanes_log2;          // lanes that share a row
  int chunks;              // tiles per group of rows: ceil(units of the longest row / lanes)
  long long tiles;
};

template <int MODE>
__device__ __forceinline__ float bn_act(float x, float r, float s, float t, float sr, float tr) {
#pragma clang fp contract(off)
  const float v = bb_bn(x, s, t);
  if (MODE == 0) return bb_relu_nan(v);
  const float d = MODE == 2 ? bb_bn(r, sr, tr) : r;
  return bb_relu_nan(v + d);
}

template <int MODE>
__global__ __launch_bounds__(BB_THREADS) void bn_act_kernel(const Pointwise p) {
  const int lanes = 1 << p.lanes_log2;
  const int lane = (int)threadIdx.x & (lanes - 1);
  const int sub = (int)threadIdx.x >> p.lanes_log2;
  const int rows_per_group = BB_THREADS >> p.lanes_log2;
  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long long group = tile / p.chunks;
    const int chunk = (int)(tile - group * p.chunks);
    const long long row = group * rows_per_group + sub;
    if (row >= p.rows) continue;
    const int c = (int)(row % p.C);
    const long long base = row * p.HW;
    const float* x = p.x + base;
    const float* r = MODE ? p.r + base : nullptr;
    float* y = p.y + base;
    const size_t in_unit = reinterpret_cast<size_t>(x) & 15;
    const bool vec = (reinterpret_cast<size_t>(y) & 15) == in_unit && (!MODE || (reinterpret_cast<size_t>(r) & 15) == in_unit);
    const int lead = vec ? (int)(in_unit >> 2) : 0;               // elements of the first unit that belong to the row before
    const int e0 = (chunk * lanes + lane) * 4 - lead;             // first element of this lane's unit; -3 ... -1 in the first unit
    if (e0 >= p.HW) continue;
    const float s = p.s[c], t = p.t[c];
    const float sr = MODE == 2 ? p.sr[c] : 0.0f, tr = MODE == 2 ? p.tr[c] : 0.0f;
    if (vec && e0 >= 0 && e0 + 4 <= p.HW) {
      const float4 a = *reinterpret_cast<const float4*>(x + e0);
      float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (MODE) b = *reinterpret_cast<const float4*>(r + e0);
      float4 o;
      o.x = bn_act<MODE>(a.x, b.x, s, t, sr, tr);
      o.y = bn_act<MODE>(a.y, b.y, s, t, sr, tr);
      o.z = bn_act<MODE>(a.z, b.z, s, t, sr, tr);
      o.w = bn_act<MODE>(a.w, b.w, s, t, sr, tr);
      *reinterpret_cast<float4*>(y + e0) = o;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q;
        if (e >= 0 && e < p.HW) y[e] = bn_act<MODE>(x[e], MODE ? r[e] : 0.0f, s, t, sr, tr);
      }
    }
  }
}

struct Pool {
  const float *x, *s, *t;
  float* y;
  int planes, C, H, W, Hp, Wp;
  int gx;                  // groups of 4 outputs per output row
  int chunks;              // tiles per plane: ceil(Hp * gx / BB_THREADS)
  long long tiles;
};

__global__ __launch_bounds__(BB_THREADS) void bn_relu_maxpool_kernel(const Pool p) {
  const int items = p.Hp * p.gx;
  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const long long plane = tile / p.chunks;
    const int item = (int)(tile - plane * p.chunks) * BB_THREADS + (int)threadIdx.x;
    if (item >= items) continue;
    const int oy = item / p.gx;
    const int ox0 = (item - oy * p.gx) * 4;
    const int c = (int)(plane % p.C);
    const float s = p.s[c], t = p.t[c];
    const float* x = p.x + plane * ((long long)p.H * p.W);
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= p.H) continue;
      const float* line = x + (long long)iy * p.W;
      float v[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int ix = 2 * ox0 - 1 + j;
        v[j] = (ix >= 0 && ix < p.W) ? bb_relu_nan(bb_bn(line[ix], s, t)) : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) m[q] = bb_max_nan(bb_max_nan(bb_max_nan(m[q], v[2 * q]), v[2 * q + 1]), v[2 * q + 2]);
    }
    float* y = p.y + plane * ((long long)p.Hp * p.Wp) + (long long)oy * p.Wp + ox0;
    if (ox0 + 4 <= p.Wp && (reinterpret_cast<size_t>(y) & 15) == 0) {
      *reinterpret_cast<float4*>(y) = make_float4(m[0], m[1], m[2], m[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (ox0 + q < p.Wp) y[q] = m[q];
    }
  }
}

// what every entry point checks of its sizes; rows = N * C
int check_sizes(const char* what, int N, int C, long long plane) {
  if (N < 1 || C < 1 || plane < 1) return OS2D_REFUSE(-1, "%s: bad shape (every size >= 1)", what);
  if ((long long)N * C > BB_MAX_ROWS || plane > BB_MAX_PLANE || (long long)N * C * plane > BB_MAX_ELEMENTS)
    return OS2D_REFUSE(-1, "%s: too large (N * C < 2^31, HW <= 2^30, N * C * HW <= 2^40)", what);
  return 0;
}

int launch_bn_act(const char* what, int mode, Pointwise p, void* stream) {
  const long long total = (long long)p.rows * p.HW;
  if (p.y != p.x && bb_overlap(p.x, p.y, total)) return OS2D_REFUSE(-1, "%s: y overlaps x without being x", what);
  if (mode && bb_overlap(p.r, p.y, total)) return OS2D_REFUSE(-1, "%s: y overlaps r", what);
  const int units = (p.HW + 3 + 3) / 4;                      // of the longest row: 3 leading elements of another row
  p.lanes_log2 = BB_MIN_LANES_LOG2;
  while (p.lanes_log2 < BB_MAX_LANES_LOG2 && (1 << p.lanes_log2) < units) ++p.lanes_log2;
  const int lanes = 1 << p.lanes_log2, rows_per_group = BB_THREADS >> p.lanes_log2;
  p.chunks = (units + lanes - 1) / lanes;
  p.tiles = (((long long)p.rows + rows_per_group - 1) / rows_per_group) * p.chunks;
  const dim3 grid(bb_groups(p.tiles)), block(BB_THREADS);
  if (mode == 0)
    hipLaunchKernelGGL(bn_act_kernel<0>, grid, block, 0, os2d_stream(stream), p);
  else if (mode == 1)
    hipLaunchKernelGGL(bn_act_kernel<1>, grid, block, 0, os2d_stream(stream), p);
  else
    hipLaunchKernelGGL(bn_act_kernel<2>, grid, block, 0, os2d_stream(stream), p);
  return os2d_launched("bn_act_kernel");
}

}  // namespace

extern "C" {

int os2d_backbone_abi_version(void) { return OS2D_BACKBONE_ABI_VERSION; }
const char* os2d_backbone_last_error(void) { return os2d_error_text; }

int os2d_backbone_bn_relu(const float* x, const float* s, const float* t, float* y, int N, int C, int HW, void* stream) {
  if (!x || !s || !t || !y) return os2d_refuse("bn_relu: null pointer");
  if (bb_misaligned(x, 4) || bb_misaligned(s, 4) || bb_misaligned(t, 4) || bb_misaligned(y, 4)) return os2d_refuse("bn_relu: pointer not aligned (4 bytes)");
  if (const int rc = check_sizes("bn_relu", N, C, HW)) return rc;
  Pointwise p = {x, s, t, nullptr, nullptr, nullptr, y, N * C, C, HW, 0, 0, 0};
  return launch_bn_act("bn_relu", 0, p, stream);
}

int os2d_backbone_bn_add_relu(const float* x, const float* s, const float* t, const float* r, const float* sr, const float* tr, float* y,
                              int N, int C, int HW, void* stream) {
  if (!x || !s || !t || !r || !y) return os2d_refuse("bn_add_relu: null pointer");
  if ((sr == nullptr) != (tr == nullptr)) return os2d_refuse("bn_add_relu: sr and tr are both given or both NULL");
  if (bb_misaligned(x, 4) || bb_misaligned(s, 4) || bb_misaligned(t, 4) || bb_misaligned(r, 4) || bb_misaligned(sr, 4) || bb_misaligned(tr, 4) ||
      bb_misaligned(y, 4))
    return os2d_refuse("bn_add_relu: pointer not aligned (4 bytes)");
  if (const int rc = check_sizes("bn_add_relu", N, C, HW)) return rc;
  Pointwise p = {x, s, t, r, sr, tr, y, N * C, C, HW, 0, 0, 0};
  return launch_bn_act("bn_add_relu", sr ? 2 : 1, p, stream);
}

int os2d_backbone_bn_relu_maxpool(const float* x, const float* s, const float* t, float* y, int N, int C, int H, int W, void* stream) {
  if (!x || !s || !t || !y) return os2d_refuse("bn_relu_maxpool: null pointer");
  if (bb_misaligned(x, 4) || bb_misaligned(s, 4) || bb_misaligned(t, 4) || bb_misaligned(y, 4)) return os2d_refuse("bn_relu_maxpool: pointer not aligned (4 bytes)");
  if (H < 1 || W < 1) return os2d_refuse("bn_relu_maxpool: bad shape (every size >= 1)");
  if (const int rc = check_sizes("bn_relu_maxpool", N, C, (long long)H * W)) return rc;
  Pool p;
  p.x = x; p.s = s; p.t = t; p.y = y;
  p.planes = N * C; p.C = C; p.H = H; p.W = W;
  p.Hp = (H - 1) / 2 + 1;
  p.Wp = (W - 1) / 2 + 1;
  if (bb_bytes_meet(x, (size_t)p.planes * H * W * sizeof(float), y, (size_t)p.planes * p.Hp * p.Wp * sizeof(float)))
    return os2d_refuse("bn_relu_maxpool: y overlaps x");
  p.gx = (p.Wp + 3) / 4;
  p.chunks = (p.Hp * p.gx + BB_THREADS - 1) / BB_THREADS;
  p.tiles = (long long)p.planes * p.chunks;
  hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(bb_groups(p.tiles)), dim3(BB_THREADS), 0, os2d_stream(stream), p);
  return os2d_launched("bn_relu_maxpool_kernel");
}

}  // extern "C"
