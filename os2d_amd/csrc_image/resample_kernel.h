// The resample kernel of libos2d_image.so (resample.hip) and its checked launch, as templates: PADDED = false is what
// os2d_image_resample instantiates, PADDED = true what os2d_augment_resample_padded of libos2d_augment.so does
// (csrc_augment/resample_padded.hip).  One source, so the two cannot drift apart; each library instantiates only its own.
#ifndef OS2D_IMAGE_RESAMPLE_KERNEL_H
#define OS2D_IMAGE_RESAMPLE_KERNEL_H
#include "image_common.h"

#define OS2D_RESAMPLE_MAX_RATIO 16 /* OS2D_IMAGE_MAX_RATIO / OS2D_AUGMENT_MAX_RATIO of the public headers */


namespace {

struct Resample {
  const unsigned char* src;
  long long row_pitch, image_stride;
  int img_w, img_h;                                                 // read by the PADDED instantiations only
  int x0, y0, w, h, hflip, vflip;
  const int *xcoef, *xbounds, *ycoef, *ybounds;
  int kx, ky, ow, oh, th, lds_rows;
  const float* lut;
  void* out;
};

__device__ __forceinline__ int clip8(int ss) { return min(max(ss >> IMG_PRECISION_BITS, 0), 255); }

// PADDED: the window may leave the image; a position outside it is a pixel of value 0 that takes its filter weight like any
// other (nothing is read for it).  Without the flag the window is inside the image and no position is tested.
template <bool U8OUT, bool PADDED>
__global__ __launch_bounds__(IMG_THREADS) void resample_kernel(const Resample p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* lut = reinterpret_cast<float*>(lds);                       // [3][256] (float output only)
  unsigned char* rows = lds + (U8OUT ? 0 : IMG_LUT_BYTES);          // [nrows][3][IMG_TW]
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * IMG_TW, ty0 = blockIdx.y * p.th, a = blockIdx.z;
  const int tw = min(IMG_TW, p.ow - tx0), th = min(p.th, p.oh - ty0);

  if (!U8OUT)
    for (int i = tid; i < 3 * 256; i += IMG_THREADS) lut[i] = p.lut[i];

  // the source rows the tile's output rows reach (the same for every thread)
  int r0 = p.h, r1 = 0;
  for (int j = 0; j < th; ++j) {
    const int lo = p.ybounds[2 * (ty0 + j)], n = p.ybounds[2 * (ty0 + j) + 1];
    r0 = min(r0, lo);
    r1 = max(r1, lo + n);
  }
  r0 = max(r0, 0);
  const int nrows = max(min(r1 - r0, p.lds_rows), 1);

  // ---- phase 1: thread = one column of the tile, every second staged row
  const unsigned char* img = p.src + (size_t)a * p.image_stride;
  const int col = tid & (IMG_TW - 1);
  if (col < tw) {
    const int ox = tx0 + col;
    const int xmin = p.xbounds[2 * ox], xn = min(p.xbounds[2 * ox + 1], p.kx);
    const int* kk = p.xcoef + (size_t)ox * p.kx;
    for (int r = tid / IMG_TW; r < nrows; r += IMG_THREADS / IMG_TW) {
      int sy = min(max(r0 + r, 0), p.h - 1);
      if (p.vflip) sy = p.h - 1 - sy;
      const bool row_inside = !PADDED || (p.y0 + sy >= 0 && p.y0 + sy < p.img_h);
      const unsigned char* row = img + (long long)(row_inside ? p.y0 + sy : 0) * p.row_pitch;
      int s0 = 1 << (IMG_PRECISION_BITS - 1), s1 = s0, s2 = s0;
      for (int t = 0; t < xn; ++t) {
        int sx = min(max(xmin + t, 0), p.w - 1);
        if (p.hflip) sx = p.w - 1 - sx;
        if (PADDED && !(row_inside && p.x0 + sx >= 0 && p.x0 + sx < p.img_w)) continue;
        const unsigned char* px = row + (size_t)(p.x0 + sx) * 3;
        const int k = kk[t];
        s0 += px[0] * k;
        s1 += px[1] * k;
        s2 += px[2] * k;
      }
      unsigned char* dst = rows + (size_t)r * 3 * IMG_TW + col;
      dst[0] = (unsigned char)clip8(s0);
      dst[IMG_TW] = (unsigned char)clip8(s1);
      dst[2 * IMG_TW] = (unsigned char)clip8(s2);
    }
  }
  __syncthreads();

  // ---- phase 2
  if (U8OUT) {
    unsigned char* out = static_cast<unsigned char*>(p.out) + (size_t)a * p.oh * p.ow * 3;
    const int per_row = tw * 3;
    for (int i = tid; i < th * per_row; i += IMG_THREADS) {
      const int j = i / per_row, e = i - j * per_row;
      const int c = e % 3, x = e / 3, oy = ty0 + j;
      const int ymin = p.ybounds[2 * oy], yn = min(p.ybounds[2 * oy + 1], p.ky);
      const int* kk = p.ycoef + (size_t)oy * p.ky;
      int ss = 1 << (IMG_PRECISION_BITS - 1);
      for (int t = 0; t < yn; ++t) {
        const int r = min(max(ymin - r0 + t, 0), nrows - 1);
        ss += rows[((size_t)r * 3 + c) * IMG_TW + x] * kk[t];
      }
      out[((size_t)oy * p.ow + tx0) * 3 + e] = (unsigned char)clip8(ss);
    }
  } else {
    float* out = static_cast<float*>(p.out);
    // item = (row j, channel c, 16-byte unit u of that plane row); unit u holds elements base + 4 u .. + 3 of the output, where
    // base is the 4-element boundary at or before the tile row's first element
    for (int i = tid; i < th * 3 * IMG_UNITS; i += IMG_THREADS) {
      const int seg = i / IMG_UNITS, u = i - seg * IMG_UNITS;
      const int j = seg / 3, c = seg - j * 3, oy = ty0 + j;
      const size_t e0 = (((size_t)a * 3 + c) * p.oh + oy) * p.ow + tx0;        // the tile row's first element
      const int mis = (int)(e0 & 3);
      const int x_first = 4 * u - mis;                                         // tile column of the unit's element 0
      if (x_first >= tw) continue;
      const int ymin = p.ybounds[2 * oy], yn = min(p.ybounds[2 * oy + 1], p.ky);
      const int* kk = p.ycoef + (size_t)oy * p.ky;
      const int half = 1 << (IMG_PRECISION_BITS - 1);
      int s[4] = {half, half, half, half};
      int xs[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xs[q] = min(max(x_first + q, 0), tw - 1);
      for (int t = 0; t < yn; ++t) {
        const int r = min(max(ymin - r0 + t, 0), nrows - 1);
        const unsigned char* line = rows + ((size_t)r * 3 + c) * IMG_TW;
        const int k = kk[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += line[xs[q]] * k;
      }
      const float* lc = lut + c * 256;
      float4 v = make_float4(lc[clip8(s[0])], lc[clip8(s[1])], lc[clip8(s[2])], lc[clip8(s[3])]);
      float* dst = out + (e0 - mis) + (size_t)4 * u;
      if (x_first >= 0 && x_first + 3 < tw) {
        *reinterpret_cast<float4*>(dst) = v;
      } else {                                                                 // head / tail unit of the row
        if (x_first >= 0) dst[0] = v.x;
        if (x_first + 1 >= 0 && x_first + 1 < tw) dst[1] = v.y;
        if (x_first + 2 >= 0 && x_first + 2 < tw) dst[2] = v.z;
        if (x_first + 3 < tw) dst[3] = v.w;
      }
    }
  }
}

// 0 <= first, 1 <= taps <= k, first + taps <= n for every output position
bool bounds_ok(const int* b, int m, int k, int n) {
  for (int i = 0; i < m; ++i) {
    const int lo = b[2 * i], cnt = b[2 * i + 1];
    if (lo < 0 || cnt < 1 || cnt > k || lo > n - cnt) return false;
  }
  return true;
}

// the most source rows a tile of th output rows reaches
int max_tile_rows(const int* b, int oh, int th) {
  int worst = 0;
  for (int y0 = 0; y0 < oh; y0 += th) {
    int lo = b[2 * y0], hi = lo + b[2 * y0 + 1];
    for (int y = y0 + 1; y < y0 + th && y < oh; ++y) {
      lo = b[2 * y] < lo ? b[2 * y] : lo;
      hi = b[2 * y] + b[2 * y + 1] > hi ? b[2 * y] + b[2 * y + 1] : hi;
    }
    worst = hi - lo > worst ? hi - lo : worst;
  }
  return worst;
}

bool misaligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) != 0; }

// both entry points: the checks, the tile height and the launch; `padded` selects the window rule and the instantiation
template <bool PADDED>
int resample(const unsigned char* src, int A, int img_w, int img_h, long long row_pitch, long long image_stride, int x0, int y0, int w,
             int h, int hflip, int vflip, const int* xcoef, const int* xbounds, const int* xbounds_host, int kx, const int* ycoef,
             const int* ybounds, const int* ybounds_host, int ky, int ow, int oh, const float* lut, void* out, int out_u8, void* stream) {
  if (!src || !xcoef || !xbounds || !xbounds_host || !ycoef || !ybounds || !ybounds_host || !out || (!out_u8 && !lut))
    return os2d_refuse("resample: null pointer");
  if (misaligned(xcoef, 4) || misaligned(xbounds, 4) || misaligned(ycoef, 4) || misaligned(ybounds, 4) || misaligned(xbounds_host, 4) ||
      misaligned(ybounds_host, 4) || (!out_u8 && (misaligned(lut, 4) || misaligned(out, 16))))
    return os2d_refuse("resample: pointer not aligned (tables 4 bytes, float output 16 bytes)");
  if (A < 1 || A > 65535 || img_w < 1 || img_h < 1 || w < 1 || h < 1 || ow < 1 || oh < 1 || kx < 1 || ky < 1)
    return os2d_refuse("resample: bad shape (1 <= A <= 65535, sizes and tap counts >= 1)");
  if (row_pitch < 3LL * img_w || (A > 1 && image_stride < row_pitch * img_h))
    return os2d_refuse("resample: bad shape (row pitch below 3 * img_w or image stride below img_h * row pitch)");
  if (PADDED) {
    const int far = 1 << 30;            // x0 + w and y0 + h stay inside int
    if (x0 < -far || y0 < -far || w > far || h > far) return os2d_refuse("resample: bad shape (window beyond 2^30)");
    if (x0 >= img_w || y0 >= img_h || x0 + w <= 0 || y0 + h <= 0) return os2d_refuse("resample: window has no pixel inside the image");
  } else if (x0 < 0 || y0 < 0 || x0 > img_w - w || y0 > img_h - h) {
    return os2d_refuse("resample: window outside the image");
  }
  const long long R = OS2D_RESAMPLE_MAX_RATIO;
  if (w > R * ow || ow > R * w || h > R * oh || oh > R * h) return os2d_refuse("resample: size ratio beyond 16 on an axis");
  if (!bounds_ok(xbounds_host, ow, kx, w) || !bounds_ok(ybounds_host, oh, ky, h))
    return os2d_refuse("resample: table bounds outside the window (0 <= first, 1 <= taps <= k, first + taps <= n)");
  // tile height: the largest whose staged rows fit in LDS (fewer tile rows for strong down-scaling)
  int th = IMG_TH_MAX, nrows = 0;
  for (; th >= 1; th >>= 1) {
    nrows = max_tile_rows(ybounds_host, oh, th);
    if (nrows <= IMG_MAX_ROWS) break;
  }
  if (th < 1) return os2d_refuse("resample: the taps of one output row do not fit in LDS");
  Resample p;
  p.src = src;
  p.row_pitch = row_pitch;
  p.image_stride = image_stride;
  p.img_w = img_w; p.img_h = img_h;
  p.x0 = x0; p.y0 = y0; p.w = w; p.h = h;
  p.hflip = hflip != 0; p.vflip = vflip != 0;
  p.xcoef = xcoef; p.xbounds = xbounds; p.ycoef = ycoef; p.ybounds = ybounds;
  p.kx = kx; p.ky = ky; p.ow = ow; p.oh = oh; p.th = th; p.lds_rows = nrows;
  p.lut = lut;
  p.out = out;
  const dim3 grid((ow + IMG_TW - 1) / IMG_TW, (oh + th - 1) / th, A);
  const size_t lds = (size_t)nrows * 3 * IMG_TW + (out_u8 ? 0 : IMG_LUT_BYTES);
  if (grid.y > 65535) return os2d_refuse("resample: bad shape (output too high)");
  if (out_u8)
    hipLaunchKernelGGL((resample_kernel<true, PADDED>), grid, dim3(IMG_THREADS), lds, os2d_stream(stream), p);
  else
    hipLaunchKernelGGL((resample_kernel<false, PADDED>), grid, dim3(IMG_THREADS), lds, os2d_stream(stream), p);
  return os2d_launched("resample_kernel");
}

}  // namespace

#endif
