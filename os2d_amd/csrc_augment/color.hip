// libos2d_augment.so: colour distortion of an 8-bit RGB image with PIL's bits (include/os2d_augment.h) - the
// chain brightness / contrast / saturation / hue that torchvision's ColorJitter runs on a PIL image, then either the bytes or
// the normalised float planes (ToTensor + Normalize as a table lookup, as in resample.hip).
//
//   color_kernel        thread = a group of 4 consecutive pixels (row-major over the image): the whole chain per pixel, then
//                       12 bytes, or per channel one 16-byte unit of the float plane where the plane's start makes the group a
//                       whole unit (else, and for the last partial group, element by element)
//   color_luma_kernel   only for a chain with a contrast operation: the operations before it are pointwise, so they are
//                       recomputed; every work-group writes the integer sum of the luma of its pixels to its own slot.  The
//                       slots are summed again by every work-group of color_kernel: integers, the same bits in any order, no
//                       atomics, nothing to clear, and the mean never visits the host.
// Every function that rounds switches contraction off itself: a fused multiply-add would round differently from PIL's C.
#include "../csrc_image/image_common.h"
#include "../../include/os2d_augment.h"

namespace {

static_assert(OS2D_AUGMENT_COLOR_SLOTS == IMG_THREADS, "color_kernel: one thread sums one slot");

struct ColorChain {
  int n, contrast_at;                       // contrast_at: index of the contrast operation, or n
  int kind[OS2D_AUGMENT_COLOR_MAX_OPS];
  float f[OS2D_AUGMENT_COLOR_MAX_OPS];        // blend factor
  int clip[OS2D_AUGMENT_COLOR_MAX_OPS];       // blend outside [0, 1]: clip before the truncation
  int shift[OS2D_AUGMENT_COLOR_MAX_OPS];      // hue: what is added to H
};

struct Color {
  const unsigned char* src;
  long long row_pitch, npix;
  int w, h;
  ColorChain chain;
  const float* lut;
  void* out;
  unsigned long long* sums;
  int slots;
};

struct Rgb {
  int r, g, b;
};

__device__ __forceinline__ int luma(const Rgb c) { return (19595 * c.r + 38470 * c.g + 7471 * c.b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) of one byte: (UINT8)(d + f * (i - d)) in float
__device__ __forceinline__ int blend(int d, int i, float f, int clip) {
#pragma clang fp contract(off)
  const float prod = f * (float)(i - d);
  const float t = (float)d + prod;
  if (clip) return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
  return (int)t & 255;
}

__device__ __forceinline__ Rgb blend3(int d, const Rgb c, float f, int clip) {
  return Rgb{blend(d, c.r, f, clip), blend(d, c.g, f, clip), blend(d, c.b, f, clip)};
}

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// PIL's rgb2hsv_row: -> (H, S, V) bytes
__device__ __forceinline__ Rgb rgb_to_hsv(const Rgb c) {
#pragma clang fp contract(off)
  const int maxc = max(c.r, max(c.g, c.b)), minc = min(c.r, min(c.g, c.b));
  if (maxc == minc) return Rgb{0, 0, maxc};
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - c.r) / cr, gc = (float)(maxc - c.g) / cr, bc = (float)(maxc - c.b) / cr;
  float h;
  if (c.r == maxc)
    h = (float)((double)bc - (double)gc);
  else if (c.g == maxc)
    h = (float)(2.0 + (double)rc - (double)bc);
  else
    h = (float)(4.0 + (double)gc - (double)rc);
  const double turn = (double)h / 6.0 + 1.0;               // in (0.8, 2): fmod(turn, 1.0) is turn - floor(turn), exactly
  h = (float)(turn - floor(turn));
  return Rgb{clip255((int)((double)h * 255.0)), clip255((int)((double)s * 255.0)), maxc};
}

// PIL's hsv2rgb_row
__device__ __forceinline__ Rgb hsv_to_rgb(const Rgb hsv) {
#pragma clang fp contract(off)
  const int v = hsv.b;
  if (hsv.g == 0) return Rgb{v, v, v};
  const double fh = (double)hsv.r * 6.0 / 255.0;
  const double fl = floor(fh);
  const int i = (int)fl;
  const float f = (float)(fh - fl);
  const float fs = (float)hsv.g / 255.0f;
  const float fv = (float)v;
  const int p = clip255((int)__builtin_rintf(fv * (1.0f - fs)));
  const int q = clip255((int)__builtin_rintf(fv * (1.0f - fs * f)));
  const int t = clip255((int)__builtin_rintf(fv * (1.0f - fs * (1.0f - f))));
  switch (i % 6) {
    case 0: return Rgb{v, t, p};
    case 1: return Rgb{q, v, p};
    case 2: return Rgb{p, v, t};
    case 3: return Rgb{p, q, v};
    case 4: return Rgb{t, p, v};
    default: return Rgb{v, p, q};
  }
}

// operations [first, last) of the chain on one pixel; mean: the degenerate value of the contrast operation
__device__ __forceinline__ Rgb apply_chain(Rgb c, const ColorChain& ch, int first, int last, int mean) {
#pragma unroll
  for (int k = 0; k < OS2D_AUGMENT_COLOR_MAX_OPS; ++k) {
    if (k < first || k >= last) continue;
    const int kind = ch.kind[k];
    if (kind == OS2D_AUGMENT_COLOR_BRIGHTNESS) {
      c = blend3(0, c, ch.f[k], ch.clip[k]);
    } else if (kind == OS2D_AUGMENT_COLOR_SATURATION) {
      c = blend3(luma(c), c, ch.f[k], ch.clip[k]);
    } else if (kind == OS2D_AUGMENT_COLOR_CONTRAST) {
      c = blend3(mean, c, ch.f[k], ch.clip[k]);
    } else if (kind == OS2D_AUGMENT_COLOR_HUE) {
      Rgb hsv = rgb_to_hsv(c);
      hsv.r = (hsv.r + ch.shift[k]) & 255;
      c = hsv_to_rgb(hsv);
    } else if (kind == OS2D_AUGMENT_COLOR_TO_HSV) {
      c = rgb_to_hsv(c);
    } else if (kind == OS2D_AUGMENT_COLOR_FROM_HSV) {
      c = hsv_to_rgb(c);
    }
  }
  return c;
}

__device__ __forceinline__ Rgb load_pixel(const Color& p, long long i) {
  const long long y = i / p.w;
  const unsigned char* px = p.src + y * p.row_pitch + (i - y * p.w) * 3;
  return Rgb{px[0], px[1], px[2]};
}

// sum over the work-group (every thread gets it); `part` is IMG_THREADS words of LDS
__device__ __forceinline__ unsigned long long group_sum(unsigned long long v, unsigned long long* part) {
  part[threadIdx.x] = v;
  __syncthreads();
  for (int s = IMG_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  const unsigned long long total = part[0];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(IMG_THREADS) void color_luma_kernel(const Color p) {
  __shared__ unsigned long long part[IMG_THREADS];
  unsigned long long acc = 0;
  for (long long i = (long long)blockIdx.x * IMG_THREADS + threadIdx.x; i < p.npix; i += (long long)p.slots * IMG_THREADS)
    acc += (unsigned long long)luma(apply_chain(load_pixel(p, i), p.chain, 0, p.chain.contrast_at, 0));
  const unsigned long long total = group_sum(acc, part);
  if (threadIdx.x == 0) p.sums[blockIdx.x] = total;
}

template <bool U8OUT>
__global__ __launch_bounds__(IMG_THREADS) void color_kernel(const Color p) {
  __shared__ unsigned long long part[IMG_THREADS];
  __shared__ float lut[U8OUT ? 1 : 3 * 256];
  const int tid = threadIdx.x;
  if (!U8OUT)
    for (int i = tid; i < 3 * 256; i += IMG_THREADS) lut[i] = p.lut[i];
  int mean = 0;
  if (p.chain.contrast_at < p.chain.n) {            // ImageEnhance.Contrast: int(mean of L + 0.5)
    const unsigned long long total = group_sum(tid < p.slots ? p.sums[tid] : 0ull, part);
    mean = (int)((double)total / (double)p.npix + 0.5);
  }
  __syncthreads();

  const long long first = ((long long)blockIdx.x * IMG_THREADS + tid) * 4;
  if (first >= p.npix) return;
  const int count = (int)min(4ll, p.npix - first);
  int v[3][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const Rgb c = apply_chain(load_pixel(p, min(first + q, p.npix - 1)), p.chain, 0, p.chain.n, mean);
    v[0][q] = c.r;
    v[1][q] = c.g;
    v[2][q] = c.b;
  }
  if (U8OUT) {
    unsigned char* out = static_cast<unsigned char*>(p.out) + first * 3;
    if (count == 4 && (reinterpret_cast<size_t>(p.out) & 3) == 0) {          // 12 bytes at a multiple of 12
      unsigned int* o32 = reinterpret_cast<unsigned int*>(out);
      o32[0] = v[0][0] | v[1][0] << 8 | v[2][0] << 16 | (unsigned)v[0][1] << 24;
      o32[1] = v[1][1] | v[2][1] << 8 | v[0][2] << 16 | (unsigned)v[1][2] << 24;
      o32[2] = v[2][2] | v[0][3] << 8 | v[1][3] << 16 | (unsigned)v[2][3] << 24;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < count) {
          out[3 * q] = (unsigned char)v[0][q];
          out[3 * q + 1] = (unsigned char)v[1][q];
          out[3 * q + 2] = (unsigned char)v[2][q];
        }
    }
  } else {
    float* out = static_cast<float*>(p.out);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* lc = lut + c * 256;
      float* dst = out + c * p.npix + first;
      if (count == 4 && ((c * p.npix) & 3) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(lc[v[c][0]], lc[v[c][1]], lc[v[c][2]], lc[v[c][3]]);
      } else {                                      // a plane that starts inside a unit, or the image's last pixels
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < count) dst[q] = lc[v[c][q]];
      }
    }
  }
}

bool misaligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int os2d_augment_color(const unsigned char* src, int w, int h, long long row_pitch, int n_ops, const int* kinds,
                                const double* factors, const float* lut, void* out, int out_u8, unsigned long long* sums, void* stream) {
  if (n_ops < 0 || n_ops > OS2D_AUGMENT_COLOR_MAX_OPS) return os2d_refuse("color: more than 4 operations (or fewer than 0)");
  if (!src || !out || (!out_u8 && !lut) || (n_ops > 0 && (!kinds || !factors))) return os2d_refuse("color: null pointer");
  if (w < 1 || h < 1 || (long long)w * h > (1ll << 30) || row_pitch < 3ll * w)
    return os2d_refuse("color: bad shape (sizes >= 1, at most 2^30 pixels, row pitch at least 3 * w)");
  if (!out_u8 && (misaligned(lut, 4) || misaligned(out, 16))) return os2d_refuse("color: pointer not aligned (table 4 bytes, float output 16 bytes)");
  Color p;
  p.chain.n = n_ops;
  p.chain.contrast_at = n_ops;
  for (int k = 0; k < OS2D_AUGMENT_COLOR_MAX_OPS; ++k) {
    p.chain.kind[k] = 0; p.chain.f[k] = 1.0f; p.chain.clip[k] = 0; p.chain.shift[k] = 0;
    if (k >= n_ops) continue;
    const int kind = kinds[k];
    const double f = factors[k];
    if (kind < OS2D_AUGMENT_COLOR_BRIGHTNESS || kind > OS2D_AUGMENT_COLOR_FROM_HSV) return os2d_refuse("color: unknown operation kind");
    if (!(f >= -1e6 && f <= 1e6)) return os2d_refuse("color: factor is not a number within +-1e6");
    if (kind == OS2D_AUGMENT_COLOR_CONTRAST) {
      if (p.chain.contrast_at < n_ops) return os2d_refuse("color: more than one contrast operation in a chain");
      p.chain.contrast_at = k;
    }
    p.chain.kind[k] = kind;
    if (kind == OS2D_AUGMENT_COLOR_HUE) {
      p.chain.shift[k] = (int)(f * 255.0) & 255;
    } else if (kind < OS2D_AUGMENT_COLOR_HUE) {
      p.chain.f[k] = (float)f;
      p.chain.clip[k] = !(p.chain.f[k] >= 0.0f && p.chain.f[k] <= 1.0f);
    }
  }
  const bool contrast = p.chain.contrast_at < n_ops;
  if (contrast && !sums) return os2d_refuse("color: null pointer (a chain with contrast needs the workspace of the mean)");
  if (contrast && misaligned(sums, 8)) return os2d_refuse("color: pointer not aligned (workspace 8 bytes)");
  p.src = src;
  p.row_pitch = row_pitch;
  p.w = w; p.h = h;
  p.npix = (long long)w * h;
  p.lut = lut;
  p.out = out;
  p.sums = sums;
  const long long groups = (p.npix + 3) / 4;
  const unsigned blocks = (unsigned)((groups + IMG_THREADS - 1) / IMG_THREADS);
  const long long per_slot = (p.npix + IMG_THREADS - 1) / IMG_THREADS;
  p.slots = (int)(per_slot < OS2D_AUGMENT_COLOR_SLOTS ? per_slot : OS2D_AUGMENT_COLOR_SLOTS);
  if (contrast) {
    hipLaunchKernelGGL(color_luma_kernel, dim3(p.slots), dim3(IMG_THREADS), 0, os2d_stream(stream), p);
    const int rc = os2d_launched("color_luma_kernel");
    if (rc) return rc;
  }
  if (out_u8)
    hipLaunchKernelGGL(color_kernel<true>, dim3(blocks), dim3(IMG_THREADS), 0, os2d_stream(stream), p);
  else
    hipLaunchKernelGGL(color_kernel<false>, dim3(blocks), dim3(IMG_THREADS), 0, os2d_stream(stream), p);
  return os2d_launched("color_kernel");
}
