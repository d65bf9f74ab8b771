// The last line of a training step on the device (include/os2d_train.h: os2d_train_optim_*), gfx950:
// the gradient norm over every parameter tensor, the clip coefficient and the NaN guard, and the SGD-momentum / Adam update.
//
// Multi-tensor addressing.  One launch serves a TABLE of up to OS2D_TRAIN_OPTIM_MAX_TENSORS tensors, which travels by value in
// the kernel arguments (gradient pointers change every step, so a table in device memory would have to be uploaded again each
// step; the kernarg segment is that upload, and the runtime owns its lifetime).  A work-group of 256 threads owns one CHUNK of
// OS2D_TRAIN_OPTIM_CHUNK = 4096 consecutive elements of one tensor.  Chunks are numbered over all tables of a step; a tensor's
// record carries its first chunk, and a work-group finds its tensor by a binary search over those (scalar loads: the index is
// uniform).  A chunk of a tensor whose pointers are all 16-byte aligned moves 16 bytes per lane and instruction (a wave touches
// 1 KB of consecutive addresses), the others 4 bytes; the tail of a tensor is masked per element.
//
// Norm.  sumsq: every thread adds the squares of its (at most 16) elements in double - an fp32 square is exact in double - the
// work-group adds its 256 sums in a fixed order and writes ONE double per chunk: no atomics.  finalize: one work-group adds the
// partials in index order (256 consecutive runs, then the 256 run sums in order) and writes the step's record: norm, coef, skip.
//
// Update.  g *= coef is written back; unless the record says skip, the parameter and its state are updated operation by
// operation in fp32: every function that rounds switches contraction off itself (the unit carries no -ffp-contract=off), and
// division and square root are the correctly rounded ones (hipcc's default; the ISA shows v_div_scale / v_div_fmas / v_div_fixup
// and the scaled v_sqrt_f32 with its two fma corrections, not v_rcp_f32 / a bare v_sqrt_f32).
//
// Step counts are device state (Adam).  prepare, one thread per tensor, runs between finalize and update: it advances the
// tensor's count unless the step is skipped and writes the two factors the update reads, so no work-group of the update reads a
// count that another one of the same launch writes.
#include <math.h>
#include <stdint.h>

#include "../../include/os2d_train.h"
#include "../csrc/os2d_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = OS2D_TRAIN_OPTIM_CHUNK;
constexpr int MAX_TENSORS = OS2D_TRAIN_OPTIM_MAX_TENSORS;
constexpr int PER_THREAD = CHUNK / THREADS;          // 16 elements = 4 x 16 bytes
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is whole 16-byte groups per thread");

typedef os2d_train_optim_tensor Tensor;
struct Table {
  Tensor t[MAX_TENSORS];
};
// the table and the few scalars next to it stay within the 4 KB of kernel arguments that every HIP runtime accepts
static_assert(sizeof(Tensor) == 64, "record layout (os2d_amd/_train_lib.py mirrors it)");
static_assert(sizeof(Table) + 128 <= 4096, "kernel arguments within 4 KB");

// the tensor that owns chunk c: the LAST record with first_chunk <= c (records without elements share the first chunk of
// their successor, or lie past the launch's last chunk)
__device__ __forceinline__ int find_tensor(const Table& tab, int n, int c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.t[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 256 doubles -> one, in a fixed order: lanes of a wave by halving distances, then the four waves in order
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid: x = the table's chunks; chunk_base = first chunk of the table
__global__ __launch_bounds__(THREADS) void optim_sumsq_kernel(const Table tab, int n, int chunk_base, double* __restrict__ partials) {
  __shared__ double lds[THREADS / 64];
  const int c = chunk_base + blockIdx.x;
  const Tensor& t = tab.t[find_tensor(tab, n, c)];
  const long long base = (long long)(c - t.first_chunk) * CHUNK;
  const long long left = t.numel - base;             // >= 1
  const float* __restrict__ g = t.grad + base;
  double acc = 0.0;
  if (t.aligned) {
#pragma unroll
    for (int k = 0; k < PER_THREAD / 4; ++k) {
      const int e = (k * THREADS + threadIdx.x) * 4;
      if (e + 4 <= left) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)v[j] * (double)v[j];
      } else {
        for (int j = 0; j < 4; ++j)
          if (e + j < left) acc += (double)g[e + j] * (double)g[e + j];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
      const int e = k * THREADS + threadIdx.x;
      if (e < left) acc += (double)g[e] * (double)g[e];
    }
  }
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[c] = s;
}

// one work-group: record = {norm, coef, skip, 0}
__global__ __launch_bounds__(THREADS) void optim_finalize_kernel(const double* __restrict__ partials, long long count, float max_norm,
                                                                 float* __restrict__ record) {
#pragma clang fp contract(off)
  __shared__ double runs[THREADS];
  const long long len = (count + THREADS - 1) / THREADS;
  const long long b = threadIdx.x * len;
  const long long e = b + len < count ? b + len : count;
  double acc = 0.0;
  for (long long i = b; i < e; ++i) acc += partials[i];
  runs[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < THREADS; ++i) sum += runs[i];
  const float norm = (float)sqrt(sum);
  float coef = 1.0f;
  if (max_norm < INFINITY) {                         // an infinite max_norm: no clipping
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;                      // a NaN norm stays a NaN coefficient, as torch.clamp(max=1) leaves it
  }
  record[0] = norm;
  record[1] = coef;
  record[2] = norm != norm ? 1.0f : 0.0f;
  record[3] = 0.0f;
}

// beta^t for a whole t >= 1 by squaring, in double
__device__ __forceinline__ double pow_whole(double beta, unsigned t) {
#pragma clang fp contract(off)
  double r = 1.0, b = beta;
  for (; t; t >>= 1) {
    if (t & 1) r *= b;
    b *= b;
  }
  return r;
}

// one thread per tensor of the table (Adam): advance the count, write factors[2 i] = lr / bc1, factors[2 i + 1] = sqrt(bc2)
__global__ __launch_bounds__(64) void optim_prepare_kernel(const Table tab, int n, const float* __restrict__ record, double beta1, double beta2,
                                                           float* __restrict__ factors) {
#pragma clang fp contract(off)
  const int i = threadIdx.x;
  if (i >= n || record[2] != 0.0f) return;
  const Tensor& t = tab.t[i];
  const float step = *t.step + 1.0f;
  *t.step = step;
  const unsigned whole = (unsigned)step;
  factors[2 * i] = (float)((double)t.lr / (1.0 - pow_whole(beta1, whole)));
  factors[2 * i + 1] = (float)sqrt(1.0 - pow_whole(beta2, whole));
}

struct Hyper {       // what every element of a launch shares
  float mu;          // SGD: momentum
  float b2, omb1, omb2, eps;     // Adam: beta2, 1 - beta1, 1 - beta2 (each rounded once from double), eps
};

// one element of SGD with momentum (dampening 0, no Nesterov); buf is not touched when mu == 0
__device__ __forceinline__ void sgd_element(float g, float& p, float& buf, float lr, float wd, float mu) {
#pragma clang fp contract(off)
  float d = g;
  if (wd != 0.0f) d = g + wd * p;
  if (mu != 0.0f) {
    buf = mu * buf + d;
    d = buf;
  }
  p = p - lr * d;
}

// one element of Adam (L2 weight decay, no amsgrad); step_size = lr / bc1, sqrt_bc2 from prepare
__device__ __forceinline__ void adam_element(float g, float& p, float& m, float& v, float wd, float step_size, float sqrt_bc2, const Hyper& h) {
#pragma clang fp contract(off)
  float d = g;
  if (wd != 0.0f) d = g + wd * p;
  m = m + (d - m) * h.omb1;
  v = h.b2 * v + (h.omb2 * d) * d;
  const float den = sqrtf(v) / sqrt_bc2 + h.eps;
  p = p - step_size * (m / den);
}

__device__ __forceinline__ float scaled(float g, float coef) {
#pragma clang fp contract(off)
  return g * coef;
}

// ADAM: false = SGD.  STATE: SGD only, false = no momentum buffer (mu == 0).  VEC: 16-byte accesses.
template <bool ADAM, bool VEC>
__device__ __forceinline__ void update_chunk(const Tensor& t, long long base, long long left, float coef, bool skip, float f0, float f1,
                                             const Hyper& h) {
  float* __restrict__ gp = t.grad + base;
  float* __restrict__ pp = t.param + base;
  float* __restrict__ s1 = t.state1 ? t.state1 + base : nullptr;
  float* __restrict__ s2 = ADAM ? t.state2 + base : nullptr;
  const float lr = t.lr, wd = t.weight_decay;
  const bool has1 = s1 != nullptr;
  constexpr int W = VEC ? 4 : 1;
#pragma unroll
  for (int k = 0; k < PER_THREAD / W; ++k) {
    const int e = (k * THREADS + threadIdx.x) * W;
    if (e >= left) continue;
    if (VEC && e + 4 <= left) {
      f32x4 g = *reinterpret_cast<const f32x4*>(gp + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = scaled(g[j], coef);
      *reinterpret_cast<f32x4*>(gp + e) = g;
      if (skip) continue;
      f32x4 p = *reinterpret_cast<const f32x4*>(pp + e);
      f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
      if (has1) a = *reinterpret_cast<const f32x4*>(s1 + e);
      if (ADAM) b = *reinterpret_cast<const f32x4*>(s2 + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], aj = a[j], bj = b[j];
        if (ADAM) adam_element(g[j], pj, aj, bj, wd, f0, f1, h);
        else sgd_element(g[j], pj, aj, lr, wd, has1 ? h.mu : 0.0f);
        p[j] = pj, a[j] = aj, b[j] = bj;
      }
      *reinterpret_cast<f32x4*>(pp + e) = p;
      if (has1) *reinterpret_cast<f32x4*>(s1 + e) = a;
      if (ADAM) *reinterpret_cast<f32x4*>(s2 + e) = b;
    } else {
      for (int j = 0; j < W; ++j) {
        if (e + j >= left) break;
        const float g = scaled(gp[e + j], coef);
        gp[e + j] = g;
        if (skip) continue;
        float p = pp[e + j], a = has1 ? s1[e + j] : 0.0f, b = ADAM ? s2[e + j] : 0.0f;
        if (ADAM) adam_element(g, p, a, b, wd, f0, f1, h);
        else sgd_element(g, p, a, lr, wd, has1 ? h.mu : 0.0f);
        pp[e + j] = p;
        if (has1) s1[e + j] = a;
        if (ADAM) s2[e + j] = b;
      }
    }
  }
}

// grid: x = the table's chunks.  factors: the table's [n][2] floats of prepare (Adam), else not read
template <bool ADAM>
__global__ __launch_bounds__(THREADS) void optim_update_kernel(const Table tab, int n, int chunk_base, const float* __restrict__ record,
                                                               const float* __restrict__ factors, const Hyper h) {
  const int c = chunk_base + blockIdx.x;
  const int i = find_tensor(tab, n, c);
  const Tensor& t = tab.t[i];
  const long long base = (long long)(c - t.first_chunk) * CHUNK;
  const long long left = t.numel - base;
  const float coef = record[1];
  const bool skip = record[2] != 0.0f;
  float f0 = 0.0f, f1 = 1.0f;
  if (ADAM && !skip) f0 = factors[2 * i], f1 = factors[2 * i + 1];
  if (t.aligned) update_chunk<ADAM, true>(t, base, left, coef, skip, f0, f1, h);
  else update_chunk<ADAM, false>(t, base, left, coef, skip, f0, f1, h);
}

size_t chunks_of(long long numel) { return numel <= 0 ? 0 : (size_t)((numel + CHUNK - 1) / CHUNK); }

// The checks every table entry point shares.  -> 0 and *chunks = the table's chunk count, or the refusal's code.  `need`: which
// of state1 (1), state2 (2), step (4) a tensor with elements must carry
int check_table(const char* who, const Tensor* tensors, int n, int need, size_t* chunks) {
  if (n < 0 || n > MAX_TENSORS) return OS2D_REFUSE(-1, "%s: %d tensors (need 0 .. %d per table)", who, n, MAX_TENSORS);
  if (n > 0 && !tensors) return OS2D_REFUSE(-1, "%s: null pointer (tensors)", who);
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const Tensor& t = tensors[i];
    if (t.numel < 0) return OS2D_REFUSE(-1, "%s: tensor %d has negative numel %lld", who, i, t.numel);
    if (t.first_chunk < 0 || (i > 0 && (size_t)t.first_chunk != (size_t)tensors[0].first_chunk + total))
      return OS2D_REFUSE(-1, "%s: tensor %d starts at chunk %d, its predecessors end at %zu", who, i, t.first_chunk,
                         (size_t)tensors[0].first_chunk + total);
    if (t.numel > 0) {
      if (!t.param || !t.grad || ((need & 1) && !t.state1) || ((need & 2) && !t.state2) || ((need & 4) && !t.step))
        return OS2D_REFUSE(-1, "%s: null pointer (tensor %d)", who, i);
      const uintptr_t bits = reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                             reinterpret_cast<uintptr_t>(t.state1) | reinterpret_cast<uintptr_t>(t.state2);
      if (bits & 3) return OS2D_REFUSE(-1, "%s: tensor %d has a pointer that is not 4-byte aligned", who, i);
      if ((t.aligned != 0 && t.aligned != 1) || (t.aligned && (bits & 15)))
        return OS2D_REFUSE(-1, "%s: tensor %d is marked 16-byte aligned (%d) and is not", who, i, t.aligned);
    }
    total += chunks_of(t.numel);
    if ((size_t)tensors[0].first_chunk + total > 0x7fffffffu) return OS2D_REFUSE(-1, "%s: more than 2^31 chunks", who);
  }
  *chunks = total;
  return 0;
}

Table table_of(const Tensor* tensors, int n) {
  Table tab;
  for (int i = 0; i < MAX_TENSORS; ++i) tab.t[i] = tensors[i < n ? i : n - 1];     // (padding records are never read)
  return tab;
}

}  // namespace

extern "C" int os2d_train_optim_max_tensors(void) { return MAX_TENSORS; }

extern "C" size_t os2d_train_optim_chunks(long long numel) { return chunks_of(numel); }

extern "C" int os2d_train_optim_sumsq(const os2d_train_optim_tensor* tensors, int n, double* partials, size_t partials_count, void* stream) {
  size_t chunks = 0;
  if (const int rc = check_table("os2d_train_optim_sumsq", tensors, n, 0, &chunks)) return rc;
  if (!partials) return os2d_refuse("os2d_train_optim_sumsq: null pointer (partials)");
  if (chunks == 0) return 0;
  const size_t first = (size_t)tensors[0].first_chunk;
  if (first + chunks > partials_count)
    return OS2D_REFUSE(-2, "os2d_train_optim_sumsq: partials holds %zu doubles, the table ends at chunk %zu", partials_count, first + chunks);
  hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, os2d_stream(stream), table_of(tensors, n), n, (int)first,
                     partials);
  return os2d_launched("optim_sumsq_kernel");
}

extern "C" int os2d_train_optim_finalize(const double* partials, size_t partials_count, float max_norm, float* record, void* stream) {
  if (!record || (partials_count > 0 && !partials)) return os2d_refuse("os2d_train_optim_finalize: null pointer");
  if (!(max_norm > 0.0f)) return OS2D_REFUSE(-1, "os2d_train_optim_finalize: max_norm=%g (need > 0; infinity = no clipping)", (double)max_norm);
  hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(THREADS), 0, os2d_stream(stream), partials, (long long)partials_count, max_norm,
                     record);
  return os2d_launched("optim_finalize_kernel");
}

extern "C" int os2d_train_optim_prepare(const os2d_train_optim_tensor* tensors, int n, const float* record, double beta1, double beta2,
                                        float* factors, void* stream) {
  size_t chunks = 0;
  if (const int rc = check_table("os2d_train_optim_prepare", tensors, n, 4, &chunks)) return rc;
  if (!record || !factors) return os2d_refuse("os2d_train_optim_prepare: null pointer");
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
    return OS2D_REFUSE(-1, "os2d_train_optim_prepare: betas (%g, %g) outside [0, 1)", beta1, beta2);
  for (int i = 0; i < n; ++i)       // a record without elements is counted too: it had a gradient
    if (!tensors[i].step) return OS2D_REFUSE(-1, "os2d_train_optim_prepare: null pointer (step of tensor %d)", i);
  if (n == 0) return 0;
  static_assert(MAX_TENSORS <= 64, "prepare is one wave");
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(64), 0, os2d_stream(stream), table_of(tensors, n), n, record, beta1, beta2, factors);
  return os2d_launched("optim_prepare_kernel");
}

extern "C" int os2d_train_optim_update(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const float* factors,
                                       double momentum_or_beta1, double beta2, double eps, void* stream) {
  if (method != OS2D_TRAIN_OPTIM_SGD && method != OS2D_TRAIN_OPTIM_ADAM)
    return OS2D_REFUSE(-1, "os2d_train_optim_update: method=%d (0 SGD, 1 Adam)", method);
  const bool adam = method == OS2D_TRAIN_OPTIM_ADAM;
  const bool momentum = !adam && momentum_or_beta1 != 0.0;
  size_t chunks = 0;
  if (const int rc = check_table("os2d_train_optim_update", tensors, n, adam ? 3 : (momentum ? 1 : 0), &chunks)) return rc;
  if (!record || (adam && !factors)) return os2d_refuse("os2d_train_optim_update: null pointer");
  Hyper h = {};
  if (adam) {
    if (!(momentum_or_beta1 >= 0.0 && momentum_or_beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0))
      return OS2D_REFUSE(-1, "os2d_train_optim_update: betas (%g, %g) outside [0, 1) or eps=%g < 0", momentum_or_beta1, beta2, eps);
    h.b2 = (float)beta2, h.omb1 = (float)(1.0 - momentum_or_beta1), h.omb2 = (float)(1.0 - beta2), h.eps = (float)eps;
  } else {
    if (!(momentum_or_beta1 >= 0.0)) return OS2D_REFUSE(-1, "os2d_train_optim_update: momentum=%g < 0", momentum_or_beta1);
    h.mu = (float)momentum_or_beta1;
  }
  if (chunks == 0) return 0;
  Table tab = table_of(tensors, n);
  if (!adam)
    for (int i = 0; i < n; ++i) {
      if (!momentum) tab.t[i].state1 = nullptr;      // the kernel takes a null buffer for "no momentum"
      tab.t[i].state2 = nullptr;
    }
  const int first = tensors[0].first_chunk;
  if (adam)
    hipLaunchKernelGGL(optim_update_kernel<true>, dim3((unsigned)chunks), dim3(THREADS), 0, os2d_stream(stream), tab, n, first, record, factors, h);
  else
    hipLaunchKernelGGL(optim_update_kernel<false>, dim3((unsigned)chunks), dim3(THREADS), 0, os2d_stream(stream), tab, n, first, record, factors, h);
  return os2d_launched("optim_update_kernel");
}
