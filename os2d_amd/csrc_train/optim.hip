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
//
// The other six methods (Adagrad, Adadelta, Adamax, ASGD, RMSprop, Rprop: prepare_ex / update_ex) share all of this: the same
// chunk loop with another element function, and a prepare that writes OS2D_TRAIN_OPTIM_FACTORS floats per tensor.  ASGD's eta and
// mu are functions of the count alone: prepare_ex hands the update the pair the previous step left and writes the next one.
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

// What one element does is an OP: op(g, p, a, b) updates the parameter and its (at most two) state values from the clipped
// gradient.  OP::STATE2: the method keeps a second per-element state tensor; op.has1: state1 is read and written (SGD without
// momentum has none).  VEC: 16-byte accesses.
template <bool VEC, class OP>
__device__ __forceinline__ void update_chunk(const Tensor& t, long long base, long long left, float coef, bool skip, const OP& op) {
  float* __restrict__ gp = t.grad + base;
  float* __restrict__ pp = t.param + base;
  float* __restrict__ s1 = t.state1 ? t.state1 + base : nullptr;
  float* __restrict__ s2 = OP::STATE2 ? t.state2 + base : nullptr;
  const bool has1 = op.has1;
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
      if (OP::STATE2) b = *reinterpret_cast<const f32x4*>(s2 + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], aj = a[j], bj = b[j];
        op(g[j], pj, aj, bj);
        p[j] = pj, a[j] = aj, b[j] = bj;
      }
      *reinterpret_cast<f32x4*>(pp + e) = p;
      if (has1) *reinterpret_cast<f32x4*>(s1 + e) = a;
      if (OP::STATE2) *reinterpret_cast<f32x4*>(s2 + e) = b;
    } else {
      for (int j = 0; j < W; ++j) {
        if (e + j >= left) break;
        const float g = scaled(gp[e + j], coef);
        gp[e + j] = g;
        if (skip) continue;
        float p = pp[e + j], a = has1 ? s1[e + j] : 0.0f, b = OP::STATE2 ? s2[e + j] : 0.0f;
        op(g, p, a, b);
        pp[e + j] = p;
        if (has1) s1[e + j] = a;
        if (OP::STATE2) s2[e + j] = b;
      }
    }
  }
}

struct SgdOp {
  static constexpr bool STATE2 = false;
  float lr, wd, mu;
  bool has1;
  __device__ __forceinline__ void operator()(float g, float& p, float& a, float&) const { sgd_element(g, p, a, lr, wd, has1 ? mu : 0.0f); }
};

struct AdamOp {
  static constexpr bool STATE2 = true;
  static constexpr bool has1 = true;
  float wd, f0, f1;
  const Hyper& h;
  __device__ __forceinline__ void operator()(float g, float& p, float& m, float& v) const { adam_element(g, p, m, v, wd, f0, f1, h); }
};

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
  if (ADAM) {
    float f0 = 0.0f, f1 = 1.0f;
    if (!skip) f0 = factors[2 * i], f1 = factors[2 * i + 1];
    const AdamOp op = {t.weight_decay, f0, f1, h};
    if (t.aligned) update_chunk<true>(t, base, left, coef, skip, op);
    else update_chunk<false>(t, base, left, coef, skip, op);
  } else {
    const SgdOp op = {t.lr, t.weight_decay, h.mu, t.state1 != nullptr};
    if (t.aligned) update_chunk<true>(t, base, left, coef, skip, op);
    else update_chunk<false>(t, base, left, coef, skip, op);
  }
}

// ---- the other six methods of torch.optim that the reference offers (include/os2d_train.h: os2d_train_optim_*_ex)

constexpr int FACTORS = OS2D_TRAIN_OPTIM_FACTORS;      // floats per tensor that prepare_ex writes

// one thread per tensor of the table: unless the step is skipped, advance the count and write what depends on it.  h0 .. h2: the
// method's hyperparameters that prepare needs, in double (Adagrad: lr_decay; Adamax: beta1; ASGD: lambd, alpha, t0)
__global__ __launch_bounds__(64) void optim_prepare_ex_kernel(const Table tab, int n, int method, const float* __restrict__ record, double h0,
                                                              double h1, double h2, float* __restrict__ factors) {
#pragma clang fp contract(off)
  const int i = threadIdx.x;
  if (i >= n || record[2] != 0.0f) return;
  const Tensor& t = tab.t[i];
  const float stepf = *t.step + 1.0f;
  *t.step = stepf;
  const double step = (double)stepf, lr = (double)t.lr;
  float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
  if (method == OS2D_TRAIN_OPTIM_ADAGRAD) {
    f0 = (float)(lr / (1.0 + (step - 1.0) * h0));
  } else if (method == OS2D_TRAIN_OPTIM_ADAMAX) {
    f0 = (float)(lr / (1.0 - pow_whole(h0, (unsigned)stepf)));
  } else if (method == OS2D_TRAIN_OPTIM_ASGD) {
    // this step runs with the eta and mu the previous one left (state2 = {eta, mu}); the next step's follow from the new count
    float* __restrict__ eta_mu = t.state2;
    const float eta = eta_mu[0], mu = eta_mu[1];
    f0 = (float)(1.0 - h0 * (double)eta), f1 = eta, f2 = mu;
    const double rest = step - h2;
    eta_mu[0] = (float)(lr / pow(1.0 + h0 * lr * step, h1));
    eta_mu[1] = (float)(1.0 / (rest > 1.0 ? rest : 1.0));
  }
  float* __restrict__ f = factors + FACTORS * i;
  f[0] = f0, f[1] = f1, f[2] = f2, f[3] = 0.0f;
}

struct HyperEx {     // the method's hyperparameters the update needs, each rounded once from double
  float v0, v1, v2, v3;
};

// One element of method M.  a, b: the method's state1 / state2 value; f0 .. f2: the tensor's factors of prepare_ex.
//   Adagrad   a sum;  f0 clr;  v0 eps                          Adadelta  a square_avg, b acc_delta;  v0 rho, v1 1 - rho, v2 eps
//   Adamax    a exp_avg, b exp_inf;  f0 lr / bc1;  v0 1 - beta1, v1 beta2, v2 eps
//   ASGD      a ax;  f0 1 - lambd eta, f1 eta, f2 mu           RMSprop   a square_avg;  v0 alpha, v1 1 - alpha, v2 eps
//   Rprop     a prev, b step_size;  v0 etaminus, v1 etaplus, v2 / v3 the smallest / largest step size
template <int M>
struct MethodOp {
  static constexpr bool STATE2 = M == OS2D_TRAIN_OPTIM_ADADELTA || M == OS2D_TRAIN_OPTIM_ADAMAX || M == OS2D_TRAIN_OPTIM_RPROP;
  static constexpr bool has1 = true;
  float lr, wd, f0, f1, f2;
  const HyperEx& h;
  __device__ __forceinline__ void operator()(float g, float& p, float& a, float& b) const {
#pragma clang fp contract(off)
    float d = g;
    if (M != OS2D_TRAIN_OPTIM_RPROP && wd != 0.0f) d = g + wd * p;
    if (M == OS2D_TRAIN_OPTIM_ADAGRAD) {
      a = a + d * d;
      p = p - f0 * (d / (sqrtf(a) + h.v0));
    } else if (M == OS2D_TRAIN_OPTIM_ADADELTA) {
      a = h.v0 * a + (h.v1 * d) * d;
      const float delta = sqrtf(b + h.v2) / sqrtf(a + h.v2) * d;
      b = h.v0 * b + (h.v1 * delta) * delta;
      p = p - lr * delta;
    } else if (M == OS2D_TRAIN_OPTIM_ADAMAX) {
      a = a + (d - a) * h.v0;
      const float x = h.v1 * b, y = fabsf(d) + h.v2;
      b = (y > x || y != y) ? y : x;                     // the larger one; a NaN on either side stays, as torch.maximum keeps it
      p = p - f0 * (a / b);
    } else if (M == OS2D_TRAIN_OPTIM_ASGD) {
      p = p * f0;
      p = p - f1 * d;
      a = f2 != 1.0f ? a + (p - a) * f2 : p;
    } else if (M == OS2D_TRAIN_OPTIM_RMSPROP) {
      a = h.v0 * a + (h.v1 * d) * d;
      p = p - lr * (d / (sqrtf(a) + h.v2));
    } else {
      const float s = d * a;
      const float eta = s > 0.0f ? h.v1 : (s < 0.0f ? h.v0 : (s == 0.0f ? 1.0f : s));      // a NaN product stays NaN
      float size = b * eta;
      size = size < h.v2 ? h.v2 : (size > h.v3 ? h.v3 : size);                            // and so does a NaN size
      b = size;
      if (s < 0.0f) d = 0.0f;
      const float sign = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : (d == 0.0f ? 0.0f : d));
      p = p - sign * size;
      a = d;
    }
  }
};

// grid: x = the table's chunks.  factors: the table's [n][FACTORS] floats of prepare_ex
template <int M>
__global__ __launch_bounds__(THREADS) void optim_update_ex_kernel(const Table tab, int n, int chunk_base, const float* __restrict__ record,
                                                                  const float* __restrict__ factors, const HyperEx h) {
  const int c = chunk_base + blockIdx.x;
  const int i = find_tensor(tab, n, c);
  const Tensor& t = tab.t[i];
  const long long base = (long long)(c - t.first_chunk) * CHUNK;
  const long long left = t.numel - base;
  const float coef = record[1];
  const bool skip = record[2] != 0.0f;
  float f0 = 0.0f, f1 = 0.0f, f2 = 1.0f;
  if (!skip) f0 = factors[FACTORS * i], f1 = factors[FACTORS * i + 1], f2 = factors[FACTORS * i + 2];
  const MethodOp<M> op = {t.lr, t.weight_decay, f0, f1, f2, h};
  if (t.aligned) update_chunk<true>(t, base, left, coef, skip, op);
  else update_chunk<false>(t, base, left, coef, skip, op);
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

namespace {

// what a method takes and needs: the length of its hyperparameter array and, for the update / for prepare, which of state1 (1),
// state2 (2), step (4) a tensor must carry
struct MethodTraits {
  const char* name;
  int nhyper, update_need, prepare_need;
};

const MethodTraits* traits_of(int method) {
  static const MethodTraits table[] = {
      {"Adagrad", 2, 1, 4},      // lr_decay, eps
      {"Adadelta", 2, 3, 4},     // rho, eps
      {"Adamax", 3, 3, 4},       // beta1, beta2, eps
      {"ASGD", 3, 1, 4 | 2},     // lambd, alpha, t0; state2 = {eta, mu}, read and written by prepare only
      {"RMSprop", 2, 1, 4},      // alpha, eps
      {"Rprop", 4, 3, 4},        // etaminus, etaplus, the smallest and the largest step size
  };
  if (method < OS2D_TRAIN_OPTIM_ADAGRAD || method > OS2D_TRAIN_OPTIM_RPROP) return nullptr;
  return &table[method - OS2D_TRAIN_OPTIM_ADAGRAD];
}

// -> 0, or the refusal's code: the method, the array's length and the values' ranges (torch's constructors check the same)
int check_hyper(const char* who, int method, const double* h, int nhyper) {
  const MethodTraits* m = traits_of(method);
  if (!m) return OS2D_REFUSE(-1, "%s: method=%d (2 Adagrad, 3 Adadelta, 4 Adamax, 5 ASGD, 6 RMSprop, 7 Rprop)", who, method);
  if (nhyper != m->nhyper) return OS2D_REFUSE(-1, "%s: %s takes %d hyperparameters, got nhyper=%d", who, m->name, m->nhyper, nhyper);
  if (!h) return OS2D_REFUSE(-1, "%s: null pointer (hyper)", who);
  bool ok = true;
  switch (method) {
    case OS2D_TRAIN_OPTIM_ADAGRAD: ok = h[0] >= 0.0 && h[1] >= 0.0; break;
    case OS2D_TRAIN_OPTIM_ADADELTA: ok = h[0] >= 0.0 && h[0] <= 1.0 && h[1] >= 0.0; break;
    case OS2D_TRAIN_OPTIM_ADAMAX: ok = h[0] >= 0.0 && h[0] < 1.0 && h[1] >= 0.0 && h[1] < 1.0 && h[2] >= 0.0; break;
    case OS2D_TRAIN_OPTIM_ASGD: ok = h[0] == h[0] && h[1] == h[1] && h[2] == h[2]; break;
    case OS2D_TRAIN_OPTIM_RMSPROP: ok = h[0] >= 0.0 && h[1] >= 0.0; break;
    default: ok = h[0] > 0.0 && h[0] < 1.0 && h[1] > 1.0 && h[2] <= h[3]; break;
  }
  if (!ok) return OS2D_REFUSE(-1, "%s: a hyperparameter of %s is outside its range", who, m->name);
  return 0;
}

template <int M>
void launch_update_ex(size_t chunks, const Table& tab, int n, int first, const float* record, const float* factors, const HyperEx& h, void* stream) {
  hipLaunchKernelGGL(optim_update_ex_kernel<M>, dim3((unsigned)chunks), dim3(THREADS), 0, os2d_stream(stream), tab, n, first, record, factors, h);
}

}  // namespace

extern "C" int os2d_train_optim_prepare_ex(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const double* hyper,
                                           int nhyper, float* factors, void* stream) {
  const char* who = "os2d_train_optim_prepare_ex";
  if (const int rc = check_hyper(who, method, hyper, nhyper)) return rc;
  const MethodTraits* m = traits_of(method);
  size_t chunks = 0;
  if (const int rc = check_table(who, tensors, n, m->prepare_need, &chunks)) return rc;
  if (!record || !factors) return OS2D_REFUSE(-1, "%s: null pointer", who);
  for (int i = 0; i < n; ++i) {     // a record without elements is counted too: it had a gradient
    if (!tensors[i].step) return OS2D_REFUSE(-1, "%s: null pointer (step of tensor %d)", who, i);
    if ((m->prepare_need & 2) && !tensors[i].state2) return OS2D_REFUSE(-1, "%s: null pointer (state2 of tensor %d)", who, i);
  }
  if (n == 0) return 0;
  double h0 = 0.0, h1 = 0.0, h2 = 0.0;
  if (method == OS2D_TRAIN_OPTIM_ADAGRAD || method == OS2D_TRAIN_OPTIM_ADAMAX) h0 = hyper[0];
  if (method == OS2D_TRAIN_OPTIM_ASGD) h0 = hyper[0], h1 = hyper[1], h2 = hyper[2];
  hipLaunchKernelGGL(optim_prepare_ex_kernel, dim3(1), dim3(64), 0, os2d_stream(stream), table_of(tensors, n), n, method, record, h0, h1, h2,
                     factors);
  return os2d_launched("optim_prepare_ex_kernel");
}

extern "C" int os2d_train_optim_update_ex(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const float* factors,
                                          const double* hyper, int nhyper, void* stream) {
  const char* who = "os2d_train_optim_update_ex";
  if (const int rc = check_hyper(who, method, hyper, nhyper)) return rc;
  size_t chunks = 0;
  if (const int rc = check_table(who, tensors, n, traits_of(method)->update_need, &chunks)) return rc;
  if (!record || !factors) return OS2D_REFUSE(-1, "%s: null pointer", who);
  if (chunks == 0) return 0;
  HyperEx h = {};
  switch (method) {
    case OS2D_TRAIN_OPTIM_ADAGRAD: h.v0 = (float)hyper[1]; break;
    case OS2D_TRAIN_OPTIM_ADADELTA:
    case OS2D_TRAIN_OPTIM_RMSPROP: h.v0 = (float)hyper[0], h.v1 = (float)(1.0 - hyper[0]), h.v2 = (float)hyper[1]; break;
    case OS2D_TRAIN_OPTIM_ADAMAX: h.v0 = (float)(1.0 - hyper[0]), h.v1 = (float)hyper[1], h.v2 = (float)hyper[2]; break;
    case OS2D_TRAIN_OPTIM_ASGD: break;
    default: h.v0 = (float)hyper[0], h.v1 = (float)hyper[1], h.v2 = (float)hyper[2], h.v3 = (float)hyper[3]; break;
  }
  const Table tab = table_of(tensors, n);
  const int first = tensors[0].first_chunk;
  switch (method) {
    case OS2D_TRAIN_OPTIM_ADAGRAD: launch_update_ex<OS2D_TRAIN_OPTIM_ADAGRAD>(chunks, tab, n, first, record, factors, h, stream); break;
    case OS2D_TRAIN_OPTIM_ADADELTA: launch_update_ex<OS2D_TRAIN_OPTIM_ADADELTA>(chunks, tab, n, first, record, factors, h, stream); break;
    case OS2D_TRAIN_OPTIM_ADAMAX: launch_update_ex<OS2D_TRAIN_OPTIM_ADAMAX>(chunks, tab, n, first, record, factors, h, stream); break;
    case OS2D_TRAIN_OPTIM_ASGD: launch_update_ex<OS2D_TRAIN_OPTIM_ASGD>(chunks, tab, n, first, record, factors, h, stream); break;
    case OS2D_TRAIN_OPTIM_RMSPROP: launch_update_ex<OS2D_TRAIN_OPTIM_RMSPROP>(chunks, tab, n, first, record, factors, h, stream); break;
    default: launch_update_ex<OS2D_TRAIN_OPTIM_RPROP>(chunks, tab, n, first, record, factors, h, stream); break;
  }
  return os2d_launched("optim_update_ex_kernel");
}
