// HBM-bound elementwise and reduction kernels: gradient-penalty helpers, dropout fill, mask compositing, reconstruction and
// adversarial losses, fused optimizers, EMA, gradient statistics, weight packing (the normalisation passes: norm.hip). All
// reductions are two-stage and deterministic (per-block partials + fixed-order final sum) except where an
// accumulate-into-gradient semantic makes a float atomic the natural form.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "bn_acc.h"
#include "vec16.h"

namespace {

// ---- gradient-penalty helpers (WGAN-GP extension) ------------------------------------
// t_out = t_in * slope(a): LeakyReLU Jacobian applied to a tangent (a = primal activation output)
template <typename T>
__global__ void __launch_bounds__(256) mul_slope_kernel(const char* tin, const char* a, char* tout, int64_t chunks) {
  constexpr int EPC = 16 / (int)sizeof(T);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * 256) {
    float t[EPC], av[EPC];
    load_vec<T, EPC>(tin, i * EPC, t);
    load_vec<T, EPC>(a, i * EPC, av);
#pragma unroll
    for (int e = 0; e < EPC; ++e) t[e] *= av[e] > 0.f ? 1.f : 0.2f;
    store_vec<T, EPC>(tout, i * EPC, t);
  }
}

// per-sample squared L2 norm of g (n, hw) -> sumsq[n], and its largest magnitude -> amax[n]
__global__ void __launch_bounds__(256) sample_sumsq_kernel(const float* g, int64_t hw, float* sumsq, float* amax) {
  __shared__ double sh[4];
  __shared__ float shm[4];
  const float* p = g + (int64_t)blockIdx.x * hw;
  double s = 0.0;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < hw; i += 256) { s += (double)p[i] * p[i]; m = fmaxf(m, fabsf(p[i])); }
  for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); m = fmaxf(m, __shfl_xor(m, off)); }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; shm[threadIdx.x >> 6] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sumsq[blockIdx.x] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
    amax[blockIdx.x] = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
  }
}
// v[n,:] = lam/N * 2 (||g_n|| - 1) / ||g_n|| * g[n,:] ; penalty = lam * mean_n (||g_n|| - 1)^2 (written by block 0)
__device__ __forceinline__ float gp_coef(const float* sumsq, int nn, int n, float lam) {
  const float norm = sqrtf(sumsq[nn]);
  return norm > 0.f ? lam / (float)n * 2.f * (norm - 1.f) / norm : 0.f;
}
// Tangent scale: the direction is written as v * s with ONE power of two s = 2^k per call, chosen from
// max|v| = max_n |coef_n| * amax_n so that max|v * s| lies in [1, 2): the fp16 tangent forward then runs in the normal range
// whatever lam and ||g_n|| - 1 are. s = 1 when v is zero or not finite (lam = 0, every ||g_n|| = 1; an overflow stays visible).
// Every block derives s from the same n values in the same order; block (0, 0) stores sc[0] = s, sc[1] = 1/s (both exact).
__global__ void __launch_bounds__(256) gp_direction_kernel(const float* g, const float* sumsq, const float* amax, int n, int64_t hw,
                                                           float lam, float* v, float* penalty, float* sc) {
  const int nn = blockIdx.y;
  float vmax = 0.f;
  for (int k = 0; k < n; ++k) vmax = fmaxf(vmax, fabsf(gp_coef(sumsq, k, n, lam)) * amax[k]);
  int e = (vmax > 0.f && isfinite(vmax)) ? -ilogbf(vmax) : 0;
  e = e < -126 ? -126 : (e > 126 ? 126 : e);
  const float s = ldexpf(1.f, e);
  const float coef = gp_coef(sumsq, nn, n, lam);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256)
    v[(int64_t)nn * hw + i] = (coef * g[(int64_t)nn * hw + i]) * s;
  if (blockIdx.x == 0 && nn == 0 && threadIdx.x == 0) {
    sc[0] = s;
    sc[1] = ldexpf(1.f, -e);
    if (penalty) {
      double acc = 0.0;
      for (int k = 0; k < n; ++k) { const double d = sqrt((double)sumsq[k]) - 1.0; acc += d * d; }
      penalty[0] = (float)(lam * acc / n);
    }
  }
}
// dst[i] += src[i] * sc[1]: the penalty's parameter gradients (accumulated at tangent scale s in a private buffer) into the bound
// gradients, one fixed-order add per element
__global__ void __launch_bounds__(256) gp_unscale_add_kernel(const float* __restrict__ src, const float* __restrict__ sc, float* __restrict__ dst,
                                                             int64_t count) {
  const float is = sc[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] += src[i] * is;
}
// out[n,:] = fake[n,:] + eps[n] * (real[n,:] - fake[n,:])
__global__ void __launch_bounds__(256) interpolate_kernel(const float* real, const float* fake, const float* eps, int64_t hw,
                                                          float* out) {
  const int nn = blockIdx.y;
  const float e = eps[nn];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const int64_t j = (int64_t)nn * hw + i;
    out[j] = e * real[j] + (1.f - e) * fake[j];
  }
}

// ---- mask pipeline (bit-exact: selects / multiplies by 0 or 1) --------------------------------
__global__ void __launch_bounds__(256) mask_apply_kernel(const float* ground, const float* mask, float* mask_c,
                                                         float* masked, int64_t count, int do_ceil) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    float m = (do_ceil & 1) ? ceilf(mask[i]) : mask[i];
    if (do_ceil & 2) m = 1.f - m;
    if (mask_c) mask_c[i] = m;
    masked[i] = ground[i] * (1.f - m);
  }
}
__global__ void __launch_bounds__(256) mask_composite_kernel(const float* masked, const float* gen, const float* mask_c,
                                                             float* out, int64_t count) {
  // two roundings like the reference (mul, then add): without the pragma the pair contracts to one fused multiply-add, which differs
  // by an ulp on a third of the elements once mask_c is fractional (__fmul_rn / __fadd_rn are plain operators here and contract too)
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    out[i] = masked[i] + gen[i] * mask_c[i];
}
__global__ void __launch_bounds__(256) mul_kernel(const float* a, const float* b, float* out, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) out[i] = a[i] * b[i];
}
__global__ void __launch_bounds__(256) add_kernel(const float* a, const float* b, float* out, int64_t count, float alpha) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) out[i] = a[i] + alpha * b[i];
}
__global__ void __launch_bounds__(256) tanh_bwd_kernel(const float* dy, const float* y, float* dx, int64_t count, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    dx[i] = dy[i] * (1.f - y[i] * y[i]) * scale;
}

// ---- reconstruction losses --------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// The masked difference x m - y m with its three roundings, as the reference's y * mask - yhat * mask has them: with one product fused
// into the difference, x == y under a fractional mask would leave the rounding residue of x m instead of 0 (an L1 gradient of
// +-m / count there, and no sqrt(eps) for equal inputs). The compiler happens to keep them apart today; the pragma makes it the rule.
__device__ __forceinline__ float masked_diff(float x, float y, float m) {
#pragma clang fp contract(off)
  return x * m - y * m;
}

// kind: 0 sum|a-b| ; 1 sum (a-b)^2 ; 2/3 masked versions (y*m - yhat*m), second sum = count(m != 0)
__global__ void __launch_bounds__(256) loss_partial_kernel(const float* a, const float* b, const float* m, int64_t count,
                                                           int kind, float* scratch) {
  __shared__ double sh[4];
  double s = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    float d;
    if (m) {
      const float mm = m[i];
      d = masked_diff(b[i], a[i], mm);
      cnt += (mm != 0.f) ? 1.0 : 0.0;
    } else {
      d = a[i] - b[i];
    }
    s += (kind & 1) ? (double)d * d : (double)fabsf(d);
  }
  s = block_sum(s, sh);
  cnt = block_sum(cnt, sh);
  if (threadIdx.x == 0) { scratch[blockIdx.x * 2] = (float)s; scratch[blockIdx.x * 2 + 1] = (float)cnt; }
}
// mode: 0 mean ; 1 sqrt(mean + eps)
__global__ void __launch_bounds__(256) loss_final_kernel(const float* scratch, int nblocks, double denom, int use_cnt,
                                                         int mode, float eps, float* loss_out) {
  __shared__ double sh[4];
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { s += scratch[i * 2]; c += scratch[i * 2 + 1]; }
  s = block_sum(s, sh);
  c = block_sum(c, sh);
  if (threadIdx.x == 0) {
    const double d = use_cnt ? c : denom;
    double l = s / d;
    if (mode == 1) l = sqrt(l + (double)eps);
    loss_out[0] = (float)l;
    loss_out[1] = (float)d;   // denominator kept for the gradient kernel
  }
}
// gkind: 0 L1 ; 1 MSE ; 2 RMSE  (masked when m != null: gradient w.r.t. yhat = a)
__global__ void __launch_bounds__(256) loss_grad_kernel(const float* a, const float* b, const float* m, int64_t count,
                                                        int gkind, const float* loss, float gscale, float* grad) {
  const float l = loss[0], den = loss[1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    float d, mm = 1.f;
    if (m) { mm = m[i]; d = masked_diff(a[i], b[i], mm); }
    else d = a[i] - b[i];
    float g;
    if (gkind == 0) g = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / den;
    else if (gkind == 1) g = 2.f * d / den;
    else g = d / (den * l);
    grad[i] = g * mm * gscale;
  }
}

// adversarial losses on (n,) predictions. Workgroup b of a two-workgroup launch (gi_loss_adv_pair: the [real | fake] halves of a
// stacked discriminator batch, their targets, loss slots and gradient signs) works on the b-th half.
__global__ void __launch_bounds__(256) adv_loss_kernel(const float* pred, int n, int kind, float target, float* loss_out,
                                                       float* grad, float gscale, float target1, float* loss_out1, float gscale1) {
  __shared__ double sh[4];
  if (blockIdx.x == 1) { pred += n; if (grad) grad += n; target = target1; loss_out = loss_out1; gscale = gscale1; }
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float p = pred[i];
    float l, g;
    if (kind == 0) {  // nn.BCELoss: log clamped at -100; backward (p-t)/max(p(1-p),1e-12)
      // log1p: 1.f - p is 1 for p < 2^-25, and the loss of a confidently rejected sample would read 0 instead of p
      const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(log1pf(-p), -100.f);
      l = -(target * lp + (1.f - target) * l1p);
      g = (p - target) / fmaxf(p * (1.f - p), 1e-12f);
    } else if (kind == 1) {
      l = (p - target) * (p - target);
      g = 2.f * (p - target);
    } else {
      l = p;
      g = 1.f;
    }
    s += l;
    if (grad) grad[i] = g / (float)n * gscale;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss_out[0] = (float)(s / n);
}

// ---- optimizers --------------------------------------------------------------------------------
// The verdict of the finite check (gi_check_finite*): guard[1] after the finish launch (vword = 0), or - vword = 2 / 3, no finish
// launch - the scan word itself: every workgroup reads it, and for the first kernel of an update (finish) one thread also does what
// the finish launch did (guard[1] = verdict, guard[0] += verdict) and clears the OTHER scan word for the next update's scan. The word
// in use cannot be cleared here (later workgroups still read it): updates alternate between the two.
__device__ __forceinline__ int gi_guard_verdict(int* guard, int vword, int finish) {
  if (!guard) return 0;
  if (vword == 0) return guard[1];
  const int verdict = guard[vword];
  if (finish && blockIdx.x == 0 && threadIdx.x == 0) {
    guard[1] = verdict;
    if (verdict) guard[0] += 1;
    guard[vword ^ 1] = 0;
  }
  return verdict;
}
// guard (may be null): guard[1] != 0 means "the gradients of this update hold inf/NaN" (gi_check_finite): skip it whole
// omb1 / omb2 / step_size: 1 - beta1, 1 - beta2 and lr / bias_correction1 are formed in double on the host and rounded once,
// as torch.optim does with its Python floats (1.f - 0.999f differs from float(1 - 0.999) by 1e-4 relative)
// seen >= 0 (with a guard): the host's step count still includes the updates skipped since its last poll (guard[0] - seen of them):
// the bias corrections are formed here from step - (guard[0] - seen), in double by one thread, so a skipped update never advances them
__global__ void __launch_bounds__(256) adam_kernel(float* p, const float* g, float* m, float* v, int64_t count, float step_size,
                                                   float b1, float b2, float eps, float omb1, float omb2, float sqrt_bc2, float gs,
                                                   int* guard, int step, int seen, double lrd, double b1d, double b2d, int vword, int finish) {
  if (gi_guard_verdict(guard, vword, finish)) return;
  if (guard && seen >= 0) {
    __shared__ float s_ss, s_sq;
    if (threadIdx.x == 0) {
      int st = step - (guard[0] - seen);
      if (st < 1) st = 1;
      s_ss = (float)(lrd / (1.0 - pow(b1d, (double)st)));
      s_sq = (float)sqrt(1.0 - pow(b2d, (double)st));
    }
    __syncthreads();
    step_size = s_ss;
    sqrt_bc2 = s_sq;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float gg = g[i] * gs;
    const float mm = b1 * m[i] + omb1 * gg;
    const float vv = b2 * v[i] + omb2 * gg * gg;
    m[i] = mm;
    v[i] = vv;
    const float denom = sqrtf(vv) / sqrt_bc2 + eps;
    p[i] = p[i] - step_size * (mm / denom);
  }
}
__global__ void __launch_bounds__(256) rmsprop_kernel(float* p, const float* g, float* sq, int64_t count, float lr,
                                                      float alpha, float oma, float eps, float clampv, float gs, int* guard, int vword, int finish) {
  if (gi_guard_verdict(guard, vword, finish)) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float gg = g[i] * gs;
    const float s = alpha * sq[i] + oma * gg * gg;
    sq[i] = s;
    float w = p[i] - lr * (gg / (sqrtf(s) + eps));
    if (clampv > 0.f) w = fminf(fmaxf(w, -clampv), clampv);
    p[i] = w;
  }
}
// flag[2] |= 1 when any element of g is inf or NaN.
// (Measured and dropped in round 4: the workgroup that ends last also doing the finish - every workgroup adds to a ticket on the
//  same word after its OR - made the scan 5 -> 20 us on the critic's 1350 workgroups: 1350 returning atomics on one address at ~12 ns.)
__global__ void __launch_bounds__(256) check_finite_kernel(const float* __restrict__ g, int64_t count, int* flag, int word) {
  int bad = 0;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? count / 4 : 0;   // 16-byte chunks, two in flight per thread
  const u4_t* g4 = (const u4_t*)g;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const u4_t a = g4[i], b = g4[i + stride];
#pragma unroll
    for (int e = 0; e < 4; ++e) bad |= (((a[e] & 0x7F800000u) == 0x7F800000u) || ((b[e] & 0x7F800000u) == 0x7F800000u)) ? 1 : 0;
  }
  if (i < n4) {
    const u4_t a = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) bad |= ((a[e] & 0x7F800000u) == 0x7F800000u) ? 1 : 0;
  }
  for (int64_t j = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += stride) {   // what 16-byte chunks do not cover
    const unsigned u = __float_as_uint(g[j]);
    bad |= ((u & 0x7F800000u) == 0x7F800000u) ? 1 : 0;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag + word, 1);
}
// flag[1] = this update's verdict, flag[0] += it (running count of skipped updates), flag[2] = 0
__global__ void check_finite_finish_kernel(int* flag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int b = flag[2];
    flag[1] = b;
    flag[0] += b;
    flag[2] = 0;
  }
}
__global__ void __launch_bounds__(256) clamp_kernel(float* p, int64_t count, float lo, float hi) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    p[i] = fminf(fmaxf(p[i], lo), hi);
}
// Exponential moving average of a flat parameter buffer (optim.EMA): ema += om * (p - ema), om = 1 - decay. Two roundings per element,
// both written out so that contraction cannot change them: diff = p - ema, then one fused multiply-add. guard (may be null): guard[1]
// is the verdict the update's first optimizer kernel recorded (gi_guard_verdict); a skipped update leaves the average alone too.
// 12 bytes per element and no reuse. Elements [head, head + 4 * n4) go as 16-byte chunks, two in flight per thread (the caller
// passes n4 > 0 only when ema + head and p + head are both 16-byte aligned); the head and what follows the chunks go one by one.
__device__ __forceinline__ float ema_one(float e, float q, float om) { return __fmaf_rn(om, __fsub_rn(q, e), e); }
__global__ void __launch_bounds__(256) ema_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t count, float om,
                                                  const int* guard, int64_t head, int64_t n4) {
  if (guard && guard[1] != 0) return;
  const int64_t stride = (int64_t)gridDim.x * 256, tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  f4_t* e4 = (f4_t*)(ema + head);
  const f4_t* p4 = (const f4_t*)(p + head);
  int64_t i = tid;
  for (; i + stride < n4; i += 2 * stride) {
    f4_t a = e4[i], b = e4[i + stride];
    const f4_t qa = p4[i], qb = p4[i + stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = ema_one(a[k], qa[k], om); b[k] = ema_one(b[k], qb[k], om); }
    e4[i] = a;
    e4[i + stride] = b;
  }
  if (i < n4) {
    f4_t a = e4[i];
    const f4_t qa = p4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = ema_one(a[k], qa[k], om);
    e4[i] = a;
  }
  const int64_t rest = count - 4 * n4;     // the head and the tail: fewer than 8 elements when the chunks cover the rest, else all
  for (int64_t j = tid; j < rest; j += stride) {
    const int64_t idx = j < head ? j : j + 4 * n4;
    ema[idx] = ema_one(ema[idx], p[idx], om);
  }
}
// grid (slices, nseg): partials[s][slice] = sum|g| over the slice's share of segment s; absmean_final_kernel adds a segment's
// slices in slice order and divides by its length. No float atomics: the logged means do not depend on which workgroup ends
// first, so a run's gradient-flow history is reproducible bit for bit like its weights.
constexpr int kAbsmeanSlices = 32, kAbsmeanMaxSeg = 256;
__global__ void __launch_bounds__(256) absmean_kernel(const float* g, const int64_t* off, const int64_t* len, double* partials) {
  __shared__ double sh[4];
  const int sgm = blockIdx.y;
  const int64_t o = off[sgm], l = len[sgm];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < l; i += (int64_t)gridDim.x * 256) s += fabsf(g[o + i]);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) partials[sgm * gridDim.x + blockIdx.x] = s;
}
__global__ void __launch_bounds__(256) absmean_final_kernel(const double* partials, const int64_t* len, int nseg, int slices, float* out) {
  const int sgm = blockIdx.x * 256 + threadIdx.x;
  if (sgm >= nseg) return;
  double s = 0.0;
  for (int k = 0; k < slices; ++k) s += partials[sgm * slices + k];
  out[sgm] = s != 0.0 ? (float)(s / (double)len[sgm]) : 0.f;
}

// ---- weight packing / conversion ---------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) convert_kernel(const float* src, T* dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = (T)src[i];
}
template <typename T>
__global__ void __launch_bounds__(256) convert_back_kernel(const T* src, float* dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = (float)src[i];
}
// w [a][16][b] -> wph [4 phases][b][4 taps][a], tap t=(ty,tx) of phase (py,px) is (ky,kx)=(1-py+2ty, 1-px+2tx).
// 32x32 (a,b) tile transposed through LDS so that both the read (b fastest) and the write
// (a fastest) are coalesced.
template <typename T>
__global__ void __launch_bounds__(256) pack_phase_kernel(const float* w, T* wph, int ca, int cb) {
  __shared__ float tile[32][33];
  const int k16 = blockIdx.z;   // ph*4 + t
  const int ph = k16 >> 2, t = k16 & 3;
  const int ky = 1 - (ph >> 1) + 2 * (t >> 1), kx = 1 - (ph & 1) + 2 * (t & 1);
  const int a0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int a = a0 + r, b = b0 + tx;
    tile[r][tx] = (a < ca && b < cb) ? w[((int64_t)a * 16 + ky * 4 + kx) * cb + b] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int b = b0 + r, a = a0 + tx;
    if (a < ca && b < cb) wph[(((int64_t)ph * cb + b) * 4 + t) * ca + a] = (T)tile[tx][r];
  }
}

// All layers of a network in one launch: a workgroup takes one 32x32 (a,b) tile of one tap of one layer, writes the
// plain converted copy (same [a][16][b] layout) and the transposed sub-pixel-phase copy from a single read.
template <typename T>
__global__ void __launch_bounds__(256) pack_batch_kernel(PackJobs P) {
  __shared__ float tile[32][33];
  int jb = 0;
  while (jb + 1 < P.n && (int)blockIdx.x >= P.j[jb + 1].tile0) ++jb;
  const float* w = P.j[jb].w;
  T* packed = (T*)P.j[jb].packed;
  T* wph = (T*)P.j[jb].phase;
  const int ca = P.j[jb].ca, cb = P.j[jb].cb, tiles_a = (ca + 31) / 32, tiles_b = (cb + 31) / 32;
  int t = (int)blockIdx.x - P.j[jb].tile0;
  const int a0 = (t % tiles_a) * 32;
  t /= tiles_a;
  const int b0 = (t % tiles_b) * 32, k16 = t / tiles_b;   // k16 = ph*4 + tap
  const int ph = k16 >> 2, tp = k16 & 3;
  const int ky = 1 - (ph >> 1) + 2 * (tp >> 1), kx = 1 - (ph & 1) + 2 * (tp & 1);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int a = a0 + r, b = b0 + tx;
    float v = 0.f;
    if (a < ca && b < cb) {
      const int64_t idx = ((int64_t)a * 16 + ky * 4 + kx) * cb + b;
      v = w[idx];
      if (P.j[jb].scale) v *= P.j[jb].scale[P.j[jb].scale_on_b ? b : a];   // inference: the following BatchNorm's scale folded in
      if (packed) packed[idx] = (T)v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  if (!wph) return;
  for (int r = ty; r < 32; r += 8) {
    const int b = b0 + r, a = a0 + tx;
    if (a < ca && b < cb) wph[(((int64_t)ph * cb + b) * 4 + tp) * ca + a] = (T)tile[tx][r];
  }
}

// The same on 64 x 64 tiles with four values per lane (layers whose channel counts are multiples of 64, i.e. every layer of the
// generator and the critic but the single-channel ones): 128-byte rows on both fp16 copies instead of 64-byte ones, a quarter of
// the workgroups.
template <typename T>
__global__ void __launch_bounds__(256) pack_batch64_kernel(PackJobs P) {
  __shared__ float tile[64][65];
  int jb = 0;
  while (jb + 1 < P.n && (int)blockIdx.x >= P.j[jb + 1].tile0) ++jb;
  const float* w = P.j[jb].w;
  T* packed = (T*)P.j[jb].packed;
  T* wph = (T*)P.j[jb].phase;
  const int ca = P.j[jb].ca, cb = P.j[jb].cb, tiles_a = ca / 64, tiles_b = cb / 64;
  int t = (int)blockIdx.x - P.j[jb].tile0;
  const int a0 = (t % tiles_a) * 64;
  t /= tiles_a;
  const int b0 = (t % tiles_b) * 64, k16 = t / tiles_b;   // k16 = ph*4 + tap
  const int ph = k16 >> 2, tp = k16 & 3;
  const int ky = 1 - (ph >> 1) + 2 * (tp >> 1), kx = 1 - (ph & 1) + 2 * (tp & 1);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // 16 x 16, four consecutive values per lane
  const float* sc = P.j[jb].scale;
  const int on_b = P.j[jb].scale_on_b;
  for (int r = ty; r < 64; r += 16) {
    const int a = a0 + r, b = b0 + tx * 4;
    const int64_t idx = ((int64_t)a * 16 + ky * 4 + kx) * cb + b;
    f4_t v = *(const f4_t*)(w + idx);
    if (sc) {
      if (on_b) v *= *(const f4_t*)(sc + b);
      else v *= sc[a];
    }
    if (packed) {
      T o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
      if constexpr (sizeof(T) == 2) *(uint2*)(packed + idx) = *(const uint2*)o;
      else *(f4_t*)(packed + idx) = *(const f4_t*)o;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[r][tx * 4 + e] = v[e];
  }
  __syncthreads();
  if (!wph) return;
  for (int r = ty; r < 64; r += 16) {
    const int b = b0 + r, a = a0 + tx * 4;
    T o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (T)tile[tx * 4 + e][r];
    T* dst = wph + (((int64_t)ph * cb + b) * 4 + tp) * ca + a;
    if constexpr (sizeof(T) == 2) *(uint2*)dst = *(const uint2*)o;
    else *(f4_t*)dst = *(const f4_t*)o;
  }
}

__global__ void __launch_bounds__(256) dropout_fill_kernel(uint8_t* mask, int64_t count, uint64_t seed, uint32_t thresh) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    mask[i] = dropout_keep(seed, i, thresh);
}
__global__ void __launch_bounds__(256) mask_layout_kernel(const uint8_t* src, uint8_t* dst, int n, int c, int hw, int to_nhwc) {
  const int64_t total = (int64_t)n * c * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    // i indexes the NHWC tensor
    const int ch = (int)(i % c);
    const int64_t t = i / c;
    const int p = (int)(t % hw);
    const int nn = (int)(t / hw);
    const int64_t j = ((int64_t)nn * c + ch) * hw + p;   // NCHW index
    if (to_nhwc) dst[i] = src[j];
    else dst[j] = src[i];
  }
}

}  // namespace

// =================================================================================================
int op_pack_weights(hipStream_t st, int dtype, const float* w, int ca, int cb, void* w_packed, void* w_phase) {
  const int64_t count = (int64_t)ca * 16 * cb;
  if (w_packed) GI_TRY(op_convert(st, dtype, w, w_packed, count));
  if (w_phase) {
    dim3 grid((ca + 31) / 32, (cb + 31) / 32, 16);
    gi_with_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(pack_phase_kernel<T>, grid, dim3(256), 0, st, w, (T*)w_phase, ca, cb);
    });
    GI_LAUNCH_CHECK();
  }
  return GI_OK;
}

int op_pack_weights_batch(hipStream_t st, int dtype, PackJobs& P) {
  if (P.n <= 0) return GI_OK;
  GI_REQUIRE(P.n <= 16, "pack_weights_batch: %d layers", P.n);
  bool all64 = true;
  for (int i = 0; i < P.n; ++i) all64 = all64 && P.j[i].ca % 64 == 0 && P.j[i].cb % 64 == 0;
  const int ts = all64 ? 64 : 32;
  int tiles = 0;
  for (int i = 0; i < P.n; ++i) {
    P.j[i].tile0 = tiles;
    tiles += ((P.j[i].ca + ts - 1) / ts) * ((P.j[i].cb + ts - 1) / ts) * 16;
  }
  gi_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (all64) hipLaunchKernelGGL(pack_batch64_kernel<T>, dim3(tiles), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(pack_batch_kernel<T>, dim3(tiles), dim3(256), 0, st, P);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_convert(hipStream_t st, int dtype, const float* src, void* dst, int64_t count) {
  gi_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(convert_kernel<T>, dim3(nblocks(count)), dim3(256), 0, st, src, (T*)dst, count);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int op_convert_back(hipStream_t st, int dtype, const void* src, float* dst, int64_t count) {
  gi_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(convert_back_kernel<T>, dim3(nblocks(count)), dim3(256), 0, st, (const T*)src, dst, count);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int op_tanh_bwd(hipStream_t st, const float* dy, const float* y, float* dx, int64_t count, float scale) {
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(nblocks(count)), dim3(256), 0, st, dy, y, dx, count, scale);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int op_fill_dropout(hipStream_t st, uint8_t* mask, int64_t count, uint64_t seed, float p) {
  const uint32_t thresh = gi_dropout_thresh(p);
  hipLaunchKernelGGL(dropout_fill_kernel, dim3(nblocks(count)), dim3(256), 0, st, mask, count, seed, thresh);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int op_mask_nchw_to_nhwc(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int c, int hw, int to_nhwc) {
  hipLaunchKernelGGL(mask_layout_kernel, dim3(nblocks((int64_t)n * c * hw)), dim3(256), 0, st, src, dst, n, c, hw, to_nhwc);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_mul_slope(hipStream_t st, int dtype, const void* tin, const void* a, void* tout, int64_t count) {
  const int epc = dtype == GI_F16 ? 8 : 4;
  GI_REQUIRE(count % epc == 0, "mul_slope: count must be a multiple of %d", epc);
  gi_with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(mul_slope_kernel<T>, dim3(nblocks(count / epc, 2)), dim3(256), 0, st, (const char*)tin, (const char*)a, (char*)tout, count / epc);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_gp_direction(hipStream_t st, const float* g, int n, int64_t hw, float lam, float* sumsq, float* amax, float* v, float* penalty,
                    float* sc) {
  hipLaunchKernelGGL(sample_sumsq_kernel, dim3(n), dim3(256), 0, st, g, hw, sumsq, amax);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_direction_kernel, dim3(nblocks(hw) > 64 ? 64 : nblocks(hw), n), dim3(256), 0, st, g, sumsq, amax, n, hw, lam, v, penalty, sc);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_gp_unscale_add(hipStream_t st, const float* src, const float* sc, float* dst, int64_t count) {
  hipLaunchKernelGGL(gp_unscale_add_kernel, dim3(nblocks(count)), dim3(256), 0, st, src, sc, dst, count);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// ---- C-ABI entry points that are pure elementwise ops -------------------------------------------
extern "C" {

int gi_mask_apply(gi_ctx* ctx, const float* ground, const float* mask, float* mask_c, float* masked, int64_t count, int do_ceil) {
  hipLaunchKernelGGL(mask_apply_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, ground, mask, mask_c, masked, count, do_ceil);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_mask_composite(gi_ctx* ctx, const float* masked, const float* gen, const float* mask_c, float* inpainted, int64_t count) {
  hipLaunchKernelGGL(mask_composite_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, masked, gen, mask_c, inpainted, count);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_mul(gi_ctx* ctx, const float* a, const float* b, float* out, int64_t count) {
  hipLaunchKernelGGL(mul_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, a, b, out, count);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_interpolate(gi_ctx* ctx, const float* real, const float* fake, const float* eps, int n, int64_t hw, float* out) {
  GI_REQUIRE(ctx && real && fake && eps && out && n > 0, "interpolate: bad argument");
  hipLaunchKernelGGL(interpolate_kernel, dim3(nblocks(hw) > 64 ? 64 : nblocks(hw), n), dim3(256), 0, ctx->stream, real, fake, eps, hw, out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_add(gi_ctx* ctx, const float* a, const float* b, float* out, int64_t count, float alpha) {
  hipLaunchKernelGGL(add_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, a, b, out, count, alpha);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

static int loss_generic(gi_ctx* ctx, const float* a, const float* b, const float* m, int64_t count, int pkind, int mode,
                        int gkind, float eps, float* loss_out, float* grad, float gscale, float* scratch) {
  GI_REQUIRE(scratch != nullptr, "loss: scratch is required (>= 4096 floats)");
  const int nb = nblocks(count) > 1024 ? 1024 : nblocks(count);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(nb), dim3(256), 0, ctx->stream, a, b, m, count, pkind, scratch);
  GI_LAUNCH_CHECK();
  // loss_out needs two floats (value, denominator): stage in scratch tail then copy the value
  float* tmp = scratch + 2048;
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, ctx->stream, scratch, nb, (double)count, m ? 1 : 0, mode, eps, tmp);
  GI_LAUNCH_CHECK();
  GI_HIP(hipMemcpyAsync(loss_out, tmp, sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  if (grad) {
    hipLaunchKernelGGL(loss_grad_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, a, b, m, count, gkind, tmp, gscale, grad);
    GI_LAUNCH_CHECK();
  }
  return GI_OK;
}

int gi_loss_l1(gi_ctx* ctx, const float* a, const float* b, int64_t count, float* loss_out, float* grad_a, float gscale, float* scratch) {
  return loss_generic(ctx, a, b, nullptr, count, 0, 0, 0, 0.f, loss_out, grad_a, gscale, scratch);
}
int gi_loss_mse(gi_ctx* ctx, const float* a, const float* b, int64_t count, float* loss_out, float* grad_a, float gscale, float* scratch) {
  return loss_generic(ctx, a, b, nullptr, count, 1, 0, 1, 0.f, loss_out, grad_a, gscale, scratch);
}
int gi_loss_rmse(gi_ctx* ctx, const float* a, const float* b, int64_t count, float eps, float* loss_out, float* grad_a, float gscale, float* scratch) {
  return loss_generic(ctx, a, b, nullptr, count, 1, 1, 2, eps, loss_out, grad_a, gscale, scratch);
}
int gi_loss_local(gi_ctx* ctx, const float* yhat, const float* y, const float* mask, int64_t count, int kind, float* loss_out,
                  float* grad_yhat, float gscale, float* scratch) {
  GI_REQUIRE(kind >= 0 && kind <= 2, "loss_local: kind=%d", kind);
  return loss_generic(ctx, yhat, y, mask, count, kind == 0 ? 0 : 1, kind == 2 ? 1 : 0, kind, 1e-16f, loss_out, grad_yhat, gscale, scratch);
}
int gi_loss_adv(gi_ctx* ctx, const float* pred, int n, int kind, float target, float* loss_out, float* grad_pred, float gscale) {
  GI_REQUIRE(kind >= 0 && kind <= 2 && n > 0, "loss_adv: kind=%d n=%d", kind, n);
  hipLaunchKernelGGL(adv_loss_kernel, dim3(1), dim3(256), 0, ctx->stream, pred, n, kind, target, loss_out, grad_pred, gscale, 0.f, (float*)nullptr, 0.f);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_loss_adv_pair(gi_ctx* ctx, const float* pred2, int n_each, int kind, float target_a, float target_b, float* loss_a, float* loss_b,
                     float* grad_pred2, float gscale_a, float gscale_b) {
  GI_REQUIRE(ctx && pred2 && loss_a && loss_b && kind >= 0 && kind <= 2 && n_each > 0, "loss_adv_pair: kind=%d n=%d", kind, n_each);
  hipLaunchKernelGGL(adv_loss_kernel, dim3(2), dim3(256), 0, ctx->stream, pred2, n_each, kind, target_a, loss_a, grad_pred2, gscale_a, target_b, loss_b,
                     gscale_b);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_adam_step(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                 float eps, int step, float grad_scale) {
  return gi_adam_step_guarded(ctx, p, g, m, v, count, lr, beta1, beta2, eps, step, grad_scale, nullptr);
}
int gi_adam_step_guarded(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                         float eps, int step, float grad_scale, const int* guard) {
  return gi_adam_step_guarded2(ctx, p, g, m, v, count, lr, beta1, beta2, eps, step, -1, grad_scale, guard);
}
int gi_adam_step_guarded2(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                          float eps, int step, int skipped_seen, float grad_scale, const int* guard) {
  return gi_adam_step_scan(ctx, p, g, m, v, count, lr, beta1, beta2, eps, step, skipped_seen, grad_scale, (int*)guard, 0, 0);
}
int gi_adam_step_scan(gi_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1, float beta2,
                      float eps, int step, int skipped_seen, float grad_scale, int* guard, int word, int finish) {
  GI_REQUIRE(word == 0 || ((word == 2 || word == 3) && guard), "adam: scan word %d", word);
  GI_REQUIRE(step >= 1, "adam: step=%d must be >= 1", step);
  // torch.optim forms 1 - beta and lr / bias_correction1 from Python floats (doubles) and rounds once. The hyper-parameters
  // arrive here as C floats (0.999f = 0.99900001...): recover the decimal the caller wrote (7 significant digits) first
  auto py = [](float x) { char b[32]; snprintf(b, sizeof b, "%.7g", (double)x); return atof(b); };
  const double b1 = py(beta1), b2 = py(beta2), lrd = py(lr);
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  hipLaunchKernelGGL(adam_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, p, g, m, v, count, (float)(lrd / bc1), beta1, beta2, eps,
                     (float)(1.0 - b1), (float)(1.0 - b2), (float)sqrt(bc2), grad_scale, (int*)guard, step, guard ? skipped_seen : -1, lrd, b1, b2, word, finish);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_rmsprop_step(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr, float alpha, float eps, float clamp,
                    float grad_scale) {
  return gi_rmsprop_step_guarded(ctx, p, g, sq, count, lr, alpha, eps, clamp, grad_scale, nullptr);
}
int gi_rmsprop_step_guarded(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr, float alpha, float eps,
                            float clamp, float grad_scale, const int* guard) {
  return gi_rmsprop_step_scan(ctx, p, g, sq, count, lr, alpha, eps, clamp, grad_scale, (int*)guard, 0, 0);
}
int gi_rmsprop_step_scan(gi_ctx* ctx, float* p, const float* g, float* sq, int64_t count, float lr, float alpha, float eps,
                         float clamp, float grad_scale, int* guard, int word, int finish) {
  GI_REQUIRE(word == 0 || ((word == 2 || word == 3) && guard), "rmsprop: scan word %d", word);
  char b[32];
  snprintf(b, sizeof b, "%.7g", (double)alpha);          // the Python float the caller meant (0.99), see gi_adam_step_guarded
  const float oma = (float)(1.0 - atof(b));
  hipLaunchKernelGGL(rmsprop_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, p, g, sq, count, lr, alpha, oma, eps, clamp, grad_scale,
                     guard, word, finish);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_check_finite_scan(gi_ctx* ctx, const float* g, int64_t count, int* flag3) { return gi_check_finite_scan_word(ctx, g, count, flag3, 2); }
int gi_check_finite_scan_word(gi_ctx* ctx, const float* g, int64_t count, int* flag4, int word) {
  GI_REQUIRE(ctx && g && flag4 && count > 0 && (word == 2 || word == 3), "check_finite_scan: bad argument");
  hipLaunchKernelGGL(check_finite_kernel, dim3(nblocks((count + 3) / 4, 2)), dim3(256), 0, ctx->stream, g, count, flag4, word);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_check_finite_finish(gi_ctx* ctx, int* flag3) {
  GI_REQUIRE(ctx && flag3, "check_finite_finish: bad argument");
  hipLaunchKernelGGL(check_finite_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, flag3);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_check_finite(gi_ctx* ctx, const float* g, int64_t count, int* flag3) {
  GI_TRY(gi_check_finite_scan(ctx, g, count, flag3));
  return gi_check_finite_finish(ctx, flag3);
}
int gi_clamp(gi_ctx* ctx, float* p, int64_t count, float lo, float hi) {
  hipLaunchKernelGGL(clamp_kernel, dim3(nblocks(count)), dim3(256), 0, ctx->stream, p, count, lo, hi);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_ema_update(gi_ctx* ctx, float* ema, const float* p, int64_t count, float decay, const int* guard) {
  GI_REQUIRE(ctx && ema && p && count > 0, "ema_update: null argument or count=%lld", (long long)count);
  GI_REQUIRE(decay >= 0.f && decay <= 1.f, "ema_update: decay=%g outside [0, 1]", (double)decay);
  const uintptr_t ae = reinterpret_cast<uintptr_t>(ema), ap = reinterpret_cast<uintptr_t>(p);
  GI_REQUIRE((ae & 3) == 0 && (ap & 3) == 0, "ema_update: pointers must be 4-byte aligned");
  // flat views start at any float offset: 16-byte chunks need both pointers to reach a 16-byte boundary after the same head
  int64_t head = 0, n4 = 0;
  if (((ae ^ ap) & 15) == 0) {
    head = (int64_t)(((16 - (ae & 15)) & 15) / 4);
    if (head > count) head = count;
    n4 = (count - head) / 4;
  }
  const float om = 1.0f - decay;
  // at most the 2048 workgroups that are resident at once (256 CUs x 8), 32 bytes of each buffer per thread and round
  hipLaunchKernelGGL(ema_kernel, dim3(nblocks(n4 > 0 ? n4 : count, 2)), dim3(256), 0, ctx->stream, ema, p, count, om, guard, head, n4);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int gi_grad_absmean(gi_ctx* ctx, const float* g, const int64_t* seg_off, const int64_t* seg_len, int nseg, float* out) {
  GI_REQUIRE(ctx && nseg > 0 && nseg <= kAbsmeanMaxSeg, "grad_absmean: nseg=%d (1 .. %d)", nseg, kAbsmeanMaxSeg);
  if (!ctx->absmean_partials) GI_HIP(hipMalloc((void**)&ctx->absmean_partials, sizeof(double) * kAbsmeanSlices * kAbsmeanMaxSeg));
  hipLaunchKernelGGL(absmean_kernel, dim3(kAbsmeanSlices, nseg), dim3(256), 0, ctx->stream, g, seg_off, seg_len, ctx->absmean_partials);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(absmean_final_kernel, dim3((nseg + 255) / 256), dim3(256), 0, ctx->stream, (const double*)ctx->absmean_partials, seg_len, nseg,
                     kAbsmeanSlices, out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // extern "C"
