// The normalisation passes (HBM-bound): BatchNorm2d statistics finalize / apply / backward through [dropout] -> activation ->
// [BatchNorm], InstanceNorm2d forward / backward, the bias gradient and the BatchNorm tangent injection of the gradient penalty.
// All reductions are two-stage and deterministic (per-block partials + fixed-order final sum, or the exact accumulators of
// stat_acc.h). Every step the backward kernels share - the chunk loader, the dz arithmetic, the coefficients of the apply pass, the
// accumulator-to-LDS prologue, the tail of a column pass - is one device function here.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "stat_acc.h"
#include "bn_acc.h"
#include "vec16.h"

namespace {

// ---- BatchNorm statistics --------------------------------------------------------------------
// partials [rows][2][c] -> per-channel scale/shift (+ running-stat update in train mode).
// nn.BatchNorm2d semantics (lib/models/networks.py:38): biased variance for normalisation,
// unbiased for running_var, momentum 0.1, eps 1e-5.
__global__ void __launch_bounds__(256) bn_finalize_kernel(const float* partials, int rows, int c, float count,
                                                          const float* gamma, const float* beta, float* rmean,
                                                          float* rvar, float* scale, float* shift, float* smean,
                                                          float* sinv, int train, float momentum, float eps, int groups,
                                                          int64_t part_stride, int out_stride) {
  // groups > 1: consecutive BatchNorm populations (stacked critic batch); group j's partial rows start at
  // partials + j*part_stride, its outputs at +j*out_stride; running statistics are updated in group order
  __shared__ double sh[8];
  const int ch = blockIdx.x;
  for (int j = 0; j < groups; ++j) {
    float mean = 0.f, var = 1.f;
    double s = 0.0, q = 0.0;
    if (train) {
      const float* pj = partials + (int64_t)j * part_stride;
      for (int r = threadIdx.x; r < rows; r += 256) {
        s += (double)pj[((int64_t)r * 2) * c + ch];
        q += (double)pj[((int64_t)r * 2 + 1) * c + ch];
      }
      block_sum2(s, q, sh);
    }
    if (threadIdx.x == 0) {
      if (train) {
        const double m = s / count;
        double v = q / count - m * m;
        // (one sample has no spread: the fp32 rounding of its square - up to 6e-8 x^2, next to eps = 1e-5 - is not a variance)
        if (v < 0.0 || count <= 1.f) v = 0.0;
        mean = (float)m;
        var = (float)v;
        const float unbiased = count > 1.f ? (float)(v * (double)count / ((double)count - 1.0)) : var;
        rmean[ch] = (1.f - momentum) * rmean[ch] + momentum * mean;
        rvar[ch] = (1.f - momentum) * rvar[ch] + momentum * unbiased;
      } else {
        mean = rmean[ch];
        var = rvar[ch];
      }
      const float inv = 1.0f / sqrtf(var + eps);
      const float sc = gamma[ch] * inv;
      const int o = j * out_stride + ch;
      scale[o] = sc;
      shift[o] = beta[ch] - mean * sc;
      smean[o] = mean;
      sinv[o] = inv;
    }
  }
}

// stand-alone form (consumers that apply the affine map themselves: C1Affine, HeadArgs::scale4)
__global__ void __launch_bounds__(256) bn_finalize_acc_kernel(BnAccP a, int c) {
  if (blockIdx.x == 0 && a.zero_next) zero_words64(a.zero_next, a.zero_words);
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  float sc, sh;
  for (int j = 0; j < a.groups; ++j) bn_from_acc(a, c, ch, j, true, sc, sh);
}

// grid-stride is a multiple of the chunks-per-pixel (a power of two <= 256), so a thread's channel
// chunk never changes: scale/shift live in registers, index math is shifts.
// FUSED: scale / shift come from the exact accumulators (every block derives the vectors of all channels into LDS,
// block 0 also publishes them and updates the running statistics): no finalize launch between GEMM and this pass.
// GEN: the dropout keep-mask is drawn here (and stored for the backward) instead of by a separate fill launch.
// G2: two BatchNorm populations in one pass, pixels >= pg use the second scale/shift set (at +gstride floats).
template <typename T, bool G2, bool FUSED>
__global__ void __launch_bounds__(256) bn_apply_kernel(const char* x, char* y, int64_t pixels, int c, int ldy, int coffy,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       int act, uint8_t* drop, float drop_scale, int64_t pg, int gstride,
                                                       BnAccP fa, uint64_t drop_seed, uint32_t drop_thresh,
                                                       const u4_t* side_src, u4_t* side_dst, int64_t side_chunks) {
  constexpr int EPC = 16 / (int)sizeof(T);
  // side copy (op_bn_apply_acc): this thread's 16-byte chunks are requested first and stored after the pass's own first loads
  u4_t sc_[2] = {u4_t{0u, 0u, 0u, 0u}, u4_t{0u, 0u, 0u, 0u}};
  const int64_t sid = (int64_t)blockIdx.x * 256 + threadIdx.x, sstride = (int64_t)gridDim.x * 256;
  if (side_chunks > 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (sid + u * sstride < side_chunks) sc_[u] = side_src[sid + u * sstride];
  }
  const int cpp = c / EPC;
  const int lg = 31 - __builtin_clz(cpp);
  const int64_t total = pixels * cpp;
  const int64_t gid0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cc = (int)(gid0 & (cpp - 1));
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t esz = (int64_t)sizeof(T);
  // the pass is HBM-bound: a thread's first four 16-byte loads are issued BEFORE the scale / shift vectors are derived (FUSED:
  // a chain of dependent accumulator / parameter loads of 2 - 3 us during which every co-resident block would otherwise
  // request nothing), and from then on the next four are in flight while the current four are finished
  int64_t gid = gid0;
  bool full = gid + 3 * stride < total;
  u4_t r[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) r[u] = full ? *(const u4_t*)(x + (((gid + u * stride) >> lg) * c + cc * EPC) * esz) : u4_t{0u, 0u, 0u, 0u};
  if (side_chunks > 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (sid + u * sstride < side_chunks) side_dst[sid + u * sstride] = sc_[u];
    for (int64_t i = sid + 2 * sstride; i < side_chunks; i += sstride) side_dst[i] = side_src[i];
  }
  float sc[EPC], sh[EPC], sc1[G2 ? EPC : 1], sh1[G2 ? EPC : 1];
  if constexpr (FUSED) {
    extern __shared__ __attribute__((aligned(16))) float aff[];   // [groups][2][c]
    for (int ch = threadIdx.x; ch < c; ch += 256)
      for (int j = 0; j < fa.groups; ++j) {
        float a, b;
        bn_from_acc(fa, c, ch, j, blockIdx.x == 0, a, b);
        aff[(j * 2) * c + ch] = a;
        aff[(j * 2 + 1) * c + ch] = b;
      }
    if (blockIdx.x == 0 && fa.zero_next) zero_words64(fa.zero_next, fa.zero_words);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPC; ++e) { sc[e] = aff[cc * EPC + e]; sh[e] = aff[c + cc * EPC + e]; }
    if constexpr (G2) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) { sc1[e] = aff[2 * c + cc * EPC + e]; sh1[e] = aff[3 * c + cc * EPC + e]; }
    }
  } else {
#pragma unroll
    for (int e = 0; e < EPC; ++e) { sc[e] = scale ? scale[cc * EPC + e] : 1.f; sh[e] = scale ? shift[cc * EPC + e] : 0.f; }
    if constexpr (G2) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) { sc1[e] = scale[gstride + cc * EPC + e]; sh1[e] = shift[gstride + cc * EPC + e]; }
    }
  }
  // one 16-byte chunk: affine map + activation (+ dropout) + store. The activation and the dropout mode are the same for every
  // element of a launch: the streaming loops below run inside gi_with_act with both as compile-time constants (written as run-time
  // tests inside `finish`, hipcc kept them as scalar branches per ELEMENT: 299 branches in this kernel's 3000 instructions)
  gi_with_act(act, [&](auto ACTc) {
  constexpr int ACT = decltype(ACTc)::value;
  auto body = [&](auto DROPc) {
  constexpr int DROP = decltype(DROPc)::value;   // 0 none, 1 read the keep-mask, 2 draw it here
  auto finish = [&](int64_t pix, u4_t raw) {
    float v[EPC];
    cvt_raw<T, EPC>(raw, v);
    const bool second = G2 && pix >= pg;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float t = G2 ? fmaf(v[e], second ? sc1[e] : sc[e], second ? sh1[e] : sh[e]) : fmaf(v[e], sc[e], sh[e]);
      v[e] = gi_act_c<ACT>(t);
    }
    if constexpr (DROP != 0) {
      const int64_t e0 = pix * c + cc * EPC;
      if constexpr (DROP == 2) {     // draw the keep-mask here; the backward reads it back
        uint8_t k[EPC];
#pragma unroll
        for (int e = 0; e < EPC; ++e) k[e] = dropout_keep(drop_seed, e0 + e, drop_thresh);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = k[e] ? v[e] * drop_scale : 0.f;
        if constexpr (EPC == 8) {
          *(uint2*)(drop + e0) = uint2{(unsigned)k[0] | ((unsigned)k[1] << 8) | ((unsigned)k[2] << 16) | ((unsigned)k[3] << 24),
                                       (unsigned)k[4] | ((unsigned)k[5] << 8) | ((unsigned)k[6] << 16) | ((unsigned)k[7] << 24)};
        } else {
          *(unsigned*)(drop + e0) = (unsigned)k[0] | ((unsigned)k[1] << 8) | ((unsigned)k[2] << 16) | ((unsigned)k[3] << 24);
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = drop[e0 + e] ? v[e] * drop_scale : 0.f;
      }
    }
    store_vec<T, EPC>(y, pix * ldy + coffy + cc * EPC, v);
  };
  while (full) {
    const int64_t gn = gid + 4 * stride;
    const bool nfull = gn + 3 * stride < total;
    u4_t rn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) rn[u] = nfull ? *(const u4_t*)(x + (((gn + u * stride) >> lg) * c + cc * EPC) * esz) : u4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 4; ++u) finish((gid + u * stride) >> lg, r[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = rn[u];
    gid = gn;
    full = nfull;
  }
  for (; gid < total; gid += stride) finish(gid >> lg, *(const u4_t*)(x + ((gid >> lg) * c + cc * EPC) * esz));
  };   // body
  if (!drop) body(std::integral_constant<int, 0>{});
  else if (!drop_thresh) body(std::integral_constant<int, 1>{});
  else body(std::integral_constant<int, 2>{});
  });  // gi_with_act
}

// The end of a column pass. A workgroup covers rows_per_block rows of a dense (pixels, c) tensor; thread rl * Q + q sums the
// 16-byte channel chunk q (of Q = c / EPC) over the rows rl, rl + RL, ... (RL = 256 / Q) and arrives here with NS sums of it. They
// go to LDS (red: NS * 256 * EPC floats); with `row` non-null the lanes rl == 0 then add the rows 1 .. RL-1 in ascending order
// and store the block's partial row [NS][c] there. row null: only the exchange (the caller reads red itself).
template <int NS, int EPC>
__device__ __forceinline__ void rows_tail(float (&s)[NS][EPC], float* red, int Q, int RL, int q, int rl, float* row, int c) {
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[(k * 256 + threadIdx.x) * EPC + e] = s[k][e];
  __syncthreads();
  if (row && rl == 0) {
    for (int i = 1; i < RL; ++i)
#pragma unroll
      for (int e = 0; e < EPC; ++e)
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k][e] += red[(k * 256 + i * Q + q) * EPC + e];
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < EPC; ++e) row[k * c + q * EPC + e] = s[k][e];
  }
}

// column sum / sumsq of a dense (pixels,c) tensor -> partials [blocks][2][c]
template <typename T>
__global__ void __launch_bounds__(256) col_stats_kernel(const char* x, int64_t pixels, int c, float* partials,
                                                        int rows_per_block) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ float red[2 * 256 * EPC];
  const int Q = c / EPC, RL = 256 / Q;
  const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(pixels, r0 + rows_per_block);
  float s[2][EPC];   // sum, sum of squares
#pragma unroll
  for (int e = 0; e < EPC; ++e) s[0][e] = s[1][e] = 0.f;
  for (int64_t r = r0 + rl; r < r1; r += RL) {
    float v[EPC];
    load_vec<T, EPC>(x, r * c + q * EPC, v);
#pragma unroll
    for (int e = 0; e < EPC; ++e) { s[0][e] += v[e]; s[1][e] = fmaf(v[e], v[e], s[1][e]); }
  }
  rows_tail<2, EPC>(s, red, Q, RL, q, rl, partials + ((int64_t)blockIdx.x * 2) * c, c);
}

// ---- backward through [dropout] -> activation -> [BatchNorm] ---------------------------------
struct BwdP {
  const char* g1; int ldg1, coffg1;
  const char* g2; int ldg2, coffg2;
  const char* y; int ldy, coffy;
  const char* x;
  char* dx;
  int64_t pixels; int c; int act; float drop_scale;
  const float* gamma; const float* mean; const float* inv;
  float* partials; const float* sums;
  int rows_per_block;
  int64_t pg;        // pixels per BatchNorm population (= pixels for one group); blocks never straddle populations
  int stat_stride;   // floats between the populations' mean / inv vectors; sums are [group][2][c]
  const float* scale; const float* shift;   // non-null: the activation's sign comes from fma(x, scale, shift), the
                                            // forward's own pre-activation value, instead of a read of y
  // exact-accumulator form (stat_acc.h): the reduce pass adds {sum dz, sum dz*xhat} into acc[group][c][4] and the apply
  // pass derives its coefficients from them itself (no sums launch). acc null in the apply pass = running-statistics
  // BatchNorm (both sums zero). Block 0 of the apply pass accumulates dgamma / dbeta and clears zero_next.
  unsigned long long* acc; int acc_reps;
  float* dgamma; float* dbeta; float inv_loss_scale; float invM;
  unsigned long long* zero_next; int zero_words;
};

// One 16-byte chunk of each input of the backward: the raw tensor x, the upstream gradients g1 (unmasked) and g2 (passes the
// parent's ReLU, masked by [y > 0]) and the saved activation y. Raw, so that a thread can keep the loads of SEVERAL pixels in flight
// before it converts and computes anything (these passes are HBM-bound; with one pixel per iteration a lane has 32 - 48 bytes
// outstanding and the chip 4 - 6 MB, i.e. 2 TB/s at the ~2 us a loaded memory system takes to answer). Which of the four exist is
// the same for every chunk of a launch: the kernels the host instantiates per input combination pass constants (fields that are
// not loaded then cost no registers), the others the pointers' null-ness.
struct RawIn { u4_t x, g1, g2, y; };
template <typename T>
__device__ __forceinline__ void load_raw(const BwdP& p, int64_t pix, int ch0, bool with_x, bool has_g1, bool has_g2, bool with_y, RawIn& r) {
  constexpr int64_t ES = (int64_t)sizeof(T);
  if (with_x) r.x = *(const u4_t*)(p.x + (pix * p.c + ch0) * ES);
  if (has_g1) r.g1 = *(const u4_t*)(p.g1 + (pix * p.ldg1 + p.coffg1 + ch0) * ES);
  if (has_g2) r.g2 = *(const u4_t*)(p.g2 + (pix * p.ldg2 + p.coffg2 + ch0) * ES);
  if (with_y) r.y = *(const u4_t*)(p.y + (pix * p.ldy + p.coffy + ch0) * ES);
}
template <int EPC>
struct DzIn { float g1[EPC], g2[EPC], y[EPC]; };
template <typename T, int EPC>
__device__ __forceinline__ void unpack_raw(const RawIn& r, bool with_x, bool has_g1, bool has_g2, bool with_y, float (&xv)[EPC], DzIn<EPC>& in) {
  if (with_x) cvt_raw<T, EPC>(r.x, xv);
  if (has_g1) cvt_raw<T, EPC>(r.g1, in.g1);
  if (has_g2) cvt_raw<T, EPC>(r.g2, in.g2);
  if (with_y) cvt_raw<T, EPC>(r.y, in.y);
}
// The one-launch kernel keeps fp32 values, not raw chunks, between its sweeps: the same chunks converted as they arrive. (Through
// load_raw + unpack_raw the null tests of the loads and of the conversions stay separate branches and <half, 2> needs 99 registers
// instead of 91, four waves per SIMD instead of five.)
template <typename T, int EPC>
__device__ __forceinline__ void load_cvt(const BwdP& p, int64_t pix, int ch0, bool with_y, float (&xv)[EPC], DzIn<EPC>& in) {
  load_vec<T, EPC>(p.x, pix * p.c + ch0, xv);
  if (p.g1) load_vec<T, EPC>(p.g1, pix * p.ldg1 + p.coffg1 + ch0, in.g1);
  if (p.g2) load_vec<T, EPC>(p.g2, pix * p.ldg2 + p.coffg2 + ch0, in.g2);
  if (with_y) load_vec<T, EPC>(p.y, pix * p.ldy + p.coffy + ch0, in.y);
}
// slope of the activation's derivative on the negative side (1 / 0 / 0.2 for none / ReLU / LeakyReLU): one select per element
// instead of a test of the activation id per element (which hipcc keeps as scalar branches inside the unrolled loops)
__device__ __forceinline__ float neg_slope_of(int act) { return act == GI_ACT_LRELU ? 0.2f : (act == GI_ACT_RELU ? 0.f : 1.f); }
// dz = (g1 + [sgn > 0] g2) * slope(sgn) * drop_scale. sgn: values with the sign of the activation's input (the saved y, or
// fma(x, scale, shift) of the forward; 1 where neither g2 nor an activation asks). A missing g1 / g2 contributes 0.
template <int EPC>
__device__ __forceinline__ void dz_of(bool has_g1, bool has_g2, float ns, float drop_scale, const float (&sgn)[EPC],
                                      const float (&g1)[EPC], const float (&g2)[EPC], float (&dz)[EPC]) {
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    const bool pos = sgn[e] > 0.f;
    float g = has_g1 ? g1[e] : 0.f;
    if (has_g2) g += pos ? g2[e] : 0.f;
    const float sl = pos ? 1.f : ns;
    dz[e] = g * sl * drop_scale;
  }
}
// coefficients of the apply pass: dx = gamma*inv*(dz - s1/M - xhat*s2/M) = k1*dz + k2*x + k3 with s1 = sum dz, s2 = sum dz*xhat
__device__ __forceinline__ void bwd_coef(float gamma, float inv, float mean, float s1, float s2, float invM, float& k1, float& k2, float& k3) {
  k1 = gamma * inv;
  k2 = -k1 * inv * s2 * invM;
  k3 = -k1 * s1 * invM - k2 * mean;
}

// pass 1: partial sums of dz and dz*xhat. IN (bit 0 = g1, bit 1 = g2) / LOAD_Y: which inputs exist; the host picks the
// instantiation from the pointers
template <typename T, int IN, bool LOAD_Y>
__global__ void __launch_bounds__(256) act_bn_bwd_reduce_kernel(BwdP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr bool G1 = (IN & 1) != 0, G2 = (IN & 2) != 0;
  __shared__ float red[2 * 256 * EPC];
  const int Q = p.c / EPC, RL = 256 / Q;
  const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block, r1 = min(p.pixels, r0 + p.rows_per_block);
  float s[2][EPC], mu[EPC], iv[EPC];   // s: sum dz, sum dz*xhat
  const int so = r0 >= p.pg ? p.stat_stride : 0;
#pragma unroll
  for (int e = 0; e < EPC; ++e) { s[0][e] = s[1][e] = 0.f; mu[e] = p.mean[so + q * EPC + e]; iv[e] = p.inv[so + q * EPC + e]; }
  float sc[EPC], sh[EPC];
  if (p.scale) {
#pragma unroll
    for (int e = 0; e < EPC; ++e) { sc[e] = p.scale[so + q * EPC + e]; sh[e] = p.shift[so + q * EPC + e]; }
  }
  const float ns = neg_slope_of(p.act), drop_scale = p.drop_scale;
  constexpr int U = 4;   // rows whose loads are in flight together (the sums still run over the rows in ascending order)
  const bool have_scale = p.scale != nullptr;
  for (int64_t r = r0 + rl; r < r1; r += (int64_t)U * RL) {
    RawIn raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (r + (int64_t)u * RL < r1) load_raw<T>(p, r + (int64_t)u * RL, q * EPC, true, G1, G2, LOAD_Y, raw[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + (int64_t)u * RL < r1) {
        float dz[EPC], xv[EPC];
        DzIn<EPC> in;
        unpack_raw<T, EPC>(raw[u], true, G1, G2, LOAD_Y, xv, in);
        if constexpr (!LOAD_Y) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) in.y[e] = have_scale ? fmaf(xv[e], sc[e], sh[e]) : 1.f;
        }
        dz_of<EPC>(G1, G2, ns, drop_scale, in.y, in.g1, in.g2, dz);
#pragma unroll
        for (int e = 0; e < EPC; ++e) { s[0][e] += dz[e]; s[1][e] = fmaf(dz[e], (xv[e] - mu[e]) * iv[e], s[1][e]); }
      }
    }
  }
  rows_tail<2, EPC>(s, red, Q, RL, q, rl, p.acc ? nullptr : p.partials + ((int64_t)blockIdx.x * 2) * p.c, p.c);
  if (p.acc) {   // one lane per channel: the lanes of an atomic instruction are consecutive words (stat_acc.h)
    const int grp = r0 >= p.pg ? 1 : 0, rep = blockIdx.x & (p.acc_reps - 1);
    for (int ch = threadIdx.x; ch < p.c; ch += 256) {
      float a = 0.f, b = 0.f;
      for (int i = 0; i < RL; ++i) { a += red[i * Q * EPC + ch]; b += red[256 * EPC + i * Q * EPC + ch]; }
      gi_stat_add(p.acc, p.c, rep, grp, 0, ch, a);
      gi_stat_add(p.acc, p.c, rep, grp, 1, ch, b);
    }
  }
}

// partials [rows][2][c] -> sums [2][c]; also accumulates dgamma/dbeta
// groups > 1: `rows` partial rows per population, one after the other; the parameter gradients accumulate population by
// population (the order of separate calls). Output per population [8][c]: s1, s2, then the coefficients of the apply pass
// (bwd_coef) and the forward's scale / shift.
// rows = 0 (running-statistics BatchNorm): s1 = s2 = 0, dx = gamma*inv*dz.
__global__ void __launch_bounds__(256) bwd_sums_kernel(const float* partials, int rows, int c, float* sums, float* dgamma,
                                                       float* dbeta, float inv_loss_scale, int groups, const float* gamma,
                                                       const float* mean, const float* inv, const float* scale,
                                                       const float* shift, int stat_stride, float invM) {
  __shared__ double sh[8];
  const int ch = blockIdx.x;
  for (int j = 0; j < groups; ++j) {
    const float* pj = partials + (int64_t)j * rows * 2 * c;
    double s = 0.0, q = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) {
      s += (double)pj[((int64_t)r * 2) * c + ch];
      q += (double)pj[((int64_t)r * 2 + 1) * c + ch];
    }
    block_sum2(s, q, sh);
    if (threadIdx.x == 0) {
      float* o = sums + (int64_t)j * 8 * c;
      const float s1 = (float)s, s2 = (float)q;
      o[ch] = s1;
      o[c + ch] = s2;
      if (dbeta) dbeta[ch] += s1 * inv_loss_scale;
      if (dgamma) dgamma[ch] += s2 * inv_loss_scale;
      const int so = j * stat_stride + ch;
      float k1, k2, k3;
      bwd_coef(gamma[ch], inv[so], mean[so], s1, s2, invM, k1, k2, k3);
      o[2 * c + ch] = k1;
      o[3 * c + ch] = k2;
      o[4 * c + ch] = k3;
      o[5 * c + ch] = scale ? scale[so] : 0.f;
      o[6 * c + ch] = scale ? shift[so] : 0.f;
    }
  }
}

// The prologue of the accumulator path's apply pass: every workgroup derives the coefficient vectors of all channels from the
// exact accumulators (BwdP::acc; null = running-statistics BatchNorm, both sums zero) into LDS - coef [groups][5][c]: k1, k2, k3,
// forward scale, forward shift - block 0 also adds dgamma / dbeta and clears zero_next. Ends with the barrier.
template <int NG>
__device__ __forceinline__ void bwd_coef_to_lds(const BwdP& p, float* coef) {
  const int c = p.c;
  for (int ch = threadIdx.x; ch < c; ch += 256)
    for (int g = 0; g < NG; ++g) {
      const int so = g * p.stat_stride + ch;
      // (parameter loads first: they and the accumulator words are one memory round trip, not two)
      const float iv = p.inv[so], gam = p.gamma[ch], mu = p.mean[so];
      const float fsc = p.scale ? p.scale[so] : 0.f, fsh = p.scale ? p.shift[so] : 0.f;
      float s1 = 0.f, s2 = 0.f;
      if (p.acc) {
        double t1, t2;
        gi_stat_read2(p.acc, c, p.acc_reps, g, ch, t1, t2);
        s1 = (float)t1;
        s2 = (float)t2;
      }
      float k1, k2, k3;
      bwd_coef(gam, iv, mu, s1, s2, p.invM, k1, k2, k3);
      float* o = coef + (int64_t)g * 5 * c;
      o[ch] = k1;
      o[c + ch] = k2;
      o[2 * c + ch] = k3;
      o[3 * c + ch] = fsc;
      o[4 * c + ch] = fsh;
      if (blockIdx.x == 0) {     // parameter gradients accumulate population by population, as separate calls would
        if (p.dbeta) p.dbeta[ch] += s1 * p.inv_loss_scale;
        if (p.dgamma) p.dgamma[ch] += s2 * p.inv_loss_scale;
      }
    }
  if (blockIdx.x == 0 && p.zero_next) zero_words64(p.zero_next, p.zero_words);
  __syncthreads();
}

// pass 2 (or the only pass when there is no BatchNorm): writes dx. HAS_BN: dx = k1*dz + k2*x + k3 (bwd_coef); the grid stride is
// a multiple of the chunks per pixel, so a thread's channels never change and the coefficients (both populations' with G2) stay
// in registers. HAS_BN = 1: they are the rows bwd_sums_kernel wrote ([group][8][c]); HAS_BN = 2: they come from the exact
// accumulators (bwd_coef_to_lds)
template <typename T, int HAS_BN, bool G2>
__global__ void __launch_bounds__(256) act_bn_bwd_apply_kernel(BwdP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int cpp = p.c / EPC;
  const int lg = 31 - __builtin_clz(cpp);
  const int64_t total = p.pixels * cpp;
  const int64_t gid0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cc = (int)(gid0 & (cpp - 1));
  constexpr int NG = G2 ? 2 : 1;
  constexpr int U = 4;   // chunks whose loads are in flight together
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool has_g1 = p.g1 != nullptr, has_g2 = p.g2 != nullptr;
  const bool need_y = has_g2 || p.act != GI_ACT_NONE;
  const bool load_y = need_y && !(HAS_BN && p.scale);
  const float ns = neg_slope_of(p.act), drop_scale = p.drop_scale;
  // the first U chunks are requested BEFORE the coefficients are derived (HAS_BN == 2: a chain of dependent accumulator and
  // parameter loads during which all co-resident blocks would otherwise request nothing)
  RawIn raw[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (gid0 + u * stride < total) load_raw<T>(p, (gid0 + u * stride) >> lg, cc * EPC, HAS_BN != 0, has_g1, has_g2, load_y, raw[u]);
  float k1[NG][EPC], k2[NG][EPC], k3[NG][EPC], sc[NG][EPC], sh[NG][EPC];
  if constexpr (HAS_BN == 2) {
    extern __shared__ __attribute__((aligned(16))) float coef[];   // [groups][5][c]: k1, k2, k3, scale, shift
    bwd_coef_to_lds<NG>(p, coef);
    const int c = p.c;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float* o = coef + (int64_t)g * 5 * c + cc * EPC;
#pragma unroll
      for (int e = 0; e < EPC; ++e) { k1[g][e] = o[e]; k2[g][e] = o[c + e]; k3[g][e] = o[2 * c + e]; sc[g][e] = o[3 * c + e]; sh[g][e] = o[4 * c + e]; }
    }
  } else if constexpr (HAS_BN == 1) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const float* o = p.sums + (int64_t)g * 8 * p.c + cc * EPC;
      load_f32<EPC>(o + 2 * p.c, k1[g]);
      load_f32<EPC>(o + 3 * p.c, k2[g]);
      load_f32<EPC>(o + 4 * p.c, k3[g]);
      if (p.scale) {
        load_f32<EPC>(o + 5 * p.c, sc[g]);
        load_f32<EPC>(o + 6 * p.c, sh[g]);
      }
    }
  }
  for (int64_t gid = gid0; gid < total; gid += U * stride) {
    if (gid != gid0) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (gid + u * stride < total) load_raw<T>(p, (gid + u * stride) >> lg, cc * EPC, HAS_BN != 0, has_g1, has_g2, load_y, raw[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (gid + u * stride >= total) break;
      const int64_t pix = (gid + u * stride) >> lg;
      float dz[EPC], xv[EPC];
      DzIn<EPC> in;
      unpack_raw<T, EPC>(raw[u], HAS_BN != 0, has_g1, has_g2, load_y, xv, in);
      if constexpr (HAS_BN == 0) {
        if (!need_y) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) in.y[e] = 1.f;
        }
        dz_of<EPC>(has_g1, has_g2, ns, drop_scale, in.y, in.g1, in.g2, dz);
      } else {
        const int g = (G2 && pix >= p.pg) ? 1 : 0;
        if (p.scale || !need_y) {
#pragma unroll
          for (int e = 0; e < EPC; ++e) in.y[e] = p.scale ? fmaf(xv[e], G2 ? (g ? sc[NG - 1][e] : sc[0][e]) : sc[0][e], G2 ? (g ? sh[NG - 1][e] : sh[0][e]) : sh[0][e]) : 1.f;
        }
        dz_of<EPC>(has_g1, has_g2, ns, drop_scale, in.y, in.g1, in.g2, dz);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const float a1 = G2 ? (g ? k1[NG - 1][e] : k1[0][e]) : k1[0][e];
          const float a2 = G2 ? (g ? k2[NG - 1][e] : k2[0][e]) : k2[0][e];
          const float a3 = G2 ? (g ? k3[NG - 1][e] : k3[0][e]) : k3[0][e];
          dz[e] = fmaf(a1, dz[e], fmaf(a2, xv[e], a3));
        }
      }
      store_vec<T, EPC>(p.dx, pix * p.c + cc * EPC, dz);
    }
  }
}

// The apply pass of the accumulator path (HAS_BN == 2) for the input combinations the networks produce (apply_acc_built), built
// for bytes in flight: measured with hardware counters (round 3, critic conv2 at n = 64: 200 MB in 57 us), a wave of the generic
// kernel above lives ~18 us - a chain of dependent accumulator / parameter loads, then eight load -> wait -> compute -> store rounds - and its 100 - 250 registers leave 2 - 4
// waves per SIMD, so the chip has ~7 MB outstanding where a plain copy of the same three streams runs at 6.7 TB/s
// (tools/micro/stream_bw.hip). Here the coefficient vectors stay in LDS (ten ds_read_b128 per chunk instead of 40 - 80
// registers), only the pointers that exist are loaded (IN: 1 = g1, 2 = g2 masked by the activation's sign, 3 = both; LOAD_Y: the
// sign comes from the saved activation, else from fma(x, scale, shift)), two chunks per thread are requested before the
// coefficients are derived and the next two before the current two are finished.
// Same arithmetic, same order: results are bit-identical to the generic kernel.
// (critic: g1; encoder: g1 + g2; decoder: g2, with the saved activation where dropout follows the norm; anything else takes the
// generic kernel: built for every combination, the others need a private segment and fp32 <3, true> 106 registers, below the
// occupancy of the five)
constexpr bool apply_acc_built(int in, bool load_y, bool g2) { return load_y ? (in == 2 && !g2) : (in == 1 || !g2); }
template <typename T, int IN, bool LOAD_Y, bool G2>
__global__ void __launch_bounds__(256) act_bn_bwd_apply_acc_kernel(BwdP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr bool G1IN = (IN & 1) != 0, G2IN = (IN & 2) != 0;
  constexpr int U = 2;
  extern __shared__ __attribute__((aligned(16))) float coef[];   // [groups][5][c]: k1, k2, k3, scale, shift
  const int c = p.c;
  const int cpp = c / EPC;
  const int lg = 31 - __builtin_clz(cpp);
  const int64_t total = p.pixels * cpp;
  const int64_t gid0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cc = (int)(gid0 & (cpp - 1));
  const int64_t stride = (int64_t)gridDim.x * 256;
  RawIn cur[U], nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (gid0 + u * stride < total) load_raw<T>(p, (gid0 + u * stride) >> lg, cc * EPC, true, G1IN, G2IN, LOAD_Y, cur[u]);
  bwd_coef_to_lds<G2 ? 2 : 1>(p, coef);
  const bool have_scale = p.scale != nullptr;
  const float ns = neg_slope_of(p.act);
  const float drop_scale = p.drop_scale;
  for (int64_t gid = gid0; gid < total; gid += U * stride) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (gid + (U + u) * stride < total) load_raw<T>(p, (gid + (U + u) * stride) >> lg, cc * EPC, true, G1IN, G2IN, LOAD_Y, nxt[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (gid + u * stride < total) {
        const int64_t pix = (gid + u * stride) >> lg;
        const float* o = coef + ((G2 && pix >= p.pg) ? 5 * c : 0) + cc * EPC;
        float xv[EPC], k[EPC], out[EPC];
        DzIn<EPC> in;
        unpack_raw<T, EPC>(cur[u], true, G1IN, G2IN, LOAD_Y, xv, in);
        if constexpr (!LOAD_Y) {
          float scv[EPC], shv[EPC];
          load_f32<EPC>(o + 3 * c, scv);
          load_f32<EPC>(o + 4 * c, shv);
#pragma unroll
          for (int e = 0; e < EPC; ++e) in.y[e] = have_scale ? fmaf(xv[e], scv[e], shv[e]) : 1.f;
        }
        dz_of<EPC>(G1IN, G2IN, ns, drop_scale, in.y, in.g1, in.g2, out);
        // dx = k1 * dz + (k2 * x + k3), the same fmaf nest as the generic kernel
        float k1v[EPC], k3v[EPC];
        load_f32<EPC>(o, k1v);
        load_f32<EPC>(o + c, k);
        load_f32<EPC>(o + 2 * c, k3v);
#pragma unroll
        for (int e = 0; e < EPC; ++e) out[e] = fmaf(k1v[e], out[e], fmaf(k[e], xv[e], k3v[e]));
        store_vec<T, EPC>(p.dx, pix * c + cc * EPC, out);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
  }
}

// Small tensors (the U-Net's innermost levels: <= 512 pixels by default, the kernel serves up to 2048): reduce and apply in ONE launch. A workgroup owns a 16-byte
// channel chunk and all pixels, every thread holds its <= 8 chunks of dz and x in registers: sums of dz and dz * xhat (fp32
// per thread, double across the block, fixed order: reproducible), coefficients, dx. The two-launch form costs 13 + 14 us
// per layer there, almost all of it launch and accumulator round trips (12 us in this form). Beyond ~512 pixels the
// channel-chunk-per-workgroup layout loses: a workgroup uses 16 bytes of every 128-byte line it touches (28 us at 2048 pixels).
template <typename T, int NIT>   // NIT = pixels / 256 rounded up: every thread keeps its NIT chunks (dz, x) in registers between the sweeps
__global__ void __launch_bounds__(256) act_bn_bwd_small_kernel(BwdP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ double sh[8];
  __shared__ float coef[3 * 8];
  const int cc = blockIdx.x;
  float mu[EPC], iv[EPC], sc[EPC], shf[EPC], s[EPC], sx[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    mu[e] = p.mean[cc * EPC + e]; iv[e] = p.inv[cc * EPC + e];
    sc[e] = p.scale ? p.scale[cc * EPC + e] : 0.f; shf[e] = p.scale ? p.shift[cc * EPC + e] : 0.f;
    s[e] = sx[e] = 0.f;
  }
  const bool need_y = p.g2 != nullptr || p.act != GI_ACT_NONE;
  float xr[NIT][EPC], dzr[NIT][EPC];
  DzIn<EPC> in[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {    // all loads first
    const int64_t pix = threadIdx.x + it * 256;
    if (pix < p.pixels) load_cvt<T, EPC>(p, pix, cc * EPC, need_y && !p.scale, xr[it], in[it]);
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t pix = threadIdx.x + it * 256;
    if (pix < p.pixels) {
      if (p.scale || !need_y) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) in[it].y[e] = p.scale ? fmaf(xr[it][e], sc[e], shf[e]) : 1.f;
      }
      dz_of<EPC>(p.g1 != nullptr, p.g2 != nullptr, neg_slope_of(p.act), p.drop_scale, in[it].y, in[it].g1, in[it].g2, dzr[it]);
#pragma unroll
      for (int e = 0; e < EPC; ++e) { s[e] += dzr[it][e]; sx[e] = fmaf(dzr[it][e], (xr[it][e] - mu[e]) * iv[e], sx[e]); }
    }
  }
  __shared__ float tot[2 * 8];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    double a = s[e], b = sx[e];
    block_sum2(a, b, sh);
    if (threadIdx.x == 0) { tot[e] = (float)a; tot[8 + e] = (float)b; }
  }
  __syncthreads();
  if (threadIdx.x < EPC) {     // one lane per channel: the parameter-gradient updates overlap instead of queueing behind one lane
    const int e = threadIdx.x, ch = cc * EPC + e;
    const float s1 = tot[e], s2 = tot[8 + e];
    float k1, k2, k3;
    bwd_coef(p.gamma[ch], p.inv[ch], p.mean[ch], s1, s2, p.invM, k1, k2, k3);
    coef[e] = k1; coef[8 + e] = k2; coef[16 + e] = k3;
    if (p.dbeta) p.dbeta[ch] += s1 * p.inv_loss_scale;
    if (p.dgamma) p.dgamma[ch] += s2 * p.inv_loss_scale;
  }
  if (blockIdx.x == 0 && p.zero_next) zero_words64(p.zero_next, p.zero_words);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int64_t pix = threadIdx.x + it * 256;
    if (pix < p.pixels) {
      float o[EPC];
#pragma unroll
      for (int e = 0; e < EPC; ++e) o[e] = fmaf(coef[e], dzr[it][e], fmaf(coef[8 + e], xr[it][e], coef[16 + e]));
      store_vec<T, EPC>(p.dx, pix * p.c + cc * EPC, o);
    }
  }
}

// ---- InstanceNorm2d(affine=False, track_running_stats=False), get_norm_layer('instance') (networks.py:38-40) -------------
// Statistics per (image, channel) over the H*W pixels, eps 1e-5, the same in train and eval mode; no parameters. One
// workgroup owns (image, 16-byte channel chunk): a first sweep over the image's pixels sums x and x^2 (fp32 per thread,
// double across the block, fixed order), a second one writes act((x - mean) * inv) (+ dropout) - the plane is re-read
// from L2. stats [n][c][2] keeps mean / inv for the backward.
template <typename T>
__global__ void __launch_bounds__(256) in_forward_kernel(const char* x, char* y, int hw, int c, int ldy, int coffy, int act,
                                                         const uint8_t* drop, float drop_scale, float eps, float* stats) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ double sh[8];
  __shared__ float aff[2 * 8];
  const int cpp = c / EPC;
  const int img = blockIdx.x / cpp, cc = blockIdx.x % cpp;
  const int64_t p0 = (int64_t)img * hw;
  float s[EPC], q[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) s[e] = q[e] = 0.f;
  for (int i = threadIdx.x; i < hw; i += 256) {
    float v[EPC];
    load_vec<T, EPC>(x, (p0 + i) * c + cc * EPC, v);
#pragma unroll
    for (int e = 0; e < EPC; ++e) { s[e] += v[e]; q[e] = fmaf(v[e], v[e], q[e]); }
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    double a = s[e], b = q[e];
    block_sum2(a, b, sh);
    if (threadIdx.x == 0) {
      const double m = a / hw;
      double var = b / hw - m * m;
      if (var < 0.0 || hw == 1) var = 0.0;   // (one pixel has no spread: what is left is the fp32 rounding of its square)
      const float inv = 1.0f / sqrtf((float)var + eps);
      aff[e] = (float)m; aff[8 + e] = inv;
      stats[((int64_t)img * c + cc * EPC + e) * 2] = (float)m;
      stats[((int64_t)img * c + cc * EPC + e) * 2 + 1] = inv;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < hw; i += 256) {
    float v[EPC];
    load_vec<T, EPC>(x, (p0 + i) * c + cc * EPC, v);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      float t = (v[e] - aff[e]) * aff[8 + e];
      if (act == GI_ACT_RELU) t = t > 0.f ? t : 0.f;
      else if (act == GI_ACT_LRELU) t = t > 0.f ? t : 0.2f * t;
      v[e] = t;
    }
    if (drop) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[e] = drop[(p0 + i) * c + cc * EPC + e] ? v[e] * drop_scale : 0.f;
    }
    store_vec<T, EPC>(y, (p0 + i) * ldy + coffy + cc * EPC, v);
  }
}

// backward through [dropout] -> activation -> InstanceNorm: dz as in act_bn_bwd (the masks come from the saved output y),
//   dx = inv * (dz - mean_p dz - xhat * mean_p (dz * xhat)),  the means over the pixels of ONE (image, channel)
template <typename T>
__global__ void __launch_bounds__(256) act_in_bwd_kernel(BwdP p, int hw, const float* stats) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ double sh[8];
  __shared__ float red[2 * 8];
  const int cpp = p.c / EPC;
  const int img = blockIdx.x / cpp, cc = blockIdx.x % cpp;
  const int64_t p0 = (int64_t)img * hw;
  float mu[EPC], iv[EPC], s[EPC], sx[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    mu[e] = stats[((int64_t)img * p.c + cc * EPC + e) * 2];
    iv[e] = stats[((int64_t)img * p.c + cc * EPC + e) * 2 + 1];
    s[e] = sx[e] = 0.f;
  }
  const bool has_g1 = p.g1 != nullptr, has_g2 = p.g2 != nullptr;
  const bool need_y = has_g2 || p.act != GI_ACT_NONE;
  const float ns = neg_slope_of(p.act), drop_scale = p.drop_scale;
  auto dz_x = [&](int64_t pix, float (&dz)[EPC], float (&xv)[EPC]) {   // both sweeps: dz and x of one chunk
    RawIn raw;
    DzIn<EPC> in;
    load_raw<T>(p, pix, cc * EPC, true, has_g1, has_g2, need_y, raw);
    unpack_raw<T, EPC>(raw, true, has_g1, has_g2, need_y, xv, in);
    if (!need_y) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) in.y[e] = 1.f;
    }
    dz_of<EPC>(has_g1, has_g2, ns, drop_scale, in.y, in.g1, in.g2, dz);
  };
  for (int i = threadIdx.x; i < hw; i += 256) {
    float dz[EPC], xv[EPC];
    dz_x(p0 + i, dz, xv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) { s[e] += dz[e]; sx[e] = fmaf(dz[e], (xv[e] - mu[e]) * iv[e], sx[e]); }
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
    double a = s[e], b = sx[e];
    block_sum2(a, b, sh);
    if (threadIdx.x == 0) { red[e] = (float)(a / hw); red[8 + e] = (float)(b / hw); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < hw; i += 256) {
    float dz[EPC], xv[EPC];
    dz_x(p0 + i, dz, xv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) dz[e] = iv[e] * (dz[e] - red[e] - (xv[e] - mu[e]) * iv[e] * red[8 + e]);
    store_vec<T, EPC>(p.dx, (p0 + i) * p.c + cc * EPC, dz);
  }
}

// bias gradient of a convolution: dbias[ch] += scale * sum over the partial rows of column sums (col_stats_kernel)
__global__ void __launch_bounds__(256) bias_grad_kernel(const float* partials, int rows, int c, float scale, float* dbias) {
  __shared__ double sh[8];
  const int ch = blockIdx.x;
  double s = 0.0, dummy = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += (double)partials[((int64_t)r * 2) * c + ch];
  block_sum2(s, dummy, sh);
  if (threadIdx.x == 0) dbias[ch] += (float)(s * scale);
}

// ---- BatchNorm tangent injection (WGAN-GP extension) ------------------------------------
// BatchNorm (train mode) tangent map tz = (gamma/sigma)(tx - mean(tx) - xhat*mean(xhat*tx)). Its dependence
// on the PRIMAL x (through sigma and xhat) sends a gradient into x when the tangent graph is
// differentiated: with a = slope(y) * d(ta) (gradient w.r.t. tz), per channel
//   A   = sum(a*u),  u = tx - m1 - xhat*m2,  m1 = mean(tx), m2 = mean(xhat*tx)
//   inj = -(gamma*inv^2)(xhat/M) A - gamma*inv*( m2*P(a) + mean(a*xhat)*P(tx) ),  P(w) = inv*(w - mean(w) - xhat*mean(w*xhat))
//   dgamma += A*inv
// pass 1: partial sums [blocks][5][c] of a, a*xhat, tx, tx*xhat, a*tx
struct InjP {
  const char* dta; const char* y; const char* tx; const char* x; char* dxp;   // dxp: += inj (in place on the primal gradient)
  int64_t pixels; int c;
  const float* gamma; const float* mean; const float* inv;
  float* partials; const float* sums; float* dgamma; float dgamma_scale;   // dgamma += dgamma_scale * A * inv
  int rows_per_block;
};
template <typename T>
__global__ void __launch_bounds__(256) bn_inject_reduce_kernel(InjP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ float red[5 * 256 * EPC];
  const int Q = p.c / EPC, RL = 256 / Q;
  const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block, r1 = min(p.pixels, r0 + p.rows_per_block);
  float s[5][EPC], mu[EPC], iv[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k][e] = 0.f;
    mu[e] = p.mean[q * EPC + e];
    iv[e] = p.inv[q * EPC + e];
  }
  for (int64_t r = r0 + rl; r < r1; r += RL) {
    float d[EPC], yv[EPC], t[EPC], xv[EPC];
    load_vec<T, EPC>(p.dta, r * p.c + q * EPC, d);
    load_vec<T, EPC>(p.y, r * p.c + q * EPC, yv);
    load_vec<T, EPC>(p.tx, r * p.c + q * EPC, t);
    load_vec<T, EPC>(p.x, r * p.c + q * EPC, xv);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const float a = d[e] * (yv[e] > 0.f ? 1.f : 0.2f);
      const float xh = (xv[e] - mu[e]) * iv[e];
      s[0][e] += a; s[1][e] = fmaf(a, xh, s[1][e]); s[2][e] += t[e]; s[3][e] = fmaf(t[e], xh, s[3][e]); s[4][e] = fmaf(a, t[e], s[4][e]);
    }
  }
  rows_tail<5, EPC>(s, red, Q, RL, q, rl, p.partials + ((int64_t)blockIdx.x * 5) * p.c, p.c);
}
__global__ void __launch_bounds__(256) bn_inject_sums_kernel(const float* partials, int rows, int c, float* sums) {
  __shared__ double sh[5][256];
  const int ch = blockIdx.x;
  double s[5] = {0, 0, 0, 0, 0};
  for (int r = threadIdx.x; r < rows; r += 256)
    for (int k = 0; k < 5; ++k) s[k] += (double)partials[((int64_t)r * 5 + k) * c + ch];
  for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) for (int k = 0; k < 5; ++k) sums[k * c + ch] = (float)sh[k][0];
}
template <typename T>
__global__ void __launch_bounds__(256) bn_inject_apply_kernel(InjP p) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int cpp = p.c / EPC;
  const int64_t total = p.pixels * cpp;
  const float M = (float)p.pixels, invM = 1.f / M;
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    const int cc = (int)(gid % cpp);
    const int64_t pix = gid / cpp;
    float d[EPC], yv[EPC], t[EPC], xv[EPC], o[EPC];
    load_vec<T, EPC>(p.dta, pix * p.c + cc * EPC, d);
    load_vec<T, EPC>(p.y, pix * p.c + cc * EPC, yv);
    load_vec<T, EPC>(p.tx, pix * p.c + cc * EPC, t);
    load_vec<T, EPC>(p.x, pix * p.c + cc * EPC, xv);
    load_vec<T, EPC>(p.dxp, pix * p.c + cc * EPC, o);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int ch = cc * EPC + e;
      const float inv = p.inv[ch], g = p.gamma[ch];
      const float a = d[e] * (yv[e] > 0.f ? 1.f : 0.2f);
      const float xh = (xv[e] - p.mean[ch]) * inv;
      const float Sa = p.sums[ch], Sax = p.sums[p.c + ch], St = p.sums[2 * p.c + ch], Stx = p.sums[3 * p.c + ch], Sat = p.sums[4 * p.c + ch];
      const float m2 = Stx * invM, max_ = Sax * invM;
      const float A = Sat - Sa * St * invM - Sax * Stx * invM;
      const float Pa = inv * (a - Sa * invM - xh * max_);
      const float Pt = inv * (t[e] - St * invM - xh * m2);
      o[e] += -(g * inv * inv) * (xh * invM) * A - g * inv * (m2 * Pa + max_ * Pt);
    }
    store_vec<T, EPC>(p.dxp, pix * p.c + cc * EPC, o);
  }
  if (p.dgamma && blockIdx.x == 0) {
    for (int ch = threadIdx.x; ch < p.c; ch += 256) {
      const float Sa = p.sums[ch], Sax = p.sums[p.c + ch], St = p.sums[2 * p.c + ch], Stx = p.sums[3 * p.c + ch], Sat = p.sums[4 * p.c + ch];
      p.dgamma[ch] += (Sat - Sa * St * invM - Sax * Stx * invM) * p.inv[ch] * p.dgamma_scale;
    }
  }
}

// the chunked passes take c as a power-of-two number (<= 256) of 16-byte chunks
inline bool chunks_ok(int dtype, int c) {
  const int epc = dtype == GI_F16 ? 8 : 4;
  return c % epc == 0 && gi_is_pow2(c / epc) && c / epc <= 256;
}

}  // namespace

// =================================================================================================
int op_bn_finalize(hipStream_t st, const float* partials, int rows, int c, int64_t count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float* scale, float* shift,
                   float* save_mean, float* save_invstd, int train, float momentum, float eps, int groups,
                   int64_t part_stride, int out_stride) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(c), dim3(256), 0, st, partials, rows, c, (float)count, gamma, beta,
                     running_mean, running_var, scale, shift, save_mean, save_invstd, train, momentum, eps, groups, part_stride,
                     out_stride);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_bn_apply(hipStream_t st, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy,
                const float* scale, const float* shift, int act, const uint8_t* drop_mask, float drop_scale, int64_t pg,
                int gstride) {
  GI_REQUIRE(chunks_ok(dtype, c), "bn_apply: c=%d", c);
  const bool g2 = pg > 0 && pg < pixels;
  GI_REQUIRE(!g2 || scale, "bn_apply: two groups need scale/shift");
  const int grid = nblocks(pixels * (c / (dtype == GI_F16 ? 8 : 4)), 4);
  gi_with_dtype(dtype, [&](auto tag) { gi_with_bool(g2, [&](auto G2c) {
    hipLaunchKernelGGL((bn_apply_kernel<typename decltype(tag)::type, decltype(G2c)::value, false>), dim3(grid), dim3(256), 0, st, (const char*)x, (char*)y, pixels, c, ldy,
                       coffy, scale, shift, act, (uint8_t*)drop_mask, drop_scale, pg, gstride, BnAccP{}, (uint64_t)0, (uint32_t)0,
                       (const u4_t*)nullptr, (u4_t*)nullptr, (int64_t)0);
  }); });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_bn_finalize_acc(hipStream_t st, int c, const BnAccArgs& b) {
  GI_REQUIRE(b.groups == 1 || b.groups == 2, "bn_finalize_acc: groups=%d", b.groups);
  BnAccP fa;
  gi_fill_acc_params(fa, b);
  hipLaunchKernelGGL(bn_finalize_acc_kernel, dim3((c + 255) / 256), dim3(256), 0, st, fa, c);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_bn_apply_acc(hipStream_t st, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy, int act,
                    uint8_t* drop_mask, float drop_scale, uint64_t drop_seed, float drop_p, const BnAccArgs& b,
                    const void* side_src, void* side_dst, int64_t side_bytes) {
  GI_REQUIRE(side_bytes % 16 == 0 && (side_bytes == 0 || (side_src && side_dst)), "bn_apply_acc: side copy of %lld bytes", (long long)side_bytes);
  GI_REQUIRE(chunks_ok(dtype, c), "bn_apply_acc: c=%d", c);
  GI_REQUIRE(b.groups == 1 || b.groups == 2, "bn_apply_acc: groups=%d", b.groups);
  GI_REQUIRE(pixels % b.groups == 0 && b.count == pixels / b.groups, "bn_apply_acc: %lld pixels, %d populations of %lld", (long long)pixels,
             b.groups, (long long)b.count);
  // fewer, fatter blocks than the plain pass: every block derives the affine maps of all channels first
  int grid = nblocks(pixels * (c / (dtype == GI_F16 ? 8 : 4)), 8);
  // at most the 1024 workgroups that are resident at once (126 VGPRs: four per CU): a second round would derive the affine maps again
  // (the critic's conv2 pass at 64 images: 2048 -> 1024 workgroups, 35.5 -> 33.4 us)
  if (grid > 1024) grid = 1024;
  BnAccP fa;
  gi_fill_acc_params(fa, b);
  const size_t lds = (size_t)b.groups * 2 * c * sizeof(float);
  const uint32_t thresh = drop_p > 0.f ? gi_dropout_thresh(drop_p) : 0u;
  gi_with_dtype(dtype, [&](auto tag) { gi_with_bool(b.groups == 2, [&](auto G2c) {
    hipLaunchKernelGGL((bn_apply_kernel<typename decltype(tag)::type, decltype(G2c)::value, true>), dim3(grid), dim3(256), lds, st, (const char*)x, (char*)y, pixels, c, ldy,
                       coffy, (const float*)nullptr, (const float*)nullptr, act, drop_mask, drop_scale, (int64_t)b.count, 0, fa, drop_seed, thresh,
                       (const u4_t*)side_src, (u4_t*)side_dst, side_bytes / 16);
  }); });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

static int rows_per_block_for(int64_t pixels, int* blocks_out) {
  int64_t rpb = (pixels + 1023) / 1024;
  if (rpb < 32) rpb = 32;
  *blocks_out = (int)((pixels + rpb - 1) / rpb);
  return (int)rpb;
}

int op_col_stats(hipStream_t st, int dtype, const void* x, int64_t pixels, int c, float* partials, int* rows_out) {
  GI_REQUIRE(chunks_ok(dtype, c), "col_stats: c=%d unsupported", c);
  int blocks;
  const int rpb = rows_per_block_for(pixels, &blocks);
  gi_with_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(col_stats_kernel<typename decltype(tag)::type>, dim3(blocks), dim3(256), 0, st, (const char*)x, pixels, c, partials, rpb);
  });
  GI_LAUNCH_CHECK();
  *rows_out = blocks;
  return GI_OK;
}

int op_bwd_rows_per_block(int64_t pixels) {
  int blocks;
  return rows_per_block_for(pixels, &blocks);
}

// the fields of BwdP that are the caller's own; op_act_bn_bwd sets what depends on the path (populations, accumulators) afterwards
static BwdP fill_bwd(const ActBnBwdArgs& a) {
  BwdP p = {};
  p.g1 = (const char*)a.g1; p.ldg1 = a.ldg1; p.coffg1 = a.coffg1;
  p.g2 = (const char*)a.g2; p.ldg2 = a.ldg2; p.coffg2 = a.coffg2;
  p.y = (const char*)a.y; p.ldy = a.ldy; p.coffy = a.coffy;
  p.x = (const char*)a.x; p.dx = (char*)a.dx;
  p.pixels = a.pixels; p.c = a.c; p.act = a.act; p.drop_scale = a.drop_scale;
  p.gamma = a.gamma; p.mean = a.save_mean; p.inv = a.save_invstd;
  p.partials = a.partials; p.sums = a.sums;
  p.scale = a.has_bn ? a.fwd_scale : nullptr; p.shift = a.has_bn ? a.fwd_shift : nullptr;
  p.pg = a.pixels; p.stat_stride = a.stat_stride;
  p.acc_reps = a.acc_reps > 0 ? a.acc_reps : 1; p.dgamma = a.dgamma; p.dbeta = a.dbeta; p.inv_loss_scale = a.inv_loss_scale;
  return p;
}

static int launch_bwd_reduce(hipStream_t st, int dtype, const BwdP& p, int blocks) {
  const bool need_y = p.g2 != nullptr || p.act != GI_ACT_NONE;
  gi_with_dtype(dtype, [&](auto tag) { gi_with_int<1, 2, 3>((p.g1 ? 1 : 0) | (p.g2 ? 2 : 0), [&](auto INc) { gi_with_bool(need_y && !p.scale, [&](auto LYc) {
    hipLaunchKernelGGL((act_bn_bwd_reduce_kernel<typename decltype(tag)::type, decltype(INc)::value, decltype(LYc)::value>), dim3(blocks), dim3(256), 0, st, p);
  }); }); });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_act_bn_bwd(hipStream_t st, int dtype, const ActBnBwdArgs& a) {
  GI_REQUIRE(chunks_ok(dtype, a.c), "act_bn_bwd: c=%d unsupported", a.c);
  GI_REQUIRE(!a.has_bn || a.g1 || a.g2, "act_bn_bwd: no upstream gradient");   // (the kernels picked by input combination read what it names)
  const int Q = a.c / (dtype == GI_F16 ? 8 : 4);
  BwdP p = fill_bwd(a);
  const int groups = (a.groups == 2 && a.has_bn && !a.eval_bn) ? 2 : 1;
  GI_REQUIRE(a.groups <= 1 || groups == 2, "act_bn_bwd: groups=%d needs a train-mode BatchNorm", a.groups);
  GI_REQUIRE(a.pixels % groups == 0, "act_bn_bwd: %lld pixels in %d groups", (long long)a.pixels, groups);
  p.pg = a.pixels / groups;
  p.invM = 1.f / (float)p.pg;
  int blocks = 0;   // per population
  p.rows_per_block = rows_per_block_for(p.pg, &blocks);
  const int grid2 = nblocks(a.pixels * Q, 4);
  auto apply_rows = [&] {   // the generic apply kernel on the coefficient rows of bwd_sums_kernel
    gi_with_dtype(dtype, [&](auto tag) { gi_with_bool(groups == 2, [&](auto G2c) {
      hipLaunchKernelGGL((act_bn_bwd_apply_kernel<typename decltype(tag)::type, 1, decltype(G2c)::value>), dim3(grid2), dim3(256), 0, st, p);
    }); });
  };
  int small_max = gi_opt(GI_OPT_BN_BWD_SMALL);   // GI_BN_BWD_SMALL: largest pixel count served by the one-launch kernel (0: off)
  if (small_max > 2048) small_max = 2048;
  if (a.has_bn && !a.eval_bn && groups == 1 && a.pixels <= small_max && !a.reduce_done) {
    p.zero_next = a.acc ? a.zero_next : nullptr; p.zero_words = a.acc ? a.zero_words : 0;   // (keeps the accumulator ping-pong of net.hip consistent)
    gi_with_dtype(dtype, [&](auto tag) { gi_with_int<1, 2, 4, 8>((int)((a.pixels + 255) / 256), [&](auto NITc) {
      hipLaunchKernelGGL((act_bn_bwd_small_kernel<typename decltype(tag)::type, decltype(NITc)::value>), dim3(Q), dim3(256), 0, st, p);
    }); });
  } else if (a.has_bn && a.acc) {
    // exact accumulators: reduce pass (train mode only) + apply pass, no sums launch in between
    // (at most 1024 workgroups: with 214 - 250 VGPRs two are resident per CU, and every round of workgroups reads the accumulators and
    //  derives its coefficients again - the critic's conv2-level pass 38.5 -> 34.5 us; fewer, fatter workgroups on the smaller passes
    //  measured slower)
    int grid3 = nblocks(a.pixels * Q, gi_tune("GI_BWD_APPLY_CPT", 8));
    if (grid3 > 1024) grid3 = 1024;
    const size_t lds = (size_t)groups * 5 * a.c * sizeof(float);
    if (!a.eval_bn) {
      GI_REQUIRE(groups == 1 || p.pg % p.rows_per_block == 0, "act_bn_bwd: %lld pixels per group not a multiple of %d rows",
                 (long long)p.pg, p.rows_per_block);
      p.acc = a.acc;
      if (!a.reduce_done) {
        GI_TRY(launch_bwd_reduce(st, dtype, p, blocks * groups));
      }
      p.zero_next = a.zero_next; p.zero_words = a.zero_words;
    } else {
      p.dgamma = nullptr; p.dbeta = nullptr;
    }
    const bool need_y = a.g2 != nullptr || a.act != GI_ACT_NONE;
    gi_with_dtype(dtype, [&](auto tag) { gi_with_int<1, 2, 3>((a.g1 ? 1 : 0) | (a.g2 ? 2 : 0), [&](auto INc) { gi_with_bool(need_y && !p.scale, [&](auto LYc) { gi_with_bool(groups == 2, [&](auto G2c) {
      using T = typename decltype(tag)::type;
      constexpr int IN = decltype(INc)::value;
      constexpr bool LY = decltype(LYc)::value, G2 = decltype(G2c)::value;
      if constexpr (apply_acc_built(IN, LY, G2)) hipLaunchKernelGGL((act_bn_bwd_apply_acc_kernel<T, IN, LY, G2>), dim3(grid3), dim3(256), lds, st, p);
      else hipLaunchKernelGGL((act_bn_bwd_apply_kernel<T, 2, G2>), dim3(grid3), dim3(256), lds, st, p);
    }); }); }); });
  } else if (a.has_bn && a.eval_bn) {
    // running-statistics BatchNorm is a per-channel affine map: the batch-mean terms vanish (sums = 0)
    hipLaunchKernelGGL(bwd_sums_kernel, dim3(a.c), dim3(256), 0, st, a.partials, 0, a.c, a.sums, (float*)nullptr, (float*)nullptr, 0.f, 1,
                       a.gamma, a.save_mean, a.save_invstd, p.scale, p.shift, 0, 0.f);
    GI_LAUNCH_CHECK();
    apply_rows();
  } else if (a.has_bn) {
    GI_REQUIRE(groups == 1 || p.pg % p.rows_per_block == 0, "act_bn_bwd: %lld pixels per group not a multiple of %d rows",
               (long long)p.pg, p.rows_per_block);
    GI_TRY(launch_bwd_reduce(st, dtype, p, blocks * groups));
    hipLaunchKernelGGL(bwd_sums_kernel, dim3(a.c), dim3(256), 0, st, a.partials, blocks, a.c, a.sums, a.dgamma, a.dbeta, a.inv_loss_scale,
                       groups, a.gamma, a.save_mean, a.save_invstd, p.scale, p.shift, a.stat_stride, p.invM);
    GI_LAUNCH_CHECK();
    apply_rows();
  } else {
    gi_with_dtype(dtype, [&](auto tag) {
      hipLaunchKernelGGL((act_bn_bwd_apply_kernel<typename decltype(tag)::type, 0, false>), dim3(grid2), dim3(256), 0, st, p);
    });
  }
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_in_forward(hipStream_t st, int dtype, const void* x, void* y, int n, int hw, int c, int ldy, int coffy, int act,
                  const uint8_t* drop_mask, float drop_scale, float eps, float* stats) {
  const int epc = dtype == GI_F16 ? 8 : 4;
  GI_REQUIRE(c % epc == 0 && n >= 1 && hw >= 1, "in_forward: n=%d hw=%d c=%d", n, hw, c);
  const dim3 grid((unsigned)n * (c / epc));
  gi_with_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(in_forward_kernel<typename decltype(tag)::type>, grid, dim3(256), 0, st, (const char*)x, (char*)y, hw, c, ldy, coffy, act,
                       drop_mask, drop_scale, eps, stats);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_act_in_bwd(hipStream_t st, int dtype, const ActBnBwdArgs& a, int n, int hw, const float* stats) {
  const int epc = dtype == GI_F16 ? 8 : 4;
  GI_REQUIRE(a.c % epc == 0 && (int64_t)n * hw == a.pixels && a.x && stats, "act_in_bwd: n=%d hw=%d pixels=%lld c=%d", n, hw, (long long)a.pixels, a.c);
  const BwdP p = fill_bwd(a);
  const dim3 grid((unsigned)n * (a.c / epc));
  gi_with_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(act_in_bwd_kernel<typename decltype(tag)::type>, grid, dim3(256), 0, st, p, hw, stats);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_bias_grad(hipStream_t st, int dtype, const void* dz, int64_t pixels, int c, float scale, float* dbias, float* partials) {
  int rows = 0;
  GI_TRY(op_col_stats(st, dtype, dz, pixels, c, partials, &rows));
  hipLaunchKernelGGL(bias_grad_kernel, dim3(c), dim3(256), 0, st, partials, rows, c, scale, dbias);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_bn_tangent_inject(hipStream_t st, int dtype, const void* dta, const void* y, const void* tx, const void* x, void* dxp,
                         int64_t pixels, int c, const float* gamma, const float* mean, const float* inv, float* dgamma,
                         float dgamma_scale, float* partials, float* sums) {
  GI_REQUIRE(chunks_ok(dtype, c), "bn_tangent_inject: c=%d unsupported", c);
  InjP p;
  p.dta = (const char*)dta; p.y = (const char*)y; p.tx = (const char*)tx; p.x = (const char*)x; p.dxp = (char*)dxp;
  p.pixels = pixels; p.c = c; p.gamma = gamma; p.mean = mean; p.inv = inv; p.partials = partials; p.sums = sums; p.dgamma = dgamma;
  p.dgamma_scale = dgamma_scale;
  int blocks = 0;
  p.rows_per_block = rows_per_block_for(pixels, &blocks);
  gi_with_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(bn_inject_reduce_kernel<typename decltype(tag)::type>, dim3(blocks), dim3(256), 0, st, p);
  });
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_inject_sums_kernel, dim3(c), dim3(256), 0, st, partials, blocks, c, sums);
  GI_LAUNCH_CHECK();
  const int grid2 = nblocks(pixels * (c / (dtype == GI_F16 ? 8 : 4)), 2);
  gi_with_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(bn_inject_apply_kernel<typename decltype(tag)::type>, dim3(grid2), dim3(256), 0, st, p);
  });
  GI_LAUNCH_CHECK();
  return GI_OK;
}
