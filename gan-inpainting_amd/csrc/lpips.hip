// LPIPS (Zhang et al. 2018, `lpips` v0.1, net = 'vgg') between two batches of grey images: the learned perceptual distance the
// inpainting papers report next to FID. The evaluation pass uses the forward alone; the opt-in backward w.r.t. `a` (second
// half of this file) needs a second workspace, and a handle that never binds it runs launch for launch as without it.
//
// `a` and `b` run as ONE stacked batch of 2n images (NHWC fp16), as in vgg.hip; what the two networks' trunks share (weight packing,
// read-backs, and the backward's scale, activation backward, first-layer adjoint, workspace arenas and chain) is vggtrunk.hip's:
//   conv1_1  the network's input is alpha_c x + beta_c per channel (the scaling layer after normalize=True) of the grey image repeated
//            over 3 channels, ZERO-PADDED AFTER the scaling: the beta term is a bias that is missing where a tap falls outside the image,
//            so it differs on the one-pixel border ring (nine position classes) and cannot go into the layer's bias. The layer is a
//            two-plane convolution over (x, inside-indicator) with wA[o][tap] = sum_c w alpha_c, wB[o][tap] = sum_c w beta_c
//            (lpips_fold_kernel, at sync_weights), each weight as an fp16 head + remainder: two v_mfma_f32_16x16x32_f16 per tile;
//   12 more  3x3/s1/p1 convolutions + bias + ReLU: op_igemm mode 2 (fp16 MFMA implicit GEMM);
//   taps     relu1_2, relu2_2, relu3_3, relu4_3, relu5_3, each before its max pool. lpips_tap_kernel: per pixel the two channel norms,
//            then sum_c lin_c (fa / (|fa| + 1e-10) - fb / (|fb| + 1e-10))^2 in fp32, per-image fp64 partials in a fixed order, and - for
//            the four taps a pool follows - the 2x2 max pool of both halves from the registers it holds anyway (one read of the largest
//            maps instead of two). No atomics: an image's value has the same bits wherever it sits in the batch and whatever n is.
#include <new>

#include "vggtrunk.h"

namespace {

constexpr int NCONV = 13, NTAP = 5;
const int kCin[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kCout[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kFeatIdx[NCONV] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};   // torchvision vgg16.features indices
const int kTapAfter[NCONV] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};
const int kPoolAfter[NCONV] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0};          // a 2x2 max pool follows every tap but the last
const int kTapC[NTAP] = {64, 128, 256, 512, 512};
constexpr int LP_MAXNB = 128;      // workgroups (= fp64 partials) per image and tap, at most

// wA[o][tap] = sum_c w[o][c][tap] * alpha_c, wB[o][tap] = sum_c w[o][c][tap] * beta_c with alpha_c = 2 / scale_c and
// beta_c = (-1 - shift_c) / scale_c: (2 x - 1 - shift_c) / scale_c = alpha_c x + beta_c. fp32, c ascending, one fma per term.
__global__ void __launch_bounds__(256) lpips_fold_kernel(const float* __restrict__ w, const float* __restrict__ shift, const float* __restrict__ scale,
                                                         float* __restrict__ wA, float* __restrict__ wB) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 64 * 9) return;
  const int o = i / 9, t = i % 9;
  float sa = 0.f, sb = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float wv = w[(o * 3 + c) * 9 + t];
    sa = fmaf(wv, 2.f / scale[c], sa);
    sb = fmaf(wv, (-1.f - shift[c]) / scale[c], sb);
  }
  wA[i] = sa;
  wB[i] = sb;
}

// out[img,y,x,0:64] = relu(b + sum_tap wA[.][tap] x[img, y-1+ky, x-1+kx] + sum_tap wB[.][tap] [the tap lies inside the image]);
// images [0,n) from xa, [n,2n) from xb. On the matrix cores as vgg_conv1_mfma_kernel: D[channel][pixel] = A[channel][k] B[k][pixel], two
// v_mfma_f32_16x16x32_f16 per tile (fp32 accumulate): the image plane, then the indicator plane. Both planes share the tap geometry:
// k = 0..8 multiplies the fp16 head of the folded weight, k = 9..17 its fp16 remainder (w = hi + lo to about 22 bits: a single fp16 of
// the folded weights costs 2^-11 of sums that cancel, several times what rounding the three channels' weights costs), k = 18..31 zero.
// The image is rounded to fp16, the indicator is exact. A wave owns 16 consecutive pixels of an image row; lane (pixel, kq) holds
// k = 8 kq .. 8 kq + 7 (selects, no divergent branches; the group index is wave-uniform). Channel order per tile as in
// vgg_conv1_mfma_kernel: two 16-byte stores per lane, 64 contiguous bytes per pixel and instruction.
__global__ void __launch_bounds__(256) lpips_conv1_mfma_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int n, int H, int W,
                                                               const float* __restrict__ wA, const float* __restrict__ wB,
                                                               const float* __restrict__ bias, half_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, kq = lane >> 4;
  h8_t af[2][4];                                            // [image plane, indicator plane][tile]
  float br[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int ch = ((mt >> 1) & 1) * 32 + (lr >> 2) * 8 + (mt & 1) * 4 + (lr & 3);     // A row lr of tile mt
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * kq + j, t = k < 9 ? k : k - 9;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const float w = k < 18 ? (pl ? wB : wA)[ch * 9 + t] : 0.f;
        const half_t hi = (half_t)w;
        af[pl][mt][j] = k < 9 ? hi : (half_t)(w - (float)hi);
      }
    }
    // D row i = 4 kq + r of tile mt is channel ((mt >> 1) & 1) * 32 + kq * 8 + (mt & 1) * 4 + r
#pragma unroll
    for (int r = 0; r < 4; ++r) br[mt][r] = bias[((mt >> 1) & 1) * 32 + kq * 8 + (mt & 1) * 4 + r];
  }
  const int gpr = W >> 4;                                   // 16-pixel groups per image row
  const int ngroups = 2 * n * H * gpr;                      // < 2^31 (host check)
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256 + threadIdx.x) >> 6));
  const int nwaves = (int)gridDim.x * 4;
  int dy[8], dx[8];                                         // this lane's taps: (ky, kx) - 1, or far outside for the padding of K
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * kq + j, t = k < 9 ? k : k - 9;
    dy[j] = k < 18 ? t / 3 - 1 : -(1 << 20);
    dx[j] = k < 18 ? t % 3 - 1 : 0;
  }
  // bv: the image at this lane's taps (0 outside the image); inside: bit j = [tap j lies inside], the indicator plane
  auto load_b = [&](int g, float (&bv)[8], unsigned& inside) {
    const int rowi = g / gpr;                               // wave-uniform
    const int x = (g - rowi * gpr) * 16 + lr;
    const int img = rowi / H, y = rowi - img * H;
    const float* src = img < n ? xa + (int64_t)img * H * W : xb + (int64_t)(img - n) * H * W;
    inside = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int iy = y + dy[j], ix = x + dx[j];
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = src[ok ? iy * W + ix : 0];
      bv[j] = ok ? v : 0.f;
      inside |= ok ? 1u << j : 0u;
    }
  };
  float bv[8], bn[8];
  unsigned iv = 0u, in = 0u;
  int g = wave;
  if (g < ngroups) load_b(g, bv, iv);
  for (; g < ngroups; g += nwaves) {
    if (g + nwaves < ngroups) load_b(g + nwaves, bn, in);
    h8_t bx, bi;
#pragma unroll
    for (int j = 0; j < 8; ++j) { bx[j] = (half_t)bv[j]; bi[j] = (iv >> j) & 1u ? (half_t)1.f : (half_t)0.f; }
    h8_t o[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f4_t acc = {br[mt][0], br[mt][1], br[mt][2], br[mt][3]};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][mt], bx, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][mt], bi, acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[mt >> 1][(mt & 1) * 4 + r] = (half_t)fmaxf(acc[r], 0.f);
    }
    half_t* dst = out + ((int64_t)g * 16 + lr) * 64;
    *(h8_t*)(dst + kq * 8) = o[0];
    *(h8_t*)(dst + 32 + kq * 8) = o[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = bn[j];
    iv = in;
  }
}

// The two products are rounded before they are subtracted (no fused multiply-add): with bit-equal inputs both sides are the same
// number and the difference is exactly zero.
__device__ __forceinline__ float lp_unit_diff(float fa, float ia, float fb, float ib) {
#pragma clang fp contract(off)
  const float pa = fa * ia, pb = fb * ib;
  return pa - pb;
}
// One pixel of one image pair, spread over the LPP = C / 8 lanes of a group (8 channels per lane): sum_c w_c (fa_c / (|fa| + 1e-10) -
// fb_c / (|fb| + 1e-10))^2 in fp32. The sums over the group's lanes are butterflies: every lane of the group ends with the same bits.
// A zero vector normalises to zeros (0 * 1e10), never to NaN.
template <int LPP>
__device__ __forceinline__ float lp_pixel(const h8_t a, const h8_t b, const float (&w)[8]) {
  float fa[8], fb[8], sa = 0.f, sb = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    fa[e] = (float)a[e];
    fb[e] = (float)b[e];
    sa = fmaf(fa[e], fa[e], sa);
    sb = fmaf(fb[e], fb[e], sb);
  }
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
  const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float d = lp_unit_diff(fa[e], ia, fb[e], ib);
    s = fmaf(w[e] * d, d, s);
  }
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// One tap of n image pairs: F [2n][H][W][C] fp16 (image i pairs with image i + n), C = 8 LPP. Workgroup (x, i) owns the units x UPB + group,
// + gridDim.x UPB, ... of pair i (a unit: one pixel, or with POOL one 2x2 window, whose max pool of BOTH images goes to pool
// [2n][H/2][W/2][C] - the same maximum, bit for bit, as a separate pooling pass). Each group adds its pixels' fp32 values to an fp64 sum in
// that order; the groups are added in a fixed order into partial[i][x]. The grid's x extent depends on (H, W, C) alone, so an image's
// partials do not depend on n or on its place in the batch.
struct LpTapP {
  const half_t* F; half_t* pool; const float* lin; double* partial;
  int n, H, W;
};
template <int LPP, bool POOL>
__global__ void __launch_bounds__(256) lpips_tap_kernel(LpTapP p) {
  constexpr int C = LPP * 8, UPB = 256 / LPP;
  __shared__ double sh[4];
  const int img = blockIdx.y;
  const int sub = threadIdx.x % LPP, grp = threadIdx.x / LPP;
  const int64_t HWC = (int64_t)p.H * p.W * C;
  const half_t* Fa = p.F + (int64_t)img * HWC + sub * 8;
  const half_t* Fb = p.F + (int64_t)(img + p.n) * HWC + sub * 8;
  float w[8];
  {
    const f4_t w0 = *(const f4_t*)(p.lin + sub * 8), w1 = *(const f4_t*)(p.lin + sub * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { w[e] = w0[e]; w[4 + e] = w1[e]; }
  }
  double acc = 0.0;
  if constexpr (POOL) {
    const int Wo = p.W / 2, units = (p.H / 2) * Wo;
    half_t* Pa = p.pool + (int64_t)img * units * C + sub * 8;
    half_t* Pb = p.pool + (int64_t)(img + p.n) * units * C + sub * 8;
    for (int u = blockIdx.x * UPB + grp; u < units; u += gridDim.x * UPB) {
      const int y = u / Wo, x = u - y * Wo;
      const int64_t o00 = ((int64_t)(2 * y) * p.W + 2 * x) * C;
      const int64_t off[4] = {o00, o00 + C, o00 + (int64_t)p.W * C, o00 + (int64_t)p.W * C + C};
      h8_t a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[q] = *(const h8_t*)(Fa + off[q]); b[q] = *(const h8_t*)(Fb + off[q]); }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc += (double)lp_pixel<LPP>(a[q], b[q], w);
      *(h8_t*)(Pa + (int64_t)u * C) = __builtin_elementwise_max(__builtin_elementwise_max(a[0], a[1]), __builtin_elementwise_max(a[2], a[3]));
      *(h8_t*)(Pb + (int64_t)u * C) = __builtin_elementwise_max(__builtin_elementwise_max(b[0], b[1]), __builtin_elementwise_max(b[2], b[3]));
    }
  } else {
    const int units = p.H * p.W;
    for (int u = blockIdx.x * UPB + grp; u < units; u += gridDim.x * UPB) {
      const h8_t a = *(const h8_t*)(Fa + (int64_t)u * C), b = *(const h8_t*)(Fb + (int64_t)u * C);
      acc += (double)lp_pixel<LPP>(a, b, w);
    }
  }
  double v = sub == 0 ? acc : 0.0;     // every lane of a group holds the group's sum: count it once
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[(int64_t)img * LP_MAXNB + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// Workgroup i: d_l[i] = inv[l] * (the nb[l] partials of pair i and tap l, added in a fixed order), rounded to fp32; out_n[i] = their sum
// (fp64, l ascending, rounded once). per_layer[l * n + i] = d_l[i] when given.
struct LpFinP { int nb[NTAP]; double inv[NTAP]; int ntap, n, pair_stride; };
__global__ void __launch_bounds__(256) lpips_finish_kernel(const double* __restrict__ partial, LpFinP f, float* __restrict__ out_n,
                                                           float* __restrict__ per_layer) {
  __shared__ double sh[4];
  const int i = blockIdx.x;
  double tot = 0.0;
  for (int l = 0; l < f.ntap; ++l) {
    const double* pp = partial + ((int64_t)l * f.pair_stride + i) * LP_MAXNB;
    double s = (int)threadIdx.x < f.nb[l] ? pp[threadIdx.x] : 0.0;          // nb <= LP_MAXNB <= 256
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    const float d = (float)(((sh[0] + sh[1]) + (sh[2] + sh[3])) * f.inv[l]);
    if (per_layer && threadIdx.x == 0) per_layer[(int64_t)l * f.n + i] = d;
    tot += (double)d;
  }
  if (out_n && threadIdx.x == 0) out_n[i] = (float)tot;
}

// ================================================================================================================================
// Opt-in backward: gscale * d d[i] / d a[i], b constant. As vgg.hip's the chain runs on s * gradient in fp16
// with fp32 accumulation, but with ONE power of two s_i PER IMAGE: d[i] depends on a[i] alone and every kernel of the chain is linear
// per image, so a nearly identical pair does not underflow next to a very different one and an image's bits do not depend on its
// chunk-mates. No float atomics: the only atomic is an unsigned max over bit patterns of non-negative floats (order-independent).
// ================================================================================================================================

// Seed of one pixel: the gradient of d_l w.r.t. the post-ReLU vector a (b constant), in the tap kernel's lane layout. With ra = |a|,
// ia = 1 / (ra + 1e-10), a^ = a ia, delta = a^ - b^ (the forward's rounded products: equal inputs give delta = 0 exactly) and
// q = sum_c w_c delta_c a^_c:   seed_k = c2 ia (w_k delta_k - q a_k / ra),  c2 = 2 / HW;   ra == 0: seed = 0 (autograd gives NaN there,
// but a post-ReLU vector is zero only where the ReLU mask below removes every channel anyway).
template <int LPP>
__device__ __forceinline__ void lp_seed_pixel(const h8_t a, const h8_t b, const float (&w)[8], float c2, float (&seed)[8]) {
  float fa[8], fb[8], sa = 0.f, sb = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    fa[e] = (float)a[e];
    fb[e] = (float)b[e];
    sa = fmaf(fa[e], fa[e], sa);
    sb = fmaf(fb[e], fb[e], sb);
  }
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
  const float ra = sqrtf(sa);
  const float ia = 1.f / (ra + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
  float pa[8], wd[8], q = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    pa[e] = fa[e] * ia;
    wd[e] = w[e] * lp_unit_diff(fa[e], ia, fb[e], ib);
    q = fmaf(wd[e], pa[e], q);
  }
#pragma unroll
  for (int off = LPP / 2; off > 0; off >>= 1) q += __shfl_xor(q, off);
  const bool live = ra > 0.f;
  const float ir = live ? 1.f / ra : 0.f, k = live ? c2 * ia : 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) seed[e] = k * (wd[e] - q * (fa[e] * ir));
}

// One tap of n pairs, F as for lpips_tap_kernel, workgroup (x, i) over the pixels of pair i.
//   STORE = false: smax[i] = max(smax[i], max |seed|) as a bit pattern (bit patterns of non-negative floats order like the floats);
//   STORE = true:  sc[i] * seed in fp16 OVER the b half of the map: a lane overwrites the eight elements of b it has just read, and
//                  nothing else reads that half after the forward.
struct LpSeedP {
  half_t* F; const float* lin; unsigned* smax; const float* sc;
  int n, HW; float c2;
};
template <int LPP, bool STORE>
__global__ void __launch_bounds__(256) lpips_seed_kernel(LpSeedP p) {
  constexpr int C = LPP * 8, UPB = 256 / LPP;
  __shared__ float red[4];
  const int img = blockIdx.y;
  const int sub = threadIdx.x % LPP, grp = threadIdx.x / LPP;
  const half_t* Fa = p.F + (int64_t)img * p.HW * C + sub * 8;
  half_t* Fb = p.F + (int64_t)(img + p.n) * p.HW * C + sub * 8;
  float w[8];
  {
    const f4_t w0 = *(const f4_t*)(p.lin + sub * 8), w1 = *(const f4_t*)(p.lin + sub * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { w[e] = w0[e]; w[4 + e] = w1[e]; }
  }
  const float s = STORE ? p.sc[img] : 1.f;
  float m = 0.f;
  // every lane of a group takes part in the butterflies: the loop bound is the same for all lanes of a group
  for (int u = blockIdx.x * UPB + grp; u < p.HW; u += gridDim.x * UPB) {
    const h8_t a = *(const h8_t*)(Fa + (int64_t)u * C), b = *(const h8_t*)(Fb + (int64_t)u * C);
    float seed[8];
    lp_seed_pixel<LPP>(a, b, w, p.c2, seed);
    if constexpr (STORE) {
      h8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)(seed[e] * s);
      *(h8_t*)(Fb + (int64_t)u * C) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(seed[e]));
    }
  }
  if constexpr (!STORE) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      if (m > 0.f) atomicMax(p.smax + img, __float_as_uint(m));
    }
  }
}

// ---- host launch code: one copy of every grid rule, shared by the runner and the gi_debug_lpips_* entries -----------------------------

int lp_fold(hipStream_t st, const float* w, const float* shift, const float* scale, float* wA, float* wB) {
  hipLaunchKernelGGL(lpips_fold_kernel, dim3(3), dim3(256), 0, st, w, shift, scale, wA, wB);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
// (W % 16 == 0 and 2 n H W 64 < 2^31 are conditions of the callers)
int lp_conv1(hipStream_t st, const float* xa, const float* xb, int n, int H, int W, const float* wA, const float* wB, const float* bias, half_t* out) {
  hipLaunchKernelGGL(lpips_conv1_mfma_kernel, dim3(grid_for((int64_t)2 * n * H * (W / 16), 4, 256 * 8)), dim3(256), 0, st, xa, xb, n, H, W, wA, wB,
                     bias, out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
// workgroups per image of a tap: a function of the map alone
int lp_tap_blocks(int H, int W, int C, bool pool) {
  const int units = pool ? (H / 2) * (W / 2) : H * W, upb = 256 / (C / 8);
  return grid_for(units, upb, LP_MAXNB);
}
// one tap of n pairs: partial[i][0 .. lp_tap_blocks) and, with pool, the pooled map of all 2n images
int lp_tap(hipStream_t st, const half_t* F, int n, int H, int W, int C, const float* lin, half_t* pool, double* partial) {
  LpTapP p;
  p.F = F; p.pool = pool; p.lin = lin; p.partial = partial; p.n = n; p.H = H; p.W = W;
  const dim3 grid(lp_tap_blocks(H, W, C, pool != nullptr), n);
#define LP_TAP_CASE(LPP)                                                                             \
  case LPP * 8:                                                                                      \
    if (pool) hipLaunchKernelGGL((lpips_tap_kernel<LPP, true>), grid, dim3(256), 0, st, p);          \
    else hipLaunchKernelGGL((lpips_tap_kernel<LPP, false>), grid, dim3(256), 0, st, p);              \
    break;
  switch (C) {
    LP_TAP_CASE(8)
    LP_TAP_CASE(16)
    LP_TAP_CASE(32)
    LP_TAP_CASE(64)
    default: gi_set_error("lpips tap: C=%d (64, 128, 256 or 512)", C); return GI_ERR_INVALID;
  }
#undef LP_TAP_CASE
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int lp_finish(hipStream_t st, const double* partial, const LpFinP& f, float* out_n, float* per_layer) {
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(f.n), dim3(256), 0, st, partial, f, out_n, per_layer);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// ---- the backward's launch code ------------------------------------------------------------------------------------------------------
// one pass of a tap's seed over n pairs (F [2n][HW][C]): store = false: smax[i] = max |seed| of pair i; store = true: sc[i] * seed over the b half
int lp_seed(hipStream_t st, bool store, half_t* F, int n, int64_t HW, int C, const float* lin, unsigned* smax, const float* sc) {
  LpSeedP p;
  p.F = F; p.lin = lin; p.smax = smax; p.sc = sc; p.n = n; p.HW = (int)HW; p.c2 = (float)(2.0 / (double)HW);
  const dim3 grid(grid_for(HW, 256 / (C / 8), LP_MAXNB), n);
#define LP_SEED_CASE(LPP)                                                                            \
  case LPP * 8:                                                                                      \
    if (store) hipLaunchKernelGGL((lpips_seed_kernel<LPP, true>), grid, dim3(256), 0, st, p);        \
    else hipLaunchKernelGGL((lpips_seed_kernel<LPP, false>), grid, dim3(256), 0, st, p);             \
    break;
  switch (C) {
    LP_SEED_CASE(8)
    LP_SEED_CASE(16)
    LP_SEED_CASE(32)
    LP_SEED_CASE(64)
    default: gi_set_error("lpips seed: C=%d (64, 128, 256 or 512)", C); return GI_ERR_INVALID;
  }
#undef LP_SEED_CASE
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // namespace

struct gi_lpips {
  gi_ctx* ctx;
  VggTrunk t;             // H, W, max_pairs; w1: conv1_1 folded weights [64][9], image plane (wA); the rest only with the grad workspace
  int64_t woff[NCONV], boff[NCONV], linoff[NTAP], shiftoff, scaleoff;   // float offsets into params
  int64_t param_floats;
  const float* params;
  char* ws;
  int64_t ws_bytes;
  half_t* act[2];
  half_t* wpk[NCONV];     // [1..12] packed fp16 weights
  float* wB;              // conv1_1 folded weights [64][9]: indicator plane
  double* partial;        // [5 taps][max_pairs][LP_MAXNB]
  bool bound, synced;
  // opt-in backward (gi_lpips_bind_grad): a separate workspace; a handle that never binds it runs exactly as before
  char* gws;
  int64_t gws_bytes;
  bool gbound;
  int grad_n;             // pairs of the last grad call (0: none yet): gi_lpips_grad_tap replays its backward
  unsigned* smax;         // [max_pairs] largest |seed| of an image over the five taps (bit patterns of non-negative floats)
  float* sc;              // [i] = s_i = 2^k, [n + i] = 1 / s_i (t.inv, stride 1): image i's backward runs on s_i * gradient
};

namespace {

int64_t lpips_ws_layout(gi_lpips* v, char* base) {
  WsTake take{base, 0};
  const int64_t act_bytes = (int64_t)2 * v->t.max_pairs * v->t.H * v->t.W * 64 * 2;      // the widest maps: relu1_1 / relu1_2
  v->act[0] = (half_t*)take(act_bytes);
  v->act[1] = (half_t*)take(act_bytes);
  v->wpk[0] = nullptr;
  for (int i = 1; i < NCONV; ++i) v->wpk[i] = (half_t*)take((int64_t)kCout[i] * 9 * kCin[i] * 2);
  v->t.w1 = (float*)take(64 * 9 * 4);
  v->wB = (float*)take(64 * 9 * 4);
  v->partial = (double*)take((int64_t)NTAP * v->t.max_pairs * LP_MAXNB * 8);
  return take.off;
}

// grad workspace: the trunk's arenas, transposed weights and gradient buffers (the [a half | b half] maps of trunk_gws_layout), then the
// per-image seed maxima and scales
int64_t lpips_gws_layout(gi_lpips* v, char* base) {
  WsTake take{base, 0};
  trunk_gws_layout(v->t, take);
  v->smax = (unsigned*)take((int64_t)v->t.max_pairs * 4);
  v->sc = (float*)take((int64_t)2 * v->t.max_pairs * 4);
  return take.off;
}

// the network on 2n stacked images; the taps leave their partials behind (fin: their counts). feat_out: stop at tap stop_tap and return
// its map of the first n images as NCHW fp32. grad: the same launches, but every stage writes its own map in the grad workspace (nothing
// the backward reads is overwritten)
int lpips_run(gi_lpips* v, const float* xa, const float* xb, int n, int stop_tap, float* feat_out, LpFinP& fin, bool grad = false) {
  hipStream_t st = v->ctx->stream;
  const int nimg = 2 * n;
  int H = v->t.H, W = v->t.W, cur = 0;
  half_t* curp = grad ? v->t.ga[0] : v->act[0];
  // (W % 16 == 0 and 2 n H W 64 < 2^31 are conditions of gi_lpips_create)
  GI_TRY(lp_conv1(st, xa, xb, n, H, W, v->t.w1, v->wB, v->params + v->boff[0], curp));
  for (int i = 1; i < NCONV; ++i) {
    half_t* outp = grad ? v->t.ga[i] : v->act[cur ^ 1];
    IgemmArgs a;
    const int rc = conv3x3(st, curp, v->wpk[i], outp, nimg, H, W, kCin[i], kCout[i], v->params + v->boff[i], GI_ACT_RELU, 0, nullptr, nullptr, a);
    if (rc == GI_ERR_UNSUPPORTED) gi_set_error("lpips: no mode-2 kernel serves n=%d %dx%d %d->%d", nimg, H, W, kCin[i], kCout[i]);
    GI_TRY(rc);
    cur ^= 1;
    curp = outp;
    const int tap = kTapAfter[i], C = kCout[i];
    if (tap < 0) continue;
    if (feat_out && tap == stop_tap) return nhwc_to_nchw(st, curp, feat_out, n, H * W, C);
    const bool pool = kPoolAfter[i] != 0;
    half_t* poolp = pool ? (grad ? v->t.gpool[i] : v->act[cur ^ 1]) : nullptr;
    double* partial = v->partial + (int64_t)tap * v->t.max_pairs * LP_MAXNB;
    fin.inv[tap] = 1.0 / ((double)H * W);
    fin.nb[tap] = lp_tap_blocks(H, W, C, pool);
    GI_TRY(lp_tap(st, curp, n, H, W, C, v->params + v->linoff[tap], poolp, partial));
    if (pool) { cur ^= 1; curp = poolp; H /= 2; W /= 2; }
  }
  return GI_OK;
}

// seeds of the five taps from the maps the grad forward left: every image's maximum, then its s_i, then s_i * seed over the b halves
int lpips_seeds(gi_lpips* v, int n) {
  hipStream_t st = v->ctx->stream;
  for (int pass = 0; pass < 2; ++pass) {
    int H = v->t.H, W = v->t.W;
    for (int i = 0; i < NCONV; ++i) {
      const int tap = kTapAfter[i];
      if (tap >= 0) GI_TRY(lp_seed(st, pass == 1, v->t.ga[i], n, (int64_t)H * W, kCout[i], v->params + v->linoff[tap], v->smax, v->sc));
      if (kPoolAfter[i]) { H /= 2; W /= 2; }
    }
    if (pass == 0) GI_TRY(seed_scale(st, v->smax, v->sc, n));
  }
  return GI_OK;
}

// The chain from conv5_3 down (trunk_backward) on s_i * gradient; every tap below the top is a pooled layer, so its seed joins in the
// un-pool. stop_tap < 0: down to the first-layer adjoint into grad_out. stop_tap = t: the gradient w.r.t. the post-ReLU map of tap t goes
// to tap_out as NCHW fp32, de-scaled.
int lpips_backward(gi_lpips* v, int n, int stop_tap, float* tap_out, float* grad_out, float gscale) {
  int stop = -1;
  for (int i = 0; i < NCONV; ++i)
    if (kTapAfter[i] >= 0 && kTapAfter[i] == stop_tap) stop = i;
  v->t.inv = v->sc + n;
  v->t.inv_stride = 1;
  return trunk_backward(v->t, v->ctx->stream, n, stop, tap_out, grad_out, gscale);
}

}  // namespace

extern "C" {

int gi_lpips_create(gi_ctx* ctx, int H, int W, int max_pairs, gi_lpips** out) {
  GI_REQUIRE(ctx && out, "lpips_create: null argument");
  GI_REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && max_pairs > 0, "lpips_create: H=%d W=%d (multiples of 16) pairs=%d", H, W, max_pairs);
  GI_REQUIRE((int64_t)2 * max_pairs * H * W * 64 < (1ll << 31), "lpips_create: 2*%d images of %dx%d exceed 32-bit activation offsets", max_pairs, H, W);
  gi_lpips* v = new (std::nothrow) gi_lpips();
  GI_REQUIRE(v, "lpips_create: out of host memory");
  v->ctx = ctx;
  v->t.nconv = NCONV; v->t.cin = kCin; v->t.cout = kCout; v->t.tap_after = kTapAfter; v->t.pool_after = kPoolAfter;
  v->t.H = H; v->t.W = W; v->t.max_pairs = max_pairs;
  int64_t off = 0;
  for (int i = 0; i < NCONV; ++i) {
    v->woff[i] = off; off += (int64_t)kCout[i] * kCin[i] * 9;
    v->boff[i] = off; off += kCout[i];
  }
  for (int t = 0; t < NTAP; ++t) { v->linoff[t] = off; off += kTapC[t]; }
  v->shiftoff = off; off += 3;
  v->scaleoff = off; off += 3;
  v->param_floats = off;
  v->params = nullptr; v->ws = nullptr; v->bound = false; v->synced = false;
  v->ws_bytes = lpips_ws_layout(v, nullptr);
  v->gws = nullptr; v->gbound = false; v->grad_n = 0;
  v->gws_bytes = lpips_gws_layout(v, nullptr);
  *out = v;
  return GI_OK;
}
void gi_lpips_destroy(gi_lpips* v) { delete v; }
int64_t gi_lpips_param_floats(const gi_lpips* v) { return v ? v->param_floats : -1; }
int64_t gi_lpips_workspace_bytes(const gi_lpips* v) { return v ? v->ws_bytes : -1; }
int gi_lpips_num_tensors(const gi_lpips* v) { return v ? 2 * NCONV + NTAP + 2 : -1; }

int gi_lpips_tensor_desc(const gi_lpips* v, int index, char* name, int name_cap, int* shape4, int64_t* offset) {
  GI_REQUIRE(v && index >= 0 && index < 2 * NCONV + NTAP + 2 && name && shape4 && offset, "lpips_tensor_desc: bad argument");
  shape4[0] = shape4[1] = shape4[2] = shape4[3] = 0;
  if (index < 2 * NCONV) {
    const int i = index / 2, is_bias = index & 1;
    snprintf(name, name_cap, "features.%d.%s", kFeatIdx[i], is_bias ? "bias" : "weight");
    shape4[0] = kCout[i];
    if (is_bias) *offset = v->boff[i];
    else { shape4[1] = kCin[i]; shape4[2] = shape4[3] = 3; *offset = v->woff[i]; }
  } else if (index < 2 * NCONV + NTAP) {
    const int t = index - 2 * NCONV;
    snprintf(name, name_cap, "lin%d.model.1.weight", t);
    shape4[0] = 1; shape4[1] = kTapC[t]; shape4[2] = shape4[3] = 1;
    *offset = v->linoff[t];
  } else {
    const bool is_scale = index == 2 * NCONV + NTAP + 1;
    snprintf(name, name_cap, "scaling_layer.%s", is_scale ? "scale" : "shift");
    shape4[0] = 1; shape4[1] = 3; shape4[2] = shape4[3] = 1;
    *offset = is_scale ? v->scaleoff : v->shiftoff;
  }
  return GI_OK;
}

int gi_lpips_bind(gi_lpips* v, const float* params, void* ws, int64_t ws_bytes) {
  GI_REQUIRE(v && params && ws, "lpips_bind: null argument");
  GI_REQUIRE(ws_bytes >= v->ws_bytes && ((uintptr_t)ws & 255) == 0, "lpips_bind: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)v->ws_bytes);
  GI_REQUIRE(((uintptr_t)params & 15) == 0, "lpips_bind: params must be 16-byte aligned");
  v->params = params; v->ws = (char*)ws;
  lpips_ws_layout(v, v->ws);
  v->bound = true; v->synced = false;
  return GI_OK;
}

int gi_lpips_sync_weights(gi_lpips* v) {
  GI_REQUIRE(v && v->bound, "lpips_sync_weights: not bound");
  hipStream_t st = v->ctx->stream;
  GI_TRY(lp_fold(st, v->params + v->woff[0], v->params + v->shiftoff, v->params + v->scaleoff, v->t.w1, v->wB));
  for (int i = 1; i < NCONV; ++i) GI_TRY(pack3x3(st, false, v->params + v->woff[i], v->wpk[i], kCout[i], kCin[i]));
  if (v->gbound)
    for (int i = 1; i < NCONV; ++i) GI_TRY(pack3x3(st, true, v->params + v->woff[i], v->t.wT[i], kCout[i], kCin[i]));
  v->synced = true;
  return GI_OK;
}

int gi_lpips_distance(gi_lpips* v, const float* a, const float* b, int n, float* out_n, float* per_layer_5n) {
  GI_REQUIRE(v && v->bound && v->synced, "lpips_distance: bind + sync_weights first");
  GI_REQUIRE(a && b && out_n && n > 0 && n <= v->t.max_pairs, "lpips_distance: n=%d (max %d)", n, v->t.max_pairs);
  LpFinP fin = {};
  fin.ntap = NTAP; fin.n = n; fin.pair_stride = v->t.max_pairs;
  GI_TRY(lpips_run(v, a, b, n, -1, nullptr, fin));
  return lp_finish(v->ctx->stream, v->partial, fin, out_n, per_layer_5n);
}

int64_t gi_lpips_grad_workspace_bytes(const gi_lpips* v) { return v ? v->gws_bytes : -1; }

int gi_lpips_bind_grad(gi_lpips* v, void* ws, int64_t ws_bytes) {
  GI_REQUIRE(v && ws, "lpips_bind_grad: null argument");
  GI_REQUIRE(v->bound, "lpips_bind_grad: gi_lpips_bind first");
  GI_REQUIRE(ws_bytes >= v->gws_bytes && ((uintptr_t)ws & 255) == 0, "lpips_bind_grad: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)v->gws_bytes);
  v->gws = (char*)ws;
  lpips_gws_layout(v, v->gws);
  v->gbound = true; v->synced = false; v->grad_n = 0;      // sync_weights packs the transposed weights
  return GI_OK;
}

int gi_lpips_distance_grad(gi_lpips* v, const float* a, const float* b, int n, float* out_n, float* per_layer_5n, float* grad_a, float gscale) {
  GI_REQUIRE(v && v->gbound, "lpips_distance_grad: no grad workspace bound (gi_lpips_bind_grad)");
  GI_REQUIRE(v->bound && v->synced, "lpips_distance_grad: bind + sync_weights first");
  GI_REQUIRE(a && b && out_n && grad_a && n > 0 && n <= v->t.max_pairs, "lpips_distance_grad: n=%d (max %d)", n, v->t.max_pairs);
  hipStream_t st = v->ctx->stream;
  v->grad_n = 0;
  GI_HIP(hipMemsetAsync(v->smax, 0, (size_t)v->t.max_pairs * 4, st));
  LpFinP fin = {};
  fin.ntap = NTAP; fin.n = n; fin.pair_stride = v->t.max_pairs;
  GI_TRY(lpips_run(v, a, b, n, -1, nullptr, fin, true));
  GI_TRY(lp_finish(st, v->partial, fin, out_n, per_layer_5n));
  GI_TRY(lpips_seeds(v, n));
  v->grad_n = n;
  return lpips_backward(v, n, -1, nullptr, grad_a, gscale);
}

int gi_lpips_grad_tap(gi_lpips* v, int tap, float* out_nchw_f32) {
  GI_REQUIRE(v && v->gbound, "lpips_grad_tap: no grad workspace bound (gi_lpips_bind_grad)");
  GI_REQUIRE(v->synced && v->grad_n > 0, "lpips_grad_tap: no gi_lpips_distance_grad call to read back");
  GI_REQUIRE(out_nchw_f32 && tap >= 0 && tap < NTAP, "lpips_grad_tap: tap=%d", tap);
  // replays the backward of the last grad call from what it left in the workspace (maps, seeds, scales), down to the tap
  return lpips_backward(v, v->grad_n, tap, out_nchw_f32, nullptr, 1.f);
}

int gi_lpips_features(gi_lpips* v, const float* x, int n, int tap, float* out_nchw) {
  GI_REQUIRE(v && v->bound && v->synced, "lpips_features: bind + sync_weights first");
  GI_REQUIRE(x && out_nchw && n > 0 && n <= v->t.max_pairs && tap >= 0 && tap < NTAP, "lpips_features: n=%d tap=%d", n, tap);
  LpFinP fin = {};
  // the runner works on 2n stacked images: feed x twice, return the first n
  return lpips_run(v, x, x, n, tap, out_nchw, fin);
}

// ---- the kernels one at a time (test seam; include/ganinpaint.h). Every entry checks what its kernel assumes and goes through the host
// launch code above ------------------------------------------------------------------------------------------------------------------------
#define GI_LP_FITS31(count) ((int64_t)(count) > 0 && (int64_t)(count) < (1ll << 31))

int gi_debug_lpips_conv1(gi_ctx* ctx, const float* xa, const float* xb, int n, int H, int W, const float* wA, const float* wB, const float* bias,
                         void* out) {
  GI_REQUIRE(ctx && xa && xb && wA && wB && bias && out, "debug_lpips_conv1: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && W % 16 == 0, "debug_lpips_conv1: n=%d H=%d W=%d (W: a multiple of 16)", n, H, W);
  GI_REQUIRE(GI_LP_FITS31((int64_t)2 * n * H * W * 64), "debug_lpips_conv1: tensor beyond 32-bit offsets");
  return lp_conv1(ctx->stream, xa, xb, n, H, W, wA, wB, bias, (half_t*)out);
}

int gi_debug_lpips_fold(gi_ctx* ctx, const float* w, const float* shift, const float* scale, float* wA, float* wB) {
  GI_REQUIRE(ctx && w && shift && scale && wA && wB, "debug_lpips_fold: null pointer");
  return lp_fold(ctx->stream, w, shift, scale, wA, wB);
}

int64_t gi_debug_lpips_tap_ws_bytes(int n) { return n > 0 ? (int64_t)n * LP_MAXNB * 8 : -1; }

int gi_debug_lpips_tap(gi_ctx* ctx, const void* F, int n, int H, int W, int C, const float* lin, void* ws, int64_t ws_bytes, float* d_n, void* pooled) {
  GI_REQUIRE(ctx && F && lin && ws && d_n, "debug_lpips_tap: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && (C == 64 || C == 128 || C == 256 || C == 512), "debug_lpips_tap: n=%d H=%d W=%d C=%d (64, 128, 256 or 512)", n, H, W, C);
  GI_REQUIRE(GI_LP_FITS31((int64_t)2 * n * H * W * C), "debug_lpips_tap: tensor beyond 32-bit offsets");
  GI_REQUIRE(!pooled || (H % 2 == 0 && W % 2 == 0), "debug_lpips_tap: the pooled map needs even H=%d W=%d", H, W);
  GI_REQUIRE(((uintptr_t)F & 15) == 0 && ((uintptr_t)lin & 15) == 0 && ((uintptr_t)pooled & 15) == 0, "debug_lpips_tap: F, lin and pooled must be 16-byte aligned");
  GI_REQUIRE(ws_bytes >= gi_debug_lpips_tap_ws_bytes(n) && ((uintptr_t)ws & 7) == 0, "debug_lpips_tap: workspace %lld bytes (need %lld, 8-byte aligned)",
             (long long)ws_bytes, (long long)gi_debug_lpips_tap_ws_bytes(n));
  hipStream_t st = ctx->stream;
  GI_TRY(lp_tap(st, (const half_t*)F, n, H, W, C, lin, (half_t*)pooled, (double*)ws));
  LpFinP fin = {};
  fin.ntap = 1; fin.n = n; fin.pair_stride = n;
  fin.nb[0] = lp_tap_blocks(H, W, C, pooled != nullptr);
  fin.inv[0] = 1.0 / ((double)H * W);
  return lp_finish(st, (const double*)ws, fin, nullptr, d_n);
}

// ---- the backward's kernels one at a time ------------------------------------------------------------------------------------------------
int gi_debug_lpips_pack_t(gi_ctx* ctx, const float* w, void* out, int cout, int cin) {
  GI_REQUIRE(ctx && w && out, "debug_lpips_pack_t: null pointer");
  GI_REQUIRE(cout > 0 && cin > 0 && GI_LP_FITS31((int64_t)cout * 9 * cin), "debug_lpips_pack_t: cout=%d cin=%d", cout, cin);
  return pack3x3(ctx->stream, true, w, (half_t*)out, cout, cin);
}

int gi_debug_lpips_seed(gi_ctx* ctx, int store, void* F, int n, int HW, int C, const float* lin, unsigned* smax, const float* sc) {
  GI_REQUIRE(ctx && F && lin && (store ? sc != nullptr : smax != nullptr), "debug_lpips_seed: null pointer");
  GI_REQUIRE(n > 0 && HW > 0 && (C == 64 || C == 128 || C == 256 || C == 512), "debug_lpips_seed: n=%d HW=%d C=%d (64, 128, 256 or 512)", n, HW, C);
  GI_REQUIRE(GI_LP_FITS31((int64_t)2 * n * HW * C), "debug_lpips_seed: tensor beyond 32-bit offsets");
  GI_REQUIRE(((uintptr_t)F & 15) == 0 && ((uintptr_t)lin & 15) == 0, "debug_lpips_seed: F and lin must be 16-byte aligned");
  return lp_seed(ctx->stream, store != 0, (half_t*)F, n, HW, C, lin, smax, sc);
}

int gi_debug_lpips_scale(gi_ctx* ctx, const unsigned* smax, float* sc, int n) {
  GI_REQUIRE(ctx && smax && sc && n > 0, "debug_lpips_scale: null pointer or n=%d", n);
  return seed_scale(ctx->stream, smax, sc, n);
}

int gi_debug_lpips_act_bwd(gi_ctx* ctx, int pool, const void* g, const void* act, const void* seed, void* out, int n, int H, int W, int C, int relu) {
  GI_REQUIRE(ctx && act && out, "debug_lpips_act_bwd: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "debug_lpips_act_bwd: n=%d H=%d W=%d C=%d (C: a multiple of 8)", n, H, W, C);
  GI_REQUIRE(GI_LP_FITS31((int64_t)n * H * W * C), "debug_lpips_act_bwd: tensor beyond 32-bit offsets");
  GI_REQUIRE(!pool || (g && out != g && H % 2 == 0 && W % 2 == 0), "debug_lpips_act_bwd: the pool form needs g, out apart from g and even H=%d W=%d", H, W);
  GI_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)act & 15) == 0 && ((uintptr_t)seed & 15) == 0 && ((uintptr_t)out & 15) == 0,
             "debug_lpips_act_bwd: g, act, seed and out must be 16-byte aligned");
  return act_bwd(ctx->stream, pool != 0, (const half_t*)g, (const half_t*)act, (const half_t*)seed, (half_t*)out, n, H, W, C, relu);
}

int gi_debug_lpips_conv1_adjoint(gi_ctx* ctx, const void* D, const float* wA, const float* sc_inv, float gscale, float* dimg, int n, int H, int W) {
  GI_REQUIRE(ctx && D && wA && sc_inv && dimg, "debug_lpips_conv1_adjoint: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && GI_LP_FITS31((int64_t)n * H * W * 64), "debug_lpips_conv1_adjoint: n=%d H=%d W=%d", n, H, W);
  GI_REQUIRE(((uintptr_t)D & 15) == 0, "debug_lpips_conv1_adjoint: D must be 16-byte aligned");
  return conv1_adjoint(ctx->stream, (const half_t*)D, wA, sc_inv, 1, gscale, dimg, n, H, W);
}

}  // extern "C"
