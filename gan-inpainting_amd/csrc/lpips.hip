// LPIPS (Zhang et al. 2018, `lpips` v0.1, net = 'vgg') between two batches of grey images: the learned perceptual distance the
// inpainting papers report next to FID. A metric of the evaluation pass only: no backward.
//
// `a` and `b` run as ONE stacked batch of 2n images (NHWC fp16), as in vgg.hip:
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

#include "common.h"

namespace {

constexpr int NCONV = 13, NTAP = 5;
const int kCin[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kCout[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kFeatIdx[NCONV] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};   // torchvision vgg16.features indices
const int kTapAfter[NCONV] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};   // a 2x2 max pool follows every tap but the last
const int kTapC[NTAP] = {64, 128, 256, 512, 512};
constexpr int LP_MAXNB = 128;      // workgroups (= fp64 partials) per image and tap, at most

// [cout][cin][3][3] fp32 -> fp16 [cout][tap][cin] (what the mode-2 kernels read; vgg.hip's pack3x3_kernel)
__global__ void __launch_bounds__(256) lpips_pack3x3_kernel(const float* __restrict__ w, half_t* __restrict__ out, int cout, int cin) {
  const int64_t total = (int64_t)cout * 9 * cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cin);
    const int t = (int)((i / cin) % 9);
    const int o = (int)(i / ((int64_t)cin * 9));
    out[i] = (half_t)w[((int64_t)o * cin + c) * 9 + t];
  }
}

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

#ifdef GI_LPIPS_UNFUSED
// the separate pooling pass of the A/B build (tools/time_lpips.py): NHWC fp16 2x2 / stride 2 max pooling, 8 channels per thread
__global__ void __launch_bounds__(256) lpips_maxpool2_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int nimg, int Ho, int Wo, int C) {
  const int cg = C / 8;
  const int64_t total = (int64_t)nimg * Ho * Wo * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % cg);
    const int64_t px = i / cg;
    const int x = (int)(px % Wo);
    const int64_t t = px / Wo;
    const int y = (int)(t % Ho);
    const int64_t img = t / Ho;
    const half_t* s = in + (((img * 2 * Ho + 2 * y) * 2 * Wo + 2 * x) * (int64_t)C) + g * 8;
    const h8_t a = *(const h8_t*)s, b = *(const h8_t*)(s + C);
    const h8_t c = *(const h8_t*)(s + (int64_t)2 * Wo * C), d = *(const h8_t*)(s + (int64_t)2 * Wo * C + C);
    *(h8_t*)(out + px * C + g * 8) = __builtin_elementwise_max(__builtin_elementwise_max(a, b), __builtin_elementwise_max(c, d));
  }
}
#endif

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

// NHWC fp16 feature map -> NCHW fp32 (parity / debugging)
__global__ void __launch_bounds__(256) lpips_nhwc_to_nchw_kernel(const half_t* __restrict__ in, float* __restrict__ out, int nimg, int HW, int C) {
  const int64_t total = (int64_t)nimg * HW * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int px = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t img = t / C;
    out[i] = (float)in[(img * HW + px) * C + c];
  }
}

// ---- host launch code: one copy of every grid rule, shared by the runner and the gi_debug_lpips_* entries -----------------------------

int lp_pack3x3(hipStream_t st, const float* w, half_t* out, int cout, int cin) {
  hipLaunchKernelGGL(lpips_pack3x3_kernel, dim3(grid_for((int64_t)cout * 9 * cin, 256, 2048)), dim3(256), 0, st, w, out, cout, cin);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
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
int lp_conv3x3(hipStream_t st, const half_t* in, const half_t* w, half_t* out, int nimg, int H, int W, int cin, int cout, const float* bias) {
  IgemmArgs a = IgemmArgs{};
  a.in = in; a.w = w; a.out = out;
  a.bias = bias; a.partials = nullptr; a.ws = nullptr; a.ws_bytes = 0;
  a.n = nimg; a.Hs = H; a.Ws = W;
  a.cin = cin; a.ldin = cin; a.coffin = 0;
  a.cout = cout; a.ldout = cout; a.coffout = 0;
  a.relu_in = 0; a.relu_cend = 0; a.act_out = GI_ACT_RELU; a.force_splitk = 0;
  const int rc = op_igemm(st, GI_F16, 2, a);
  if (rc == GI_ERR_UNSUPPORTED) gi_set_error("lpips: no mode-2 kernel serves n=%d %dx%d %d->%d", nimg, H, W, cin, cout);
  return rc;
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

}  // namespace

struct gi_lpips {
  gi_ctx* ctx;
  int H, W, max_pairs;
  int64_t woff[NCONV], boff[NCONV], linoff[NTAP], shiftoff, scaleoff;   // float offsets into params
  int64_t param_floats;
  const float* params;
  char* ws;
  int64_t ws_bytes;
  half_t* act[2];
  half_t* wpk[NCONV];     // [1..12] packed fp16 weights
  float* wA;              // conv1_1 folded weights [64][9]: image plane
  float* wB;              //                                 indicator plane
  double* partial;        // [5 taps][max_pairs][LP_MAXNB]
  bool bound, synced;
};

namespace {

int64_t lpips_ws_layout(gi_lpips* v, char* base) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += gi_align_up(bytes, 256); return p; };
  const int64_t act_bytes = (int64_t)2 * v->max_pairs * v->H * v->W * 64 * 2;      // the widest maps: relu1_1 / relu1_2
  v->act[0] = (half_t*)take(act_bytes);
  v->act[1] = (half_t*)take(act_bytes);
  v->wpk[0] = nullptr;
  for (int i = 1; i < NCONV; ++i) v->wpk[i] = (half_t*)take((int64_t)kCout[i] * 9 * kCin[i] * 2);
  v->wA = (float*)take(64 * 9 * 4);
  v->wB = (float*)take(64 * 9 * 4);
  v->partial = (double*)take((int64_t)NTAP * v->max_pairs * LP_MAXNB * 8);
  return off;
}

// the network on 2n stacked images; the taps leave their partials behind (fin: their counts). feat_out: stop at tap stop_tap and return
// its map of the first n images as NCHW fp32
int lpips_run(gi_lpips* v, const float* xa, const float* xb, int n, int stop_tap, float* feat_out, LpFinP& fin) {
  hipStream_t st = v->ctx->stream;
  const int nimg = 2 * n;
  int H = v->H, W = v->W, cur = 0;
  // (W % 16 == 0 and 2 n H W 64 < 2^31 are conditions of gi_lpips_create)
  GI_TRY(lp_conv1(st, xa, xb, n, H, W, v->wA, v->wB, v->params + v->boff[0], v->act[0]));
  for (int i = 1; i < NCONV; ++i) {
    GI_TRY(lp_conv3x3(st, v->act[cur], v->wpk[i], v->act[cur ^ 1], nimg, H, W, kCin[i], kCout[i], v->params + v->boff[i]));
    cur ^= 1;
    const int tap = kTapAfter[i], C = kCout[i];
    if (tap < 0) continue;
    if (feat_out && tap == stop_tap) {
      hipLaunchKernelGGL(lpips_nhwc_to_nchw_kernel, dim3(grid_for((int64_t)n * H * W * C, 256, 4096)), dim3(256), 0, st, v->act[cur], feat_out, n, H * W, C);
      GI_LAUNCH_CHECK();
      return GI_OK;
    }
    const bool pool = tap < NTAP - 1;
    double* partial = v->partial + (int64_t)tap * v->max_pairs * LP_MAXNB;
    fin.inv[tap] = 1.0 / ((double)H * W);
#ifdef GI_LPIPS_UNFUSED
    fin.nb[tap] = lp_tap_blocks(H, W, C, false);
    GI_TRY(lp_tap(st, v->act[cur], n, H, W, C, v->params + v->linoff[tap], nullptr, partial));
    if (pool) {
      hipLaunchKernelGGL(lpips_maxpool2_kernel, dim3(grid_for((int64_t)nimg * (H / 2) * (W / 2) * (C / 8), 256, 8192)), dim3(256), 0, st, v->act[cur],
                         v->act[cur ^ 1], nimg, H / 2, W / 2, C);
      GI_LAUNCH_CHECK();
    }
#else
    fin.nb[tap] = lp_tap_blocks(H, W, C, pool);
    GI_TRY(lp_tap(st, v->act[cur], n, H, W, C, v->params + v->linoff[tap], pool ? v->act[cur ^ 1] : nullptr, partial));
#endif
    if (pool) { cur ^= 1; H /= 2; W /= 2; }
  }
  return GI_OK;
}

}  // namespace

extern "C" {

int gi_lpips_create(gi_ctx* ctx, int H, int W, int max_pairs, gi_lpips** out) {
  GI_REQUIRE(ctx && out, "lpips_create: null argument");
  GI_REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && max_pairs > 0, "lpips_create: H=%d W=%d (multiples of 16) pairs=%d", H, W, max_pairs);
  GI_REQUIRE((int64_t)2 * max_pairs * H * W * 64 < (1ll << 31), "lpips_create: 2*%d images of %dx%d exceed 32-bit activation offsets", max_pairs, H, W);
  gi_lpips* v = new (std::nothrow) gi_lpips();
  GI_REQUIRE(v, "lpips_create: out of host memory");
  v->ctx = ctx; v->H = H; v->W = W; v->max_pairs = max_pairs;
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
  GI_TRY(lp_fold(st, v->params + v->woff[0], v->params + v->shiftoff, v->params + v->scaleoff, v->wA, v->wB));
  for (int i = 1; i < NCONV; ++i) GI_TRY(lp_pack3x3(st, v->params + v->woff[i], v->wpk[i], kCout[i], kCin[i]));
  v->synced = true;
  return GI_OK;
}

int gi_lpips_distance(gi_lpips* v, const float* a, const float* b, int n, float* out_n, float* per_layer_5n) {
  GI_REQUIRE(v && v->bound && v->synced, "lpips_distance: bind + sync_weights first");
  GI_REQUIRE(a && b && out_n && n > 0 && n <= v->max_pairs, "lpips_distance: n=%d (max %d)", n, v->max_pairs);
  LpFinP fin = {};
  fin.ntap = NTAP; fin.n = n; fin.pair_stride = v->max_pairs;
  GI_TRY(lpips_run(v, a, b, n, -1, nullptr, fin));
  return lp_finish(v->ctx->stream, v->partial, fin, out_n, per_layer_5n);
}

int gi_lpips_features(gi_lpips* v, const float* x, int n, int tap, float* out_nchw) {
  GI_REQUIRE(v && v->bound && v->synced, "lpips_features: bind + sync_weights first");
  GI_REQUIRE(x && out_nchw && n > 0 && n <= v->max_pairs && tap >= 0 && tap < NTAP, "lpips_features: n=%d tap=%d", n, tap);
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

}  // extern "C"
