// The VGG trunk that the VGG-19 perceptual / style losses (vgg.hip) and VGG-16 LPIPS (lpips.hip) both
// carry: weight packing for the mode-2 implicit-GEMM kernels, 2x2 max pooling, the read-backs, and the opt-in input-gradient chain
// (scale from the largest seed, activation backward with and without un-pooling, first-layer adjoint, grad-workspace arenas, the loop
// from the top convolution down). Everything the backward touches is s * gradient in fp16 with fp32 accumulation; s is a power of two
// per batch (VGG-19) or per image (LPIPS) and leaves in fp32 through `inv`. No float atomics here.
#include "vggtrunk.h"

namespace {

// [cout][cin][3][3] fp32 -> fp16 [cout][tap][cin]
__global__ void __launch_bounds__(256) pack3x3_kernel(const float* __restrict__ w, half_t* __restrict__ out, int cout, int cin) {
  const int64_t total = (int64_t)cout * 9 * cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cin);
    const int t = (int)((i / cin) % 9);
    const int o = (int)(i / ((int64_t)cin * 9));
    out[i] = (half_t)w[((int64_t)o * cin + c) * 9 + t];
  }
}
// [cout][cin][3][3] fp32 -> fp16 [cin][tap'][cout] with tap' = 8 - tap: the transpose of a 3x3 / s1 / p1 convolution is that convolution
// with the taps reversed and the channel roles exchanged, so the input-gradient GEMMs run on the forward's mode-2 kernels
__global__ void __launch_bounds__(256) pack3x3_t_kernel(const float* __restrict__ w, half_t* __restrict__ out, int cout, int cin) {
  const int64_t total = (int64_t)cin * 9 * cout;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i % cout);
    const int t = (int)((i / cout) % 9);
    const int c = (int)(i / ((int64_t)cout * 9));
    out[i] = (half_t)w[((int64_t)o * cin + c) * 9 + (8 - t)];
  }
}

// NHWC fp16 2x2 / stride 2 max pooling, 8 channels per thread
__global__ void __launch_bounds__(256) maxpool2_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int nimg, int Ho, int Wo,
                                                       int C) {
  const int cg = C / 8;
  const int64_t total = (int64_t)nimg * Ho * Wo * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % cg);
    const int64_t p = i / cg;
    const int x = (int)(p % Wo);
    const int64_t t = p / Wo;
    const int y = (int)(t % Ho);
    const int64_t img = t / Ho;
    const half_t* s = in + (((img * 2 * Ho + 2 * y) * 2 * Wo + 2 * x) * (int64_t)C) + g * 8;
    const h8_t a = *(const h8_t*)s, b = *(const h8_t*)(s + C);
    const h8_t c = *(const h8_t*)(s + (int64_t)2 * Wo * C), d = *(const h8_t*)(s + (int64_t)2 * Wo * C + C);
    *(h8_t*)(out + p * C + g * 8) = __builtin_elementwise_max(__builtin_elementwise_max(a, b), __builtin_elementwise_max(c, d));
  }
}

// NHWC fp16 feature map -> NCHW fp32 (parity / debugging)
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const half_t* __restrict__ in, float* __restrict__ out, int nimg, int HW, int C) {
  const int64_t total = (int64_t)nimg * HW * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t img = t / C;
    out[i] = (float)in[(img * HW + p) * C + c];
  }
}
// NHWC fp16 (s_i * gradient) -> NCHW fp32 gradient (gi_vgg19_grad_layer, gi_lpips_grad_tap)
__global__ void __launch_bounds__(256) nhwc_to_nchw_unscale_kernel(const half_t* __restrict__ in, const float* __restrict__ inv, int inv_stride,
                                                                   float* __restrict__ out, int nimg, int HW, int C) {
  const int64_t total = (int64_t)nimg * HW * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t img = t / C;
    out[i] = (float)in[(img * HW + p) * C + c] * inv[img * inv_stride];
  }
}

// Image i: s_i = 2^(kSeedExp - e) with its largest seed m * 2^e, m in [0.5, 1): the largest scaled seed lands in [2^(kSeedExp-1), 2^kSeedExp).
// All seeds zero (the two inputs are equal) or a non-finite maximum: s_i = 1. sc[i] = s_i, sc[n + i] = 1 / s_i; VGG-19 scales the whole
// batch by one s (n = 1: sc[0] = s, sc[1] = 1 / s). kSeedExp = -2: with the stand-in weights the largest gradient of
// any layer stays within 2x the largest seed (fp64 oracle), so 2^-2 leaves a factor 2^18 up to fp16's 65504 for weights that amplify
// more, and 12 binades of normal numbers (22 with subnormals) below the maximum.
constexpr int kSeedExp = -2;
__global__ void __launch_bounds__(64) seed_scale_kernel(const unsigned* __restrict__ smax, float* __restrict__ sc, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float am = __uint_as_float(smax[i]);
  int ex = 0;
  float s = 1.f;
  if (am > 0.f && am < INFINITY) {
    (void)frexpf(am, &ex);
    int k = kSeedExp - ex;
    k = k > 100 ? 100 : (k < -100 ? -100 : k);
    s = ldexpf(1.f, k);
  }
  sc[i] = s;
  sc[n + i] = 1.f / s;
}

// Activation backward between two input-gradient GEMMs, 16-byte NHWC accesses, 8 channels per thread; one fp16 rounding of the fp32 sum:
//   POOL = false: out = [act > 0] * (g + seed)                        (g and / or seed may be null; out may alias g)
//   POOL = true:  g lives on the (H/2, W/2) grid: every 2x2 window of `act` routes its value to the first maximum in row-major order
//                 (F.max_pool2d's backward; the arg-max is recomputed from the kept map), then out = [act > 0] * (routed g + seed) at all
//                 four positions. seed is null where the pooled layer is no tap (every pooled layer of VGG-19; the taps of LPIPS are its
//                 pooled layers, so there the seed joins here). The routed value passes through (half)((float)g + 0.f) even then: a
//                 gradient of -0 is stored as +0, every other value keeps its bits.
// relu = 0 drops the [act > 0] factor: the gradient w.r.t. the post-ReLU map itself (gi_vgg19_grad_layer, gi_lpips_grad_tap).
template <bool POOL>
__global__ void __launch_bounds__(256) act_bwd_kernel(const half_t* g, const half_t* __restrict__ act, const half_t* __restrict__ seed,
                                                      half_t* out, int nimg, int H, int W, int C, int relu) {
  const int cg = C / 8;
  const h8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (!POOL) {
    const int64_t total = (int64_t)nimg * H * W * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const h8_t a = *(const h8_t*)(act + i * 8);
      const h8_t gv = g ? *(const h8_t*)(g + i * 8) : z8;
      const h8_t sv = seed ? *(const h8_t*)(seed + i * 8) : z8;
      h8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (!relu || (float)a[e] > 0.f) ? (half_t)((float)gv[e] + (float)sv[e]) : (half_t)0.f;
      *(h8_t*)(out + i * 8) = o;
    }
  } else {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t total = (int64_t)nimg * Ho * Wo * cg;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int gq = (int)(i % cg);
      const int64_t pq = i / cg;
      const int x = (int)(pq % Wo);
      const int64_t tt = pq / Wo;
      const int y = (int)(tt % Ho);
      const int64_t img = tt / Ho;
      const int64_t o00 = (((img * H + 2 * y) * W + 2 * x) * (int64_t)C) + gq * 8;
      const int64_t off[4] = {o00, o00 + C, o00 + (int64_t)W * C, o00 + (int64_t)W * C + C};
      h8_t a[4], sv[4], o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[q] = *(const h8_t*)(act + off[q]); sv[q] = seed ? *(const h8_t*)(seed + off[q]) : z8; }
      const h8_t gv = *(const h8_t*)(g + pq * C + gq * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int best = 0;
        float bv = (float)a[0][e];
#pragma unroll
        for (int q = 1; q < 4; ++q) { const float av = (float)a[q][e]; if (av > bv) { bv = av; best = q; } }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float val = (q == best ? (float)gv[e] : 0.f) + (float)sv[q][e];
          o[q][e] = (!relu || (float)a[q][e] > 0.f) ? (half_t)val : (half_t)0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) *(h8_t*)(out + off[q]) = o[q];
    }
  }
}

// First-layer adjoint: dimg[i][y][x] = mul_i * sum_{ky,kx,o} w1[o][ky][kx] * D[i][y+1-ky][x+1-kx][o] in fp32 (the grey image feeds all three
// input channels, so the weights are the network's [64][9] fold of the first convolution over them), mul_i = gscale / s_i with 1 / s_i
// from device memory: the fp16 scale leaves here. A workgroup owns a 16 x 32 pixel tile: its threads reduce the 64 channels of each of
// the 18 x 34 halo pixels of D to nine per-tap sums T[tap] (one pass over D: 128 bytes per pixel in 16-byte loads, the weights through
// wave-uniform addresses) into LDS, then every output pixel adds its nine neighbours' sums. HBM-bound: D is read once plus the halo
// (20 %, mostly from L2).
__global__ void __launch_bounds__(256) conv1_adjoint_kernel(const half_t* __restrict__ D, const float* __restrict__ w1, const float* __restrict__ inv,
                                                            int inv_stride, float gscale, float* __restrict__ dimg, int H, int W) {
  constexpr int TH = 16, TW = 32, HH = TH + 2, HW_ = TW + 2, NH = HH * HW_;
  __shared__ float T[NH * 9];
  const int img = blockIdx.z, y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
  const half_t* Di = D + (int64_t)img * H * W * 64;
  for (int h = threadIdx.x; h < NH; h += 256) {
    const int hy = h / HW_, hx = h - hy * HW_;
    const int y = y0 - 1 + hy, x = x0 - 1 + hx;
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const half_t* src = Di + ((int64_t)y * W + x) * 64;
      h8_t v[8];
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8) v[c8] = *(const h8_t*)(src + c8 * 8);
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = (float)v[c8][e];
#pragma unroll
          for (int k = 0; k < 9; ++k) t[k] = fmaf(w1[(c8 * 8 + e) * 9 + k], d, t[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) T[h * 9 + k] = t[k];
  }
  __syncthreads();
  const float mul = gscale * inv[img * inv_stride];
  for (int o = threadIdx.x; o < TH * TW; o += 256) {
    const int ty = o / TW, tx = o - ty * TW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    float s = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) s += T[((ty + 2 - ky) * HW_ + (tx + 2 - kx)) * 9 + ky * 3 + kx];
    dimg[((int64_t)img * H + y) * W + x] = s * mul;
  }
}

}  // namespace

int pack3x3(hipStream_t st, bool transposed, const float* w, half_t* out, int cout, int cin) {
  const dim3 grid(grid_for((int64_t)cout * 9 * cin, 256, 2048));
  if (transposed) hipLaunchKernelGGL(pack3x3_t_kernel, grid, dim3(256), 0, st, w, out, cout, cin);
  else hipLaunchKernelGGL(pack3x3_kernel, grid, dim3(256), 0, st, w, out, cout, cin);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int conv3x3(hipStream_t st, const half_t* in, const half_t* w, half_t* out, int nimg, int H, int W, int cin, int cout, const float* bias, int act_out,
            int pool2, const half_t* mask, const half_t* add, IgemmArgs& a) {
  a = IgemmArgs{};
  a.in = in; a.w = w; a.out = out;
  a.bias = bias; a.partials = nullptr; a.ws = nullptr; a.ws_bytes = 0;
  a.n = nimg; a.Hs = H; a.Ws = W;
  a.cin = cin; a.ldin = cin; a.coffin = 0;
  a.cout = cout; a.ldout = cout; a.coffout = 0;
  a.relu_in = 0; a.relu_cend = 0; a.act_out = act_out; a.force_splitk = 0;
  a.pool2 = pool2;
  if (mask) {
    a.mask = mask; a.ldmask = cout; a.coffmask = 0; a.mask_slope = 0.f;
    a.add = add; a.ldadd = cout; a.coffadd = 0;
  }
  return op_igemm(st, GI_F16, 2, a);
}
int maxpool2(hipStream_t st, const half_t* in, half_t* out, int nimg, int Ho, int Wo, int C) {
  hipLaunchKernelGGL(maxpool2_kernel, dim3(grid_for((int64_t)nimg * Ho * Wo * (C / 8), 256, 8192)), dim3(256), 0, st, in, out, nimg, Ho, Wo, C);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int nhwc_to_nchw(hipStream_t st, const half_t* in, float* out, int nimg, int HW, int C) {
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((int64_t)nimg * HW * C, 256, 4096)), dim3(256), 0, st, in, out, nimg, HW, C);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int nhwc_to_nchw_unscale(hipStream_t st, const half_t* in, const float* inv, int inv_stride, float* out, int nimg, int HW, int C) {
  hipLaunchKernelGGL(nhwc_to_nchw_unscale_kernel, dim3(grid_for((int64_t)nimg * HW * C, 256, 4096)), dim3(256), 0, st, in, inv, inv_stride, out, nimg, HW,
                     C);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int seed_scale(hipStream_t st, const unsigned* smax, float* sc, int n) {
  hipLaunchKernelGGL(seed_scale_kernel, dim3((n + 63) / 64), dim3(64), 0, st, smax, sc, n);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int act_bwd(hipStream_t st, bool pool, const half_t* g, const half_t* act, const half_t* seed, half_t* out, int n, int H, int W, int C, int relu) {
  if (pool) {
    hipLaunchKernelGGL(act_bwd_kernel<true>, dim3(grid_for((int64_t)n * (H / 2) * (W / 2) * (C / 8), 256, 8192)), dim3(256), 0, st, g, act, seed, out, n, H,
                       W, C, relu);
  } else {
    hipLaunchKernelGGL(act_bwd_kernel<false>, dim3(grid_for((int64_t)n * H * W * (C / 8), 256, 8192)), dim3(256), 0, st, g, act, seed, out, n, H, W, C, relu);
  }
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int conv1_adjoint(hipStream_t st, const half_t* D, const float* w1, const float* inv, int inv_stride, float gscale, float* dimg, int n, int H, int W) {
  hipLaunchKernelGGL(conv1_adjoint_kernel, dim3((W + 31) / 32, (H + 15) / 16, n), dim3(256), 0, st, D, w1, inv, inv_stride, gscale, dimg, H, W);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// The forward's maps go to two arenas, alternating per stage (convolution or pooling): a stage reads the other arena and writes
// [first half | second half] behind what its arena must keep - the first halves of all convolutions (ReLU masks, pool routing) and both
// halves at the taps - so a second half nobody needs is overwritten by the stage after next.
void trunk_gws_layout(VggTrunk& t, WsTake& take) {
  int64_t pos[2] = {0, 0}, ext[2] = {0, 0}, start[2 * VGGTRUNK_MAXCONV];
  int H = t.H, W = t.W, k = 0;
  for (int i = 0; i < t.nconv; ++i) {
    const int64_t half = (int64_t)t.max_pairs * H * W * t.cout[i] * 2;
    start[2 * i] = pos[k & 1];
    if (start[2 * i] + 2 * half > ext[k & 1]) ext[k & 1] = start[2 * i] + 2 * half;
    pos[k & 1] += half * (t.tap_after[i] >= 0 ? 2 : 1);
    ++k;
    start[2 * i + 1] = -1;
    if (t.pool_after[i]) {
      H /= 2; W /= 2;
      start[2 * i + 1] = pos[k & 1];       // kept by nobody: the next stage of this arena starts at the same place
      const int64_t ph = (int64_t)t.max_pairs * H * W * t.cout[i] * 2;
      if (start[2 * i + 1] + 2 * ph > ext[k & 1]) ext[k & 1] = start[2 * i + 1] + 2 * ph;
      ++k;
    }
  }
  char* arena[2];
  arena[0] = take(ext[0]);
  arena[1] = take(ext[1]);
  for (int i = 0, kk = 0; i < t.nconv; ++i) {
    t.ga[i] = arena[kk & 1] ? (half_t*)(arena[kk & 1] + start[2 * i]) : nullptr;
    ++kk;
    t.gpool[i] = nullptr;
    if (t.pool_after[i]) { t.gpool[i] = arena[kk & 1] ? (half_t*)(arena[kk & 1] + start[2 * i + 1]) : nullptr; ++kk; }
  }
  t.wT[0] = nullptr;
  for (int i = 1; i < t.nconv; ++i) t.wT[i] = (half_t*)take((int64_t)t.cout[i] * 9 * t.cin[i] * 2);
  const int64_t gbytes = (int64_t)t.max_pairs * t.H * t.W * 64 * 2;
  t.gbuf[0] = (half_t*)take(gbytes);
  t.gbuf[1] = (half_t*)take(gbytes);
}

// D_l = s * gradient w.r.t. the PRE-activation of layer l = [a_l > 0] * (transposed conv of D_(l+1), un-pooled where a pool sits between,
// + seed_l at a tap). The seed of the layer below (null where it is no tap) goes to whichever site that layer uses: the GEMM epilogue's
// addend beside the ReLU mask, the un-pool, or the plain activation backward where the dispatched kernel applied no mask. At stop the
// [a > 0] factor is dropped and nothing is fused into the GEMM.
int trunk_backward(const VggTrunk& t, hipStream_t st, int n, int stop, float* layer_out, float* grad_out, float gscale) {
  int Hl[VGGTRUNK_MAXCONV], Wl[VGGTRUNK_MAXCONV];
  { int H = t.H, W = t.W; for (int i = 0; i < t.nconv; ++i) { Hl[i] = H; Wl[i] = W; if (t.pool_after[i]) { H /= 2; W /= 2; } } }
  auto seed_of = [&](int l) -> const half_t* { return t.tap_after[l] >= 0 ? t.ga[l] + (int64_t)n * Hl[l] * Wl[l] * t.cout[l] : nullptr; };
  auto readback = [&](const half_t* g, int l) { return nhwc_to_nchw_unscale(st, g, t.inv, t.inv_stride, layer_out, n, Hl[l] * Wl[l], t.cout[l]); };
  int cur = 0;
  const int top = t.nconv - 1;
  GI_TRY(act_bwd(st, false, nullptr, t.ga[top], seed_of(top), t.gbuf[cur], n, Hl[top], Wl[top], t.cout[top], stop != top));
  if (stop == top) return readback(t.gbuf[cur], top);
  for (int l = top; l >= 1; --l) {
    const int below = l - 1;
    const bool pool = t.pool_after[below] != 0, last = stop == below;
    const bool fuse = !pool && !last;
    IgemmArgs a;
    const int rc = conv3x3(st, t.gbuf[cur], t.wT[l], t.gbuf[cur ^ 1], n, Hl[l], Wl[l], t.cout[l], t.cin[l], nullptr, GI_ACT_NONE, 0,
                           fuse ? t.ga[below] : nullptr, fuse ? seed_of(below) : nullptr, a);
    if (rc == GI_ERR_UNSUPPORTED) gi_set_error("vgg trunk backward: no mode-2 kernel serves n=%d %dx%d %d->%d", n, Hl[l], Wl[l], t.cout[l], t.cin[l]);
    GI_TRY(rc);
    if (pool) {
      GI_TRY(act_bwd(st, true, t.gbuf[cur ^ 1], t.ga[below], seed_of(below), t.gbuf[cur], n, Hl[below], Wl[below], t.cout[below], !last));
    } else {
      cur ^= 1;
      if (!a.mask || !a.mask_applied)
        GI_TRY(act_bwd(st, false, t.gbuf[cur], t.ga[below], seed_of(below), t.gbuf[cur], n, Hl[below], Wl[below], t.cout[below], !last));
    }
    if (last) return readback(t.gbuf[cur], below);
  }
  return conv1_adjoint(st, t.gbuf[cur], t.w1, t.inv, t.inv_stride, gscale, grad_out, n, t.H, t.W);
}
