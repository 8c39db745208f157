// VGG-19 feature extractor for the perceptual / style losses of the reference
// (lib/models/loss.py:50-115 perceptual_loss / style_loss / perceptual_and_style_loss, gram_matrix
// :117-136; taps after features[1,6,11,20,29] = relu1_1 .. relu5_1).
//
// Forward: the reference evaluates these losses under no_grad on detached inputs, so by default nothing
// reaches the generator and gi_vgg19_perceptual_style is all that runs. The opt-in backward (second half of
// this file, gi_vgg19_perceptual_style_grad) is the analytic gradient of the same two terms
// w.r.t. `output`: it needs its own workspace (gi_vgg19_bind_grad) and departs from the reference.
// `output` and `target` run as ONE stacked batch of 2n images (NHWC fp16):
//   conv1_1  the input is the grey image repeated over 3 channels (loss.py:54-55), so the 3->64 conv is
//            a 1->64 conv with the weights summed over the input channel: one HBM-bound VALU kernel;
//   12 more  3x3/s1/p1 convolutions + bias + ReLU: igemm3 mode 2 (fp16 MFMA implicit GEMM, LDS-DMA ring; vggtrunk.hip's conv3x3);
//   2x2 max pooling: 16-byte NHWC kernel (vggtrunk.hip's maxpool2);
//   taps     perceptual term mean((F_o - F_t)^2) and the Gram matrices F^T F / (H W C) (MFMA GEMM with K = pixels,
//            both operands pixel-major: transposing LDS reads as in wgrad.hip) in ONE pass per tap over the
//            image pairs (gram2_kernel: partial tiles, no atomics), then mean((G_o - G_t)^2) from the
//            partial tiles in a fixed order; one finish launch for all ten terms.
// The trunk's shared pieces (weight packing, pooling, read-backs, and the backward's scale, activation backward, first-layer adjoint,
// workspace arenas and chain) are vggtrunk.hip's, which LPIPS (lpips.hip) runs too.
#include <new>

#include "vggtrunk.h"

namespace {

constexpr int NCONV = 13;
const int kCin[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
const int kCout[NCONV] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
const int kFeatIdx[NCONV] = {0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28};   // torchvision vgg19.features indices
// after conv i: tap index (or -1), then pool?
const int kTapAfter[NCONV] = {0, -1, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, 4};
const int kPoolAfter[NCONV] = {0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0};

// conv1_1 on a channel-replicated grey image: w1[o][tap] = sum_c w[o][c][tap]
__global__ void __launch_bounds__(256) sum_cin_kernel(const float* __restrict__ w, float* __restrict__ w1, int cout, int cin) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cout * 9) return;
  const int o = i / 9, t = i % 9;
  float s = 0.f;
  for (int c = 0; c < cin; ++c) s += w[((int64_t)o * cin + c) * 9 + t];
  w1[i] = s;
}

// out[img,y,x,0:64] = relu(b + sum_tap w1[.][tap] * x[img, y-1+ky, x-1+kx]); images [0,n) from xa, [n,2n) from xb.
// On the matrix cores: D[channel][pixel] = A[channel][tap] * B[tap][pixel] with K = 9 taps padded to 16
// (v_mfma_f32_16x16x16_f16, fp32 accumulate; image and summed weights rounded to fp16 - the layer's output is stored in fp16
// anyway). A wave owns 16 consecutive pixels of an image row; lane (pixel, k-chunk kq) loads taps 4 kq .. 4 kq + 3 from clamped
// addresses (selects, no divergent branches; the group index is wave-uniform: scalar 32-bit index arithmetic). Channel order per
// tile as in c1_gather_mfma_kernel: two 16-byte stores per lane, 64 contiguous bytes per pixel and instruction. The VALU form of
// rounds 1-2 ran at 2 TB/s of stores (72 FMAs and 9 guarded loads per 16 output bytes); this layer is 537 MB of stores at 512x512.
__global__ void __launch_bounds__(256) vgg_conv1_mfma_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int n, int H, int W,
                                                             const float* __restrict__ w1, const float* __restrict__ bias,
                                                             half_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, kq = lane >> 4;
  h4_t af[4];
  float br[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int ch = ((mt >> 1) & 1) * 32 + (lr >> 2) * 8 + (mt & 1) * 4 + (lr & 3);     // A row lr of tile mt
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int t = 4 * kq + j; af[mt][j] = t < 9 ? (half_t)w1[ch * 9 + t] : (half_t)0.f; }
    // D row i = 4 kq + r of tile mt is channel ((mt >> 1) & 1) * 32 + kq * 8 + (mt & 1) * 4 + r
#pragma unroll
    for (int r = 0; r < 4; ++r) br[mt][r] = bias[((mt >> 1) & 1) * 32 + kq * 8 + (mt & 1) * 4 + r];
  }
  const int gpr = W >> 4;                                   // 16-pixel groups per image row
  const int ngroups = 2 * n * H * gpr;                      // < 2^31 (host check)
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256 + threadIdx.x) >> 6));
  const int nwaves = (int)gridDim.x * 4;
  int dy[4], dx[4];                                         // this lane's taps: (ky, kx) - 1, or far outside for the padding of K
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = 4 * kq + j;
    dy[j] = t < 9 ? t / 3 - 1 : -(1 << 20);
    dx[j] = t < 9 ? t % 3 - 1 : 0;
  }
  auto load_b = [&](int g, float (&bv)[4]) {
    const int rowi = g / gpr;                               // wave-uniform
    const int x = (g - rowi * gpr) * 16 + lr;
    const int img = rowi / H, y = rowi - img * H;
    const float* src = img < n ? xa + (int64_t)img * H * W : xb + (int64_t)(img - n) * H * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iy = y + dy[j], ix = x + dx[j];
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = src[ok ? iy * W + ix : 0];
      bv[j] = ok ? v : 0.f;
    }
  };
  float bv[4], bn[4];
  int g = wave;
  if (g < ngroups) load_b(g, bv);
  for (; g < ngroups; g += nwaves) {
    if (g + nwaves < ngroups) load_b(g + nwaves, bn);
    const h4_t bf = {(half_t)bv[0], (half_t)bv[1], (half_t)bv[2], (half_t)bv[3]};
    h8_t o[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f4_t acc = {br[mt][0], br[mt][1], br[mt][2], br[mt][3]};
      acc = __builtin_amdgcn_mfma_f32_16x16x16f16(af[mt], bf, acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[mt >> 1][(mt & 1) * 4 + r] = (half_t)fmaxf(acc[r], 0.f);
    }
    half_t* dst = out + ((int64_t)g * 16 + lr) * 64;
    *(h8_t*)(dst + kq * 8) = o[0];
    *(h8_t*)(dst + 32 + kq * 8) = o[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = bn[j];
  }
}

__device__ __forceinline__ double blk_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// ---- Gram + perceptual term in one pass over a tap's feature maps (deterministic) ------------------------------------------------
// A workgroup owns one (c1 block, c2 block) tile of the Gram matrix (blocks of BLK = 2 WT channels, c1 block <= c2 block: the matrix
// is symmetric), one pixel range (split) and one image PAIR (output image i, target image i + n): per 32-pixel step it stages the
// 32 x BLK slices of both images (one slice on diagonal tiles), multiplies both Grams on the matrix cores (four waves, WT x WT each,
// transposing LDS reads as in the kernel above) and - on diagonal tiles, where every channel slice passes exactly once - adds up
// (F_o - F_t)^2 from the staging registers. Partial Grams go to P[pair][o|t][tile][split][BLK*BLK] with plain stores;
// gram2_diff_kernel adds the splits in a fixed order and reduces (G_o - G_t)^2 (off-diagonal tiles count twice). No atomics, no
// memset, the feature maps are read C / BLK (+1) / 2 times instead of 2 C / 64 times + once more for the perceptual term.
struct Gram2P {
  const char* F;      // [2n][HW][C] fp16
  float* P;           // partial Grams
  double* sq;         // [pairs][nblk][split] partial sums of (F_o - F_t)^2
  int C, HW, n, nblk, ntile, split, steps_per_split;
};
template <int WT>
__global__ void __launch_bounds__(256) gram2_kernel(Gram2P p) {
  constexpr int BLK = 2 * WT, ROWB = BLK * 2, LROW = ROWB + 32, SL = 32 * LROW;   // one staged slice: 32 pixels
  constexpr int CPR = ROWB / 16, RPP = 256 / CPR, NL = 32 / RPP;                  // 16-byte chunks per row, rows per pass, passes
  constexpr int MT = WT / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];                     // [2 stages][o c1, o c2, t c1, t c2][SL]
  __shared__ double shd[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int bi = 0, bj = 0;
  { int t = blockIdx.x; for (bi = 0; t >= p.nblk - bi; ++bi) t -= p.nblk - bi; bj = bi + t; }   // tile index -> (bi <= bj)
  const bool diag = bi == bj;
  const int pair = blockIdx.z, sp = blockIdx.y;
  const char* Fo = p.F + (int64_t)pair * p.HW * p.C * 2;
  const char* Ft = p.F + (int64_t)(pair + p.n) * p.HW * p.C * 2;
  const int steps = (p.HW + 31) / 32;
  const int s0 = sp * p.steps_per_split, s1 = min(steps, s0 + p.steps_per_split);
  const int chunk = tid % CPR, rbase = tid / CPR;
  u4_t r[4][NL];      // [o c1, o c2, t c1, t c2]
  auto gload = [&](int st) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int pix = st * 32 + rbase + RPP * i;
      const bool ok = pix < p.HW;
      const int64_t o1 = ((int64_t)pix * p.C + bi * BLK + chunk * 8) * 2, o2 = ((int64_t)pix * p.C + bj * BLK + chunk * 8) * 2;
      const u4_t z = u4_t{0u, 0u, 0u, 0u};
      r[0][i] = ok ? *(const u4_t*)(Fo + o1) : z;
      r[2][i] = ok ? *(const u4_t*)(Ft + o1) : z;
      if (!diag) { r[1][i] = ok ? *(const u4_t*)(Fo + o2) : z; r[3][i] = ok ? *(const u4_t*)(Ft + o2) : z; }
    }
  };
  float sq = 0.f;
  auto lds_store = [&](int stage) {
    char* base = smem + stage * 4 * SL;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int off = (rbase + RPP * i) * LROW + chunk * 16;
      *(u4_t*)(base + 0 * SL + off) = r[0][i];
      *(u4_t*)(base + 2 * SL + off) = r[2][i];
      if (!diag) { *(u4_t*)(base + 1 * SL + off) = r[1][i]; *(u4_t*)(base + 3 * SL + off) = r[3][i]; }
      else {
        const h8_t a = __builtin_bit_cast(h8_t, r[0][i]), b = __builtin_bit_cast(h8_t, r[2][i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = (float)a[e] - (float)b[e]; sq = fmaf(d, d, sq); }
      }
    }
  };
  f4_t acc[2][MT][MT];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[q][i][j] = f4_t{0.f, 0.f, 0.f, 0.f};
  auto frag = [&](const char* base, int ch) -> h8_t {      // 32 (k = pixels) x 16 (channels ch ..) as an MFMA operand
    const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, pp = i16 & 3;
    const char* lo_p = base + (8 * g + q) * LROW + (ch + 4 * pp) * 2;
    const char* hi_p = base + (8 * g + 4 + q) * LROW + (ch + 4 * pp) * 2;
    fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)lo_p);
    fp16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)hi_p);
    h4_t l4 = __builtin_bit_cast(h4_t, lo), h4 = __builtin_bit_cast(h4_t, hi);
    return h8_t{l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
  };
  auto compute = [&](int stage) {
    const char* base = smem + stage * 4 * SL;
#pragma unroll
    for (int q = 0; q < 2; ++q) {       // output image, target image
      const char* sA = base + (2 * q) * SL;
      const char* sB = diag ? sA : sA + SL;
      h8_t af[MT], bf[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[mt] = frag(sA, wm * WT + mt * 16);
#pragma unroll
      for (int nt = 0; nt < MT; ++nt) bf[nt] = frag(sB, wn * WT + nt * 16);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < MT; ++nt) acc[q][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf[nt], acc[q][mt][nt], 0, 0, 0);
    }
  };
  // (a second register set holding step st + 2 while st + 1 waits was measured slower: 54 -> 87 us average on the 128-channel taps)
  if (s0 < s1) {
    gload(s0);
    lds_store(0);
    __syncthreads();
    int stage = 0;
    for (int st = s0; st < s1; ++st) {
      const bool more = st + 1 < s1;
      if (more) gload(st + 1);
      compute(stage);
      if (more) lds_store(stage ^ 1);
      __syncthreads();
      stage ^= 1;
    }
  }
  // partial Grams: P[((pair * 2 + q) * ntile + tile) * split + sp][BLK][BLK]
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float* P = p.P + ((((int64_t)pair * 2 + q) * p.ntile + blockIdx.x) * p.split + sp) * (BLK * BLK);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = wm * WT + mt * 16 + (lane >> 4) * 4 + rr;
#pragma unroll
        for (int nt = 0; nt < MT; ++nt) P[row * BLK + wn * WT + nt * 16 + (lane & 15)] = acc[q][mt][nt][rr];
      }
  }
  if (diag) {
    double s = (double)sq;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) shd[wave] = s;
    __syncthreads();
    if (tid == 0) p.sq[((int64_t)pair * p.nblk + bi) * p.split + sp] = (shd[0] + shd[1]) + (shd[2] + shd[3]);
  }
}
// partial[block] = sum over the block's groups of 64 Gram elements (grid-stride) of w * ((sum_s P_o - sum_s P_t) * scale)^2: thread
// (element, part) adds a quarter of the splits (contiguous range, ascending), the four parts are added in ascending order; w = 2 on
// off-diagonal tiles (their mirror images are never computed). bb = BLK * BLK is a multiple of 64: a group lies inside one tile.
__global__ void __launch_bounds__(256) gram2_diff_kernel(const float* __restrict__ P, int n, int nblk, int ntile, int split, int bb,
                                                         float scale, double* __restrict__ partial) {
  __shared__ float red[2][3][64];
  __shared__ double sh[4];
  const int e64 = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int64_t per_pair = (int64_t)ntile * bb;
  const int64_t groups = (int64_t)n * per_pair / 64;
  const int per = (split + 3) / 4, k0 = part * per, k1 = min(split, k0 + per);
  double s = 0.0;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t i = g * 64 + e64;
    const int pair = (int)(i / per_pair);
    const int64_t rem = i - (int64_t)pair * per_pair;
    const int tile = (int)(rem / bb), e = (int)(rem - (int64_t)tile * bb);
    const float* po = P + ((((int64_t)pair * 2 + 0) * ntile + tile) * split) * bb + e;
    const float* pt = P + ((((int64_t)pair * 2 + 1) * ntile + tile) * split) * bb + e;
    float go = 0.f, gt = 0.f;
    for (int k = k0; k < k1; ++k) { go += po[(int64_t)k * bb]; gt += pt[(int64_t)k * bb]; }
    __syncthreads();                 // the previous group's sums have been read
    if (part > 0) { red[0][part - 1][e64] = go; red[1][part - 1][e64] = gt; }
    __syncthreads();
    if (part == 0) {
      go = ((go + red[0][0][e64]) + red[0][1][e64]) + red[0][2][e64];
      gt = ((gt + red[1][0][e64]) + red[1][1][e64]) + red[1][2][e64];
      int t = tile, bi = 0;
      for (; t >= nblk - bi; ++bi) t -= nblk - bi;
      const double d = (double)(go * scale) - (double)(gt * scale);
      s += (t == 0 ? 1.0 : 2.0) * d * d;
    }
  }
  s = blk_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
struct VggFinP { int nb[10]; double inv[10]; };
// per_tap[k] = inv[k] * sum of the nb[k] partials of term k (ascending), then out2 = (wp * sum of the 5 perceptual terms, ws * sum of the 5 style terms)
__global__ void __launch_bounds__(256) vgg_finish_kernel(const double* __restrict__ partial, VggFinP f, float* __restrict__ per_tap, float wp, float ws,
                                                         float* __restrict__ out2) {
  __shared__ double sh[4];
  __shared__ float terms[10];
  for (int k = 0; k < 10; ++k) {
    double s = 0.0;
    for (int i = threadIdx.x; i < f.nb[k]; i += 256) s += partial[k * 1024 + i];
    s = blk_sum(s, sh);
    if (threadIdx.x == 0) { terms[k] = (float)(s * f.inv[k]); per_tap[k] = terms[k]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float pp = 0.f, ss = 0.f;
    for (int t = 0; t < 5; ++t) { pp += terms[t]; ss += terms[5 + t]; }
    out2[0] = wp * pp;
    out2[1] = ws * ss;
  }
}

// ================================================================================================================================
// Opt-in backward: d(weight_p * P + weight_s * S) / d(output), target constant. Everything runs on s * gradient in fp16 with
// fp32 accumulation, s = 2^k chosen on the device from the largest seed (vggtrunk.hip's seed_scale_kernel, n = 1) and removed in fp32 by
// the last kernel. This file holds the seeds; the chain below them is vggtrunk.hip's trunk_backward.
// No float atomics: the only atomic is an unsigned max over bit patterns of non-negative floats, whose result does not depend on order.
// ================================================================================================================================

// max over a 256-thread workgroup, then ONE unsigned atomic max per workgroup (bit patterns of non-negative floats order like the
// floats; a maximum does not depend on the order of its operands, so the result is the same in every run)
__device__ __forceinline__ void amax_commit_block(float m, float* red4, unsigned* dst) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red4[0], red4[1]), fmaxf(red4[2], red4[3]));
    if (m > 0.f) atomicMax(dst, __float_as_uint(m));
  }
}

// dense Gram difference of a tap from gram2_kernel's partial tiles: dg[pair][c1][c2] = (sum_s P_o - sum_s P_t) * scale, splits added in
// ascending order (eight loads in flight), off-diagonal tiles mirrored (the matrix is symmetric); amax: max |dg| of the tap. A workgroup
// owns a 16 x 16 block of a tile (grid: blocks per tile, tiles, pairs): both the block and its mirror image (through LDS) leave in 64-byte rows.
__global__ void __launch_bounds__(256) gram_delta_kernel(const float* __restrict__ P, int nblk, int ntile, int split, int BLK, int C, float scale,
                                                         float* __restrict__ dg, unsigned* __restrict__ amax) {
  __shared__ float sm[16][17];
  __shared__ float red[4];
  const int bb = BLK * BLK, per_row = BLK / 16;
  const int pair = blockIdx.z, tile = blockIdx.y;
  const int r0 = (blockIdx.x / per_row) * 16, c0 = (blockIdx.x % per_row) * 16;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int e = (r0 + ty) * BLK + c0 + tx;
  const float* po = P + ((((int64_t)pair * 2 + 0) * ntile + tile) * split) * bb + e;
  const float* pt = P + ((((int64_t)pair * 2 + 1) * ntile + tile) * split) * bb + e;
  float go = 0.f, gt = 0.f;
  int k = 0;
  for (; k + 8 <= split; k += 8) {
    float vo[8], vt[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { vo[j] = po[(int64_t)(k + j) * bb]; vt[j] = pt[(int64_t)(k + j) * bb]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { go += vo[j]; gt += vt[j]; }
  }
  for (; k < split; ++k) { go += po[(int64_t)k * bb]; gt += pt[(int64_t)k * bb]; }
  const float d = go * scale - gt * scale;
  int t = tile, bi = 0;
  for (; t >= nblk - bi; ++bi) t -= nblk - bi;
  const int bj = bi + t;
  float* D = dg + (int64_t)pair * C * C;
  D[(int64_t)(bi * BLK + r0 + ty) * C + bj * BLK + c0 + tx] = d;
  if (bi != bj) {
    sm[ty][tx] = d;
    __syncthreads();
    D[(int64_t)(bj * BLK + c0 + ty) * C + bi * BLK + r0 + tx] = sm[tx][ty];
  }
  amax_commit_block(fabsf(d), red, amax);
}

// Seed of a tap: seed[p][c] = cs * sum_k dG[c][k] F_o[p][k] + cp * (F_o[p][c] - F_t[p][c])   (style: one MFMA GEMM per image, K = C;
// perceptual: the epilogue). dG is rounded to fp16 after a power-of-two normalisation by its own maximum (dmax), which the fp32
// coefficient takes back. A wave owns 64 pixels x 64 channels; both operands come straight from global memory in MFMA layout (dG is
// symmetric: row c of dG is column c, K contiguous; F_o is pixel-major, K contiguous). The channel order per 16-row tile is
// vgg_conv1_mfma_kernel's: a lane ends up with 2 x 8 consecutive channels of a pixel, 16-byte accesses.
// STORE = true: s * seed in fp16 OVER the target half of the tap's feature map (each element of F_t is read by the one lane that
// overwrites it; nothing else reads F_t after the forward).
// STORE = false: max |seed| only - the magnitude the scale s is chosen from. Maps of more than kSeedSampleAll pixel blocks per image
// are SAMPLED: one block of every eight (block 8 j + (3 j mod 8): all column positions, spread over the rows), so that this pass
// costs an eighth of the store pass where the maps are large. The sample can only under-estimate the maximum; the headroom of
// kSeedExp (vggtrunk.hip) covers that.
struct SeedP {
  const half_t* Fo; half_t* Ft; const float* dg; const unsigned* dmax; unsigned* smax; const float* sc;
  int C, HW, nb; float cp, cs;      // nb: 256-pixel blocks per image
};
constexpr int kSeedSampleAll = 8;
template <bool STORE>
__global__ void __launch_bounds__(256) vgg_seed_kernel(SeedP p) {
  constexpr int NJ = 4;
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, g = lane >> 4;
  int pb = blockIdx.x;
  if (!STORE && p.nb > kSeedSampleAll) { pb = 8 * blockIdx.x + ((3 * blockIdx.x) & 7); if (pb >= p.nb) pb = 8 * blockIdx.x; }
  const int pair = blockIdx.z, c0 = blockIdx.y * 64, pix0 = pb * 256 + wave * 64;
  const half_t* Fo = p.Fo + (int64_t)pair * p.HW * p.C;
  half_t* Ft = p.Ft + (int64_t)pair * p.HW * p.C;
  const float* dg = p.dg + (int64_t)pair * p.C * p.C;
  const float dm = __uint_as_float(*p.dmax);
  int ex = 0;
  if (dm > 0.f) (void)frexpf(dm, &ex);          // dm = m * 2^ex, m in [0.5, 1)
  const float t = ldexpf(1.f, -ex), cs = p.cs * ldexpf(1.f, ex);
  f4_t acc[4][NJ];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[mt][j] = f4_t{0.f, 0.f, 0.f, 0.f};
  const float* arow[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) arow[mt] = dg + (int64_t)(c0 + ((mt >> 1) & 1) * 32 + (lr >> 2) * 8 + (mt & 1) * 4 + (lr & 3)) * p.C + g * 8;
  bool ok[NJ];
  const half_t* brow[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int pix = pix0 + 16 * j + lr;
    ok[j] = pix < p.HW;
    brow[j] = Fo + (int64_t)(ok[j] ? pix : 0) * p.C + g * 8;
  }
  for (int k0 = 0; k0 < p.C; k0 += 32) {
    h8_t af[4], bf[NJ];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const f4_t x = *(const f4_t*)(arow[mt] + k0), y = *(const f4_t*)(arow[mt] + k0 + 4);
      af[mt] = h8_t{(half_t)(x[0] * t), (half_t)(x[1] * t), (half_t)(x[2] * t), (half_t)(x[3] * t),
                    (half_t)(y[0] * t), (half_t)(y[1] * t), (half_t)(y[2] * t), (half_t)(y[3] * t)};
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const u4_t raw = *(const u4_t*)(brow[j] + k0);
      bf[j] = __builtin_bit_cast(h8_t, ok[j] ? raw : u4_t{0u, 0u, 0u, 0u});
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf[j], acc[mt][j], 0, 0, 0);
  }
  // D row 4 g + r of tile mt is channel c0 + (mt >> 1) * 32 + g * 8 + (mt & 1) * 4 + r, D column lr is the pixel
  const float s = STORE ? p.sc[0] : 1.f;
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (!ok[j]) continue;
    const int64_t base = (int64_t)(pix0 + 16 * j + lr) * p.C + c0 + g * 8;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const h8_t fo = *(const h8_t*)(Fo + base + hf * 32), ft = *(const h8_t*)(Ft + base + hf * 32);
      h8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float val = fmaf(cs, acc[hf * 2 + (e >> 2)][j][e & 3], p.cp * ((float)fo[e] - (float)ft[e]));
        if (STORE) o[e] = (half_t)(val * s);
        else m = fmaxf(m, fabsf(val));
      }
      if (STORE) *(h8_t*)(Ft + base + hf * 32) = o;
    }
  }
  if (!STORE) amax_commit_block(m, red, p.smax);
}

// ---- host launch code of this file's kernels: one copy of every grid rule, shared by the network runners below and the
// gi_debug_vgg_* entries (the trunk's: vggtrunk.h) ------------------------------------------------------------------------------------

int sum_cin(hipStream_t st, const float* w, float* w1) {
  hipLaunchKernelGGL(sum_cin_kernel, dim3(3), dim3(256), 0, st, w, w1, 64, 3);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
// (W % 16 == 0 and 2 n H W 64 < 2^31 are conditions of the callers)
int conv1(hipStream_t st, const float* xa, const float* xb, int n, int H, int W, const float* w1, const float* bias, half_t* out) {
  hipLaunchKernelGGL(vgg_conv1_mfma_kernel, dim3(grid_for((int64_t)2 * n * H * (W / 16), 4, 256 * 8)), dim3(256), 0, st, xa, xb, n, H, W, w1, bias, out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
// Both terms of one tap (+ its dense Gram difference when dgram is given) from F [2n][HW][C]: gram2_kernel over `split` pixel ranges,
// then the fixed-order reductions. The partial counts and the 1 / element counts of the two terms go to fin (terms tap and 5 + tap),
// the partial sums to partial[tap * 1024 ..] and partial[(5 + tap) * 1024 ..]. force_split > 0 replaces the heuristic's first guess
// (test seam); the workspace limits and the even division of the steps apply to it as to the heuristic's.
int tap_terms(hipStream_t st, const half_t* F, int n, int64_t HW, int C, int tap, float* gram, int64_t gram_bytes, double* partial, VggFinP& fin,
              float* dgram, unsigned* amax, int force_split, int* split_out) {
  const int BLK = C >= 128 ? 128 : 64, nb_ = C / BLK, ntile = nb_ * (nb_ + 1) / 2;
  const int steps = (int)((HW + 31) / 32);
  int split = (512 + n * ntile - 1) / (n * ntile);
  if (split > steps / 4) split = steps / 4;
  if (force_split > 0) split = force_split < steps ? force_split : steps;
  while (split > 1 && ((int64_t)2 * n * ntile * split * BLK * BLK * 4 > gram_bytes || n * nb_ * split > 1024)) --split;
  if (split < 1) split = 1;
  GI_REQUIRE((int64_t)2 * n * ntile * split * BLK * BLK * 4 <= gram_bytes && n * nb_ * split <= 1024, "vgg19: %d pairs exceed the Gram workspace", n);
  Gram2P gp;
  gp.F = (const char*)F; gp.P = gram; gp.sq = partial + tap * 1024;
  gp.C = C; gp.HW = (int)HW; gp.n = n; gp.nblk = nb_; gp.ntile = ntile;
  gp.steps_per_split = (steps + split - 1) / split;
  split = (steps + gp.steps_per_split - 1) / gp.steps_per_split;
  gp.split = split;
  if (BLK == 128) {
    static GiDevOnce attr;
    if (attr.first()) { GI_HIP(hipFuncSetAttribute((const void*)gram2_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4 * 32 * 288)); }
    hipLaunchKernelGGL(gram2_kernel<64>, dim3(ntile, split, n), dim3(256), 2 * 4 * 32 * 288, st, gp);
  } else {
    hipLaunchKernelGGL(gram2_kernel<32>, dim3(ntile, split, n), dim3(256), 2 * 4 * 32 * 160, st, gp);
  }
  GI_LAUNCH_CHECK();
  fin.nb[tap] = n * nb_ * split;
  fin.inv[tap] = 1.0 / (double)((int64_t)n * HW * C);
  const int nb2 = grid_for((int64_t)n * ntile * BLK * BLK / 64, 1, 1024);
  hipLaunchKernelGGL(gram2_diff_kernel, dim3(nb2), dim3(256), 0, st, (const float*)gram, n, nb_, ntile, split, BLK * BLK,
                     (float)(1.0 / ((double)HW * C)), partial + (5 + tap) * 1024);
  GI_LAUNCH_CHECK();
  fin.nb[5 + tap] = nb2;
  fin.inv[5 + tap] = 1.0 / (double)((int64_t)n * C * C);
  if (dgram) {
    hipLaunchKernelGGL(gram_delta_kernel, dim3(BLK * BLK / 256, ntile, n), dim3(256), 0, st, (const float*)gram, nb_, ntile, split, BLK, C,
                       (float)(1.0 / ((double)HW * C)), dgram, amax);
    GI_LAUNCH_CHECK();
  }
  if (split_out) *split_out = split;
  return GI_OK;
}
int finish_terms(hipStream_t st, const double* partial, const VggFinP& fin, float* per_tap, float weight_p, float weight_s, float* out2) {
  hipLaunchKernelGGL(vgg_finish_kernel, dim3(1), dim3(256), 0, st, partial, fin, per_tap, weight_p, weight_s, out2);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
// one pass of a tap's seed over n pairs: store = false: max |seed| into smax (maps of more than kSeedSampleAll blocks are sampled),
// store = true: s * seed over Ft
int seed_pass(hipStream_t st, bool store, const half_t* Fo, half_t* Ft, const float* dg, const unsigned* dmax, unsigned* smax, const float* sc, int n,
              int64_t HW, int C, float weight_p, float weight_s) {
  SeedP p;
  p.Fo = Fo; p.Ft = Ft; p.dg = dg; p.dmax = dmax; p.smax = smax; p.sc = sc;
  p.C = C; p.HW = (int)HW; p.nb = (int)((HW + 255) / 256);
  p.cp = (float)((double)weight_p * 2.0 / ((double)n * C * HW));
  p.cs = (float)((double)weight_s * 4.0 / ((double)n * C * C * (double)HW * C));
  const int nbx = !store && p.nb > kSeedSampleAll ? (p.nb + 7) / 8 : p.nb;      // the maximum pass samples large maps (vgg_seed_kernel)
  const dim3 grid(nbx, C / 64, n);
  if (!store) hipLaunchKernelGGL(vgg_seed_kernel<false>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(vgg_seed_kernel<true>, grid, dim3(256), 0, st, p);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // namespace

struct gi_vgg {
  gi_ctx* ctx;
  VggTrunk t;             // H, W, max_pairs; w1: conv1_1 summed weights [64][9]; the rest only with the grad workspace
  int64_t woff[NCONV], boff[NCONV];   // float offsets into params
  int64_t param_floats;
  const float* params;
  // workspace carve-up
  char* ws;
  int64_t ws_bytes;
  half_t* act[2];
  half_t* wpk[NCONV];     // [1..12] packed fp16 weights
  float* gram;            // partial Gram tiles (gram2_kernel): gram_bytes
  int64_t gram_bytes;
  double* partial;        // [10 terms][1024] doubles
  VggFinP fin;            // per term: partial count and 1 / element count (filled by vgg_run)
  float* per_tap;         // 10 floats
  bool bound, synced;
  // opt-in backward (gi_vgg19_bind_grad): a separate workspace; a handle that never binds it runs exactly as before
  char* gws;
  int64_t gws_bytes;
  bool gbound;
  int grad_n;             // pairs of the last grad call (0: none yet): gi_vgg19_grad_layer replays its backward
  float* dgram[5];        // per tap: dense G_o - G_t, [pairs][C][C] fp32
  unsigned* amax;         // [0..4] max |G_o - G_t| per tap, [5] max |seed| over the taps (bit patterns of non-negative floats)
  float* sc;              // [0] = s = 2^k, [1] = 1 / s (t.inv, stride 0): the backward runs on s * gradient
};

namespace {

// grad workspace: the trunk's arenas, transposed weights and gradient buffers (the [output half | target half] maps of trunk_gws_layout),
// then the dense Gram differences and the two small arrays of the seeds
int64_t vgg_gws_layout(gi_vgg* v, char* base) {
  WsTake take{base, 0};
  trunk_gws_layout(v->t, take);
  const int tapC[5] = {64, 128, 256, 512, 512};
  for (int t = 0; t < 5; ++t) v->dgram[t] = (float*)take((int64_t)v->t.max_pairs * tapC[t] * tapC[t] * 4);
  v->amax = (unsigned*)take(256);
  v->sc = (float*)take(256);
  v->t.inv = v->sc ? v->sc + 1 : nullptr;
  v->t.inv_stride = 0;
  return take.off;
}

int64_t vgg_ws_layout(gi_vgg* v, char* base) {
  WsTake take{base, 0};
  const int64_t act_bytes = (int64_t)2 * v->t.max_pairs * v->t.H * v->t.W * 64 * 2;
  v->act[0] = (half_t*)take(act_bytes);
  v->act[1] = (half_t*)take(act_bytes);
  v->wpk[0] = nullptr;
  for (int i = 1; i < NCONV; ++i) v->wpk[i] = (half_t*)take((int64_t)kCout[i] * 9 * kCin[i] * 2);
  v->t.w1 = (float*)take(64 * 9 * 4);
  v->gram_bytes = (int64_t)2 * v->t.max_pairs * 10 * 65536;          // one split of the widest tap (ten 128 x 128 tiles per image)
  if (v->gram_bytes < (32ll << 20)) v->gram_bytes = 32ll << 20;
  v->gram = (float*)take(v->gram_bytes);
  v->partial = (double*)take(10 * 1024 * 8);
  v->per_tap = (float*)take(64);
  return take.off;
}

// grad: every layer writes its own map in the grad workspace (nothing is overwritten that the backward reads), the pooled layers keep
// their full-resolution map and pool in a separate pass, and every tap leaves its dense Gram difference behind
int vgg_run(gi_vgg* v, const float* xa, const float* xb, int n, int stop_tap, float* feat_out, bool grad = false) {
  hipStream_t st = v->ctx->stream;
  const int nimg = 2 * n;
  int H = v->t.H, W = v->t.W, cur = 0;
  half_t* curp = grad ? v->t.ga[0] : v->act[0];
  // (W % 16 == 0 and 2 n H W 64 < 2^31 are conditions of gi_vgg19_create)
  GI_TRY(conv1(st, xa, xb, n, H, W, v->t.w1, v->params + v->boff[0], curp));
  for (int i = 0; i < NCONV; ++i) {
    bool pooled = false;
    if (i > 0) {
      IgemmArgs a;
      half_t* outp = grad ? v->t.ga[i] : v->act[cur ^ 1];
      // the pooled layers (conv1_2, conv2_2, conv3_4, conv4_4) are never taps: where the kernel can, it stores the 2x2 max pool of
      // its tile and the full-resolution map is never written
      const int pool2 = (!grad && kPoolAfter[i] && kTapAfter[i] < 0) ? 1 : 0;
      GI_TRY(conv3x3(st, curp, v->wpk[i], outp, nimg, H, W, kCin[i], kCout[i], v->params + v->boff[i], GI_ACT_RELU, pool2, nullptr, nullptr, a));
      cur ^= 1;
      curp = outp;
      pooled = a.pool_applied != 0;
    }
    const int C = kCout[i];
    const int tap = kTapAfter[i];
    if (tap >= 0) {
      const half_t* F = curp;
      const int64_t HW = (int64_t)H * W;
      if (feat_out && tap == stop_tap) return nhwc_to_nchw(st, F, feat_out, n, (int)HW, C);
      if (!feat_out) {
        // perceptual term mean over (n, C, H, W) of (F_o - F_t)^2 and style term mean over (n, C, C) of (G_o - G_t)^2, G = F^T F / (HW C):
        // one pass over the tap's feature maps (gram2_kernel) + the fixed-order reduction of its partial tiles
        GI_TRY(tap_terms(st, F, n, HW, C, tap, v->gram, v->gram_bytes, v->partial, v->fin, grad ? v->dgram[tap] : nullptr, grad ? v->amax + tap : nullptr,
                         0, nullptr));
      }
    }
    if (kPoolAfter[i] && pooled) {
      H /= 2;
      W /= 2;
    } else if (kPoolAfter[i]) {
      GI_TRY(maxpool2(st, curp, grad ? v->t.gpool[i] : v->act[cur ^ 1], nimg, H / 2, W / 2, C));
      curp = grad ? v->t.gpool[i] : v->act[cur ^ 1];
      cur ^= 1;
      H /= 2;
      W /= 2;
    }
  }
  return GI_OK;
}

// seeds of the five taps from the maps and Gram differences the grad forward left: first their maximum, then s, then s * seed over F_t
int vgg_seeds(gi_vgg* v, int n, float weight_p, float weight_s) {
  hipStream_t st = v->ctx->stream;
  for (int pass = 0; pass < 2; ++pass) {
    int H = v->t.H, W = v->t.W;
    for (int i = 0; i < NCONV; ++i) {
      const int tap = kTapAfter[i], C = kCout[i];
      if (tap >= 0) {
        const int64_t HW = (int64_t)H * W;
        GI_TRY(seed_pass(st, pass == 1, v->t.ga[i], v->t.ga[i] + (int64_t)n * HW * C, v->dgram[tap], v->amax + tap, v->amax + 5, v->sc, n, HW, C, weight_p,
                         weight_s));
      }
      if (kPoolAfter[i]) { H /= 2; W /= 2; }
    }
    if (pass == 0) GI_TRY(seed_scale(st, v->amax + 5, v->sc, 1));
  }
  return GI_OK;
}

}  // namespace

extern "C" {

int gi_vgg19_create(gi_ctx* ctx, int H, int W, int max_pairs, gi_vgg** out) {
  GI_REQUIRE(ctx && out, "vgg19_create: null argument");
  GI_REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && max_pairs > 0, "vgg19_create: H=%d W=%d (multiples of 16) pairs=%d", H, W,
             max_pairs);
  GI_REQUIRE((int64_t)2 * max_pairs * H * W * 64 < (1ll << 31), "vgg19_create: 2*%d images of %dx%d exceed 32-bit activation offsets", max_pairs,
             H, W);
  gi_vgg* v = new (std::nothrow) gi_vgg();
  GI_REQUIRE(v, "vgg19_create: out of host memory");
  v->ctx = ctx;
  v->t.nconv = NCONV; v->t.cin = kCin; v->t.cout = kCout; v->t.tap_after = kTapAfter; v->t.pool_after = kPoolAfter;
  v->t.H = H; v->t.W = W; v->t.max_pairs = max_pairs;
  int64_t off = 0;
  for (int i = 0; i < NCONV; ++i) {
    v->woff[i] = off; off += (int64_t)kCout[i] * kCin[i] * 9;
    v->boff[i] = off; off += kCout[i];
  }
  v->param_floats = off;
  v->params = nullptr; v->ws = nullptr; v->bound = false; v->synced = false;
  v->gws = nullptr; v->gbound = false; v->grad_n = 0;
  v->gws_bytes = vgg_gws_layout(v, nullptr);
  v->ws_bytes = vgg_ws_layout(v, nullptr);
  *out = v;
  return GI_OK;
}
void gi_vgg19_destroy(gi_vgg* v) { delete v; }
int64_t gi_vgg19_param_floats(const gi_vgg* v) { return v ? v->param_floats : -1; }
int64_t gi_vgg19_workspace_bytes(const gi_vgg* v) { return v ? v->ws_bytes : -1; }
int gi_vgg19_num_tensors(const gi_vgg* v) { return v ? 2 * NCONV : -1; }

int gi_vgg19_tensor_desc(const gi_vgg* v, int index, char* name, int name_cap, int* shape4, int64_t* offset) {
  GI_REQUIRE(v && index >= 0 && index < 2 * NCONV && name && shape4 && offset, "vgg19_tensor_desc: bad argument");
  const int i = index / 2, is_bias = index & 1;
  snprintf(name, name_cap, "features.%d.%s", kFeatIdx[i], is_bias ? "bias" : "weight");
  if (is_bias) { shape4[0] = kCout[i]; shape4[1] = shape4[2] = shape4[3] = 0; *offset = v->boff[i]; }
  else { shape4[0] = kCout[i]; shape4[1] = kCin[i]; shape4[2] = shape4[3] = 3; *offset = v->woff[i]; }
  return GI_OK;
}

int gi_vgg19_bind(gi_vgg* v, const float* params, void* ws, int64_t ws_bytes) {
  GI_REQUIRE(v && params && ws, "vgg19_bind: null argument");
  GI_REQUIRE(ws_bytes >= v->ws_bytes && ((uintptr_t)ws & 255) == 0, "vgg19_bind: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)v->ws_bytes);
  v->params = params; v->ws = (char*)ws;
  vgg_ws_layout(v, v->ws);
  v->bound = true; v->synced = false;
  return GI_OK;
}

int gi_vgg19_sync_weights(gi_vgg* v) {
  GI_REQUIRE(v && v->bound, "vgg19_sync_weights: not bound");
  hipStream_t st = v->ctx->stream;
  GI_TRY(sum_cin(st, v->params + v->woff[0], v->t.w1));
  for (int i = 1; i < NCONV; ++i) GI_TRY(pack3x3(st, false, v->params + v->woff[i], v->wpk[i], kCout[i], kCin[i]));
  if (v->gbound) {     // the transposed convolutions' weights, only for a handle that can run the backward
    for (int i = 1; i < NCONV; ++i) GI_TRY(pack3x3(st, true, v->params + v->woff[i], v->t.wT[i], kCout[i], kCin[i]));
  }
  v->synced = true;
  return GI_OK;
}

int gi_vgg19_perceptual_style(gi_vgg* v, const float* output, const float* target, int n, float weight_p, float weight_s, float* out2,
                              float* per_tap10) {
  GI_REQUIRE(v && v->bound && v->synced, "vgg19_perceptual_style: bind + sync_weights first");
  GI_REQUIRE(output && target && out2 && n > 0 && n <= v->t.max_pairs, "vgg19_perceptual_style: n=%d (max %d)", n, v->t.max_pairs);
  GI_TRY(vgg_run(v, output, target, n, -1, nullptr));
  GI_TRY(finish_terms(v->ctx->stream, v->partial, v->fin, v->per_tap, weight_p, weight_s, out2));
  if (per_tap10) GI_HIP(hipMemcpyAsync(per_tap10, v->per_tap, 10 * sizeof(float), hipMemcpyDeviceToDevice, v->ctx->stream));
  return GI_OK;
}

int64_t gi_vgg19_grad_workspace_bytes(const gi_vgg* v) { return v ? v->gws_bytes : -1; }

int gi_vgg19_bind_grad(gi_vgg* v, void* ws, int64_t ws_bytes) {
  GI_REQUIRE(v && ws, "vgg19_bind_grad: null argument");
  GI_REQUIRE(v->bound, "vgg19_bind_grad: gi_vgg19_bind first");
  GI_REQUIRE(ws_bytes >= v->gws_bytes && ((uintptr_t)ws & 255) == 0, "vgg19_bind_grad: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)v->gws_bytes);
  v->gws = (char*)ws;
  vgg_gws_layout(v, v->gws);
  v->gbound = true; v->synced = false; v->grad_n = 0;      // sync_weights packs the transposed weights
  return GI_OK;
}

int gi_vgg19_perceptual_style_grad(gi_vgg* v, const float* output, const float* target, int n, float weight_p, float weight_s, float* out2,
                                   float* per_tap10, float* grad_out, float gscale) {
  GI_REQUIRE(v && v->gbound, "vgg19_perceptual_style_grad: no grad workspace bound (gi_vgg19_bind_grad)");
  GI_REQUIRE(v->bound && v->synced, "vgg19_perceptual_style_grad: bind + sync_weights first");
  GI_REQUIRE(output && target && out2 && grad_out && n > 0 && n <= v->t.max_pairs, "vgg19_perceptual_style_grad: n=%d (max %d)", n, v->t.max_pairs);
  hipStream_t st = v->ctx->stream;
  v->grad_n = 0;
  GI_HIP(hipMemsetAsync(v->amax, 0, 256, st));
  GI_TRY(vgg_run(v, output, target, n, -1, nullptr, true));
  GI_TRY(finish_terms(st, v->partial, v->fin, v->per_tap, weight_p, weight_s, out2));
  if (per_tap10) GI_HIP(hipMemcpyAsync(per_tap10, v->per_tap, 10 * sizeof(float), hipMemcpyDeviceToDevice, st));
  GI_TRY(vgg_seeds(v, n, weight_p, weight_s));
  v->grad_n = n;
  return trunk_backward(v->t, st, n, -1, nullptr, grad_out, gscale);
}

int gi_vgg19_grad_layer(gi_vgg* v, int layer, float* out_nchw) {
  GI_REQUIRE(v && v->gbound, "vgg19_grad_layer: no grad workspace bound (gi_vgg19_bind_grad)");
  GI_REQUIRE(v->synced && v->grad_n > 0, "vgg19_grad_layer: no gi_vgg19_perceptual_style_grad call to read back");
  GI_REQUIRE(out_nchw && layer >= 0 && layer < NCONV, "vgg19_grad_layer: layer=%d", layer);
  // replays the backward of the last grad call from what it left in the workspace (maps, seeds, scale), down to `layer`
  return trunk_backward(v->t, v->ctx->stream, v->grad_n, layer, out_nchw, nullptr, 1.f);
}

int gi_vgg19_features(gi_vgg* v, const float* x, int n, int tap, float* out_nchw) {
  GI_REQUIRE(v && v->bound && v->synced, "vgg19_features: bind + sync_weights first");
  GI_REQUIRE(x && out_nchw && n > 0 && n <= v->t.max_pairs && tap >= 0 && tap < 5, "vgg19_features: n=%d tap=%d", n, tap);
  // the runner works on 2n stacked images: feed x twice, return the first n
  GI_TRY(vgg_run(v, x, x, n, tap, out_nchw));
  return GI_OK;
}

// ---- the loss path's kernels one at a time (test seam; include/ganinpaint.h). Every entry checks what its kernel assumes and goes
// through the host launch code above; nothing here is on a training path ----------------------------------------------------------
#define GI_VGG_FITS31(count) ((int64_t)(count) > 0 && (int64_t)(count) < (1ll << 31))

int gi_debug_vgg_conv3x3(gi_ctx* ctx, const void* in, const float* w, void* w_packed, void* out, int n, int H, int W, int cin, int cout, int transposed,
                         const float* bias, int act_out, int pool2, const void* mask, const void* add, int* pool_applied, int* mask_applied) {
  GI_REQUIRE(ctx && in && w && w_packed && out && pool_applied && mask_applied, "debug_vgg_conv3x3: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && cin > 0 && cout > 0 && cin % 64 == 0 && cout % 64 == 0, "debug_vgg_conv3x3: n=%d H=%d W=%d cin=%d cout=%d (channels: multiples of 64)",
             n, H, W, cin, cout);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)n * H * W * (cin > cout ? cin : cout)) && GI_VGG_FITS31((int64_t)cin * 9 * cout), "debug_vgg_conv3x3: tensor beyond 32-bit offsets");
  GI_REQUIRE(act_out == GI_ACT_NONE || act_out == GI_ACT_RELU, "debug_vgg_conv3x3: act_out=%d", act_out);
  GI_REQUIRE(!pool2 || (H % 2 == 0 && W % 2 == 0), "debug_vgg_conv3x3: pool2 needs even H=%d W=%d", H, W);
  GI_REQUIRE(mask || !add, "debug_vgg_conv3x3: add without mask");
  hipStream_t st = ctx->stream;
  GI_TRY(pack3x3(st, transposed != 0, w, (half_t*)w_packed, cout, cin));
  IgemmArgs a;
  const int ci = transposed ? cout : cin, co = transposed ? cin : cout;     // the input gradient: the channel roles swap
  const int rc = conv3x3(st, (const half_t*)in, (const half_t*)w_packed, (half_t*)out, n, H, W, ci, co, bias, act_out, pool2 ? 1 : 0, (const half_t*)mask,
                         (const half_t*)add, a);
  if (rc == GI_ERR_UNSUPPORTED) gi_set_error("debug_vgg_conv3x3: no mode-2 kernel serves n=%d %dx%d %d->%d", n, H, W, ci, co);
  GI_TRY(rc);
  *pool_applied = a.pool_applied; *mask_applied = a.mask_applied;
  return GI_OK;
}

int gi_debug_vgg_conv1(gi_ctx* ctx, const float* xa, const float* xb, int n, int H, int W, const float* w, const float* bias, float* w1, void* out) {
  GI_REQUIRE(ctx && xa && xb && w && bias && w1 && out, "debug_vgg_conv1: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && W % 16 == 0, "debug_vgg_conv1: n=%d H=%d W=%d (W: a multiple of 16)", n, H, W);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)2 * n * H * W * 64), "debug_vgg_conv1: tensor beyond 32-bit offsets");
  GI_TRY(sum_cin(ctx->stream, w, w1));
  return conv1(ctx->stream, xa, xb, n, H, W, w1, bias, (half_t*)out);
}

int gi_debug_vgg_maxpool2(gi_ctx* ctx, const void* in, void* out, int nimg, int Ho, int Wo, int C) {
  GI_REQUIRE(ctx && in && out, "debug_vgg_maxpool2: null pointer");
  GI_REQUIRE(nimg > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 8 == 0, "debug_vgg_maxpool2: nimg=%d Ho=%d Wo=%d C=%d (C: a multiple of 8)", nimg, Ho, Wo, C);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)nimg * Ho * Wo * 4 * C), "debug_vgg_maxpool2: tensor beyond 32-bit offsets");
  return maxpool2(ctx->stream, (const half_t*)in, (half_t*)out, nimg, Ho, Wo, C);
}

int64_t gi_debug_vgg_tap_ws_bytes(void) { return 10 * 1024 * 8 + 256 + (32ll << 20); }

int gi_debug_vgg_tap_terms(gi_ctx* ctx, const void* F, int n, int HW, int C, int force_split, void* ws, int64_t ws_bytes, float* terms2, float* dg,
                           unsigned* amax, int* split_out) {
  GI_REQUIRE(ctx && F && ws && terms2 && split_out, "debug_vgg_tap_terms: null pointer");
  GI_REQUIRE((dg != nullptr) == (amax != nullptr), "debug_vgg_tap_terms: dg and amax go together");
  GI_REQUIRE(n > 0 && HW > 0 && (C == 64 || (C > 0 && C % 128 == 0)) && force_split >= 0, "debug_vgg_tap_terms: n=%d HW=%d C=%d (64 or a multiple of 128) split=%d", n, HW,
             C, force_split);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)2 * n * HW * C) && GI_VGG_FITS31((int64_t)n * C * C), "debug_vgg_tap_terms: tensor beyond 32-bit offsets");
  GI_REQUIRE(ws_bytes >= gi_debug_vgg_tap_ws_bytes() && ((uintptr_t)ws & 255) == 0, "debug_vgg_tap_terms: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)gi_debug_vgg_tap_ws_bytes());
  hipStream_t st = ctx->stream;
  double* partial = (double*)ws;                                  // [10 terms][1024], as gi_vgg's
  float* per_tap = (float*)((char*)ws + 10 * 1024 * 8);
  float* gram = (float*)((char*)ws + 10 * 1024 * 8 + 256);
  VggFinP fin = {};                                               // the other four taps: no partials, terms of zero
  if (amax) GI_HIP(hipMemsetAsync(amax, 0, 4, st));
  GI_TRY(tap_terms(st, (const half_t*)F, n, HW, C, 0, gram, ws_bytes - (10 * 1024 * 8 + 256), partial, fin, dg, amax, force_split, split_out));
  return finish_terms(st, partial, fin, per_tap, 1.f, 1.f, terms2);
}

int gi_debug_vgg_seed(gi_ctx* ctx, int store, const void* Fo, void* Ft, const float* dg, const unsigned* dmax, unsigned* smax, const float* sc, int n, int HW,
                      int C, float weight_p, float weight_s) {
  GI_REQUIRE(ctx && Fo && Ft && dg && dmax && (store ? sc != nullptr : smax != nullptr), "debug_vgg_seed: null pointer");
  GI_REQUIRE(n > 0 && HW > 0 && C > 0 && C % 64 == 0, "debug_vgg_seed: n=%d HW=%d C=%d (a multiple of 64)", n, HW, C);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)n * HW * C) && GI_VGG_FITS31((int64_t)n * C * C), "debug_vgg_seed: tensor beyond 32-bit offsets");
  return seed_pass(ctx->stream, store != 0, (const half_t*)Fo, (half_t*)Ft, dg, dmax, smax, sc, n, HW, C, weight_p, weight_s);
}

int gi_debug_vgg_scale(gi_ctx* ctx, const unsigned* smax, float* sc) {
  GI_REQUIRE(ctx && smax && sc, "debug_vgg_scale: null pointer");
  return seed_scale(ctx->stream, smax, sc, 1);
}

int gi_debug_vgg_act_bwd(gi_ctx* ctx, int pool, const void* g, const void* act, const void* seed, void* out, int n, int H, int W, int C, int relu) {
  GI_REQUIRE(ctx && act && out, "debug_vgg_act_bwd: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "debug_vgg_act_bwd: n=%d H=%d W=%d C=%d (C: a multiple of 8)", n, H, W, C);
  GI_REQUIRE(GI_VGG_FITS31((int64_t)n * H * W * C), "debug_vgg_act_bwd: tensor beyond 32-bit offsets");
  GI_REQUIRE(!pool || (g && !seed && out != g && H % 2 == 0 && W % 2 == 0), "debug_vgg_act_bwd: the pool form needs g, no seed, out apart from g and even H=%d W=%d",
             H, W);
  return act_bwd(ctx->stream, pool != 0, (const half_t*)g, (const half_t*)act, (const half_t*)seed, (half_t*)out, n, H, W, C, relu);
}

int gi_debug_vgg_conv1_adjoint(gi_ctx* ctx, const void* D, const float* w1, const float* sc, float gscale, float* dimg, int n, int H, int W) {
  GI_REQUIRE(ctx && D && w1 && sc && dimg, "debug_vgg_conv1_adjoint: null pointer");
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && GI_VGG_FITS31((int64_t)n * H * W * 64), "debug_vgg_conv1_adjoint: n=%d H=%d W=%d", n, H, W);
  return conv1_adjoint(ctx->stream, (const half_t*)D, w1, sc + 1, 0, gscale, dimg, n, H, W);
}

}  // extern "C"
