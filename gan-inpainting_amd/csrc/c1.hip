// HBM-bound kernels for the layers whose large-resolution side has ONE channel:
//   generator d1  Conv2d(1->ngf)            (lib/models/networks.py:285, outermost block :296)
//   generator u1  ConvTranspose2d(2ngf->1)  (networks.py:293-297) + bias + tanh
//   discriminator Conv2d(1->64)             (networks.py:337)
// and their gradients. Weights are fp32 [c][16] (= [a][ky][kx][b] with b == 1). The image side is
// the public fp32 (n,1,H,W) tensor, the feature side NHWC of type T.
// These layers carry <1% of the FLOPs and ~45% of the activation bytes, so they are written as
// vectorised streaming kernels (16-byte feature accesses, weights in registers/LDS), not GEMMs.
#include "common.h"
#include "stat_acc.h"
#include "bn_acc.h"

namespace {

__device__ __forceinline__ float act_f(float v, int act) {
  if (act == GI_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == GI_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
  return v;
}

// ---- gather: out[p][c] = act(sum_tap img[n,2y-1+ky,2x-1+kx] * w[c][tap]) ---------------------
// One thread per (pixel, 8-channel group): 16 image taps (L1 broadcast among the pixel's threads),
// weights staged TRANSPOSED in LDS (swT[tap][c]) so the 8 channels of a tap are two 16-byte reads and
// the lanes of a wave (consecutive groups) hit consecutive LDS slots; one 16-byte store per thread.
template <typename T>
__global__ void __launch_bounds__(256) c1_gather_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                        char* out, int n, int Hs, int Ws, int c, int ldout,
                                                        int coffout, int act, float in_scale, const float* __restrict__ bias) {
  constexpr int G = 8;  // channels per thread
  extern __shared__ __attribute__((aligned(16))) float swT[];  // [16][c]
  for (int i = threadIdx.x; i < c * 16; i += 256) swT[(i & 15) * c + (i >> 4)] = w[i];
  __syncthreads();
  const int groups = c / G;
  const int lg = 31 - __builtin_clz(groups);   // groups is a power of two
  const int64_t total = (int64_t)n * Hs * Ws * groups;
  const int H = 2 * Hs, W = 2 * Ws;
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    const int grp = (int)(gid & (groups - 1));
    const int64_t pix = gid >> lg;
    const int x = (int)(pix % Ws);
    const int64_t t = pix / Ws;
    const int y = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    const float* ip = img + (int64_t)nn * H * W;
    float o[G];
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = bias ? bias[grp * G + j] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const int iy = 2 * y - 1 + ky;
      const bool yok = iy >= 0 && iy < H;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int ix = 2 * x - 1 + kx;
        const float v = (yok && ix >= 0 && ix < W) ? ip[(int64_t)iy * W + ix] * in_scale : 0.f;
        const float* wr = swT + (ky * 4 + kx) * c + grp * G;
        const f4_t w0 = *(const f4_t*)wr, w1 = *(const f4_t*)(wr + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = fmaf(v, w0[j], o[j]); o[4 + j] = fmaf(v, w1[j], o[4 + j]); }
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = act_f(o[j], act);
    T* dst = (T*)(out + (pix * ldout + coffout + grp * G) * (int64_t)sizeof(T));
    if constexpr (std::is_same<T, half_t>::value) {
      h8_t h;
#pragma unroll
      for (int j = 0; j < G; ++j) h[j] = (half_t)o[j];
      *(h8_t*)dst = h;
    } else {
      *(f4_t*)dst = f4_t{o[0], o[1], o[2], o[3]};
      *(f4_t*)(dst + 4) = f4_t{o[4], o[5], o[6], o[7]};
    }
  }
}

// Strip form of the gather (used when a row of Ws pixels splits evenly into strips of 256/groups
// pixels): a block walks strips; the 4 x (2S+2) image window of a strip is staged once in LDS
// (double-buffered, one barrier per strip) instead of 16 bounds-checked global loads per thread.
template <typename T>
__global__ void __launch_bounds__(256) c1_gather_strip_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                              char* out, int n, int Hs, int Ws, int c, int ldout,
                                                              int coffout, int act, float in_scale, const float* __restrict__ bias) {
  constexpr int G = 8;
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  const int groups = c / G;
  const int S = 256 / groups;            // pixels per strip
  const int TW = 2 * S + 2;              // staged columns
  float* swT = smem_f;                   // [16][c]
  float* tile = smem_f + 16 * c;         // [2][4][TW]
  for (int i = threadIdx.x; i < c * 16; i += 256) swT[(i & 15) * c + (i >> 4)] = w[i];
  const int H = 2 * Hs, W = 2 * Ws;
  const int spr = Ws / S;                                  // strips per row
  const int64_t nstrips = (int64_t)n * Hs * spr;
  const int grp = threadIdx.x % groups, pi = threadIdx.x / groups;
  auto stage = [&](int64_t strip, int buf) {
    const int sx = (int)(strip % spr);
    const int64_t t = strip / spr;
    const int y = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    const float* ip = img + (int64_t)nn * H * W;
    for (int idx = threadIdx.x; idx < 4 * TW; idx += 256) {
      const int r = idx / TW, cc = idx % TW;
      const int iy = 2 * y - 1 + r, ix = 2 * sx * S - 1 + cc;
      tile[(buf * 4 + r) * TW + cc] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? ip[(int64_t)iy * W + ix] * in_scale : 0.f;
    }
  };
  int buf = 0;
  int64_t strip = blockIdx.x;
  if (strip < nstrips) stage(strip, 0);
  __syncthreads();
  for (; strip < nstrips; strip += gridDim.x) {
    const int64_t next = strip + gridDim.x;
    if (next < nstrips) stage(next, buf ^ 1);
    const float* tl = tile + buf * 4 * TW + 2 * pi;
    float o[G];
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = bias ? bias[grp * G + j] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const float v = tl[ky * TW + kx];
        const float* wr = swT + (ky * 4 + kx) * c + grp * G;
        const f4_t w0 = *(const f4_t*)wr, w1 = *(const f4_t*)(wr + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = fmaf(v, w0[j], o[j]); o[4 + j] = fmaf(v, w1[j], o[4 + j]); }
      }
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = act_f(o[j], act);
    const int64_t pix = strip * S + pi;      // strips enumerate pixels in (n, y, x) order
    T* dst = (T*)(out + (pix * ldout + coffout + grp * G) * (int64_t)sizeof(T));
    if constexpr (std::is_same<T, half_t>::value) {
      h8_t h;
#pragma unroll
      for (int j = 0; j < G; ++j) h[j] = (half_t)o[j];
      *(h8_t*)dst = h;
    } else {
      *(f4_t*)dst = f4_t{o[0], o[1], o[2], o[3]};
      *(f4_t*)(dst + 4) = f4_t{o[4], o[5], o[6], o[7]};
    }
    __syncthreads();
    buf ^= 1;
  }
}

// ---- fp16 gather on the matrix cores ---------------------------------------------------------------
// out[p][c] = act(sum_tap G[p][tap] * w[c][tap]) as D[c][pixel] = A[c][tap] * B[tap][pixel], K = 16 taps = one
// v_mfma_f32_16x16x16_f16: the weights (A) live in registers, each wave gathers the 16 taps of 16 consecutive pixels of
// one image row - lane (pixel lr, k-chunk kq) holds tap row ky = kq, i.e. the four image columns 2x-1 .. 2x+2 of image row
// 2y-1+kq: one 8-byte load for the aligned middle pair and two single loads, from clamped addresses with the padding
// zeroed by selects (no divergent branches; the group index is wave-uniform, so the (image, row, column) split is
// scalar 32-bit arithmetic). Every lane ends with 4 consecutive channels of its pixel per 16-channel tile.
// The first form of this kernel (K padded to 32, half the lanes loading 8 taps behind per-tap bounds branches, 64-bit
// divisions per group) spent 22 of its 39 us on the critic's conv1 in address arithmetic, measured with loads and stores
// switched off; the layer is 134 MB of stores.
// (Measured and dropped in round 4: the same launch also writing the copy of the image that the generator keeps for d1's weight
//  gradient - lanes kq = 1, 2 hold exactly the 2 x 2 input pixels under their output pixel - made this store-bound kernel 5.6 us
//  slower, what the separate 8.4 MB device copy costs; the copy now rides in a latency-bound pass instead: bn_apply's side copy.)
template <int MTC, int ACT>   // MTC = c / 16
__global__ void __launch_bounds__(256) c1_gather_mfma_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                             char* out, int n, int Hs, int Ws, int ldout, int coffout,
                                                             float in_scale, unsigned long long* __restrict__ bits) {
  __shared__ __attribute__((aligned(16))) char slab[4][2048];   // a wave's 16 pixels x 128 bytes, re-read pixel-major for the stores
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, kq = lane >> 4;
  // A[row lr of tile mt][k = 4*kq + j] = w[ch][tap 4*kq + j] with
  //   ch(mt, lr) = (mt >> 2) * 64 + ((mt >> 1) & 1) * 32 + (lr >> 2) * 8 + (mt & 1) * 4 + (lr & 3)
  // D row i of a tile lands in lane group kq = i >> 2, register r = i & 3, so after tiles 0,1 a lane owns the 8
  // consecutive channels kq * 8 .. + 7 of its pixel's first 32 and after tiles 2,3 those of the second 32 (the 16-byte
  // chunks kq and 4 + kq of the pixel's 128-byte row, staged through LDS below).
  h4_t af[MTC];
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) {
    const int ch = (mt >> 2) * 64 + ((mt >> 1) & 1) * 32 + (lr >> 2) * 8 + (mt & 1) * 4 + (lr & 3);
    const f4_t v = *(const f4_t*)(w + ch * 16 + kq * 4);
    af[mt] = h4_t{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
  }
  const int H = 2 * Hs, W = 2 * Ws;
  const int gpr = Ws >> 4;                       // groups per small-grid row (Ws % 16 == 0)
  const int ngroups = n * Hs * gpr;              // < 2^31 (checked by the host)
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256 + threadIdx.x) >> 6));
  const int nwaves = (int)gridDim.x * 4;
  auto load_b = [&](int g, float (&bv)[4]) {
    const int rowi = g / gpr;                    // wave-uniform
    const int x = (g - rowi * gpr) * 16 + lr;
    const int nn = rowi / Hs, y = rowi - nn * Hs;
    const int iy = 2 * y - 1 + kq;
    const bool rok = iy >= 0 && iy < H;
    const float* rp = img + ((int64_t)nn * H + (rok ? iy : 0)) * W;
    const int ix0 = 2 * x - 1;                   // -1 only at x = 0; ix0 + 3 = W only at x = Ws - 1
    const float a0 = rp[ix0 < 0 ? 0 : ix0];
    const float2 mid = *(const float2*)(rp + ix0 + 1);
    const float a3 = rp[ix0 + 3 < W ? ix0 + 3 : W - 1];
    bv[0] = (rok && ix0 >= 0) ? a0 : 0.f;
    bv[1] = rok ? mid.x : 0.f;
    bv[2] = rok ? mid.y : 0.f;
    bv[3] = (rok && ix0 + 3 < W) ? a3 : 0.f;
  };
  float bv[4], bn[4];
  int g = wave;
  if (g < ngroups) load_b(g, bv);
  for (; g < ngroups; g += nwaves) {
    if (g + nwaves < ngroups) load_b(g + nwaves, bn);
    const h4_t bf = {(half_t)(bv[0] * in_scale), (half_t)(bv[1] * in_scale), (half_t)(bv[2] * in_scale), (half_t)(bv[3] * in_scale)};
#pragma unroll
    for (int mq = 0; mq < MTC / 4; ++mq) {
      h8_t o[2];
#pragma unroll
      for (int m4 = 0; m4 < 4; ++m4) {
        f4_t acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(af[mq * 4 + m4], bf, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[r];
          if (ACT == GI_ACT_RELU) v = fmaxf(v, 0.f);
          if (ACT == GI_ACT_LRELU) v = fmaxf(v, 0.2f * v);      // = v > 0 ? v : 0.2 v
          o[m4 >> 1][(m4 & 1) * 4 + r] = (half_t)v;
        }
      }
      if (MTC == 4 && bits) {
        // sign word of the pixel (bit c = [out[p][c] > 0], 64 channels): what the fused activation backward of the next layer's
        // input-gradient GEMM needs of this tensor (IgemmArgs::mask_bits: 8 bytes per pixel instead of 128). Lane (lr, kq) holds
        // channels 8 kq .. + 7 and 32 + 8 kq .. + 7 of pixel lr; the four kq lanes of a pixel are 16 lanes apart.
        typedef short s8_t __attribute__((ext_vector_type(8)));
        const s8_t s0 = __builtin_bit_cast(s8_t, o[0]), s1 = __builtin_bit_cast(s8_t, o[1]);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { lo |= (s0[j] > 0 ? 1u : 0u) << j; hi |= (s1[j] > 0 ? 1u : 0u) << j; }
        lo <<= 8 * kq; hi <<= 8 * kq;
        // OR over the four 16-lane rows: v_permlane16_swap / v_permlane32_swap (gfx950) pair the rows in registers, no LDS crossbar
        typedef unsigned u2v_t __attribute__((ext_vector_type(2)));
        u2v_t t = __builtin_amdgcn_permlane16_swap(lo, lo, false, false); lo = t[0] | t[1];
        t = __builtin_amdgcn_permlane16_swap(hi, hi, false, false); hi = t[0] | t[1];
        t = __builtin_amdgcn_permlane32_swap(lo, lo, false, false); lo = t[0] | t[1];
        t = __builtin_amdgcn_permlane32_swap(hi, hi, false, false); hi = t[0] | t[1];
        if (kq == 0) bits[(int64_t)g * 16 + lr] = (unsigned long long)lo | ((unsigned long long)hi << 32);
      }
      {
        // through a wave-private LDS slab so that one store instruction covers whole 128-byte pixel rows (8 pixels each; measured
        // against two 64-byte pieces per pixel and instruction: d1 17.6 -> 16.2 us, critic conv1 30.4 -> 30.0): pixel lr's 16-byte
        // chunk q at physical chunk q ^ (lr & 7); lane l reads chunk l & 7 of pixels l >> 3 and (l >> 3) + 8
        char* my = slab[threadIdx.x >> 6];
        __builtin_amdgcn_wave_barrier();
        *(h8_t*)(my + lr * 128 + ((kq ^ (lr & 7)) << 4)) = o[0];
        *(h8_t*)(my + lr * 128 + (((4 + kq) ^ (lr & 7)) << 4)) = o[1];
        __builtin_amdgcn_wave_barrier();
        const int p0 = lane >> 3, q = lane & 7;
        const h8_t v0 = *(const h8_t*)(my + p0 * 128 + ((q ^ (p0 & 7)) << 4));
        const h8_t v1 = *(const h8_t*)(my + (p0 + 8) * 128 + ((q ^ (p0 & 7)) << 4));
        char* d2 = out + ((((int64_t)g * 16 + p0) * ldout + coffout + mq * 64 + q * 8) << 1);
        *(h8_t*)d2 = v0;
        *(h8_t*)(d2 + (((int64_t)8 * ldout) << 1)) = v1;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = bn[j];
  }
}

// ---- the col step and the overlap-add, shared --------------------------------------------------------------------------------------
// One copy of what c1_col_kernel and c1_scatter_fused_kernel (the col step) and the three overlap-adding kernels share: the fused
// launch gives the bits of the two-launch form because it runs the same code. Lane (tapr, kq) = (lane & 15, lane >> 4): tapr is the A
// row (tap) and the B column (pixel of the group), kq the 8-channel chunk of a 32-channel K step.
// c1_col_load and c1_overlap_add return BY VALUE on purpose (through references the loads were scheduled worse).

// A fragments: af[ks][j] = w[channel ks * 32 + kq * 8 + j][tap tapr]
template <int KS>
__device__ __forceinline__ void c1_col_afrag(const float* w, int tapr, int kq, h8_t (&af)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) af[ks][j] = (half_t)w[(ks * 32 + kq * 8 + j) * 16 + tapr];
}

// raw B operand of pixel pix, K step ks: this lane's 16-byte piece, from X2 for the upper half of the channels when there is one; zeros
// where the pixel is not live (no load)
template <int KS>
__device__ __forceinline__ h8_t c1_col_load(const char* X, const char* X2, int64_t pix, bool live, int ldx, int coffx, int ld2, int kq, int ks) {
  constexpr int KH = KS / 2;
  const h8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  if (X2 && ks >= KH) return live ? *(const h8_t*)(X2 + ((pix * ld2 + (ks - KH) * 32 + kq * 8) << 1)) : zero;
  return live ? *(const h8_t*)(X + ((pix * ldx + coffx + ks * 32 + kq * 8) << 1)) : zero;
}

// s2 / h2 of this lane's upper-half channels: from sc2 / sh2, or (use_fa) derived by every workgroup from the layer's exact accumulators
// into aff ([2][KH * 32] floats of LDS); workgroup 0 publishes them and clears the layer's other accumulator region. Called by ALL threads
// of the workgroup under kernel-uniform conditions only: the use_fa side holds a __syncthreads().
// aff MUST point into LDS (the callers cast their __shared__ array / dynamic-LDS tail): typed so, its reads stay LDS reads
typedef __attribute__((address_space(3))) float lds_float_t;
template <int KH>
__device__ __forceinline__ void c1_upper_coefs(lds_float_t* aff, const BnAccP& fa, int use_fa, const float* sc2, const float* sh2, int kq,
                                               float (&s2)[KH][8], float (&h2)[KH][8]) {
  if (use_fa) {
    if (threadIdx.x < KH * 32) {
      float a, b;
      bn_from_acc(fa, KH * 32, threadIdx.x, 0, blockIdx.x == 0, a, b);
      aff[threadIdx.x] = a;
      aff[KH * 32 + threadIdx.x] = b;
    }
    if (blockIdx.x == 0 && fa.zero_next) zero_words64(fa.zero_next, fa.zero_words);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KH; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) { s2[ks][j] = aff[ks * 32 + kq * 8 + j]; h2[ks][j] = aff[KH * 32 + ks * 32 + kq * 8 + j]; }
  } else {
#pragma unroll
    for (int ks = 0; ks < KH; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) { s2[ks][j] = sc2[ks * 32 + kq * 8 + j]; h2[ks][j] = sh2[ks * 32 + kq * 8 + j]; }
  }
}

// the upper-half transform of 8 channels: relu(fma(x, s, h)) in fp32, ONE rounding to fp16 (the separate apply pass's expression).
// Also the X2 side of c1_wgrad_mfma_kernel.
__device__ __forceinline__ h8_t c1_upper8(h8_t raw, const float (&s)[8], const float (&h)[8]) {
  h8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = fmaf((float)raw[j], s[j], h[j]);
    o[j] = (half_t)(t > 0.f ? t : 0.f);
  }
  return o;
}

// B fragments from the raw pieces: lower half relu?(x), upper half (has_x2) through c1_upper8, zero where the pixel is not live (raw is
// zero there, relu(fma(0, s, h)) is not)
template <int KS>
__device__ __forceinline__ void c1_col_bfrag(const h8_t (&raw)[KS], bool has_x2, int relu_in, bool live, const float (&s2)[KS / 2][8],
                                             const float (&h2)[KS / 2][8], h8_t (&bf)[KS]) {
  constexpr int KH = KS / 2;
  const h8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (has_x2 && ks >= KH) {
      const h8_t u = c1_upper8(raw[ks], s2[ks >= KH ? ks - KH : 0], h2[ks >= KH ? ks - KH : 0]);
      bf[ks] = live ? u : zero;
    } else {
      bf[ks] = raw[ks];
      if (relu_in) bf[ks] = __builtin_elementwise_max(bf[ks], zero);
    }
  }
}

// Overlap-add of the 16 taps for the output quad (2j .. 2j+1, 2i .. 2i+1) of small-grid pixel (j, i):
//   o[py * 2 + px] = sum_{ty,tx} col[(j+py-ty, i+px-tx)][(1-py+2ty)*4 + 1-px+2tx]
// colrow(sy, sx) returns the 16 taps of the col row of pixel (sy, sx), 8-byte aligned. The ORDER of the additions is part of the contract
// (the fused launch and the two-launch form give equal bits): neighbours dy = -1, 0, 1 outermost, then dx = -1, 0, 1, then py, then px,
// every o[] starting from 0.f.
// A tap is taken out of the aligned 8-byte word of its tap row (taps 4r .. 4r + 3): no 4-byte load at a 2-byte-aligned address.
template <typename F>
__device__ __forceinline__ f4_t c1_overlap_add(F&& colrow, int j, int i, int Hs, int Ws) {
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int sy = j + dy, sx = i + dx;
      if (sy < 0 || sy >= Hs || sx < 0 || sx >= Ws) continue;
      const uint64_t* rows = (const uint64_t*)colrow(sy, sx);
#pragma unroll
      for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const int ty = py - dy, tx = px - dx;
          if (ty < 0 || ty > 1 || tx < 0 || tx > 1) continue;
          const int tap = (1 - py + 2 * ty) * 4 + (1 - px + 2 * tx);
          o[py * 2 + px] += (float)__builtin_bit_cast(half_t, (unsigned short)(rows[tap >> 2] >> (16 * (tap & 3))));
        }
    }
  return f4_t{o[0], o[1], o[2], o[3]};
}

// the quad's two rows: post(o + b) [* out_scale when SCALED] as one float2 each at image row row0 + py, column 2i, to img and (the
// caller's copy of the saved output) img2
template <bool SCALED>
__device__ __forceinline__ void c1_store_quad(f4_t o, float b, int post, float* img, float* img2, int64_t row0, int W, int i,
                                              float out_scale = 1.f) {
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    float v0 = o[py * 2] + b, v1 = o[py * 2 + 1] + b;
    if (post == 1) { v0 = tanhf(v0); v1 = tanhf(v1); }
    const int64_t oo = (row0 + py) * W + 2 * i;
    if constexpr (SCALED) {
      *(float2*)(img + oo) = make_float2(v0 * out_scale, v1 * out_scale);
      if (img2) *(float2*)(img2 + oo) = make_float2(v0 * out_scale, v1 * out_scale);
    } else {
      *(float2*)(img + oo) = make_float2(v0, v1);
      if (img2) *(float2*)(img2 + oo) = make_float2(v0, v1);
    }
  }
}

// ---- fp16 transposed conv to one channel on the matrix cores -------------------------------------
// col[p][tap] = sum_c relu?(X[p][c]) * w[c][tap]: D[tap][pixel] = A[tap][c] * B[c][pixel] with
// v_mfma_f32_16x16x32_f16; B fragments are 16-byte row loads of X straight from global memory (each
// lane: 8 consecutive channels of its pixel), A fragments (the 16 x c weights) live in registers.
// Each lane ends with 4 consecutive taps of one pixel -> one 8-byte store; a wave writes 512 B.
// X2 != null: channels [c/2, c) are not read from X but produced on the fly as relu(fma(X2[p][ch - c/2], sc2, sh2)),
// the BatchNorm + ReLU of the raw decoder output X2 (dense, ld2): the same fp32 expression and fp16 rounding as the
// separate apply pass, which then never has to materialise that half of the concat buffer.
// use_fa: sc2 / sh2 do not exist yet - every workgroup derives them from the layer's exact accumulators (bn_acc.h) into LDS while
// its first rows are in flight, workgroup 0 publishes them with the backward's vectors and moves the running statistics (the
// bn_finalize_acc launch between the GEMM and this kernel, 5 us behind a dependent launch, is gone).
template <int KS>   // KS = c / 32
__global__ void __launch_bounds__(256) c1_col_kernel(const char* X, const float* __restrict__ w, half_t* col,
                                                     int64_t P, int ldx, int coffx, int relu_in, const char* X2, int ld2,
                                                     const float* __restrict__ sc2, const float* __restrict__ sh2, BnAccP fa, int use_fa) {
  constexpr int KH = KS / 2;
  __shared__ float aff[2 * KH * 32];
  const int lane = threadIdx.x & 63;
  const int tapr = lane & 15, kq = lane >> 4;
  const int64_t ngroups = (P + 15) / 16;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
  // a wave walks 4+ groups: the next group's 16-byte row pieces are requested before this group's are used
  auto load_g = [&](int64_t g, h8_t (&raw)[KS]) {
    const int64_t pix = g * 16 + tapr;   // this lane's B column = pixel
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) raw[ks] = c1_col_load<KS>(X, X2, pix, pix < P, ldx, coffx, ld2, kq, ks);
  };
  h8_t raw[KS], nxt[KS];
  int64_t g = wave;
  if (g < ngroups) load_g(g, raw);
  h8_t af[KS];
  c1_col_afrag<KS>(w, tapr, kq, af);
  float s2[KH][8], h2[KH][8];
  if (X2) c1_upper_coefs<KH>((lds_float_t*)aff, fa, use_fa, sc2, sh2, kq, s2, h2);
  for (; g < ngroups; g += nwaves) {
    if (g + nwaves < ngroups) load_g(g + nwaves, nxt);
    const int64_t pix = g * 16 + tapr;
    const bool live = pix < P;
    h8_t bf[KS];
    c1_col_bfrag<KS>(raw, X2 != nullptr, relu_in, live, s2, h2, bf);
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks], bf[ks], acc, 0, 0, 0);
    if (live) {
      h4_t o = {(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
      *(h4_t*)(col + pix * 16 + kq * 4) = o;   // taps 4kq..4kq+3 of this pixel
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) raw[ks] = nxt[ks];
  }
}

// overlap-add of the col tensor (c1_overlap_add), bias, tanh (post = 1), out_scale: one thread per small-grid pixel
__global__ void __launch_bounds__(256) c1_col2im_kernel(const half_t* __restrict__ col, const float* __restrict__ bias,
                                                        float* img, float* img2, int n, int Hs, int Ws, int post, float out_scale) {
  const int64_t total = (int64_t)n * Hs * Ws;
  const int H = 2 * Hs, W = 2 * Ws;
  const float b = bias ? bias[0] : 0.f;
  for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * 256) {
    const int i = (int)(pix % Ws);
    const int64_t t = pix / Ws;
    const int j = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    // (col rows are 32 bytes apart: 8-byte aligned, as c1_overlap_add needs)
    const f4_t o = c1_overlap_add([=](int sy, int sx) { return col + (((int64_t)nn * Hs + sy) * Ws + sx) * 16; }, j, i, Hs, Ws);
    c1_store_quad<true>(o, b, post, img, img2, (int64_t)nn * H + 2 * j, W, i, out_scale);
  }
}

// ---- the same two steps in ONE launch (round 4) ----------------------------------------------------------------------------
// A workgroup owns TH rows of one image of the small grid (all Ws columns, so only rows have a halo): it computes col[p][tap] for
// its TH + 2 rows on the MFMA with the pieces c1_col_kernel is made of, keeps them in LDS ((TH + 2) x Ws x 32 bytes) and overlap-adds its
// own TH rows with c1_overlap_add, as c1_col2im_kernel does - bit-identical output, the col tensor (16.8 MB written and re-read at the
// headline shape) and one launch gone; the price is (TH + 2) / TH of the input reads, the extra rows being the neighbour workgroup's
// (L2). u1 of the generator at 256x256, n = 32: 28.6 + 15.6 us -> see DESIGN.md.
template <int KS>   // KS = c / 32
__global__ void __launch_bounds__(256) c1_scatter_fused_kernel(const char* X, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* img, float* img2, int Hs, int Ws, int TH, int ldx, int coffx, int relu_in,
                                                               const char* X2, int ld2, const float* __restrict__ sc2,
                                                               const float* __restrict__ sh2, BnAccP fa, int use_fa, int post, float out_scale) {
  constexpr int KH = KS / 2;
  extern __shared__ __attribute__((aligned(16))) char smem_u1[];
  half_t* col = (half_t*)smem_u1;                              // [(TH + 2) * Ws][16]
  float* aff = (float*)(smem_u1 + (int64_t)(TH + 2) * Ws * 32);  // [2][KH * 32]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tapr = lane & 15, kq = lane >> 4;
  const int bands = (Hs + TH - 1) / TH;
  const int nn = blockIdx.x / bands, y0 = (blockIdx.x % bands) * TH;
  const int gpr = Ws >> 4, G = (TH + 2) * gpr;                 // pixel groups of 16 along a row
  // the row pieces of the next TWO groups of a wave are in flight (c1_col_kernel: one)
  auto load_g = [&](int g, h8_t (&raw)[KS]) {
    const int ry = g / gpr, x = (g - ry * gpr) * 16 + tapr, y = y0 - 1 + ry;
    const bool live = g < G && y >= 0 && y < Hs;
    const int64_t pix = ((int64_t)nn * Hs + (live ? y : 0)) * Ws + x;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) raw[ks] = c1_col_load<KS>(X, X2, pix, live, ldx, coffx, ld2, kq, ks);
  };
  h8_t raw[KS], nx1[KS], nx2[KS];
  int g = wave;
  load_g(g, raw);
  load_g(g + 4, nx1);
  h8_t af[KS];
  c1_col_afrag<KS>(w, tapr, kq, af);
  float s2[KH][8], h2[KH][8];
  if (X2) c1_upper_coefs<KH>((lds_float_t*)aff, fa, use_fa, sc2, sh2, kq, s2, h2);
  for (; g < G; g += 4) {
    load_g(g + 8, nx2);
    const int ry = g / gpr, x = (g - ry * gpr) * 16 + tapr, y = y0 - 1 + ry;
    const bool live = y >= 0 && y < Hs;
    h8_t bf[KS];
    c1_col_bfrag<KS>(raw, X2 != nullptr, relu_in, live, s2, h2, bf);
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks], bf[ks], acc, 0, 0, 0);
    const h4_t o = {(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};     // rows outside the image: zeros
    *(h4_t*)(col + ((int64_t)ry * Ws + x) * 16 + kq * 4) = o;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { raw[ks] = nx1[ks]; nx1[ks] = nx2[ks]; }
  }
  __syncthreads();
  const int H = 2 * Hs, W = 2 * Ws;
  const float b = bias ? bias[0] : 0.f;
  for (int p = threadIdx.x; p < TH * Ws; p += 256) {
    const int jl = p / Ws, i = p - jl * Ws, j = y0 + jl;
    if (j >= Hs) break;
    // band row 0 = y0 - 1; rows of 32 bytes in 16-byte aligned LDS: 8-byte aligned, as c1_overlap_add needs
    const f4_t o = c1_overlap_add([=](int sy, int sx) { return col + ((int64_t)(sy - y0 + 1) * Ws + sx) * 16; }, j, i, Hs, Ws);
    c1_store_quad<true>(o, b, post, img, img2, (int64_t)nn * H + 2 * j, W, i, out_scale);
  }
}

// ---- transposed conv to a FEW channels (the frozen face-parsing network's head: 4 classes) -------------------------------
// The same two steps with OC output channels: col[p][o*16 + tap] = sum_c relu?(X[p][c]) * w[c][tap][o] - a 16*OC-row GEMM, OC MFMA
// row tiles per 32-channel step on the same B fragments - and the overlap-add per channel. 2*P*c*16*OC FLOP instead of the
// 2*4*P*(4c)*64 of the general kernels on weights padded to 64 output channels (16x less for OC = 4).
template <int KS, int OC>   // KS = c / 32
__global__ void __launch_bounds__(256) c1_col_mc_kernel(const char* X, const float* __restrict__ w, half_t* col, int64_t P, int ldx,
                                                        int coffx, int relu_in) {
  const int lane = threadIdx.x & 63;
  const int tapr = lane & 15, kq = lane >> 4;
  h8_t af[OC][KS];
#pragma unroll
  for (int o = 0; o < OC; ++o)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) af[o][ks][j] = (half_t)w[((ks * 32 + kq * 8 + j) * 16 + tapr) * OC + o];
  const int64_t ngroups = (P + 15) / 16;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
  const h8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    const int64_t pix = g * 16 + tapr;
    const bool live = pix < P;
    h8_t bf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf[ks] = live ? *(const h8_t*)(X + ((pix * ldx + coffx + ks * 32 + kq * 8) << 1)) : zero;
      if (relu_in) bf[ks] = __builtin_elementwise_max(bf[ks], zero);
    }
#pragma unroll
    for (int o = 0; o < OC; ++o) {
      f4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[o][ks], bf[ks], acc, 0, 0, 0);
      if (live) {
        h4_t v = {(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
        *(h4_t*)(col + pix * (16 * OC) + o * 16 + kq * 4) = v;   // taps 4kq..4kq+3 of channel o
      }
    }
  }
}

// overlap-add per channel into (n, OC, H, W) fp32, bias + tanh (post = 1)
template <int OC>
__global__ void __launch_bounds__(256) c1_col2im_mc_kernel(const half_t* __restrict__ col, const float* __restrict__ bias, float* img,
                                                           float* img2, int n, int Hs, int Ws, int post) {
  const int64_t total = (int64_t)n * Hs * Ws * OC;
  const int H = 2 * Hs, W = 2 * Ws;
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int o = (int)(id % OC);            // (channel fastest: the OC lanes of a pixel read one 32*OC-byte col row)
    const int64_t pix = id / OC;
    const int i = (int)(pix % Ws);
    const int64_t t = pix / Ws;
    const int j = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    static_assert((16 * sizeof(half_t)) % 8 == 0, "c1_overlap_add reads 8-byte words of a channel's col row");
    const f4_t acc = c1_overlap_add([=](int sy, int sx) { return col + ((((int64_t)nn * Hs + sy) * Ws + sx) * OC + o) * 16; }, j, i, Hs, Ws);
    const float b = bias ? bias[o] : 0.f;
    c1_store_quad<false>(acc, b, post, img, img2, ((int64_t)nn * OC + o) * H + 2 * j, W, i);   // (no out_scale here: stored unscaled)
  }
}

// input gradient of that head: out[p][c] = sum_{o,tap} G[o][p's tap] * w[c][tap][o], G the (n, OC, H, W) fp32 gradient: the gather of
// c1_gather_mfma_kernel with K = 16*OC (OC = 4: two full 32-wide MFMA steps, k = o*16 + tap)
template <int MTC>   // c / 16; OC = 4
__global__ void __launch_bounds__(256) c1_gather_mc4_kernel(const float* __restrict__ img, const float* __restrict__ w, char* out, int n, int Hs,
                                                            int Ws, int ldout, int coffout) {
  constexpr int OC = 4;
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, kq = lane >> 4;
  // A[row lr of tile mt][k = 32 s + 8 kq + j] = w[ch][tap = 8 (kq & 1) + j][o = 2 s + (kq >> 1)], ch = 16 consecutive channels per lane (the mapping c1_gather_mfma_kernel used before its 64-byte store pieces)
  h8_t af[MTC][2];
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) {
    const int ch = (mt >> 2) * 64 + (lr >> 2) * 16 + (mt & 3) * 4 + (lr & 3);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) af[mt][s2][j] = (half_t)w[(ch * 16 + (kq & 1) * 8 + j) * OC + 2 * s2 + (kq >> 1)];
  }
  const int H = 2 * Hs, W = 2 * Ws;
  const int64_t ngroups = (int64_t)n * Hs * Ws / 16;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
  auto load_b = [&](int64_t g, float (&bv)[2][8]) {
    const int64_t p0 = g * 16;
    const int x = (int)(p0 % Ws) + lr;
    const int64_t rowi = p0 / Ws;
    const int y = (int)(rowi % Hs);
    const int nn = (int)(rowi / Hs);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const float* ip = img + ((int64_t)nn * OC + 2 * s2 + (kq >> 1)) * H * W;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int iy = 2 * y - 1 + 2 * (kq & 1) + (j >> 2), ix = 2 * x - 1 + (j & 3);
        bv[s2][j] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? ip[(int64_t)iy * W + ix] : 0.f;
      }
    }
  };
  float bv[2][8], bn[2][8];
  int64_t g = wave;
  if (g < ngroups) load_b(g, bv);
  for (; g < ngroups; g += nwaves) {
    if (g + nwaves < ngroups) load_b(g + nwaves, bn);     // the next group's 16 loads are in flight during this group's MFMAs and stores
    const int64_t p0 = g * 16;
    h8_t bf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) bf[s2][j] = (half_t)bv[s2][j];
    const int64_t pix = p0 + lr;
    char* dst = out + ((pix * ldout + coffout) << 1);
#pragma unroll
    for (int mq = 0; mq < MTC / 4; ++mq) {
      h8_t o[2];
#pragma unroll
      for (int m4 = 0; m4 < 4; ++m4) {
        f4_t acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mq * 4 + m4][0], bf[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mq * 4 + m4][1], bf[1], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[m4 >> 1][(m4 & 1) * 4 + r] = (half_t)acc[r];
      }
      *(h8_t*)(dst + ((mq * 64 + kq * 16) << 1)) = o[0];
      *(h8_t*)(dst + ((mq * 64 + kq * 16 + 8) << 1)) = o[1];
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[s2][j] = bn[s2][j];
  }
}

// ---- scatter (transposed conv to one channel), one lane group per small-resolution pixel ------
// The 2x2 output quad (2j..2j+1, 2i..2i+1) reads the 3x3 neighbourhood of (j,i):
//   out(2j+py, 2i+px) = sum_{ty,tx} X[j+py-ty][i+px-tx] . w[:, (1-py+2ty)*4 + (1-px+2tx)]
template <typename T>
__global__ void __launch_bounds__(256) c1_scatter_kernel(const char* X, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* img, int n, int Hs,
                                                         int Ws, int c, int ldx, int coffx, int relu_in, int post,
                                                         float out_scale) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int LPP = c / EPC;  // lanes per pixel (power of two <= 64)
  const int cl = threadIdx.x % LPP;
  float wr[16][EPC];  // this lane's weights
#pragma unroll
  for (int j = 0; j < EPC; ++j)
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) wr[tt][j] = w[(cl * EPC + j) * 16 + tt];
  const float b = bias ? bias[0] : 0.f;
  const int gpb = 256 / LPP;
  const int64_t total = (int64_t)n * Hs * Ws;
  const int H = 2 * Hs, W = 2 * Ws;
  const int64_t niter = (total + (int64_t)gridDim.x * gpb - 1) / ((int64_t)gridDim.x * gpb);
  for (int64_t it = 0; it < niter; ++it) {
    const int64_t pix = (it * gridDim.x + blockIdx.x) * gpb + threadIdx.x / LPP;
    const bool live = pix < total;
    const int i = live ? (int)(pix % Ws) : 0;
    const int64_t t = live ? pix / Ws : 0;
    const int j = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int sy = j + dy, sx = i + dx;
          if (sy < 0 || sy >= Hs || sx < 0 || sx >= Ws) continue;
          const char* src = X + ((((int64_t)nn * Hs + sy) * Ws + sx) * ldx + coffx + cl * EPC) * (int64_t)sizeof(T);
          float xv[EPC];
          if constexpr (std::is_same<T, half_t>::value) {
            const h8_t h = *(const h8_t*)src;
#pragma unroll
            for (int e = 0; e < EPC; ++e) xv[e] = (float)h[e];
          } else {
            const f4_t f = *(const f4_t*)src;
#pragma unroll
            for (int e = 0; e < EPC; ++e) xv[e] = f[e];
          }
          if (relu_in) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) xv[e] = xv[e] > 0.f ? xv[e] : 0.f;
          }
#pragma unroll
          for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
              const int ty = py - dy, tx = px - dx;  // source = (j+py-ty, i+px-tx)
              if (ty < 0 || ty > 1 || tx < 0 || tx > 1) continue;
              const int tap = (1 - py + 2 * ty) * 4 + (1 - px + 2 * tx);
              float s = 0.f;
#pragma unroll
              for (int e = 0; e < EPC; ++e) s = fmaf(xv[e], wr[tap][e], s);
              o[py * 2 + px] += s;
            }
        }
    }
    for (int off = LPP >> 1; off > 0; off >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] += __shfl_xor(o[q], off);
    }
    if (live && cl == 0) {
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        float v0 = o[py * 2] + b, v1 = o[py * 2 + 1] + b;
        if (post == 1) { v0 = tanhf(v0); v1 = tanhf(v1); }
        float2 r = make_float2(v0 * out_scale, v1 * out_scale);
        *(float2*)(img + ((int64_t)nn * H + 2 * j + py) * W + 2 * i) = r;
      }
    }
  }
}

// ---- weight gradient: dW[c][tap] += scale * sum_p relu?(X[p][c]) * img[n,2y-1+ky,2x-1+kx] ------
template <typename T>
__global__ void __launch_bounds__(256) c1_wgrad_kernel(const char* X, const float* __restrict__ img, float* dW, int n,
                                                       int Hs, int Ws, int c, int ldx, int coffx, int relu_in,
                                                       float scale, float img_scale, int pix_per_block, float* __restrict__ part) {
  // part != null: the block's sums go to part[block][c*16] and c1_wgrad_reduce_kernel adds the blocks in a fixed order (bit-reproducible,
  // and no queue at the atomic unit: 1024 blocks x 1024 float atomics on the same 64 lines took most of this kernel's 130 us)
  constexpr int EPC = 16 / (int)sizeof(T);
  extern __shared__ float sred[];  // [pl][c][4] per round
  const int LPP = c / EPC;
  const int cl = threadIdx.x % LPP, pl = threadIdx.x / LPP;
  const int gpb = 256 / LPP;
  const int64_t total = (int64_t)n * Hs * Ws;
  const int H = 2 * Hs, W = 2 * Ws;
  const int64_t p0 = (int64_t)blockIdx.x * pix_per_block;
  const int64_t p1 = min(total, p0 + pix_per_block);
  float acc[16][EPC];
#pragma unroll
  for (int tt = 0; tt < 16; ++tt)
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[tt][e] = 0.f;
  for (int64_t pix = p0 + pl; pix < p1; pix += gpb) {
    const int x = (int)(pix % Ws);
    const int64_t t = pix / Ws;
    const int y = (int)(t % Hs);
    const int nn = (int)(t / Hs);
    const char* src = X + (pix * ldx + coffx + cl * EPC) * (int64_t)sizeof(T);
    float xv[EPC];
    if constexpr (std::is_same<T, half_t>::value) {
      const h8_t h = *(const h8_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) xv[e] = (float)h[e];
    } else {
      const f4_t f = *(const f4_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) xv[e] = f[e];
    }
    if (relu_in) {
#pragma unroll
      for (int e = 0; e < EPC; ++e) xv[e] = xv[e] > 0.f ? xv[e] : 0.f;
    }
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        const int iy = 2 * y - 1 + ky, ix = 2 * x - 1 + kx;
        const float g = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[((int64_t)nn * H + iy) * W + ix] * img_scale : 0.f;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[ky * 4 + kx][e] = fmaf(xv[e], g, acc[ky * 4 + kx][e]);
      }
  }
  // block reduction over pixel lanes, 4 taps per round: sred[pl][c][4]
#pragma unroll
  for (int rnd = 0; rnd < 4; ++rnd) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPC; ++e)
#pragma unroll
      for (int q = 0; q < 4; ++q) sred[(pl * c + cl * EPC + e) * 4 + q] = acc[rnd * 4 + q][e];
    __syncthreads();
    for (int idx = threadIdx.x; idx < c * 4; idx += 256) {
      float s = 0.f;
      for (int k = 0; k < gpb; ++k) s += sred[k * c * 4 + idx];
      const int ch = idx >> 2, q = idx & 3;
      if (part) part[(int64_t)blockIdx.x * (c * 16) + ch * 16 + rnd * 4 + q] = s * scale;
      else atomicAdd(dW + ch * 16 + rnd * 4 + q, s * scale);
    }
  }
}

// ---- fp16 weight gradient of the single-channel layers on the matrix cores ------------------------
// dW[c][tap] += scale * sum_p relu?(X[p][c]) * img[n,2y-1+ky,2x-1+kx]:  D[tap][c] = A[tap][p] * B[p][c],
// K = pixels in tiles of 32 that lie in one image row (Ws % 32 == 0). Every wave works alone on its
// own K tiles: A fragments (16 taps x 8 pixels per lane) are gathered from the fp32 image, the X tile
// (32 pixels x c, pixel-major = K-major) is staged in a wave-private LDS slab and read with the
// transposing ds_read_b64_tr_b16; no block barrier. One float atomic per (c, tap) per wave at the end.
template <int NT>   // NT = c / 16
__global__ void __launch_bounds__(256) c1_wgrad_mfma_kernel(const char* X, const float* __restrict__ img, float* dW,
                                                            int n, int Hs, int Ws, int ldx, int coffx, int relu_in,
                                                            float scale, float img_scale, const char* X2, int ld2,
                                                            const float* __restrict__ sc2, const float* __restrict__ sh2, float* __restrict__ part) {
  constexpr int C = NT * 16;
  constexpr int LROW = C * 2 + 32;                  // padded LDS row: conflict-free transposing reads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* slab = smem + wave * (32 * LROW);
  const int tap = lane & 15, kq = lane >> 4;
  const int ky = tap >> 2, kx = tap & 3;
  const int H = 2 * Hs, W = 2 * Ws;
  const int64_t ntiles = (int64_t)n * Hs * Ws / 32;
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave, nw = (int64_t)gridDim.x * 4;
  constexpr int CPR = C * 2 / 16;                   // 16-byte chunks per X row
  constexpr int RPP = 64 / CPR;                     // rows per load pass
  constexpr int NP = 32 / RPP;
  const int xr = lane / CPR, xc = lane % CPR;
  f4_t acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f4_t{0.f, 0.f, 0.f, 0.f};
  const h8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const int g16 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;

  // X2 != null: the channel chunks of the upper half come from the raw decoder output through relu(fma(x, sc2, sh2))
  const bool upper = X2 != nullptr && xc * 8 >= C / 2;
  float s2[8], h2[8];
  if (upper) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { s2[j] = sc2[xc * 8 - C / 2 + j]; h2[j] = sh2[xc * 8 - C / 2 + j]; }
  }
  auto load_x = [&](int64_t t, u4_t (&xv)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t row = t * 32 + xr + RPP * i;
      xv[i] = upper ? *(const u4_t*)(X2 + ((row * ld2 + xc * 8 - C / 2) << 1)) : *(const u4_t*)(X + ((row * ldx + coffx) << 1) + xc * 16);
    }
  };
  auto load_a = [&](int64_t t64, float (&av)[8]) {   // 8 pixels x0 + 8*kq + j of the tile's image row, tap (ky,kx)
    // the tile index is wave-uniform and < 2^31 (host check): scalar 32-bit divisions; clamped addresses + selects, no branches
    const int t32 = __builtin_amdgcn_readfirstlane((int)t64);
    const int tpr = Ws >> 5;                      // tiles per small-grid row (Ws % 32 == 0)
    const int rowi = t32 / tpr;
    const int x0 = (t32 - rowi * tpr) * 32;
    const int nn = rowi / Hs, y = rowi - nn * Hs;
    const int iy = 2 * y - 1 + ky;
    const bool yok = iy >= 0 && iy < H;
    const float* ip = img + ((int64_t)nn * H + (yok ? iy : 0)) * W;
    const int ixb = 2 * (x0 + 8 * kq) - 1 + kx;   // -1 only for j = 0 at the row start, W only for j = 7 at the row end
    const float a0 = ip[ixb < 0 ? 0 : ixb];
    const float a7 = ip[ixb + 14 < W ? ixb + 14 : W - 1];
    av[0] = (yok && ixb >= 0) ? a0 : 0.f;
#pragma unroll
    for (int j = 1; j < 7; ++j) { const float a = ip[ixb + 2 * j]; av[j] = yok ? a : 0.f; }
    av[7] = (yok && ixb + 14 < W) ? a7 : 0.f;
  };
  u4_t xv[NP], xn[NP];
  float av[8], an[8];
  int64_t t = gw;
  if (t < ntiles) { load_x(t, xv); load_a(t, av); }
  for (; t < ntiles; t += nw) {
    const int64_t tn = t + nw;
    if (tn < ntiles) { load_x(tn, xn); load_a(tn, an); }   // next tile in flight during this one
    h8_t af;
#pragma unroll
    for (int j = 0; j < 8; ++j) af[j] = (half_t)(av[j] * img_scale);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      u4_t v = xv[i];
      if (upper) {
        v = __builtin_bit_cast(u4_t, c1_upper8(__builtin_bit_cast(h8_t, v), s2, h2));
      } else if (relu_in) {
        typedef short s8_t __attribute__((ext_vector_type(8)));
        s8_t hh = __builtin_bit_cast(s8_t, v);
        const s8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
        hh = __builtin_elementwise_max(hh, z);
        v = __builtin_bit_cast(u4_t, hh);
      }
      *(u4_t*)(slab + (xr + RPP * i) * LROW + xc * 16) = v;
    }
    // (wave-private slab: the LDS unit executes one wave's accesses in program order)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int ch = nt * 16 + 4 * tp;
      const char* b_lo = slab + (8 * g16 + tq) * LROW + ch * 2;
      const char* b_hi = slab + (8 * g16 + 4 + tq) * LROW + ch * 2;
      fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)b_lo);
      fp16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)b_hi);
      h4_t l4 = __builtin_bit_cast(h4_t, lo), h4 = __builtin_bit_cast(h4_t, hi);
      const h8_t bf = h8_t{l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[nt], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) xv[i] = xn[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) av[j] = an[j];
  }
  // block reduction (4 waves) through LDS, then one float atomic per (c, tap) per block.
  // D[row = tap][col = channel]: lane holds channel nt*16 + (lane&15), taps 4*(lane>>4) + r
  __syncthreads();
  float* red = (float*)smem;   // [4][C*16]
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave * (C * 16) + (nt * 16 + (lane & 15)) * 16 + 4 * (lane >> 4) + r] = acc[nt][r];
  __syncthreads();
  // part != null: this block's sums go to part[block][C*16] (plain stores) and c1_wgrad_reduce_kernel adds the blocks in a fixed
  // order (bit-reproducible); else one float atomic per (c, tap) and block
  for (int i = threadIdx.x; i < C * 16; i += 256) {
    const float v = (red[i] + red[C * 16 + i] + red[2 * C * 16 + i] + red[3 * C * 16 + i]) * scale;
    if (part) part[(int64_t)blockIdx.x * (C * 16) + i] = v;
    else atomicAdd(dW + i, v);
  }
}

// dW[i] += sum over blocks of part[block][i] in a fixed order: a workgroup owns 16 outputs, thread (i, g) adds the blocks of
// group g (a contiguous range, four independent chains) and the 16 group sums are added in ascending order by one thread
// per output. (One thread per output walking all 512 blocks was 41 us on 4 workgroups; this is latency-bound on 32 loads.)
__global__ void __launch_bounds__(256) c1_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dW, int count, int blocks) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  const int per = (blocks + 15) / 16;
  const int b0 = g * per, b1 = min(blocks, b0 + per);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < count) {
    int b = b0;
    for (; b + 4 <= b1; b += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += part[(int64_t)(b + u) * count + i];
    }
    for (; b < b1; ++b) s[0] += part[(int64_t)b * count + i];
  }
  red[g][o] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (g == 0 && i < count) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][o];
    dW[i] += t;
  }
}

// C1Affine as the kernels take it (all null / 0 without one)
struct C1AffineP { const char* x2; int ld2; const float* sc2; const float* sh2; BnAccP fa; int use_fa; };
C1AffineP c1_affine_p(const C1Affine* aff) {
  C1AffineP p = {};
  if (aff) {
    p.x2 = (const char*)aff->x2; p.ld2 = aff->ld2; p.sc2 = aff->scale; p.sh2 = aff->shift;
    if (aff->bn) { p.use_fa = 1; gi_fill_acc_params(p.fa, *aff->bn); }
  }
  return p;
}

}  // namespace

// 256-thread launch of KERNEL<half_t> or KERNEL<float> by `dtype`, of KERNEL<c / PER> for c = 64 or 128 (`dtype`, `c`, `st`: the caller's)
#define C1_LAUNCH_T(KERNEL, grid, lds, ...)                                                                \
  do {                                                                                                     \
    if (dtype == GI_F16) hipLaunchKernelGGL(KERNEL<half_t>, dim3(grid), dim3(256), lds, st, __VA_ARGS__);  \
    else hipLaunchKernelGGL(KERNEL<float>, dim3(grid), dim3(256), lds, st, __VA_ARGS__);                   \
  } while (0)
#define C1_LAUNCH_C(KERNEL, PER, grid, lds, ...)                                                           \
  do {                                                                                                     \
    if (c == 128) hipLaunchKernelGGL(KERNEL<128 / PER>, dim3(grid), dim3(256), lds, st, __VA_ARGS__);      \
    else hipLaunchKernelGGL(KERNEL<64 / PER>, dim3(grid), dim3(256), lds, st, __VA_ARGS__);                \
  } while (0)

int op_c1_gather(hipStream_t st, int dtype, const float* img, const float* w, void* out, int n, int Hs, int Ws, int c,
                 int ldout, int coffout, int act_out, float in_scale, const float* bias, unsigned long long* bits, int* bits_written) {
  GI_REQUIRE(c % 8 == 0 && c <= 1024, "c1_gather: c=%d", c);
  if (bits_written) *bits_written = 0;
  const int64_t total = (int64_t)n * Hs * Ws * (c / 8);
  const int groups = c / 8;
  if (dtype == GI_F16 && !bias && (c == 64 || c == 128) && Ws % 16 == 0 && ldout % 8 == 0 && coffout % 8 == 0) {
    const int64_t ngroups = (int64_t)n * Hs * Ws / 16;
    GI_REQUIRE(ngroups < (1ll << 31) && (act_out == GI_ACT_NONE || act_out == GI_ACT_RELU || act_out == GI_ACT_LRELU), "c1_gather: %lld pixel groups / activation %d",
               (long long)ngroups, act_out);
    const int grid = grid_for(ngroups, 4, 256 * 8);
    unsigned long long* const bw = c == 64 ? bits : nullptr;   // (the sign words cover 64 channels)
    if (bw && bits_written) *bits_written = 1;
#define GI_C1G_(MTC_, ACT_) hipLaunchKernelGGL((c1_gather_mfma_kernel<MTC_, ACT_>), dim3(grid), dim3(256), 0, st, img, w, (char*)out, n, Hs, Ws, ldout, coffout, in_scale, bw)
#define GI_C1G(ACT_) do { if (c == 64) GI_C1G_(4, ACT_); else GI_C1G_(8, ACT_); } while (0)
    if (act_out == GI_ACT_LRELU) GI_C1G(GI_ACT_LRELU); else if (act_out == GI_ACT_RELU) GI_C1G(GI_ACT_RELU); else GI_C1G(GI_ACT_NONE);
#undef GI_C1G
#undef GI_C1G_
    GI_LAUNCH_CHECK();
    gi_note_kernel(c == 64 ? "c1_gather_mfma<4>" : "c1_gather_mfma<8>");
    return GI_OK;
  }
  if (gi_is_pow2(groups) && groups <= 32 && Ws % (256 / groups) == 0) {
    const int S = 256 / groups;
    const int64_t nstrips = (int64_t)n * Hs * (Ws / S);
    const int grid = (int)(nstrips < 256 * 8 ? nstrips : 256 * 8);
    const size_t lds = (size_t)(16 * c + 2 * 4 * (2 * S + 2)) * 4;
    C1_LAUNCH_T(c1_gather_strip_kernel, grid, lds, img, w, (char*)out, n, Hs, Ws, c, ldout, coffout, act_out, in_scale, bias);
    GI_LAUNCH_CHECK();
    gi_note_kernel("c1_gather_strip");
    return GI_OK;
  }
  // the generic form splits a thread index into (pixel, 8-channel group) with a mask and a shift
  GI_REQUIRE(gi_is_pow2(groups), "c1_gather: c=%d unsupported here (c / 8 must be a power of two)", c);
  const int grid = grid_for(total, 256, 256 * 16);
  C1_LAUNCH_T(c1_gather_kernel, grid, c * 16 * 4, img, w, (char*)out, n, Hs, Ws, c, ldout, coffout, act_out, in_scale, bias);
  GI_LAUNCH_CHECK();
  gi_note_kernel("c1_gather");
  return GI_OK;
}

// first stage for many rows (the fused form writes one row per GEMM workgroup: 2048 on the critic): workgroup g adds rows
// [g * per, (g + 1) * per) in order for all `count` outputs, 16-byte loads, eight in flight, and writes row g of `out`
__global__ void __launch_bounds__(256) c1_wgrad_rows_kernel(const float* __restrict__ part, float* __restrict__ out, int count, int blocks, int per) {
  const int b0 = blockIdx.x * per, b1 = min(blocks, b0 + per);
  const int stride = count / 4;
  for (int i = threadIdx.x; i < stride; i += 256) {
    f4_t s = {0.f, 0.f, 0.f, 0.f};
    s = gi_ordered_sum_f4((const f4_t*)part + i, stride, b0, b1, s);
    ((f4_t*)out)[(int64_t)blockIdx.x * stride + i] = s;
  }
}

int op_c1_wgrad_reduce(hipStream_t st, const float* part, float* dW, int count, int blocks, float* scratch, int64_t scratch_floats) {
  constexpr int G1 = 64;
  if (blocks >= 4 * G1 && count % 4 == 0 && scratch && scratch_floats >= (int64_t)G1 * count) {
    const int per = (blocks + G1 - 1) / G1;
    hipLaunchKernelGGL(c1_wgrad_rows_kernel, dim3(G1), dim3(256), 0, st, part, scratch, count, blocks, per);
    GI_LAUNCH_CHECK();
    part = scratch;
    blocks = (blocks + per - 1) / per;
  }
  hipLaunchKernelGGL(c1_wgrad_reduce_kernel, dim3((count + 15) / 16), dim3(256), 0, st, part, dW, count, blocks);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

bool op_c1_affine_ok(int dtype, int c, int Ws, int ldx, int coffx) {
  return dtype == GI_F16 && (c == 64 || c == 128) && Ws % 32 == 0 && ldx % 8 == 0 && coffx % 8 == 0;
}

int op_c1_scatter(hipStream_t st, int dtype, const void* X, const float* w, const float* bias, float* img, int n, int Hs,
                  int Ws, int c, int ldx, int coffx, int relu_in, int post, float out_scale, void* col_scratch, float* img2,
                  const C1Affine* aff) {
  GI_REQUIRE(!aff || (col_scratch && op_c1_affine_ok(dtype, c, Ws, ldx, coffx) && aff->ld2 % 8 == 0), "c1_scatter: fused upper half unsupported here");
  if (dtype == GI_F16 && col_scratch && (c == 64 || c == 128) && ldx % 8 == 0 && coffx % 8 == 0) {
    const int64_t P = (int64_t)n * Hs * Ws;
    const int grid = grid_for((P + 15) / 16, 4, 256 * 8);
    GI_REQUIRE(!(aff && aff->bn) || aff->bn->groups == 1, "c1_scatter: one BatchNorm population expected");
    const C1AffineP u = c1_affine_p(aff);
    // one launch (c1_scatter_fused_kernel) where a band of rows fits LDS; GI_C1_FUSED=0: the col tensor + the overlap-add launch
    int TH = 1024 / Ws;
    if (TH < 1) TH = 1;
    if (TH > Hs) TH = Hs;
    const size_t lds_f = (size_t)(TH + 2) * Ws * 32 + 2 * (c / 2) * sizeof(float);
    if (gi_opt(GI_OPT_C1_FUSED) && Ws % 16 == 0 && lds_f <= 64 * 1024 && (int64_t)n * ((Hs + TH - 1) / TH) < (1ll << 31)) {
      const int gridf = n * ((Hs + TH - 1) / TH);
      C1_LAUNCH_C(c1_scatter_fused_kernel, 32, gridf, lds_f, (const char*)X, w, bias, img, img2, Hs, Ws, TH, ldx, coffx, relu_in, u.x2, u.ld2, u.sc2, u.sh2,
                  u.fa, u.use_fa, post, out_scale);
      GI_LAUNCH_CHECK();
      gi_note_kernel(c == 128 ? "c1_scatter_fused<4>" : "c1_scatter_fused<2>");
      return GI_OK;
    }
    C1_LAUNCH_C(c1_col_kernel, 32, grid, 0, (const char*)X, w, (half_t*)col_scratch, P, ldx, coffx, relu_in, u.x2, u.ld2, u.sc2, u.sh2, u.fa, u.use_fa);
    GI_LAUNCH_CHECK();
    hipLaunchKernelGGL(c1_col2im_kernel, dim3(grid_for(P, 256, 256 * 8)), dim3(256), 0, st, (const half_t*)col_scratch, bias, img, img2, n, Hs,
                       Ws, post, out_scale);
    GI_LAUNCH_CHECK();
    gi_note_kernel(c == 128 ? "c1_col+col2im<4>" : "c1_col+col2im<2>");
    return GI_OK;
  }
  const int epc = dtype == GI_F16 ? 8 : 4;
  const int lpp = c / epc;
  GI_REQUIRE(c % epc == 0 && gi_is_pow2(lpp) && lpp <= 64, "c1_scatter: c=%d unsupported", c);
  const int64_t total = (int64_t)n * Hs * Ws;
  const int grid = grid_for(total, 256 / lpp, 256 * 8);
  C1_LAUNCH_T(c1_scatter_kernel, grid, 0, (const char*)X, w, bias, img, n, Hs, Ws, c, ldx, coffx, relu_in, post, out_scale);
  GI_LAUNCH_CHECK();
  if (img2) GI_HIP(hipMemcpyAsync(img2, img, (size_t)n * 4 * Hs * Ws * 4, hipMemcpyDeviceToDevice, st));
  gi_note_kernel("c1_scatter");
  return GI_OK;
}

int op_c1_wgrad(hipStream_t st, int dtype, const void* X, const float* img, float* dW, int n, int Hs, int Ws, int c,
                int ldx, int coffx, int relu_in, float scale, float img_scale, const C1Affine* aff, float* scratch, int64_t scratch_floats) {
  GI_REQUIRE(!aff || (op_c1_affine_ok(dtype, c, Ws, ldx, coffx) && aff->ld2 % 8 == 0), "c1_wgrad: fused upper half unsupported here");
  if (dtype == GI_F16 && (c == 64 || c == 128) && Ws % 32 == 0 && ldx % 8 == 0 && coffx % 8 == 0) {
    const int64_t ntiles = (int64_t)n * Hs * Ws / 32;
    GI_REQUIRE(ntiles < (1ll << 31), "c1_wgrad: %lld pixel tiles", (long long)ntiles);
    int grid = (int)((ntiles + 3) / 4);
    const int cap = gi_tune("GI_C1W_GRID", 512);       // per workgroup: c*16 partial sums (stores or atomics)
    if (grid > cap) grid = cap;
    size_t lds = (size_t)4 * 32 * (c * 2 + 32);
    if (lds < (size_t)4 * c * 16 * 4) lds = (size_t)4 * c * 16 * 4;
    float* part = (scratch && scratch_floats >= (int64_t)grid * c * 16) ? scratch : nullptr;   // deterministic two-stage sum
    const C1AffineP u = c1_affine_p(aff);   // (the vectors exist by now: u.fa is not used)
    C1_LAUNCH_C(c1_wgrad_mfma_kernel, 16, grid, lds, (const char*)X, img, dW, n, Hs, Ws, ldx, coffx, relu_in, scale, img_scale, u.x2, u.ld2, u.sc2, u.sh2,
                part);
    GI_LAUNCH_CHECK();
    if (part) {
      hipLaunchKernelGGL(c1_wgrad_reduce_kernel, dim3((c * 16 + 15) / 16), dim3(256), 0, st, (const float*)part, dW, c * 16, grid);
      GI_LAUNCH_CHECK();
    }
    gi_note_kernel(part ? "c1_wgrad_mfma" : "c1_wgrad_mfma,atomics");   // (which summation ran: fixed-order partials or float atomics)
    return GI_OK;
  }
  const int epc = dtype == GI_F16 ? 8 : 4;
  const int lpp = c / epc;
  GI_REQUIRE(c % epc == 0 && gi_is_pow2(lpp) && lpp <= 64, "c1_wgrad: c=%d unsupported", c);
  const int64_t total = (int64_t)n * Hs * Ws;
  const int gpb = 256 / lpp;
  int ppb = (int)((total + 1023) / 1024);
  ppb = (ppb + gpb - 1) / gpb * gpb;
  if (ppb < gpb) ppb = gpb;
  const int grid = (int)((total + ppb - 1) / ppb);
  const size_t lds = (size_t)gpb * c * 4 * 4;
  float* part = (scratch && scratch_floats >= (int64_t)grid * c * 16) ? scratch : nullptr;   // deterministic two-stage sum
  C1_LAUNCH_T(c1_wgrad_kernel, grid, lds, (const char*)X, img, dW, n, Hs, Ws, c, ldx, coffx, relu_in, scale, img_scale, ppb, part);
  GI_LAUNCH_CHECK();
  if (part) {
    hipLaunchKernelGGL(c1_wgrad_reduce_kernel, dim3((c * 16 + 15) / 16), dim3(256), 0, st, (const float*)part, dW, c * 16, grid);
    GI_LAUNCH_CHECK();
  }
  gi_note_kernel(part ? "c1_wgrad" : "c1_wgrad,atomics");
  return GI_OK;
}
#undef C1_LAUNCH_T
#undef C1_LAUNCH_C

// The 4-channel head of a narrow generator (fp16, c = 128 input channels): forward (col + col2im, bias + tanh) and input gradient.
bool op_c1_head4_ok(int dtype, int c, int out_c, int Ws, int ldx, int coffx) {
  return dtype == GI_F16 && c == 128 && out_c == 4 && Ws % 16 == 0 && ldx % 8 == 0 && coffx % 8 == 0;
}
int64_t op_c1_head4_col_bytes(int n, int Hs, int Ws) { return (int64_t)n * Hs * Ws * 16 * 4 * 2; }
int op_c1_head4_forward(hipStream_t st, const void* X, const float* w, const float* bias, float* out, float* out2, int n, int Hs, int Ws, int ldx,
                        int coffx, int relu_in, void* col_scratch) {
  const int64_t P = (int64_t)n * Hs * Ws;
  hipLaunchKernelGGL((c1_col_mc_kernel<4, 4>), dim3(grid_for((P + 15) / 16, 4, 256 * 8)), dim3(256), 0, st, (const char*)X, w, (half_t*)col_scratch, P,
                     ldx, coffx, relu_in);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(c1_col2im_mc_kernel<4>, dim3(grid_for(P * 4, 256, 256 * 8)), dim3(256), 0, st, (const half_t*)col_scratch, bias, out, out2, n, Hs,
                     Ws, 1);
  GI_LAUNCH_CHECK();
  gi_note_kernel("c1_head4");
  return GI_OK;
}
int op_c1_head4_dgrad(hipStream_t st, const float* g, const float* w, void* out, int n, int Hs, int Ws, int ldout, int coffout) {
  GI_REQUIRE(Ws % 16 == 0 && ldout % 8 == 0 && coffout % 8 == 0, "c1_head4_dgrad: layout");
  const int64_t ngroups = (int64_t)n * Hs * Ws / 16;
  hipLaunchKernelGGL(c1_gather_mc4_kernel<8>, dim3(grid_for(ngroups, 4, 256 * 8)), dim3(256), 0, st, g, w, (char*)out, n, Hs, Ws, ldout, coffout);
  GI_LAUNCH_CHECK();
  gi_note_kernel("c1_head4_dgrad");
  return GI_OK;
}
