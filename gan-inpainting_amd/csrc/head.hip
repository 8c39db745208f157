// The PatchGAN critic head: Conv2d(512,1,4,1,0) + Flatten + Linear(P,1) [+ Sigmoid] (lib/models/networks.py:352-357), forward and
// backward: generic kernels for any dtype / channel count and the fp16 c = 512 kernels the networks run (GI_HEAD_FAST).
#include "common.h"
#include "stat_acc.h"
#include "bn_acc.h"

namespace {

// ---- discriminator head ----------------------------------------------------------------------
// h[n,py,px] = sum_{ky,kx,c} a4[n,py+ky,px+kx,c] * w5[ky*4+kx][c]     (Conv2d(512,1,4,1,0), networks.py:352)
template <typename T>
__global__ void __launch_bounds__(256) head_conv_kernel(const char* a4, const float* __restrict__ w5, float* h, int Hh,
                                                        int Wh, int c) {
  constexpr int EPC = 16 / (int)sizeof(T);
  __shared__ float red[4];
  const int Ph = Hh - 3, Pw = Wh - 3;
  const int o = blockIdx.x;  // (n, py, px)
  const int px = o % Pw, py = (o / Pw) % Ph, nn = o / (Pw * Ph);
  const int cpt = c / EPC;  // chunks per tap
  float s = 0.f;
  for (int idx = threadIdx.x; idx < 16 * cpt; idx += 256) {
    const int tap = idx / cpt, cc = idx % cpt;
    const int iy = py + (tap >> 2), ix = px + (tap & 3);
    const char* src = a4 + ((((int64_t)nn * Hh + iy) * Wh + ix) * c + cc * EPC) * (int64_t)sizeof(T);
    const float* wr = w5 + tap * c + cc * EPC;
    if constexpr (std::is_same<T, half_t>::value) {
      const h8_t v = *(const h8_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) s = fmaf((float)v[e], wr[e], s);
    } else {
      const f4_t v = *(const f4_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) s = fmaf(v[e], wr[e], s);
    }
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) h[o] = red[0] + red[1] + red[2] + red[3];
}

// out[n] = [sigmoid](bl + sum_p wl[p]*h[n,p])     (Flatten + Linear(P,1) [+ Sigmoid], networks.py:353-357)
__global__ void __launch_bounds__(64) head_linear_kernel(const float* h, const float* wl, const float* bl, float* out,
                                                         int P, int sigmoid) {
  const int nn = blockIdx.x;
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += 64) s = fmaf(h[(int64_t)nn * P + i], wl[i], s);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) {
    s += bl[0];
    out[nn] = sigmoid ? 1.f / (1.f + expf(-s)) : s;
  }
}

// dz[n] = dy[n] * (sigmoid ? out(1-out) : 1); dh[n,p] = dz[n]*wl[p]; dwl[p] += sum_n dz[n]*h[n,p]; dbl += sum dz
__global__ void __launch_bounds__(256) head_linear_bwd_kernel(const float* dy, const float* out, const float* h,
                                                              const float* wl, float* dh, float* dwl, float* dbl, int n,
                                                              int P, int sigmoid) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
    float gw = 0.f;
    for (int nn = 0; nn < n; ++nn) {
      const float o = out[nn];
      const float dz = dy[nn] * (sigmoid ? o * (1.f - o) : 1.f);
      dh[(int64_t)nn * P + p] = dz * wl[p];
      gw = fmaf(dz, h[(int64_t)nn * P + p], gw);
    }
    if (dwl) atomicAdd(dwl + p, gw);
  }
  if (dbl && blockIdx.x == 0 && threadIdx.x == 0) {
    float gb = 0.f;
    for (int nn = 0; nn < n; ++nn) {
      const float o = out[nn];
      gb += dy[nn] * (sigmoid ? o * (1.f - o) : 1.f);
    }
    atomicAdd(dbl, gb);
  }
}

// da4[n,y,x,c] = loss_scale * sum_{tap: (y-ky,x-kx) valid} dh[n,y-ky,x-kx] * w5[tap][c]
template <typename T>
__global__ void __launch_bounds__(256) head_dgrad_kernel(const float* dh, const float* __restrict__ w5, char* da4, int n,
                                                         int Hh, int Wh, int c, float loss_scale) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int Ph = Hh - 3, Pw = Wh - 3;
  const int cpt = c / EPC;
  const int64_t total = (int64_t)n * Hh * Wh * cpt;
  for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (int64_t)gridDim.x * 256) {
    const int cc = (int)(gid % cpt);
    const int64_t pix = gid / cpt;
    const int x = (int)(pix % Wh), y = (int)((pix / Wh) % Hh), nn = (int)(pix / ((int64_t)Wh * Hh));
    float s[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) s[e] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      const int py = y - (tap >> 2), px = x - (tap & 3);
      if (py < 0 || py >= Ph || px < 0 || px >= Pw) continue;
      const float g = dh[((int64_t)nn * Ph + py) * Pw + px];
      const float* wr = w5 + tap * c + cc * EPC;
#pragma unroll
      for (int e = 0; e < EPC; ++e) s[e] = fmaf(g, wr[e], s[e]);
    }
    T* dst = (T*)(da4 + (pix * c + cc * EPC) * (int64_t)sizeof(T));
#pragma unroll
    for (int e = 0; e < EPC; ++e) dst[e] = (T)(s[e] * loss_scale);
  }
}

// dw5[tap][c] += sum_{n,p} dh[n,p] * a4[n,p+tap][c]   (grid.y = n, grid.z = output row py)
// part != null: the (image, row band) blocks store their sums there ([block][16 c]) and head_wgrad_sum_kernel adds them in block
// order - bit-reproducible (the fp32 critic of BASELINE config 2); part == null: float atomics into dw5
template <typename T>
__global__ void __launch_bounds__(256) head_wgrad_kernel(const float* dh, const char* a4, float* dw5, int Hh, int Wh,
                                                         int c, float* part) {
  constexpr int EPC = 16 / (int)sizeof(T);
  const int Ph = Hh - 3, Pw = Wh - 3;
  const int cpt = c / EPC;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 16 * cpt) return;
  const int tap = idx / cpt, cc = idx % cpt;
  // blockIdx.z covers a band of output rows: 1/band of the atomics (they contend on 16*c addresses)
  const int nn = blockIdx.y;
  const int band = (Ph + (int)gridDim.z - 1) / (int)gridDim.z;
  const int py0 = blockIdx.z * band, py1 = min(Ph, py0 + band);
  float s[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) s[e] = 0.f;
  for (int py = py0; py < py1; ++py)
  for (int px = 0; px < Pw; ++px) {
    const float g = dh[((int64_t)nn * Ph + py) * Pw + px];
    const char* src = a4 + ((((int64_t)nn * Hh + py + (tap >> 2)) * Wh + px + (tap & 3)) * c + cc * EPC) * (int64_t)sizeof(T);
    if constexpr (std::is_same<T, half_t>::value) {
      const h8_t v = *(const h8_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) s[e] = fmaf(g, (float)v[e], s[e]);
    } else {
      const f4_t v = *(const f4_t*)src;
#pragma unroll
      for (int e = 0; e < EPC; ++e) s[e] = fmaf(g, v[e], s[e]);
    }
  }
  if (part) {
    float* o = part + ((int64_t)blockIdx.y * gridDim.z + blockIdx.z) * 16 * c + tap * c + cc * EPC;
#pragma unroll
    for (int e = 0; e < EPC; ++e) o[e] = s[e];
    return;
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) atomicAdd(dw5 + tap * c + cc * EPC + e, s[e]);
}
__global__ void __launch_bounds__(256) head_wgrad_sum_kernel(const float* part, int nparts, float* dw5, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(int64_t)k * count + i];
  dw5[i] += s;
}

// ---- fp16 head at c = 512 (the PatchGAN of networks.py:331-363): one pixel row = 1 KiB = one wave load --------
// Forward, one workgroup per image: t[px][tap] = a4[px][:] . w5[tap][:] on the MFMA (16 px x 16 taps x 32 channels
// per instruction; w5 as fp16 fragments resident in registers, fp32 accumulation), so every activation is read once;
// then h[p] = sum_tap t[p + (ky,kx)][tap], the Linear(P,1) and the optional sigmoid in the same workgroup.
constexpr int HT_PITCH = 17;   // floats per pixel row of t in LDS (16 taps + 1: conflict-free column reads)
__global__ void __launch_bounds__(1024) head_fwd512_kernel(const char* __restrict__ a4, const float* __restrict__ w5,
                                                           const float* __restrict__ wl, const float* __restrict__ bl,
                                                           float* __restrict__ h, float* __restrict__ out,
                                                           float* __restrict__ out2, int Hh, int Wh, int sigmoid,
                                                           const float* __restrict__ sc4, const float* __restrict__ sh4,
                                                           int n_per_group, int gstride, float* __restrict__ tbuf, int slices,
                                                           BnAccP fa, int use_fa) {
  // tbuf != null (large feature maps, few images): `slices` workgroups per image each compute t for their share of
  // the pixel tiles into tbuf[image][pixel][16] and stop; head_h512_kernel finishes (h, Linear, sigmoid).
  // sc4 != null: a4 is the RAW conv4 output; LeakyReLU(fma(x, sc4, sh4)) (the layer's BatchNorm + activation, the
  // population of image nn at +gstride floats) is applied to the fragments as they are loaded, the same fp32
  // expression and fp16 rounding as the separate apply pass
  extern __shared__ float t_lds[];   // [Hh*Wh][HT_PITCH] | 16 partial sums | w5 as fp16 [16 taps][512] | scale, shift [2][512]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nn = tbuf ? blockIdx.x / slices : blockIdx.x, npx = Hh * Wh;
  float* red = t_lds + (tbuf ? 0 : ((npx * HT_PITCH + 3) & ~3));   // 16-byte aligned
  half_t* wh = (half_t*)(red + 16);
  float* aff = (float*)(wh + 16 * 512);
  // this wave's first pixel tile is requested before the prologue (weights to LDS, the scale / shift derivation with its accumulator
  // round trip): at the critic's map sizes a wave owns ONE tile, so that is all of its activation traffic
  const char* img = a4 + (int64_t)nn * npx * 1024;
  const int ntile = (npx + 15) / 16;
  const int tile0 = tbuf ? (int)((int64_t)ntile * (blockIdx.x % slices) / slices) : 0;
  const int tile1 = tbuf ? (int)((int64_t)ntile * (blockIdx.x % slices + 1) / slices) : ntile;
  h8_t av[16];
  constexpr int AV_EARLY = 12;   // chunks requested before the prologue; the rest behind it (all 16 + the prologue's 64 accumulator
                                 // registers went 16 bytes over the 128 VGPRs of a 1024-thread workgroup)
  const char* row0;
  {
    const int t0 = tile0 + wave < tile1 ? tile0 + wave : tile0;     // (a wave without a tile loads one it will not use)
    row0 = img + (int64_t)min(t0 * 16 + (lane & 15), npx - 1) * 1024 + (lane >> 4) * 16;
#pragma unroll
    for (int ks = 0; ks < AV_EARLY; ++ks) av[ks] = *(const h8_t*)(row0 + ks * 64);
  }
  if (sc4 && use_fa) {
    // the scale / shift vectors do not exist yet: derived here from conv4's exact accumulators (bn_acc.h) - every workgroup the
    // vectors of its image's population; workgroup 0 publishes ALL populations' vectors (sc4 / sh4 and the backward's), moves the
    // running statistics population by population and clears the layer's other accumulator region: no finalize launch
    const int grp = nn / n_per_group;
    if (threadIdx.x < 512) {
      float a = 0.f, b = 0.f;
      if (blockIdx.x == 0) {
        for (int j = 0; j < fa.groups; ++j) {
          float aj, bj;
          bn_from_acc(fa, 512, threadIdx.x, j, true, aj, bj);
          if (j == grp) { a = aj; b = bj; }
        }
      } else {
        bn_from_acc(fa, 512, threadIdx.x, grp, false, a, b);
      }
      aff[threadIdx.x] = a;
      aff[512 + threadIdx.x] = b;
    }
    if (blockIdx.x == 0 && fa.zero_next) {
      for (int i = threadIdx.x; i < fa.zero_words; i += 1024) fa.zero_next[i] = 0ull;
    }
  } else if (sc4) {
    const int go = (nn / n_per_group) * gstride;
    for (int i = threadIdx.x; i < 512; i += 1024) { aff[i] = sc4[go + i]; aff[512 + i] = sh4[go + i]; }
  }
  for (int i = threadIdx.x; i < 16 * 512 / 4; i += 1024) {
    const f4_t v = *(const f4_t*)(w5 + i * 4);
    *(h4_t*)(wh + i * 4) = h4_t{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
  }
#pragma unroll
  for (int ks = AV_EARLY; ks < 16; ++ks) av[ks] = *(const h8_t*)(row0 + ks * 64);
  __syncthreads();
  // (the weight fragments are read from LDS next to their MFMA: kept in registers beside av - 64 + 64 of the 128 a 1024-thread
  //  workgroup has per lane - the kernel spilled 132 bytes per lane, and at the critic's map sizes a wave owns one tile anyway)
  const half_t* bfp = wh + (lane & 15) * 512 + (lane >> 4) * 8;
  for (int tile = tile0 + wave; tile < tile1; tile += 16) {
    if (tile != tile0 + wave) {      // later tiles of this wave (large maps)
      const int px = min(tile * 16 + (lane & 15), npx - 1);
      const char* row = img + (int64_t)px * 1024 + (lane >> 4) * 16;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) av[ks] = *(const h8_t*)(row + ks * 64);
    }
    if (sc4) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const float* a0 = aff + ks * 32 + (lane >> 4) * 8;
        const f4_t s0 = *(const f4_t*)a0, s1 = *(const f4_t*)(a0 + 4), h0 = *(const f4_t*)(a0 + 512), h1 = *(const f4_t*)(a0 + 516);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = fmaf((float)av[ks][j], j < 4 ? s0[j & 3] : s1[j & 3], j < 4 ? h0[j & 3] : h1[j & 3]);
          av[ks][j] = (half_t)(t > 0.f ? t : 0.2f * t);
        }
      }
    }
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[ks], *(const h8_t*)(bfp + ks * 32), acc, 0, 0, 0);
    // D[row = pixel][col = tap]: lane holds tap (lane&15), pixels 4*(lane>>4) + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = tile * 16 + 4 * (lane >> 4) + r;
      if (q < npx) {
        if (tbuf) tbuf[((int64_t)nn * npx + q) * 16 + (lane & 15)] = acc[r];
        else t_lds[q * HT_PITCH + (lane & 15)] = acc[r];
      }
    }
  }
  if (tbuf) return;
  __syncthreads();
  const int Ph = Hh - 3, Pw = Wh - 3, P = Ph * Pw;
  float part = 0.f;
  for (int p = threadIdx.x; p < P; p += 1024) {
    const int py = p / Pw, px = p - py * Pw;
    float sacc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) sacc += t_lds[((py + (tap >> 2)) * Wh + px + (tap & 3)) * HT_PITCH + tap];
    h[(int64_t)nn * P + p] = sacc;
    part = fmaf(sacc, wl[p], part);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float z = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) z += red[w];
    z += bl[0];
    z = sigmoid ? 1.f / (1.f + expf(-z)) : z;
    out[nn] = z;
    if (out2) out2[nn] = z;
  }
}

// second stage of the sliced forward: h[p] = sum_tap t[p + (ky,kx)][tap], Linear(P,1), sigmoid; one workgroup per image
__global__ void __launch_bounds__(256) head_h512_kernel(const float* __restrict__ tbuf, const float* __restrict__ wl,
                                                        const float* __restrict__ bl, float* __restrict__ h,
                                                        float* __restrict__ out, float* __restrict__ out2, int Hh, int Wh,
                                                        int sigmoid) {
  __shared__ float red[4];
  const int nn = blockIdx.x, npx = Hh * Wh, Ph = Hh - 3, Pw = Wh - 3, P = Ph * Pw;
  const float* t = tbuf + (int64_t)nn * npx * 16;
  float part = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) {
    const int py = p / Pw, px = p - py * Pw;
    float sacc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) sacc += t[((py + (tap >> 2)) * Wh + px + (tap & 3)) * 16 + tap];
    h[(int64_t)nn * P + p] = sacc;
    part = fmaf(sacc, wl[p], part);
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float z = ((red[0] + red[1]) + (red[2] + red[3])) + bl[0];
    z = sigmoid ? 1.f / (1.f + expf(-z)) : z;
    out[nn] = z;
    if (out2) out2[nn] = z;
  }
}

// Backward, two roles by blockIdx in one launch (dh[n,p] = dz[n]*wl[p] is never materialised):
//   [0, nb)        input gradient: da4[n,y,x,:] = loss_scale * sum_tap dh[n,y-ky,x-kx] * w5[tap][:], a lane owns 8
//                  channels with its 16x8 weights in registers, a wave owns a pixel (one 1-KiB store);
//   [nb, 2nb)      weight-gradient partial of the same pixel range: acc[tap][8ch] += dh[..] * a4[n,y,x,8ch], reduced over
//                  the 4 waves in LDS and stored to part[block][16][512] (summed in fixed order by head_wsum512_kernel);
//   The Linear's gradients dwl[p] += sum_n dz[n]*h[n,p], dbl += sum_n dz[n] ride in head_wsum512_kernel.
// Without parameter gradients (frozen critic) only the first nb blocks are launched.
__global__ void __launch_bounds__(256) head_bwd512_kernel(const float* __restrict__ dy, const float* __restrict__ outv,
                                                          const float* __restrict__ hsave, const float* __restrict__ wl,
                                                          const float* __restrict__ w5, const char* __restrict__ a4,
                                                          char* __restrict__ da4, float* __restrict__ part,
                                                          float* __restrict__ dwl, float* __restrict__ dbl, int n, int Hh,
                                                          int Wh, int bands, int sigmoid, float loss_scale,
                                                          const float* __restrict__ sc4, const float* __restrict__ sh4,
                                                          int n_per_group, int gstride, HeadBwdFuse hf) {
  __shared__ float red[2 * 16 * 512];   // 64 KiB: two waves' accumulators at a time
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Ph = Hh - 3, Pw = Wh - 3, P = Ph * Pw, npx = Hh * Wh;
  const int nb = n * bands;
  int b = blockIdx.x;
  const bool wgrad = b >= nb;
  if (wgrad) b -= nb;
  const int nn = b / bands, band = b - nn * bands;
  const int ppb = (npx + bands - 1) / bands;               // pixels per block
  const int q0 = band * ppb, q1 = min(npx, q0 + ppb);
  const float o = outv[nn];
  const float dz = dy[nn] * (sigmoid ? o * (1.f - o) : 1.f) * (wgrad ? 1.f : loss_scale);
  // gp[(py+3)*GW + px+3] = dz * wl[py*Pw+px] with a 3-wide zero border: dh of this image without bounds checks
  const int GW = Pw + 6;
  float* gp = red;
  for (int i = threadIdx.x; i < (Ph + 6) * GW; i += 256) {
    const int py = i / GW - 3, px = i - (py + 3) * GW - 3;
    gp[i] = (py >= 0 && py < Ph && px >= 0 && px < Pw) ? dz * wl[py * Pw + px] : 0.f;
  }
  __syncthreads();
  if (!wgrad) {
    float w[16][8];
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      const f4_t lo = *(const f4_t*)(w5 + tap * 512 + lane * 8), hi = *(const f4_t*)(w5 + tap * 512 + lane * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { w[tap][e] = lo[e]; w[tap][4 + e] = hi[e]; }
    }
    // hf.acc != null: the BatchNorm-backward sums of the layer in front (HeadBwdArgs::bwd_*) from the gradient this block produces -
    // the rounded value it stores, as the separate reduction would read it back - and the layer's raw output x, four pixels' rows
    // of x requested ahead per wave
    const bool bw = hf.acc != nullptr;
    float bsc[8], bsh[8], bmu[8], biv[8], bs[8], bsx[8];
    if (bw) {
      const int go = (nn / hf.n_per_group) * hf.stride + lane * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) { bsc[e] = hf.scale[go + e]; bsh[e] = hf.shift[go + e]; bmu[e] = hf.mean[go + e]; biv[e] = hf.inv[go + e]; bs[e] = bsx[e] = 0.f; }
    }
    const char* xrow = hf.x + (int64_t)nn * npx * 1024 + lane * 16;
    for (int qb = q0 + wave; qb < q1; qb += 16) {
      h8_t xs[4];
      if (bw) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = *(const h8_t*)(xrow + (int64_t)min(qb + 4 * j, npx - 1) * 1024);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = qb + 4 * j;
        if (q < q1) {                              // wave-uniform
          const int y = q / Wh, x = q - y * Wh;
          const float* gq = gp + (y + 3) * GW + x + 3;
          float g[16];
#pragma unroll
          for (int tap = 0; tap < 16; ++tap) g[tap] = gq[-(tap >> 2) * GW - (tap & 3)];   // LDS broadcast reads
          float sacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int tap = 0; tap < 16; ++tap)
#pragma unroll
            for (int e = 0; e < 8; ++e) sacc[e] = fmaf(g[tap], w[tap][e], sacc[e]);
          h8_t v;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (half_t)sacc[e];
          *(h8_t*)(da4 + ((int64_t)nn * npx + q) * 1024 + lane * 16) = v;
          if (bw) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float xf = (float)xs[j][e];
              const float dz = (float)v[e] * (fmaf(xf, bsc[e], bsh[e]) > 0.f ? 1.f : hf.slope);
              bs[e] += dz;
              bsx[e] = fmaf(dz, (xf - bmu[e]) * biv[e], bsx[e]);
            }
          }
        }
      }
    }
    if (bw) {     // the four waves' sums through LDS (gp is done with), then one exact add per channel and quantity
      __syncthreads();
      float* fold = red;   // [4 waves][512][2]
#pragma unroll
      for (int e = 0; e < 8; ++e) { fold[(wave * 512 + lane * 8 + e) * 2] = bs[e]; fold[(wave * 512 + lane * 8 + e) * 2 + 1] = bsx[e]; }
      __syncthreads();
      const int grp = nn / hf.n_per_group, rep = b & (hf.reps - 1);
      for (int ch = threadIdx.x; ch < 512; ch += 256) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) { s0 += fold[(wv * 512 + ch) * 2]; s1 += fold[(wv * 512 + ch) * 2 + 1]; }
        gi_stat_add(hf.acc, 512, rep, grp, 0, ch, s0);
        gi_stat_add(hf.acc, 512, rep, grp, 1, ch, s1);
      }
    }
    return;
  }
  float acc[16][8];
#pragma unroll
  for (int tap = 0; tap < 16; ++tap)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[tap][e] = 0.f;
  float s4[8], h4[8];   // sc4 != null: a4 is the raw conv4 output (see head_fwd512_kernel); a lane owns 8 channels
  if (sc4) {
    const int go = (nn / n_per_group) * gstride + lane * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { s4[e] = sc4[go + e]; h4[e] = sh4[go + e]; }
  }
  const char* arow = a4 + (int64_t)nn * npx * 1024 + lane * 16;
  for (int qb = q0 + wave; qb < q1; qb += 32) {   // 8 pixel rows in flight per wave
    h8_t v[8];
#pragma unroll
    for (int jx = 0; jx < 8; ++jx) v[jx] = *(const h8_t*)(arow + (int64_t)min(qb + 4 * jx, npx - 1) * 1024);
#pragma unroll
    for (int jx = 0; jx < 8; ++jx) {
      const int q = qb + 4 * jx;
      if (q >= q1) break;                          // wave-uniform
      const int y = q / Wh, x = q - y * Wh;
      const float* gq = gp + (y + 3) * GW + x + 3;
      float g[16];
#pragma unroll
      for (int tap = 0; tap < 16; ++tap) g[tap] = gq[-(tap >> 2) * GW - (tap & 3)];
      float vf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) vf[e] = (float)v[jx][e];
      if (sc4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = fmaf(vf[e], s4[e], h4[e]);
          vf[e] = (float)(half_t)(t > 0.f ? t : 0.2f * t);
        }
      }
#pragma unroll
      for (int tap = 0; tap < 16; ++tap)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[tap][e] = fmaf(g[tap], vf[e], acc[tap][e]);
    }
  }
  __syncthreads();   // every wave is done with gp before red is reused
  // waves 2,3 -> LDS, waves 0,1 add; wave 1 -> LDS, wave 0 adds and stores the block's partial
  auto put = [&](int slot) {
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      float* d = red + slot * 8192 + tap * 512 + lane * 8;
      *(f4_t*)d = f4_t{acc[tap][0], acc[tap][1], acc[tap][2], acc[tap][3]};
      *(f4_t*)(d + 4) = f4_t{acc[tap][4], acc[tap][5], acc[tap][6], acc[tap][7]};
    }
  };
  auto take = [&](int slot) {
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      const float* d = red + slot * 8192 + tap * 512 + lane * 8;
      const f4_t lo = *(const f4_t*)d, hi = *(const f4_t*)(d + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[tap][e] += lo[e]; acc[tap][4 + e] += hi[e]; }
    }
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) take(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    take(0);
    float* dst = part + (int64_t)b * 8192;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      *(f4_t*)(dst + tap * 512 + lane * 8) = f4_t{acc[tap][0], acc[tap][1], acc[tap][2], acc[tap][3]};
      *(f4_t*)(dst + tap * 512 + lane * 8 + 4) = f4_t{acc[tap][4], acc[tap][5], acc[tap][6], acc[tap][7]};
    }
  }
}

// dw5[i] += sum_b part[b][i] in a fixed order (deterministic): a workgroup owns 32 elements, 8 thread groups
// each sum every 8th partial, LDS combines the groups. Workgroups 256 .. 256+P-1 compute dwl[p] (threads over the
// batch, tree reduction), workgroup 256+P the Linear's bias gradient.
__global__ void __launch_bounds__(256) head_wsum512_kernel(const float* __restrict__ part, int nb, float* __restrict__ dw5,
                                                           const float* __restrict__ dy, const float* __restrict__ outv,
                                                           const float* __restrict__ hsave, float* __restrict__ dwl,
                                                           float* __restrict__ dbl, int n, int P, int sigmoid) {
  __shared__ float red[8][32];
  if (blockIdx.x >= 256) {
    const int p = blockIdx.x - 256;
    if (p == P && !dbl) return;
    float g = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float o = outv[i];
      const float dz = dy[i] * (sigmoid ? o * (1.f - o) : 1.f);
      g += p < P ? dz * hsave[(int64_t)i * P + p] : dz;
    }
    for (int off = 32; off > 0; off >>= 1) g += __shfl_xor(g, off);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float t = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      if (p < P) dwl[p] += t; else dbl[0] += t;
    }
    return;
  }
  const int e = threadIdx.x & 31, gq = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + e;   // < 8192
  float s0 = 0.f, s1 = 0.f;
  int b = gq;
  for (; b + 8 < nb; b += 16) {
    s0 += part[(int64_t)b * 8192 + i];
    s1 += part[(int64_t)(b + 8) * 8192 + i];
  }
  if (b < nb) s0 += part[(int64_t)b * 8192 + i];
  red[gq][e] = s0 + s1;
  __syncthreads();
  if (gq == 0) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += red[q][e];
    dw5[i] += t;
  }
}

// row bands per image for the backward: ~256 workgroups, at least 32 pixels each
static bool head_fast() { return gi_opt(GI_OPT_HEAD_FAST) != 0; }   // GI_HEAD_FAST=0: the generic kernels
static int head_bands(int n, int npx) {
  int bands = 1;
  while (n * bands < 256 && npx / (bands * 2) >= 32) bands *= 2;
  return bands;
}

}  // namespace

bool op_head_affine_ok(int dtype, int c) { return dtype == GI_F16 && c == 512 && head_fast(); }

int64_t op_head_scratch_bytes(int max_n, int Hh, int Wh) {
  (void)Hh; (void)Wh;   // n * head_bands(n, .) < 512 while bands > 1, = n otherwise
  return (int64_t)(max_n > 512 ? max_n : 512) * 8192 * 4;
}

int op_head_forward(hipStream_t st, int dtype, const HeadArgs& a) {
  const int Ph = a.Hh - 3, Pw = a.Wh - 3;
  GI_REQUIRE(Ph >= 1 && Pw >= 1, "head: feature map %dx%d too small", a.Hh, a.Wh);
  const int blocks = a.n * Ph * Pw;
  GI_REQUIRE(!a.scale4 || op_head_affine_ok(dtype, a.c), "head: fused BatchNorm input needs the fp16 c=512 kernels");
  GI_REQUIRE(!a.bn || (a.scale4 && dtype == GI_F16 && a.c == 512 && head_fast()), "head: accumulator-derived BatchNorm needs the fused fp16 c=512 path");
  if (dtype == GI_F16 && a.c == 512 && head_fast()) {
    BnAccP fa = {};
    const int use_fa = a.bn ? 1 : 0;
    if (use_fa) {
      gi_fill_acc_params(fa, *a.bn);
      GI_REQUIRE(fa.out_stride == a.gstride, "head: population stride %d != %d", fa.out_stride, a.gstride);
    }
    const int lds = (((a.Hh * a.Wh * HT_PITCH + 3) & ~3) + 16) * 4 + 16 * 512 * 2 + 2 * 512 * 4;
    GI_REQUIRE(lds <= 160 * 1024, "head: feature map %dx%d too large", a.Hh, a.Wh);
    if (lds > 64 * 1024) {
      static GiDevOnce attr;
      if (attr.first()) { GI_HIP(hipFuncSetAttribute((const void*)head_fwd512_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); }
    }
    // large maps with few images (512x512 inputs: 32x32 map, 64 tiles per image): slice each image over several
    // workgroups so that ~256 of them stream the activations, and finish in a second small kernel
    const int npx = a.Hh * a.Wh;
    int slices = 1;
    while (a.n * slices < 256 && npx / (slices * 2) >= 256) slices *= 2;
    if (slices > 1 && a.tbuf && a.tbuf_bytes >= (int64_t)a.n * npx * 16 * 4) {
      const int lds2 = (16) * 4 + 16 * 512 * 2 + 2 * 512 * 4;
      gi_note_kernel("head_fwd512_sliced");
      hipLaunchKernelGGL(head_fwd512_kernel, dim3(a.n * slices), dim3(1024), lds2, st, (const char*)a.a4, a.w5, a.wl, a.bl, a.h, a.out, a.out2, a.Hh,
                         a.Wh, a.sigmoid, a.scale4, a.shift4, a.n_per_group > 0 ? a.n_per_group : a.n, a.gstride, a.tbuf, slices, fa, use_fa);
      GI_LAUNCH_CHECK();
      hipLaunchKernelGGL(head_h512_kernel, dim3(a.n), dim3(256), 0, st, a.tbuf, a.wl, a.bl, a.h, a.out, a.out2, a.Hh, a.Wh, a.sigmoid);
      GI_LAUNCH_CHECK();
      return GI_OK;
    }
    gi_note_kernel("head_fwd512");
    hipLaunchKernelGGL(head_fwd512_kernel, dim3(a.n), dim3(1024), lds, st, (const char*)a.a4, a.w5, a.wl, a.bl, a.h, a.out, a.out2, a.Hh, a.Wh, a.sigmoid,
                       a.scale4, a.shift4, a.n_per_group > 0 ? a.n_per_group : a.n, a.gstride, (float*)nullptr, 1, fa, use_fa);
    GI_LAUNCH_CHECK();
    return GI_OK;
  }
  gi_note_kernel("head_fwd");
  if (dtype == GI_F16)
    hipLaunchKernelGGL(head_conv_kernel<half_t>, dim3(blocks), dim3(256), 0, st, (const char*)a.a4, a.w5, a.h, a.Hh, a.Wh, a.c);
  else
    hipLaunchKernelGGL(head_conv_kernel<float>, dim3(blocks), dim3(256), 0, st, (const char*)a.a4, a.w5, a.h, a.Hh, a.Wh, a.c);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_linear_kernel, dim3(a.n), dim3(64), 0, st, a.h, a.wl, a.bl, a.out, Ph * Pw, a.sigmoid);
  GI_LAUNCH_CHECK();
  if (a.out2) GI_HIP(hipMemcpyAsync(a.out2, a.out, (size_t)a.n * 4, hipMemcpyDeviceToDevice, st));
  return GI_OK;
}

int op_head_backward(hipStream_t st, int dtype, const HeadBwdArgs& a) {
  const int Ph = a.Hh - 3, Pw = a.Wh - 3, P = Ph * Pw;
  GI_REQUIRE(!a.scale4 || (op_head_affine_ok(dtype, a.c) && (!a.dw5 || (a.scratch && a.scratch_bytes >= (int64_t)a.n * head_bands(a.n, a.Hh * a.Wh) * 8192 * 4))),
             "head: fused BatchNorm input needs the fp16 c=512 kernels");
  if (dtype == GI_F16 && a.c == 512 && head_fast()) {
    const int bands = head_bands(a.n, a.Hh * a.Wh), nb = a.n * bands;
    const bool wg = a.dw5 != nullptr;
    HeadBwdFuse hf;
    hf.x = (const char*)a.bwd_x; hf.scale = a.bwd_scale; hf.shift = a.bwd_shift; hf.mean = a.bwd_mean; hf.inv = a.bwd_inv;
    hf.stride = a.bwd_stride; hf.n_per_group = a.bwd_n_per_group > 0 ? a.bwd_n_per_group : a.n; hf.reps = a.bwd_reps > 0 ? a.bwd_reps : 1;
    hf.slope = a.bwd_slope; hf.acc = (a.bwd_acc && a.bwd_x) ? a.bwd_acc : nullptr;
    if (!wg || (a.scratch && a.scratch_bytes >= (int64_t)nb * 8192 * 4)) {
      GI_REQUIRE(!wg || a.dwl, "head: dw5 without dwl");
      gi_note_kernel("head_bwd512");
      hipLaunchKernelGGL(head_bwd512_kernel, dim3(wg ? 2 * nb : nb), dim3(256), 0, st, a.dy, a.out, a.h, a.wl, a.w5, (const char*)a.a4,
                         (char*)a.da4, a.scratch, a.dwl, a.dbl, a.n, a.Hh, a.Wh, bands, a.sigmoid, a.loss_scale,
                         a.scale4, a.shift4, a.n_per_group > 0 ? a.n_per_group : a.n, a.gstride, hf);
      GI_LAUNCH_CHECK();
      if (hf.acc && a.bwd_applied) *a.bwd_applied = 1;
      if (wg) {
        hipLaunchKernelGGL(head_wsum512_kernel, dim3(256 + P + 1), dim3(256), 0, st, a.scratch, nb, a.dw5, a.dy, a.out, a.h, a.dwl, a.dbl, a.n, P, a.sigmoid);
        GI_LAUNCH_CHECK();
      }
      return GI_OK;
    }
  }
  gi_note_kernel("head_bwd");
  hipLaunchKernelGGL(head_linear_bwd_kernel, dim3((P + 255) / 256), dim3(256), 0, st, a.dy, a.out, a.h, a.wl, a.dh, a.dwl,
                     a.dbl, a.n, P, a.sigmoid);
  GI_LAUNCH_CHECK();
  const int epc = dtype == GI_F16 ? 8 : 4;
  const int64_t total = (int64_t)a.n * a.Hh * a.Wh * (a.c / epc);
  const int grid = grid_for(total, 256, 4096);
  if (dtype == GI_F16)
    hipLaunchKernelGGL(head_dgrad_kernel<half_t>, dim3(grid), dim3(256), 0, st, a.dh, a.w5, (char*)a.da4, a.n, a.Hh, a.Wh, a.c, a.loss_scale);
  else
    hipLaunchKernelGGL(head_dgrad_kernel<float>, dim3(grid), dim3(256), 0, st, a.dh, a.w5, (char*)a.da4, a.n, a.Hh, a.Wh, a.c, a.loss_scale);
  GI_LAUNCH_CHECK();
  if (a.dw5) {
    dim3 g((16 * (a.c / epc) + 255) / 256, a.n, Ph >= 8 ? 2 : 1);
    const int nparts = a.n * (int)g.z;
    float* part = (a.scratch && a.scratch_bytes >= (int64_t)nparts * 16 * a.c * 4) ? a.scratch : nullptr;
    if (dtype == GI_F16)
      hipLaunchKernelGGL(head_wgrad_kernel<half_t>, g, dim3(256), 0, st, a.dh, (const char*)a.a4, a.dw5, a.Hh, a.Wh, a.c, part);
    else
      hipLaunchKernelGGL(head_wgrad_kernel<float>, g, dim3(256), 0, st, a.dh, (const char*)a.a4, a.dw5, a.Hh, a.Wh, a.c, part);
    GI_LAUNCH_CHECK();
    if (part) {
      hipLaunchKernelGGL(head_wgrad_sum_kernel, dim3((16 * a.c + 255) / 256), dim3(256), 0, st, part, nparts, a.dw5, 16 * a.c);
      GI_LAUNCH_CHECK();
    }
  }
  return GI_OK;
}
