// DCGANDiscriminator (reference lib/models/networks.py:162-212) at 128x128, 1 channel:
//   4 x [Conv2d 5x5 s1 p1 + bias, ReLU, MaxPool 2/2]   128 -> 63 -> 30 -> 14 -> 6 (1 -> 128 -> 256 -> 512 -> 1024 channels)
//   Linear 36864 -> 4096, ReLU, Linear 4096 -> 512, ReLU, Linear 512 -> 2, Softmax(dim 1), view(-1, 1)
// Every GEMM runs on dc_gemm_kernel: a 64x64 MFMA tile (fp16: v_mfma_f32_16x16x32_f16, fp32: exact v_mfma_f32_32x32x2_f32,
// fp32 accumulation) whose operands are gathered by an operation struct (implicit GEMM) and whose epilogue that struct owns:
//   * convolution forward: M = output pixels ordered (image, pooled row, pooled column, 2x2 sub-position), N = Cout,
//     K = 25 Cin (tap-major). The four rows of one pool window are four consecutive accumulator registers of one lane, so
//     bias, ReLU, the 2x2 max pool and its argmax are register-local; only the pooled map and one decision byte per pooled
//     element (sub-position | 4 if the winner was > 0) are stored. Conv 1's row / column 60, which no pool window reads,
//     is never computed.
//   * input gradient: a 5x5 p3 correlation of the pre-pool gradient dZ with the rotated, (o, i)-transposed weights (a second
//     packed copy made at sync_weights). Its epilogue IS the unpooling of the layer below: it writes that layer's dZ
//     (gradient at the argmax position times ReLU', zero at the other three), so no separate scatter pass exists. The
//     same holds for Linear 12's input gradient, which writes conv 3's dZ.
//   * weight gradient: M = Cout, N = 25 Cin, K = pixels, split along K into fixed slices whose fp32 partials one pass adds
//     in slice order (no float atomics: bit-reproducible).
//   * Linear 12 reads the pooled NHWC map directly: its packed copy has its columns in (y, x, c) order.
// The fp16 backward runs on gradients times the loss scale L; fp32 parameter gradients and dx are written times 1/L.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"

namespace {

constexpr int DC_NCONV = 4;
constexpr int DC_CH[5] = {1, 128, 256, 512, 1024};
constexpr int DC_HI[4] = {128, 63, 30, 14};   // input map of conv l
constexpr int DC_HP[4] = {63, 30, 14, 6};     // pooled map of conv l (the conv output rows it reads: 2 HP)
constexpr int DC_F12 = 36864, DC_F14 = 4096, DC_F16 = 512;

int64_t dc_align(int64_t bytes) { return gi_align_up(bytes < 16 ? 16 : bytes, 256); }
int dc_grid1d(int64_t work) { return (int)(work / 256 + 1 < 4096 ? work / 256 + 1 : 4096); }

// ---- 8-element operand pieces ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void dc_zero8(T (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
}
template <typename T>
__device__ __forceinline__ void dc_ld8(const T* __restrict__ p, T (&v)[8]) {   // 16-byte aligned
  if constexpr (sizeof(T) == 2) {
    const u4_t a = *(const u4_t*)p;
    const h8_t h = __builtin_bit_cast(h8_t, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = h[j];
  } else {
    const f4_t a = *(const f4_t*)p, b = *(const f4_t*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
}

template <typename T>
__device__ __forceinline__ void dc_st8(T* p, const T (&v)[8]) {   // 16-byte aligned (LDS)
  if constexpr (sizeof(T) == 2) {
    h8_t h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = v[j];
    *(h8_t*)p = h;
  } else {
    f4_t a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = v[j]; b[j] = v[4 + j]; }
    *(f4_t*)p = a;
    *(f4_t*)(p + 4) = b;
  }
}

// unpool one pooled gradient value into the 2x2 window of the layer's pre-pool gradient dZ (Hz = 2 Hp rows and columns):
// the argmax position gets v if the forward's winner was > 0 (ReLU'), the other three get 0
template <typename T>
__device__ __forceinline__ void dc_unpool(T* __restrict__ dz, const uint8_t* __restrict__ dec, int64_t q, int hp, int c, int ch, float v) {
  const int64_t pix = q / ch;
  const int px = (int)(pix % hp);
  const int64_t t = pix / hp;
  const int py = (int)(t % hp);
  const int64_t img = t / hp;
  const int d = dec[q];
  const int s = d & 3;
  const float g = (d & 4) ? v : 0.f;
  const int hz = 2 * hp;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t o = ((img * hz + 2 * py + (k >> 1)) * hz + 2 * px + (k & 1)) * ch + c;
    dz[o] = (T)(k == s ? g : 0.f);
  }
}

// ---- operations ------------------------------------------------------------------------------------------------------
// a8(m, k0, v): A[m][k0 .. k0+7]; b8(k0, n, v): B[k0 .. k0+7][n] (callers guarantee m < M, n < N; k >= K reads 0)
// store4(m, n, v, rows): rows = valid rows of m .. m+3 (m % 4 == 0); store1(m, n, v): split-K reduction results

// convolution forward + bias + ReLU + 2x2 max pool. TI: the input map's type (fp32 image for conv 0, T after)
template <typename T, typename TI>
struct ConvFwdOp {
  const TI* x; const T* w; const float* bias; T* out; uint8_t* dec;
  int M, N, K, hi, hp, cin;
  __device__ void a8(int m, int k0, T (&v)[8]) const {
    const int q = m >> 2, s = m & 3;
    const int px = q % hp, t = q / hp, py = t % hp, img = t / hp;
    const int oy = 2 * py + (s >> 1), ox = 2 * px + (s & 1);
    if (cin % 8 == 0) {
      const int tap = k0 / cin, ci = k0 - tap * cin;
      const int iy = oy + tap / 5 - 1, ix = ox + tap % 5 - 1;
      if (tap < 25 && iy >= 0 && iy < hi && ix >= 0 && ix < hi) {
        if constexpr (std::is_same<TI, T>::value) dc_ld8(x + (((int64_t)img * hi + iy) * hi + ix) * cin + ci, v);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (T)x[(((int64_t)img * hi + iy) * hi + ix) * cin + ci + j];
        }
      } else dc_zero8(v);
    } else {   // cin == 1: k = tap
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int tap = k0 + j;
        const int iy = oy + tap / 5 - 1, ix = ox + tap % 5 - 1;
        v[j] = (tap < 25 && iy >= 0 && iy < hi && ix >= 0 && ix < hi) ? (T)x[((int64_t)img * hi + iy) * hi + ix] : (T)0.f;
      }
    }
  }
  __device__ void b8(int k0, int n, T (&v)[8]) const {
    if (K % 8 == 0) { dc_ld8(w + (int64_t)n * K + k0, v); return; }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? w[(int64_t)n * K + k0 + j] : (T)0.f;
  }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
    const float b = bias[n];
    int best = 0;
    float z = v[0] + b;
#pragma unroll
    for (int s = 1; s < 4; ++s) {   // first maximum in window order (0,0) (0,1) (1,0) (1,1), as max_pool2d
      const float c = v[s] + b;
      if (c > z) { z = c; best = s; }
    }
    const int64_t q = (int64_t)(m >> 2) * N + n;
    out[q] = (T)(z > 0.f ? z : 0.f);
    dec[q] = (uint8_t)(best | (z > 0.f ? 4 : 0));
  }
  __device__ void store1(int, int, float) const {}
};

// Linear + bias + ReLU on a row-major activation [M][K] and a packed weight [N][K]
template <typename T>
struct LinFwdOp {
  const T* a; const T* w; const float* bias; T* out;
  int M, N, K;
  __device__ void a8(int m, int k0, T (&v)[8]) const { dc_ld8(a + (int64_t)m * K + k0, v); }
  __device__ void b8(int k0, int n, T (&v)[8]) const { dc_ld8(w + (int64_t)n * K + k0, v); }
  __device__ void store1(int m, int n, float v) const {
    v += bias[n];
    out[(int64_t)m * N + n] = (T)(v > 0.f ? v : 0.f);
  }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// Linear 14 input gradient: dh12 = (dh14 W14) * [h12 > 0]; B = the packed transposed copy [4096][512]
template <typename T>
struct Lin14DgradOp {
  const T* d; const T* wt; const T* h; T* out;
  int M, N, K;
  __device__ void a8(int m, int k0, T (&v)[8]) const { dc_ld8(d + (int64_t)m * K + k0, v); }
  __device__ void b8(int k0, int n, T (&v)[8]) const { dc_ld8(wt + (int64_t)n * K + k0, v); }
  __device__ void store1(int m, int n, float v) const {
    const int64_t o = (int64_t)m * N + n;
    out[o] = (T)((float)h[o] > 0.f ? v : 0.f);
  }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// Linear 12 input gradient (K = 4096) with conv 3's unpooling in the epilogue: columns in (y, x, c) order
template <typename T>
struct Lin12DgradOp {
  const T* d; const T* w; T* dz; const uint8_t* dec;
  int M, N, K;
  __device__ void a8(int m, int k0, T (&v)[8]) const { dc_ld8(d + (int64_t)m * K + k0, v); }
  __device__ void b8(int k0, int n, T (&v)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)(k0 + j) * N + n];
  }
  __device__ void store1(int m, int n, float v) const { dc_unpool(dz, dec, (int64_t)m * N + n, 6, n % 1024, 1024, v); }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// parameter gradient of a Linear layer: G[o][i] += inv * sum_rows d[row][o] act[row][i] (K = rows). perm: the weight's
// columns are the NCHW flatten c*36 + s of an activation stored (s, c) (Linear 12)
template <typename T, bool PERM>
struct LinWgradOp {
  const T* d; const T* act; float* g; float inv;
  int M, N, K;
  __device__ void a8(int m, int k0, T (&v)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? d[(int64_t)(k0 + j) * M + m] : (T)0.f;
  }
  __device__ void b8(int k0, int n, T (&v)[8]) const {
    const int col = PERM ? (n % 36) * 1024 + n / 36 : n;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? act[(int64_t)(k0 + j) * N + col] : (T)0.f;
  }
  __device__ void store1(int m, int n, float v) const { g[(int64_t)m * N + n] += v * inv; }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// convolution input gradient: dX[pix][ci] = sum_{tap', co} dZ[pix shifted by tap' - 3][co] Wd[ci][tap'][co], written as the
// pre-pool gradient of the layer below through its decisions (dc_unpool)
template <typename T>
struct ConvDgradOp {
  const T* dz; const T* wd; T* dzp; const uint8_t* decp;
  int M, N, K, hi, hz, cout;
  __device__ void a8(int m, int k0, T (&v)[8]) const {
    const int px = m % hi, t = m / hi, py = t % hi, img = t / hi;
    const int tap = k0 / cout, co = k0 - tap * cout;
    const int zy = py - 3 + tap / 5, zx = px - 3 + tap % 5;
    if (zy >= 0 && zy < hz && zx >= 0 && zx < hz) dc_ld8(dz + (((int64_t)img * hz + zy) * hz + zx) * cout + co, v);
    else dc_zero8(v);
  }
  __device__ void b8(int k0, int n, T (&v)[8]) const { dc_ld8(wd + (int64_t)n * K + k0, v); }
  __device__ void store1(int m, int n, float v) const { dc_unpool(dzp, decp, (int64_t)m * N + n, hi, n, N, v); }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// convolution weight gradient: dW[co][tap][ci] += inv * sum_pix dZ[pix][co] X[pix shifted by tap - 1][ci] (K = pixels of the
// hz x hz pre-pool grid). Always split along K: store1 receives the fixed-order sum of the slices
template <typename T, typename TI>
struct ConvWgradOp {
  const T* dz; const TI* x; float* g; float inv;
  int M, N, K, hi, hz, cin;
  __device__ void a8(int m, int k0, T (&v)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? dz[(int64_t)(k0 + j) * M + m] : (T)0.f;
  }
  __device__ void b8(int k0, int n, T (&v)[8]) const {
    const int tap = n / cin, ci = n - tap * cin, ky = tap / 5 - 1, kx = tap % 5 - 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = k0 + j;
      const int ox = p % hz, t = p / hz, oy = t % hz, img = t / hz;
      const int iy = oy + ky, ix = ox + kx;
      v[j] = (p < K && iy >= 0 && iy < hi && ix >= 0 && ix < hi) ? (T)x[(((int64_t)img * hi + iy) * hi + ix) * cin + ci] : (T)0.f;
    }
  }
  __device__ void store1(int m, int n, float v) const { g[(int64_t)m * N + n] += v * inv; }
  __device__ void store4(int m, int n, const float (&v)[4], int rows) const {
#pragma unroll
    for (int r = 0; r < 4; ++r) if (r < rows) store1(m + r, n, v[r]);
  }
};

// ---- the GEMM ----------------------------------------------------------------------------------------------------------
// 64 x 64 tile, K step 32, four waves of 32 x 32. blockIdx.z = K slice of kt_split steps; part != null: the slice's fp32
// partial goes to part[z][M][N] (dc_splitk_reduce adds the slices in order), else the operation's epilogue runs.
constexpr int DC_BM = 64, DC_BN = 64, DC_BK = 32;

template <typename T, class Op>
__global__ void __launch_bounds__(256) dc_gemm_kernel(Op op, float* __restrict__ part, int kt_split) {
  constexpr bool F16 = std::is_same<T, half_t>::value;
  constexpr int LDK = F16 ? 40 : 36;   // LDS row stride (elements): 16-byte aligned rows
  constexpr int WM = DC_BM / 2, WN = DC_BN / 2;
  constexpr int AC = DC_BM * 4 / 256, BC = DC_BN * 4 / 256;   // 8-element chunks per thread
  __shared__ __attribute__((aligned(16))) T sA[DC_BM * LDK];
  __shared__ __attribute__((aligned(16))) T sB[DC_BN * LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * DC_BM, n0 = blockIdx.y * DC_BN;
  const int nkt = (op.K + DC_BK - 1) / DC_BK;
  const int kt0 = blockIdx.z * kt_split;
  const int kt1 = min(nkt, kt0 + kt_split);

  T ra[AC][8], rb[BC][8];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const int c = tid + 256 * i, row = c % DC_BM, kc = c / DC_BM;
      if (m0 + row < op.M) op.a8(m0 + row, kt * DC_BK + kc * 8, ra[i]);
      else dc_zero8(ra[i]);
    }
#pragma unroll
    for (int i = 0; i < BC; ++i) {
      const int c = tid + 256 * i, col = c % DC_BN, kc = c / DC_BN;
      if (n0 + col < op.N) op.b8(kt * DC_BK + kc * 8, n0 + col, rb[i]);
      else dc_zero8(rb[i]);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const int c = tid + 256 * i, row = c % DC_BM, kc = c / DC_BM;
      dc_st8(&sA[row * LDK + kc * 8], ra[i]);
    }
#pragma unroll
    for (int i = 0; i < BC; ++i) {
      const int c = tid + 256 * i, col = c % DC_BN, kc = c / DC_BN;
      dc_st8(&sB[col * LDK + kc * 8], rb[i]);
    }
  };

  constexpr int MT = F16 ? WM / 16 : WM / 32, NT = F16 ? WN / 16 : WN / 32;
  using acc_t = typename std::conditional<F16, f4_t, f16_t>::type;
  acc_t acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < (F16 ? 4 : 16); ++r) acc[i][j][r] = 0.f;

  if (kt0 < kt1) gload(kt0);
  for (int kt = kt0; kt < kt1; ++kt) {
    __syncthreads();
    lstore();
    __syncthreads();
    if (kt + 1 < kt1) gload(kt + 1);   // next step's loads in flight during the MFMAs
    if constexpr (F16) {
      h8_t af[MT], bf[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[mt] = *(const h8_t*)&sA[(wm * WM + mt * 16 + (lane & 15)) * LDK + (lane >> 4) * 8];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[nt] = *(const h8_t*)&sB[(wn * WN + nt * 16 + (lane & 15)) * LDK + (lane >> 4) * 8];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
    } else {
#pragma unroll 4
      for (int kk = 0; kk < DC_BK / 2; ++kk) {
        float af[MT], bf[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = sA[(wm * WM + mt * 32 + (lane & 31)) * LDK + 2 * kk + (lane >> 5)];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[nt] = sB[(wn * WN + nt * 32 + (lane & 31)) * LDK + 2 * kk + (lane >> 5)];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
      }
    }
  }

  // epilogue: every lane holds groups of 4 consecutive rows of one column
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < (F16 ? 1 : 4); ++g) {
        int row, col;
        if constexpr (F16) { row = wm * WM + mt * 16 + (lane >> 4) * 4; col = wn * WN + nt * 16 + (lane & 15); }
        else { row = wm * WM + mt * 32 + 8 * g + 4 * (lane >> 5); col = wn * WN + nt * 32 + (lane & 31); }
        const int m = m0 + row, n = n0 + col;
        if (m >= op.M || n >= op.N) continue;
        const float v[4] = {acc[mt][nt][4 * g], acc[mt][nt][4 * g + 1], acc[mt][nt][4 * g + 2], acc[mt][nt][4 * g + 3]};
        const int rows = min(4, op.M - m);
        if (part) {
          float* p = part + ((int64_t)blockIdx.z * op.M + m) * op.N + n;
#pragma unroll
          for (int r = 0; r < 4; ++r) if (r < rows) p[(int64_t)r * op.N] = v[r];
        } else op.store4(m, n, v, rows);
      }
}

template <class Op>
__global__ void __launch_bounds__(256) dc_splitk_reduce_kernel(Op op, const float* __restrict__ part, int splits) {
  const int64_t total = (int64_t)op.M * op.N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[z * total + i];
    op.store1((int)(i / op.N), (int)(i % op.N), s);
  }
}

template <typename T, class Op>
int dc_gemm(hipStream_t st, const Op& op, float* part, int splits, const char* name) {
  const int nkt = (op.K + DC_BK - 1) / DC_BK;
  if (splits < 1) splits = 1;
  if (splits > nkt) splits = nkt;
  const int kt_split = (nkt + splits - 1) / splits;
  splits = (nkt + kt_split - 1) / kt_split;
  const dim3 grid((op.M + DC_BM - 1) / DC_BM, (op.N + DC_BN - 1) / DC_BN, splits);
  hipLaunchKernelGGL((dc_gemm_kernel<T, Op>), grid, dim3(256), 0, st, op, splits > 1 ? part : nullptr, kt_split);
  GI_LAUNCH_CHECK();
  if (splits > 1) {
    hipLaunchKernelGGL((dc_splitk_reduce_kernel<Op>), dim3(dc_grid1d((int64_t)op.M * op.N)), dim3(256), 0, st, op, (const float*)part, splits);
    GI_LAUNCH_CHECK();
  }
  gi_note_kernel(name);
  return GI_OK;
}

// ---- small kernels -----------------------------------------------------------------------------------------------------
// Linear 16 + Softmax(dim 1): one block per row, fp32; y[2 r + j] = p_j, probabilities kept for the backward
template <typename T>
__global__ void __launch_bounds__(256) dc_head_fwd_kernel(const T* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ prob, float* __restrict__ y) {
  __shared__ float red[2][256];
  const int r = blockIdx.x, t = threadIdx.x;
  float s0 = 0.f, s1 = 0.f;
  for (int k = t; k < DC_F16; k += 256) {
    const float v = (float)h[(int64_t)r * DC_F16 + k];
    s0 = fmaf(v, w[k], s0);
    s1 = fmaf(v, w[DC_F16 + k], s1);
  }
  red[0][t] = s0; red[1][t] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    const float l0 = red[0][0] + b[0], l1 = red[1][0] + b[1];
    const float mx = fmaxf(l0, l1);
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
    const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
    prob[2 * r] = p0; prob[2 * r + 1] = p1;
    y[2 * r] = p0; y[2 * r + 1] = p1;
  }
}

// softmax + Linear 16 backward, one thread per input feature k: dlogit_0 = p_0 p_1 (dy_0 - dy_1) = -dlogit_1, the two-class form of
// p_j (dy_j - sum p dy) without its cancellation (p_0 + p_1 rounds away from 1 in fp32), unscaled fp32;
// dh14[r][k] = L * sum_j dlogit_j W16[j][k] * [h14 > 0]; dW16 / db16 accumulate over the rows in order
template <typename T>
__global__ void __launch_bounds__(256) dc_head_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ dy, const T* __restrict__ h,
                                                          const float* __restrict__ w, T* __restrict__ dh, float* __restrict__ gw,
                                                          float* __restrict__ gb, int n, float L, int need_wgrad) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= DC_F16) return;
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
  for (int r = 0; r < n; ++r) {
    const float p0 = prob[2 * r], p1 = prob[2 * r + 1], g0 = dy[2 * r], g1 = dy[2 * r + 1];
    const float d0 = p0 * p1 * (g0 - g1), d1 = -d0;
    const float hv = (float)h[(int64_t)r * DC_F16 + k];
    dh[(int64_t)r * DC_F16 + k] = (T)(hv > 0.f ? L * (d0 * w[k] + d1 * w[DC_F16 + k]) : 0.f);
    a0 = fmaf(d0, hv, a0); a1 = fmaf(d1, hv, a1);
    b0 += d0; b1 += d1;
  }
  if (need_wgrad) {
    gw[k] += a0; gw[DC_F16 + k] += a1;
    if (k == 0) { gb[0] += b0; gb[1] += b1; }
  }
}

// bias gradient: g[c] += inv * sum_rows d[row][c], in two fixed-order stages (row chunks, then the chunks in order)
template <typename T>
__global__ void __launch_bounds__(256) dc_colsum_part_kernel(const T* __restrict__ d, int64_t rows, int cols, int64_t chunk, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float s = 0.f;
  for (int64_t r = r0; r < r1; ++r) s += (float)d[r * cols + c];
  part[(int64_t)blockIdx.y * cols + c] = s;
}
__global__ void __launch_bounds__(256) dc_colsum_fin_kernel(const float* __restrict__ part, int chunks, int cols, float inv, float* __restrict__ g) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int i = 0; i < chunks; ++i) s += part[(int64_t)i * cols + c];
  g[c] += s * inv;
}

// conv 0 input gradient (1 output channel): dx[img][y][x] = inv * sum_{tap, co} dZ0[img][y + 1 - ky][x + 1 - kx][co] W0[co][tap]
template <typename T>
__global__ void __launch_bounds__(256) dc_conv0_dgrad_kernel(const T* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx, int n,
                                                             float inv) {
  __shared__ float sw[25 * 128];
  for (int i = threadIdx.x; i < 25 * 128; i += 256) sw[(i % 25) * 128 + i / 25] = w[i];   // [tap][co]
  __syncthreads();
  const int64_t total = (int64_t)n * 128 * 128;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % 128), y = (int)((i / 128) % 128);
    const int64_t img = i / (128 * 128);
    float s = 0.f;
    for (int tap = 0; tap < 25; ++tap) {
      const int zy = y + 1 - tap / 5, zx = x + 1 - tap % 5;
      if (zy < 0 || zy >= 126 || zx < 0 || zx >= 126) continue;
      const T* p = dz + ((img * 126 + zy) * 126 + zx) * 128;
      for (int co = 0; co < 128; ++co) s = fmaf((float)p[co], sw[tap * 128 + co], s);
    }
    dx[i] = s * inv;
  }
}

// ---- weight packing (sync_weights) -------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) dc_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = (T)src[i];
}
// Wd[ci][tap'][co] = W[co][24 - tap'][ci]
template <typename T>
__global__ void __launch_bounds__(256) dc_pack_dgrad_kernel(const float* __restrict__ w, T* __restrict__ wd, int cout, int cin) {
  const int64_t total = (int64_t)cout * 25 * cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int co = (int)(i % cout);
    const int64_t t = i / cout;
    const int tp = (int)(t % 25), ci = (int)(t / 25);
    wd[i] = (T)w[((int64_t)co * 25 + 24 - tp) * cin + ci];
  }
}
// Linear 12: Wp[j][s * 1024 + c] = W[j][c * 36 + s]
template <typename T>
__global__ void __launch_bounds__(256) dc_pack_l12_kernel(const float* __restrict__ w, T* __restrict__ wp) {
  const int64_t total = (int64_t)DC_F14 * DC_F12;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t j = i / DC_F12;
    const int col = (int)(i % DC_F12);
    wp[i] = (T)w[j * DC_F12 + (col % 1024) * 36 + col / 1024];
  }
}
// Linear 14 transposed: Wt[k][o] = W[o][k]
template <typename T>
__global__ void __launch_bounds__(256) dc_pack_l14t_kernel(const float* __restrict__ w, T* __restrict__ wt) {
  const int64_t total = (int64_t)DC_F16 * DC_F14;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i % DC_F16);
    const int64_t k = i / DC_F16;
    wt[i] = (T)w[(int64_t)o * DC_F14 + k];
  }
}

// NHWC (pixels x c) -> fp32 (n, c, hw)
template <typename S>
__global__ void __launch_bounds__(256) dc_export_kernel(const S* __restrict__ src, float* __restrict__ out, int n, int c, int hw) {
  const int64_t total = (int64_t)n * c * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % hw);
    const int64_t t = i / hw;
    const int ch = (int)(t % c);
    const int64_t img = t / c;
    out[i] = (float)src[(img * hw + p) * c + ch];
  }
}

}  // namespace

// =================================================================================================
// state
// =================================================================================================
struct gi_dcgan {
  int dtype = GI_F32, max_n = 0, n_slots = 1;
  // parameter offsets (floats into the flat buffers)
  int64_t w_off[4], b_off[4], w12 = -1, b12 = -1, w14 = -1, b14 = -1, w16 = -1, b16 = -1;
  // shared workspace: packed weights (fp16: forward copies of the convs, Linear 14; both dtypes: the convs' input-gradient
  // copies, Linear 12 in (y, x, c) column order, Linear 14 transposed), backward scratch
  int64_t oWf[4] = {-1, -1, -1, -1}, oWd[4] = {-1, -1, -1, -1}, oW12 = -1, oW14 = -1, oW14t = -1;
  int64_t oDZ[4] = {-1, -1, -1, -1}, oDH12 = -1, oDH14 = -1, oPart = -1, part_floats = 0, oCol = -1;
  // per slot: input image, pooled maps + decisions, Linear activations, probabilities
  int64_t sX = -1, sP[4], sDec[4], sH12 = -1, sH14 = -1, sProb = -1, slot_bytes = 0, slot_base = 0, ws_bytes = 0;
  std::vector<int> slot_n;
  int splits[4] = {1, 1, 1, 1};
  size_t tsz() const { return gi_dtype_size(dtype); }
};

namespace {
constexpr int DC_COL_CHUNKS = 256;

int dc_wgrad_splits(int64_t m, int64_t n) {   // ~2048 workgroups per weight-gradient GEMM
  const int64_t tiles = ((m + DC_BM - 1) / DC_BM) * ((n + DC_BN - 1) / DC_BN);
  const int64_t s = (2048 + tiles - 1) / tiles;
  return (int)(s < 1 ? 1 : s);
}

template <typename T>
int dc_colsum(hipStream_t st, const gi_dcgan* dc, char* ws, const T* d, int64_t rows, int cols, float inv, float* g) {
  const int64_t chunk = (rows + DC_COL_CHUNKS - 1) / DC_COL_CHUNKS;
  const int chunks = (int)((rows + chunk - 1) / chunk);
  float* part = (float*)(ws + dc->oCol);
  hipLaunchKernelGGL(dc_colsum_part_kernel<T>, dim3((cols + 255) / 256, chunks), dim3(256), 0, st, d, rows, cols, chunk, part);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(dc_colsum_fin_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, (const float*)part, chunks, cols, inv, g);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

template <typename T>
const T* dc_fwd_weight(const gi_dcgan* dc, const float* params, char* ws, int l) {
  if constexpr (std::is_same<T, float>::value) return params + dc->w_off[l];
  else return (const T*)(ws + dc->oWf[l]);
}

template <typename T>
int dc_sync_t(gi_dcgan* dc, hipStream_t st, const float* params, char* ws) {
  for (int l = 0; l < DC_NCONV; ++l) {
    const int64_t cnt = (int64_t)DC_CH[l + 1] * 25 * DC_CH[l];
    if (dc->oWf[l] >= 0) {
      hipLaunchKernelGGL(dc_cast_kernel<T>, dim3(dc_grid1d(cnt)), dim3(256), 0, st, params + dc->w_off[l], (T*)(ws + dc->oWf[l]), cnt);
      GI_LAUNCH_CHECK();
    }
    if (dc->oWd[l] >= 0) {
      hipLaunchKernelGGL(dc_pack_dgrad_kernel<T>, dim3(dc_grid1d(cnt)), dim3(256), 0, st, params + dc->w_off[l], (T*)(ws + dc->oWd[l]),
                         DC_CH[l + 1], DC_CH[l]);
      GI_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(dc_pack_l12_kernel<T>, dim3(4096), dim3(256), 0, st, params + dc->w12, (T*)(ws + dc->oW12));
  GI_LAUNCH_CHECK();
  if (dc->oW14 >= 0) {
    hipLaunchKernelGGL(dc_cast_kernel<T>, dim3(dc_grid1d((int64_t)DC_F16 * DC_F14)), dim3(256), 0, st, params + dc->w14, (T*)(ws + dc->oW14),
                       (int64_t)DC_F16 * DC_F14);
    GI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(dc_pack_l14t_kernel<T>, dim3(dc_grid1d((int64_t)DC_F16 * DC_F14)), dim3(256), 0, st, params + dc->w14, (T*)(ws + dc->oW14t));
  GI_LAUNCH_CHECK();
  return GI_OK;
}

template <typename T>
int dc_forward_t(gi_dcgan* dc, hipStream_t st, const float* params, char* ws, int slot, const float* x, float* y, int n, bool convs_only = false) {
  char* sb = ws + dc->slot_base + (int64_t)slot * dc->slot_bytes;
  float* x0 = (float*)(sb + dc->sX);
  GI_HIP(hipMemcpyAsync(x0, x, (size_t)n * 128 * 128 * 4, hipMemcpyDeviceToDevice, st));
  {
    ConvFwdOp<T, float> op{x0, dc_fwd_weight<T>(dc, params, ws, 0), params + dc->b_off[0], (T*)(sb + dc->sP[0]), (uint8_t*)(sb + dc->sDec[0]),
                           n * DC_HP[0] * DC_HP[0] * 4, DC_CH[1], 25, DC_HI[0], DC_HP[0], 1};
    GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_conv_fwd"));
  }
  for (int l = 1; l < DC_NCONV; ++l) {
    ConvFwdOp<T, T> op{(const T*)(sb + dc->sP[l - 1]), dc_fwd_weight<T>(dc, params, ws, l), params + dc->b_off[l], (T*)(sb + dc->sP[l]),
                       (uint8_t*)(sb + dc->sDec[l]), n * DC_HP[l] * DC_HP[l] * 4, DC_CH[l + 1], 25 * DC_CH[l], DC_HI[l], DC_HP[l], DC_CH[l]};
    GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_conv_fwd"));
  }
  if (convs_only) return GI_OK;
  float* part = (float*)(ws + dc->oPart);
  {   // Linear 12: K = 36864 split into slices (M = rows is small), epilogue after the fixed-order reduction
    LinFwdOp<T> op{(const T*)(sb + dc->sP[3]), (const T*)(ws + dc->oW12), params + dc->b12, (T*)(sb + dc->sH12), n, DC_F14, DC_F12};
    int s = 16;
    while (s > 1 && (int64_t)s * n * DC_F14 > dc->part_floats) s >>= 1;
    GI_TRY(dc_gemm<T>(st, op, part, s, "dc_linear_fwd"));
  }
  {
    const T* w14 = std::is_same<T, float>::value ? (const T*)(params + dc->w14) : (const T*)(ws + dc->oW14);
    LinFwdOp<T> op{(const T*)(sb + dc->sH12), w14, params + dc->b14, (T*)(sb + dc->sH14), n, DC_F16, DC_F14};
    GI_TRY(dc_gemm<T>(st, op, part, 8, "dc_linear_fwd"));
  }
  hipLaunchKernelGGL(dc_head_fwd_kernel<T>, dim3(n), dim3(256), 0, st, (const T*)(sb + dc->sH14), params + dc->w16, params + dc->b16,
                     (float*)(sb + dc->sProb), y);
  GI_LAUNCH_CHECK();
  dc->slot_n[slot] = n;
  return GI_OK;
}

// phase 0: everything; 1: softmax .. Linear 12 (their gradients are [w12, end) of the flat buffer) and conv 3's dZ;
// 2: conv 3 .. conv 0 from that dZ
template <typename T>
int dc_backward_t(gi_dcgan* dc, hipStream_t st, const float* params, float* grads, char* ws, int slot, const float* dy, float* dx,
                  int need_wgrad, float L, int phase) {
  const int n = dc->slot_n[slot];
  GI_REQUIRE(n > 0, "dcgan backward: slot %d holds no forward", slot);
  char* sb = ws + dc->slot_base + (int64_t)slot * dc->slot_bytes;
  const float inv = 1.f / L;
  float* part = (float*)(ws + dc->oPart);
  T* dh14 = (T*)(ws + dc->oDH14);
  T* dh12 = (T*)(ws + dc->oDH12);
  const T* h12 = (const T*)(sb + dc->sH12);
  const T* h14 = (const T*)(sb + dc->sH14);
  if (phase != 2) {
    hipLaunchKernelGGL(dc_head_bwd_kernel<T>, dim3(DC_F16 / 256), dim3(256), 0, st, (const float*)(sb + dc->sProb), dy, h14, params + dc->w16, dh14,
                       grads + dc->w16, grads + dc->b16, n, L, need_wgrad);
    GI_LAUNCH_CHECK();
    {
      Lin14DgradOp<T> op{dh14, (const T*)(ws + dc->oW14t), h12, dh12, n, DC_F14, DC_F16};
      GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_linear_dgrad"));
    }
    if (need_wgrad) {
      LinWgradOp<T, false> op{dh14, h12, grads + dc->w14, inv, DC_F16, DC_F14, n};
      GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_linear_wgrad"));
      GI_TRY(dc_colsum<T>(st, dc, ws, dh14, n, DC_F16, inv, grads + dc->b14));
    }
    {
      Lin12DgradOp<T> op{dh12, (const T*)(ws + dc->oW12), (T*)(ws + dc->oDZ[3]), (const uint8_t*)(sb + dc->sDec[3]), n, DC_F12, DC_F14};
      GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_linear_dgrad"));
    }
    if (need_wgrad) {
      LinWgradOp<T, true> op{dh12, (const T*)(sb + dc->sP[3]), grads + dc->w12, inv, DC_F14, DC_F12, n};
      GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_linear_wgrad"));
      GI_TRY(dc_colsum<T>(st, dc, ws, dh12, n, DC_F14, inv, grads + dc->b12));
    }
  }
  if (phase == 1) return GI_OK;
  for (int l = DC_NCONV - 1; l >= 0; --l) {
    const int hz = 2 * DC_HP[l], cout = DC_CH[l + 1], cin = DC_CH[l];
    const T* dz = (const T*)(ws + dc->oDZ[l]);
    if (need_wgrad) {
      const int64_t pix = (int64_t)n * hz * hz;
      if (l == 0) {
        ConvWgradOp<T, float> op{dz, (const float*)(sb + dc->sX), grads + dc->w_off[0], inv, cout, 25, (int)pix, DC_HI[0], hz, 1};
        GI_TRY(dc_gemm<T>(st, op, part, dc->splits[0], "dc_conv_wgrad"));
      } else {
        ConvWgradOp<T, T> op{dz, (const T*)(sb + dc->sP[l - 1]), grads + dc->w_off[l], inv, cout, 25 * cin, (int)pix, DC_HI[l], hz, cin};
        GI_TRY(dc_gemm<T>(st, op, part, dc->splits[l], "dc_conv_wgrad"));
      }
      GI_TRY(dc_colsum<T>(st, dc, ws, dz, pix, cout, inv, grads + dc->b_off[l]));
    }
    if (l > 0) {
      ConvDgradOp<T> op{dz, (const T*)(ws + dc->oWd[l]), (T*)(ws + dc->oDZ[l - 1]), (const uint8_t*)(sb + dc->sDec[l - 1]),
                        n * DC_HI[l] * DC_HI[l], cin, 25 * cout, DC_HI[l], hz, cout};
      GI_TRY(dc_gemm<T>(st, op, nullptr, 1, "dc_conv_dgrad"));
    } else if (dx) {
      hipLaunchKernelGGL(dc_conv0_dgrad_kernel<T>, dim3(dc_grid1d((int64_t)n * 128 * 128)), dim3(256), 0, st, dz, params + dc->w_off[0], dx, n, inv);
      GI_LAUNCH_CHECK();
    }
  }
  return GI_OK;
}
}  // namespace

// =================================================================================================
// entry points used by net.hip's generic gi_net_* functions (kind 2)
// =================================================================================================
struct gi_net;
gi_net* gi_net_new_dcgan(gi_ctx* ctx, int dtype, int max_n, int n_slots, gi_dcgan* dc);
void gi_net_add_param(gi_net* net, const char* name, int kind, const int64_t* shape, int ndim, int64_t* off);
void gi_net_set_workspace(gi_net* net, int64_t bytes);
gi_dcgan* gi_net_dcgan_state(gi_net* net);
void gi_net_dcgan_bound(gi_net* net, hipStream_t* st, const float** params, char** ws);

void gi_dcgan_free(gi_dcgan* dc) { delete dc; }

int gi_dcgan_sync(gi_dcgan* dc, hipStream_t st, const float* params, char* ws) {
  return dc->dtype == GI_F16 ? dc_sync_t<half_t>(dc, st, params, ws) : dc_sync_t<float>(dc, st, params, ws);
}
int gi_dcgan_forward(gi_dcgan* dc, hipStream_t st, const float* params, char* ws, int slot, const float* x, float* y, int n) {
  return dc->dtype == GI_F16 ? dc_forward_t<half_t>(dc, st, params, ws, slot, x, y, n) : dc_forward_t<float>(dc, st, params, ws, slot, x, y, n);
}
int gi_dcgan_backward(gi_dcgan* dc, hipStream_t st, const float* params, float* grads, char* ws, int slot, const float* dy, float* dx,
                      int need_wgrad, float loss_scale, int phase) {
  return dc->dtype == GI_F16 ? dc_backward_t<half_t>(dc, st, params, grads, ws, slot, dy, dx, need_wgrad, loss_scale, phase)
                             : dc_backward_t<float>(dc, st, params, grads, ws, slot, dy, dx, need_wgrad, loss_scale, phase);
}
int64_t gi_dcgan_phase_split(gi_dcgan* dc) { return dc->w12; }

// Debug: the four convolution blocks of a forward only (the slot is left without a complete forward)
extern "C" int gi_dcgan_debug_forward_convs(gi_net* net, int slot, const float* x, int n) {
  gi_dcgan* dc = gi_net_dcgan_state(net);
  GI_REQUIRE(dc && x && n >= 1 && n <= dc->max_n && slot >= 0 && slot < dc->n_slots, "dcgan_debug_forward_convs: bound DCGAN handle, n=%d", n);
  hipStream_t st;
  const float* params;
  char* ws;
  gi_net_dcgan_bound(net, &st, &params, &ws);
  GI_REQUIRE(ws, "dcgan_debug_forward_convs: net not bound");
  dc->slot_n[slot] = 0;
  return dc->dtype == GI_F16 ? dc_forward_t<half_t>(dc, st, params, ws, slot, x, nullptr, n, true)
                             : dc_forward_t<float>(dc, st, params, ws, slot, x, nullptr, n, true);
}

// kind 0: pooled map of conv `level` (1..4), (n, C, h, w); kind 1: its pool decisions (sub-position + 4 if the winning
// pre-activation was > 0); kind 2: level 1 = ReLU(Linear 12) (n, 4096), level 2 = ReLU(Linear 14) (n, 512), level 3 = the
// softmax probabilities (n, 2)
int gi_dcgan_saved(gi_dcgan* dc, hipStream_t st, char* ws, int slot, int kind, int level, float* out, int64_t count) {
  const int n = dc->slot_n[slot];
  GI_REQUIRE(n > 0, "saved_activation: slot %d holds no forward", slot);
  char* sb = ws + dc->slot_base + (int64_t)slot * dc->slot_bytes;
  int c = 0, hw = 0;
  const void* src = nullptr;
  bool bytes = false, f32 = false;
  if ((kind == 0 || kind == 1) && level >= 1 && level <= 4) {
    c = DC_CH[level]; hw = DC_HP[level - 1] * DC_HP[level - 1];
    src = sb + (kind == 0 ? dc->sP[level - 1] : dc->sDec[level - 1]);
    bytes = kind == 1;
  } else if (kind == 2 && level >= 1 && level <= 3) {
    c = level == 1 ? DC_F14 : (level == 2 ? DC_F16 : 2); hw = 1;
    src = sb + (level == 1 ? dc->sH12 : (level == 2 ? dc->sH14 : dc->sProb));
    f32 = level == 3;
  } else {
    GI_REQUIRE(false, "saved_activation: DCGAN kind=%d level=%d (kinds 0 / 1: levels 1..4, kind 2: levels 1..3)", kind, level);
  }
  GI_REQUIRE(count == (int64_t)n * c * hw, "saved_activation: count %lld != %lld", (long long)count, (long long)n * c * hw);
  const dim3 g(dc_grid1d(count));
  if (bytes) hipLaunchKernelGGL(dc_export_kernel<uint8_t>, g, dim3(256), 0, st, (const uint8_t*)src, out, n, c, hw);
  else if (f32 || dc->dtype == GI_F32) hipLaunchKernelGGL(dc_export_kernel<float>, g, dim3(256), 0, st, (const float*)src, out, n, c, hw);
  else hipLaunchKernelGGL(dc_export_kernel<half_t>, g, dim3(256), 0, st, (const half_t*)src, out, n, c, hw);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

extern "C" int gi_dcgan_create(gi_ctx* ctx, int H, int W, int max_n, int dtype, int n_slots, gi_net** out) {
  GI_REQUIRE(out, "dcgan_create: null argument");   // ctx may be null: inventory-only handle
  GI_REQUIRE(dtype == GI_F16 || dtype == GI_F32, "dcgan_create: dtype=%d", dtype);
  GI_REQUIRE(H == 128 && W == 128,
             "dcgan_create: H=%d W=%d: the network's first Linear takes 36864 = 1024*6*6 inputs, which only a 128x128 image gives", H, W);
  GI_REQUIRE(max_n >= 1 && max_n <= 4096 && n_slots >= 1 && n_slots <= 8, "dcgan_create: max_n=%d n_slots=%d", max_n, n_slots);
  gi_dcgan* dc = new gi_dcgan();
  dc->dtype = dtype; dc->max_n = max_n; dc->n_slots = n_slots;
  gi_net* net = gi_net_new_dcgan(ctx, dtype, max_n, n_slots, dc);
  for (int l = 0; l < DC_NCONV; ++l) {
    const std::string p = "model." + std::to_string(3 * l);
    const int64_t ws_[4] = {DC_CH[l + 1], DC_CH[l], 5, 5}, bs[1] = {DC_CH[l + 1]};
    gi_net_add_param(net, (p + ".weight").c_str(), 0, ws_, 4, &dc->w_off[l]);
    gi_net_add_param(net, (p + ".bias").c_str(), 1, bs, 1, &dc->b_off[l]);
  }
  const int64_t s12[2] = {DC_F14, DC_F12}, s14[2] = {DC_F16, DC_F14}, s16[2] = {2, DC_F16};
  const int64_t b12[1] = {DC_F14}, b14[1] = {DC_F16}, b16[1] = {2};
  gi_net_add_param(net, "model.12.weight", 1, s12, 2, &dc->w12);
  gi_net_add_param(net, "model.12.bias", 1, b12, 1, &dc->b12);
  gi_net_add_param(net, "model.14.weight", 1, s14, 2, &dc->w14);
  gi_net_add_param(net, "model.14.bias", 1, b14, 1, &dc->b14);
  gi_net_add_param(net, "model.16.weight", 1, s16, 2, &dc->w16);
  gi_net_add_param(net, "model.16.bias", 1, b16, 1, &dc->b16);

  const int64_t T = (int64_t)dc->tsz(), N = max_n;
  int64_t A = 0;
  auto take = [&](int64_t bytes) { const int64_t o = A; A += dc_align(bytes); return o; };
  for (int l = 0; l < DC_NCONV; ++l) {
    const int64_t cnt = (int64_t)DC_CH[l + 1] * 25 * DC_CH[l];
    if (dtype == GI_F16) dc->oWf[l] = take(cnt * T);
    if (l > 0) dc->oWd[l] = take(cnt * T);
    dc->oDZ[l] = take(N * 4 * DC_HP[l] * DC_HP[l] * DC_CH[l + 1] * T);
  }
  dc->oW12 = take((int64_t)DC_F14 * DC_F12 * T);
  if (dtype == GI_F16) dc->oW14 = take((int64_t)DC_F16 * DC_F14 * T);
  dc->oW14t = take((int64_t)DC_F16 * DC_F14 * T);
  dc->oDH12 = take(N * DC_F14 * T);
  dc->oDH14 = take(N * DC_F16 * T);
  int64_t pf = 16 * N * DC_F14;   // Linear 12's K slices
  for (int l = 0; l < DC_NCONV; ++l) {
    const int64_t m = DC_CH[l + 1], nn = 25 * DC_CH[l];
    dc->splits[l] = dc_wgrad_splits(m, nn);
    pf = std::max(pf, (int64_t)dc->splits[l] * m * nn);
  }
  dc->part_floats = pf;
  dc->oPart = take(pf * 4);
  dc->oCol = take((int64_t)DC_COL_CHUNKS * 4096 * 4);
  int64_t S = 0;
  auto stake = [&](int64_t bytes) { const int64_t o = S; S += dc_align(bytes); return o; };
  dc->sX = stake(N * 128 * 128 * 4);
  for (int l = 0; l < DC_NCONV; ++l) {
    const int64_t e = N * DC_HP[l] * DC_HP[l] * DC_CH[l + 1];
    dc->sP[l] = stake(e * T);
    dc->sDec[l] = stake(e);
  }
  dc->sH12 = stake(N * DC_F14 * T);
  dc->sH14 = stake(N * DC_F16 * T);
  dc->sProb = stake(N * 2 * 4);
  dc->slot_bytes = S;
  dc->slot_base = A;
  A += S * n_slots;
  dc->ws_bytes = A;
  dc->slot_n.assign(n_slots, 0);
  gi_net_set_workspace(net, A);
  *out = net;
  return GI_OK;
}
