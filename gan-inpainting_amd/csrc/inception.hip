// Inception-V3 pool3 features for the Frechet Inception Distance (reference lib/fid/inception.py: the FID variant of the
// network, output block 3 = the 2048-wide global average) and the streaming fp64 mean / covariance of those features
// (reference lib/fid/fid_score.py calculate_activation_statistics).
//
// Forward only. Activations are NHWC in the compute type T (fp16 or fp32):
//   inc_input_kernel    bilinear resize to 299x299 (align_corners = False, no antialiasing) and 2x - 1, NCHW fp32 -> NHWC with the
//                       3 channels padded to 8 (zeros; one input channel is replicated), so every convolution reads 8-element chunks
//   inc_gemm_kernel     ONE implicit-GEMM template for all 94 convolutions: M = output pixels, N = Cout, K = kh kw Cin (tap-major),
//                       64 x 64 tile, K step 32, four waves of 32 x 32 (fp16: v_mfma_f32_16x16x32_f16, fp32: v_mfma_f32_32x32x2_f32,
//                       fp32 accumulation). Kernel size, stride and padding are run-time arguments; the taps are walked incrementally
//                       (no division in the K loop). PW = true is the 1x1 / stride 1 form whose A rows are the pixels themselves.
//                       BatchNorm (running statistics, eps 0.001) is folded into weight and bias at sync_weights, in fp32, before the
//                       weights are rounded to T; the epilogue adds the bias, applies ReLU and writes at the branch's channel offset of
//                       the block's concatenated output (ldout / coffout), so no concatenation pass exists. Rows >= M, columns >= N
//                       and k >= K are zero-filled on load and skipped on store: 147, 73, 71, 35, 17, 8 and 48 / 80 / 320 need no padding.
//   inc_maxpool3s2_kernel, inc_pool3s1_kernel (average without the padding in the divisor, or max), inc_gap_kernel: separate NHWC
//                       kernels, 8 channels per thread.
//   fid_sum_kernel / fid_xtx_kernel / fid_finish_kernel: sum and X^T X in fp64, every element accumulated over the rows in arrival order
//                       by ONE thread (fma chain continued from the accumulator), so the bits depend neither on the launch geometry nor
//                       on how the rows were split into calls.
#include <new>
#include <string>
#include <vector>

#include "common.h"

namespace {

constexpr int INC_HW = 299;          // the network's input size
constexpr int INC_FEAT = 2048;
constexpr float INC_BN_EPS = 0.001f;

struct IncConvDesc { std::string name; int cin, cout, kh, kw, stride, ph, pw; int64_t woff; };   // woff: float offset of conv.weight; then bn.weight, bn.bias, bn.running_mean, bn.running_var (cout each)
enum { INC_OP_CONV = 0, INC_OP_MAXPOOL_S2, INC_OP_AVGPOOL_S1, INC_OP_MAXPOOL_S1 };
// one step of the forward program: buffers are indices into gi_inception::buf; ld / coff in channels
struct IncStep { int kind, conv, src, dst, H, W, Ho, Wo, C, ldin, coffin, ldout, coffout; };
constexpr int INC_NBUF = 4;          // block input / output ping-pong (0, 1) and two branch temporaries (2, 3)

template <typename T>
struct IncConvP {
  const T* x; const T* w; const float* bias; T* out;
  int M, N, K, H, W, Ho, Wo, cin, ldin, coffin, ldout, coffout, kh, kw, stride, ph, pw;
};

template <typename T>
__device__ __forceinline__ void inc_zero8(T (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
}
template <typename T>
__device__ __forceinline__ void inc_ld8(const T* __restrict__ p, T (&v)[8]) {   // 16-byte aligned
  if constexpr (sizeof(T) == 2) {
    const h8_t h = __builtin_bit_cast(h8_t, *(const u4_t*)p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = h[j];
  } else {
    const f4_t a = *(const f4_t*)p, b = *(const f4_t*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
}
template <typename T>
__device__ __forceinline__ void inc_st8(T* p, const T (&v)[8]) {   // 16-byte aligned
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

constexpr int INC_BM = 64, INC_BN = 64, INC_BK = 32;

// out[pixel m][coffout + n] = relu(bias[n] + sum_k A[m][k] W[n][k]), A gathered from the NHWC input (cin % 8 == 0: a chunk of 8 k
// never straddles a tap). Thread t stages A chunk (row t % 64, k chunk t / 64) and B chunk (column t % 64, k chunk t / 64) per K step.
template <typename T, bool PW>
__global__ void __launch_bounds__(256) inc_gemm_kernel(IncConvP<T> p) {
  constexpr bool F16 = std::is_same<T, half_t>::value;
  constexpr int LDK = F16 ? 40 : 36;   // LDS row stride (elements): 16-byte aligned rows
  constexpr int WM = INC_BM / 2, WN = INC_BN / 2;
  __shared__ __attribute__((aligned(16))) T sA[INC_BM * LDK];
  __shared__ __attribute__((aligned(16))) T sB[INC_BN * LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * INC_BM, n0 = blockIdx.y * INC_BN;
  const int nkt = (p.K + INC_BK - 1) / INC_BK;

  // this thread's A row and B column
  const int srow = tid & 63, kc = tid >> 6;
  const int m = m0 + srow, ncol = n0 + srow;
  const bool mok = m < p.M, nok = ncol < p.N;
  const T* xrow = p.x;      // PW: the pixel's channels; else: the image's origin
  int iy0 = 0, ix0 = 0;
  if (mok) {
    if constexpr (PW) xrow = p.x + (int64_t)m * p.ldin + p.coffin;
    else {
      const int ox = m % p.Wo, t = m / p.Wo, oy = t % p.Ho, img = t / p.Ho;
      iy0 = oy * p.stride - p.ph;
      ix0 = ox * p.stride - p.pw;
      xrow = p.x + (int64_t)img * p.H * p.W * p.ldin + p.coffin;
    }
  }
  const T* wrow = p.w + (int64_t)(nok ? ncol : 0) * p.K;
  // tap walk of this thread's k chunk: k = (ky * kw + kx) * cin + ci
  int ci = kc * 8, ky = 0, kx = 0;
  auto norm = [&]() {
    while (ci >= p.cin) { ci -= p.cin; if (++kx == p.kw) { kx = 0; ++ky; } }
  };
  if constexpr (!PW) norm();

  T ra[8], rb[8];
  auto gload = [&](int kt) {
    const int k0 = kt * INC_BK + kc * 8;
    if (mok && k0 < p.K) {
      if constexpr (PW) inc_ld8(xrow + k0, ra);
      else {
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) inc_ld8(xrow + ((int64_t)iy * p.W + ix) * p.ldin + ci, ra);
        else inc_zero8(ra);
      }
    } else inc_zero8(ra);
    if (nok && k0 < p.K) inc_ld8(wrow + k0, rb);
    else inc_zero8(rb);
    if constexpr (!PW) { ci += INC_BK; norm(); }
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

  gload(0);
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    inc_st8(&sA[srow * LDK + kc * 8], ra);
    inc_st8(&sB[srow * LDK + kc * 8], rb);
    __syncthreads();
    if (kt + 1 < nkt) gload(kt + 1);   // next step's loads in flight during the MFMAs
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
      for (int kk = 0; kk < INC_BK / 2; ++kk) {
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

  // epilogue: every lane holds groups of 4 consecutive rows (pixels) of one column (channel)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < (F16 ? 1 : 4); ++g) {
        int row, col;
        if constexpr (F16) { row = wm * WM + mt * 16 + (lane >> 4) * 4; col = wn * WN + nt * 16 + (lane & 15); }
        else { row = wm * WM + mt * 32 + 8 * g + 4 * (lane >> 5); col = wn * WN + nt * 32 + (lane & 31); }
        const int mm = m0 + row, nn = n0 + col;
        if (mm >= p.M || nn >= p.N) continue;
        const float b = p.bias[nn];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (mm + r >= p.M) break;
          const float v = acc[mt][nt][4 * g + r] + b;
          p.out[(int64_t)(mm + r) * p.ldout + p.coffout + nn] = (T)(v > 0.f ? v : 0.f);
        }
      }
}

// (n, c, H, W) fp32 in [0, 1], c = 1 or 3 -> (n, 299, 299, 8) T: bilinear (align_corners = False) of every channel, 2 v - 1,
// channels 3 .. 7 zero. Source index arithmetic in fp32 as torch's upsample_bilinear2d does it.
template <typename T>
__global__ void __launch_bounds__(256) inc_input_kernel(const float* __restrict__ x, int n, int c, int H, int W, T* __restrict__ out) {
  const int64_t total = (int64_t)n * INC_HW * INC_HW;
  const float sy = (float)H / (float)INC_HW, sx = (float)W / (float)INC_HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % INC_HW);
    const int64_t t = i / INC_HW;
    const int oy = (int)(t % INC_HW);
    const int64_t img = t / INC_HW;
    float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    T v[8];
    inc_zero8(v);
    float last = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (ch < c) {
        const float* s = x + (img * c + ch) * (int64_t)H * W;
        const float r = hy * (hx * s[(int64_t)y0 * W + x0] + lx * s[(int64_t)y0 * W + x1]) +
                        ly * (hx * s[(int64_t)y1 * W + x0] + lx * s[(int64_t)y1 * W + x1]);
        last = 2.f * r - 1.f;
      }
      v[ch] = (T)last;
    }
    inc_st8(out + i * 8, v);
  }
}

// 3x3 / stride 2 / no padding max pool, NHWC, 8 channels per thread; reads channels [0, C) of rows of ldin, writes at coffout of ldout
template <typename T>
__global__ void __launch_bounds__(256) inc_maxpool3s2_kernel(const T* __restrict__ in, T* __restrict__ out, int n, int H, int W, int Ho, int Wo,
                                                             int C, int ldin, int ldout, int coffout) {
  const int cg = C / 8;
  const int64_t total = (int64_t)n * Ho * Wo * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % cg);
    const int64_t pix = i / cg;
    const int ox = (int)(pix % Wo);
    const int64_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const int64_t img = t / Ho;
    T best[8], v[8];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        inc_ld8(in + ((img * H + 2 * oy + dy) * W + 2 * ox + dx) * ldin + g * 8, v);   // 2 oy + 2 <= H - 1 by the size formula
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = (dy == 0 && dx == 0) ? v[j] : (v[j] > best[j] ? v[j] : best[j]);
      }
    inc_st8(out + pix * ldout + coffout + g * 8, best);
  }
}

// 3x3 / stride 1 / padding 1 pool of a dense NHWC map: MAXP ? max : average over the taps INSIDE the map (count_include_pad = False)
template <typename T, bool MAXP>
__global__ void __launch_bounds__(256) inc_pool3s1_kernel(const T* __restrict__ in, T* __restrict__ out, int n, int H, int W, int C) {
  const int cg = C / 8;
  const int64_t total = (int64_t)n * H * W * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % cg);
    const int64_t pix = i / cg;
    const int x = (int)(pix % W);
    const int64_t t = pix / W;
    const int y = (int)(t % H);
    const int64_t img = t / H;
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = MAXP ? -3.0e38f : 0.f;
    int cnt = 0;
    T v[8];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        inc_ld8(in + ((img * H + yy) * W + xx) * C + g * 8, v);
        ++cnt;
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = MAXP ? fmaxf(a[j], (float)v[j]) : a[j] + (float)v[j];
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)(MAXP ? a[j] : a[j] / (float)cnt);
    inc_st8(out + pix * C + g * 8, v);
  }
}

// global average over the HW pixels of a dense NHWC map -> (n, C) fp32, pixels added in order
template <typename T>
__global__ void __launch_bounds__(256) inc_gap_kernel(const T* __restrict__ in, float* __restrict__ out, int n, int HW, int C) {
  const int64_t total = (int64_t)n * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ch = (int)(i % C);
    const int64_t img = i / C;
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += (float)in[(img * HW + q) * C + ch];
    out[i] = s / (float)HW;
  }
}

// debug read-back: channels [coff, coff + C) of the ld-wide NHWC rows of n HW-pixel maps -> (n, C, HW) fp32 (every T is exact in fp32)
template <typename T>
__global__ void __launch_bounds__(256) inc_export_kernel(const T* __restrict__ in, float* __restrict__ out, int n, int HW, int C, int ld, int coff) {
  const int64_t total = (int64_t)n * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % HW);
    const int64_t t = i / HW;
    const int ch = (int)(t % C);
    const int64_t img = t / C;
    out[i] = (float)in[(img * HW + q) * ld + coff + ch];
  }
}

// BasicConv2d = conv (no bias) + BatchNorm(eps 0.001, running statistics) + ReLU, folded in fp32:
// wp[o][tap][ci] = w[o][ci][tap] * g[o] / sqrt(var[o] + eps) (ci >= cin: 0), bias[o] = beta[o] - mean[o] * g[o] / sqrt(var[o] + eps)
template <typename T>
__global__ void __launch_bounds__(256) inc_fold_pack_kernel(const float* __restrict__ w, const float* __restrict__ bn, T* __restrict__ wp,
                                                            float* __restrict__ bias, int cout, int cin, int cinp, int taps) {
  const int64_t total = (int64_t)cout * taps * cinp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cinp);
    const int t = (int)((i / cinp) % taps);
    const int o = (int)(i / ((int64_t)cinp * taps));
    const float s = bn[o] / sqrtf(bn[3 * cout + o] + INC_BN_EPS);
    wp[i] = c < cin ? (T)(w[((int64_t)o * cin + c) * taps + t] * s) : (T)0.f;
    if (c == 0 && t == 0) bias[o] = bn[cout + o] - bn[2 * cout + o] * s;
  }
}

// ---- streaming fp64 statistics: acc = [count, sum[d], xtx[d][d]] --------------------------------------------------------
__global__ void __launch_bounds__(256) fid_sum_kernel(double* __restrict__ acc, const float* __restrict__ f, int n, int d) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  double s = acc[1 + j];
  for (int r = 0; r < n; ++r) s += (double)f[(int64_t)r * d + j];
  acc[1 + j] = s;
  if (j == 0) acc[0] += (double)n;
}
// thread (j, i-group): xtx[i][j] for 4 consecutive i
__global__ void __launch_bounds__(256) fid_xtx_kernel(double* __restrict__ acc, const float* __restrict__ f, int n, int d) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i0 = blockIdx.y * 4;
  if (j >= d) return;
  double* a = acc + 1 + d;
  double s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = i0 + q < d ? a[(int64_t)(i0 + q) * d + j] : 0.0;
  for (int r = 0; r < n; ++r) {
    const float* row = f + (int64_t)r * d;
    const double xj = (double)row[j];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = fma(i0 + q < d ? (double)row[i0 + q] : 0.0, xj, s[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) if (i0 + q < d) a[(int64_t)(i0 + q) * d + j] = s[q];
}
// mu = sum / n, sigma = (xtx - sum sum^T / n) / (n - 1)   (np.cov(rowvar=False))
__global__ void __launch_bounds__(256) fid_finish_kernel(const double* __restrict__ acc, double* __restrict__ mu, double* __restrict__ sigma, int d) {
  const double n = acc[0];
  const double* sum = acc + 1;
  const double* a = acc + 1 + d;
  const int64_t total = (int64_t)d * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / d), c = (int)(i % d);
    sigma[i] = (a[i] - sum[r] * sum[c] / n) / (n - 1.0);
    if (r == 0) mu[c] = sum[c] / n;
  }
}

int inc_grid(int64_t work) {
  int64_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

}  // namespace

struct gi_inception {
  gi_ctx* ctx;
  int dtype, max_batch;
  std::vector<IncConvDesc> convs;
  std::vector<IncStep> steps;
  int64_t param_floats;
  int64_t buf_elems[INC_NBUF];     // per image
  int final_buf;
  const float* params;
  char* ws;
  int64_t ws_bytes;
  void* in8;                       // (n, 299, 299, 8)
  void* buf[INC_NBUF];
  std::vector<void*> wpk;
  std::vector<float*> bias;
  bool bound, synced;
  int dbg_steps, dbg_n;            // the last call was debug_forward_steps(dbg_steps) on dbg_n images (-1: it was not): what debug_read may read
};

namespace {

// ---- the program ---------------------------------------------------------------------------------------------------------------
struct IncBuilder {
  gi_inception* v;
  int64_t off = 0;
  int H[INC_NBUF] = {0, 0, 0, 0}, W[INC_NBUF] = {0, 0, 0, 0};
  void need(int b, int h, int w, int ld) {
    const int64_t e = (int64_t)h * w * ld;
    if (e > v->buf_elems[b]) v->buf_elems[b] = e;
  }
  // src < 0: the 8-channel resized input
  void conv(const std::string& name, int src, int hin, int win, int cin, int ldin, int dst, int cout, int ldout, int coffout, int kh, int kw,
            int stride = 1, int ph = 0, int pw = 0) {
    IncConvDesc d{name, cin, cout, kh, kw, stride, ph, pw, off};
    off += (int64_t)cout * cin * kh * kw + 4 * (int64_t)cout;
    const int ho = (hin + 2 * ph - kh) / stride + 1, wo = (win + 2 * pw - kw) / stride + 1;
    IncStep s{INC_OP_CONV, (int)v->convs.size(), src, dst, hin, win, ho, wo, cout, ldin, 0, ldout, coffout};
    v->convs.push_back(d);
    v->steps.push_back(s);
    need(dst, ho, wo, ldout);
    H[dst] = ho; W[dst] = wo;
  }
  void pool(int kind, int src, int C, int ldin, int dst, int ldout, int coffout) {
    const int hin = H[src], win = W[src];
    const int ho = kind == INC_OP_MAXPOOL_S2 ? (hin - 3) / 2 + 1 : hin, wo = kind == INC_OP_MAXPOOL_S2 ? (win - 3) / 2 + 1 : win;
    v->steps.push_back(IncStep{kind, -1, src, dst, hin, win, ho, wo, C, ldin, 0, ldout, coffout});
    need(dst, ho, wo, ldout);
    H[dst] = ho; W[dst] = wo;
  }
  // blocks read buffer x (C channels, dense) and write buffer y = x ^ 1; temporaries 2 and 3
  void blockA(const std::string& n, int x, int C, int pf) {
    const int y = x ^ 1, h = H[x], w = W[x], ld = 224 + pf;
    conv(n + ".branch1x1", x, h, w, C, C, y, 64, ld, 0, 1, 1);
    conv(n + ".branch5x5_1", x, h, w, C, C, 2, 48, 48, 0, 1, 1);
    conv(n + ".branch5x5_2", 2, h, w, 48, 48, y, 64, ld, 64, 5, 5, 1, 2, 2);
    conv(n + ".branch3x3dbl_1", x, h, w, C, C, 2, 64, 64, 0, 1, 1);
    conv(n + ".branch3x3dbl_2", 2, h, w, 64, 64, 3, 96, 96, 0, 3, 3, 1, 1, 1);
    conv(n + ".branch3x3dbl_3", 3, h, w, 96, 96, y, 96, ld, 128, 3, 3, 1, 1, 1);
    pool(INC_OP_AVGPOOL_S1, x, C, C, 2, C, 0);
    conv(n + ".branch_pool", 2, h, w, C, C, y, pf, ld, 224, 1, 1);
  }
  void blockB(const std::string& n, int x, int C) {
    const int y = x ^ 1, h = H[x], w = W[x], ld = 384 + 96 + C;
    conv(n + ".branch3x3", x, h, w, C, C, y, 384, ld, 0, 3, 3, 2);
    conv(n + ".branch3x3dbl_1", x, h, w, C, C, 2, 64, 64, 0, 1, 1);
    conv(n + ".branch3x3dbl_2", 2, h, w, 64, 64, 3, 96, 96, 0, 3, 3, 1, 1, 1);
    conv(n + ".branch3x3dbl_3", 3, h, w, 96, 96, y, 96, ld, 384, 3, 3, 2);
    pool(INC_OP_MAXPOOL_S2, x, C, C, y, ld, 480);
  }
  void blockC(const std::string& n, int x, int C, int c7) {
    const int y = x ^ 1, h = H[x], w = W[x], ld = 768;
    conv(n + ".branch1x1", x, h, w, C, C, y, 192, ld, 0, 1, 1);
    conv(n + ".branch7x7_1", x, h, w, C, C, 2, c7, c7, 0, 1, 1);
    conv(n + ".branch7x7_2", 2, h, w, c7, c7, 3, c7, c7, 0, 1, 7, 1, 0, 3);
    conv(n + ".branch7x7_3", 3, h, w, c7, c7, y, 192, ld, 192, 7, 1, 1, 3, 0);
    conv(n + ".branch7x7dbl_1", x, h, w, C, C, 2, c7, c7, 0, 1, 1);
    conv(n + ".branch7x7dbl_2", 2, h, w, c7, c7, 3, c7, c7, 0, 7, 1, 1, 3, 0);
    conv(n + ".branch7x7dbl_3", 3, h, w, c7, c7, 2, c7, c7, 0, 1, 7, 1, 0, 3);
    conv(n + ".branch7x7dbl_4", 2, h, w, c7, c7, 3, c7, c7, 0, 7, 1, 1, 3, 0);
    conv(n + ".branch7x7dbl_5", 3, h, w, c7, c7, y, 192, ld, 384, 1, 7, 1, 0, 3);
    pool(INC_OP_AVGPOOL_S1, x, C, C, 2, C, 0);
    conv(n + ".branch_pool", 2, h, w, C, C, y, 192, ld, 576, 1, 1);
  }
  void blockD(const std::string& n, int x, int C) {
    const int y = x ^ 1, h = H[x], w = W[x], ld = 320 + 192 + C;
    conv(n + ".branch3x3_1", x, h, w, C, C, 2, 192, 192, 0, 1, 1);
    conv(n + ".branch3x3_2", 2, h, w, 192, 192, y, 320, ld, 0, 3, 3, 2);
    conv(n + ".branch7x7x3_1", x, h, w, C, C, 2, 192, 192, 0, 1, 1);
    conv(n + ".branch7x7x3_2", 2, h, w, 192, 192, 3, 192, 192, 0, 1, 7, 1, 0, 3);
    conv(n + ".branch7x7x3_3", 3, h, w, 192, 192, 2, 192, 192, 0, 7, 1, 1, 3, 0);
    conv(n + ".branch7x7x3_4", 2, h, w, 192, 192, y, 192, ld, 320, 3, 3, 2);
    pool(INC_OP_MAXPOOL_S2, x, C, C, y, ld, 512);
  }
  void blockE(const std::string& n, int x, int C, bool maxpool) {
    const int y = x ^ 1, h = H[x], w = W[x], ld = 2048;
    conv(n + ".branch1x1", x, h, w, C, C, y, 320, ld, 0, 1, 1);
    conv(n + ".branch3x3_1", x, h, w, C, C, 2, 384, 384, 0, 1, 1);
    conv(n + ".branch3x3_2a", 2, h, w, 384, 384, y, 384, ld, 320, 1, 3, 1, 0, 1);
    conv(n + ".branch3x3_2b", 2, h, w, 384, 384, y, 384, ld, 704, 3, 1, 1, 1, 0);
    conv(n + ".branch3x3dbl_1", x, h, w, C, C, 2, 448, 448, 0, 1, 1);
    conv(n + ".branch3x3dbl_2", 2, h, w, 448, 448, 3, 384, 384, 0, 3, 3, 1, 1, 1);
    conv(n + ".branch3x3dbl_3a", 3, h, w, 384, 384, y, 384, ld, 1088, 1, 3, 1, 0, 1);
    conv(n + ".branch3x3dbl_3b", 3, h, w, 384, 384, y, 384, ld, 1472, 3, 1, 1, 1, 0);
    pool(maxpool ? INC_OP_MAXPOOL_S1 : INC_OP_AVGPOOL_S1, x, C, C, 2, C, 0);
    conv(n + ".branch_pool", 2, h, w, C, C, y, 192, ld, 1856, 1, 1);
  }
  void build() {
    conv("Conv2d_1a_3x3", -1, INC_HW, INC_HW, 3, 8, 0, 32, 32, 0, 3, 3, 2);           // 149
    conv("Conv2d_2a_3x3", 0, H[0], W[0], 32, 32, 1, 32, 32, 0, 3, 3);                 // 147
    conv("Conv2d_2b_3x3", 1, H[1], W[1], 32, 32, 0, 64, 64, 0, 3, 3, 1, 1, 1);
    pool(INC_OP_MAXPOOL_S2, 0, 64, 64, 1, 64, 0);                                     // 73
    conv("Conv2d_3b_1x1", 1, H[1], W[1], 64, 64, 0, 80, 80, 0, 1, 1);
    conv("Conv2d_4a_3x3", 0, H[0], W[0], 80, 80, 1, 192, 192, 0, 3, 3);               // 71
    pool(INC_OP_MAXPOOL_S2, 1, 192, 192, 0, 192, 0);                                  // 35
    blockA("Mixed_5b", 0, 192, 32);
    blockA("Mixed_5c", 1, 256, 64);
    blockA("Mixed_5d", 0, 288, 64);
    blockB("Mixed_6a", 1, 288);                                                       // 17
    blockC("Mixed_6b", 0, 768, 128);
    blockC("Mixed_6c", 1, 768, 160);
    blockC("Mixed_6d", 0, 768, 160);
    blockC("Mixed_6e", 1, 768, 192);
    blockD("Mixed_7a", 0, 768);                                                       // 8
    blockE("Mixed_7b", 1, 1280, false);
    blockE("Mixed_7c", 0, 2048, true);
    v->final_buf = 1;
    v->param_floats = off;
  }
};

int64_t inc_ws_layout(gi_inception* v, char* base) {
  int64_t off = 0;
  const int64_t es = (int64_t)gi_dtype_size(v->dtype);
  auto take = [&](int64_t bytes) { char* p = base ? base + off : nullptr; off += gi_align_up(bytes, 256); return p; };
  v->in8 = take((int64_t)v->max_batch * INC_HW * INC_HW * 8 * es);
  for (int b = 0; b < INC_NBUF; ++b) v->buf[b] = take((int64_t)v->max_batch * v->buf_elems[b] * es);
  v->wpk.resize(v->convs.size());
  v->bias.resize(v->convs.size());
  for (size_t i = 0; i < v->convs.size(); ++i) {
    const IncConvDesc& c = v->convs[i];
    const int cinp = (c.cin + 7) / 8 * 8;
    v->wpk[i] = take((int64_t)c.cout * c.kh * c.kw * cinp * es);
    v->bias[i] = (float*)take((int64_t)c.cout * 4);
  }
  return off;
}

template <typename T>
int inc_conv_launch(gi_inception* v, const IncStep& s, int n) {
  const IncConvDesc& c = v->convs[s.conv];
  const int cinp = (c.cin + 7) / 8 * 8;
  IncConvP<T> p;
  p.x = (const T*)(s.src < 0 ? v->in8 : v->buf[s.src]);
  p.w = (const T*)v->wpk[s.conv];
  p.bias = v->bias[s.conv];
  p.out = (T*)v->buf[s.dst];
  const int64_t M = (int64_t)n * s.Ho * s.Wo;
  GI_REQUIRE(M < (1ll << 31) && M * s.ldout < (1ll << 40), "inception: %s: %lld output pixels", c.name.c_str(), (long long)M);
  p.M = (int)M; p.N = c.cout; p.K = c.kh * c.kw * cinp;
  p.H = s.H; p.W = s.W; p.Ho = s.Ho; p.Wo = s.Wo;
  p.cin = cinp; p.ldin = s.ldin; p.coffin = s.coffin; p.ldout = s.ldout; p.coffout = s.coffout;
  p.kh = c.kh; p.kw = c.kw; p.stride = c.stride; p.ph = c.ph; p.pw = c.pw;
  const dim3 grid((p.M + INC_BM - 1) / INC_BM, (p.N + INC_BN - 1) / INC_BN);
  const bool pw = c.kh == 1 && c.kw == 1 && c.stride == 1;
  constexpr bool F16 = std::is_same<T, half_t>::value;
  if (pw) {
    hipLaunchKernelGGL((inc_gemm_kernel<T, true>), grid, dim3(256), 0, v->ctx->stream, p);
    gi_note_kernel(F16 ? "inc_gemm_kernel<f16,pointwise>" : "inc_gemm_kernel<f32,pointwise>");
  } else {
    hipLaunchKernelGGL((inc_gemm_kernel<T, false>), grid, dim3(256), 0, v->ctx->stream, p);
    gi_note_kernel(F16 ? "inc_gemm_kernel<f16,taps>" : "inc_gemm_kernel<f32,taps>");
  }
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// runs the program; nconvs >= 0: stops after that many convolutions, nsteps >= 0: after that many steps (either writes no features)
template <typename T>
int inc_run(gi_inception* v, const float* x, int n, int c, int H, int W, float* out, int nconvs, int nsteps = -1) {
  hipStream_t st = v->ctx->stream;
  hipLaunchKernelGGL((inc_input_kernel<T>), dim3(inc_grid((int64_t)n * INC_HW * INC_HW)), dim3(256), 0, st, x, n, c, H, W, (T*)v->in8);
  GI_LAUNCH_CHECK();
  int done = 0, ran = 0;
  for (const IncStep& s : v->steps) {
    if (nconvs >= 0 && done >= nconvs) return GI_OK;
    if (nsteps >= 0 && ran++ >= nsteps) return GI_OK;
    if (s.kind == INC_OP_CONV) {
      GI_TRY(inc_conv_launch<T>(v, s, n));
      ++done;
      continue;
    }
    const T* in = (const T*)v->buf[s.src];
    T* o = (T*)v->buf[s.dst];
    const int grid = inc_grid((int64_t)n * s.Ho * s.Wo * (s.C / 8));
    if (s.kind == INC_OP_MAXPOOL_S2)
      hipLaunchKernelGGL((inc_maxpool3s2_kernel<T>), dim3(grid), dim3(256), 0, st, in, o, n, s.H, s.W, s.Ho, s.Wo, s.C, s.ldin, s.ldout, s.coffout);
    else if (s.kind == INC_OP_AVGPOOL_S1)
      hipLaunchKernelGGL((inc_pool3s1_kernel<T, false>), dim3(grid), dim3(256), 0, st, in, o, n, s.H, s.W, s.C);
    else
      hipLaunchKernelGGL((inc_pool3s1_kernel<T, true>), dim3(grid), dim3(256), 0, st, in, o, n, s.H, s.W, s.C);
    GI_LAUNCH_CHECK();
  }
  if (nconvs >= 0 || nsteps >= 0) return GI_OK;
  const IncStep& last = v->steps.back();
  hipLaunchKernelGGL((inc_gap_kernel<T>), dim3(inc_grid((int64_t)n * INC_FEAT)), dim3(256), 0, st, (const T*)v->buf[v->final_buf], out, n,
                     last.Ho * last.Wo, INC_FEAT);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// channels of a step's input view: a convolution's cin (step 0: the 8 channels of the padded resized input), a pool's C
int inc_step_cin(const gi_inception* v, const IncStep& s) { return s.kind != INC_OP_CONV ? s.C : s.src < 0 ? 8 : v->convs[s.conv].cin; }

int inc_check_call(const gi_inception* v, const float* x, int n, int c, int H, int W, const char* who) {
  GI_REQUIRE(v && v->ctx, "%s: the handle was created without a context (inventory only)", who);
  GI_REQUIRE(v->bound && v->synced, "%s: bind + sync_weights first", who);
  GI_REQUIRE(x && n > 0 && n <= v->max_batch && (c == 1 || c == 3) && H > 0 && W > 0 && (int64_t)n * c * H * W < (1ll << 31),
             "%s: n=%d (max %d) c=%d (1 or 3) H=%d W=%d", who, n, v->max_batch, c, H, W);
  return GI_OK;
}

}  // namespace

extern "C" {

int gi_inception_create(gi_ctx* ctx, int dtype, int max_batch, gi_inception** out) {
  GI_REQUIRE(out, "inception_create: null argument");
  GI_REQUIRE((dtype == GI_F16 || dtype == GI_F32) && max_batch > 0 && max_batch <= 1024, "inception_create: dtype=%d max_batch=%d (1..1024)", dtype,
             max_batch);
  gi_inception* v = new (std::nothrow) gi_inception();
  GI_REQUIRE(v, "inception_create: out of host memory");
  v->ctx = ctx; v->dtype = dtype; v->max_batch = max_batch;
  for (int b = 0; b < INC_NBUF; ++b) v->buf_elems[b] = 0;
  IncBuilder bld;
  bld.v = v;
  bld.build();
  v->params = nullptr; v->ws = nullptr; v->bound = false; v->synced = false;
  v->dbg_steps = -1; v->dbg_n = 0;
  v->ws_bytes = inc_ws_layout(v, nullptr);
  *out = v;
  return GI_OK;
}
void gi_inception_destroy(gi_inception* v) { delete v; }
int64_t gi_inception_param_floats(const gi_inception* v) { return v ? v->param_floats : -1; }
int64_t gi_inception_workspace_bytes(const gi_inception* v) { return v ? v->ws_bytes : -1; }
int gi_inception_num_tensors(const gi_inception* v) { return v ? 5 * (int)v->convs.size() : -1; }

int gi_inception_tensor_desc(const gi_inception* v, int index, char* name, int name_cap, int* shape4, int64_t* offset) {
  GI_REQUIRE(v && index >= 0 && index < 5 * (int)v->convs.size() && name && shape4 && offset, "inception_tensor_desc: bad argument");
  static const char* kSuffix[5] = {"conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"};
  const IncConvDesc& c = v->convs[index / 5];
  const int k = index % 5;
  snprintf(name, name_cap, "%s.%s", c.name.c_str(), kSuffix[k]);
  const int64_t wn = (int64_t)c.cout * c.cin * c.kh * c.kw;
  if (k == 0) { shape4[0] = c.cout; shape4[1] = c.cin; shape4[2] = c.kh; shape4[3] = c.kw; *offset = c.woff; }
  else { shape4[0] = c.cout; shape4[1] = shape4[2] = shape4[3] = 0; *offset = c.woff + wn + (int64_t)(k - 1) * c.cout; }
  return GI_OK;
}

int gi_inception_bind(gi_inception* v, const float* params, void* ws, int64_t ws_bytes) {
  GI_REQUIRE(v && v->ctx, "inception_bind: the handle was created without a context (inventory only)");
  GI_REQUIRE(params && ws, "inception_bind: null argument");
  GI_REQUIRE(ws_bytes >= v->ws_bytes && ((uintptr_t)ws & 255) == 0, "inception_bind: workspace %lld bytes (need %lld, 256-byte aligned)",
             (long long)ws_bytes, (long long)v->ws_bytes);
  v->params = params; v->ws = (char*)ws;
  inc_ws_layout(v, v->ws);
  v->bound = true; v->synced = false;
  v->dbg_steps = -1;
  return GI_OK;
}

int gi_inception_sync_weights(gi_inception* v) {
  GI_REQUIRE(v && v->ctx && v->bound, "inception_sync_weights: not bound");
  hipStream_t st = v->ctx->stream;
  v->dbg_steps = -1;
  for (size_t i = 0; i < v->convs.size(); ++i) {
    const IncConvDesc& c = v->convs[i];
    const int taps = c.kh * c.kw, cinp = (c.cin + 7) / 8 * 8;
    const float* w = v->params + c.woff;
    const float* bn = w + (int64_t)c.cout * c.cin * taps;
    const int grid = inc_grid((int64_t)c.cout * taps * cinp);
    if (v->dtype == GI_F16)
      hipLaunchKernelGGL((inc_fold_pack_kernel<half_t>), dim3(grid), dim3(256), 0, st, w, bn, (half_t*)v->wpk[i], v->bias[i], c.cout, c.cin, cinp, taps);
    else
      hipLaunchKernelGGL((inc_fold_pack_kernel<float>), dim3(grid), dim3(256), 0, st, w, bn, (float*)v->wpk[i], v->bias[i], c.cout, c.cin, cinp, taps);
    GI_LAUNCH_CHECK();
  }
  v->synced = true;
  return GI_OK;
}

int gi_inception_features(gi_inception* v, const float* x, int n, int c, int H, int W, float* out) {
  GI_TRY(inc_check_call(v, x, n, c, H, W, "inception_features"));
  GI_REQUIRE(out, "inception_features: null output");
  v->dbg_steps = -1;
  return v->dtype == GI_F16 ? inc_run<half_t>(v, x, n, c, H, W, out, -1) : inc_run<float>(v, x, n, c, H, W, out, -1);
}

int gi_inception_debug_forward_convs(gi_inception* v, const float* x, int n, int c, int H, int W, int nconvs) {
  GI_TRY(inc_check_call(v, x, n, c, H, W, "inception_debug_forward_convs"));
  GI_REQUIRE(nconvs >= 0 && nconvs <= (int)v->convs.size(), "inception_debug_forward_convs: nconvs=%d (0..%d)", nconvs, (int)v->convs.size());
  v->dbg_steps = -1;
  return v->dtype == GI_F16 ? inc_run<half_t>(v, x, n, c, H, W, nullptr, nconvs) : inc_run<float>(v, x, n, c, H, W, nullptr, nconvs);
}

int gi_inception_num_steps(const gi_inception* v) { return v ? (int)v->steps.size() : -1; }

int gi_inception_step_desc(const gi_inception* v, int step, int* kind, int* conv, int* in_chw, int* out_chw, int* route4) {
  GI_REQUIRE(v && step >= 0 && step < (int)v->steps.size() && kind && conv && in_chw && out_chw && route4, "inception_step_desc: bad argument");
  const IncStep& s = v->steps[step];
  *kind = s.kind; *conv = s.conv;
  in_chw[0] = inc_step_cin(v, s); in_chw[1] = s.H; in_chw[2] = s.W;
  out_chw[0] = s.C; out_chw[1] = s.Ho; out_chw[2] = s.Wo;
  route4[0] = s.src; route4[1] = s.dst; route4[2] = s.ldout; route4[3] = s.coffout;
  return GI_OK;
}

int gi_inception_debug_forward_steps(gi_inception* v, const float* x, int n, int c, int H, int W, int nsteps) {
  GI_TRY(inc_check_call(v, x, n, c, H, W, "inception_debug_forward_steps"));
  GI_REQUIRE(nsteps >= 0 && nsteps <= (int)v->steps.size(), "inception_debug_forward_steps: nsteps=%d (0..%d)", nsteps, (int)v->steps.size());
  v->dbg_steps = -1;
  GI_TRY(v->dtype == GI_F16 ? inc_run<half_t>(v, x, n, c, H, W, nullptr, -1, nsteps) : inc_run<float>(v, x, n, c, H, W, nullptr, -1, nsteps));
  v->dbg_steps = nsteps; v->dbg_n = n;
  return GI_OK;
}

int gi_inception_debug_read(gi_inception* v, int step, int which, int n, float* out) {
  GI_REQUIRE(v && v->ctx, "inception_debug_read: the handle was created without a context (inventory only)");
  GI_REQUIRE(v->bound && v->synced && out, "inception_debug_read: bind + sync_weights first, non-null output");
  GI_REQUIRE(step >= 0 && step < (int)v->steps.size() && which >= 0 && which <= 2, "inception_debug_read: step=%d (0..%d) which=%d (0..2)", step,
             (int)v->steps.size() - 1, which);
  GI_REQUIRE(v->dbg_steps == step + 1 && v->dbg_n == n, "inception_debug_read: step %d of %d images is readable only directly after "
             "debug_forward_steps(nsteps=%d) on as many (last debug run: nsteps=%d, n=%d)", step, n, step + 1, v->dbg_steps, v->dbg_n);
  const IncStep& s = v->steps[step];
  const void* src = which == 0 ? (s.src < 0 ? v->in8 : v->buf[s.src]) : v->buf[s.dst];
  const int HW = which == 0 ? s.H * s.W : s.Ho * s.Wo;
  const int C = which == 0 ? inc_step_cin(v, s) : which == 1 ? s.C : s.ldout;
  const int ld = which == 0 ? s.ldin : s.ldout, coff = which == 0 ? s.coffin : which == 1 ? s.coffout : 0;
  const int grid = inc_grid((int64_t)n * C * HW);
  if (v->dtype == GI_F16)
    hipLaunchKernelGGL((inc_export_kernel<half_t>), dim3(grid), dim3(256), 0, v->ctx->stream, (const half_t*)src, out, n, HW, C, ld, coff);
  else
    hipLaunchKernelGGL((inc_export_kernel<float>), dim3(grid), dim3(256), 0, v->ctx->stream, (const float*)src, out, n, HW, C, ld, coff);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int64_t gi_fid_stats_acc_doubles(int d) { return d > 0 ? 1 + (int64_t)d + (int64_t)d * d : -1; }

int gi_fid_stats_update(gi_ctx* ctx, double* acc, const float* feats, int n, int d) {
  GI_REQUIRE(ctx && acc && feats && n > 0 && d > 0 && d <= 8192, "fid_stats_update: n=%d d=%d (1..8192)", n, d);
  hipLaunchKernelGGL(fid_sum_kernel, dim3((d + 255) / 256), dim3(256), 0, ctx->stream, acc, feats, n, d);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(fid_xtx_kernel, dim3((d + 255) / 256, (d + 3) / 4), dim3(256), 0, ctx->stream, acc, feats, n, d);
  GI_LAUNCH_CHECK();
  gi_note_kernel("fid_xtx_kernel");
  return GI_OK;
}

int gi_fid_stats_finish(gi_ctx* ctx, const double* acc, double* mu, double* sigma, int d) {
  GI_REQUIRE(ctx && acc && mu && sigma && d > 0 && d <= 8192, "fid_stats_finish: d=%d (1..8192)", d);
  hipLaunchKernelGGL(fid_finish_kernel, dim3(inc_grid((int64_t)d * d)), dim3(256), 0, ctx->stream, acc, mu, sigma, d);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // extern "C"
