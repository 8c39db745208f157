// Spectral normalisation of the PatchGAN critic's weights (torch.nn.utils.spectral_norm semantics), fp32 throughout:
//   power iteration   v = W^T u / max(|W^T u|, eps),  u = W v / max(|W v|, eps),  sigma = u . (W v)
//   effective copy    W_eff = W / sigma  (every other parameter copied)
//   projected add     dst += scale * (G - <G, W_eff>_F u v^T) / sigma
// The matrices are memory-bound matvecs between 1 x 1 and 512 x 4096. W^T u splits the ROWS of a matrix over workgroups (16-row
// chunks, one thread per column: coalesced) and adds the chunk partials in chunk order in a second launch; W v splits the COLUMNS
// of a row over waves (1024-column chunks: a 1 x 8192 tensor still runs on 8 waves) and adds those in chunk order. No float
// atomics, no arrival-order tickets: every sum has one order, fixed by the shapes alone, so parameter gradients stay
// bit-reproducible. Each launch serves all tensors through one job table (SnJobs), as op_pack_weights_batch does.
#include "common.h"

namespace {

constexpr int SN_ROWS = 16;      // rows per W^T u chunk
constexpr int SN_CTILE = 256;    // columns per W^T u workgroup
constexpr int SN_CCHUNK = 1024;  // columns per W v wave
constexpr int SN_DCHUNK = 4096;  // elements per <G, W_eff> workgroup
constexpr float SN_EPS = 1e-12f;

// memory column m of a [ky][kx][b] row -> column of v in torch's (b, ky, kx) order
__device__ __forceinline__ int sn_col(int m, int cb) { return cb > 0 ? (m % cb) * 16 + m / cb : m; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;   // lane 0 holds the total
}
// total of a 256-thread workgroup in every thread: wave trees, then the four wave totals in wave order
__device__ __forceinline__ float block_sum(float v, float* lds4) {
  v = wave_sum(v);
  __syncthreads();   // lds4 may still be read from a previous call
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// the tensor a workgroup of a by-tensor grid belongs to (which: index into SnJob::blk)
__device__ __forceinline__ int sn_job_of(const SnJobs& P, int which, int b) {
  int t = 0;
  for (int i = 1; i < P.n; ++i)
    if (b >= P.j[i].blk[which]) t = i;
  return t;
}

// A: part_t[chunk][m] = sum over the chunk's rows (ascending) of W[r][m] u[r]
__global__ void __launch_bounds__(256) sn_wtu_partial_kernel(SnJobs P) {
  const int t = sn_job_of(P, 0, blockIdx.x);
  const SnJob& J = P.j[t];
  const int local = blockIdx.x - J.blk[0];
  const int tile = local % J.ctiles, chunk = local / J.ctiles;
  const int m = tile * SN_CTILE + threadIdx.x;
  if (m >= J.K) return;
  const int r0 = chunk * SN_ROWS, r1 = min(J.ca, r0 + SN_ROWS);
  const float* w = J.w + (int64_t)r0 * J.K + m;
  float acc = 0.f;
  if (r1 - r0 == SN_ROWS) {   // all sixteen loads in flight, then the same additions in the same order
    float x[SN_ROWS];
#pragma unroll
    for (int i = 0; i < SN_ROWS; ++i) x[i] = w[(int64_t)i * J.K];
#pragma unroll
    for (int i = 0; i < SN_ROWS; ++i) acc = fmaf(x[i], J.u[r0 + i], acc);
  } else {
    for (int r = r0; r < r1; ++r, w += J.K) acc = fmaf(*w, J.u[r], acc);
  }
  J.part_t[(int64_t)chunk * J.K + m] = acc;
}

// B: t[m] = sum of the chunk partials in chunk order -> t_raw (torch's column order); the tile's sum of squares -> nrm_part
__global__ void __launch_bounds__(256) sn_wtu_finish_kernel(SnJobs P) {
  __shared__ float lds4[4];
  const int t = sn_job_of(P, 1, blockIdx.x);
  const SnJob& J = P.j[t];
  const int tile = blockIdx.x - J.blk[1];
  const int m = tile * SN_CTILE + threadIdx.x;
  float s = 0.f;
  if (m < J.K) {
    const float* part = J.part_t + m;
    int c = 0;
    for (; c + 8 <= J.rchunks; c += 8) {   // eight loads in flight, the additions in chunk order (as gi_ordered_sum_f4)
      float x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = part[(int64_t)(c + i) * J.K];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += x[i];
    }
    for (; c < J.rchunks; ++c) s += part[(int64_t)c * J.K];
    J.t_raw[sn_col(m, J.cb)] = s;
  }
  const float q = block_sum(s * s, lds4);
  if (threadIdx.x == 0) J.nrm_part[tile] = q;
}

// C: one wave per (row, 1024-column chunk): part_s[row][chunk] = sum of W[row][m] v[col(m)]. from_raw: v = t_raw / max(|t|, eps)
// with |t|^2 the tile sums in tile order, and the waves of row 0 store v
__global__ void __launch_bounds__(256) sn_wv_partial_kernel(SnJobs P, int from_raw) {
  const int t = sn_job_of(P, 2, blockIdx.x);
  const SnJob& J = P.j[t];
  const int64_t unit = (int64_t)(blockIdx.x - J.blk[2]) * 4 + (threadIdx.x >> 6);
  if (unit >= (int64_t)J.ca * J.cchunks) return;   // wave-uniform
  const int row = (int)(unit / J.cchunks), cc = (int)(unit % J.cchunks), lane = threadIdx.x & 63;
  float d = 1.f;
  if (from_raw) {
    float q = 0.f;
    for (int i = 0; i < J.ctiles; ++i) q += J.nrm_part[i];
    d = fmaxf(sqrtf(q), SN_EPS);
  }
  const float* __restrict__ w = J.w + (int64_t)row * J.K;
  const float* __restrict__ vsrc = from_raw ? J.t_raw : J.v;
  const int m1 = min(J.K, (cc + 1) * SN_CCHUNK);
  if (from_raw && row == 0)
    for (int m = cc * SN_CCHUNK + lane; m < m1; m += 64) {
      const int j = sn_col(m, J.cb);
      J.v[j] = J.t_raw[j] / d;
    }
  float acc = 0.f;
#pragma unroll 4
  for (int m = cc * SN_CCHUNK + lane; m < m1; m += 64) {
    const float x = vsrc[sn_col(m, J.cb)];
    acc = fmaf(w[m], from_raw ? x / d : x, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) J.part_s[(int64_t)row * J.cchunks + cc] = acc;
}

// D: one workgroup per tensor: s = W v from the chunk partials in chunk order; train: u = s / max(|s|, eps), stored; sigma = u . s
__global__ void __launch_bounds__(256) sn_u_sigma_kernel(SnJobs P, int train) {
  __shared__ float lds4[4];
  const SnJob& J = P.j[blockIdx.x];
  float q = 0.f;
  for (int r = threadIdx.x; r < J.ca; r += 256) {
    float s = 0.f;
    for (int c = 0; c < J.cchunks; ++c) s += J.part_s[(int64_t)r * J.cchunks + c];
    J.s_vec[r] = s;   // read back below by this same thread only
    q = fmaf(s, s, q);
  }
  float d = 1.f;
  if (train) d = fmaxf(sqrtf(block_sum(q, lds4)), SN_EPS);
  float dot = 0.f;
  for (int r = threadIdx.x; r < J.ca; r += 256) {
    const float s = J.s_vec[r];
    float ur;
    if (train) { ur = s / d; J.u[r] = ur; }
    else ur = J.u[r];
    dot = fmaf(ur, s, dot);
  }
  dot = block_sum(dot, lds4);
  if (threadIdx.x == 0) *J.sigma = dot;
}

__device__ __forceinline__ int sn_seg_of(const SnSegs& S, int64_t e) {
  for (int i = 0; i < S.n; ++i)
    if (e >= S.s[i].off && e < S.s[i].off + S.s[i].numel) return i;
  return -1;
}

// E: dst = src, the table's tensors divided by their sigma (a true division: a 1 x 1 tensor gives exactly +-1). VEC: 16 bytes
// per lane, the tensor looked up once per group of four - the host takes it when the pointers are 16-byte aligned and every
// tensor starts on a multiple of four (a group whose first element lies outside every tensor then holds none of any); the
// elements behind the last whole group go one per lane. Per element the same operations either way.
template <bool VEC>
__global__ void __launch_bounds__(256) sn_effective_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count, SnSegs S) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t groups = VEC ? count / 4 : 0;
  for (int64_t g = tid; g < groups; g += nth) {
    const int64_t e0 = g * 4;
    const int i = sn_seg_of(S, e0);
    f4_t x = ((const f4_t*)src)[g];
    if (i >= 0) {
      const float sigma = *S.s[i].sigma;
      const int64_t left = S.s[i].off + S.s[i].numel - e0;   // >= 1 elements of the group belong to the tensor
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < left) x[k] = x[k] / sigma;
    }
    ((f4_t*)dst)[g] = x;
  }
  for (int64_t e = groups * 4 + tid; e < count; e += nth) {
    const int i = sn_seg_of(S, e);
    const float x = src[e];
    dst[e] = i >= 0 ? x / *S.s[i].sigma : x;
  }
}

// P1: dot_part[chunk] = sum of G W_eff over 4096 elements (per thread 16 elements 256 apart, ascending; then the block tree)
__global__ void __launch_bounds__(256) sn_dot_partial_kernel(SnJobs P) {
  __shared__ float lds4[4];
  const int t = sn_job_of(P, 3, blockIdx.x);
  const SnJob& J = P.j[t];
  const int chunk = blockIdx.x - J.blk[3];
  const int64_t total = (int64_t)J.ca * J.K, e0 = (int64_t)chunk * SN_DCHUNK;
  const int64_t e1 = e0 + SN_DCHUNK < total ? e0 + SN_DCHUNK : total;
  float acc = 0.f;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) acc = fmaf(J.g[e], J.w[e], acc);
  acc = block_sum(acc, lds4);
  if (threadIdx.x == 0) J.dot_part[chunk] = acc;
}

// P2: c = the chunk sums (per thread every 256th, ascending; then the block tree); one workgroup per tensor
__global__ void __launch_bounds__(256) sn_dot_finish_kernel(SnJobs P) {
  __shared__ float lds4[4];
  const SnJob& J = P.j[blockIdx.x];
  float acc = 0.f;
  for (int i = threadIdx.x; i < J.dchunks; i += 256) acc += J.dot_part[i];
  acc = block_sum(acc, lds4);
  if (threadIdx.x == 0) *J.c = acc;
}

// P3: over [lo, hi) of the flat buffers. VEC as in sn_effective_kernel (lo a multiple of four as well): one tensor lookup and one
// row / column division per group of four, the column then counted up
template <bool VEC>
__global__ void __launch_bounds__(256) sn_project_add_kernel(const float* __restrict__ g, float* __restrict__ dst, int64_t lo, int64_t hi, SnSegs S,
                                                             const float* __restrict__ scale_dev) {
  const float scale = scale_dev ? *scale_dev : 1.f;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t groups = VEC ? (hi - lo) / 4 : 0;
  for (int64_t q = tid; q < groups; q += nth) {
    const int64_t e0 = lo + q * 4;
    const int i = sn_seg_of(S, e0);
    f4_t val = *(const f4_t*)(g + e0);
    if (i >= 0) {
      const SnSeg& s = S.s[i];
      const float c = *s.c, sigma = *s.sigma;
      const int64_t r0 = e0 - s.off, left = s.numel - r0;
      int a = (int)(r0 / s.K), m = (int)(r0 - (int64_t)a * s.K);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < left) val[k] = (val[k] - c * s.u[a] * s.v[sn_col(m, s.cb)]) / sigma;
        if (++m == s.K) { m = 0; ++a; }
      }
    }
    f4_t d = *(f4_t*)(dst + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] += scale * val[k];
    *(f4_t*)(dst + e0) = d;
  }
  for (int64_t e = lo + groups * 4 + tid; e < hi; e += nth) {
    const int i = sn_seg_of(S, e);
    float val = g[e];
    if (i >= 0) {
      const SnSeg& s = S.s[i];
      const int64_t r = e - s.off;
      const int a = (int)(r / s.K), m = (int)(r - (int64_t)a * s.K);
      val = (val - *s.c * s.u[a] * s.v[sn_col(m, s.cb)]) / *s.sigma;
    }
    dst[e] += scale * val;
  }
}

int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace

int64_t op_sn_scratch_floats(int ca, int K) {
  const int64_t rch = cdiv(ca, SN_ROWS), ct = cdiv(K, SN_CTILE), cch = cdiv(K, SN_CCHUNK), dch = cdiv((int64_t)ca * K, SN_DCHUNK);
  return gi_align_up(rch * K, 64) + gi_align_up(K, 64) + gi_align_up(ct, 64) + gi_align_up((int64_t)ca * cch, 64) + gi_align_up(ca, 64) +
         gi_align_up(dch, 64) + 64;
}

void op_sn_carve(SnJob& J, float* p) {
  J.rchunks = cdiv(J.ca, SN_ROWS); J.ctiles = cdiv(J.K, SN_CTILE); J.cchunks = cdiv(J.K, SN_CCHUNK);
  J.dchunks = cdiv((int64_t)J.ca * J.K, SN_DCHUNK);
  J.part_t = p; p += gi_align_up((int64_t)J.rchunks * J.K, 64);
  J.t_raw = p; p += gi_align_up(J.K, 64);
  J.nrm_part = p; p += gi_align_up(J.ctiles, 64);
  J.part_s = p; p += gi_align_up((int64_t)J.ca * J.cchunks, 64);
  J.s_vec = p; p += gi_align_up(J.ca, 64);
  J.dot_part = p; p += gi_align_up(J.dchunks, 64);
  J.c = p;
}

int op_sn_power_iteration(hipStream_t st, SnJobs& P, int iters, int train) {
  GI_REQUIRE(P.n >= 1 && P.n <= 6, "sn_power_iteration: %d tensors", P.n);
  GI_REQUIRE(iters >= 1, "sn_power_iteration: iters=%d", iters);
  int64_t nA = 0, nB = 0, nC = 0;
  for (int i = 0; i < P.n; ++i) {
    SnJob& J = P.j[i];
    GI_REQUIRE(J.w && J.u && J.v && J.sigma && J.part_t && J.ca >= 1 && J.K >= 1 && (J.cb == 0 || J.K == 16 * J.cb),
               "sn_power_iteration: tensor %d: ca=%d K=%d cb=%d", i, J.ca, J.K, J.cb);
    J.blk[0] = (int)nA; J.blk[1] = (int)nB; J.blk[2] = (int)nC;
    nA += (int64_t)J.rchunks * J.ctiles;
    nB += J.ctiles;
    nC += ((int64_t)J.ca * J.cchunks + 3) / 4;
    GI_REQUIRE(nA < (1 << 30) && nC < (1 << 30), "sn_power_iteration: tensor %d too large", i);
  }
  for (int it = 0; it < (train ? iters : 0); ++it) {
    hipLaunchKernelGGL(sn_wtu_partial_kernel, dim3((unsigned)nA), dim3(256), 0, st, P);
    hipLaunchKernelGGL(sn_wtu_finish_kernel, dim3((unsigned)nB), dim3(256), 0, st, P);
    hipLaunchKernelGGL(sn_wv_partial_kernel, dim3((unsigned)nC), dim3(256), 0, st, P, 1);
    hipLaunchKernelGGL(sn_u_sigma_kernel, dim3(P.n), dim3(256), 0, st, P, 1);
    GI_LAUNCH_CHECK();
  }
  if (!train) {
    hipLaunchKernelGGL(sn_wv_partial_kernel, dim3((unsigned)nC), dim3(256), 0, st, P, 0);
    hipLaunchKernelGGL(sn_u_sigma_kernel, dim3(P.n), dim3(256), 0, st, P, 0);
    GI_LAUNCH_CHECK();
  }
  return GI_OK;
}

namespace {
bool sn_vec_ok(const SnSegs& S, const void* a, const void* b, int64_t lo) {
  bool ok = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && lo % 4 == 0;
  for (int i = 0; i < S.n; ++i) ok = ok && S.s[i].off % 4 == 0;
  return ok;
}
}  // namespace

int op_sn_effective(hipStream_t st, const float* src, float* dst, int64_t count, const SnSegs& S) {
  if (sn_vec_ok(S, src, dst, 0))
    hipLaunchKernelGGL(sn_effective_kernel<true>, dim3(grid_for(count, 1024, 2048)), dim3(256), 0, st, src, dst, count, S);
  else
    hipLaunchKernelGGL(sn_effective_kernel<false>, dim3(grid_for(count, 256, 2048)), dim3(256), 0, st, src, dst, count, S);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int op_sn_project_add(hipStream_t st, SnJobs& P, const SnSegs& S, const float* g_flat, float* dst_flat, int64_t lo, int64_t hi,
                      const float* scale_dev) {
  GI_REQUIRE(P.n >= 0 && P.n <= 6 && S.n == P.n && lo <= hi, "sn_project_add: %d / %d tensors", P.n, S.n);
  int64_t nD = 0;
  for (int i = 0; i < P.n; ++i) {
    SnJob& J = P.j[i];
    GI_REQUIRE(J.g && J.w && J.dot_part && J.c && J.ca >= 1 && J.K >= 1, "sn_project_add: tensor %d", i);
    J.blk[3] = (int)nD;
    nD += J.dchunks;
  }
  if (P.n > 0) {
    hipLaunchKernelGGL(sn_dot_partial_kernel, dim3((unsigned)nD), dim3(256), 0, st, P);
    hipLaunchKernelGGL(sn_dot_finish_kernel, dim3(P.n), dim3(256), 0, st, P);
  }
  if (hi > lo && sn_vec_ok(S, g_flat, dst_flat, lo))
    hipLaunchKernelGGL(sn_project_add_kernel<true>, dim3(grid_for(hi - lo, 1024, 2048)), dim3(256), 0, st, g_flat, dst_flat, lo, hi, S, scale_dev);
  else if (hi > lo)
    hipLaunchKernelGGL(sn_project_add_kernel<false>, dim3(grid_for(hi - lo, 256, 2048)), dim3(256), 0, st, g_flat, dst_flat, lo, hi, S, scale_dev);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// ---- single-op entries (tests) ----------------------------------------------------------------------------------------------
namespace {
struct DevScratch {   // debug entries only: allocated and freed around the call (the stream is synchronised first)
  float* p = nullptr;
  ~DevScratch() { if (p) (void)hipFree(p); }
};
}  // namespace

extern "C" int gi_debug_sn_power_iteration(gi_ctx* ctx, const float* w, int ca, int K, int cb, float* u, float* v, int iters, int train,
                                           float* sigma_out) {
  GI_REQUIRE(ctx && w && u && v && sigma_out, "debug_sn_power_iteration: null pointer");
  GI_REQUIRE(ca >= 1 && K >= 1 && (int64_t)ca * K < (1ll << 31) && (cb == 0 || K == 16 * cb) && iters >= 1,
             "debug_sn_power_iteration: ca=%d K=%d cb=%d iters=%d", ca, K, cb, iters);
  DevScratch sc;
  GI_HIP(hipMalloc((void**)&sc.p, (size_t)op_sn_scratch_floats(ca, K) * 4));
  SnJobs P;
  P.n = 1;
  SnJob& J = P.j[0];
  J.w = w; J.u = u; J.v = v; J.sigma = sigma_out; J.ca = ca; J.K = K; J.cb = cb;
  op_sn_carve(J, sc.p);
  const int rc = op_sn_power_iteration(ctx->stream, P, iters, train);
  GI_HIP(hipStreamSynchronize(ctx->stream));
  return rc;
}

extern "C" int gi_debug_sn_project_add(gi_ctx* ctx, const float* g, const float* w_eff, const float* u, const float* v, const float* sigma,
                                       int ca, int K, int cb, const float* scale_dev, float* dst) {
  GI_REQUIRE(ctx && g && w_eff && u && v && sigma && dst, "debug_sn_project_add: null pointer");
  GI_REQUIRE(ca >= 1 && K >= 1 && (int64_t)ca * K < (1ll << 31) && (cb == 0 || K == 16 * cb), "debug_sn_project_add: ca=%d K=%d cb=%d", ca, K,
             cb);
  DevScratch sc;
  GI_HIP(hipMalloc((void**)&sc.p, (size_t)op_sn_scratch_floats(ca, K) * 4));
  SnJobs P;
  P.n = 1;
  SnJob& J = P.j[0];
  J.w = w_eff; J.g = g; J.ca = ca; J.K = K; J.cb = cb;
  op_sn_carve(J, sc.p);
  SnSegs S;
  S.n = 1;
  S.s[0] = SnSeg{0, (int64_t)ca * K, sigma, ca, K, cb, u, v, J.c};
  const int rc = op_sn_project_add(ctx->stream, P, S, g, dst, 0, (int64_t)ca * K, scale_dev);
  GI_HIP(hipStreamSynchronize(ctx->stream));
  return rc;
}
