// Distribution metrics on the 2048-wide pool3 features: the Kernel Inception Distance (Binkowski et al. 2018) and
// improved precision / recall (Kynkaanniemi et al. 2019). Both are reductions of a Gram matrix of feature rows, which is never
// stored: one 64 x 64 tile of G[i][j] = sum_k A[ia[i]][k] * B[ib[j]][k] per workgroup in fp64 (v_mfma_f64_16x16x4_f64, the fp32
// features widened on the way into LDS, which is exact), reduced by the epilogue of the kernel that computed it.
//
// Determinism. Every product of two widened fp32 values is exact in fp64, and an element's sum runs over K in ascending groups of
// four (one MFMA each) from zero, the tail zero-filled: its bits depend on the two feature rows alone, not on the tile, the
// position in the tile, the index lists or the size of the call. Every reduction after it has one fixed order (in-lane, then an
// xor butterfly, then the four waves, then the tiles by index); minima and integer counts do not depend on order. No float atomics.
#include "common.h"

namespace {

constexpr int FT = 64;         // tile edge: 4 waves, each a 32 x 32 quadrant = 2 x 2 MFMA blocks of 16 x 16
constexpr int FKC = 32;        // K per LDS chunk
constexpr int FLD = FKC + 2;   // doubles per LDS row: row stride 68 dwords = 4 mod 64, so the 16 rows x 2 k of a half-wave's
                               // ds_read_b64 fall on 32 distinct bank pairs
constexpr int FLDS_DOUBLES = 2 * FT * FLD;   // A and B chunk (34,816 bytes); the radius epilogue re-uses them for its 64 x 65 tile
typedef double d4_t __attribute__((ext_vector_type(4)));

struct GramOps {
  const float* A; const int* ia; int na;   // ia / ib null: the identity
  const float* B; const int* ib; int nb;
  int d;
};

// acc[i][j][reg] = G[row0 + 32 wr + 16 i + (lane >> 4) + 4 reg][col0 + 32 wc + 16 j + (lane & 15)], wave = 2 wr + wc.
// Rows >= na and columns >= nb are computed from zeros (the caller does not store them).
__device__ __forceinline__ void gram_tile(const GramOps& g, int row0, int col0, double* lds, int64_t* offs, d4_t (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* sA = lds;
  double* sB = lds + FT * FLD;
  __syncthreads();   // a previous use of lds / offs by this workgroup is over
  if (t < 2 * FT) {
    const bool isB = t >= FT;
    const int r = (isB ? col0 : row0) + (t & (FT - 1));
    const int n = isB ? g.nb : g.na;
    const int* idx = isB ? g.ib : g.ia;
    offs[t] = r < n ? (int64_t)(idx ? idx[r] : r) * g.d : (int64_t)-1;
  }
  __syncthreads();
  const int lr = t >> 5, lk = t & 31;   // this thread stages rows lr + 8 r, column lk of a chunk: 128 contiguous bytes per row
  float ra[8], rb[8];
  auto gload = [&](int k0) {
    const int k = k0 + lk;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int64_t oa = offs[lr + 8 * r], ob = offs[FT + lr + 8 * r];
      ra[r] = (oa >= 0 && k < g.d) ? g.A[oa + k] : 0.f;
      rb[r] = (ob >= 0 && k < g.d) ? g.B[ob + k] : 0.f;
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
  const int wr = wave >> 1, wc = wave & 1;
  const double* pa = sA + (32 * wr + (lane & 15)) * FLD + (lane >> 4);
  const double* pb = sB + (32 * wc + (lane & 15)) * FLD + (lane >> 4);
  gload(0);
  for (int k0 = 0; k0 < g.d; k0 += FKC) {
    __syncthreads();   // the previous chunk has been read
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      sA[(lr + 8 * r) * FLD + lk] = (double)ra[r];
      sB[(lr + 8 * r) * FLD + lk] = (double)rb[r];
    }
    __syncthreads();
    if (k0 + FKC < g.d) gload(k0 + FKC);   // in flight during the MFMAs below
#pragma unroll
    for (int kk = 0; kk < FKC; kk += 4) {
      const double a0 = pa[kk], a1 = pa[16 * FLD + kk], b0 = pb[kk], b1 = pb[16 * FLD + kk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

// f(i, j, reg, row, col) over this lane's 16 elements in one fixed order
template <typename F>
__device__ __forceinline__ void for_each_elem(int row0, int col0, F&& f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rb = row0 + 32 * (wave >> 1) + (lane >> 4), cb = col0 + 32 * (wave & 1) + (lane & 15);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) f(i, j, reg, rb + 16 * i + 4 * reg, cb + 16 * j);
}

__device__ __forceinline__ double block_sum_fixed(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ void __launch_bounds__(256) feat_gram_kernel(GramOps g, double* __restrict__ G) {
  __shared__ double lds[FLDS_DOUBLES];
  __shared__ int64_t offs[2 * FT];
  d4_t acc[2][2];
  const int row0 = blockIdx.y * FT, col0 = blockIdx.x * FT;
  gram_tile(g, row0, col0, lds, offs, acc);
  for_each_elem(row0, col0, [&](int i, int j, int reg, int r, int c) {
    if (r < g.na && c < g.nb) G[(int64_t)r * g.nb + c] = acc[i][j][reg];
  });
}

// grid (tiles, tiles, 3 n_subsets): z = 3 s + q, q = 0: sum_{i != j} k(x_i, x_j), 1: the same over y, 2: sum_{i, j} k(x_i, y_j);
// k = (G / d + 1)^3. The diagonal is skipped by position in the subset. G (and with it k) is symmetric bit for bit when both
// sides are one list, so for q < 2 only the tiles on and above the diagonal are computed and the others' share is their mirror's:
// twice the partial sum, which is exact.
struct KidArgs {
  const float* X; const float* Y; const int* ix; const int* iy;
  int m, d, tiles;
  double* part;   // [3 n_subsets][tiles][tiles]
};
__global__ void __launch_bounds__(256) feat_kid_kernel(KidArgs a) {
  __shared__ double lds[FLDS_DOUBLES];
  __shared__ int64_t offs[2 * FT];
  __shared__ double sh[4];
  const int z = blockIdx.z, s = z / 3, q = z - 3 * s;
  double* out = a.part + ((int64_t)z * a.tiles + blockIdx.y) * a.tiles + blockIdx.x;
  if (q < 2 && blockIdx.x < blockIdx.y) {   // (workgroup-uniform)
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  const int* lx = a.ix + (int64_t)s * a.m;
  const int* ly = a.iy + (int64_t)s * a.m;
  GramOps g;
  g.A = q == 1 ? a.Y : a.X; g.ia = q == 1 ? ly : lx; g.na = a.m;
  g.B = q == 0 ? a.X : a.Y; g.ib = q == 0 ? lx : ly; g.nb = a.m;
  g.d = a.d;
  d4_t acc[2][2];
  const int row0 = blockIdx.y * FT, col0 = blockIdx.x * FT;
  gram_tile(g, row0, col0, lds, offs, acc);
  const double dd = (double)a.d;
  double sum = 0.0;
  for_each_elem(row0, col0, [&](int i, int j, int reg, int r, int c) {
    if (r < a.m && c < a.m && !(q < 2 && r == c)) {
      const double tt = acc[i][j][reg] / dd + 1.0;
      sum += tt * tt * tt;
    }
  });
  sum = block_sum_fixed(sum, sh);
  if (threadIdx.x == 0) *out = (q < 2 && blockIdx.x > blockIdx.y) ? 2.0 * sum : sum;
}
// sums[z] = part[z][0] + part[z][1] + ... : strided over 256 threads in ascending order, then the fixed block sum
__global__ void __launch_bounds__(256) feat_kid_final_kernel(const double* __restrict__ part, int per, double* __restrict__ sums) {
  __shared__ double sh[4];
  const double* p = part + (int64_t)blockIdx.x * per;
  double v = 0.0;
  for (int i = threadIdx.x; i < per; i += 256) v += p[i];
  v = block_sum_fixed(v, sh);
  if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// nrm[i] = sum_k a_ik^2: one wave per row, lane l adds k = l, l + 64, ... in ascending order, then the xor butterfly
__global__ void __launch_bounds__(256) feat_rownorm_kernel(const float* __restrict__ A, int n, int d, double* __restrict__ nrm) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* a = A + (int64_t)row * d;
  double v = 0.0;
  for (int k = lane; k < d; k += 64) {
    const double x = (double)a[k];
    v += x * x;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if (lane == 0) nrm[row] = v;
}

__device__ __forceinline__ double feat_dist(double ni, double nj, double gij) {
  const double v = (ni + nj) - 2.0 * gij;
  return v > 0.0 ? v : 0.0;
}

// grid (ctiles, rtiles): the kk = min(k, 64) smallest D_ij of every row of the tile over the tile's columns j != i, ascending, to
// part[row][column tile][kk] (+inf where the tile has fewer). Selection by repeated minimum over (value, column) pairs in
// lexicographic order: ties count once per column, no array indexed at run time.
struct RadArgs {
  const float* A; int n, d, k, kk, ctiles;
  const double* nrm;
  double* part;   // [n][ctiles][kk]
};
__global__ void __launch_bounds__(256) feat_knn_tile_kernel(RadArgs a) {
  __shared__ double lds[FLDS_DOUBLES];
  __shared__ int64_t offs[2 * FT];
  GramOps g;
  g.A = a.A; g.ia = nullptr; g.na = a.n; g.B = a.A; g.ib = nullptr; g.nb = a.n; g.d = a.d;
  d4_t acc[2][2];
  const int row0 = blockIdx.y * FT, col0 = blockIdx.x * FT;
  gram_tile(g, row0, col0, lds, offs, acc);
  __syncthreads();   // every wave has read its last chunk: the operand space becomes the 64 x 65 distance tile
  const double inf = __builtin_huge_val();
  for_each_elem(row0, col0, [&](int i, int j, int reg, int r, int c) {
    double v = inf;
    if (r < a.n && c < a.n && r != c) v = feat_dist(a.nrm[r], a.nrm[c], acc[i][j][reg]);
    lds[(r - row0) * (FT + 1) + (c - col0)] = v;
  });
  __syncthreads();
  const int t = threadIdx.x, r = row0 + t;
  if (t >= FT || r >= a.n) return;
  const double* drow = lds + t * (FT + 1);
  double* out = a.part + ((int64_t)r * a.ctiles + blockIdx.x) * a.kk;
  double pv = -inf;
  int pj = -1;
  for (int p = 0; p < a.kk; ++p) {
    double bv = inf;
    int bj = FT;
    for (int j = 0; j < FT; ++j) {
      const double v = drow[j];
      if ((v > pv || (v == pv && j > pj)) && v < bv) { bv = v; bj = j; }
    }
    out[p] = bv;
    pv = bv;
    pj = bj;
    if (bj == FT) {   // nothing finite is left: the rest is +inf
      for (int p2 = p + 1; p2 < a.kk; ++p2) out[p2] = inf;
      break;
    }
  }
}
// radii[row] = the k-th smallest of the row's `len` candidates: one wave per row, k rounds of the lexicographic minimum
__global__ void __launch_bounds__(256) feat_knn_merge_kernel(const double* __restrict__ part, int n, int64_t len, int k,
                                                             double* __restrict__ radii) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* p = part + (int64_t)row * len;
  const double inf = __builtin_huge_val();
  double pv = -inf;
  long long pj = -1;
  for (int round = 0; round < k; ++round) {
    double bv = inf;
    long long bj = len;
    for (long long j = lane; j < len; j += 64) {
      const double v = p[j];
      if ((v > pv || (v == pv && j > pj)) && v < bv) { bv = v; bj = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off);
      const long long oj = __shfl_xor(bj, off);
      if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
    }
    pv = bv;
    pj = bj;
  }
  if (lane == 0) radii[row] = pv;
}

// grid (tiles over B's rows, tiles over A's rows): member[j] = 1 when some row i of this tile has D(a_i, b_j) <= radii[i]. member is
// zeroed before the launch; every writer stores the same 1.
struct MemArgs {
  const float* A; int na; const float* B; int nb; int d;
  const double* radii; const double* nrmA; const double* nrmB;
  uint8_t* member;
};
__global__ void __launch_bounds__(256) feat_member_kernel(MemArgs a) {
  __shared__ double lds[FLDS_DOUBLES];
  __shared__ int64_t offs[2 * FT];
  GramOps g;
  g.A = a.A; g.ia = nullptr; g.na = a.na; g.B = a.B; g.ib = nullptr; g.nb = a.nb; g.d = a.d;
  d4_t acc[2][2];
  const int row0 = blockIdx.y * FT, col0 = blockIdx.x * FT;
  gram_tile(g, row0, col0, lds, offs, acc);
  int hit[2] = {0, 0};
  for_each_elem(row0, col0, [&](int i, int j, int reg, int r, int c) {
    if (r < a.na && c < a.nb && feat_dist(a.nrmA[r], a.nrmB[c], acc[i][j][reg]) <= a.radii[r]) hit[j] = 1;
  });
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int h = hit[j];
    h |= __shfl_xor(h, 16);
    h |= __shfl_xor(h, 32);
    const int c = col0 + 32 * (wave & 1) + 16 * j + lane;
    if (lane < 16 && h && c < a.nb) a.member[c] = 1;
  }
}
__global__ void __launch_bounds__(256) feat_count_kernel(const uint8_t* __restrict__ member, int n, int* __restrict__ count) {
  __shared__ int sh[4];
  int v = 0;
  for (int i = threadIdx.x; i < n; i += 256) v += member[i] != 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *count = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

inline int ftiles(int64_t n) { return (int)((n + FT - 1) / FT); }
constexpr int FEAT_MAX_ROWS = 1 << 22;   // 65,535 tiles on a grid axis

}  // namespace

extern "C" {

int64_t gi_featmetrics_workspace_bytes(int op, int64_t n, int64_t n2, int count) {
  if (n < 1 || n > FEAT_MAX_ROWS) return -1;
  const int64_t T = ftiles(n);
  switch (op) {
    case GI_FEAT_WS_KID: return count >= 1 ? 8 * 3 * (int64_t)count * T * T : -1;
    case GI_FEAT_WS_RADIUS: return count >= 1 ? 8 * (n + n * T * (count < FT ? count : FT)) : -1;
    case GI_FEAT_WS_MEMBERS: return (n2 >= 1 && n2 <= FEAT_MAX_ROWS) ? 8 * (n + n2) : -1;
    default: return -1;
  }
}

int gi_debug_feat_gram(gi_ctx* ctx, const float* A, const int* ia, int na, const float* B, const int* ib, int nb, int d, double* G) {
  GI_REQUIRE(ctx && A && B && G, "feat_gram: null argument");
  GI_REQUIRE(na >= 1 && nb >= 1 && na <= FEAT_MAX_ROWS && nb <= FEAT_MAX_ROWS, "feat_gram: na=%d nb=%d (1..%d)", na, nb, FEAT_MAX_ROWS);
  GI_REQUIRE(d >= 1 && d <= 8192, "feat_gram: d=%d (1..8192)", d);
  GramOps g;
  g.A = A; g.ia = ia; g.na = na; g.B = B; g.ib = ib; g.nb = nb; g.d = d;
  hipLaunchKernelGGL(feat_gram_kernel, dim3(ftiles(nb), ftiles(na)), dim3(256), 0, ctx->stream, g, G);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_kid_subset_sums(gi_ctx* ctx, const float* X, const float* Y, const int* ix, const int* iy, int n_subsets, int m, int d, void* ws,
                       int64_t ws_bytes, double* sums) {
  GI_REQUIRE(ctx && X && Y && ix && iy && ws && sums, "kid_subset_sums: null argument");
  GI_REQUIRE(d >= 1 && d <= 8192, "kid_subset_sums: d=%d (1..8192)", d);
  GI_REQUIRE(m >= 2 && m <= FEAT_MAX_ROWS, "kid_subset_sums: m=%d (2..%d): the unbiased estimator divides by m (m - 1)", m, FEAT_MAX_ROWS);
  GI_REQUIRE(n_subsets >= 1 && n_subsets <= 65535 / 3, "kid_subset_sums: n_subsets=%d (1..%d)", n_subsets, 65535 / 3);
  const int64_t need = gi_featmetrics_workspace_bytes(GI_FEAT_WS_KID, m, 0, n_subsets);
  GI_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "kid_subset_sums: workspace of %lld bytes, %lld needed (8-byte aligned)",
             (long long)ws_bytes, (long long)need);
  KidArgs a;
  a.X = X; a.Y = Y; a.ix = ix; a.iy = iy; a.m = m; a.d = d; a.tiles = ftiles(m); a.part = (double*)ws;
  hipLaunchKernelGGL(feat_kid_kernel, dim3(a.tiles, a.tiles, 3 * n_subsets), dim3(256), 0, ctx->stream, a);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(feat_kid_final_kernel, dim3(3 * n_subsets), dim3(256), 0, ctx->stream, (const double*)ws, a.tiles * a.tiles, sums);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_feat_knn_radius(gi_ctx* ctx, const float* A, int n, int d, int k, void* ws, int64_t ws_bytes, double* radii) {
  GI_REQUIRE(ctx && A && ws && radii, "feat_knn_radius: null argument");
  GI_REQUIRE(d >= 1 && d <= 8192, "feat_knn_radius: d=%d (1..8192)", d);
  GI_REQUIRE(n >= 2 && n <= FEAT_MAX_ROWS, "feat_knn_radius: n=%d (2..%d)", n, FEAT_MAX_ROWS);
  GI_REQUIRE(k >= 1 && k < n, "feat_knn_radius: k=%d needs 1 <= k < n=%d (a row is not its own neighbour)", k, n);
  const int64_t need = gi_featmetrics_workspace_bytes(GI_FEAT_WS_RADIUS, n, 0, k);
  GI_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "feat_knn_radius: workspace of %lld bytes, %lld needed (8-byte aligned)",
             (long long)ws_bytes, (long long)need);
  RadArgs a;
  a.A = A; a.n = n; a.d = d; a.k = k; a.kk = k < FT ? k : FT; a.ctiles = ftiles(n);
  double* nrm = (double*)ws;
  a.nrm = nrm; a.part = nrm + n;
  hipLaunchKernelGGL(feat_rownorm_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, A, n, d, nrm);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(feat_knn_tile_kernel, dim3(a.ctiles, a.ctiles), dim3(256), 0, ctx->stream, a);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(feat_knn_merge_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, (const double*)a.part, n,
                     (int64_t)a.ctiles * a.kk, k, radii);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_feat_manifold_members(gi_ctx* ctx, const float* A, int na, const double* radii, const float* B, int nb, int d, void* ws,
                             int64_t ws_bytes, uint8_t* member, int* count) {
  GI_REQUIRE(ctx && A && radii && B && ws && member && count, "feat_manifold_members: null argument");
  GI_REQUIRE(d >= 1 && d <= 8192, "feat_manifold_members: d=%d (1..8192)", d);
  GI_REQUIRE(na >= 1 && nb >= 1 && na <= FEAT_MAX_ROWS && nb <= FEAT_MAX_ROWS, "feat_manifold_members: na=%d nb=%d (1..%d)", na, nb,
             FEAT_MAX_ROWS);
  const int64_t need = gi_featmetrics_workspace_bytes(GI_FEAT_WS_MEMBERS, na, nb, 0);
  GI_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "feat_manifold_members: workspace of %lld bytes, %lld needed (8-byte aligned)",
             (long long)ws_bytes, (long long)need);
  MemArgs a;
  double* nrm = (double*)ws;
  a.A = A; a.na = na; a.B = B; a.nb = nb; a.d = d; a.radii = radii; a.nrmA = nrm; a.nrmB = nrm + na; a.member = member;
  hipLaunchKernelGGL(feat_rownorm_kernel, dim3((na + 3) / 4), dim3(256), 0, ctx->stream, A, na, d, nrm);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(feat_rownorm_kernel, dim3((nb + 3) / 4), dim3(256), 0, ctx->stream, B, nb, d, nrm + na);
  GI_LAUNCH_CHECK();
  GI_HIP(hipMemsetAsync(member, 0, (size_t)nb, ctx->stream));
  hipLaunchKernelGGL(feat_member_kernel, dim3(ftiles(nb), ftiles(na)), dim3(256), 0, ctx->stream, a);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(feat_count_kernel, dim3(1), dim3(256), 0, ctx->stream, (const uint8_t*)member, nb, count);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // extern "C"
