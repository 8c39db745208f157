// Connected components of a hole mask (NOT in the reference): what splits a mask into its holes on the device, so that
// lib/inpaint.py can plan one window per group of holes. tests/components_ref.py is the Python restatement, exact in every output.
//
//   gi_mask_components  labels (the smallest linear index of each pixel's component, -1 on background), the number of components,
//                       and per component in label order (label, y0, x0, y1, x1, area)
//
// Seven launches on the context's stream, the kernel boundary the only hand-off between workgroups:
//   local     one workgroup per CT x CT tile: union-find of the tile in LDS, labels = the global index of the tile-local root
//   merge     the pixels on tile borders: unions across the border in global memory, atomicMin links of the larger root to the smaller
//   compress  the same pixels: every tile-local root that took part in a merge is pointed at its final root
//   flatten   every pixel reads its final root (at most two hops) and stores it; roots (labels[p] == p) are counted per chunk
//   scan      exclusive prefix sum of the chunk counts: the rank of every chunk's first root, and the total
//   collect   roots in label order: rank[root] = k, table row k initialised
//   stats     box and area by integer min / max / add, one update per run of equal labels in a row (per wave for the long ones)
// Integer atomics only. A label is the minimum of a set and a table entry an integer min / max / sum: no output depends on the order
// in which workgroups run. The union-find invariant everywhere: L[x] <= x and L[x] is a pixel of x's component, so the smallest pixel
// of a component is always a root and in the end the only one. A stale read (the XCDs' L2 caches are not coherent inside a launch)
// yields an older link, which is still a link to a smaller pixel of the same component: it can cost a step, never a wrong union,
// because every write of the merge and compress launches is an atomicMin performed at memory.
#include <limits.h>

#include "common.h"

namespace {

constexpr int CT = 64;                 // tile side: 4096 labels (16 KB) + 4096 hole flags (4 KB) of LDS
constexpr int CT_PIX = CT * CT;
constexpr int CHUNK = 256 * 16;        // pixels per workgroup of the linear passes: 16 consecutive pixels per thread

// ---- tile-local union-find in LDS ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(const volatile int* L, int a) {
  // ends: L[x] <= x for every x at all times, so p != a means p < a: a strictly decreases and is bounded by 0
  for (int p = L[a]; p != a; p = L[a]) a = p;
  return a;
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  // ends: an iteration that does not return replaces a by old < a (or by a root found below it) and leaves b at or below its value:
  // a + b strictly decreases and is bounded by 0. No lane waits for another one.
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);   // a was a root when read: link it below b
    if (old == a) return;                   // it still was: linked
    a = old;                                // someone linked a to old < a first; L[a] = min(old, b) now, so old and b remain to be joined
  }
}

struct CompP {
  const uint8_t* mask;
  int* labels;
  int H, W, conn;
  unsigned tiles_x;
};

__global__ void __launch_bounds__(256) cc_local_kernel(CompP p) {
  __shared__ int s_L[CT_PIX];
  __shared__ uint32_t s_hw[CT_PIX / 4];
  uint8_t* s_h = (uint8_t*)s_hw;
  const int tid = threadIdx.x;
  const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int ty0 = (int)tile_y * CT, tx0 = (int)tile_x * CT;
  // hole flags, a wave per 64 consecutive bytes of a row; outside the image: background
  for (int k = 0; k < 16; ++k) {
    const int i = tid + 256 * k, ly = i >> 6, lx = i & 63;
    const int gy = ty0 + ly, gx = tx0 + lx;
    uint8_t h = 0;
    if (gy < p.H && gx < p.W) h = p.mask[(int64_t)gy * p.W + gx] != 0;
    s_h[i] = h;
  }
  __syncthreads();
  // a thread owns 16 consecutive pixels of one tile row: bit k of `own` = pixel k, bit k + 1 of `up` = the pixel above pixel k
  const int ly = tid >> 2, seg = tid & 3, i0 = ly * CT + seg * 16;
  uint32_t own = 0, up = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t w = s_hw[(i0 >> 2) + q];
#pragma unroll
    for (int e = 0; e < 4; ++e) own |= ((w >> (8 * e)) & 1u) << (4 * q + e);
  }
  const bool left_in = seg > 0 && s_h[i0 - 1] != 0;
  if (ly > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t w = s_hw[((i0 - CT) >> 2) + q];
#pragma unroll
      for (int e = 0; e < 4; ++e) up |= ((w >> (8 * e)) & 1u) << (4 * q + e + 1);
    }
    if (seg > 0 && s_h[i0 - CT - 1]) up |= 1u;
    if (seg < 3 && s_h[i0 - CT + 16]) up |= 1u << 17;
  }
  // runs inside the 16 pixels point at their first pixel
  int start = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const bool h = (own >> k) & 1u, hl = k > 0 && ((own >> (k - 1)) & 1u);
    if (h && !hl) start = i0 + k;
    s_L[i0 + k] = h ? start : -1;
  }
  __syncthreads();
  // unions with the previous row and across the 16-pixel seams. A pixel whose left neighbour and the pixel above that one are both
  // holes needs no union with the pixel above itself: by induction along the row, left ~ above-left, and the rows join the rest.
  const bool c8 = p.conn == 8;
  for (int k = 0; k < 16; ++k) {
    if (!((own >> k) & 1u)) continue;
    const int i = i0 + k;
    const bool left = k > 0 ? ((own >> (k - 1)) & 1u) != 0 : left_in;
    if (k == 0 && left) lds_union(s_L, i, i - 1);
    const bool ul = (up >> k) & 1u, u = (up >> (k + 1)) & 1u, ur = (up >> (k + 2)) & 1u;
    if (u) {
      if (!(left && ul)) lds_union(s_L, i, i - CT);
    } else if (c8) {
      if (ul && !left) lds_union(s_L, i, i - CT - 1);
      if (ur) lds_union(s_L, i, i - CT + 1);
    }
  }
  __syncthreads();
  // local order equals global order inside a tile (both row-major): the local root is the tile component's smallest global index
  for (int k = 0; k < 16; ++k) {
    const int i = tid + 256 * k, y = i >> 6, x = i & 63;
    const int gy = ty0 + y, gx = tx0 + x;
    if (gy >= p.H || gx >= p.W) continue;
    int v = s_L[i];
    if (v >= 0) {
      const int r = lds_find(s_L, v);
      v = (ty0 + (r >> 6)) * p.W + tx0 + (r & 63);
    }
    p.labels[(int64_t)gy * p.W + gx] = v;
  }
}

// ---- unions across tile borders in global memory --------------------------------------------------------------------------------------
__device__ __forceinline__ int g_load(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(const int* L, int a) {
  // ends: L[x] <= x always (links go to smaller indices only, a stale value included), so a strictly decreases, bounded by 0
  for (int p = g_load(L, a); p != a; p = g_load(L, a)) a = p;
  return a;
}
// the same with path halving: a visited root is linked to its grandparent (an atomicMin with a smaller pixel of the same component
// keeps the invariant). Called with roots of tiles only, so the label of a pixel that is no tile root is never written here.
__device__ __forceinline__ int g_find_halve(int* L, int a) {
  int p = g_load(L, a);
  // ends: p != a means p < a, and a takes the value of p: a strictly decreases, bounded by 0
  while (p != a) {
    const int g = g_load(L, p);
    if (g != p) atomicMin(&L[a], g);
    a = p;
    p = g;
  }
  return a;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
  a = g_load(L, a);   // the tile-local roots (or the pixels themselves)
  b = g_load(L, b);
  // ends: as lds_union: a + b strictly decreases with every iteration that does not return
  for (;;) {
    a = g_find_halve(L, a);
    b = g_find_halve(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}
__device__ __forceinline__ void g_compress(int* L, int a) {
  const int t = g_load(L, a);           // a's tile-local root: the merge launch never wrote the label of a pixel that is none
  const int r = g_find(L, t);           // every union is done (kernel boundary): r is the component's final root
  if (r != t) atomicMin(&L[t], r);
}

// f(pixel, neighbour) for the pairs of hole pixels that are neighbours across a tile border, the pixel being the later one in
// raster order, that the other pairs do not already imply. Threads 0 .. 63: the tile's top row (up, and with 8 neighbours up-left and up-right); 64 .. 127: the left column
// (left, and up-left below the top row); 128 .. 191: the right column (up-right below the top row, 8 neighbours only).
template <typename F>
__device__ __forceinline__ void for_border_pairs(const CompP& p, F&& f) {
  const int tid = threadIdx.x;
  if (tid >= 3 * CT) return;
  const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int role = tid >> 6, j = tid & 63;
  const int ly = role == 0 ? 0 : j, lx = role == 0 ? j : (role == 1 ? 0 : CT - 1);
  const int gy = (int)tile_y * CT + ly, gx = (int)tile_x * CT + lx;
  if (gy >= p.H || gx >= p.W) return;
  const int W = p.W, i = gy * W + gx;     // < 2^31
  if (p.labels[i] < 0) return;            // (a label's sign never changes)
  const bool c8 = p.conn == 8;
  const int* L = p.labels;
  auto hole = [&](int n) { return L[n] >= 0; };
  // Pairs that other pairs imply are skipped, as in the local launch. Two claims hold for the final forest, each by induction:
  //   rows     a top-row pixel and the hole above it are joined (induction along the row, towards smaller x, across tiles);
  //   columns  a left-column pixel and the hole left of it are joined (induction up the column, to the tile's top row, which always pairs).
  if (role == 0) {
    if (gy == 0) return;
    const bool left = gx > 0 && hole(i - 1), ul = gx > 0 && hole(i - W - 1);
    if (hole(i - W)) {
      if (!(left && ul)) f(i, i - W);      // else: pixel ~ left (local, or columns), left ~ up-left (rows), up-left ~ up (local, or columns)
    } else if (c8) {
      if (ul && !left) f(i, i - W - 1);    // (left: left ~ up-left by rows)
      if (gx + 1 < W && hole(i - W + 1)) f(i, i - W + 1);
    }
  } else if (role == 1) {
    if (gx == 0) return;
    const bool left = hole(i - 1), up = ly > 0 && hole(i - W), ul = ly > 0 && hole(i - W - 1);   // (ly > 0: gy > 0)
    if (left) {
      if (!(up && ul)) f(i, i - 1);        // else: pixel ~ up (local), up ~ up-left (columns), up-left ~ left (local in the left tile)
    } else if (c8 && ul && !up) {
      f(i, i - W - 1);                     // (up: up ~ up-left by columns)
    }
  } else if (c8 && ly > 0 && gx + 1 < W) {
    // up-right lies in the next tile: implied when the pixel above (its left neighbour) or the pixel to the right (below it) is a hole
    if (hole(i - W + 1) && !hole(i - W) && !hole(i + 1)) f(i, i - W + 1);
  }
}

__global__ void __launch_bounds__(256) cc_merge_kernel(CompP p) {
  for_border_pairs(p, [&](int a, int b) { g_union(p.labels, a, b); });
}
__global__ void __launch_bounds__(256) cc_compress_kernel(CompP p) {
  for_border_pairs(p, [&](int a, int b) { g_compress(p.labels, a); g_compress(p.labels, b); });
}

// ---- final labels, roots in label order -----------------------------------------------------------------------------------------------
// After the compress launch a pixel's label is a tile-local root whose label is the final root: two reads. The only writes of this
// launch are each thread's own labels, with their final values.
__global__ void __launch_bounds__(256) cc_flatten_kernel(int* labels, unsigned HW, int* __restrict__ chunk_roots) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i0 = blockIdx.x * (unsigned)CHUNK + threadIdx.x * 16u;   // < 2^31 + 4096
  int n = 0;
  for (unsigned k = 0; k < 16 && i0 + k < HW; ++k) {
    const int i = (int)(i0 + k);
    int a = labels[i];
    if (a < 0) continue;
    // ends: labels[x] <= x, so a strictly decreases while it is not a root (at most two steps after the compress launch)
    for (int q = labels[a]; q != a; q = labels[a]) a = q;
    labels[i] = a;
    n += a == i;
  }
  if (n) atomicAdd(&s_n, n);
  __syncthreads();
  if (threadIdx.x == 0) chunk_roots[blockIdx.x] = s_n;
}

// chunk_roots -> exclusive prefix sums in place, the total to count_out. One workgroup; a thread owns a contiguous slice.
__global__ void __launch_bounds__(256) cc_scan_kernel(int* __restrict__ chunk_roots, unsigned chunks, int* __restrict__ count_out, int* __restrict__ limit) {
  __shared__ int s_sum[256];
  const unsigned per = (chunks + 255u) / 256u, a = threadIdx.x * per, b = min(a + per, chunks);
  int s = 0;
  for (unsigned i = a; i < b; ++i) s += chunk_roots[i];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  int run = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) run += s_sum[t];
  if (threadIdx.x == 255) *count_out = run + s;
  if (threadIdx.x == 0) *limit = INT_MAX;   // the largest label with a table row: the collect launch lowers it when there are more than cap
  for (unsigned i = a; i < b; ++i) {
    const int c = chunk_roots[i];
    chunk_roots[i] = run;
    run += c;
  }
}

// rank[root] = its place in label order; row k < cap of the table: (label, H, W, -1, -1, 0), the neutral elements of the stats launch
__global__ void __launch_bounds__(256) cc_collect_kernel(const int* __restrict__ labels, unsigned HW, int H, int W, const int* __restrict__ chunk_first,
                                                         int cap, int* __restrict__ rank, int* __restrict__ table, int* __restrict__ limit) {
  __shared__ int s_cnt[256];
  const unsigned i0 = blockIdx.x * (unsigned)CHUNK + threadIdx.x * 16u;
  uint32_t roots = 0;
  for (unsigned k = 0; k < 16 && i0 + k < HW; ++k) roots |= (uint32_t)(labels[i0 + k] == (int)(i0 + k)) << k;
  s_cnt[threadIdx.x] = __popc(roots);
  __syncthreads();
  if (!roots) return;
  int r = chunk_first[blockIdx.x];
  for (int t = 0; t < (int)threadIdx.x; ++t) r += s_cnt[t];
  for (unsigned k = 0; k < 16; ++k) {
    if (!((roots >> k) & 1u)) continue;
    rank[i0 + k] = r;
    if (r < cap) {
      int* row = table + 6 * r;
      row[0] = (int)(i0 + k); row[1] = H; row[2] = W; row[3] = -1; row[4] = -1; row[5] = 0;
      if (r == cap - 1) *limit = (int)(i0 + k);   // (one thread of the launch)
    }
    ++r;
  }
}

// one update of a component's row: the box grows to (ya .. yb, xa .. xb), the area by n
__device__ __forceinline__ void cc_emit(const int* rank, int limit, int* table, int label, int ya, int yb, int xa, int xb, int n) {
  if (label > limit) return;   // no table row: spares the read of its rank (a mask of many small components is all such labels)
  const int k = rank[label];
  int* row = table + 6 * k;
  atomicMin(row + 1, ya); atomicMin(row + 2, xa);
  atomicMax(row + 3, yb); atomicMax(row + 4, xb);
  atomicAdd(row + 5, n);
}

constexpr int SR = 8;    // rows and
constexpr int SG = 8;    // groups of 64 columns per wave of the stats launch

// A wave per SR rows x 64 SG columns, a lane per pixel of 64 consecutive ones: the loads coalesce. A run of equal labels that begins
// and ends inside the 64 pixels is one update by the lane of its first pixel (ballot of the lanes whose label differs from their left
// neighbour's). The run that reaches the end of the 64 is carried into the next 64 (wave-uniform: label and first x), so a run is one
// update however long; and lane 0 keeps the carried runs of one label in registers across the wave's rows (the inside of a large
// hole: one update per wave, not per row).
__global__ void __launch_bounds__(256) cc_stats_kernel(const int* __restrict__ labels, int H, int W, unsigned spans, const int* __restrict__ rank,
                                                       const int* __restrict__ limit_p, int* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  const int limit = *limit_p;
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned rb = wave / spans, s = wave - rb * spans;
  const unsigned y0 = rb * SR;
  if (y0 >= (unsigned)H) return;   // (the whole wave)
  const unsigned xbase = s * (64u * SG), uW = (unsigned)W;   // xbase < W: no sum below wraps
  const int xend = (int)min(xbase + 64u * SG, uW) - 1;     // the last pixel of the span
  int a_lab = -1, a_y0 = 0, a_y1 = 0, a_x0 = 0, a_x1 = 0, a_n = 0;   // lane 0: the carried runs of one label
  auto acc_add = [&](int lab, int y, int xa, int xb) {
    if (lab == a_lab) {
      a_y1 = y; a_x0 = min(a_x0, xa); a_x1 = max(a_x1, xb); a_n += xb - xa + 1;
    } else {
      if (a_lab >= 0) cc_emit(rank, limit, table, a_lab, a_y0, a_y1, a_x0, a_x1, a_n);
      a_lab = lab; a_y0 = a_y1 = y; a_x0 = xa; a_x1 = xb; a_n = xb - xa + 1;
    }
  };
  for (unsigned r = 0; r < SR && y0 + r < (unsigned)H; ++r) {
    const int y = (int)(y0 + r);
    const int* row = labels + (int64_t)y * W;
    int v[SG];
#pragma unroll
    for (int g = 0; g < SG; ++g) {
      const unsigned x = xbase + 64u * g + lane;
      v[g] = x < uW ? row[x] : -2;   // -2: no pixel, equal to no label and not to the background
    }
    int p_lab = -2, p_xs = 0;   // the run carried from the pixels before (wave-uniform)
#pragma unroll
    for (int g = 0; g < SG; ++g) {
      const unsigned xg = xbase + 64u * g;
      if (xg < uW) {   // (wave-uniform)
        const int prev = __shfl_up(v[g], 1);
        const bool is_brk = lane == 0 ? v[g] != p_lab : v[g] != prev;
        const unsigned long long brk = __ballot(is_brk);
        if (brk) {
          const int first = __ffsll((long long)brk) - 1, last = 63 - __clzll((long long)brk);
          if (lane == 0 && p_lab >= 0) acc_add(p_lab, y, p_xs, (int)xg + first - 1);   // the carried run ends in front of the first break
          if (is_brk && v[g] >= 0) {
            const unsigned long long later = lane < 63 ? brk >> (lane + 1) : 0ull;
            if (later) cc_emit(rank, limit, table, v[g], y, y, (int)xg + lane, (int)xg + lane + __ffsll((long long)later) - 1, __ffsll((long long)later));
          }
          p_lab = __shfl(v[g], last);   // the run of the last break is carried on
          p_xs = (int)xg + last;
        }
      }
    }
    if (lane == 0 && p_lab >= 0) acc_add(p_lab, y, p_xs, xend);
  }
  if (lane == 0 && a_lab >= 0) cc_emit(rank, limit, table, a_lab, a_y0, a_y1, a_x0, a_x1, a_n);
}

static inline unsigned cc_chunks(int64_t HW) { return (unsigned)((HW + CHUNK - 1) / CHUNK); }
static inline bool cc_size_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < 0x7fffffffll - 32; }

}  // namespace

extern "C" {

size_t gi_mask_components_workspace_bytes(int H, int W, int cap) {
  if (!cc_size_ok(H, W) || cap < 1 || cap > 65536) return 0;
  const int64_t HW = (int64_t)H * W;
  return (size_t)gi_align_up((HW + cc_chunks(HW) + 1) * 4, 256);   // rank (H, W) + the chunks' root counts + the label limit
}

int gi_mask_components(gi_ctx* ctx, const uint8_t* mask, int H, int W, int connectivity, int cap, int* labels_out, int* count_out,
                       int* table_out, void* workspace) {
  GI_REQUIRE(ctx && mask && labels_out && count_out && table_out && workspace, "mask_components: null argument");
  GI_REQUIRE(connectivity == 4 || connectivity == 8, "mask_components: connectivity = %d (4 or 8)", connectivity);
  GI_REQUIRE(cap >= 1 && cap <= 65536, "mask_components: cap = %d (1 .. 65536)", cap);
  GI_REQUIRE(cc_size_ok(H, W), "mask_components: %d x %d is empty or its pixels do not fit 31 bits", H, W);
  GI_REQUIRE((((uintptr_t)labels_out | (uintptr_t)count_out | (uintptr_t)table_out | (uintptr_t)workspace) & 3) == 0,
             "mask_components: labels, count, table and workspace are 4-byte aligned");
  const unsigned HW = (unsigned)H * (unsigned)W, chunks = cc_chunks(HW);
  const unsigned tiles_x = (unsigned)(W + CT - 1) / CT, tiles_y = (unsigned)(H + CT - 1) / CT;   // tiles_x * tiles_y <= HW / CT + 1 + tiles of one row / column < 2^26
  int* rank = (int*)workspace;
  int* chunk_roots = rank + HW;
  int* limit = chunk_roots + chunks;
  CompP p;
  p.mask = mask; p.labels = labels_out; p.H = H; p.W = W; p.conn = connectivity; p.tiles_x = tiles_x;
  const unsigned tiles = tiles_x * tiles_y;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(cc_local_kernel, dim3(tiles), dim3(256), 0, st, p);
  GI_LAUNCH_CHECK();
  if (tiles > 1) {
    hipLaunchKernelGGL(cc_merge_kernel, dim3(tiles), dim3(256), 0, st, p);
    GI_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_compress_kernel, dim3(tiles), dim3(256), 0, st, p);
    GI_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(chunks), dim3(256), 0, st, labels_out, HW, chunk_roots);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(256), 0, st, chunk_roots, chunks, count_out, limit);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_collect_kernel, dim3(chunks), dim3(256), 0, st, (const int*)labels_out, HW, H, W, (const int*)chunk_roots, cap, rank, table_out, limit);
  GI_LAUNCH_CHECK();
  const unsigned spans = (unsigned)(W + 64 * SG - 1) / (64 * SG);
  const uint64_t waves = (uint64_t)((H + SR - 1) / SR) * spans;   // <= (H / SR + 1) * (W / (64 SG) + 1) < 2^31
  hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, (const int*)labels_out, H, W, spans, (const int*)rank, (const int*)limit, table_out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // extern "C"
