// Device mask generator: the hole masks of an inpainting batch, rectangles (the benchmark's distribution)
// or free-form strokes (thick polylines: Liu et al. 2018; Yu et al. 2019, Algorithm 1), as a pure integer function of
// (kind, seed, key, H, W). Counter-based draws on the finaliser dropout_keep uses (bn_acc.h): draw k of a mask never depends on
// another draw, on the batch or on the image's place in it, and the numpy restatement (tests/maskgen_ref.py) is bit-exact.
//
// One workgroup per (band of BAND rows, image): 141 lanes take the image's draws (one splitmix64 each), one lane per stroke walks
// its polyline into LDS, wave 0 keeps the segments whose bounding box grown by the radius meets the band, then every thread owns
// four consecutive pixels of a row and loops over that sub-list (the same LDS address in every lane: broadcast reads).
#include "bn_acc.h"
#include "common.h"

namespace {

constexpr int BAND = 8;          // rows per workgroup
constexpr int MAX_STROKES = 5;   // ns = uni(0, 2, 5)
constexpr int MAX_VERTS = 12;    // nv = uni(b, 4, 12)
constexpr int SEGS_PER_STROKE = MAX_VERTS - 1;
constexpr int MAX_SEGS = MAX_STROKES * SEGS_PER_STROKE;   // 55 (one wave compacts them)
constexpr int DRAWS_PER_STROKE = 6 + 2 * SEGS_PER_STROKE;   // b .. b + 5 + 2 * 11
static_assert(MAX_SEGS <= 64 && DRAWS_PER_STROKE <= 32, "the prologue's lane layout");

// draw(k) of a stream, on the finaliser dropout_keep uses (bn_acc.h)
__device__ __forceinline__ uint32_t draw32(uint64_t stream, int k) { return (uint32_t)(gi_mix64(stream + GI_GOLDEN64 * (uint64_t)(k + 1)) >> 32); }
// lo + ((d * (hi - lo + 1)) >> 32), bounds inclusive
__device__ __forceinline__ int uni_of(uint32_t d, int lo, int hi) { return lo + (int)__umulhi(d, (uint32_t)(hi - lo + 1)); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a capsule: start A, d = B - A, L2 = d.d, r2 = r * r, r2L2 = r2 * L2 (low / high word)
struct Seg { int ax, ay, dx, dy, L2, r2; uint32_t r2L2_lo, r2L2_hi; };
static_assert(sizeof(Seg) == 32, "two 16-byte LDS reads per segment");

struct MaskP {
  const int64_t* keys;
  float* out;
  int* coverage;
  uint64_t seed;
  int H, W, bands;
};

// Is pixel q = P - A (t = q.d, cr = q x d) inside the capsule? Exact:  t <= 0: |q|^2 <= r^2 ; t >= L2: |P - B|^2 = |q|^2 - 2 t + L2 <= r^2 ;
// else (q x d)^2 <= r^2 L2 (which also serves d = 0: t = 0 there).
// WIDE = false squares the cross product in 32 bits (unsigned). That is exact when |q x d| <= 65535; |q x d| <= (|qx| + |qy|) * max|d|
// <= (W - 1 + H - 1) * L, so the host takes this path only when (W + H - 2) * L <= 65535 (maskgen_narrow_ok). r^2 L2 <= rmax^2 * 2 L^2
// is below 2^32 in that range too (S <= 512: 32^2 * 2 * 64^2 = 2^23). All other products fit 32 bits at every size up to 4096:
// |t| <= 2 * 4095 * 512 < 2^23, |q|^2 <= 2 * 4095^2 < 2^25.
template <bool WIDE>
__device__ __forceinline__ bool in_capsule(const Seg& s, int qx, int qy, int t, int cr) {
  const int qq = qx * qx + qy * qy;
  const bool ends = (t <= 0) ? (qq <= s.r2) : (qq - 2 * t + s.L2 <= s.r2);
  bool side;
  if constexpr (WIDE) {
    const uint64_t c = (uint64_t)(cr < 0 ? -cr : cr);
    side = c * c <= (((uint64_t)s.r2L2_hi << 32) | s.r2L2_lo);
  } else {
    const uint32_t c = (uint32_t)(cr < 0 ? -cr : cr);
    side = c * c <= s.r2L2_lo;
  }
  return (t > 0 && t < s.L2) ? side : ends;
}

template <int KIND, bool WIDE>
__global__ void __launch_bounds__(256) maskgen_kernel(MaskP p) {
  __shared__ uint32_t s_draw[1 + MAX_STROKES * DRAWS_PER_STROKE];   // [0]: draw(0); then draw(64 * (s + 1) + i)
  __shared__ Seg s_seg[MAX_SEGS];    // stroke s at [s * SEGS_PER_STROKE ..)
  __shared__ Seg s_sub[MAX_SEGS];    // the band's segments
  __shared__ int s_cnt[MAX_STROKES];
  __shared__ int s_nsub, s_cover;
  __shared__ int s_rect[4];
  const int tid = threadIdx.x;
  const int img = blockIdx.x / p.bands, band = blockIdx.x - img * p.bands;
  const int H = p.H, W = p.W;
  const int y0 = band * BAND, y1 = min(y0 + BAND, H) - 1;   // the band's rows, inclusive
  const uint64_t stream = gi_mix64(p.seed + GI_GOLDEN64 * ((uint64_t)p.keys[img] + 1ull));
  if (tid == 0) s_cover = 0;

  if constexpr (KIND == 0) {
    if (tid == 0) {
      const int h = uni_of(draw32(stream, 0), H / 8, H / 2);
      const int w = uni_of(draw32(stream, 1), W / 8, W / 2);
      s_rect[0] = uni_of(draw32(stream, 2), 0, H - h);
      s_rect[1] = uni_of(draw32(stream, 3), 0, W - w);
      s_rect[2] = h;
      s_rect[3] = w;
    }
    __syncthreads();
  } else {
    // every draw the image can use, one lane each
    if (tid < MAX_STROKES * 32) {
      const int s = tid >> 5, i = tid & 31;
      if (i < DRAWS_PER_STROKE) s_draw[1 + s * DRAWS_PER_STROKE + i] = draw32(stream, 64 * (s + 1) + i);
    } else if (tid == MAX_STROKES * 32) {
      s_draw[0] = draw32(stream, 0);
    }
    __syncthreads();
    // one lane per stroke: the polyline
    if (tid < MAX_STROKES) {
      const int S = min(H, W), L = max(2, S / 8), rmin = max(1, S / 48), rmax = max(rmin, S / 16);
      const int ns = uni_of(s_draw[0], 2, 5);
      const uint32_t* d = s_draw + 1 + tid * DRAWS_PER_STROKE;
      int cnt = 0;
      if (tid < ns) {
        const int nv = uni_of(d[0], 4, MAX_VERTS), r = uni_of(d[1], rmin, rmax);
        int x = uni_of(d[2], 0, W - 1), y = uni_of(d[3], 0, H - 1);
        int vx = uni_of(d[4], -L, L), vy = uni_of(d[5], -L, L);
        for (int j = 1; j < nv; ++j) {
          int nx = x + vx, ny = y + vy;
          if (nx < 0 || nx > W - 1) { nx = clampi(nx, 0, W - 1); vx = -vx; }
          if (ny < 0 || ny > H - 1) { ny = clampi(ny, 0, H - 1); vy = -vy; }
          Seg g;
          g.ax = x; g.ay = y; g.dx = nx - x; g.dy = ny - y;
          g.L2 = g.dx * g.dx + g.dy * g.dy;
          g.r2 = r * r;
          const uint64_t rl = (uint64_t)g.r2 * (uint64_t)g.L2;
          g.r2L2_lo = (uint32_t)rl; g.r2L2_hi = (uint32_t)(rl >> 32);
          s_seg[tid * SEGS_PER_STROKE + cnt++] = g;
          x = nx; y = ny;
          vx = clampi(vx + uni_of(d[4 + 2 * j], -(L / 2), L / 2), -L, L);
          vy = clampi(vy + uni_of(d[5 + 2 * j], -(L / 2), L / 2), -L, L);
        }
      }
      s_cnt[tid] = cnt;
    }
    __syncthreads();
    // wave 0: the segments whose bounding box, grown by r, meets rows [y0, y1] (r <= sqrt(r2): compare squared distances of rows)
    if (tid < 64) {
      const int s = tid / SEGS_PER_STROKE, j = tid - s * SEGS_PER_STROKE;
      bool keep = false;
      Seg g;
      if (tid < MAX_SEGS && j < s_cnt[s]) {
        g = s_seg[tid];
        const int lo = min(g.ay, g.ay + g.dy), hi = max(g.ay, g.ay + g.dy);
        const int gap = lo > y1 ? lo - y1 : (hi < y0 ? y0 - hi : 0);   // rows between the band and the segment's row span
        keep = gap * gap <= g.r2;
      }
      const uint64_t m = __ballot(keep);
      if (keep) s_sub[__popcll(m & ((1ull << tid) - 1ull))] = g;
      if (tid == 0) s_nsub = __popcll(m);
    }
    __syncthreads();
  }

  // pixels: quads aligned to 16 bytes in memory. Row y starts `shift` floats past a 16-byte boundary; quad k covers x = 4k - shift .. + 3
  const int64_t img_off = (int64_t)img * H * W;
  int ones = 0;
  const int nsub = KIND == 0 ? 0 : s_nsub;
  const int ry0 = KIND == 0 ? s_rect[0] : 0, rx0 = KIND == 0 ? s_rect[1] : 0, rh = KIND == 0 ? s_rect[2] : 0, rw = KIND == 0 ? s_rect[3] : 0;
  // quads per row = ceil((W + largest shift) / 4). W % 4 == 0: every row of every image has mask_out's own shift (0 for a 16-byte
  // aligned tensor: exactly W / 4 quads, no idle one - 512 quads per band at W = 256, two per thread); else rows differ, up to 3
  const int max_shift = (W & 3) == 0 ? (int)(((uintptr_t)p.out >> 2) & 3) : 3;
  const int qpr = (W + max_shift + 3) / 4;
  const int rows = y1 - y0 + 1;
  for (int q = tid; q < rows * qpr; q += 256) {
    const int ry = q / qpr, k = q - ry * qpr;
    const int y = y0 + ry;
    float* row = p.out + img_off + (int64_t)y * W;
    const int shift = (int)(((uintptr_t)row >> 2) & 3);
    const int x0 = 4 * k - shift;
    if (x0 >= W) continue;
    bool hit[4] = {false, false, false, false};
    if constexpr (KIND == 0) {
      const bool yin = y >= ry0 && y < ry0 + rh;
#pragma unroll
      for (int e = 0; e < 4; ++e) hit[e] = yin && x0 + e >= rx0 && x0 + e < rx0 + rw;
    } else {
      for (int i = 0; i < nsub; ++i) {
        const Seg g = s_sub[i];
        const int qx = x0 - g.ax, qy = y - g.ay;
        const int t = qx * g.dx + qy * g.dy, cr = qx * g.dy - qy * g.dx;
#pragma unroll
        for (int e = 0; e < 4; ++e) hit[e] |= in_capsule<WIDE>(g, qx + e, qy, t + e * g.dx, cr + e * g.dy);
      }
    }
    if (x0 >= 0 && x0 + 3 < W) {
      f4_t v;
      v.x = hit[0] ? 1.f : 0.f; v.y = hit[1] ? 1.f : 0.f; v.z = hit[2] ? 1.f : 0.f; v.w = hit[3] ? 1.f : 0.f;
      *(f4_t*)(row + x0) = v;
      ones += (int)hit[0] + (int)hit[1] + (int)hit[2] + (int)hit[3];
    } else {   // ragged ends of the row
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (x0 + e >= 0 && x0 + e < W) {
          row[x0 + e] = hit[e] ? 1.f : 0.f;
          ones += (int)hit[e];
        }
      }
    }
  }
  if (p.coverage) {   // integer adds only: the count does not depend on their order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o);
    if ((tid & 63) == 0 && ones) atomicAdd(&s_cover, ones);
    __syncthreads();
    if (tid == 0 && s_cover) atomicAdd(p.coverage + img, s_cover);
  }
}

// the 32-bit cross-product path is exact (in_capsule)
bool maskgen_narrow_ok(int H, int W) {
  const int S = H < W ? H : W, L = S / 8 > 2 ? S / 8 : 2;
  return (int64_t)(W + H - 2) * L <= 65535;
}

}  // namespace

extern "C" int gi_mask_generate(gi_ctx* ctx, int kind, uint64_t seed, const int64_t* keys_dev, int n, int H, int W, float* mask_out,
                                int* coverage_out) {
  GI_REQUIRE(ctx && keys_dev && mask_out, "mask_generate: null argument");
  GI_REQUIRE(kind == 0 || kind == 1, "mask_generate: kind %d (0 rect, 1 freeform)", kind);
  GI_REQUIRE(n > 0, "mask_generate: n = %d", n);
  GI_REQUIRE(H >= 16 && H <= 4096 && W >= 16 && W <= 4096, "mask_generate: %d x %d outside 16 .. 4096", H, W);
  GI_REQUIRE(((uintptr_t)mask_out & 3) == 0, "mask_generate: mask_out is not 4-byte aligned");
  MaskP p;
  p.keys = keys_dev; p.out = mask_out; p.coverage = coverage_out; p.seed = seed; p.H = H; p.W = W;
  p.bands = (H + BAND - 1) / BAND;
  const int64_t blocks = (int64_t)n * p.bands;
  GI_REQUIRE(blocks <= 0x7fffffff, "mask_generate: n = %d images of %d rows exceed the grid", n, H);
  if (coverage_out) GI_HIP(hipMemsetAsync(coverage_out, 0, (size_t)n * sizeof(int), ctx->stream));   // the kernel adds into it
  const dim3 grid((unsigned)blocks), block(256);
  if (kind == 0) hipLaunchKernelGGL((maskgen_kernel<0, false>), grid, block, 0, ctx->stream, p);
  else if (maskgen_narrow_ok(H, W)) hipLaunchKernelGGL((maskgen_kernel<1, false>), grid, block, 0, ctx->stream, p);
  else hipLaunchKernelGGL((maskgen_kernel<1, true>), grid, block, 0, ctx->stream, p);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
