// Batch assembly from a device-resident image store: out[i][y][x] = f(store[rows[i]][y][flip_i ? w-1-x : x]), the
// store the resized 8-bit images of a dataset (lib/data/cache.py), f the ToTensor quotient of resize_v_kernel, the label widening
// or the identity. The horizontal flip of image i is a pure integer function of (flip_seed, flip_keys[i]) on the dropout hash
// (bn_acc.h), independent of the mask draws: stream = mix((seed ^ 0x666C6970) + G * (key + 1)), flip = mix(stream + G) >> 63.
//
// Memory-bound: every lane owns four consecutive output pixels (a quad). One workgroup takes 256 quads of ONE image per step, so the
// row index, the flip bit and the image bases are uniform in the workgroup. w % 4 == 0 with aligned pointers: one 4-byte load
// (the mirrored quad, byte-reversed, when flipped) and 16-byte stores (two per lane for int64, one 4-byte store for uint8); every
// other width or alignment takes byte loads and element stores. All offsets are 64-bit: rows[i] * h * w passes 2^31 at 32768
// images of 256 x 256.
#include "bn_acc.h"
#include "common.h"

namespace {

constexpr int GRID_CAP = 2048;   // workgroups per launch: 256 CUs x 8 resident blocks of 256 lanes; the chunks beyond it are grid-strided

struct GatherP {
  const uint8_t* store;
  const int64_t* rows;
  const int64_t* keys;   // nullptr: no flips
  void* out;
  uint64_t seed;
  int64_t n_store, chunks;   // chunks = n * cpi
  int h, w;
  int qpr, pq, cpi;          // quads per row, quads per image, 256-quad chunks per image
};

template <int KIND> struct OutOf;
template <> struct OutOf<0> { typedef float type; };
template <> struct OutOf<1> { typedef int64_t type; };
template <> struct OutOf<2> { typedef uint8_t type; };

template <int KIND>
__device__ __forceinline__ typename OutOf<KIND>::type value_of(uint32_t v) {
  if constexpr (KIND == 0) return (float)(int)v / 255.0f;   // resize_v_kernel's expression
  else return (typename OutOf<KIND>::type)v;
}

template <int KIND, bool VEC>
__global__ void __launch_bounds__(256) batch_gather_kernel(GatherP p) {
  typedef typename OutOf<KIND>::type OUT;
  const int64_t hw = (int64_t)p.h * p.w;
  for (int64_t c = blockIdx.x; c < p.chunks; c += gridDim.x) {
    const int64_t img = c / p.cpi;
    const int j = (int)(c - img * p.cpi) * 256 + (int)threadIdx.x;   // quad of the image
    if (j >= p.pq) continue;
    const int64_t r = p.rows[img];
    const bool ok = r >= 0 && r < p.n_store;   // defence only: a row outside the store reads nothing and yields zeros
    bool flip = false;
    if (p.keys) {
      const uint64_t stream = gi_mix64((p.seed ^ 0x666C6970ull) + GI_GOLDEN64 * ((uint64_t)p.keys[img] + 1ull));
      flip = (gi_mix64(stream + GI_GOLDEN64) >> 63) != 0;
    }
    const int y = j / p.qpr, k = j - y * p.qpr;
    const uint8_t* src = p.store + (ok ? r * hw : 0) + (int64_t)y * p.w;   // the source row (dereferenced only when ok)
    OUT* dst = (OUT*)p.out + img * hw + (int64_t)y * p.w + 4 * k;
    if constexpr (VEC) {
      uint32_t word = 0;
      if (ok) {
        word = *(const uint32_t*)(src + 4 * (flip ? p.qpr - 1 - k : k));
        if (flip) word = __builtin_bswap32(word);
      }
      const uint32_t v0 = word & 255u, v1 = (word >> 8) & 255u, v2 = (word >> 16) & 255u, v3 = word >> 24;
      if constexpr (KIND == 0) {
        f4_t o;
        o.x = value_of<0>(v0); o.y = value_of<0>(v1); o.z = value_of<0>(v2); o.w = value_of<0>(v3);
        *(f4_t*)dst = o;
      } else if constexpr (KIND == 1) {   // little-endian int64 pairs
        u4_t a, b;
        a.x = v0; a.y = 0; a.z = v1; a.w = 0;
        b.x = v2; b.y = 0; b.z = v3; b.w = 0;
        ((u4_t*)dst)[0] = a;
        ((u4_t*)dst)[1] = b;
      } else {
        *(uint32_t*)dst = word;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = 4 * k + e;
        if (x < p.w) dst[e] = value_of<KIND>(ok ? (uint32_t)src[flip ? p.w - 1 - x : x] : 0u);
      }
    }
  }
}

template <int KIND>
void launch(const GatherP& p, bool vec, unsigned grid, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((batch_gather_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((batch_gather_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, p);
}

}  // namespace

extern "C" int gi_batch_gather(gi_ctx* ctx, const uint8_t* store, int64_t n_store, int h, int w, const int64_t* rows_dev, int n,
                               const int64_t* flip_keys_dev, uint64_t flip_seed, int out_kind, void* out) {
  GI_REQUIRE(ctx && store && rows_dev && out, "batch_gather: null argument");
  GI_REQUIRE(n > 0 && n_store > 0, "batch_gather: n = %d rows of a store of %lld images", n, (long long)n_store);
  GI_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= 0x7fffffff, "batch_gather: %d x %d images", h, w);
  GI_REQUIRE(out_kind >= 0 && out_kind <= 2, "batch_gather: out_kind %d (0 fp32, 1 int64, 2 uint8)", out_kind);
  const int esize = out_kind == 0 ? 4 : (out_kind == 1 ? 8 : 1);
  GI_REQUIRE(((uintptr_t)out & (uintptr_t)(esize - 1)) == 0, "batch_gather: out is not aligned to its %d-byte elements", esize);
  GatherP p;
  p.store = store; p.rows = rows_dev; p.keys = flip_keys_dev; p.out = out; p.seed = flip_seed; p.n_store = n_store; p.h = h; p.w = w;
  p.qpr = (w + 3) / 4;
  const int64_t pq = (int64_t)h * p.qpr;
  p.pq = (int)pq;
  p.cpi = (int)((pq + 255) / 256);
  p.chunks = (int64_t)n * p.cpi;
  // w % 4 == 0: every image base and every row of the store is a multiple of 4 bytes from `store`, every output quad a multiple of
  // 16 (4 for uint8) bytes from `out`, so the two pointers decide the path for the whole launch
  const bool vec = (w & 3) == 0 && ((uintptr_t)store & 3) == 0 && ((uintptr_t)out & (uintptr_t)(out_kind == 2 ? 3 : 15)) == 0;
  const unsigned grid = (unsigned)(p.chunks < GRID_CAP ? p.chunks : GRID_CAP);
  if (out_kind == 0) launch<0>(p, vec, grid, ctx->stream);
  else if (out_kind == 1) launch<1>(p, vec, grid, ctx->stream);
  else launch<2>(p, vec, grid, ctx->stream);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
