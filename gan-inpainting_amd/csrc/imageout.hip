// Image output path (NOT in the reference): what turns the engine's fp32 tensors back into 8-bit pictures, and what
// puts a repaired window back into a photograph of any size. Everything here is exact: integer arithmetic, or one fp32 multiply
// followed by rintf. tests/imageout_ref.py is the numpy restatement, bit-exact with every entry.
//
//   gi_image_quantize   q(x) = rintf(clamp(x, 0, 1) * 255), NaN -> 0 (round to nearest even, every byte v round-trips through v / 255f)
//   gi_panel_assemble   up to 8 columns of (n,1,H,W) fp32 batches as one uint8 canvas with white gutters, every byte written once
//   gi_mask_bbox        inclusive bounding box of the nonzero bytes of each mask (integer min / max: no order dependence)
//   gi_window_crop      a window of a uint8 image as a dense array, optionally binarised to {0, 255}
//   gi_feather_paste    the window's bytes of dst = blend of patch and orig, the weight a box count of the hole (LDS running sums)
#include <limits.h>

#include "common.h"

namespace {

__device__ __forceinline__ uint32_t quant8(float x) {
  x = x > 0.f ? x : 0.f;   // NaN and -0 take the zero
  x = x < 1.f ? x : 1.f;
  return (uint32_t)rintf(x * 255.0f);
}
__device__ __forceinline__ uint32_t quant8x4(float a, float b, float c, float d) {
  return quant8(a) | (quant8(b) << 8) | (quant8(c) << 16) | (quant8(d) << 24);
}

// dst[head + 16 k ..] is 16-byte aligned: one 16-byte store per 16 pixels; SRC16: the floats under it are 16-byte aligned too (four
// 16-byte loads, else sixteen 4-byte ones). The `head` pixels in front of the first boundary and the last (count - head) % 16 go
// one by one (workgroup 0).
template <bool SRC16>
__global__ void __launch_bounds__(256) quantize_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t count, int head) {
  const int64_t chunks = (count - head) >> 4;
  const float* s = src + head;
  uint8_t* d = dst + head;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    u4_t o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* p = s + c * 16 + 4 * q;
      if constexpr (SRC16) {
        const f4_t v = *(const f4_t*)p;
        o[q] = quant8x4(v.x, v.y, v.z, v.w);
      } else {
        o[q] = quant8x4(p[0], p[1], p[2], p[3]);
      }
    }
    *(u4_t*)(d + c * 16) = o;
  }
  if (blockIdx.x == 0) {
    const int64_t body_end = head + chunks * 16;
    const int ragged = head + (int)(count - body_end);   // < 32
    if ((int)threadIdx.x < ragged) {
      const int64_t i = (int)threadIdx.x < head ? (int64_t)threadIdx.x : body_end + ((int)threadIdx.x - head);
      dst[i] = (uint8_t)quant8(src[i]);
    }
  }
}

constexpr int PANEL_MAX_COLS = 8;
struct PanelP {
  const float* cols[PANEL_MAX_COLS];
  uint8_t* canvas;
  int ncol, n, H, W, g;
  int Wc;   // canvas width ncol * (W + g) + g
};

// One workgroup per canvas row; a thread owns the 4-byte aligned words of the row (the row starts `shift` bytes past a word boundary,
// word k covers x = 4 k - shift .. + 3), so full words are one store and only the row's ends go byte by byte.
__global__ void __launch_bounds__(256) panel_kernel(PanelP p) {
  const int r = blockIdx.x;
  const int pitch_y = p.H + p.g, pitch_x = p.W + p.g;
  const int ti = r / pitch_y, ty = r - ti * pitch_y - p.g;   // ty < 0: a gutter row; ti == n: the last gutter
  const bool gutter_row = ti >= p.n || ty < 0;
  uint8_t* row = p.canvas + (int64_t)r * p.Wc;
  const int shift = (int)((uintptr_t)row & 3);
  const int words = (p.Wc + shift + 3) >> 2;
  const int64_t src_row = ((int64_t)ti * p.H + ty) * p.W;
  for (int k = threadIdx.x; k < words; k += 256) {
    const int x0 = 4 * k - shift;
    uint32_t b[4];
    int tj = x0 >= 0 ? x0 / pitch_x : 0, tx = (x0 >= 0 ? x0 - tj * pitch_x : x0) - p.g;   // column tile / x inside it of byte x0
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = x0 + e;
      uint32_t v = 255u;
      if (!gutter_row && x >= 0 && x < p.Wc && tx >= 0 && tj < p.ncol) {
        const float* col = p.cols[0];
#pragma unroll
        for (int j = 1; j < PANEL_MAX_COLS; ++j) col = tj == j ? p.cols[j] : col;   // (selects: a per-lane index would make the argument block a private array)
        v = quant8(col[src_row + tx]);
      }
      b[e] = v;
      if (++tx == p.W) { tx = -p.g; ++tj; }
    }
    if (x0 >= 0 && x0 + 3 < p.Wc) {
      *(uint32_t*)(row + x0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + e >= 0 && x0 + e < p.Wc) row[x0 + e] = (uint8_t)b[e];
    }
  }
}

__global__ void bbox_init_kernel(int* bbox, int n, int H, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    bbox[4 * i] = H; bbox[4 * i + 1] = W; bbox[4 * i + 2] = -1; bbox[4 * i + 3] = -1;
  }
}

// Workgroups (blockIdx.x) share the pixels of image blockIdx.y in 16-byte aligned chunks (an image starts anywhere: chunk 0 and the
// last one may be partial and are read byte by byte). Rows come from the smallest and largest nonzero pixel index alone; columns need
// every nonzero pixel's x, kept by increments from one division per chunk. Wave min / max, one LDS atomic per wave, one global
// atomic set per workgroup that saw a hole.
__global__ void __launch_bounds__(256) bbox_kernel(const uint8_t* __restrict__ mask, int HW, int W, int* __restrict__ bbox) {
  __shared__ int s_red[4];
  const int img = blockIdx.y;
  const uint8_t* m = mask + (int64_t)img * HW;
  const int lead = (int)((uintptr_t)m & 15);         // chunk c covers pixels 16 c - lead .. + 15
  const int chunks = (HW + lead + 15) >> 4;
  int pmin = INT_MAX, pmax = -1, xmin = INT_MAX, xmax = -1;
  if (threadIdx.x == 0) { s_red[0] = INT_MAX; s_red[1] = INT_MAX; s_red[2] = -1; s_red[3] = -1; }
  __syncthreads();
  for (int c = blockIdx.x * 256 + threadIdx.x; c < chunks; c += gridDim.x * 256) {
    const int p0 = 16 * c - lead;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (p0 >= 0 && p0 + 16 <= HW) {
      const u4_t v = *(const u4_t*)(m + p0);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (p0 + e >= 0 && p0 + e < HW) w[e >> 2] |= (uint32_t)m[p0 + e] << (8 * (e & 3));
    }
    if ((w[0] | w[1] | w[2] | w[3]) == 0u) continue;
    const int pf = p0 < 0 ? 0 : p0;
    int x = pf % W;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (p0 + e < pf) continue;   // (bytes in front of the image: zero above, no pixel)
      if ((w[e >> 2] >> (8 * (e & 3))) & 255u) {
        const int pix = p0 + e;
        pmin = min(pmin, pix); pmax = max(pmax, pix);
        xmin = min(xmin, x); xmax = max(xmax, x);
      }
      if (++x == W) x = 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pmin = min(pmin, __shfl_xor(pmin, o)); xmin = min(xmin, __shfl_xor(xmin, o));
    pmax = max(pmax, __shfl_xor(pmax, o)); xmax = max(xmax, __shfl_xor(xmax, o));
  }
  if ((threadIdx.x & 63) == 0 && pmax >= 0) {
    atomicMin(&s_red[0], pmin); atomicMin(&s_red[1], xmin);
    atomicMax(&s_red[2], pmax); atomicMax(&s_red[3], xmax);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_red[2] >= 0) {
    atomicMin(bbox + 4 * img, s_red[0] / W); atomicMin(bbox + 4 * img + 1, s_red[1]);
    atomicMax(bbox + 4 * img + 2, s_red[2] / W); atomicMax(bbox + 4 * img + 3, s_red[3]);
  }
}

__global__ void __launch_bounds__(256) crop_kernel(const uint8_t* __restrict__ src, int W, int wy, int wx, int wh, int ww, int binarize,
                                                   uint8_t* __restrict__ dst) {
  const unsigned total = (unsigned)wh * ww;   // < 2^31: the unsigned index cannot wrap
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int y = (int)(i / (unsigned)ww), x = (int)i - y * ww;
    const uint8_t v = src[(int64_t)(wy + y) * W + wx + x];
    dst[i] = binarize ? (v ? 255 : 0) : v;
  }
}

// ---- feather paste ----------------------------------------------------------------------------------------------------------------
// One workgroup per FT x FT tile of the window. LDS: the hole bits of the tile and its r halo as bytes (zero outside the window),
// then per halo row the horizontal (2r+1)-count of every tile column (<= 127: a byte), both by running sums; then every thread takes
// a column of FT / 4 rows, keeps the vertical running sum of those counts in a register (<= 16129) and blends and stores as it goes:
// no count ever reaches memory. Lanes of a wave are consecutive x: the byte loads and stores of a row coalesce.
constexpr int FT = 64;
constexpr int FEATHER_MAX_R = 63;
struct FeatherP {
  const uint8_t* orig; const uint8_t* mask; const uint8_t* patch;
  uint8_t* dst;
  int W, wy, wx, wh, ww, r;
};
inline int feather_lds_bytes(int r) {
  const int e = FT + 2 * r;
  return e * gi_align_up(e, 4) + e * FT;
}

__global__ void __launch_bounds__(256) feather_kernel(FeatherP p) {
  extern __shared__ uint8_t s_mem[];
  const int r = p.r, tid = threadIdx.x;
  const int u0 = blockIdx.y * FT, v0 = blockIdx.x * FT;             // the tile's origin inside the window
  const int th = min(FT, p.wh - u0), tw = min(FT, p.ww - v0);
  const int eh = th + 2 * r, ew = tw + 2 * r;                       // tile + halo
  const int pitch = (int)((FT + 2 * r + 3) & ~3);
  uint8_t* s_hole = s_mem;                          // [eh][pitch]
  uint8_t* s_hcnt = s_mem + (FT + 2 * r) * pitch;   // [eh][FT]

  for (int i = tid; i < eh * ew; i += 256) {
    const int ly = i / ew, lx = i - ly * ew;
    const int u = u0 + ly - r, v = v0 + lx - r;
    uint8_t h = 0;
    if (u >= 0 && u < p.wh && v >= 0 && v < p.ww) h = p.mask[(int64_t)(p.wy + u) * p.W + p.wx + v] != 0;
    s_hole[ly * pitch + lx] = h;
  }
  __syncthreads();
  // horizontal counts: a task is 16 consecutive tile columns of one halo row
  const int segs = (tw + 15) >> 4;
  for (int t = tid; t < eh * segs; t += 256) {
    const int ly = t / segs, x0 = (t - ly * segs) * 16, x1 = min(x0 + 16, tw);
    const uint8_t* row = s_hole + ly * pitch;
    int s = 0;
    for (int k = 0; k <= 2 * r; ++k) s += row[x0 + k];
    for (int x = x0; x < x1; ++x) {
      s_hcnt[ly * FT + x] = (uint8_t)s;
      s += (int)row[x + 2 * r + 1 < ew ? x + 2 * r + 1 : ew - 1] - (int)row[x];   // (the clamped read belongs to a sum nobody uses)
    }
  }
  __syncthreads();
  const int tx = tid & (FT - 1), yseg = tid >> 6;   // 4 row segments of FT / 4 rows
  if (tx < tw) {
    const int ya = yseg * (FT / 4), yb = min(ya + FT / 4, th);
    const uint32_t A = (uint32_t)((2 * r + 1) * (2 * r + 1));
    int a = 0;
    if (ya < yb)
      for (int k = 0; k <= 2 * r; ++k) a += s_hcnt[(ya + k) * FT + tx];
    for (int y = ya; y < yb; ++y) {
      const bool hole = s_hole[(y + r) * pitch + tx + r] != 0;
      const uint32_t alpha = hole ? A : min(A, 2u * (uint32_t)a);
      const int64_t g = (int64_t)(p.wy + u0 + y) * p.W + p.wx + v0 + tx;
      const uint32_t pv = p.patch[(int64_t)(u0 + y) * p.ww + v0 + tx], ov = p.orig[g];
      p.dst[g] = (uint8_t)((alpha * pv + (A - alpha) * ov + A / 2) / A);
      if (y + 1 < yb) a += (int)s_hcnt[(y + 2 * r + 1) * FT + tx] - (int)s_hcnt[y * FT + tx];
    }
  }
}

}  // namespace

extern "C" {

int gi_image_quantize(gi_ctx* ctx, const float* src, int64_t count, uint8_t* dst) {
  GI_REQUIRE(ctx && src && dst, "image_quantize: null argument");
  GI_REQUIRE(count > 0, "image_quantize: count = %lld", (long long)count);
  GI_REQUIRE(((uintptr_t)src & 3) == 0, "image_quantize: src is not 4-byte aligned");
  int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15);
  if (head > count) head = count;
  const int64_t chunks = (count - head) >> 4;
  const int grid = grid_for(chunks, 256, 4096);
  if ((((uintptr_t)(src + head)) & 15) == 0) hipLaunchKernelGGL(quantize_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, src, dst, count, (int)head);
  else hipLaunchKernelGGL(quantize_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, src, dst, count, (int)head);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_panel_assemble(gi_ctx* ctx, const float* const* cols_host, int ncol, int n, int H, int W, int gutter, uint8_t* canvas) {
  GI_REQUIRE(ctx && cols_host && canvas, "panel_assemble: null argument");
  GI_REQUIRE(ncol >= 1 && ncol <= PANEL_MAX_COLS, "panel_assemble: %d columns (1 .. %d)", ncol, PANEL_MAX_COLS);
  GI_REQUIRE(n > 0 && H > 0 && W > 0 && gutter >= 0, "panel_assemble: n = %d, %d x %d, gutter %d", n, H, W, gutter);
  const int64_t Hc = (int64_t)n * (H + (int64_t)gutter) + gutter, Wc = (int64_t)ncol * (W + (int64_t)gutter) + gutter;
  GI_REQUIRE(Hc <= INT_MAX && Wc <= INT_MAX && (int64_t)n * H * W <= INT_MAX, "panel_assemble: a %lld x %lld canvas is too large", (long long)Hc, (long long)Wc);
  PanelP p;
  for (int j = 0; j < PANEL_MAX_COLS; ++j) {
    p.cols[j] = cols_host[j < ncol ? j : 0];
    GI_REQUIRE(p.cols[j] && ((uintptr_t)p.cols[j] & 3) == 0, "panel_assemble: column %d is null or not 4-byte aligned", j);
  }
  p.canvas = canvas; p.ncol = ncol; p.n = n; p.H = H; p.W = W; p.g = gutter; p.Wc = (int)Wc;
  hipLaunchKernelGGL(panel_kernel, dim3((unsigned)Hc), dim3(256), 0, ctx->stream, p);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_mask_bbox(gi_ctx* ctx, const uint8_t* mask, int n, int H, int W, int* bbox_out) {
  GI_REQUIRE(ctx && mask && bbox_out, "mask_bbox: null argument");
  GI_REQUIRE(n > 0 && n <= 65535 && H > 0 && W > 0, "mask_bbox: n = %d (1 .. 65535), %d x %d", n, H, W);
  GI_REQUIRE((int64_t)H * W < 0x7fffffffll - 32, "mask_bbox: %d x %d pixels do not fit 31 bits", H, W);
  const int HW = H * W;
  hipLaunchKernelGGL(bbox_init_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, bbox_out, n, H, W);
  GI_LAUNCH_CHECK();
  hipLaunchKernelGGL(bbox_kernel, dim3(grid_for(((int64_t)HW + 15) / 16 + 1, 256 * 4, 1024), n), dim3(256), 0, ctx->stream, mask, HW, W, bbox_out);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

static int window_ok(int H, int W, int wy, int wx, int wh, int ww) {
  return H > 0 && W > 0 && (int64_t)H * W <= INT_MAX && wy >= 0 && wx >= 0 && wh > 0 && ww > 0 && wh <= H - wy && ww <= W - wx;
}

int gi_window_crop(gi_ctx* ctx, const uint8_t* src, int H, int W, int wy, int wx, int wh, int ww, int binarize, uint8_t* dst) {
  GI_REQUIRE(ctx && src && dst, "window_crop: null argument");
  GI_REQUIRE(window_ok(H, W, wy, wx, wh, ww), "window_crop: window (%d, %d) + %d x %d leaves the %d x %d image", wy, wx, wh, ww, H, W);
  hipLaunchKernelGGL(crop_kernel, dim3(grid_for((int64_t)wh * ww, 256 * 4, 4096)), dim3(256), 0, ctx->stream, src, W, wy, wx, wh, ww, binarize, dst);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_feather_paste(gi_ctx* ctx, const uint8_t* orig, const uint8_t* mask, int H, int W, int wy, int wx, int wh, int ww,
                     const uint8_t* patch, int r, uint8_t* dst) {
  GI_REQUIRE(ctx && orig && mask && patch && dst, "feather_paste: null argument");
  GI_REQUIRE(r >= 0 && r <= FEATHER_MAX_R, "feather_paste: r = %d (0 .. %d)", r, FEATHER_MAX_R);
  GI_REQUIRE(window_ok(H, W, wy, wx, wh, ww), "feather_paste: window (%d, %d) + %d x %d leaves the %d x %d image", wy, wx, wh, ww, H, W);
  const int gx = (ww + FT - 1) / FT, gy = (wh + FT - 1) / FT;
  GI_REQUIRE(gy <= 65535, "feather_paste: a window of %d rows exceeds the grid", wh);
  FeatherP p;
  p.orig = orig; p.mask = mask; p.patch = patch; p.dst = dst;
  p.W = W; p.wy = wy; p.wx = wx; p.wh = wh; p.ww = ww; p.r = r;
  hipLaunchKernelGGL(feather_kernel, dim3(gx, gy), dim3(256), feather_lds_bytes(r), ctx->stream, p);   // <= 48.6 KB: below the default limit
  GI_LAUNCH_CHECK();
  return GI_OK;
}

}  // extern "C"
