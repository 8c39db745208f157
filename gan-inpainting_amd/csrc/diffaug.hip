// Differentiable augmentation of the critic's inputs (Zhao et al. 2020): per sample a colour change (brightness b,
// contrast c about the sample's mean), an integer translation (ty, tx) with zero fill and a cutout window, in that order, and
// the adjoint of the three. The parameters are counter-based draws on the mask generator's scheme (bn_acc.h):
// a pure function of (policy, seed, key, H, W), restated in numpy by tests/diffaug_ref.py.
//
//   forward   v[p] = c (x[p] - m) + (m + b),  m = mean(x)           y[q]  = v[q - t]  if q - t is in the image and q outside the window, else 0
//   adjoint   dv[p] = dy[p + t]  if p + t is in the image and outside the window, else 0         dx[p] = c dv[p] + (1 - c) mean(dv)
//
// Both directions are one pass  out[q] = f(in[q - s])  (s = t forward, s = -t in the adjoint; the window is tested at q forward and
// at q - s in the adjoint), so one apply kernel serves both. With colour on, a partial-sum launch comes first: PARTS(H, W) fp64
// partial sums per sample in a fixed order (per thread, then a fixed shuffle tree, then the four waves in order), which EVERY
// workgroup of the apply launch re-adds in index order in fp64: no finish launch, no float atomics, and a sample's result depends
// on (H, W) and its own pixels only - not on n, on its row or on how the workgroups are scheduled. The partials live in a small
// buffer of the context (one context per stream, so launches that share it are ordered); calls of more than MAX_N samples are
// issued in pieces. With colour off the values are moved as 32-bit words: bit for bit, NaN payloads and -0 included.
//
// Which side is vectorised: a shifted row is unaligned on one side whatever is done. The STORE side is kept aligned (one 16-byte
// store per lane, whole 64-byte segments per quarter-wave): a partial-line store costs a read-modify-write at the memory side,
// while an unaligned 16-byte load only touches one more cache line per wave, which the neighbouring wave wants anyway. The loads
// are therefore 16-byte loads of 4-byte alignment (global_load_dwordx4 takes any dword address); groups that straddle the image's
// border, and every width that is not a multiple of four (or an output that is not 16-byte aligned), go element by element.
#include "bn_acc.h"
#include "common.h"

// the colour arithmetic rounds after every operation (no FMA contraction): tests/diffaug_ref.py restates it step by step
#pragma clang fp contract(off)

namespace {

constexpr int MAX_PARTS = 64;     // partial sums per sample, at most
constexpr int MAX_N = 256;        // samples per launch (the context's partial buffer holds MAX_N * MAX_PARTS doubles)
constexpr int ITEMS_PER_PART = 1024;
constexpr uint64_t SEED_SALT = 0x4449464641554721ull;   // "DIFFAUG!": equal seeds do not replay the mask generator's streams
constexpr int POL_COLOUR = 1, POL_TRANSLATION = 2, POL_CUTOUT = 4;

typedef uint32_t u4a4_t __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte load from any 4-byte aligned address

__device__ __forceinline__ uint32_t draw32(uint64_t stream, int k) { return (uint32_t)(gi_mix64(stream + GI_GOLDEN64 * (uint64_t)(k + 1)) >> 32); }
__device__ __forceinline__ int uni_of(uint32_t d, int lo, int hi) { return lo + (int)__umulhi(d, (uint32_t)(hi - lo + 1)); }

// the table's row of a sample: b, c, ty, tx, y0, x0, ch, cw (the window unclipped: rows y0 <= q0 < y0 + ch)
struct Params { float b, c; int ty, tx, y0, x0, ch, cw; };
static_assert(sizeof(Params) == 32, "8 32-bit words per sample");

// where a launch takes its parameters from: a table on the device, or the draws themselves (the production entries)
struct Source {
  const Params* table;
  uint64_t seed, key0;    // seed already salted
  int policy;
};

__device__ __forceinline__ Params draw_params(int policy, uint64_t seed, uint64_t key, int H, int W) {
  const uint64_t st = gi_mix64(seed + GI_GOLDEN64 * (key + 1ull));
  Params p;
  p.b = 0.f; p.c = 1.f; p.ty = p.tx = 0; p.y0 = p.x0 = p.ch = p.cw = 0;
  if (policy & POL_COLOUR) {
    p.b = (float)(draw32(st, 0) >> 8) * 0x1p-24f - 0.5f;     // exact: a multiple of 2^-24 in [-0.5, 0.5)
    p.c = 0.5f + (float)(draw32(st, 1) >> 9) * 0x1p-23f;     // exact: a multiple of 2^-23 in [0.5, 1.5)
  }
  if (policy & POL_TRANSLATION) {
    p.ty = uni_of(draw32(st, 2), -(H / 8), H / 8);
    p.tx = uni_of(draw32(st, 3), -(W / 8), W / 8);
  }
  if (policy & POL_CUTOUT) {
    p.ch = H / 2; p.cw = W / 2;
    p.y0 = uni_of(draw32(st, 4), 0, H) - p.ch / 2;
    p.x0 = uni_of(draw32(st, 5), 0, W) - p.cw / 2;
  }
  return p;
}

__device__ __forceinline__ Params params_of(const Source& s, int i, int H, int W) {
  return s.table ? s.table[i] : draw_params(s.policy, s.seed, s.key0 + (uint64_t)i, H, W);
}

__global__ void __launch_bounds__(256) diffaug_params_kernel(int policy, uint64_t seed, uint64_t key0, int n, int H, int W, Params* table) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) table[i] = draw_params(policy, seed, key0 + (uint64_t)i, H, W);
}

__device__ __forceinline__ bool in_window(const Params& p, int y, int x) {
  return y >= p.y0 && y - p.y0 < p.ch && x >= p.x0 && x - p.x0 < p.cw;
}

struct AugP {
  const uint32_t* in;      // n samples of H * W words
  uint32_t* out;
  double* partials;        // [n][parts]
  Source src;
  int n, H, W;
  int items;               // per sample: H * W / E
  int parts, per_part;     // partial sums per sample, items per partial sum
  int adjoint, colour;
};

// Partial sums of a sample's mean. Forward: every pixel of x. Adjoint: sum(dv) = the sum of dy over the positions q the forward pass
// wrote a value to (q - t in the image, q outside the window). E pixels per item; blockIdx.x = part, blockIdx.y = sample.
template <int E>
__global__ void __launch_bounds__(256) diffaug_partial_kernel(AugP a) {
  __shared__ double s_w[4];
  const int i = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const Params p = params_of(a.src, i, H, W);
  const uint32_t* in = a.in + (int64_t)i * H * W;
  const int g0 = part * a.per_part, g1 = min(g0 + a.per_part, a.items);
  const int ipr = W / E;     // items per row (E == 4: W % 4 == 0)
  double s = 0.0;
  for (int g = g0 + tid; g < g1; g += 256) {
    uint32_t w[E];
    if constexpr (E == 4) {
      const u4_t q = *(const u4_t*)(in + (int64_t)g * 4);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
      w[0] = in[g];
    }
    if (a.adjoint) {   // select, never multiply: a NaN or an infinity outside the kept set must not reach the sum
      const int y = g / ipr, x0 = (g - y * ipr) * E;
      const int ys = y - p.ty, yw = y - p.y0;
      const int row_in = (ys >= 0) & (ys < H), row_win = (yw >= 0) & (yw < p.ch);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int xs = x0 + e - p.tx, xw = x0 + e - p.x0;
        const int keep = row_in & (xs >= 0) & (xs < W) & !(row_win & (xw >= 0) & (xw < p.cw));
        w[e] &= (uint32_t)-keep;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) s += (double)__uint_as_float(w[e]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) s_w[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) a.partials[(int64_t)i * a.parts + part] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// out[q] = f(in[q - s]); E pixels per item, 256 * ITEMS items per workgroup; blockIdx.y = sample.
template <int E, bool COLOUR>
__global__ void __launch_bounds__(256) diffaug_apply_kernel(AugP a) {
  constexpr int ITEMS = 4;
  __shared__ double s_part[MAX_PARTS];
  __shared__ float s_mean;
  const int i = blockIdx.y, tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const Params p = params_of(a.src, i, H, W);
  const uint32_t* in = a.in + (int64_t)i * H * W;
  uint32_t* out = a.out + (int64_t)i * H * W;
  const int sy = a.adjoint ? -p.ty : p.ty, sx = a.adjoint ? -p.tx : p.tx;
  float mean = 0.f;
  if constexpr (COLOUR) {
    if (tid < MAX_PARTS) s_part[tid] = tid < a.parts ? a.partials[(int64_t)i * a.parts + tid] : 0.0;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < a.parts; ++k) s += s_part[k];
      s_mean = (float)(s / (double)((int64_t)H * W));
    }
    __syncthreads();
    mean = s_mean;
  }
  // forward: y = c * (x - m) + (m + b); adjoint: dx = c * dv + (1 - c) * mean(dv). Every operation rounds once, in this order
  // (contraction into an FMA is off for this file): tests/diffaug_ref.py fwd32 / bwd32
  const float add = a.adjoint ? (1.f - p.c) * mean : mean + p.b;
  const int ipr = W / E;
  const int g_base = blockIdx.x * (256 * ITEMS);
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int g = g_base + it * 256 + tid;
    if (g >= a.items) break;
    const int y = g / ipr, x0 = (g - y * ipr) * E;
    const int ys = y - sy, xs0 = x0 - sx;
    uint32_t w[E];
#pragma unroll
    for (int e = 0; e < E; ++e) w[e] = 0u;
    bool have[E];
#pragma unroll
    for (int e = 0; e < E; ++e) have[e] = false;
    if (ys >= 0 && ys < H) {
      const uint32_t* row = in + (int64_t)ys * W;
      if (E == 4 && xs0 >= 0 && xs0 + 3 < W) {
        const u4a4_t q = *(const u4a4_t*)(row + xs0);
        w[0] = q.x;
        if constexpr (E == 4) { w[1] = q.y; w[2] = q.z; w[3] = q.w; }
#pragma unroll
        for (int e = 0; e < E; ++e) have[e] = true;
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int xs = xs0 + e;
          if (xs >= 0 && xs < W) { w[e] = row[xs]; have[e] = true; }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      // the window lies in the coordinates of the forward pass's OUTPUT: q forward, the source position in the adjoint
      const bool cut = a.adjoint ? in_window(p, ys, xs0 + e) : in_window(p, y, x0 + e);
      if (cut) { have[e] = false; w[e] = 0u; }
      if constexpr (COLOUR) {
        const float v = __uint_as_float(w[e]);
        if (a.adjoint) w[e] = __float_as_uint(p.c * v + add);                   // zeros of dv included
        else if (have[e]) w[e] = __float_as_uint(p.c * (v - mean) + add);
      }
    }
    if constexpr (E == 4) {
      u4_t o;
      o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
      *(u4_t*)(out + (int64_t)g * 4) = o;
    } else {
      out[g] = w[0];
    }
  }
}

int policy_ok(int policy) { return policy > 0 && policy <= (POL_COLOUR | POL_TRANSLATION | POL_CUTOUT); }

// one direction of n samples; src.table (if any) holds n rows
int run(gi_ctx* ctx, const char* who, const float* in, Source src, int n, int H, int W, int adjoint, int colour, float* out) {
  GI_REQUIRE(ctx && in && out, "%s: null argument", who);
  GI_REQUIRE(n > 0 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff, "%s: n = %d, %d x %d", who, n, H, W);
  GI_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "%s: a buffer is not 4-byte aligned", who);
  const int64_t hw = (int64_t)H * W;
  const float *in_end = in + hw * n, *out_end = out + hw * n;
  GI_REQUIRE(in_end <= out || out_end <= in, "%s: the input and the output overlap", who);
  if (colour && !ctx->diffaug_partials) GI_HIP(hipMalloc((void**)&ctx->diffaug_partials, sizeof(double) * MAX_N * MAX_PARTS));
  // 16-byte path: rows and samples keep the alignment of the base pointers. The partial sums read `in` only
  const bool vec_in = (W & 3) == 0 && ((uintptr_t)in & 15) == 0, vec_out = (W & 3) == 0 && ((uintptr_t)out & 15) == 0;
  for (int i0 = 0; i0 < n; i0 += MAX_N) {
    AugP a;
    a.n = n - i0 < MAX_N ? n - i0 : MAX_N;
    a.in = (const uint32_t*)(in + hw * i0);
    a.out = (uint32_t*)(out + hw * i0);
    a.partials = ctx->diffaug_partials;
    a.src = src;
    if (src.table) a.src.table = src.table + i0;
    a.src.key0 = src.key0 + (uint64_t)i0;
    a.H = H; a.W = W; a.adjoint = adjoint; a.colour = colour;
    a.parts = 1; a.per_part = 0;
    if (colour) {
      a.items = (int)(vec_in ? hw / 4 : hw);
      // a function of (H, W) and the input's alignment alone: a sample's sum does not depend on n or on its row
      a.parts = (a.items + ITEMS_PER_PART - 1) / ITEMS_PER_PART;
      if (a.parts > MAX_PARTS) a.parts = MAX_PARTS;
      a.per_part = (a.items + a.parts - 1) / a.parts;
      const dim3 grid((unsigned)a.parts, (unsigned)a.n);
      if (vec_in) hipLaunchKernelGGL(diffaug_partial_kernel<4>, grid, dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL(diffaug_partial_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
      GI_LAUNCH_CHECK();
    }
    a.items = (int)(vec_out ? hw / 4 : hw);
    const dim3 grid((unsigned)((a.items + 1023) / 1024), (unsigned)a.n);
    if (vec_out) {
      if (colour) hipLaunchKernelGGL((diffaug_apply_kernel<4, true>), grid, dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL((diffaug_apply_kernel<4, false>), grid, dim3(256), 0, ctx->stream, a);
    } else {
      if (colour) hipLaunchKernelGGL((diffaug_apply_kernel<1, true>), grid, dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL((diffaug_apply_kernel<1, false>), grid, dim3(256), 0, ctx->stream, a);
    }
    GI_LAUNCH_CHECK();
  }
  return GI_OK;
}

}  // namespace

extern "C" {

int gi_diffaug_params(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, int n, int H, int W, void* table) {
  GI_REQUIRE(ctx && table, "diffaug_params: null argument");
  GI_REQUIRE(policy_ok(policy), "diffaug_params: policy %d (bits 1 colour, 2 translation, 4 cutout)", policy);
  GI_REQUIRE(n > 0 && H >= 1 && W >= 1, "diffaug_params: n = %d, %d x %d", n, H, W);
  GI_REQUIRE(((uintptr_t)table & 3) == 0, "diffaug_params: table is not 4-byte aligned");
  hipLaunchKernelGGL(diffaug_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, policy, seed ^ SEED_SALT, key0, n, H, W,
                     (Params*)table);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_diffaug_fwd(gi_ctx* ctx, const float* x, const void* table, int n, int H, int W, int colour, float* y) {
  GI_REQUIRE(table && ((uintptr_t)table & 3) == 0, "diffaug_fwd: table is null or not 4-byte aligned");
  Source s;
  s.table = (const Params*)table; s.seed = 0; s.key0 = 0; s.policy = 0;
  return run(ctx, "diffaug_fwd", x, s, n, H, W, 0, colour ? 1 : 0, y);
}

int gi_diffaug_bwd(gi_ctx* ctx, const float* dy, const void* table, int n, int H, int W, int colour, float* dx) {
  GI_REQUIRE(table && ((uintptr_t)table & 3) == 0, "diffaug_bwd: table is null or not 4-byte aligned");
  Source s;
  s.table = (const Params*)table; s.seed = 0; s.key0 = 0; s.policy = 0;
  return run(ctx, "diffaug_bwd", dy, s, n, H, W, 1, colour ? 1 : 0, dx);
}

int gi_diffaug_apply(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, const float* x, int n, int H, int W, float* y) {
  GI_REQUIRE(policy_ok(policy), "diffaug_apply: policy %d (bits 1 colour, 2 translation, 4 cutout)", policy);
  Source s;
  s.table = nullptr; s.seed = seed ^ SEED_SALT; s.key0 = key0; s.policy = policy;
  return run(ctx, "diffaug_apply", x, s, n, H, W, 0, policy & POL_COLOUR, y);
}

int gi_diffaug_apply_bwd(gi_ctx* ctx, int policy, uint64_t seed, uint64_t key0, const float* dy, int n, int H, int W, float* dx) {
  GI_REQUIRE(policy_ok(policy), "diffaug_apply_bwd: policy %d (bits 1 colour, 2 translation, 4 cutout)", policy);
  Source s;
  s.table = nullptr; s.seed = seed ^ SEED_SALT; s.key0 = key0; s.policy = policy;
  return run(ctx, "diffaug_apply_bwd", dy, s, n, H, W, 1, policy & POL_COLOUR, dx);
}

}  // extern "C"
