// C-ABI glue: error reporting, context, single-layer entry points (see include/ganinpaint.h).
#include <string.h>

#include <stdlib.h>

#include "common.h"
#include "stat_acc.h"
#include "igemm_plan.h"

static thread_local char g_err[1024] = "";

void gi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {
// state 0: unread, 1: from default / environment, 2: set by the caller. value / state are relaxed atomics: two host threads that
// drive separate contexts may read (and lazily initialise, to the same value) an option at the same time
struct OptDesc { const char* name; int dflt; int value; int state; };
inline int opt_load(const int& v) { return __atomic_load_n(&v, __ATOMIC_RELAXED); }
inline void opt_store(int& v, int x) { __atomic_store_n(&v, x, __ATOMIC_RELAXED); }
OptDesc g_opts[GI_OPT_COUNT] = {
  {"GI_IGEMM5", 7, 0, 0}, {"GI_IGEMM6", 1, 0, 0}, {"GI_IGEMM7", 1, 0, 0}, {"GI_IGEMM_FIXUP", 1, 0, 0}, {"GI_IGEMM_VARIANT", 3, 0, 0},
  {"GI_BN_ACC", 1, 0, 0}, {"GI_FUSE_HEAD", 1, 0, 0}, {"GI_HEAD_FAST", 1, 0, 0}, {"GI_BN_BWD_FUSE", 1, 0, 0}, {"GI_BN_BWD_SMALL", 512, 0, 0},
  {"GI_WGRAD2", 1, 0, 0}, {"GI_WGRAD3", 1, 0, 0}, {"GI_IGEMM8", 1, 0, 0}, {"GI_BN_FOLD", 0, 0, 0}, {"GI_C1_FUSED", 1, 0, 0},
  {"GI_WGRAD_STREAM", 1, 0, 0}, {"GI_MASK_BITS", 1, 0, 0}, {"GI_C1W_FUSE", 1, 0, 0}, {"GI_IGEMM7_WAVES", 8, 0, 0},
};
thread_local const char* g_last_kernel = "";   // per host thread: gi_debug_last_kernel never reports another thread's launch
int g_fold_count = 0;
}  // namespace
void gi_note_fold() { __atomic_fetch_add(&g_fold_count, 1, __ATOMIC_RELAXED); }

int gi_opt(int id) {
  OptDesc& o = g_opts[id];
  if (opt_load(o.state) == 0) {
    const char* e = getenv(o.name);
    opt_store(o.value, e ? atoi(e) : o.dflt);
    __atomic_store_n(&o.state, 1, __ATOMIC_RELEASE);
  }
  return opt_load(o.value);
}
void gi_note_kernel(const char* name) { g_last_kernel = name; }

extern "C" {

int gi_set_option(const char* name, int value) {
  GI_REQUIRE(name, "set_option: null name");
  for (int i = 0; i < GI_OPT_COUNT; ++i)
    if (strcmp(name, g_opts[i].name) == 0) {
      if (value < 0) opt_store(g_opts[i].state, 0);      // back to the environment / default
      else { opt_store(g_opts[i].value, value); __atomic_store_n(&g_opts[i].state, 2, __ATOMIC_RELEASE); }
      return GI_OK;
    }
  gi_set_error("set_option: unknown option '%s'", name);
  return GI_ERR_INVALID;
}
int gi_get_option(const char* name, int* value) {
  GI_REQUIRE(name && value, "get_option: null argument");
  for (int i = 0; i < GI_OPT_COUNT; ++i)
    if (strcmp(name, g_opts[i].name) == 0) { *value = gi_opt(i); return GI_OK; }
  gi_set_error("get_option: unknown option '%s'", name);
  return GI_ERR_INVALID;
}
const char* gi_debug_last_kernel(void) { return g_last_kernel; }
int gi_debug_fold_count(void) { return __atomic_load_n(&g_fold_count, __ATOMIC_RELAXED); }

const char* gi_last_error(void) { return g_err; }
int gi_version(void) { return 100; }

int gi_ctx_create(int device_id, void* hip_stream, gi_ctx** out) {
  GI_REQUIRE(out != nullptr, "ctx_create: out is null");
  int count = 0;
  GI_HIP(hipGetDeviceCount(&count));
  GI_REQUIRE(device_id >= 0 && device_id < count, "ctx_create: device %d not present (%d visible)", device_id, count);
  GI_HIP(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  GI_HIP(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    gi_set_error("ctx_create: device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
    return GI_ERR_UNSUPPORTED;
  }
  gi_ctx* c = new gi_ctx();
  c->device = device_id;
  c->stream = (hipStream_t)hip_stream;
  *out = c;
  return GI_OK;
}
int gi_ctx_destroy(gi_ctx* ctx) {
  if (ctx && ctx->tickets) (void)hipFree(ctx->tickets);
  if (ctx && ctx->absmean_partials) (void)hipFree(ctx->absmean_partials);
  if (ctx && ctx->diffaug_partials) (void)hipFree(ctx->diffaug_partials);
  delete ctx;
  return GI_OK;
}
int gi_ctx_sync(gi_ctx* ctx) {
  GI_REQUIRE(ctx, "ctx_sync: null");
  GI_HIP(hipStreamSynchronize(ctx->stream));
  return GI_OK;
}

static unsigned* ctx_tickets(gi_ctx* ctx) {
  if (!ctx->tickets) {
    if (hipMalloc((void**)&ctx->tickets, GI_IGEMM_TICKETS * 4) != hipSuccess) { ctx->tickets = nullptr; return nullptr; }
    if (hipMemset(ctx->tickets, 0, GI_IGEMM_TICKETS * 4) != hipSuccess) { (void)hipFree(ctx->tickets); ctx->tickets = nullptr; }
  }
  return ctx->tickets;
}

int gi_conv_s2_forward(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out, int n, int H, int W, int cb, int ldin,
                       int ca, int ldout, int relu_in, int act_out, float* ws, int64_t ws_bytes) {
  GI_REQUIRE(ctx && in && w_packed && out, "conv_s2_forward: null pointer");
  GI_REQUIRE(H % 2 == 0 && W % 2 == 0, "conv_s2_forward: H=%d W=%d must be even", H, W);
  IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.w = w_packed; a.out = out; a.ws = ws; a.ws_bytes = ws_bytes;
  a.tickets = ws ? ctx_tickets(ctx) : nullptr;
  a.n = n; a.Hs = H / 2; a.Ws = W / 2;
  a.cin = cb; a.ldin = ldin; a.cout = ca; a.ldout = ldout;
  a.relu_in = relu_in; a.act_out = act_out;
  return op_igemm(ctx->stream, dtype, 0, a);
}

int gi_convT_s2_forward(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out, int n, int H, int W, int ca, int ldin,
                        int cb, int ldout, int relu_in, int act_out, float* ws, int64_t ws_bytes) {
  GI_REQUIRE(ctx && in && w_phase && out, "convT_s2_forward: null pointer");
  IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.w = w_phase; a.out = out; a.ws = ws; a.ws_bytes = ws_bytes;
  a.tickets = ws ? ctx_tickets(ctx) : nullptr;
  a.n = n; a.Hs = H; a.Ws = W;
  a.cin = ca; a.ldin = ldin; a.cout = cb; a.ldout = ldout;
  a.relu_in = relu_in; a.act_out = act_out;
  return op_igemm(ctx->stream, dtype, 1, a);
}

// the same two layers with the optional fused epilogues of IgemmArgs (what the networks pass; include/ganinpaint.h: gi_igemm_ex)
static int apply_ex(IgemmArgs& a, const gi_igemm_ex* ex) {
  if (!ex) return GI_OK;
  // relu_cend is a HINT (IgemmArgs::relu_cend): kernels apply the input ReLU per 32- or 64-channel chunk up to it, the generic
  // kernel to every channel - all agree only when the channels from relu_cend on are non-negative already and it is chunk-aligned
  GI_REQUIRE(ex->relu_cend >= 0 && ex->relu_cend % 64 == 0 && ex->relu_cend <= a.cin, "igemm_ex: relu_cend=%d must be a multiple of 64 within the %d input channels",
             ex->relu_cend, a.cin);
  a.relu_cend = ex->relu_cend;
  a.mask = ex->mask; a.ldmask = ex->ldmask; a.mask_slope = ex->mask_slope;
  a.add = ex->add; a.ldadd = ex->ldadd;
  a.mask_bits = ex->mask ? ex->mask_bits : nullptr;
  a.stat_acc = ex->stat_acc; a.stat_reps = ex->stat_reps; a.stat_pg = ex->stat_pg;
  a.partials = ex->partials;
  a.bwd_x = ex->bwd_x; a.bwd_ldx = ex->bwd_ldx; a.bwd_scale = ex->bwd_scale; a.bwd_shift = ex->bwd_shift; a.bwd_mean = ex->bwd_mean;
  a.bwd_inv = ex->bwd_inv; a.bwd_stride = ex->bwd_stride; a.bwd_slope = ex->bwd_slope; a.bwd_acc = ex->bwd_acc; a.bwd_reps = ex->bwd_reps;
  a.bwd_pg = ex->bwd_pg;
  a.bwd_c0 = ex->bwd_c0; a.bwd_c = ex->bwd_c;
  return GI_OK;
}
static void return_ex(const IgemmArgs& a, gi_igemm_ex* ex) {
  if (!ex) return;
  ex->mask_applied = a.mask_applied; ex->bwd_applied = a.bwd_applied; ex->stat_used = a.stat_used; ex->ntiles_out = a.ntiles_out;
}

int gi_conv_s2_forward_ex(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out, int n, int H, int W, int cb, int ldin,
                          int ca, int ldout, int relu_in, int act_out, float* ws, int64_t ws_bytes, gi_igemm_ex* ex) {
  GI_REQUIRE(ctx && in && w_packed && out, "conv_s2_forward_ex: null pointer");
  GI_REQUIRE(H % 2 == 0 && W % 2 == 0, "conv_s2_forward_ex: H=%d W=%d must be even", H, W);
  IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.w = w_packed; a.out = out; a.ws = ws; a.ws_bytes = ws_bytes;
  a.tickets = ws ? ctx_tickets(ctx) : nullptr;
  a.n = n; a.Hs = H / 2; a.Ws = W / 2;
  a.cin = cb; a.ldin = ldin; a.cout = ca; a.ldout = ldout;
  a.relu_in = relu_in; a.act_out = act_out;
  GI_TRY(apply_ex(a, ex));
  const int rc = op_igemm(ctx->stream, dtype, 0, a);
  return_ex(a, ex);
  return rc;
}

int gi_convT_s2_forward_ex(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out, int n, int H, int W, int ca, int ldin,
                           int cb, int ldout, int relu_in, int act_out, float* ws, int64_t ws_bytes, gi_igemm_ex* ex) {
  GI_REQUIRE(ctx && in && w_phase && out, "convT_s2_forward_ex: null pointer");
  IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.w = w_phase; a.out = out; a.ws = ws; a.ws_bytes = ws_bytes;
  a.tickets = ws ? ctx_tickets(ctx) : nullptr;
  a.n = n; a.Hs = H; a.Ws = W;
  a.cin = ca; a.ldin = ldin; a.cout = cb; a.ldout = ldout;
  a.relu_in = relu_in; a.act_out = act_out;
  GI_TRY(apply_ex(a, ex));
  const int rc = op_igemm(ctx->stream, dtype, 1, a);
  return_ex(a, ex);
  return rc;
}

int gi_debug_igemm_plan(int dtype, int mode, int n, int Hs, int Ws, int cin, int ldin, int cout, int ldout, int relu_in, int act_out,
                        int64_t ws_bytes, int has_tickets, const gi_igemm_ex* ex, int offered, gi_igemm_plan_info* out) {
  GI_REQUIRE(out, "debug_igemm_plan: null pointer");
  static char dummy[8];   // stands for every operand: the plan only asks whether a pointer is null
  IgemmArgs a;
  memset(&a, 0, sizeof(a));
  a.in = a.w = a.out = dummy;
  if (ws_bytes > 0) { a.ws = (float*)dummy; a.ws_bytes = ws_bytes; }
  a.tickets = has_tickets ? (unsigned*)dummy : nullptr;
  a.n = n; a.Hs = Hs; a.Ws = Ws;
  a.cin = cin; a.ldin = ldin; a.cout = cout; a.ldout = ldout;
  a.relu_in = relu_in; a.act_out = act_out;
  GI_TRY(apply_ex(a, ex));
  IgemmFold fold = {};
  if ((offered & 1) && a.stat_acc) { fold.bn.groups = 1; fold.bn.acc = a.stat_acc; fold.lddst = ldout; fold.act = GI_ACT_RELU; a.fold = &fold; }
  if ((offered & 2) && a.mask_bits) { a.c1w_img = (const float*)dummy; a.c1w_part = (float*)dummy; a.c1w_part_floats = (int64_t)1 << 40; a.c1w_scale = 1.f; }
  if (offered & 4) a.pool2 = 1;
  if (offered & 8) a.bias = (const float*)dummy;
  IgemmPlan p;
  GI_TRY(gi_igemm_plan(dtype, mode, a, &p));
  gi_igemm_returns(p, a);
  memset(out, 0, sizeof(*out));
  strncpy(out->name, p.name, sizeof(out->name) - 1);
  out->grid = p.grid; out->splitk = p.splitk > 1 ? p.splitk : 1; out->ntiles_out = a.ntiles_out;
  out->mask_applied = a.mask_applied; out->bwd_applied = a.bwd_applied; out->stat_used = a.stat_used;
  out->c1w_applied = a.c1w_applied; out->c1w_blocks = a.c1w_blocks; out->pool_applied = a.pool_applied; out->fold_applied = a.fold_applied;
  return GI_OK;
}

int64_t gi_stat_acc_words(int c) { return gi_stat_block_words(c, GI_STAT_MAXREP); }

namespace {
__global__ void __launch_bounds__(256) stat_acc_read_kernel(const unsigned long long* acc, int c, int reps, int group, double* out) {
  for (int ch = blockIdx.x * 256 + threadIdx.x; ch < c; ch += gridDim.x * 256) {
    out[ch] = gi_stat_read(acc, c, reps, group, 0, ch);
    out[c + ch] = gi_stat_read(acc, c, reps, group, 1, ch);
  }
}
}  // namespace

int gi_stat_acc_read(gi_ctx* ctx, const unsigned long long* acc, int c, int reps, int group, double* out_dev) {
  GI_REQUIRE(ctx && acc && out_dev && c > 0 && reps >= 1 && reps <= GI_STAT_MAXREP && (group == 0 || group == 1), "stat_acc_read: bad argument");
  hipLaunchKernelGGL(stat_acc_read_kernel, dim3((c + 255) / 256), dim3(256), 0, ctx->stream, acc, c, reps, group, out_dev);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

int gi_wgrad_s2(gi_ctx* ctx, int dtype, const void* S, const void* L, float* dW, int n, int Hs, int Ws, int ca, int ldS, int cb, int ldL,
                int relu_S, float scale) {
  GI_REQUIRE(ctx && S && L && dW, "wgrad_s2: null pointer");
  WgradArgs a;
  a.S = S; a.L = L; a.dW = dW; a.n = n; a.Hs = Hs; a.Ws = Ws;
  a.ca = ca; a.ldS = ldS; a.coffS = 0; a.cb = cb; a.ldL = ldL; a.coffL = 0;
  a.relu_S = relu_S; a.scale = scale;
  a.scratch = nullptr; a.scratch_bytes = 0;      // atomics across the pixel-range splits
  return op_wgrad(ctx->stream, dtype, a);
}

int64_t gi_wgrad_s2_scratch_bytes(int dtype, int n, int Hs, int Ws, int ca, int cb) {
  return op_wgrad_scratch_bytes(dtype, n, Hs, Ws, ca, cb);
}

int gi_wgrad_s2_ws(gi_ctx* ctx, int dtype, const void* S, const void* L, float* dW, int n, int Hs, int Ws, int ca, int ldS, int cb, int ldL,
                   int relu_S, float scale, float* scratch, int64_t scratch_bytes) {
  GI_REQUIRE(ctx && S && L && dW, "wgrad_s2_ws: null pointer");
  WgradArgs a;
  a.S = S; a.L = L; a.dW = dW; a.n = n; a.Hs = Hs; a.Ws = Ws;
  a.ca = ca; a.ldS = ldS; a.coffS = 0; a.cb = cb; a.ldL = ldL; a.coffL = 0;
  a.relu_S = relu_S; a.scale = scale;
  a.scratch = scratch; a.scratch_bytes = scratch_bytes;
  return op_wgrad(ctx->stream, dtype, a);
}


// ---- the single-channel layers (c1.hip) on their own: what tests/test_c1_gpu.py drives ------------------------------------------
int gi_c1_gather(gi_ctx* ctx, int dtype, const float* img, const float* w, void* out, int n, int Hs, int Ws, int c, int ldout, int coffout,
                 int act_out, float in_scale, const float* bias, unsigned long long* bits, int* bits_written) {
  GI_REQUIRE(ctx && img && w && out, "c1_gather: null pointer");
  return op_c1_gather(ctx->stream, dtype, img, w, out, n, Hs, Ws, c, ldout, coffout, act_out, in_scale, bias, bits, bits_written);
}

int gi_c1_scatter(gi_ctx* ctx, int dtype, const void* X, const float* w, const float* bias, float* img, int n, int Hs, int Ws, int c, int ldx,
                  int coffx, int relu_in, int post, float out_scale, void* col_scratch, float* img2, const void* x2, int ld2,
                  const float* scale2, const float* shift2) {
  GI_REQUIRE(ctx && X && w && img, "c1_scatter: null pointer");
  GI_REQUIRE(!x2 || (scale2 && shift2), "c1_scatter: x2 without scale2 / shift2");
  C1Affine aff;
  aff.x2 = x2; aff.ld2 = ld2; aff.scale = scale2; aff.shift = shift2;
  return op_c1_scatter(ctx->stream, dtype, X, w, bias, img, n, Hs, Ws, c, ldx, coffx, relu_in, post, out_scale, col_scratch, img2,
                       x2 ? &aff : nullptr);
}

int gi_c1_wgrad(gi_ctx* ctx, int dtype, const void* X, const float* img, float* dW, int n, int Hs, int Ws, int c, int ldx, int coffx,
                int relu_in, float scale, float img_scale, const void* x2, int ld2, const float* scale2, const float* shift2, float* scratch,
                int64_t scratch_floats) {
  GI_REQUIRE(ctx && X && img && dW, "c1_wgrad: null pointer");
  GI_REQUIRE(!x2 || (scale2 && shift2), "c1_wgrad: x2 without scale2 / shift2");
  C1Affine aff;
  aff.x2 = x2; aff.ld2 = ld2; aff.scale = scale2; aff.shift = shift2;
  return op_c1_wgrad(ctx->stream, dtype, X, img, dW, n, Hs, Ws, c, ldx, coffx, relu_in, scale, img_scale, x2 ? &aff : nullptr, scratch,
                     scratch_floats);
}

int gi_c1_wgrad_reduce(gi_ctx* ctx, const float* part, float* dW, int count, int blocks, float* scratch, int64_t scratch_floats) {
  GI_REQUIRE(ctx && part && dW, "c1_wgrad_reduce: null pointer");
  return op_c1_wgrad_reduce(ctx->stream, part, dW, count, blocks, scratch, scratch_floats);
}

int64_t gi_c1_head4_col_bytes(int n, int Hs, int Ws) { return op_c1_head4_col_bytes(n, Hs, Ws); }

int gi_c1_head4_forward(gi_ctx* ctx, const void* X, const float* w, const float* bias, float* out, float* out2, int n, int Hs, int Ws, int ldx,
                        int coffx, int relu_in, void* col_scratch) {
  GI_REQUIRE(ctx && X && w && out && col_scratch, "c1_head4_forward: null pointer");
  GI_REQUIRE(op_c1_head4_ok(GI_F16, 128, 4, Ws, ldx, coffx), "c1_head4_forward: Ws=%d ldx=%d coffx=%d unsupported", Ws, ldx, coffx);
  return op_c1_head4_forward(ctx->stream, X, w, bias, out, out2, n, Hs, Ws, ldx, coffx, relu_in, col_scratch);
}

int gi_c1_head4_dgrad(gi_ctx* ctx, const float* g, const float* w, void* out, int n, int Hs, int Ws, int ldout, int coffout) {
  GI_REQUIRE(ctx && g && w && out, "c1_head4_dgrad: null pointer");
  return op_c1_head4_dgrad(ctx->stream, g, w, out, n, Hs, Ws, ldout, coffout);
}

// ---- the normalisation / activation-backward passes (norm.hip, elementwise.hip) on their own: what tests/test_norm_ops_gpu.py drives ------
namespace {
inline int dbg_epc(int dtype) { return dtype == GI_F16 ? 8 : 4; }
inline bool dbg_dtype_ok(int dtype) { return dtype == GI_F16 || dtype == GI_F32; }
inline bool dbg_act_ok(int act) { return act == GI_ACT_NONE || act == GI_ACT_RELU || act == GI_ACT_LRELU; }
// c as the chunked passes take it: c / chunk a power of two <= 256
inline bool dbg_c_ok(int dtype, int c) { const int e = dbg_epc(dtype); return c > 0 && c % e == 0 && gi_is_pow2(c / e) && c / e <= 256; }
// a (pixels, ld) view at channel offset coff holding c channels, every chunk 16-byte aligned
inline bool dbg_view_ok(int dtype, int c, int ld, int coff) { const int e = dbg_epc(dtype); return coff >= 0 && coff % e == 0 && ld % e == 0 && coff + c <= ld; }

int dbg_bn_acc(const char* who, int c, const gi_bn_acc_args* b, BnAccArgs& o) {
  GI_REQUIRE(b && b->acc && b->gamma && b->beta && b->running_mean && b->running_var && b->scale && b->shift && b->save_mean && b->save_invstd,
             "%s: null pointer", who);
  GI_REQUIRE(b->reps >= 1 && b->reps <= GI_STAT_MAXREP, "%s: reps=%d outside 1..%d", who, b->reps, GI_STAT_MAXREP);
  GI_REQUIRE(b->groups == 1 || b->groups == 2, "%s: groups=%d (1 or 2)", who, b->groups);
  GI_REQUIRE(b->count >= 1, "%s: count=%lld", who, (long long)b->count);
  GI_REQUIRE(b->groups == 1 || b->out_stride >= c, "%s: out_stride=%d below the %d channels", who, b->out_stride, c);
  GI_REQUIRE(b->zero_words >= 0 && (b->zero_words == 0 || b->zero_next), "%s: zero_words=%d without zero_next", who, b->zero_words);
  o.acc = b->acc; o.reps = b->reps; o.gamma = b->gamma; o.beta = b->beta; o.running_mean = b->running_mean; o.running_var = b->running_var;
  o.scale = b->scale; o.shift = b->shift; o.save_mean = b->save_mean; o.save_invstd = b->save_invstd;
  o.count = b->count; o.momentum = b->momentum; o.eps = b->eps; o.groups = b->groups; o.out_stride = b->out_stride;
  o.zero_next = b->zero_words > 0 ? b->zero_next : nullptr; o.zero_words = b->zero_words;
  return GI_OK;
}

// the checks shared by the BatchNorm and the InstanceNorm backward, and the copy into ActBnBwdArgs
int dbg_bwd_args(const char* who, int dtype, const gi_act_bn_bwd_args* s, bool chunks_pow2, ActBnBwdArgs& a) {
  GI_REQUIRE(s && s->dx, "%s: null pointer", who);
  GI_REQUIRE(dbg_dtype_ok(dtype) && dbg_act_ok(s->act), "%s: dtype=%d act=%d", who, dtype, s->act);
  GI_REQUIRE(chunks_pow2 ? dbg_c_ok(dtype, s->c) : (s->c > 0 && s->c % dbg_epc(dtype) == 0), "%s: c=%d unsupported", who, s->c);
  GI_REQUIRE(s->pixels >= 1, "%s: pixels=%lld", who, (long long)s->pixels);
  GI_REQUIRE(s->g1 || s->g2, "%s: no upstream gradient", who);
  GI_REQUIRE(!s->g1 || dbg_view_ok(dtype, s->c, s->ldg1, s->coffg1), "%s: g1 ld=%d coff=%d for %d channels", who, s->ldg1, s->coffg1, s->c);
  GI_REQUIRE(!s->g2 || dbg_view_ok(dtype, s->c, s->ldg2, s->coffg2), "%s: g2 ld=%d coff=%d for %d channels", who, s->ldg2, s->coffg2, s->c);
  GI_REQUIRE(!s->y || dbg_view_ok(dtype, s->c, s->ldy, s->coffy), "%s: y ld=%d coff=%d for %d channels", who, s->ldy, s->coffy, s->c);
  GI_REQUIRE(s->drop_scale == 1.f || s->act == GI_ACT_RELU,
             "%s: drop_scale=%g with act=%d: the backward takes the dropout zeros from y > 0, which only a ReLU output can carry", who,
             (double)s->drop_scale, s->act);
  memset(&a, 0, sizeof(a));
  a.g1 = s->g1; a.ldg1 = s->ldg1; a.coffg1 = s->coffg1;
  a.g2 = s->g2; a.ldg2 = s->ldg2; a.coffg2 = s->coffg2;
  a.y = s->y; a.ldy = s->ldy; a.coffy = s->coffy;
  a.x = s->x; a.dx = s->dx; a.pixels = s->pixels; a.c = s->c; a.act = s->act; a.drop_scale = s->drop_scale;
  a.has_bn = s->has_bn; a.eval_bn = s->eval_bn;
  a.gamma = s->gamma; a.save_mean = s->save_mean; a.save_invstd = s->save_invstd;
  a.dgamma = s->dgamma; a.dbeta = s->dbeta; a.inv_loss_scale = s->inv_loss_scale;
  a.partials = s->partials; a.sums = s->sums; a.fwd_scale = s->fwd_scale; a.fwd_shift = s->fwd_shift;
  a.groups = s->groups; a.stat_stride = s->stat_stride;
  a.acc = s->acc; a.acc_reps = s->acc_reps; a.zero_next = s->zero_words > 0 ? s->zero_next : nullptr; a.zero_words = s->zero_words;
  a.reduce_done = s->reduce_done;
  return GI_OK;
}

// one workgroup per row, one lane per channel (the lanes of an atomic instruction are consecutive words, stat_acc.h)
__global__ void __launch_bounds__(256) stat_acc_add_kernel(unsigned long long* acc, int c, int reps, int group, int q, const float* addends) {
  const int r = blockIdx.x;
  for (int ch = threadIdx.x; ch < c; ch += 256) gi_stat_add(acc, c, r & (reps - 1), group, q, ch, addends[(int64_t)r * c + ch]);
}
}  // namespace

int gi_debug_col_stats(gi_ctx* ctx, int dtype, const void* x, int64_t pixels, int c, float* partials, int* rows_out) {
  GI_REQUIRE(ctx && x && partials && rows_out, "debug_col_stats: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && pixels >= 1, "debug_col_stats: dtype=%d pixels=%lld", dtype, (long long)pixels);
  return op_col_stats(ctx->stream, dtype, x, pixels, c, partials, rows_out);
}

int gi_debug_bn_finalize(gi_ctx* ctx, const float* partials, int rows, int c, int64_t count, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* scale, float* shift, float* save_mean, float* save_invstd, int train,
                         float momentum, float eps, int groups, int64_t part_stride, int out_stride) {
  GI_REQUIRE(ctx && gamma && beta && running_mean && running_var && scale && shift && save_mean && save_invstd, "debug_bn_finalize: null pointer");
  GI_REQUIRE(!train || (partials && rows >= 1), "debug_bn_finalize: train mode needs partial rows (rows=%d)", rows);
  GI_REQUIRE(c >= 1 && count >= 1, "debug_bn_finalize: c=%d count=%lld", c, (long long)count);
  GI_REQUIRE(groups == 1 || groups == 2, "debug_bn_finalize: groups=%d (1 or 2)", groups);
  GI_REQUIRE(groups == 1 || (out_stride >= c && (!train || part_stride >= (int64_t)rows * 2 * c)),
             "debug_bn_finalize: two populations overlap (part_stride=%lld out_stride=%d)", (long long)part_stride, out_stride);
  return op_bn_finalize(ctx->stream, partials, rows, c, count, gamma, beta, running_mean, running_var, scale, shift, save_mean, save_invstd, train,
                        momentum, eps, groups, part_stride, out_stride);
}

int gi_debug_bn_apply(gi_ctx* ctx, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy, const float* scale,
                      const float* shift, int act, const uint8_t* drop_mask, float drop_scale, int64_t pg, int gstride) {
  GI_REQUIRE(ctx && x && y, "debug_bn_apply: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && dbg_act_ok(act) && pixels >= 1, "debug_bn_apply: dtype=%d act=%d pixels=%lld", dtype, act, (long long)pixels);
  GI_REQUIRE(dbg_c_ok(dtype, c), "debug_bn_apply: c=%d unsupported", c);
  GI_REQUIRE(dbg_view_ok(dtype, c, ldy, coffy), "debug_bn_apply: ldy=%d coffy=%d for %d channels", ldy, coffy, c);
  GI_REQUIRE((scale == nullptr) == (shift == nullptr), "debug_bn_apply: scale and shift go together");
  GI_REQUIRE(pg >= 0 && pg <= pixels, "debug_bn_apply: pg=%lld of %lld pixels", (long long)pg, (long long)pixels);
  GI_REQUIRE(!(pg > 0 && pg < pixels) || gstride >= c, "debug_bn_apply: gstride=%d below the %d channels", gstride, c);
  return op_bn_apply(ctx->stream, dtype, x, y, pixels, c, ldy, coffy, scale, shift, act, drop_mask, drop_scale, pg, gstride);
}

int gi_debug_bn_finalize_acc(gi_ctx* ctx, int c, const gi_bn_acc_args* b) {
  GI_REQUIRE(ctx && c >= 1, "debug_bn_finalize_acc: bad argument");
  BnAccArgs o;
  GI_TRY(dbg_bn_acc("debug_bn_finalize_acc", c, b, o));
  return op_bn_finalize_acc(ctx->stream, c, o);
}

int gi_debug_bn_apply_acc(gi_ctx* ctx, int dtype, const void* x, void* y, int64_t pixels, int c, int ldy, int coffy, int act, uint8_t* drop_mask,
                          float drop_scale, uint64_t drop_seed, float drop_p, const gi_bn_acc_args* b, const void* side_src, void* side_dst,
                          int64_t side_bytes) {
  GI_REQUIRE(ctx && x && y, "debug_bn_apply_acc: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && dbg_act_ok(act) && pixels >= 1, "debug_bn_apply_acc: dtype=%d act=%d pixels=%lld", dtype, act, (long long)pixels);
  GI_REQUIRE(dbg_c_ok(dtype, c), "debug_bn_apply_acc: c=%d unsupported", c);
  GI_REQUIRE(dbg_view_ok(dtype, c, ldy, coffy), "debug_bn_apply_acc: ldy=%d coffy=%d for %d channels", ldy, coffy, c);
  GI_REQUIRE(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || drop_mask), "debug_bn_apply_acc: drop_p=%g needs a mask to store the draw", (double)drop_p);
  GI_REQUIRE(side_bytes >= 0, "debug_bn_apply_acc: side_bytes=%lld", (long long)side_bytes);
  BnAccArgs o;
  GI_TRY(dbg_bn_acc("debug_bn_apply_acc", c, b, o));
  return op_bn_apply_acc(ctx->stream, dtype, x, y, pixels, c, ldy, coffy, act, drop_mask, drop_scale, drop_seed, drop_p, o, side_src, side_dst,
                         side_bytes);
}

int gi_debug_act_bn_bwd(gi_ctx* ctx, int dtype, const gi_act_bn_bwd_args* s) {
  GI_REQUIRE(ctx, "debug_act_bn_bwd: null context");
  ActBnBwdArgs a;
  GI_TRY(dbg_bwd_args("debug_act_bn_bwd", dtype, s, true, a));
  GI_REQUIRE(a.groups == 1 || a.groups == 2, "debug_act_bn_bwd: groups=%d (1 or 2)", a.groups);
  GI_REQUIRE(a.groups == 1 || a.stat_stride >= a.c, "debug_act_bn_bwd: stat_stride=%d below the %d channels", a.stat_stride, a.c);
  GI_REQUIRE(!a.has_bn || (a.x && a.gamma && a.save_mean && a.save_invstd), "debug_act_bn_bwd: BatchNorm without x / gamma / save_mean / save_invstd");
  GI_REQUIRE((a.fwd_scale == nullptr) == (a.fwd_shift == nullptr), "debug_act_bn_bwd: fwd_scale and fwd_shift go together");
  const bool need_y = a.g2 != nullptr || a.act != GI_ACT_NONE;
  GI_REQUIRE(!need_y || a.y || (a.has_bn && a.fwd_scale), "debug_act_bn_bwd: the activation's sign needs y or fwd_scale / fwd_shift");
  GI_REQUIRE(!a.acc || (a.acc_reps >= 1 && a.acc_reps <= GI_STAT_MAXREP), "debug_act_bn_bwd: acc_reps=%d outside 1..%d", a.acc_reps, GI_STAT_MAXREP);
  GI_REQUIRE(!a.reduce_done || (a.acc && a.has_bn && !a.eval_bn), "debug_act_bn_bwd: reduce_done needs train-mode accumulators");
  GI_REQUIRE(!a.has_bn || a.acc || (a.partials && a.sums), "debug_act_bn_bwd: BatchNorm without accumulators needs partials and sums");
  GI_REQUIRE(a.zero_words >= 0, "debug_act_bn_bwd: zero_words=%d", a.zero_words);
  return op_act_bn_bwd(ctx->stream, dtype, a);
}

int gi_debug_in_forward(gi_ctx* ctx, int dtype, const void* x, void* y, int n, int hw, int c, int ldy, int coffy, int act,
                        const uint8_t* drop_mask, float drop_scale, float eps, float* stats) {
  GI_REQUIRE(ctx && x && y && stats, "debug_in_forward: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && dbg_act_ok(act), "debug_in_forward: dtype=%d act=%d", dtype, act);
  GI_REQUIRE(c > 0 && c % dbg_epc(dtype) == 0 && dbg_view_ok(dtype, c, ldy, coffy), "debug_in_forward: c=%d ldy=%d coffy=%d", c, ldy, coffy);
  return op_in_forward(ctx->stream, dtype, x, y, n, hw, c, ldy, coffy, act, drop_mask, drop_scale, eps, stats);
}

int gi_debug_act_in_bwd(gi_ctx* ctx, int dtype, const gi_act_bn_bwd_args* s, int n, int hw, const float* stats) {
  GI_REQUIRE(ctx && stats, "debug_act_in_bwd: null pointer");
  ActBnBwdArgs a;
  GI_TRY(dbg_bwd_args("debug_act_in_bwd", dtype, s, false, a));
  GI_REQUIRE(n >= 1 && hw >= 1, "debug_act_in_bwd: n=%d hw=%d", n, hw);
  const bool need_y = a.g2 != nullptr || a.act != GI_ACT_NONE;
  GI_REQUIRE(!need_y || a.y, "debug_act_in_bwd: the activation's sign needs y");
  return op_act_in_bwd(ctx->stream, dtype, a, n, hw, stats);
}

int gi_debug_bias_grad(gi_ctx* ctx, int dtype, const void* dz, int64_t pixels, int c, float scale, float* dbias, float* partials) {
  GI_REQUIRE(ctx && dz && dbias && partials, "debug_bias_grad: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && pixels >= 1, "debug_bias_grad: dtype=%d pixels=%lld", dtype, (long long)pixels);
  return op_bias_grad(ctx->stream, dtype, dz, pixels, c, scale, dbias, partials);
}

int gi_debug_tanh_bwd(gi_ctx* ctx, const float* dy, const float* y, float* dx, int64_t count, float scale) {
  GI_REQUIRE(ctx && dy && y && dx && count >= 0, "debug_tanh_bwd: bad argument");
  return op_tanh_bwd(ctx->stream, dy, y, dx, count, scale);
}

int gi_debug_fill_dropout(gi_ctx* ctx, uint8_t* mask_nhwc, int64_t count, uint64_t seed, float p) {
  GI_REQUIRE(ctx && mask_nhwc && count >= 0, "debug_fill_dropout: bad argument");
  GI_REQUIRE(p >= 0.f && p < 1.f, "debug_fill_dropout: p=%g outside [0, 1)", (double)p);
  return op_fill_dropout(ctx->stream, mask_nhwc, count, seed, p);
}

int gi_debug_mask_layout(gi_ctx* ctx, const uint8_t* src, uint8_t* dst, int n, int c, int hw, int to_nhwc) {
  GI_REQUIRE(ctx && src && dst && src != dst, "debug_mask_layout: bad pointer");
  GI_REQUIRE(n >= 1 && c >= 1 && hw >= 1, "debug_mask_layout: n=%d c=%d hw=%d", n, c, hw);
  return op_mask_nchw_to_nhwc(ctx->stream, src, dst, n, c, hw, to_nhwc);
}

int gi_debug_mul_slope(gi_ctx* ctx, int dtype, const void* tin, const void* a, void* tout, int64_t count) {
  GI_REQUIRE(ctx && tin && a && tout, "debug_mul_slope: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && count >= 0, "debug_mul_slope: dtype=%d count=%lld", dtype, (long long)count);
  return op_mul_slope(ctx->stream, dtype, tin, a, tout, count);
}

int gi_debug_bn_tangent_inject(gi_ctx* ctx, int dtype, const void* dta, const void* y, const void* tx, const void* x, void* dxp, int64_t pixels,
                               int c, const float* gamma, const float* mean, const float* inv, float* dgamma, float dgamma_scale, float* partials,
                               float* sums) {
  GI_REQUIRE(ctx && dta && y && tx && x && dxp && gamma && mean && inv && partials && sums, "debug_bn_tangent_inject: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype) && pixels >= 1, "debug_bn_tangent_inject: dtype=%d pixels=%lld", dtype, (long long)pixels);
  return op_bn_tangent_inject(ctx->stream, dtype, dta, y, tx, x, dxp, pixels, c, gamma, mean, inv, dgamma, dgamma_scale, partials, sums);
}

int gi_debug_gp_direction(gi_ctx* ctx, const float* g, int n, int64_t hw, float lam, float* sumsq, float* amax, float* v, float* penalty,
                          float* sc) {
  GI_REQUIRE(ctx && g && sumsq && amax && v && sc, "debug_gp_direction: null pointer");
  GI_REQUIRE(n >= 1 && hw >= 1, "debug_gp_direction: n=%d hw=%lld", n, (long long)hw);
  return op_gp_direction(ctx->stream, g, n, hw, lam, sumsq, amax, v, penalty, sc);
}

int gi_debug_gp_unscale_add(gi_ctx* ctx, const float* src, const float* sc, float* dst, int64_t count) {
  GI_REQUIRE(ctx && src && sc && dst && count >= 0, "debug_gp_unscale_add: bad argument");
  return op_gp_unscale_add(ctx->stream, src, sc, dst, count);
}

int gi_debug_stat_acc_add(gi_ctx* ctx, unsigned long long* acc, int c, int reps, int group, int q, const float* addends, int rows) {
  GI_REQUIRE(ctx && acc && addends, "debug_stat_acc_add: null pointer");
  GI_REQUIRE(c >= 1 && rows >= 1, "debug_stat_acc_add: c=%d rows=%d", c, rows);
  GI_REQUIRE(reps >= 1 && reps <= GI_STAT_MAXREP, "debug_stat_acc_add: reps=%d outside 1..%d", reps, GI_STAT_MAXREP);
  GI_REQUIRE((group == 0 || group == 1) && (q == 0 || q == 1), "debug_stat_acc_add: group=%d q=%d (0 or 1 each)", group, q);
  hipLaunchKernelGGL(stat_acc_add_kernel, dim3(rows), dim3(256), 0, ctx->stream, acc, c, reps, group, q, addends);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// the one-launch weight re-pack of a network's update (pack_batch_kernel / pack_batch64_kernel) on jobs the caller describes
int gi_debug_pack_weights_batch(gi_ctx* ctx, int dtype, const gi_pack_job* jobs, int n) {
  GI_REQUIRE(ctx && jobs, "debug_pack_weights_batch: null pointer");
  GI_REQUIRE(dbg_dtype_ok(dtype), "debug_pack_weights_batch: dtype=%d", dtype);
  GI_REQUIRE(n >= 1 && n <= 16, "debug_pack_weights_batch: %d jobs (1 .. 16)", n);
  PackJobs P;
  P.n = 0;
  bool all64 = true;
  for (int i = 0; i < n; ++i) all64 = all64 && jobs[i].ca > 0 && jobs[i].cb > 0 && jobs[i].ca % 64 == 0 && jobs[i].cb % 64 == 0;
  for (int i = 0; i < n; ++i) {
    const gi_pack_job& s = jobs[i];
    GI_REQUIRE(s.w, "debug_pack_weights_batch: job %d has no weights", i);
    GI_REQUIRE(s.ca >= 1 && s.cb >= 1 && s.ca <= 4096 && s.cb <= 4096, "debug_pack_weights_batch: job %d ca=%d cb=%d", i, s.ca, s.cb);
    GI_REQUIRE(s.scale_on_b == 0 || s.scale_on_b == 1, "debug_pack_weights_batch: job %d scale_on_b=%d", i, s.scale_on_b);
    // the 64 x 64 kernel moves four values per lane: 16-byte chunks of fp32, 8-byte ones of fp16
    const uintptr_t in = reinterpret_cast<uintptr_t>(s.w) | (s.scale_on_b ? reinterpret_cast<uintptr_t>(s.scale) : 0);
    const uintptr_t out = reinterpret_cast<uintptr_t>(s.packed) | reinterpret_cast<uintptr_t>(s.phase);
    GI_REQUIRE(!all64 || ((in & 15) == 0 && (out & (dtype == GI_F16 ? 7 : 15)) == 0), "debug_pack_weights_batch: job %d is not aligned for the 64-tile kernel", i);
    PackJob& J = P.j[P.n++];
    J.w = s.w; J.packed = s.packed; J.phase = s.phase; J.ca = s.ca; J.cb = s.cb; J.tile0 = 0; J.scale_on_b = s.scale_on_b; J.scale = s.scale;
  }
  return op_pack_weights_batch(ctx->stream, dtype, P);
}

// ---- the critic head (head.hip) on its own: what tests/test_head_gpu.py drives ---------------------------------------------------
namespace {
// the shape checks shared by the head's forward and backward; *pops = the number of BatchNorm populations the images fall into
int dbg_head_shape(const char* who, int dtype, int n, int Hh, int Wh, int c, int n_per_group, int* pops) {
  GI_REQUIRE(dbg_dtype_ok(dtype), "%s: dtype=%d", who, dtype);
  GI_REQUIRE(n >= 1 && c >= 1 && c % dbg_epc(dtype) == 0, "%s: n=%d c=%d (c a multiple of %d)", who, n, c, dbg_epc(dtype));
  GI_REQUIRE(Hh >= 4 && Wh >= 4, "%s: feature map %dx%d below the 4x4 kernel", who, Hh, Wh);
  GI_REQUIRE(n_per_group >= 0 && (n_per_group == 0 || n % n_per_group == 0), "%s: n_per_group=%d does not divide n=%d", who, n_per_group, n);
  *pops = n_per_group > 0 ? n / n_per_group : 1;
  return GI_OK;
}
}  // namespace

int gi_debug_head_forward(gi_ctx* ctx, int dtype, const gi_head_args* s) {
  GI_REQUIRE(ctx && s && s->a4 && s->w5 && s->wl && s->bl && s->h && s->out, "debug_head_forward: null pointer");
  int pops = 1;
  GI_TRY(dbg_head_shape("debug_head_forward", dtype, s->n, s->Hh, s->Wh, s->c, s->n_per_group, &pops));
  GI_REQUIRE((s->scale4 == nullptr) == (s->shift4 == nullptr), "debug_head_forward: scale4 and shift4 go together");
  GI_REQUIRE(!s->scale4 || pops == 1 || (pops == 2 && s->gstride >= s->c), "debug_head_forward: %d populations, gstride=%d for %d channels", pops,
             s->gstride, s->c);
  GI_REQUIRE(s->tbuf_bytes >= 0 && (s->tbuf_bytes == 0 || s->tbuf), "debug_head_forward: tbuf_bytes=%lld without tbuf", (long long)s->tbuf_bytes);
  HeadArgs a;
  a.a4 = s->a4; a.w5 = s->w5; a.wl = s->wl; a.bl = s->bl; a.h = s->h; a.out = s->out;
  a.n = s->n; a.Hh = s->Hh; a.Wh = s->Wh; a.c = s->c; a.sigmoid = s->sigmoid; a.out2 = s->out2;
  a.scale4 = s->scale4; a.shift4 = s->shift4; a.n_per_group = s->n_per_group; a.gstride = s->gstride;
  a.tbuf = s->tbuf_bytes > 0 ? s->tbuf : nullptr; a.tbuf_bytes = s->tbuf_bytes;
  BnAccArgs bn;
  if (s->bn) {
    GI_TRY(dbg_bn_acc("debug_head_forward", s->c, s->bn, bn));
    GI_REQUIRE(bn.groups == pops, "debug_head_forward: %d accumulator populations for %d populations of images", bn.groups, pops);
    a.bn = &bn;
  }
  return op_head_forward(ctx->stream, dtype, a);
}

int gi_debug_head_backward(gi_ctx* ctx, int dtype, gi_head_bwd_args* s) {
  GI_REQUIRE(ctx && s && s->w5 && s->wl && s->h && s->out && s->dy && s->da4, "debug_head_backward: null pointer");
  GI_REQUIRE(s->dh, "debug_head_backward: dh is missing (the generic kernels write it)");
  s->bwd_applied = 0;
  int pops = 1, bpops = 1;
  GI_TRY(dbg_head_shape("debug_head_backward", dtype, s->n, s->Hh, s->Wh, s->c, s->n_per_group, &pops));
  GI_REQUIRE(!s->dw5 || (s->dwl && s->a4), "debug_head_backward: dw5 without dwl / a4");
  GI_REQUIRE((s->scale4 == nullptr) == (s->shift4 == nullptr), "debug_head_backward: scale4 and shift4 go together");
  GI_REQUIRE(!s->scale4 || pops == 1 || (pops == 2 && s->gstride >= s->c), "debug_head_backward: %d populations, gstride=%d for %d channels", pops,
             s->gstride, s->c);
  GI_REQUIRE(s->scratch_bytes >= 0 && (s->scratch_bytes == 0 || s->scratch), "debug_head_backward: scratch_bytes=%lld without scratch",
             (long long)s->scratch_bytes);
  if (s->bwd_acc) {
    GI_REQUIRE(s->bwd_x && s->bwd_scale && s->bwd_shift && s->bwd_mean && s->bwd_inv, "debug_head_backward: bwd_acc without x / scale / shift / mean / inv");
    GI_REQUIRE(s->bwd_reps >= 1 && s->bwd_reps <= GI_STAT_MAXREP && gi_is_pow2(s->bwd_reps), "debug_head_backward: bwd_reps=%d (1, 2 or %d)", s->bwd_reps,
               GI_STAT_MAXREP);
    GI_TRY(dbg_head_shape("debug_head_backward", dtype, s->n, s->Hh, s->Wh, s->c, s->bwd_n_per_group, &bpops));
    GI_REQUIRE(bpops == 1 || (bpops == 2 && s->bwd_stride >= s->c), "debug_head_backward: %d populations, bwd_stride=%d for %d channels", bpops,
               s->bwd_stride, s->c);
  }
  HeadBwdArgs a;
  a.a4 = s->a4; a.w5 = s->w5; a.wl = s->wl; a.h = s->h; a.out = s->out; a.dy = s->dy; a.da4 = s->da4;
  a.dw5 = s->dw5; a.dwl = s->dwl; a.dbl = s->dbl; a.dh = s->dh;
  a.n = s->n; a.Hh = s->Hh; a.Wh = s->Wh; a.c = s->c; a.sigmoid = s->sigmoid; a.loss_scale = s->loss_scale;
  a.scratch = s->scratch_bytes > 0 ? s->scratch : nullptr; a.scratch_bytes = s->scratch_bytes;
  a.scale4 = s->scale4; a.shift4 = s->shift4; a.n_per_group = s->n_per_group; a.gstride = s->gstride;
  a.bwd_x = s->bwd_x; a.bwd_scale = s->bwd_scale; a.bwd_shift = s->bwd_shift; a.bwd_mean = s->bwd_mean; a.bwd_inv = s->bwd_inv;
  a.bwd_stride = s->bwd_stride; a.bwd_n_per_group = s->bwd_n_per_group; a.bwd_reps = s->bwd_reps; a.bwd_slope = s->bwd_slope;
  a.bwd_acc = s->bwd_acc; a.bwd_applied = &s->bwd_applied;
  return op_head_backward(ctx->stream, dtype, a);
}

int64_t gi_debug_head_scratch_bytes(int max_n, int Hh, int Wh) { return op_head_scratch_bytes(max_n, Hh, Wh); }

int gi_pack_weights(gi_ctx* ctx, int dtype, const float* w, int ca, int cb, void* w_packed, void* w_phase) {
  GI_REQUIRE(ctx && w, "pack_weights: null pointer");
  return op_pack_weights(ctx->stream, dtype, w, ca, cb, w_packed, w_phase);
}
int gi_convert(gi_ctx* ctx, int dtype, const float* src, void* dst, int64_t count) {
  GI_REQUIRE(ctx && src && dst, "convert: null pointer");
  return op_convert(ctx->stream, dtype, src, dst, count);
}
int gi_convert_back(gi_ctx* ctx, int dtype, const void* src, float* dst, int64_t count) {
  GI_REQUIRE(ctx && src && dst, "convert_back: null pointer");
  return op_convert_back(ctx->stream, dtype, src, dst, count);
}

int gi_time_convT_s2(gi_ctx* ctx, int dtype, const void* in, const void* w_phase, void* out, int n, int H, int W, int ca, int ldin, int cb,
                     int ldout, int iters, float* ms_out_host) {
  GI_REQUIRE(ctx && ms_out_host && iters > 0, "time_convT_s2: bad argument");
  hipEvent_t e0, e1;
  GI_HIP(hipEventCreate(&e0));
  GI_HIP(hipEventCreate(&e1));
  const int relu = gi_tune("GI_TIME_RELU", 1);   // (ablation build: 0 times the variant without the fused input ReLU)
  // warm-up
  GI_TRY(gi_convT_s2_forward(ctx, dtype, in, w_phase, out, n, H, W, ca, ldin, cb, ldout, relu, GI_ACT_NONE, nullptr, 0));
  GI_HIP(hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < iters; ++i)
    GI_TRY(gi_convT_s2_forward(ctx, dtype, in, w_phase, out, n, H, W, ca, ldin, cb, ldout, relu, GI_ACT_NONE, nullptr, 0));
  GI_HIP(hipEventRecord(e1, ctx->stream));
  GI_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  GI_HIP(hipEventElapsedTime(&ms, e0, e1));
  *ms_out_host = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return GI_OK;
}

/* the same for the strided convolution (gi_conv_s2_forward): the critic's conv2 / the generator's d2 family */
int gi_time_conv_s2(gi_ctx* ctx, int dtype, const void* in, const void* w_packed, void* out, int n, int H, int W, int cb, int ldin, int ca,
                    int ldout, int iters, float* ms_out_host) {
  GI_REQUIRE(ctx && ms_out_host && iters > 0, "time_conv_s2: bad argument");
  hipEvent_t e0, e1;
  GI_HIP(hipEventCreate(&e0));
  GI_HIP(hipEventCreate(&e1));
  GI_TRY(gi_conv_s2_forward(ctx, dtype, in, w_packed, out, n, H, W, cb, ldin, ca, ldout, 0, GI_ACT_NONE, nullptr, 0));
  GI_HIP(hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < iters; ++i)
    GI_TRY(gi_conv_s2_forward(ctx, dtype, in, w_packed, out, n, H, W, cb, ldin, ca, ldout, 0, GI_ACT_NONE, nullptr, 0));
  GI_HIP(hipEventRecord(e1, ctx->stream));
  GI_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  GI_HIP(hipEventElapsedTime(&ms, e0, e1));
  *ms_out_host = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return GI_OK;
}

}  // extern "C"
