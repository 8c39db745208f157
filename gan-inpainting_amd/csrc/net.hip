// Host-side schedules: which kernels run, in which order, on which buffers, for
//   UnetGenerator      (lib/models/networks.py:216-324)  forward + backward
//   PatchGANDiscriminator (networks.py:331-363)          forward + backward
// (DCGANDiscriminator, networks.py:162-212, keeps its own state and schedule in dcgan.hip behind gi_net::dc)
// Data layout in HBM (per activation slot): NHWC tensors of the compute type T; for every U-Net
// level k one "concat buffer" C[k] = [skip a_k | decoder u_{k+1}] (2*ch_k channels) that both
// producers write at their channel offset, so torch.cat (networks.py:324) never materialises.
#include <string>
#include <vector>
#include <string.h>

#include "common.h"
#include "stat_acc.h"

namespace {

struct TensorDesc {
  std::string name;
  int kind;  // 0 conv weight, 1 contiguous param, 2 running_mean, 3 running_var, 4 plain buffer (spectral norm u / v)
  int64_t shape[4];
  int ndim;
  int64_t offset, numel;
};

struct Conv {            // 4x4 weight [a][16][b] fp32 master at params+w_off
  int ca = 0, cb = 0;
  int64_t w_off = -1, bias_off = -1;
  int64_t packed_off = -1, phase_off = -1;  // workspace offsets of the T copies (-1: b == 1 layer)
  int64_t inf_off = -1;                     // inference: the forward's copy with the following BatchNorm's scale folded in
};
struct BN {
  int c = 0;
  int64_t gamma_off = -1, beta_off = -1, rmean_off = -1, rvar_off = -1;
  int64_t stat_off = -1;  // per-slot: [scale|shift|mean|inv] * c floats (offset inside slot)
  int id = -1;            // index into gi_net::eval_gen
  int64_t inf_off = -1;   // shared workspace: [scale|shift|mean|inv] * c floats of the inference affine map
  // exact-statistics accumulators (stat_acc.h), 64-bit words into the net's region: four blocks of [2 groups][c][4] words,
  // two for the forward statistics and two for the backward reductions. Each use takes the block its parity bit names
  // and its consuming pass clears the other one for the next use (ping-pong): no memset launches.
  int64_t acc_off = -1;
  int64_t in_off = -1;    // InstanceNorm generator: per-slot [n][c][2] mean / inv of the last forward
  mutable int fwd_par = 0, bwd_par = 0;
  mutable int dirty[4] = {0, 0, 0, 0};   // replicas a use has added to in block {fwd 0, fwd 1, bwd 0, bwd 1}, not yet cleared
  int64_t acc_block() const { return gi_stat_block_words(c, GI_STAT_MAXREP); }
};

// BatchNorm-backward reduction fused into the GEMM that produces the gradient (IgemmArgs::bwd_*): fixed BEFORE that GEMM
// runs (the accumulator ping-pong state moves here), consumed by act_bn_bwd, which then launches only its apply pass - or
// both passes on the same accumulator block when the kernel that ran did not take the fusion (`applied` false).
struct BwdFuse {
  bool planned = false, applied = false;
  unsigned long long* acc = nullptr; unsigned long long* zero_next = nullptr;
  int zero_words = 0, reps_gemm = 1, reps_reduce = 1, groups = 1;
  const void* x = nullptr; int ldx = 0;
  const float* scale = nullptr; const float* shift = nullptr; const float* mean = nullptr; const float* inv = nullptr;
  int stride = 0; float slope = 1.f; int64_t pg = 0;
  int c0 = 0, c = 0;   // IgemmArgs::bwd_c0 / bwd_c (0: all output columns)
};

struct Arena {
  int64_t size = 0;
  int64_t take(int64_t bytes) {
    const int64_t o = size;
    size += gi_align_up(bytes < 16 ? 16 : bytes, 256);
    return o;
  }
};

}  // namespace

// DCGANDiscriminator (dcgan.hip): the generic gi_net_* entries below hand a kind-2 handle to these
struct gi_dcgan;
void gi_dcgan_free(gi_dcgan* dc);
int gi_dcgan_sync(gi_dcgan* dc, hipStream_t st, const float* params, char* ws);
int gi_dcgan_forward(gi_dcgan* dc, hipStream_t st, const float* params, char* ws, int slot, const float* x, float* y, int n);
int gi_dcgan_backward(gi_dcgan* dc, hipStream_t st, const float* params, float* grads, char* ws, int slot, const float* dy, float* dx,
                      int need_wgrad, float loss_scale, int phase);
int64_t gi_dcgan_phase_split(gi_dcgan* dc);
int gi_dcgan_saved(gi_dcgan* dc, hipStream_t st, char* ws, int slot, int kind, int level, float* out, int64_t count);

struct gi_net {
  gi_ctx* ctx = nullptr;
  int kind = 0;  // 0 unet, 1 patchgan, 2 dcgan (state in dc)
  gi_dcgan* dc = nullptr;
  int dtype = GI_F32;
  int H = 0, W = 0, max_n = 0, n_slots = 1;
  int train = 1;
  float loss_scale = 1.f;
  uint64_t drop_seed = 0x5EED0000ull, drop_counter = 0;
  // unet
  int nd = 0, ngf = 0;
  int bn_groups = 1;                 // discriminator: the batch holds this many independent BatchNorm groups (stacked real|fake)
  int bwd_eval = 0;                  // (transient) the backward in progress differentiates an eval-mode forward
  int out_c = 1;                     // output channels; > 1: u1 runs on the generic kernels with b zero-padded to 64
  int64_t oU1 = -1, oUp1Pad = -1, oUp1Packed = -1, oUp1Phase = -1;
  float dropout_p = 0.f;
  std::vector<int> ch, Hk, Wk;       // 1-based per level
  std::vector<Conv> conv, up;        // 1-based
  std::vector<BN> dnorm, unorm;      // 1-based (c == 0: absent)
  // patchgan
  int sigmoid = 1;
  Conv dconv[5];                     // 1..4
  BN dbn[5];                         // 2..4
  int64_t w5_off = -1, wl_off = -1, bl_off = -1;
  int P = 0, Hh = 0, Wh = 0;

  std::vector<TensorDesc> tensors;
  int64_t n_params = 0, n_buffers = 0;
  // workspace layout
  Arena arena;
  int64_t slot_bytes = 0, slot_base = 0;
  std::vector<int64_t> oC, oR, oU, oMask;  // per-slot offsets (1-based level)
  int64_t oE = -1, oOut = -1, oX = -1, oStats = -1, oHh = -1;
  int64_t oA[5] = {-1, -1, -1, -1, -1}, oRd[5] = {-1, -1, -1, -1, -1};
  // shared scratch
  std::vector<int64_t> ogC, ogA;
  int64_t ogE = -1, oD = -1, oG0 = -1, oPart = -1, oSums = -1, oSplit = -1, oDh = -1, oCol = -1;
  int64_t part_floats = 0, split_bytes = 0;
  int64_t oHw = -1, hw_bytes = 0;    // head weight-gradient partials
  int64_t oHt = -1, ht_bytes = 0;    // head forward: per-pixel tap products of large feature maps (sliced forward)
  // eval-mode BatchNorm is a fixed affine map of (gamma, beta, running statistics): its scale / shift in a slot stay
  // valid until those change (weights re-synced, a train-mode forward, set_train), tracked by a generation counter
  uint64_t affine_gen = 1;
  uint64_t inf_gen = 0;              // generation the folded inference copies were built at
  int inference = 0;                 // gi_net_set_inference: eval-mode forwards will never be differentiated
  std::vector<int> slot_inference;
  std::vector<std::vector<uint64_t>> eval_gen;   // [slot][BN id]: generation the slot's scale / shift were computed at
  // generator norm layer (get_norm_layer, networks.py:29-45): 0 BatchNorm2d, 1 InstanceNorm2d(affine=False,
  // track_running_stats=False) - every convolution then carries a bias (use_bias, networks.py:270-273) -, 2 none (Identity)
  int norm_kind = 0;
  int64_t oInStats = -1;
  int fuse_head = 1;                 // generator: last decoder level's BatchNorm + ReLU applied inside the head kernels
  std::vector<int> slot_fused_u2;    // per slot: the forward ran that way (the backward must match)
  int64_t oWg = -1, wg_bytes = 0;    // weight-gradient split scratch (deterministic two-stage reduction)
  // GI_WGRAD_STREAM: the weight-gradient GEMMs of a backward (and their fixed-order reduce launches) run on a second HIP stream
  // beside the input-gradient chain, which never reads their result. dz buffers rotate (oDr; oD == oDr[0]) so that the chain
  // does not wait for a weight gradient before it overwrites its operand; gi_net_backward[_phase] joins before it returns.
  int64_t oDr[3] = {-1, -1, -1};
  // per slot: one 64-bit sign word per pixel of the first layer's activation (op_c1_gather), what the fused LeakyReLU backward in
  // the second layer's input-gradient GEMM reads instead of the activation itself (IgemmArgs::mask_bits); slot_bits1: written
  int64_t oBits1 = -1;
  std::vector<int> slot_bits1;
  int64_t oC1w = -1, c1w_floats = 0;   // shared: per-workgroup partial sums of the fused first-layer weight gradient (IgemmArgs::c1w_part)
  hipStream_t st2 = nullptr;
  hipEvent_t ev_dz = nullptr, ev_wg[3] = {nullptr, nullptr, nullptr};
  bool wg_busy[3] = {false, false, false};
  int dz_i = 0;
  bool side = false;                 // (transient) the backward in progress uses st2
  // train-mode BatchNorm statistics without a reduction launch: the GEMM epilogues add their tile sums into exact
  // per-channel accumulators (stat_acc.h), the normalisation pass derives scale / shift from them itself (and the backward
  // reductions likewise). Regions per BatchNorm layer: BN::acc_off; all zero after gi_net_bind, then kept zero by the
  // consuming passes. GI_BN_ACC=0 restores partial rows + finalize / sums launches.
  int64_t oAcc = -1, acc_words = 0;
  int use_acc = 1;
  std::vector<BwdFuse> bwd_pending;  // per BatchNorm id: a reduction planned / done by the producing GEMM, waiting for act_bn_bwd
  int64_t oTickets = -1;             // split-K fix-up counters (IgemmArgs::tickets): zero at bind, zero after every launch
  // gradient-penalty scratch (patchgan): stacked 2n tensors, see patchgan_gradient_penalty
  int64_t oA2[5] = {-1, -1, -1, -1, -1}, oG2[5] = {-1, -1, -1, -1, -1}, oTX[5] = {-1, -1, -1, -1, -1};
  int64_t oD2 = -1, oTZ = -1, oGimg = -1, oVimg = -1, oGPs = -1, oGPpart = -1, oGPsums = -1, oTh = -1;
  int64_t oGPgrad = -1;              // n_params floats: the penalty's parameter gradients at tangent scale, before the 1/s add
  int gp_slot = -1;
  // spectral normalisation (patchgan, gi_patchgan_create_sn; specnorm.hip). The kernels of a forward / backward read the EFFECTIVE
  // parameters (oSnEff: the six weights divided by their sigma, everything else copied) because `params` points there for the
  // duration (ParamsBack); `master` keeps the bound buffer. A backward writes gradients with respect to the effective weights into
  // oSnGrad and sn_project folds them into the bound ones. Per slot (oSnSlot): the u | v the forward ended with, then its six sigma.
  int sn = 0, sn_iters = 1;
  struct SnTensor { int64_t off = 0, u_off = 0, v_off = 0, scratch = 0; int ca = 0, K = 0, cb = 0; } snt[6];
  int64_t oSnEff = -1, oSnGrad = -1, oSnSlot = -1;
  int64_t sn_uv_off = 0, sn_uv_floats = 0;   // the u / v buffers: one contiguous range of the flat buffer allocation
  uint64_t sn_gen = 0, sn_eff_gen = 0;       // forwards so far; the forward whose sigma the effective (and packed) copies hold
  std::vector<uint64_t> slot_sn_gen;
  float* master = nullptr;
  std::vector<int> slot_n, slot_train, slot_groups;
  std::vector<std::vector<const uint8_t*>> ext_mask;  // [slot][level]

  float* params = nullptr;
  float* grads = nullptr;
  float* buffers = nullptr;
  char* ws = nullptr;
  bool bound = false;

  size_t tsz() const { return gi_dtype_size(dtype); }
  char* slot(int s, int64_t off) const { return ws + slot_base + (int64_t)s * slot_bytes + off; }
  char* shared(int64_t off) const { return ws + off; }
};

namespace {

void add_tensor(gi_net* net, const std::string& name, int kind, std::initializer_list<int64_t> shape, int64_t* off_out) {
  TensorDesc t;
  t.name = name;
  t.kind = kind;
  t.ndim = (int)shape.size();
  t.numel = 1;
  int i = 0;
  for (int64_t s : shape) { t.shape[i++] = s; t.numel *= s; }
  for (; i < 4; ++i) t.shape[i] = 1;
  int64_t& ctr = (kind <= 1) ? net->n_params : net->n_buffers;
  t.offset = ctr;
  ctr += gi_align_up(t.numel, 64);
  *off_out = t.offset;
  net->tensors.push_back(t);
}

void add_bn(gi_net* net, const std::string& prefix, BN& bn, int c, std::vector<std::pair<std::string, BN*>>& later) {
  bn.c = c;
  add_tensor(net, prefix + ".weight", 1, {c}, &bn.gamma_off);
  add_tensor(net, prefix + ".bias", 1, {c}, &bn.beta_off);
  later.push_back({prefix, &bn});
}

int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// upper bound on partial-statistics rows any kernel may write for a (pixels, c) tensor
int64_t part_rows(int64_t pixels) { return max64(pixels / 64 + 8, 1100); }

}  // namespace

// =================================================================================================
// creation
// =================================================================================================
extern "C" int gi_unet_create_padded(gi_ctx* ctx, int num_downs, int ngf, int ch1, int out_c, int norm_kind, float dropout_p, int H, int W,
                                     int max_n, int dtype, int n_slots, gi_net** out) {
  GI_REQUIRE(out, "unet_create: null argument");  // ctx may be null: inventory-only handle
  GI_REQUIRE(norm_kind >= 0 && norm_kind <= 2, "unet_create: norm_kind=%d (0 batch, 1 instance, 2 none)", norm_kind);
  GI_REQUIRE(ch1 == 0 || (ch1 >= ngf && ch1 % 64 == 0), "unet_create: ch1=%d must be 0 or a multiple of 64 >= ngf", ch1);
  GI_REQUIRE(dtype == GI_F16 || dtype == GI_F32, "unet_create: dtype=%d", dtype);
  GI_REQUIRE(num_downs >= 5 && num_downs <= 9, "unet_create: num_downs=%d (supported 5..9)", num_downs);
  // the GEMM kernels take channel counts that are multiples of 64: every level must qualify. ngf = 32 does from level 2 on
  // (64, 128, 256, ...); its level 1 is then computed ch1 = 64 channels wide with the upper half zero (gi_unet_create_padded)
  if (ctx) GI_REQUIRE(ngf >= 32 && (2 * ngf) % 64 == 0 && ((ch1 ? ch1 : ngf) % 64 == 0),
                      "unet_create: ngf=%d ch1=%d: every level needs a multiple of 64 channels (ngf a multiple of 64, or of 32 with ch1)", ngf, ch1);
  else GI_REQUIRE(ngf % 8 == 0 && ngf >= 8, "unet_create: ngf=%d must be a multiple of 8 (inventory-only handle)", ngf);
  GI_REQUIRE(out_c >= 1 && out_c <= 64, "unet_create: out_c=%d (1..64)", out_c);
  // (powers of two take the halo-resident kernels; other multiples of 2^num_downs - 192, 384 - fall back to the gather kernels)
  GI_REQUIRE(H >= (1 << num_downs) && W >= (1 << num_downs) && H % (1 << num_downs) == 0 && W % (1 << num_downs) == 0,
             "unet_create: H=%d W=%d must be multiples of 2^num_downs = %d", H, W, 1 << num_downs);
  GI_REQUIRE(max_n >= 1 && n_slots >= 1 && n_slots <= 8, "unet_create: max_n=%d n_slots=%d", max_n, n_slots);
  gi_net* net = new gi_net();
  net->ctx = ctx; net->kind = 0; net->dtype = dtype; net->H = H; net->W = W; net->max_n = max_n; net->n_slots = n_slots;
  net->nd = num_downs; net->ngf = ngf; net->dropout_p = dropout_p; net->out_c = out_c; net->norm_kind = norm_kind;
  net->loss_scale = dtype == GI_F16 ? 65536.f : 1.f;
  const int nd = num_downs;
  net->ch.assign(nd + 1, 0); net->Hk.assign(nd + 1, 0); net->Wk.assign(nd + 1, 0);
  net->conv.assign(nd + 1, Conv()); net->up.assign(nd + 1, Conv());
  net->dnorm.assign(nd + 1, BN()); net->unorm.assign(nd + 1, BN());
  for (int k = 1; k <= nd; ++k) {
    int m = 1 << (k - 1);
    if (m > 8) m = 8;
    net->ch[k] = (k == 1 && ch1) ? ch1 : ngf * m;
    net->Hk[k] = H >> k;
    net->Wk[k] = W >> k;
  }
  // parameters in the reference's named_parameters() order (recursive nesting, networks.py:296-318)
  std::vector<std::pair<std::string, BN*>> bns;
  std::vector<std::string> prefix(nd + 2);
  prefix[1] = "model.model";
  struct Emit {
    gi_net* net; int nd; std::vector<std::string>& prefix; std::vector<std::pair<std::string, BN*>>& bns;
    void run(int k) {
      const std::string& p = prefix[k];
      const bool outer = (k == 1), inner = (k == nd);
      const std::string down = p + (outer ? ".0" : ".1");
      const std::string upn = p + ((outer || inner) ? ".3" : ".5");
      Conv& cv = net->conv[k];
      cv.ca = net->ch[k]; cv.cb = outer ? 1 : net->ch[k - 1];
      const bool inorm = net->norm_kind == 1;
      add_tensor(net, down + ".weight", 0, {cv.ca, cv.cb, 4, 4}, &cv.w_off);
      if (inorm) add_tensor(net, down + ".bias", 1, {cv.ca}, &cv.bias_off);
      if (!outer && !inner) {
        if (net->norm_kind == 0) add_bn(net, p + ".2", net->dnorm[k], net->ch[k], bns);
        else net->dnorm[k].c = net->ch[k];     // parameter-free (or absent) norm: only the channel count
      }
      if (!inner) {
        prefix[k + 1] = p + (outer ? ".1" : ".3") + ".model";
        run(k + 1);
      }
      Conv& uv = net->up[k];
      uv.ca = inner ? net->ch[k] : 2 * net->ch[k];
      uv.cb = outer ? net->out_c : net->ch[k - 1];
      add_tensor(net, upn + ".weight", 0, {uv.ca, uv.cb, 4, 4}, &uv.w_off);
      if (outer || inorm) add_tensor(net, upn + ".bias", 1, {uv.cb}, &uv.bias_off);
      if (!outer) {
        if (net->norm_kind == 0) add_bn(net, p + (inner ? ".4" : ".6"), net->unorm[k], net->ch[k - 1], bns);
        else net->unorm[k].c = net->ch[k - 1];
      }
    }
  } emit{net, nd, prefix, bns};
  emit.run(1);
  for (auto& pb : bns) {
    add_tensor(net, pb.first + ".running_mean", 2, {pb.second->c}, &pb.second->rmean_off);
    add_tensor(net, pb.first + ".running_var", 3, {pb.second->c}, &pb.second->rvar_off);
  }

  // ---- workspace layout
  const int64_t T = (int64_t)net->tsz();
  Arena& A = net->arena;
  for (int k = 2; k <= nd; ++k) {
    for (Conv* c : {&net->conv[k], &net->up[k]}) {
      const int64_t cnt = (int64_t)c->ca * 16 * c->cb;
      c->packed_off = (dtype == GI_F32) ? -2 : A.take(cnt * T);  // fp32: the master itself is [a][16*b]
      c->phase_off = A.take(cnt * T);
    }
  }
  for (int k = 2; k <= nd; ++k) {   // inference copies: conv in its packed form, transposed conv in its phase form
    if (k < nd) { net->conv[k].inf_off = A.take((int64_t)net->conv[k].ca * 16 * net->conv[k].cb * T); net->dnorm[k].inf_off = A.take(4 * net->dnorm[k].c * 4); }
    net->up[k].inf_off = A.take((int64_t)net->up[k].ca * 16 * net->up[k].cb * T);
    net->unorm[k].inf_off = A.take(4 * net->unorm[k].c * 4);
  }
  const int64_t N = max_n;
  net->ogC.assign(nd + 1, -1); net->ogA.assign(nd + 1, -1);
  int64_t maxD = 0, maxPart = 0, maxSplit = 0, maxc = 0;
  for (int k = 1; k <= nd - 1; ++k) {
    const int64_t pix = N * net->Hk[k] * net->Wk[k];
    net->ogC[k] = A.take(pix * 2 * net->ch[k] * T);
    net->ogA[k] = A.take(pix * net->ch[k] * T);
    maxD = max64(maxD, pix * net->ch[k] * T);
    maxPart = max64(maxPart, part_rows(pix) * 2 * 2 * net->ch[k]);
    maxc = max64(maxc, 2 * net->ch[k]);
    if (pix <= 32768) maxSplit = max64(maxSplit, pix * 2 * net->ch[k] * 4);
  }
  {
    const int64_t pix = N * net->Hk[nd] * net->Wk[nd];
    net->ogE = A.take(pix * net->ch[nd] * T);
    maxD = max64(maxD, pix * net->ch[nd] * T);
    maxSplit = max64(maxSplit, pix * net->ch[nd] * 4);
  }
  net->oD = net->oDr[0] = A.take(maxD);
  net->oDr[1] = A.take(maxD);
  net->oDr[2] = A.take(maxD);
  if (nd >= 2) {   // workgroups of d2's input-gradient GEMM (256-pixel patches of level 2, two py phases) x 64 x 16 sums
    net->c1w_floats = ((N * net->Hk[2] * net->Wk[2] / 256 + 8) * 2 + 64) * 1024;   // + 64 rows: op_c1_wgrad_reduce's first stage
    net->oC1w = A.take(net->c1w_floats * 4);
  }
  net->oG0 = A.take(N * H * W * 4 * out_c);
  if (out_c > 1) {   // u1 on the generic kernels: weights [a][16][b] with b zero-padded to 64, NHWC staging buffer
    const int64_t cnt = (int64_t)2 * net->ch[1] * 16 * 64;
    net->oUp1Pad = A.take(cnt * 4);
    net->oUp1Packed = (dtype == GI_F32) ? -2 : A.take(cnt * T);
    net->oUp1Phase = A.take(cnt * T);
    net->oU1 = A.take(N * H * W * 64 * T);
  }
  net->oCol = A.take(N * (H / 2) * (W / 2) * 16 * 2 * (out_c == 4 ? 4 : 1));   // (x4: the 4-channel head's col buffer)
  net->part_floats = maxPart;
  net->oPart = A.take(maxPart * 4);
  net->oSums = A.take(8 * maxc * 4);   // [8][c]: sums + apply coefficients
  // split-K scratch: one fp32 buffer per split (split x output ~ 384 tiles of 128 x 128) for the deterministic path
  if (maxSplit > 0) maxSplit = max64(maxSplit, (int64_t)400 * 128 * 128 * 4);
  net->split_bytes = maxSplit;
  net->oSplit = A.take(maxSplit);
  for (int k = 2; k <= nd; ++k) {
    net->wg_bytes = max64(net->wg_bytes, op_wgrad_scratch_bytes(dtype, max_n, net->Hk[k], net->Wk[k], net->conv[k].ca, net->conv[k].cb));
    net->wg_bytes = max64(net->wg_bytes, op_wgrad_scratch_bytes(dtype, max_n, net->Hk[k], net->Wk[k], net->up[k].ca, net->up[k].cb));
  }
  if (net->wg_bytes > 0) net->oWg = A.take(net->wg_bytes);
  // per-slot
  Arena S;
  net->oC.assign(nd + 1, -1); net->oR.assign(nd + 1, -1); net->oU.assign(nd + 1, -1); net->oMask.assign(nd + 1, -1);
  for (int k = 1; k <= nd - 1; ++k) net->oC[k] = S.take(N * net->Hk[k] * net->Wk[k] * 2 * net->ch[k] * T);
  for (int k = 2; k <= nd - 1; ++k) net->oR[k] = S.take(N * net->Hk[k] * net->Wk[k] * net->ch[k] * T);
  net->oE = S.take(N * net->Hk[nd] * net->Wk[nd] * net->ch[nd] * T);
  for (int k = 2; k <= nd; ++k) net->oU[k] = S.take(N * net->Hk[k - 1] * net->Wk[k - 1] * net->ch[k - 1] * T);
  for (int k = 5; k <= nd - 1; ++k) net->oMask[k] = S.take(N * net->Hk[k - 1] * net->Wk[k - 1] * net->ch[k - 1]);
  net->oOut = S.take(N * H * W * 4 * out_c);
  net->oX = S.take(N * H * W * 4);
  net->oBits1 = S.take(N * net->Hk[1] * net->Wk[1] * 8 + 16);
  int64_t stat_floats = 0;
  int nbn = 0;
  for (int k = 1; k <= nd; ++k)
    for (BN* b : {&net->dnorm[k], &net->unorm[k]})
      if (b->c) { b->stat_off = stat_floats; stat_floats += 4 * b->c; b->id = nbn++; }
  net->oStats = S.take(stat_floats * 4);
  if (norm_kind == 1) {
    int64_t in_floats = 0;
    for (int k = 1; k <= nd; ++k)
      for (BN* b : {&net->dnorm[k], &net->unorm[k]})
        if (b->c) { b->in_off = in_floats; in_floats += 2 * N * b->c; }
    net->oInStats = S.take(in_floats * 4);
  }
  net->slot_bytes = S.size;
  net->slot_base = A.take(S.size * n_slots);
  for (int k = 1; k <= nd; ++k)
    for (BN* b : {&net->dnorm[k], &net->unorm[k]})
      if (b->c && norm_kind == 0) { b->acc_off = net->acc_words; net->acc_words += 4 * b->acc_block(); }
  net->oAcc = A.take(net->acc_words * 8);
  net->oTickets = A.take((int64_t)GI_IGEMM_TICKETS * 4);
  net->use_acc = gi_opt(GI_OPT_BN_ACC);   // GI_BN_ACC=0: partial rows + finalize / sums launches
  net->slot_n.assign(n_slots, 0);
  net->slot_train.assign(n_slots, 0);
  net->slot_fused_u2.assign(n_slots, 0);
  net->slot_bits1.assign(n_slots, 0);
  net->slot_inference.assign(n_slots, 0);
  net->eval_gen.assign(n_slots, std::vector<uint64_t>(nbn, 0));
  net->bwd_pending.assign(nbn, BwdFuse());
  net->fuse_head = gi_opt(GI_OPT_FUSE_HEAD);   // GI_FUSE_HEAD=0: materialise the last decoder level
  net->ext_mask.assign(n_slots, std::vector<const uint8_t*>(nd + 1, nullptr));
  *out = net;
  return GI_OK;
}

extern "C" int gi_unet_create_norm(gi_ctx* ctx, int num_downs, int ngf, int out_c, int norm_kind, float dropout_p, int H, int W,
                                   int max_n, int dtype, int n_slots, gi_net** out) {
  return gi_unet_create_padded(ctx, num_downs, ngf, 0, out_c, norm_kind, dropout_p, H, W, max_n, dtype, n_slots, out);
}

extern "C" int gi_unet_create_ex(gi_ctx* ctx, int num_downs, int ngf, int out_c, float dropout_p, int H, int W, int max_n,
                                 int dtype, int n_slots, gi_net** out) {
  return gi_unet_create_norm(ctx, num_downs, ngf, out_c, 0, dropout_p, H, W, max_n, dtype, n_slots, out);
}

extern "C" int gi_unet_create(gi_ctx* ctx, int num_downs, int ngf, float dropout_p, int H, int W, int max_n, int dtype,
                              int n_slots, gi_net** out) {
  return gi_unet_create_ex(ctx, num_downs, ngf, 1, dropout_p, H, W, max_n, dtype, n_slots, out);
}

extern "C" int gi_patchgan_create_sn(gi_ctx* ctx, int H, int W, int sigmoid, int spectral_norm, int n_power_iterations, int max_n, int dtype,
                                    int n_slots, gi_net** out) {
  GI_REQUIRE(out, "patchgan_create: null argument");  // ctx may be null: inventory-only handle
  GI_REQUIRE(!spectral_norm || n_power_iterations >= 1, "patchgan_create: n_power_iterations=%d", n_power_iterations);
  GI_REQUIRE(dtype == GI_F16 || dtype == GI_F32, "patchgan_create: dtype=%d", dtype);
  GI_REQUIRE(H >= 64 && W >= 64 && H % 16 == 0 && W % 16 == 0, "patchgan_create: H=%d W=%d must be multiples of 16, >= 64", H, W);
  GI_REQUIRE(max_n >= 1 && n_slots >= 1 && n_slots <= 8, "patchgan_create: max_n=%d n_slots=%d", max_n, n_slots);
  gi_net* net = new gi_net();
  net->ctx = ctx; net->kind = 1; net->dtype = dtype; net->H = H; net->W = W; net->max_n = max_n; net->n_slots = n_slots;
  net->sigmoid = sigmoid;
  net->sn = spectral_norm ? 1 : 0; net->sn_iters = n_power_iterations;
  net->loss_scale = dtype == GI_F16 ? 65536.f : 1.f;
  net->Hh = H / 16; net->Wh = W / 16;
  net->P = (net->Hh - 3) * (net->Wh - 3);
  const int chans[5] = {1, 64, 128, 256, 512};
  const int conv_idx[5] = {0, 0, 2, 5, 8};
  const int bn_idx[5] = {0, 0, 3, 6, 9};
  const std::string wname = net->sn ? ".weight_orig" : ".weight";
  std::vector<std::pair<std::string, BN*>> bns;
  for (int i = 1; i <= 4; ++i) {
    Conv& c = net->dconv[i];
    c.ca = chans[i]; c.cb = chans[i - 1];
    add_tensor(net, "model." + std::to_string(conv_idx[i]) + wname, 0, {c.ca, c.cb, 4, 4}, &c.w_off);
    if (i >= 2) add_bn(net, "model." + std::to_string(bn_idx[i]), net->dbn[i], chans[i], bns);
  }
  add_tensor(net, "model.11" + wname, 0, {1, 512, 4, 4}, &net->w5_off);
  add_tensor(net, "model.13" + wname, 1, {1, net->P}, &net->wl_off);
  add_tensor(net, "model.13.bias", 1, {1}, &net->bl_off);
  for (auto& pb : bns) {
    add_tensor(net, pb.first + ".running_mean", 2, {pb.second->c}, &pb.second->rmean_off);
    add_tensor(net, pb.first + ".running_var", 3, {pb.second->c}, &pb.second->rvar_off);
  }
  if (net->sn) {   // the normalised tensors as ca x K matrices, and their u / v buffers (torch's names)
    const int layer[6] = {0, 2, 5, 8, 11, 13};
    for (int t = 0; t < 6; ++t) {
      gi_net::SnTensor& T = net->snt[t];
      if (t < 4) { T.off = net->dconv[t + 1].w_off; T.ca = chans[t + 1]; T.cb = chans[t]; T.K = 16 * T.cb; }
      else if (t == 4) { T.off = net->w5_off; T.ca = 1; T.cb = 512; T.K = 8192; }
      else { T.off = net->wl_off; T.ca = 1; T.cb = 0; T.K = net->P; }
      const std::string base = "model." + std::to_string(layer[t]);
      add_tensor(net, base + ".weight_u", 4, {T.ca}, &T.u_off);
      add_tensor(net, base + ".weight_v", 4, {T.K}, &T.v_off);
    }
    net->sn_uv_off = net->snt[0].u_off;
    net->sn_uv_floats = net->n_buffers - net->sn_uv_off;
  }
  const int64_t T = (int64_t)net->tsz();
  Arena& A = net->arena;
  for (int i = 2; i <= 4; ++i) {
    Conv& c = net->dconv[i];
    const int64_t cnt = (int64_t)c.ca * 16 * c.cb;
    c.packed_off = (dtype == GI_F32) ? -2 : A.take(cnt * T);
    c.phase_off = A.take(cnt * T);
  }
  const int64_t N = max_n;
  int64_t maxD = 0, maxPart = 0, maxSplit = 0;
  net->ogA.assign(5, -1);
  for (int i = 1; i <= 4; ++i) {
    const int64_t pix = N * (H >> i) * (W >> i);
    net->ogA[i] = A.take(pix * chans[i] * T);
    maxD = max64(maxD, pix * chans[i] * T);
    maxPart = max64(maxPart, part_rows(pix) * 2 * chans[i] * 3);   // x3: room for the per-group column pass (BN groups)
    if (pix <= 32768) maxSplit = max64(maxSplit, pix * chans[i] * 4);
  }
  net->oD = net->oDr[0] = A.take(maxD);
  net->oDr[1] = A.take(maxD);
  net->oDr[2] = A.take(maxD);
  net->c1w_floats = ((N * (H >> 2) * (W >> 2) / 256 + 8) * 2 + 64) * 1024;   // + 64 rows: op_c1_wgrad_reduce's first stage
  net->oC1w = A.take(net->c1w_floats * 4);
  net->part_floats = maxPart;
  net->oPart = A.take(maxPart * 4);
  net->oSums = A.take(2 * 8 * 512 * 4);   // [groups][8][c]: sums + apply coefficients
  if (maxSplit > 0) maxSplit = max64(maxSplit, (int64_t)400 * 128 * 128 * 4);
  net->split_bytes = maxSplit;
  net->oSplit = A.take(maxSplit > 0 ? maxSplit : 16);
  for (int i = 2; i <= 4; ++i)   // 2 * max_n: the gradient penalty's stacked weight gradients (fixed-order split reduction there too)
    for (int m : {max_n, 2 * max_n})
      net->wg_bytes = max64(net->wg_bytes, op_wgrad_scratch_bytes(dtype, m, H >> i, W >> i, net->dconv[i].ca, net->dconv[i].cb));
  if (net->wg_bytes > 0) net->oWg = A.take(net->wg_bytes);
  net->oDh = A.take(N * net->P * 4);
  net->hw_bytes = op_head_scratch_bytes((int)N, net->Hh, net->Wh);
  net->oHw = A.take(net->hw_bytes);
  if (net->Hh * net->Wh > 256) { net->ht_bytes = N * net->Hh * net->Wh * 16 * 4; net->oHt = A.take(net->ht_bytes); }
  net->oCol = A.take(N * (H / 2) * (W / 2) * 16 * 2);
  {   // gradient penalty: tangent / stacked-gradient tensors (compute type), its private gradient buffer
    int64_t maxl = 0;
    for (int i = 1; i <= 4; ++i) {
      const int64_t e = N * (H >> i) * (W >> i) * chans[i] * T;
      net->oA2[i] = A.take(2 * e);
      net->oG2[i] = A.take(2 * e);
      net->oTX[i] = A.take(e);
      maxl = max64(maxl, e);
    }
    net->oD2 = A.take(2 * maxl);
    net->oTZ = A.take(maxl);
    net->oGimg = A.take(N * H * W * 4);
    net->oVimg = A.take(N * H * W * 4);
    net->oGPs = A.take((N + 16) * 4 * 4);   // ones | sumsq | amax | tangent scale s, 1/s
    net->oGPgrad = A.take(net->n_params * 4);
    net->oGPpart = A.take((int64_t)1100 * 5 * 512 * 4);
    net->oGPsums = A.take(5 * 512 * 4);
    net->oTh = A.take(N * net->P * 4 * 2);
  }
  if (net->sn) {
    net->oSnEff = A.take(net->n_params * 4);
    net->oSnGrad = A.take(net->n_params * 4);
    for (gi_net::SnTensor& t : net->snt) t.scratch = A.take(op_sn_scratch_floats(t.ca, t.K) * 4);
  }
  Arena S;
  if (net->sn) net->oSnSlot = S.take((net->sn_uv_floats + 64) * 4);
  for (int i = 1; i <= 4; ++i) net->oA[i] = S.take(N * (H >> i) * (W >> i) * chans[i] * T);
  for (int i = 2; i <= 4; ++i) net->oRd[i] = S.take(N * (H >> i) * (W >> i) * chans[i] * T);
  net->oHh = S.take(N * net->P * 4);
  net->oOut = S.take(N * 4);
  net->oX = S.take(N * H * W * 4);
  net->oBits1 = S.take(N * (H >> 1) * (W >> 1) * 8 + 16);
  int64_t stat_floats = 0;
  for (int i = 2; i <= 4; ++i) { net->dbn[i].stat_off = stat_floats; stat_floats += 2 * 4 * net->dbn[i].c; net->dbn[i].id = i - 2; }   // x2: BN groups
  net->eval_gen.assign(n_slots + 1, std::vector<uint64_t>(3, 0));
  net->bwd_pending.assign(3, BwdFuse());
  net->oStats = S.take(stat_floats * 4);
  net->slot_bytes = S.size;
  for (int i = 2; i <= 4; ++i) { net->dbn[i].acc_off = net->acc_words; net->acc_words += 4 * net->dbn[i].acc_block(); }
  net->oAcc = A.take(net->acc_words * 8);
  net->oTickets = A.take((int64_t)GI_IGEMM_TICKETS * 4);
  net->use_acc = gi_opt(GI_OPT_BN_ACC);   // GI_BN_ACC=0: partial rows + finalize / sums launches
  net->gp_slot = n_slots;                      // one private activation set for the gradient penalty
  net->slot_base = A.take(S.size * (n_slots + 1));
  net->slot_n.assign(n_slots + 1, 0);
  net->slot_train.assign(n_slots + 1, 0);
  net->slot_fused_u2.assign(n_slots + 1, 0);
  net->slot_bits1.assign(n_slots + 1, 0);
  net->fuse_head = gi_opt(GI_OPT_FUSE_HEAD);
  net->slot_groups.assign(n_slots + 1, 1);
  net->slot_sn_gen.assign(n_slots + 1, 0);
  *out = net;
  return GI_OK;
}

extern "C" int gi_patchgan_create(gi_ctx* ctx, int H, int W, int sigmoid, int max_n, int dtype, int n_slots, gi_net** out) {
  return gi_patchgan_create_sn(ctx, H, W, sigmoid, 0, 1, max_n, dtype, n_slots, out);
}

// a kind-2 handle for gi_dcgan_create (dcgan.hip): inventory entries through gi_net_add_param, workspace size from dcgan.hip
gi_net* gi_net_new_dcgan(gi_ctx* ctx, int dtype, int max_n, int n_slots, gi_dcgan* dc) {
  gi_net* net = new gi_net();
  net->ctx = ctx; net->kind = 2; net->dc = dc; net->dtype = dtype; net->H = 128; net->W = 128; net->max_n = max_n;
  net->n_slots = n_slots;
  net->loss_scale = dtype == GI_F16 ? 65536.f : 1.f;
  return net;
}
void gi_net_add_param(gi_net* net, const char* name, int kind, const int64_t* shape, int ndim, int64_t* off) {
  TensorDesc t;
  t.name = name; t.kind = kind; t.ndim = ndim; t.numel = 1;
  for (int i = 0; i < 4; ++i) { t.shape[i] = i < ndim ? shape[i] : 1; t.numel *= t.shape[i]; }
  t.offset = net->n_params;
  net->n_params += gi_align_up(t.numel, 64);
  *off = t.offset;
  net->tensors.push_back(t);
}
void gi_net_set_workspace(gi_net* net, int64_t bytes) { net->arena.size = bytes; }
gi_dcgan* gi_net_dcgan_state(gi_net* net) { return net && net->kind == 2 ? net->dc : nullptr; }
void gi_net_dcgan_bound(gi_net* net, hipStream_t* st, const float** params, char** ws) {
  *st = net->bound ? net->ctx->stream : nullptr;
  *params = net->params;
  *ws = net->bound ? net->ws : nullptr;
}

extern "C" int gi_net_destroy(gi_net* net) {
  if (net) {
    if (net->dc) gi_dcgan_free(net->dc);
    if (net->st2) { (void)hipStreamSynchronize(net->st2); (void)hipStreamDestroy(net->st2); }
    if (net->ev_dz) (void)hipEventDestroy(net->ev_dz);
    for (hipEvent_t e : net->ev_wg) if (e) (void)hipEventDestroy(e);
  }
  delete net;
  return GI_OK;
}

// =================================================================================================
// inventory / binding
// =================================================================================================
extern "C" int gi_net_tensor_count(gi_net* net) { return net ? (int)net->tensors.size() : GI_ERR_INVALID; }

extern "C" int gi_net_tensor_desc(gi_net* net, int index, char* name, int name_cap, int* kind, int64_t* shape4, int* ndim,
                                  int64_t* offset, int64_t* numel) {
  GI_REQUIRE(net && index >= 0 && index < (int)net->tensors.size(), "tensor_desc: index %d out of range", index);
  const TensorDesc& t = net->tensors[index];
  if (name && name_cap > 0) {
    strncpy(name, t.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (kind) *kind = t.kind;
  if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
  if (ndim) *ndim = t.ndim;
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  return GI_OK;
}
extern "C" int64_t gi_net_param_floats(gi_net* net) { return net ? net->n_params : GI_ERR_INVALID; }
extern "C" int64_t gi_net_buffer_floats(gi_net* net) { return net ? net->n_buffers : GI_ERR_INVALID; }
extern "C" int64_t gi_net_workspace_bytes(gi_net* net) { return net ? net->arena.size : GI_ERR_INVALID; }

extern "C" int gi_net_bind(gi_net* net, float* params, float* grads, float* buffers, void* workspace, int64_t workspace_bytes) {
  GI_REQUIRE(net && params && grads && workspace, "net_bind: null pointer");
  GI_REQUIRE(buffers || net->n_buffers == 0, "net_bind: null buffers for a net with %lld buffer floats", (long long)net->n_buffers);
  GI_REQUIRE(net->ctx != nullptr, "net_bind: handle was created without a context (inventory only)");
  GI_REQUIRE(workspace_bytes >= net->arena.size, "net_bind: workspace %lld < required %lld", (long long)workspace_bytes,
             (long long)net->arena.size);
  GI_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)params & 15) == 0, "net_bind: workspace must be 256-byte aligned");
  net->params = net->master = params; net->grads = grads; net->buffers = buffers; net->ws = (char*)workspace;
  net->bound = true;
  net->sn_eff_gen = 0;
  if (net->acc_words > 0) GI_HIP(hipMemsetAsync(net->shared(net->oAcc), 0, (size_t)net->acc_words * 8, net->ctx->stream));
  if (net->oTickets >= 0) GI_HIP(hipMemsetAsync(net->shared(net->oTickets), 0, (size_t)GI_IGEMM_TICKETS * 4, net->ctx->stream));
  return GI_OK;
}

namespace {
const void* packed_ptr(const gi_net* net, const Conv& c) {
  return c.packed_off == -2 ? (const void*)(net->params + c.w_off) : (const void*)net->shared(c.packed_off);
}
const void* phase_ptr(const gi_net* net, const Conv& c) { return net->shared(c.phase_off); }

void pack_job(const gi_net* net, const Conv& c, PackJobs& P) {
  PackJob& J = P.j[P.n++];
  J.w = net->params + c.w_off; J.ca = c.ca; J.cb = c.cb; J.tile0 = 0; J.scale_on_b = 0; J.scale = nullptr;
  J.packed = c.packed_off >= 0 ? (void*)net->shared(c.packed_off) : nullptr;
  J.phase = net->shared(c.phase_off);
}

// ---- spectral normalisation (gi_net::sn) ----
// net->params points at the effective parameters while a forward / backward / penalty of such a handle runs
struct ParamsBack { gi_net* net; float* p; ~ParamsBack() { net->params = p; } };

float* sn_slot_uv(const gi_net* net, int s) { return (float*)net->slot(s, net->oSnSlot); }
float* sn_slot_sigma(const gi_net* net, int s) { return sn_slot_uv(net, s) + net->sn_uv_floats; }

SnSegs sn_segs(const gi_net* net, int s, int64_t lo, int64_t hi) {
  SnSegs S;
  for (int t = 0; t < 6; ++t) {
    const gi_net::SnTensor& T = net->snt[t];
    if (T.off < lo || T.off >= hi) continue;
    const float* uv = sn_slot_uv(net, s);
    S.s[S.n++] = SnSeg{T.off, (int64_t)T.ca * T.K, sn_slot_sigma(net, s) + t, T.ca, T.K, T.cb, uv + (T.u_off - net->sn_uv_off),
                       uv + (T.v_off - net->sn_uv_off), nullptr};
  }
  return S;
}

// Points net->params at the effective parameters of slot s's forward and re-derives them, and the packed copies, unless they
// already hold that forward's. fresh: this IS the forward - power iteration on the master weights (train mode; eval mode: sigma of
// the stored u, v), the slot keeps u | v | sigma. The caller holds a ParamsBack.
int sn_enter(gi_net* net, int s, bool fresh) {
  hipStream_t st = net->ctx->stream;
  float* eff = (float*)net->shared(net->oSnEff);
  if (fresh) {
    SnJobs P;
    P.n = 6;
    for (int t = 0; t < 6; ++t) {
      const gi_net::SnTensor& T = net->snt[t];
      SnJob& J = P.j[t];
      J.w = net->master + T.off; J.u = net->buffers + T.u_off; J.v = net->buffers + T.v_off; J.sigma = sn_slot_sigma(net, s) + t;
      J.ca = T.ca; J.K = T.K; J.cb = T.cb;
      op_sn_carve(J, (float*)net->shared(T.scratch));
    }
    GI_TRY(op_sn_power_iteration(st, P, net->sn_iters, net->train));
    GI_HIP(hipMemcpyAsync(sn_slot_uv(net, s), net->buffers + net->sn_uv_off, (size_t)net->sn_uv_floats * 4, hipMemcpyDeviceToDevice, st));
    net->slot_sn_gen[s] = ++net->sn_gen;
  }
  net->params = eff;
  if (net->sn_eff_gen == net->slot_sn_gen[s]) return GI_OK;
  GI_TRY(op_sn_effective(st, net->master, eff, net->n_params, sn_segs(net, s, 0, net->n_params)));
  PackJobs P;
  P.n = 0;
  for (int i = 2; i <= 4; ++i) pack_job(net, net->dconv[i], P);
  GI_TRY(op_pack_weights_batch(st, net->dtype, P));
  net->sn_eff_gen = net->slot_sn_gen[s];
  return GI_OK;
}

// dst[lo, hi) += scale * (projection of g through slot s's u, v, sigma; plain add outside the normalised tensors). g holds
// gradients with respect to the effective parameters, which the workspace must hold for slot s (sn_enter)
int sn_project(gi_net* net, int s, const float* g, float* dst, int64_t lo, int64_t hi, const float* scale_dev) {
  SnSegs S = sn_segs(net, s, lo, hi);
  SnJobs P;
  const float* eff = (const float*)net->shared(net->oSnEff);
  for (int t = 0; t < 6; ++t) {
    const gi_net::SnTensor& T = net->snt[t];
    if (T.off < lo || T.off >= hi) continue;
    SnJob& J = P.j[P.n];
    J.w = eff + T.off; J.g = g + T.off; J.ca = T.ca; J.K = T.K; J.cb = T.cb;
    op_sn_carve(J, (float*)net->shared(T.scratch));
    S.s[P.n].c = J.c;
    ++P.n;
  }
  return op_sn_project_add(net->ctx->stream, P, S, g, dst, lo, hi, scale_dev);
}

// [rows][b] -> [rows][bp] zero-padded (the outermost up-convolution of a multi-channel generator)
__global__ void __launch_bounds__(256) pad_b_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int b, int bp) {
  const int64_t total = rows * bp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % bp);
    dst[i] = j < b ? src[(i / bp) * b + j] : 0.f;
  }
}

}  // namespace

extern "C" int gi_net_sync_weights(gi_net* net) {
  GI_REQUIRE(net && net->bound, "sync_weights: net not bound");
  if (net->kind == 2) return gi_dcgan_sync(net->dc, net->ctx->stream, net->params, net->ws);
  ++net->affine_gen;   // parameters (and possibly running statistics) were written from outside
  // spectral norm: the packed copies derive from the effective weights, which every forward re-derives (patchgan_forward)
  if (net->sn) { net->sn_eff_gen = 0; return GI_OK; }
  PackJobs P;
  P.n = 0;
  auto add = [&](const Conv& c) { pack_job(net, c, P); };
  if (net->kind == 0) {
    for (int k = 2; k <= net->nd; ++k) {
      if (P.n + 2 > 16) { GI_TRY(op_pack_weights_batch(net->ctx->stream, net->dtype, P)); P.n = 0; }
      add(net->conv[k]);
      add(net->up[k]);
    }
    GI_TRY(op_pack_weights_batch(net->ctx->stream, net->dtype, P));
    if (net->out_c > 1) {
      const int ca = net->up[1].ca;
      float* pad = (float*)net->shared(net->oUp1Pad);
      hipLaunchKernelGGL(pad_b_kernel, dim3(256), dim3(256), 0, net->ctx->stream, net->params + net->up[1].w_off, pad, (int64_t)ca * 16,
                         net->out_c, 64);
      GI_LAUNCH_CHECK();
      GI_TRY(op_pack_weights(net->ctx->stream, net->dtype, pad, ca, 64, net->oUp1Packed >= 0 ? (void*)net->shared(net->oUp1Packed) : nullptr,
                             net->shared(net->oUp1Phase)));
    }
  } else {
    for (int i = 2; i <= 4; ++i) add(net->dconv[i]);
    GI_TRY(op_pack_weights_batch(net->ctx->stream, net->dtype, P));
  }
  return GI_OK;
}
extern "C" int gi_net_set_train(gi_net* net, int train) {
  GI_REQUIRE(net, "set_train: null");
  if (net->train != (train ? 1 : 0)) ++net->affine_gen;
  net->train = train ? 1 : 0;
  return GI_OK;
}
extern "C" int gi_net_set_inference(gi_net* net, int inference) {
  GI_REQUIRE(net, "set_inference: null");
  net->inference = inference ? 1 : 0;
  return GI_OK;
}
extern "C" int gi_net_set_bn_groups(gi_net* net, int groups) {
  GI_REQUIRE(net && net->kind != 0, "set_bn_groups: discriminator handle required");
  GI_REQUIRE(groups == 1 || groups == 2, "set_bn_groups: groups=%d (1 or 2)", groups);
  if (net->kind == 2) return GI_OK;   // DCGAN: no BatchNorm, a stacked batch is plain rows
  net->bn_groups = groups;
  return GI_OK;
}
extern "C" int gi_net_set_loss_scale(gi_net* net, float scale) {
  GI_REQUIRE(net && scale > 0.f, "set_loss_scale: scale must be > 0");
  net->loss_scale = scale;
  return GI_OK;
}
extern "C" int gi_net_set_dropout_seed(gi_net* net, uint64_t seed) {
  GI_REQUIRE(net, "set_dropout_seed: null");
  net->drop_seed = seed;
  net->drop_counter = 0;
  return GI_OK;
}
// The dropout stream is (seed, counter): every train-mode forward of a generator with dropout advances the counter by one. Reading
// and writing both lets a resumed run draw the masks the uninterrupted run would have drawn.
extern "C" int gi_net_get_dropout_state(gi_net* net, uint64_t* seed, uint64_t* counter) {
  GI_REQUIRE(net && seed && counter, "get_dropout_state: null");
  *seed = net->drop_seed;
  *counter = net->drop_counter;
  return GI_OK;
}
extern "C" int gi_net_set_dropout_state(gi_net* net, uint64_t seed, uint64_t counter) {
  GI_REQUIRE(net, "set_dropout_state: null");
  net->drop_seed = seed;
  net->drop_counter = counter;
  return GI_OK;
}
extern "C" int gi_net_dropout_mask(gi_net* net, int slot, int level, uint8_t* out_nchw, int64_t count) {
  GI_REQUIRE(net && net->kind == 0 && net->bound, "dropout_mask: generator handle required");
  GI_REQUIRE(slot >= 0 && slot < net->n_slots && level >= 5 && level <= net->nd - 1, "dropout_mask: slot=%d level=%d", slot, level);
  const int n = net->slot_n[slot], c = net->ch[level - 1], hw = net->Hk[level - 1] * net->Wk[level - 1];
  GI_REQUIRE(count == (int64_t)n * c * hw, "dropout_mask: count %lld != %lld", (long long)count, (long long)n * c * hw);
  return op_mask_nchw_to_nhwc(net->ctx->stream, (const uint8_t*)net->slot(slot, net->oMask[level]), out_nchw, n, c, hw, 0);
}
extern "C" int gi_net_set_dropout_mask(gi_net* net, int slot, int level, const uint8_t* mask_nchw) {
  GI_REQUIRE(net && net->kind == 0, "set_dropout_mask: generator handle required");
  GI_REQUIRE(slot >= 0 && slot < net->n_slots && level >= 5 && level <= net->nd - 1, "set_dropout_mask: slot=%d level=%d", slot, level);
  net->ext_mask[slot][level] = mask_nchw;
  return GI_OK;
}

// =================================================================================================
// forward / backward
// =================================================================================================
namespace {

struct BNPtrs { float *scale, *shift, *mean, *inv; };
BNPtrs bn_ptrs(const gi_net* net, int slot, const BN& b, int group = 0) {
  float* base = (float*)net->slot(slot, net->oStats) + b.stat_off + (int64_t)group * 4 * b.c;
  return {base, base + b.c, base + 2 * b.c, base + 3 * b.c};
}

// Channels [coff, coff + c) of an NHWC tensor whose pixels are ld elements apart (ld omitted: dense, ld = c)
struct Slice { const void* p = nullptr; int c = 0, ld = 0, coff = 0; };
Slice sl(const void* p, int c, int ld = 0, int coff = 0) { return {p, c, ld ? ld : c, coff}; }
// the generator's concat buffer of level k (gi_net::oC) and its halves; the input of up-convolution k
void* concat_buf(const gi_net* net, int s, int k) { return net->slot(s, net->oC[k]); }
Slice concat(const gi_net* net, int s, int k) { return sl(concat_buf(net, s, k), 2 * net->ch[k]); }
Slice skip_half(const gi_net* net, int s, int k) { return sl(concat_buf(net, s, k), net->ch[k], 2 * net->ch[k], 0); }
Slice up_half(const gi_net* net, int s, int k) { return sl(concat_buf(net, s, k), net->ch[k], 2 * net->ch[k], net->ch[k]); }
Slice up_input(const gi_net* net, int s, int k) { return k == net->nd ? sl(net->slot(s, net->oE), net->ch[k]) : concat(net, s, k); }

// Statistics plan of one BatchNorm layer, fixed BEFORE its GEMM runs: with `use` the GEMM adds its tile sums to the
// layer's exact accumulators (IgemmArgs::stat_acc) and bn_forward needs no reduction launch.
struct StatPlan { unsigned long long* acc = nullptr; unsigned long long* zero_next = nullptr; int zero_words = 0; int pg = 0; int reps = 1; bool use = false; };
// (`use` is cleared by gemm_run when the kernel that ran put its statistics into partial rows instead)
// replicas for `adders` tiles adding to one block: about 256 requests per 64-byte line (~3 us of queueing at the atomic unit)
int stat_reps_for(int64_t adders) {
  int r = 1;
  while (r < GI_STAT_MAXREP && adders > 256 * r) r <<= 1;
  return r;
}
// tile_rows: an upper bound on the partial rows the GEMM's tiles would write (tiles along M x sub-pixel phases)
StatPlan stat_plan(const gi_net* net, const BN& b, int64_t gemm_rows, int64_t tile_rows, int train) {
  StatPlan sp;
  const int g = net->kind == 1 ? net->bn_groups : 1;
  // two populations: every tile (256 / 128 rows, or a patch of one image) must lie inside one of them
  if (!train || !net->use_acc || b.acc_off < 0 || (g == 2 && (gemm_rows % 2 != 0 || (gemm_rows / 2) % 256 != 0))) return sp;
  unsigned long long* base = (unsigned long long*)net->shared(net->oAcc) + b.acc_off;
  sp.use = true;
  sp.reps = stat_reps_for(tile_rows);
  sp.acc = base + b.fwd_par * b.acc_block();
  sp.zero_next = base + (b.fwd_par ^ 1) * b.acc_block();
  sp.zero_words = (int)gi_stat_block_words(b.c, b.dirty[b.fwd_par ^ 1]);   // (the state moves when the plan is consumed: bn_forward)
  sp.pg = g == 2 ? (int)(gemm_rows / 2) : 0;
  return sp;
}

// the accumulator-path arguments of a layer's normalisation (pg pixels per population, g populations), and the state change of
// the layer's ping-pong accumulator regions once a launch that consumes them has been issued
BnAccArgs bn_acc_args(const gi_net* net, int slot, const BN& b, const StatPlan& sp, int64_t pg, int g) {
  BNPtrs p = bn_ptrs(net, slot, b, 0);
  BnAccArgs a;
  a.acc = sp.acc; a.gamma = net->params + b.gamma_off; a.beta = net->params + b.beta_off;
  a.running_mean = net->buffers + b.rmean_off; a.running_var = net->buffers + b.rvar_off;
  a.scale = p.scale; a.shift = p.shift; a.save_mean = p.mean; a.save_invstd = p.inv;
  a.count = pg; a.momentum = 0.1f; a.eps = 1e-5f; a.groups = g; a.out_stride = 4 * b.c;
  a.zero_next = sp.zero_words > 0 ? sp.zero_next : nullptr; a.zero_words = sp.zero_words;
  a.reps = sp.reps;
  return a;
}
void bn_acc_commit(gi_net* net, int slot, const BN& b, const StatPlan& sp) {
  b.dirty[b.fwd_par ^ 1] = 0;
  b.dirty[b.fwd_par] = sp.reps;
  b.fwd_par ^= 1;
  if (b.id >= 0) net->eval_gen[slot][b.id] = 0;
}

// Dropout of a decoder level as the pass that applies it sees it. p == 0: `mask` (if any) is read; p > 0: the keep-mask is drawn
// inside that pass (same hash, same masks as op_fill_dropout) from `seed` and stored at `mask`.
struct Dropout { uint8_t* mask = nullptr; float scale = 1.f; uint64_t seed = 0; float p = 0.f; };
int dropout_draw(gi_net* net, Dropout& d, int64_t count) {
  GI_TRY(op_fill_dropout(net->ctx->stream, d.mask, count, d.seed, d.p));
  d.p = 0.f;
  return GI_OK;
}
// The dropout of decoder level k in this forward (train mode, levels 5 .. nd - 1): an imposed mask is converted into the slot;
// otherwise the next seed is taken and the mask drawn at once, or with `defer` left to the pass that applies it (Dropout::p > 0;
// the BatchNorm generator calls dropout_draw itself where that pass turns out not to draw)
int dropout_prepare(gi_net* net, int s, int k, int n, bool defer, Dropout& d) {
  d = Dropout();
  if (!net->train || !(net->dropout_p > 0.f) || k < 5 || k > net->nd - 1) return GI_OK;
  const int co = net->ch[k - 1], hw = net->Hk[k - 1] * net->Wk[k - 1];
  d.mask = (uint8_t*)net->slot(s, net->oMask[k]);
  d.scale = 1.f / (1.f - net->dropout_p);
  if (net->ext_mask[s][k]) return op_mask_nchw_to_nhwc(net->ctx->stream, net->ext_mask[s][k], d.mask, n, co, hw, 1);
  d.seed = net->drop_seed + 0x1000003ull * (++net->drop_counter);
  d.p = net->dropout_p;
  return defer ? GI_OK : dropout_draw(net, d, (int64_t)n * hw * co);
}

// The copy of the input that the first layer's weight gradient reads (8.4 MB at the headline shape) rides in layer 2's
// normalisation pass where that pass takes a side copy (bn_forward on the accumulator path, a multiple of 16 bytes);
// input_copy is the device copy for every other case.
struct SideCopy { const void* src = nullptr; void* dst = nullptr; int64_t bytes = 0; };
SideCopy input_side_copy(const gi_net* net, int s, const float* x, int n, const StatPlan& sp) {
  const int64_t bytes = (int64_t)n * net->H * net->W * 4;
  if (!sp.use || bytes % 16 != 0) return SideCopy();
  return {x, net->slot(s, net->oX), bytes};
}
int input_copy(gi_net* net, int s, const float* x, int n) {
  GI_HIP(hipMemcpyAsync(net->slot(s, net->oX), x, (size_t)n * net->H * net->W * 4, hipMemcpyDeviceToDevice, net->ctx->stream));
  return GI_OK;
}

// raw (pixels,c) conv output with per-tile partial statistics -> normalise + activation into dst.
// With bn_groups = g the batch is g consecutive groups of pixels/g pixels, each normalised with its OWN batch
// statistics (the reference calls the critic separately on the real and on the fake batch: two BatchNorm
// populations, running statistics updated group by group in that order).
// apply = false: statistics / scale / shift only (a consumer applies the affine map itself, C1Affine)
// side: accumulator path only
struct BnOpts { bool apply = true; Dropout drop; SideCopy side; };
int bn_forward(gi_net* net, int slot, const BN& b, const void* raw, int64_t pixels, int ntiles, Slice dst, int act, int train,
               const StatPlan& sp, const BnOpts& o = BnOpts()) {
  hipStream_t st = net->ctx->stream;
  const int g = net->kind == 1 ? net->bn_groups : 1;
  const int64_t pg = pixels / g;
  const size_t T = net->tsz();
  const Dropout& drop = o.drop;
  if (sp.use) {
    const BnAccArgs a = bn_acc_args(net, slot, b, sp, pg, g);
    bn_acc_commit(net, slot, b, sp);
    if (o.apply) return op_bn_apply_acc(st, net->dtype, raw, (void*)dst.p, pixels, b.c, dst.ld, dst.coff, act, drop.mask, drop.scale, drop.seed, drop.p, a,
                                        o.side.src, o.side.dst, o.side.bytes);
    return op_bn_finalize_acc(st, b.c, a);
  }
  // the GEMM epilogue's partial rows can be split between the groups when a group is a whole number of tiles
  // (tile heights are 256, 128 or a power of two <= 64); otherwise each group's statistics come from a column pass
  const bool aligned = g == 1 || (pg % 256 == 0 && ntiles % g == 0);
  if (g == 2 && aligned) {   // both populations in one finalize and one apply launch
    BNPtrs p = bn_ptrs(net, slot, b, 0);
    const int rows = ntiles / 2;
    GI_TRY(op_bn_finalize(st, (const float*)net->shared(net->oPart), rows, b.c, pg, net->params + b.gamma_off, net->params + b.beta_off,
                          net->buffers + b.rmean_off, net->buffers + b.rvar_off, p.scale, p.shift, p.mean, p.inv, train, 0.1f, 1e-5f, 2,
                          (int64_t)rows * 2 * b.c, 4 * b.c));
    if (o.apply) GI_TRY(op_bn_apply(st, net->dtype, raw, (void*)dst.p, pixels, b.c, dst.ld, dst.coff, p.scale, p.shift, act, drop.mask, drop.scale, pg, 4 * b.c));
    return GI_OK;
  }
  for (int j = 0; j < g; ++j) {
    BNPtrs p = bn_ptrs(net, slot, b, j);
    const char* rj = (const char*)raw + (int64_t)j * pg * b.c * T;
    const float* part = (const float*)net->shared(net->oPart);
    int rows = ntiles / g;
    if (aligned) {
      part += (int64_t)j * rows * 2 * b.c;
    } else {
      float* scratch = (float*)net->shared(net->oPart) + (int64_t)ntiles * 2 * b.c;
      GI_REQUIRE((int64_t)ntiles * 2 * b.c + (pg / 32 + 8) * 2 * b.c <= net->part_floats, "internal: partials buffer too small for a column pass");
      GI_TRY(op_col_stats(st, net->dtype, rj, pg, b.c, scratch, &rows));
      part = scratch;
    }
    const bool cached = !train && g == 1 && b.id >= 0 && net->eval_gen[slot][b.id] == net->affine_gen;
    if (!cached) {
      GI_TRY(op_bn_finalize(st, part, rows, b.c, pg, net->params + b.gamma_off, net->params + b.beta_off, net->buffers + b.rmean_off,
                            net->buffers + b.rvar_off, p.scale, p.shift, p.mean, p.inv, train, 0.1f, 1e-5f));
      if (b.id >= 0) net->eval_gen[slot][b.id] = (!train && g == 1) ? net->affine_gen : 0;
    }
    if (o.apply)
      GI_TRY(op_bn_apply(st, net->dtype, rj, (char*)dst.p + (int64_t)j * pg * dst.ld * T, pg, b.c, dst.ld, dst.coff, p.scale, p.shift, act,
                         drop.mask ? drop.mask + (int64_t)j * pg * b.c : nullptr, drop.scale));
  }
  return GI_OK;
}

// pixels: rows of the BatchNorm'd tensor; gemm_tiles: workgroups of the producing GEMM that will add (tiles x phases)
BwdFuse bwd_fuse_plan(gi_net* net, int slot, const BN& bn, const void* x, int64_t pixels, int64_t gemm_tiles, float slope) {
  BwdFuse f;
  const int on = gi_opt(GI_OPT_BN_BWD_FUSE);   // GI_BN_BWD_FUSE=0: reduce pass as a separate launch
  const int g = net->kind == 1 ? net->bn_groups : 1;
  if (!on || !net->use_acc || bn.acc_off < 0 || net->bwd_eval || net->dtype != GI_F16) return f;
  const int64_t pg = pixels / g;
  if (g == 2) {   // the same condition under which act_bn_bwd reduces both populations in one launch
    const int rpb = op_bwd_rows_per_block(pg);
    if (pixels % 2 != 0 || pg % rpb != 0 || (2 * (pg / rpb)) * 2 * bn.c > net->part_floats) return f;
  }
  const int64_t blocks = (pg + op_bwd_rows_per_block(pg) - 1) / op_bwd_rows_per_block(pg);
  unsigned long long* base = (unsigned long long*)net->shared(net->oAcc) + bn.acc_off + 2 * bn.acc_block();
  f.planned = true;
  f.groups = g;
  f.acc = base + bn.bwd_par * bn.acc_block();
  f.reps_gemm = stat_reps_for(gemm_tiles);
  f.reps_reduce = stat_reps_for(blocks);
  const int other = 2 + (bn.bwd_par ^ 1);
  f.zero_words = (int)gi_stat_block_words(bn.c, bn.dirty[other]);
  f.zero_next = f.zero_words > 0 ? base + (bn.bwd_par ^ 1) * bn.acc_block() : nullptr;
  bn.dirty[other] = 0;
  bn.dirty[2 + bn.bwd_par] = f.reps_gemm > f.reps_reduce ? f.reps_gemm : f.reps_reduce;
  bn.bwd_par ^= 1;
  BNPtrs p0 = bn_ptrs(net, slot, bn, 0);
  f.x = x; f.ldx = bn.c; f.scale = p0.scale; f.shift = p0.shift; f.mean = p0.mean; f.inv = p0.inv; f.stride = 4 * bn.c;
  f.slope = slope; f.pg = g == 2 ? pg : 0;
  return f;
}
// a reduction planned by an earlier, abandoned backward (a phase 1 without its phase 2) left sums in its accumulator block
int clear_pending_bwd(gi_net* net, const BN* bn, int count) {
  for (int i = 0; i < count; ++i) {
    if (bn[i].c == 0 || bn[i].id < 0) continue;
    BwdFuse& pend = net->bwd_pending[bn[i].id];
    if (pend.planned) GI_HIP(hipMemsetAsync(pend.acc, 0, (size_t)bn[i].acc_block() * 8, net->ctx->stream));
    pend = BwdFuse();
  }
  return GI_OK;
}

// IgemmArgs::c1w_*: the first layer's weight gradient from the second layer's input-gradient GEMM
struct C1WFuse {
  const float* img = nullptr; float* part = nullptr; int64_t part_floats = 0; float scale = 1.f; int skip_out = 0;
  int applied = 0, blocks = 0;   // (returned)
};

// One layer's implicit GEMM while it is assembled: gemm_args() fills what the net owns and what every call needs, the call site
// sets the optional IgemmArgs fields it uses by name (bias, relu_in, relu_cend, act_out), the with_*() functions attach the fused
// passes, gemm_run() launches and copies what the kernel reports back into the attached plans. Everything else stays zero.
struct Gemm {
  IgemmArgs a;
  StatPlan* sp = nullptr; BwdFuse* bf = nullptr; C1WFuse* c1w = nullptr;
};
Gemm gemm_args(const gi_net* net, Slice in, const void* w, Slice out, int n, int Hs, int Ws) {
  Gemm g;
  IgemmArgs& a = g.a;
  memset(&a, 0, sizeof(a));
  a.in = in.p; a.cin = in.c; a.ldin = in.ld; a.coffin = in.coff;
  a.w = w;
  a.out = (void*)out.p; a.cout = out.c; a.ldout = out.ld; a.coffout = out.coff;
  a.n = n; a.Hs = Hs; a.Ws = Ws;
  a.ws = net->split_bytes > 0 ? (float*)net->shared(net->oSplit) : nullptr;
  a.ws_bytes = net->split_bytes;
  a.tickets = net->oTickets >= 0 ? (unsigned*)net->shared(net->oTickets) : nullptr;
  return g;
}
// column statistics of the result for the BatchNorm that follows: partial rows, or with a plan in use the exact accumulators and
// then, if offered, the normalisation pass folded into the launch (IgemmFold; the kernel decides: IgemmArgs::fold_applied)
void with_stats(const gi_net* net, Gemm& g, StatPlan& sp, const IgemmFold* fold = nullptr) {
  g.sp = &sp;
  g.a.partials = (float*)net->shared(net->oPart);
  if (sp.use) { g.a.stat_acc = sp.acc; g.a.stat_pg = sp.pg; g.a.stat_reps = sp.reps; g.a.fold = fold; }
}
// the BatchNorm-backward reduction of the layer the result is the output gradient of (bwd_fuse_plan)
void with_bn_bwd(Gemm& g, BwdFuse& bf) {
  g.bf = &bf;
  if (!bf.planned) return;
  IgemmArgs& a = g.a;
  a.bwd_x = bf.x; a.bwd_ldx = bf.ldx; a.bwd_scale = bf.scale; a.bwd_shift = bf.shift; a.bwd_mean = bf.mean; a.bwd_inv = bf.inv;
  a.bwd_stride = bf.stride; a.bwd_slope = bf.slope; a.bwd_acc = bf.acc; a.bwd_reps = bf.reps_gemm; a.bwd_pg = bf.pg;
  a.bwd_c0 = bf.c0; a.bwd_c = bf.c;
}
// The result is the gradient at the output of the net's first layer (slot s; no norm, activation y1): its LeakyReLU backward rides
// in the epilogue (IgemmArgs::mask; the generator names a second gradient, IgemmArgs::add, itself), reading the sign words the
// forward wrote instead of y1 where it did (mask_bits). With the sign words the first layer's weight gradient can be formed
// from the tiles while they are in LDS (c1w_*); without an input gradient to compute the result is then never stored.
void with_first_layer_bwd(gi_net* net, int s, Gemm& g, Slice y1, bool need_wgrad, bool need_dx, C1WFuse& c1w) {
  IgemmArgs& a = g.a;
  a.mask = y1.p; a.ldmask = y1.ld; a.mask_slope = 0.2f;
  if (net->slot_bits1[s] && gi_opt(GI_OPT_MASK_BITS)) a.mask_bits = (const unsigned long long*)net->slot(s, net->oBits1);
  if (!a.mask_bits || !need_wgrad || net->oC1w < 0 || !gi_opt(GI_OPT_C1W_FUSE)) return;
  c1w.img = (const float*)net->slot(s, net->oX); c1w.part = (float*)net->shared(net->oC1w); c1w.part_floats = net->c1w_floats - 64 * 1024;
  c1w.scale = 1.f / net->loss_scale; c1w.skip_out = need_dx ? 0 : 1;
  a.c1w_img = c1w.img; a.c1w_part = c1w.part; a.c1w_part_floats = c1w.part_floats; a.c1w_scale = c1w.scale; a.c1w_skip_out = c1w.skip_out;
  g.c1w = &c1w;
}
// phase: op_igemm's mode (0: the stride-2 gather, 1: sub-pixel phases)
int gemm_run(gi_net* net, int phase, Gemm& g) {
  IgemmArgs& a = g.a;
  GI_TRY(op_igemm(net->ctx->stream, net->dtype, phase, a));
  if (g.c1w) { g.c1w->applied = a.c1w_applied; g.c1w->blocks = a.c1w_blocks; }
  if (g.bf && g.bf->planned) g.bf->applied = a.bwd_applied != 0;
  if (g.sp && g.sp->use && !a.stat_used) g.sp->use = false;
  if (a.partials) GI_REQUIRE((int64_t)a.ntiles_out * 2 * a.cout <= net->part_floats, "internal: partials buffer too small");
  return GI_OK;
}
int gemm_run(gi_net* net, int phase, Gemm&& g) { return gemm_run(net, phase, g); }

WgradArgs wgrad_args(const gi_net* net, Slice S, Slice L, int n, int Hs, int Ws, float* dW) {
  WgradArgs a;
  a.S = S.p; a.L = L.p; a.dW = dW; a.n = n; a.Hs = Hs; a.Ws = Ws;
  a.ca = S.c; a.ldS = S.ld; a.coffS = S.coff; a.cb = L.c; a.ldL = L.ld; a.coffL = L.coff;
  a.relu_S = 0; a.scale = 1.f / net->loss_scale;
  a.scratch = net->wg_bytes > 0 ? (float*)net->shared(net->oWg) : nullptr;
  a.scratch_bytes = net->wg_bytes;
  return a;
}
int wgrad_run(gi_net* net, const WgradArgs& a) {
  if (!net->side) return op_wgrad(net->ctx->stream, net->dtype, a);
  // second stream: starts when everything the chain has issued so far (dz of this level) is done; the event recorded behind it
  // guards the dz buffer of this level (side_dz)
  GI_HIP(hipEventRecord(net->ev_dz, net->ctx->stream));
  GI_HIP(hipStreamWaitEvent(net->st2, net->ev_dz, 0));
  GI_TRY(op_wgrad(net->st2, net->dtype, a));
  GI_HIP(hipEventRecord(net->ev_wg[net->dz_i], net->st2));
  net->wg_busy[net->dz_i] = true;
  return GI_OK;
}

// --- second stream of a backward (gi_net::st2) ---
int side_begin(gi_net* net, int need_wgrad) {
  net->side = false;
  net->dz_i = 0;
  if (!need_wgrad || !gi_opt(GI_OPT_WGRAD_STREAM) || (net->kind == 0 && net->norm_kind != 0)) return GI_OK;
  if (!net->st2) {
    if (gi_opt(GI_OPT_WGRAD_STREAM) == 2) {   // lowest priority: the weight gradients fill what the chain leaves free
      int least = 0, greatest = 0;
      GI_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      GI_HIP(hipStreamCreateWithPriority(&net->st2, hipStreamNonBlocking, least));
    } else {
      GI_HIP(hipStreamCreateWithFlags(&net->st2, hipStreamNonBlocking));
    }
    GI_HIP(hipEventCreateWithFlags(&net->ev_dz, hipEventDisableTiming));
    for (hipEvent_t& e : net->ev_wg) GI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  net->side = true;
  return GI_OK;
}
// the chain's stream waits for every weight gradient still in flight (also after an error return: the flags outlive the call)
int side_join(gi_net* net) {
  for (int i = 0; i < 3; ++i)
    if (net->wg_busy[i]) {
      net->wg_busy[i] = false;
      GI_HIP(hipStreamWaitEvent(net->ctx->stream, net->ev_wg[i], 0));
    }
  net->side = false;
  return GI_OK;
}
// the buffer the next level's dz is written to
void* side_dz(gi_net* net) {
  if (!net->side) return net->shared(net->oDr[0]);
  net->dz_i = (net->dz_i + 1) % 3;
  if (net->wg_busy[net->dz_i]) {   // read by the weight gradient three levels back
    net->wg_busy[net->dz_i] = false;
    (void)hipStreamWaitEvent(net->ctx->stream, net->ev_wg[net->dz_i], 0);
  }
  return net->shared(net->oDr[net->dz_i]);
}

// Backward through [dropout] -> activation -> [norm] of a layer with the saved activation y: act_bwd_args() fills what every call
// needs, the call site names its gradient sources (set_g1 / set_g2, the latter masked by [y > 0]), the raw tensor x and drop_scale;
// act_bn_bwd() adds what the net owns and launches into dx (dense), per BatchNorm population where they cannot share the launches.
ActBnBwdArgs act_bwd_args(Slice y, int64_t pixels, int act) {
  ActBnBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y.p; a.ldy = y.ld; a.coffy = y.coff; a.c = y.c;
  a.pixels = pixels; a.act = act; a.drop_scale = 1.f;
  return a;
}
void set_g1(ActBnBwdArgs& a, Slice g) { a.g1 = g.p; a.ldg1 = g.ld; a.coffg1 = g.coff; }
void set_g2(ActBnBwdArgs& a, Slice g) { a.g2 = g.p; a.ldg2 = g.ld; a.coffg2 = g.coff; }
// bn: the layer's BatchNorm (none: activation backward only); pre: a reduction the producing GEMM was asked for (bwd_fuse_plan)
int act_bn_bwd(gi_net* net, int slot, const ActBnBwdArgs& in, void* dx, const BN* bn = nullptr, int need_wgrad = 0, const BwdFuse* pre = nullptr) {
  const int64_t pixels = in.pixels;
  const int c = in.c;
  int g = (net->kind == 1 && bn) ? net->bn_groups : 1;   // BatchNorm groups: reductions per group
  int64_t pg = pixels / g;
  const int64_t T = (int64_t)net->tsz();
  // both populations in the same three launches when a reduce workgroup never straddles them
  const bool merged = g == 2 && !net->bwd_eval && pg % op_bwd_rows_per_block(pg) == 0 &&
                      (2 * (pg / op_bwd_rows_per_block(pg))) * 2 * c <= net->part_floats;
  if (merged) { g = 1; pg = pixels; }
  for (int j = 0; j < g; ++j) {
    ActBnBwdArgs a = in;
    a.groups = merged ? 2 : 1; a.stat_stride = 4 * c;
    const int64_t o = (int64_t)j * pg;
    if (a.g1) a.g1 = (const char*)in.g1 + o * a.ldg1 * T;
    if (a.g2) a.g2 = (const char*)in.g2 + o * a.ldg2 * T;
    a.y = (const char*)in.y + o * a.ldy * T;
    if (a.x) a.x = (const char*)in.x + o * c * T;
    a.dx = (char*)dx + o * c * T;
    a.pixels = pg;
    a.has_bn = bn ? 1 : 0;
    a.eval_bn = net->bwd_eval;
    if (bn) {
      BNPtrs p = bn_ptrs(net, slot, *bn, j);
      a.gamma = net->params + bn->gamma_off; a.save_mean = p.mean; a.save_invstd = p.inv;
      if (a.drop_scale == 1.f && a.x) { a.fwd_scale = p.scale; a.fwd_shift = p.shift; }   // dropout zeros live only in y
      a.dgamma = need_wgrad ? net->grads + bn->gamma_off : nullptr;
      a.dbeta = need_wgrad ? net->grads + bn->beta_off : nullptr;
    }
    a.inv_loss_scale = 1.f / net->loss_scale;
    a.partials = (float*)net->shared(net->oPart);
    a.sums = (float*)net->shared(net->oSums);
    if (pre && pre->planned) {   // the accumulator block was chosen before the producing GEMM ran (bwd_fuse_plan)
      GI_REQUIRE(bn && (merged || g == 1), "internal: fused BatchNorm-backward plan without the one-launch reduction");
      a.acc = pre->acc;
      a.acc_reps = pre->reps_gemm > pre->reps_reduce ? pre->reps_gemm : pre->reps_reduce;
      a.zero_next = pre->zero_next; a.zero_words = pre->zero_words;
      a.reduce_done = pre->applied ? 1 : 0;
    } else if (bn && net->use_acc && bn->acc_off >= 0 && (merged || g == 1)) {   // exact accumulators: no sums launch (stat_acc.h)
      unsigned long long* base = (unsigned long long*)net->shared(net->oAcc) + bn->acc_off + 2 * bn->acc_block();
      a.acc = base + bn->bwd_par * bn->acc_block();
      if (!net->bwd_eval) {   // (a running-statistics backward adds nothing: the block stays clean)
        a.acc_reps = stat_reps_for((pg + op_bwd_rows_per_block(pg / a.groups) - 1) / op_bwd_rows_per_block(pg / a.groups));
        const int other = 2 + (bn->bwd_par ^ 1);
        a.zero_words = (int)gi_stat_block_words(bn->c, bn->dirty[other]);
        a.zero_next = a.zero_words > 0 ? base + (bn->bwd_par ^ 1) * bn->acc_block() : nullptr;
        bn->dirty[other] = 0;
        bn->dirty[2 + bn->bwd_par] = a.acc_reps;
        bn->bwd_par ^= 1;
      }
    }
    GI_TRY(op_act_bn_bwd(net->ctx->stream, net->dtype, a));
  }
  return GI_OK;
}

__global__ void __launch_bounds__(256) fill_f32_kernel(float* dst, int count, float v) {
  for (int i = threadIdx.x; i < count; i += 256) dst[i] = v;
}

// dst += scale * sum(src), bit-reproducible: per-block sums (fp64) to part[gridDim.x], then ONE block adds them in index order
__global__ void __launch_bounds__(256) sum_part_kernel(const float* src, int64_t count, double* part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) s += src[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ void __launch_bounds__(256) sum_finish_kernel(const double* part, int blocks, float* dst, float scale) {
  __shared__ double sh[256];
  sh[threadIdx.x] = threadIdx.x < blocks ? part[threadIdx.x] : 0.0;   // blocks <= 256
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) dst[0] += (float)(sh[0] * scale);
}

int grid1d(int64_t work) {
  int64_t b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b < 1 ? 1 : b);
}
// y[n][j][p] = tanh(u[n][p][j] + bias[j]), j < out_c, u NHWC with 64 (padded) channels
template <typename T>
__global__ void __launch_bounds__(256) head_tanh_kernel(const T* __restrict__ u, const float* __restrict__ bias, float* __restrict__ y, int n,
                                                        int out_c, int hw) {
  const int64_t total = (int64_t)n * out_c * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % hw);
    const int64_t t = i / hw;
    const int j = (int)(t % out_c);
    const int64_t img = t / out_c;
    y[i] = tanhf((float)u[(img * hw + p) * 64 + j] + bias[j]);
  }
}
// g (n,out_c,hw) fp32 -> NHWC T with 64 channels, zero beyond out_c
template <typename T>
__global__ void __launch_bounds__(256) pad_dy_kernel(const float* __restrict__ g, T* __restrict__ out, int n, int out_c, int hw) {
  const int64_t total = (int64_t)n * hw * 64;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i & 63);
    const int64_t t = i >> 6;
    const int p = (int)(t % hw);
    const int64_t img = t / hw;
    out[i] = j < out_c ? (T)g[(img * out_c + j) * hw + p] : (T)0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// Inference (gi_net_set_inference + eval mode): every BatchNorm is a fixed affine map, so its scale goes into the
// preceding convolution's weights (a second copy in the forward's layout), its shift becomes the GEMM's bias and
// the activation runs in the GEMM epilogue, which writes straight into the skip buffers: no normalisation pass at all.
// The folded copies are rebuilt when the generation counter says weights or running statistics changed.
int unet_sync_inference(gi_net* net) {
  hipStream_t st = net->ctx->stream;
  const int nd = net->nd;
  auto aff = [&](const BN& b) { return (float*)net->shared(b.inf_off); };
  PackJobs P;
  P.n = 0;
  for (int k = 2; k <= nd; ++k) {
    for (int up = 0; up < 2; ++up) {
      if (!up && k == nd) continue;   // the innermost convolution has no norm
      const BN& b = up ? net->unorm[k] : net->dnorm[k];
      const Conv& c = up ? net->up[k] : net->conv[k];
      float* a = aff(b);
      GI_TRY(op_bn_finalize(st, nullptr, 0, b.c, 1, net->params + b.gamma_off, net->params + b.beta_off, net->buffers + b.rmean_off,
                            net->buffers + b.rvar_off, a, a + b.c, a + 2 * b.c, a + 3 * b.c, 0, 0.1f, 1e-5f));
      if (P.n == 16) { GI_TRY(op_pack_weights_batch(st, net->dtype, P)); P.n = 0; }
      PackJob& J = P.j[P.n++];
      J.w = net->params + c.w_off; J.ca = c.ca; J.cb = c.cb; J.tile0 = 0;
      J.packed = up ? nullptr : (void*)net->shared(c.inf_off);
      J.phase = up ? (void*)net->shared(c.inf_off) : nullptr;
      J.scale = a; J.scale_on_b = up;
    }
  }
  GI_TRY(op_pack_weights_batch(st, net->dtype, P));
  net->inf_gen = net->affine_gen;
  return GI_OK;
}

int launch_head_tanh(gi_net* net, const void* u, float* y, int n) {
  const int hw = net->H * net->W;
  const float* bias = net->params + net->up[1].bias_off;
  const dim3 grid(grid1d((int64_t)n * net->out_c * hw));
  if (net->dtype == GI_F16) hipLaunchKernelGGL(head_tanh_kernel<half_t>, grid, dim3(256), 0, net->ctx->stream, (const half_t*)u, bias, y, n, net->out_c, hw);
  else hipLaunchKernelGGL(head_tanh_kernel<float>, grid, dim3(256), 0, net->ctx->stream, (const float*)u, bias, y, n, net->out_c, hw);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
int launch_pad_dy(gi_net* net, const float* g, void* out, int n) {
  const int hw = net->H * net->W;
  const dim3 grid(grid1d((int64_t)n * hw * 64));
  if (net->dtype == GI_F16) hipLaunchKernelGGL(pad_dy_kernel<half_t>, grid, dim3(256), 0, net->ctx->stream, g, (half_t*)out, n, net->out_c, hw);
  else hipLaunchKernelGGL(pad_dy_kernel<float>, grid, dim3(256), 0, net->ctx->stream, g, (float*)out, n, net->out_c, hw);
  GI_LAUNCH_CHECK();
  return GI_OK;
}

// The last decoder level of the BatchNorm generator feeds only the single-channel head: its BatchNorm + ReLU is applied by the
// head's kernels while they read the raw tensor, so the upper half of the level-1 concat buffer is never written
C1Affine u2_affine(const gi_net* net, int s) {
  BNPtrs p = bn_ptrs(net, s, net->unorm[2]);
  C1Affine aff;
  aff.x2 = net->slot(s, net->oU[2]); aff.ld2 = net->ch[1]; aff.scale = p.scale; aff.shift = p.shift;
  return aff;
}

// u1: ConvTranspose2d(2 ngf -> out_c) + bias + Tanh of the level-1 concat buffer into y (n, out_c, H, W) fp32. save: also into
// the slot, for the backward (an inference forward does not). aff: u2_affine.
int head_forward(gi_net* net, int s, float* y, int n, bool save, const C1Affine* aff = nullptr) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, c1 = 2 * net->ch[1], Hs = net->Hk[1], Ws = net->Wk[1];
  const void* X = concat_buf(net, s, 1);
  const float* w = net->params + net->up[1].w_off;
  const float* bias = net->params + net->up[1].bias_off;
  float* osave = (float*)net->slot(s, net->oOut);
  if (net->out_c == 1)   // y written beside the saved output
    return op_c1_scatter(st, dt, X, w, bias, osave, n, Hs, Ws, c1, c1, 0, 1, 1, 1.f, net->shared(net->oCol), y, aff);
  if (op_c1_head4_ok(dt, c1, net->out_c, Ws, c1, 0))   // the face-parsing network's head: 64-row col GEMM + overlap-add
    return op_c1_head4_forward(st, X, w, bias, osave, y, n, Hs, Ws, c1, 0, 1, net->shared(net->oCol));
  // out_c channels: the same sub-pixel GEMM as the other up-convolutions on weights zero-padded to 64 output channels,
  // then bias + tanh of the first out_c channels
  void* U1 = net->shared(net->oU1);
  Gemm g = gemm_args(net, sl(X, c1), net->shared(net->oUp1Phase), sl(U1, 64), n, Hs, Ws);
  g.a.relu_in = 1; g.a.relu_cend = net->ch[1];
  GI_TRY(gemm_run(net, 1, g));
  GI_TRY(launch_head_tanh(net, U1, save ? osave : y, n));
  if (save) GI_HIP(hipMemcpyAsync(y, osave, (size_t)n * net->out_c * net->H * net->W * 4, hipMemcpyDeviceToDevice, st));
  return GI_OK;
}

// backward of head_forward: tanh' and loss scaling of dy into G0, u1's bias and weight gradients, the gradient of the level-1
// concat buffer into ogC[1]
int head_backward(gi_net* net, int s, const float* dy, int need_wgrad, const C1Affine* aff = nullptr) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, n = net->slot_n[s], c1 = 2 * net->ch[1], Hs = net->Hk[1], Ws = net->Wk[1];
  const int64_t npx = (int64_t)n * net->H * net->W;
  const float iLS = 1.f / net->loss_scale;
  float* G0 = (float*)net->shared(net->oG0);
  const float* w = net->params + net->up[1].w_off;
  void* g1 = net->shared(net->ogC[1]);
  GI_TRY(op_tanh_bwd(st, dy, (const float*)net->slot(s, net->oOut), G0, npx * net->out_c, net->loss_scale));
  if (need_wgrad) {
    // (the u1 bias gradient: a sum over every output pixel, fixed order)
    hipLaunchKernelGGL(sum_part_kernel, dim3(256), dim3(256), 0, st, G0, npx, (double*)net->shared(net->oPart));
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)net->shared(net->oPart), 256, net->grads + net->up[1].bias_off, iLS);
    GI_LAUNCH_CHECK();
    GI_TRY(op_c1_wgrad(st, dt, concat_buf(net, s, 1), G0, net->grads + net->up[1].w_off, n, Hs, Ws, c1, c1, 0, 1, iLS, 1.f, aff,
                       (float*)net->shared(net->oPart), net->part_floats));
  }
  if (net->out_c == 1) return op_c1_gather(st, dt, G0, w, g1, n, Hs, Ws, c1, c1, 0, GI_ACT_NONE, 1.f);
  if (op_c1_head4_ok(dt, c1, net->out_c, Ws, c1, 0)) return op_c1_head4_dgrad(st, G0, w, g1, n, Hs, Ws, c1, 0);
  void* U1 = net->shared(net->oU1);
  GI_TRY(launch_pad_dy(net, G0, U1, n));
  const void* wp = net->oUp1Packed >= 0 ? (const void*)net->shared(net->oUp1Packed) : (const void*)net->shared(net->oUp1Pad);
  return gemm_run(net, 0, gemm_args(net, sl(U1, 64), wp, sl(g1, c1), n, Hs, Ws));
}

const float* conv_bias(const gi_net* net, const Conv& c) { return c.bias_off >= 0 ? net->params + c.bias_off : nullptr; }

// dbias += (1 / loss scale) * column sums of the convolution's output gradient (InstanceNorm generator: use_bias)
int bias_grad(gi_net* net, const Conv& c, const void* dz, int64_t pixels, int ch) {
  if (c.bias_off < 0) return GI_OK;
  GI_REQUIRE((pixels / 32 + 8) * 2 * ch <= net->part_floats, "internal: partials buffer too small for a bias gradient");
  return op_bias_grad(net->ctx->stream, net->dtype, dz, pixels, ch, 1.f / net->loss_scale, net->grads + c.bias_off,
                      (float*)net->shared(net->oPart));
}

// The end of a backward at the net's first layer cv (single-channel input, (n, Hs, Ws, c) output, no norm). a1: its activation
// backward; it is skipped when the second layer's input-gradient GEMM already applied it to a1.g1
// (lrelu1_done, with_first_layer_bwd). Then the layer's weight (and bias) gradient - from the partial sums of that GEMM where it
// formed them (c1w) - and, if asked for, the input gradient dx.
int first_layer_tail(gi_net* net, int s, const Conv& cv, int n, int Hs, int Ws, const ActBnBwdArgs& a1, int need_wgrad, float* dx,
                     int lrelu1_done = 0, const C1WFuse* c1w = nullptr) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, c = a1.c;
  const float iLS = 1.f / net->loss_scale;
  float* dW = net->grads + cv.w_off;
  void* D = side_dz(net);
  const void* D1 = lrelu1_done ? a1.g1 : D;
  if (!lrelu1_done) GI_TRY(act_bn_bwd(net, s, a1, D));
  if (need_wgrad) GI_TRY(bias_grad(net, cv, D1, a1.pixels, c));
  if (need_wgrad && c1w && c1w->applied)
    GI_TRY(op_c1_wgrad_reduce(st, c1w->part, dW, c * 16, c1w->blocks, c1w->part + (int64_t)c1w->blocks * 1024,
                              net->c1w_floats - (int64_t)c1w->blocks * 1024));
  else if (need_wgrad)
    GI_TRY(op_c1_wgrad(st, dt, D1, (const float*)net->slot(s, net->oX), dW, n, Hs, Ws, c, c, 0, 0, iLS, 1.f, nullptr,
                       (float*)net->shared(net->oPart), net->part_floats));
  if (dx) GI_TRY(op_c1_scatter(st, dt, D1, net->params + cv.w_off, nullptr, dx, n, Hs, Ws, c, c, 0, 0, 0, iLS, net->shared(net->oCol)));
  return GI_OK;
}

int unet_forward_inference(gi_net* net, int s, const float* x, float* y, int n) {
  hipStream_t st = net->ctx->stream;
  const int nd = net->nd, dt = net->dtype;
  if (net->inf_gen != net->affine_gen) GI_TRY(unet_sync_inference(net));
  net->slot_n[s] = n;
  net->slot_train[s] = 0;
  net->slot_inference[s] = 1;
  net->slot_fused_u2[s] = 0;
  auto shift = [&](const BN& b) { return (const float*)net->shared(b.inf_off) + b.c; };
  GI_TRY(op_c1_gather(st, dt, x, net->params + net->conv[1].w_off, concat_buf(net, s, 1), n, net->Hk[1], net->Wk[1], net->ch[1], 2 * net->ch[1], 0,
                      GI_ACT_LRELU, 1.f));
  for (int k = 2; k < nd; ++k) {
    Gemm g = gemm_args(net, skip_half(net, s, k - 1), net->shared(net->conv[k].inf_off), skip_half(net, s, k), n, net->Hk[k], net->Wk[k]);
    g.a.act_out = GI_ACT_LRELU; g.a.bias = shift(net->dnorm[k]);
    GI_TRY(gemm_run(net, 0, g));
  }
  {
    Gemm g = gemm_args(net, skip_half(net, s, nd - 1), packed_ptr(net, net->conv[nd]), up_input(net, s, nd), n, net->Hk[nd], net->Wk[nd]);
    g.a.act_out = GI_ACT_RELU;
    GI_TRY(gemm_run(net, 0, g));
  }
  for (int k = nd; k >= 2; --k) {
    Gemm g = gemm_args(net, up_input(net, s, k), net->shared(net->up[k].inf_off), up_half(net, s, k - 1), n, net->Hk[k], net->Wk[k]);
    if (k < nd) { g.a.relu_in = 1; g.a.relu_cend = net->ch[k]; }
    g.a.act_out = GI_ACT_RELU; g.a.bias = shift(net->unorm[k]);
    GI_TRY(gemm_run(net, 1, g));
  }
  return head_forward(net, s, y, n, false);
}

// generator with InstanceNorm2d / without norm layers: the normalisation step after a convolution (raw -> dst with
// activation and dropout). InstanceNorm keeps (mean, inv) per image and channel in the slot for the backward.
int plain_norm_forward(gi_net* net, int slot, const BN& b, const void* raw, int n, int hw, Slice dst, int act, const Dropout& drop = Dropout()) {
  hipStream_t st = net->ctx->stream;
  if (net->norm_kind == 1)
    return op_in_forward(st, net->dtype, raw, (void*)dst.p, n, hw, b.c, dst.ld, dst.coff, act, drop.mask, drop.scale, 1e-5f,
                         (float*)net->slot(slot, net->oInStats) + b.in_off);
  return op_bn_apply(st, net->dtype, raw, (void*)dst.p, (int64_t)n * hw, b.c, dst.ld, dst.coff, nullptr, nullptr, act, drop.mask, drop.scale);
}

int unet_forward_plain(gi_net* net, int s, const float* x, float* y, int n);
int unet_backward_plain(gi_net* net, int s, const float* dy, float* dx, int need_wgrad, int phase);

// the normalisation pass of a small layer offered to the GEMM that produces it (IgemmFold; igemm7 decides)
IgemmFold fold_offer(const gi_net* net, int s, const BN& b, const StatPlan& sp, int64_t pixels, Slice dst, int act, const Dropout& drop = Dropout()) {
  IgemmFold fold;
  fold.bn = bn_acc_args(net, s, b, sp, pixels, 1);
  fold.dst = (void*)dst.p; fold.lddst = dst.ld; fold.coffdst = dst.coff; fold.act = act;
  fold.drop_mask = drop.mask; fold.drop_scale = drop.scale; fold.drop_seed = drop.seed; fold.drop_p = drop.p;
  return fold;
}

int unet_forward(gi_net* net, int s, const float* x, float* y, int n) {
  hipStream_t st = net->ctx->stream;
  const int nd = net->nd, dt = net->dtype, train = net->train;
  if (net->norm_kind != 0) return unet_forward_plain(net, s, x, y, n);
  if (!train && net->inference && nd >= 3) return unet_forward_inference(net, s, x, y, n);
  net->slot_inference[s] = 0;
  if (train) ++net->affine_gen;   // running statistics change below
  net->slot_n[s] = n;
  net->slot_train[s] = train;
  const bool fuse_u2 = nd >= 3 && net->out_c == 1 && net->fuse_head && op_c1_affine_ok(dt, 2 * net->ch[1], net->Wk[1], 2 * net->ch[1], 0);
  net->slot_fused_u2[s] = fuse_u2 ? 1 : 0;
  // d1: Conv2d(1->ngf) then the next block's in-place LeakyReLU (networks.py:287): the skip IS lrelu(x)
  GI_TRY(op_c1_gather(st, dt, x, net->params + net->conv[1].w_off, concat_buf(net, s, 1), n, net->Hk[1], net->Wk[1], net->ch[1], 2 * net->ch[1], 0,
                      GI_ACT_LRELU, 1.f, nullptr, gi_opt(GI_OPT_MASK_BITS) ? (unsigned long long*)net->slot(s, net->oBits1) : nullptr, &net->slot_bits1[s]));
  bool x_saved = false;
  for (int k = 2; k < nd; ++k) {
    const int64_t pix = (int64_t)n * net->Hk[k] * net->Wk[k];
    void* R = net->slot(s, net->oR[k]);
    StatPlan sp = stat_plan(net, net->dnorm[k], pix, (pix + 127) / 128, train);
    const bool offer = sp.use && dt == GI_F16;   // small layers: the GEMM's last finisher per channel column normalises the column itself
    IgemmFold fold;
    if (offer) fold = fold_offer(net, s, net->dnorm[k], sp, pix, skip_half(net, s, k), GI_ACT_LRELU);
    Gemm g = gemm_args(net, skip_half(net, s, k - 1), packed_ptr(net, net->conv[k]), sl(R, net->ch[k]), n, net->Hk[k], net->Wk[k]);
    with_stats(net, g, sp, offer ? &fold : nullptr);
    GI_TRY(gemm_run(net, 0, g));
    if (g.a.fold_applied) { bn_acc_commit(net, s, net->dnorm[k], sp); continue; }
    BnOpts o;
    if (k == 2) o.side = input_side_copy(net, s, x, n, sp);
    GI_TRY(bn_forward(net, s, net->dnorm[k], R, pix, g.a.ntiles_out, skip_half(net, s, k), GI_ACT_LRELU, train, sp, o));
    if (o.side.bytes > 0) x_saved = true;
  }
  {  // innermost: no down-norm; uprelu follows directly (networks.py:299-305)
    Gemm g = gemm_args(net, skip_half(net, s, nd - 1), packed_ptr(net, net->conv[nd]), up_input(net, s, nd), n, net->Hk[nd], net->Wk[nd]);
    g.a.act_out = GI_ACT_RELU;
    GI_TRY(gemm_run(net, 0, g));
  }
  BnAccArgs u2_acc;
  bool u2_deferred = false;
  if (!x_saved) GI_TRY(input_copy(net, s, x, n));
  for (int k = nd; k >= 2; --k) {
    const int64_t pix = (int64_t)n * net->Hk[k] * net->Wk[k], opix = 4 * pix;
    void* U = net->slot(s, net->oU[k]);
    StatPlan sp = stat_plan(net, net->unorm[k], pix, (pix + 127) / 128 * 4, train);
    Dropout drop;
    GI_TRY(dropout_prepare(net, s, k, n, true, drop));
    const bool fused = (k == 2) && fuse_u2;
    const bool offer = sp.use && dt == GI_F16 && !fused;
    IgemmFold fold;
    if (offer) fold = fold_offer(net, s, net->unorm[k], sp, opix, up_half(net, s, k - 1), GI_ACT_RELU, drop);
    Gemm g = gemm_args(net, up_input(net, s, k), phase_ptr(net, net->up[k]), sl(U, net->ch[k - 1]), n, net->Hk[k], net->Wk[k]);
    if (k < nd) { g.a.relu_in = 1; g.a.relu_cend = net->ch[k]; }
    with_stats(net, g, sp, offer ? &fold : nullptr);
    GI_TRY(gemm_run(net, 1, g));
    if (g.a.fold_applied) { bn_acc_commit(net, s, net->unorm[k], sp); continue; }
    if (drop.p > 0.f && !sp.use) GI_TRY(dropout_draw(net, drop, opix * net->ch[k - 1]));   // (else drawn inside the normalisation pass)
    // the decoder half is only ever consumed through the parent's in-place ReLU (networks.py:289): store
    // relu(u) so that consumers need the ReLU on the skip half only; [u > 0] masks are unchanged
    if (fused && sp.use) {   // the head's first kernel derives u2's scale / shift itself (C1Affine::bn): no finalize launch
      u2_acc = bn_acc_args(net, s, net->unorm[k], sp, opix, 1);
      bn_acc_commit(net, s, net->unorm[k], sp);
      u2_deferred = true;
      continue;
    }
    BnOpts o;
    o.apply = !fused; o.drop = drop;
    GI_TRY(bn_forward(net, s, net->unorm[k], U, opix, g.a.ntiles_out, up_half(net, s, k - 1), GI_ACT_RELU, train, sp, o));
  }
  C1Affine aff = u2_affine(net, s);
  if (u2_deferred) aff.bn = &u2_acc;
  return head_forward(net, s, y, n, true, fuse_u2 ? &aff : nullptr);
}

// phase: 0 = whole backward; 1 = decoder half (u1 .. u_nd: their parameter gradients occupy the tail
// of the flat gradient buffer and are complete when this returns); 2 = encoder half (d_nd .. d1).
// Splitting lets the host start the decoder gradients' all-reduce while the encoder half runs.
int unet_backward(gi_net* net, int s, const float* dy, float* dx, int need_wgrad, int phase) {
  if (net->norm_kind != 0) return unet_backward_plain(net, s, dy, dx, need_wgrad, phase);
  const int nd = net->nd, n = net->slot_n[s];
  // a forward in eval mode (running-statistics BatchNorm, no dropout) can be differentiated w.r.t. its input only:
  // the frozen segmentation network of the face-parsing loss (wgan_perceptual_style_faceparsing.py:212-213)
  GI_REQUIRE(n > 0 && (net->slot_train[s] || !need_wgrad), "unet_backward: slot %d holds no train-mode forward", s);
  GI_REQUIRE(!net->slot_inference[s], "unet_backward: slot %d holds an inference forward (gi_net_set_inference): nothing was saved for a backward", s);
  GI_REQUIRE(net->out_c == 1 || !need_wgrad, "unet_backward: parameter gradients of a %d-channel generator are not built", net->out_c);
  const int evalbn = net->slot_train[s] ? 0 : 1;
  net->bwd_eval = evalbn;
  auto gC = [&](int k) { return (void*)net->shared(net->ogC[k]); };
  auto gA = [&](int k) { return (void*)net->shared(net->ogA[k]); };
  auto dropped = [&](int k) { return !evalbn && net->dropout_p > 0.f && k >= 5 && k <= nd - 1; };   // decoder level k ran with dropout
  void* D = nullptr;   // dz of the level in progress (side_dz: rotates when the weight gradients run on the second stream)
  if (phase == 0 || phase == 1) {
    // the upper half of the level-1 concat buffer was never written where the forward fused u2 into the head: recomputed from the raw decoder output
    C1Affine aff = u2_affine(net, s);
    GI_TRY(head_backward(net, s, dy, need_wgrad, net->slot_fused_u2[s] ? &aff : nullptr));
    GI_TRY(clear_pending_bwd(net, &net->unorm[2], nd - 1));
    // decoder, outermost -> innermost: level k's concat gradient feeds up[k+1]
    for (int k = 1; k <= nd - 1; ++k) {
      const int kk = k + 1, ck = net->ch[k], ca = net->up[kk].ca;
      const int64_t pix = (int64_t)n * net->Hk[k] * net->Wk[k];
      D = side_dz(net);
      BwdFuse& pend = net->bwd_pending[net->unorm[kk].id];
      ActBnBwdArgs b = act_bwd_args(up_half(net, s, k), pix, GI_ACT_NONE);
      set_g2(b, sl(gC(k), ck, 2 * ck, ck));
      b.x = net->slot(s, net->oU[kk]);
      if (dropped(kk)) b.drop_scale = 1.f / (1.f - net->dropout_p);
      GI_TRY(act_bn_bwd(net, s, b, D, &net->unorm[kk], need_wgrad, &pend));
      pend = BwdFuse();
      if (need_wgrad) {
        WgradArgs wa = wgrad_args(net, up_input(net, s, kk), sl(D, ck), n, net->Hk[kk], net->Wk[kk], net->grads + net->up[kk].w_off);
        wa.relu_S = kk < nd ? 1 : 0;
        GI_TRY(wgrad_run(net, wa));
      }
      void* gout = (kk == nd) ? (void*)net->shared(net->ogE) : gC(kk);
      Gemm g = gemm_args(net, sl(D, ck), packed_ptr(net, net->up[kk]), sl(gout, ca), n, net->Hk[kk], net->Wk[kk]);
      // the upper half of this GEMM's columns is the gradient at the output of the NEXT decoder level's BatchNorm (its ReLU is the
      // consumer's): that layer's backward reduction rides in the epilogue (IgemmArgs::bwd_c0; levels without dropout, kernels that take it)
      const int kn = kk + 1;
      if (kk <= nd - 1 && !dropped(kn)) {
        const int64_t pixn = (int64_t)n * net->Hk[kk] * net->Wk[kk];
        BwdFuse& bf = net->bwd_pending[net->unorm[kn].id];
        bf = bwd_fuse_plan(net, s, net->unorm[kn], net->slot(s, net->oU[kn]), pixn, pixn / 256, 0.f);
        bf.c0 = ca / 2; bf.c = ca / 2;
        with_bn_bwd(g, bf);
      }
      GI_TRY(gemm_run(net, 0, g));
    }
  }  // decoder half
  if (phase == 1) return GI_OK;
  // the encoder half may be split once more: phase 3 = innermost .. level 5 (their parameter gradients, the bulk
  // of the encoder's, are complete first), phase 4 = levels 4 .. 1; phase 2 (or 0) runs both
  const bool run_inner = phase != 4, run_outer = phase != 3;
  int lrelu1_done = 0;
  C1WFuse c1w;
  // innermost conv (no norm): dz = gE * [E > 0]
  if (run_inner) {
    const int c = net->ch[nd], cb = net->ch[nd - 1];
    D = side_dz(net);
    ActBnBwdArgs b = act_bwd_args(up_input(net, s, nd), (int64_t)n * net->Hk[nd] * net->Wk[nd], GI_ACT_NONE);
    set_g2(b, sl(net->shared(net->ogE), c));
    GI_TRY(act_bn_bwd(net, s, b, D));
    if (need_wgrad)
      GI_TRY(wgrad_run(net, wgrad_args(net, sl(D, c), skip_half(net, s, nd - 1), n, net->Hk[nd], net->Wk[nd], net->grads + net->conv[nd].w_off)));
    GI_TRY(gemm_run(net, 1, gemm_args(net, sl(D, c), phase_ptr(net, net->conv[nd]), sl(gA(nd - 1), cb), n, net->Hk[nd], net->Wk[nd])));
  }
  // encoder, innermost -> outermost
  for (int k = nd - 1; k >= 2; --k) {
    if (k >= 5 ? !run_inner : !run_outer) continue;
    const int c = net->ch[k], cb = net->ch[k - 1];
    D = side_dz(net);
    ActBnBwdArgs b = act_bwd_args(skip_half(net, s, k), (int64_t)n * net->Hk[k] * net->Wk[k], GI_ACT_LRELU);
    set_g1(b, sl(gA(k), c));
    set_g2(b, sl(gC(k), c, 2 * c));
    b.x = net->slot(s, net->oR[k]);
    GI_TRY(act_bn_bwd(net, s, b, D, &net->dnorm[k], need_wgrad));
    if (need_wgrad)
      GI_TRY(wgrad_run(net, wgrad_args(net, sl(D, c), skip_half(net, s, k - 1), n, net->Hk[k], net->Wk[k], net->grads + net->conv[k].w_off)));
    Gemm g = gemm_args(net, sl(D, c), phase_ptr(net, net->conv[k]), sl(gA(k - 1), cb), n, net->Hk[k], net->Wk[k]);
    if (k == 2) {   // d1's backward, (g + [y>0] * skip gradient) * LeakyReLU'(y), and its weight gradient ride in this GEMM where the kernel takes them
      with_first_layer_bwd(net, s, g, skip_half(net, s, 1), need_wgrad, dx != nullptr, c1w);
      g.a.add = gC(1); g.a.ldadd = 2 * cb;
    }
    GI_TRY(gemm_run(net, 1, g));
    if (k == 2) lrelu1_done = g.a.mask_applied;
  }
  if (run_outer) {
    const int c = net->ch[1];
    ActBnBwdArgs a1 = act_bwd_args(skip_half(net, s, 1), (int64_t)n * net->Hk[1] * net->Wk[1], GI_ACT_LRELU);
    set_g1(a1, sl(gA(1), c));
    set_g2(a1, sl(gC(1), c, 2 * c));
    GI_TRY(first_layer_tail(net, s, net->conv[1], n, net->Hk[1], net->Wk[1], a1, need_wgrad, dx, lrelu1_done, &c1w));
  }
  return GI_OK;
}

// ---------------------------------------------------------------------------------------------
// Generator built with get_norm_layer('instance') or ('none') (networks.py:29-45, 270-318). Same skeleton as above on
// the unfused building blocks: convolution (+ bias) -> raw tensor -> normalisation pass (InstanceNorm statistics per
// image, or identity) with the activation and dropout. InstanceNorm has no running statistics: train and eval differ
// only by dropout. A bias in front of an InstanceNorm cancels in the forward and has a zero gradient up to rounding; it
// is still applied and differentiated like the reference does.
int unet_forward_plain(gi_net* net, int s, const float* x, float* y, int n) {
  hipStream_t st = net->ctx->stream;
  const int nd = net->nd, dt = net->dtype, train = net->train;
  net->slot_inference[s] = 0;
  net->slot_n[s] = n;
  net->slot_train[s] = train;
  net->slot_fused_u2[s] = 0;
  GI_TRY(input_copy(net, s, x, n));
  GI_TRY(op_c1_gather(st, dt, x, net->params + net->conv[1].w_off, concat_buf(net, s, 1), n, net->Hk[1], net->Wk[1], net->ch[1], 2 * net->ch[1], 0,
                      GI_ACT_LRELU, 1.f, conv_bias(net, net->conv[1])));
  for (int k = 2; k < nd; ++k) {
    void* R = net->slot(s, net->oR[k]);
    Gemm g = gemm_args(net, skip_half(net, s, k - 1), packed_ptr(net, net->conv[k]), sl(R, net->ch[k]), n, net->Hk[k], net->Wk[k]);
    g.a.bias = conv_bias(net, net->conv[k]);
    GI_TRY(gemm_run(net, 0, g));
    GI_TRY(plain_norm_forward(net, s, net->dnorm[k], R, n, net->Hk[k] * net->Wk[k], skip_half(net, s, k), GI_ACT_LRELU));
  }
  {
    Gemm g = gemm_args(net, skip_half(net, s, nd - 1), packed_ptr(net, net->conv[nd]), up_input(net, s, nd), n, net->Hk[nd], net->Wk[nd]);
    g.a.act_out = GI_ACT_RELU; g.a.bias = conv_bias(net, net->conv[nd]);
    GI_TRY(gemm_run(net, 0, g));
  }
  for (int k = nd; k >= 2; --k) {
    void* U = net->slot(s, net->oU[k]);
    Dropout drop;
    GI_TRY(dropout_prepare(net, s, k, n, false, drop));
    Gemm g = gemm_args(net, up_input(net, s, k), phase_ptr(net, net->up[k]), sl(U, net->ch[k - 1]), n, net->Hk[k], net->Wk[k]);
    if (k < nd) { g.a.relu_in = 1; g.a.relu_cend = net->ch[k]; }
    g.a.bias = conv_bias(net, net->up[k]);
    GI_TRY(gemm_run(net, 1, g));
    GI_TRY(plain_norm_forward(net, s, net->unorm[k], U, n, net->Hk[k - 1] * net->Wk[k - 1], up_half(net, s, k - 1), GI_ACT_RELU, drop));
  }
  return head_forward(net, s, y, n, true);
}

// backward of one normalisation step of the plain generator: dz of [dropout] -> activation, then through InstanceNorm (a: as for act_bn_bwd)
int plain_norm_backward(gi_net* net, int s, const BN& b, ActBnBwdArgs a, void* dx, int n, int hw) {
  if (net->norm_kind != 1) {
    a.x = nullptr;   // no norm: nothing reads the raw tensor
    return act_bn_bwd(net, s, a, dx);
  }
  a.dx = dx;
  return op_act_in_bwd(net->ctx->stream, net->dtype, a, n, hw, (const float*)net->slot(s, net->oInStats) + b.in_off);
}

int unet_backward_plain(gi_net* net, int s, const float* dy, float* dx, int need_wgrad, int phase) {
  const int nd = net->nd, n = net->slot_n[s];
  GI_REQUIRE(n > 0, "unet_backward: slot %d holds no forward", s);
  GI_REQUIRE(net->out_c == 1 || !need_wgrad, "unet_backward: parameter gradients of a %d-channel generator are not built", net->out_c);
  net->bwd_eval = 0;
  auto gC = [&](int k) { return (void*)net->shared(net->ogC[k]); };
  auto gA = [&](int k) { return (void*)net->shared(net->ogA[k]); };
  void* D = net->shared(net->oD);
  const bool dropped = net->slot_train[s] && net->dropout_p > 0.f;
  if (phase == 0 || phase == 1) {
    GI_TRY(head_backward(net, s, dy, need_wgrad));
    for (int k = 1; k <= nd - 1; ++k) {
      const int kk = k + 1, ck = net->ch[k], ca = net->up[kk].ca;
      const int64_t pix = (int64_t)n * net->Hk[k] * net->Wk[k];
      ActBnBwdArgs b = act_bwd_args(up_half(net, s, k), pix, GI_ACT_NONE);
      set_g2(b, sl(gC(k), ck, 2 * ck, ck));
      b.x = net->slot(s, net->oU[kk]);
      if (dropped && kk >= 5 && kk <= nd - 1) b.drop_scale = 1.f / (1.f - net->dropout_p);
      GI_TRY(plain_norm_backward(net, s, net->unorm[kk], b, D, n, net->Hk[k] * net->Wk[k]));
      if (need_wgrad) {
        GI_TRY(bias_grad(net, net->up[kk], D, pix, ck));
        WgradArgs wa = wgrad_args(net, up_input(net, s, kk), sl(D, ck), n, net->Hk[kk], net->Wk[kk], net->grads + net->up[kk].w_off);
        wa.relu_S = kk < nd ? 1 : 0;
        GI_TRY(wgrad_run(net, wa));
      }
      void* gout = (kk == nd) ? (void*)net->shared(net->ogE) : gC(kk);
      GI_TRY(gemm_run(net, 0, gemm_args(net, sl(D, ck), packed_ptr(net, net->up[kk]), sl(gout, ca), n, net->Hk[kk], net->Wk[kk])));
    }
  }
  if (phase == 1) return GI_OK;
  const bool run_inner = phase != 4, run_outer = phase != 3;
  if (run_inner) {
    const int c = net->ch[nd], cb = net->ch[nd - 1];
    const int64_t pix = (int64_t)n * net->Hk[nd] * net->Wk[nd];
    ActBnBwdArgs b = act_bwd_args(up_input(net, s, nd), pix, GI_ACT_NONE);
    set_g2(b, sl(net->shared(net->ogE), c));
    GI_TRY(act_bn_bwd(net, s, b, D));
    if (need_wgrad) {
      GI_TRY(bias_grad(net, net->conv[nd], D, pix, c));
      GI_TRY(wgrad_run(net, wgrad_args(net, sl(D, c), skip_half(net, s, nd - 1), n, net->Hk[nd], net->Wk[nd], net->grads + net->conv[nd].w_off)));
    }
    GI_TRY(gemm_run(net, 1, gemm_args(net, sl(D, c), phase_ptr(net, net->conv[nd]), sl(gA(nd - 1), cb), n, net->Hk[nd], net->Wk[nd])));
  }
  for (int k = nd - 1; k >= 2; --k) {
    if (k >= 5 ? !run_inner : !run_outer) continue;
    const int c = net->ch[k], cb = net->ch[k - 1];
    const int64_t pix = (int64_t)n * net->Hk[k] * net->Wk[k];
    ActBnBwdArgs b = act_bwd_args(skip_half(net, s, k), pix, GI_ACT_LRELU);
    set_g1(b, sl(gA(k), c));
    set_g2(b, sl(gC(k), c, 2 * c));
    b.x = net->slot(s, net->oR[k]);
    GI_TRY(plain_norm_backward(net, s, net->dnorm[k], b, D, n, net->Hk[k] * net->Wk[k]));
    if (need_wgrad) {
      GI_TRY(bias_grad(net, net->conv[k], D, pix, c));
      GI_TRY(wgrad_run(net, wgrad_args(net, sl(D, c), skip_half(net, s, k - 1), n, net->Hk[k], net->Wk[k], net->grads + net->conv[k].w_off)));
    }
    GI_TRY(gemm_run(net, 1, gemm_args(net, sl(D, c), phase_ptr(net, net->conv[k]), sl(gA(k - 1), cb), n, net->Hk[k], net->Wk[k])));
  }
  if (run_outer) {
    const int c = net->ch[1];
    ActBnBwdArgs a1 = act_bwd_args(skip_half(net, s, 1), (int64_t)n * net->Hk[1] * net->Wk[1], GI_ACT_LRELU);
    set_g1(a1, sl(gA(1), c));
    set_g2(a1, sl(gC(1), c, 2 * c));
    GI_TRY(first_layer_tail(net, s, net->conv[1], n, net->Hk[1], net->Wk[1], a1, need_wgrad, dx));
  }
  return GI_OK;
}

// ---------------------------------------------------------------------------------------------
int patchgan_forward(gi_net* net, int s, const float* x, float* y, int n) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, train = net->train, H = net->H, W = net->W;
  if (train) ++net->affine_gen;   // running statistics change below
  GI_REQUIRE(n % net->bn_groups == 0, "patchgan_forward: %d images do not split into %d BatchNorm groups", n, net->bn_groups);
  net->slot_groups[s] = net->bn_groups;
  net->slot_n[s] = n;
  net->slot_train[s] = train;
  const bool fuse_a4 = net->fuse_head && op_head_affine_ok(dt, 512);
  net->slot_fused_u2[s] = fuse_a4 ? 1 : 0;   // (critic: "conv4's activation was not materialised")
  ParamsBack params_back{net, net->params};
  if (net->sn) GI_TRY(sn_enter(net, s, true));
  GI_TRY(op_c1_gather(st, dt, x, net->params + net->dconv[1].w_off, net->slot(s, net->oA[1]), n, H / 2, W / 2, 64, 64, 0, GI_ACT_LRELU, 1.f, nullptr,
                      gi_opt(GI_OPT_MASK_BITS) ? (unsigned long long*)net->slot(s, net->oBits1) : nullptr, &net->slot_bits1[s]));
  bool x_saved = false, a4_deferred = false;
  BnAccArgs a4_acc;
  for (int i = 2; i <= 4; ++i) {
    const Conv& c = net->dconv[i];
    const int Hs = H >> i, Ws = W >> i;
    const int64_t pix = (int64_t)n * Hs * Ws;
    void* R = net->slot(s, net->oRd[i]);
    StatPlan sp = stat_plan(net, net->dbn[i], pix, (pix + 127) / 128, train);
    Gemm g = gemm_args(net, sl(net->slot(s, net->oA[i - 1]), c.cb), packed_ptr(net, c), sl(R, c.ca), n, Hs, Ws);
    with_stats(net, g, sp);
    GI_TRY(gemm_run(net, 0, g));
    BnOpts o;
    if (i == 2) o.side = input_side_copy(net, s, x, n, sp);
    // conv4 feeds only the head: its BatchNorm + LeakyReLU is applied by the head kernels from the raw tensor
    if (i == 4 && fuse_a4 && sp.use && gi_opt(GI_OPT_HEAD_FAST)) {   // the head's first kernel derives conv4's scale / shift itself (HeadArgs::bn)
      a4_acc = bn_acc_args(net, s, net->dbn[i], sp, pix / net->bn_groups, net->bn_groups);
      bn_acc_commit(net, s, net->dbn[i], sp);
      a4_deferred = true;
      continue;
    }
    o.apply = !(i == 4 && fuse_a4);
    GI_TRY(bn_forward(net, s, net->dbn[i], R, pix, g.a.ntiles_out, sl(net->slot(s, net->oA[i]), c.ca), GI_ACT_LRELU, train, sp, o));
    if (o.side.bytes > 0) x_saved = true;
  }
  if (!x_saved) GI_TRY(input_copy(net, s, x, n));
  HeadArgs h;
  h.a4 = net->slot(s, fuse_a4 ? net->oRd[4] : net->oA[4]);
  if (fuse_a4) {
    BNPtrs p = bn_ptrs(net, s, net->dbn[4]);
    h.scale4 = p.scale; h.shift4 = p.shift; h.n_per_group = n / net->bn_groups; h.gstride = 4 * 512;
    if (a4_deferred) h.bn = &a4_acc;
  }
  if (net->oHt >= 0) { h.tbuf = (float*)net->shared(net->oHt); h.tbuf_bytes = net->ht_bytes; }
  h.w5 = net->params + net->w5_off; h.wl = net->params + net->wl_off; h.bl = net->params + net->bl_off;
  h.h = (float*)net->slot(s, net->oHh); h.out = (float*)net->slot(s, net->oOut);
  h.n = n; h.Hh = net->Hh; h.Wh = net->Wh; h.c = 512; h.sigmoid = net->sigmoid;
  h.out2 = y;
  GI_TRY(op_head_forward(st, dt, h));
  return GI_OK;
}

// phase: 0 = whole backward; 1 = head + conv4 block (their gradients, 8.5 of the critic's 11 MB, are the tail of the
// flat buffer and complete when this returns); 2 = conv3 .. conv1
int patchgan_backward(gi_net* net, int s, const float* dy, float* dx, int need_wgrad, int phase = 0) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, H = net->H, W = net->W, n = net->slot_n[s];
  GI_REQUIRE(n > 0 && net->slot_train[s], "patchgan_backward: slot %d holds no train-mode forward", s);
  GI_REQUIRE(net->slot_groups[s] == net->bn_groups, "patchgan_backward: slot %d was produced with %d BatchNorm groups, the net is set to %d", s,
             net->slot_groups[s], net->bn_groups);
  net->bwd_eval = 0;
  HeadBwdArgs hb;
  hb.a4 = net->slot(s, net->oA[4]); hb.w5 = net->params + net->w5_off; hb.wl = net->params + net->wl_off;
  hb.h = (const float*)net->slot(s, net->oHh); hb.out = (const float*)net->slot(s, net->oOut);
  hb.dy = dy; hb.da4 = net->shared(net->ogA[4]);
  hb.dw5 = need_wgrad ? net->grads + net->w5_off : nullptr;
  hb.dwl = need_wgrad ? net->grads + net->wl_off : nullptr;
  hb.dbl = need_wgrad ? net->grads + net->bl_off : nullptr;
  hb.dh = (float*)net->shared(net->oDh);
  hb.scratch = (float*)net->shared(net->oHw); hb.scratch_bytes = net->hw_bytes;
  if (net->slot_fused_u2[s]) {   // the forward left conv4's activation to the head kernels: so does the backward
    BNPtrs p = bn_ptrs(net, s, net->dbn[4]);
    hb.a4 = net->slot(s, net->oRd[4]);
    hb.scale4 = p.scale; hb.shift4 = p.shift; hb.n_per_group = n / net->bn_groups; hb.gstride = 4 * 512;
  }
  hb.n = n; hb.Hh = net->Hh; hb.Wh = net->Wh; hb.c = 512; hb.sigmoid = net->sigmoid; hb.loss_scale = net->loss_scale;
  if (phase != 2) {
    GI_TRY(clear_pending_bwd(net, &net->dbn[2], 3));
    // conv4's BatchNorm-backward sums ride in the head's input-gradient blocks (HeadBwdArgs::bwd_*): no reduce launch
    BwdFuse& p4 = net->bwd_pending[net->dbn[4].id];
    int head_bw = 0;
    p4 = bwd_fuse_plan(net, s, net->dbn[4], net->slot(s, net->oRd[4]), (int64_t)n * net->Hh * net->Wh, (int64_t)n * 4, 0.2f);
    if (p4.planned) {
      hb.bwd_x = p4.x; hb.bwd_scale = p4.scale; hb.bwd_shift = p4.shift; hb.bwd_mean = p4.mean; hb.bwd_inv = p4.inv;
      hb.bwd_stride = p4.stride; hb.bwd_n_per_group = n / (p4.groups > 0 ? p4.groups : 1); hb.bwd_reps = p4.reps_gemm; hb.bwd_slope = p4.slope;
      hb.bwd_acc = p4.acc; hb.bwd_applied = &head_bw;
    }
    GI_TRY(op_head_backward(st, dt, hb));
    p4.applied = head_bw != 0;
  }
  int lrelu1_done = 0;
  C1WFuse c1w;
  const Slice y1 = sl(net->slot(s, net->oA[1]), 64);
  for (int i = 4; i >= 2; --i) {
    if (i == 4 ? phase == 2 : phase == 1) continue;
    const Conv& c = net->dconv[i];
    const int Hs = H >> i, Ws = W >> i;
    const int64_t pix = (int64_t)n * Hs * Ws;
    BwdFuse& pend = net->bwd_pending[net->dbn[i].id];
    void* D = side_dz(net);
    ActBnBwdArgs b = act_bwd_args(sl(net->slot(s, net->oA[i]), c.ca), pix, GI_ACT_LRELU);
    set_g1(b, sl(net->shared(net->ogA[i]), c.ca));
    b.x = net->slot(s, net->oRd[i]);
    GI_TRY(act_bn_bwd(net, s, b, D, &net->dbn[i], need_wgrad, &pend));
    pend = BwdFuse();
    if (need_wgrad)
      GI_TRY(wgrad_run(net, wgrad_args(net, sl(D, c.ca), sl(net->slot(s, net->oA[i - 1]), c.cb), n, Hs, Ws, net->grads + c.w_off)));
    Gemm g = gemm_args(net, sl(D, c.ca), phase_ptr(net, c), sl(net->shared(net->ogA[i - 1]), c.cb), n, Hs, Ws);
    if (i >= 3) {   // the gradient this GEMM produces enters BatchNorm + LeakyReLU of layer i - 1: its reduction rides in the GEMM's epilogue
      BwdFuse& bf = net->bwd_pending[net->dbn[i - 1].id];
      bf = bwd_fuse_plan(net, s, net->dbn[i - 1], net->slot(s, net->oRd[i - 1]), pix * 4, pix / 256 * 4, 0.2f);
      with_bn_bwd(g, bf);
    } else {        // conv1 has no BatchNorm: its LeakyReLU backward and its weight gradient ride in this GEMM where the kernel takes them
      with_first_layer_bwd(net, s, g, y1, need_wgrad, dx != nullptr, c1w);
    }
    GI_TRY(gemm_run(net, 1, g));
    if (i == 2) lrelu1_done = g.a.mask_applied;
  }
  if (phase == 1) return GI_OK;
  ActBnBwdArgs a1 = act_bwd_args(y1, (int64_t)n * (H / 2) * (W / 2), GI_ACT_LRELU);
  set_g1(a1, sl(net->shared(net->ogA[1]), 64));
  return first_layer_tail(net, s, net->dconv[1], n, H / 2, W / 2, a1, need_wgrad, dx, lrelu1_done, &c1w);
}

}  // namespace

namespace {

// WGAN-GP extension (NOT in the reference): accumulates d/dtheta of
//   lam * mean_n ( || grad_x sum_m D(x)_m ||_2 - 1 )^2
// into the bound gradients. Formulation: g = grad_x sum D (one frozen backward); v = d(penalty)/dg;
// d(penalty)/dtheta = d/dtheta [ v . g ] = d/dtheta [ JVP of sum D along v ]. The JVP (tangent forward)
// and the reverse pass over the tangent graph reuse the convolution kernels; BatchNorm in train mode
// couples the tangent to the PRIMAL activations through the batch statistics, which injects a primal
// gradient at every norm layer (op_bn_tangent_inject). Tangent-side and primal-side gradients are
// stacked as a 2n batch so every layer needs one input-gradient GEMM and one weight-gradient GEMM.
// Scaling, both dtypes: the tangent forward runs on v * s (s = 2^k derived on the device, op_gp_direction) and
// the reverse pass is seeded with the loss scale L. Tangent-side gradients (stacked half 0) then carry L, primal-side ones
// (half 1) s * L, and every parameter-gradient product - stacked wgrad, conv1's two halves, the head's dw5 / dwl, dgamma of
// the inject pass, dgamma / dbeta of the primal BatchNorm backward - carries s * L. The kernels remove L where they write fp32
// as in every backward; the gradients land in a private buffer that one fixed-order pass adds into the bound ones times 1/s.
int patchgan_gradient_penalty(gi_net* net, const float* xhat, int n, float lam, float* penalty_out) {
  hipStream_t st = net->ctx->stream;
  const int dt = net->dtype, H = net->H, W = net->W, s = net->gp_slot;
  GI_REQUIRE(!net->sigmoid && net->train, "gradient_penalty: needs a train-mode critic without sigmoid");
  GI_REQUIRE(net->bn_groups == 1, "internal: gradient_penalty runs with one BatchNorm group");
  const int64_t T = (int64_t)net->tsz();
  const float LS = net->loss_scale, iLS = 1.f / LS;
  const int chans[5] = {1, 64, 128, 256, 512};
  auto A2 = [&](int i, int half) { return (void*)(net->shared(net->oA2[i]) + (int64_t)half * n * (H >> i) * (W >> i) * chans[i] * T); };
  auto G2 = [&](int i, int half) { return (void*)(net->shared(net->oG2[i]) + (int64_t)half * n * (H >> i) * (W >> i) * chans[i] * T); };
  float* gimg = (float*)net->shared(net->oGimg);
  float* vimg = (float*)net->shared(net->oVimg);
  float* ones = (float*)net->shared(net->oGPs);
  float* sumsq = ones + (n + 16);
  float* amax = sumsq + (n + 16);
  float* sc = amax + (n + 16);   // s, 1/s
  float* th = (float*)net->shared(net->oTh);
  float* dth = th + (int64_t)n * net->P;
  float* ytmp = sumsq;   // (n) critic outputs, overwritten by sumsq afterwards
  // 1) primal forward + frozen backward: g = d(sum D)/dx. Spectral norm: this forward runs its own power iteration, and every pass
  // below reads the effective parameters it derived
  ParamsBack params_back{net, net->params};
  GI_TRY(patchgan_forward(net, s, xhat, ytmp, n));
  if (net->sn) GI_TRY(sn_enter(net, s, false));
  GI_REQUIRE(!net->slot_fused_u2[s], "internal: gradient_penalty needs conv4's activation materialised");
  hipLaunchKernelGGL(fill_f32_kernel, dim3(1), dim3(256), 0, st, ones, n, 1.0f);
  GI_LAUNCH_CHECK();
  GI_TRY(patchgan_backward(net, s, ones, gimg, 0));
  // 2) penalty value and the scaled direction v * s = s * d(penalty)/dg
  GI_TRY(op_gp_direction(st, gimg, n, (int64_t)H * W, lam, sumsq, amax, vimg, penalty_out, sc));
  // the parameter gradients of steps 3-4 go to the private buffer (gi_net::oGPgrad), added to the bound ones times 1/s at the end
  float* const grads = net->grads;
  float* const gbuf = (float*)net->shared(net->oGPgrad);
  GI_HIP(hipMemsetAsync(gbuf, 0, (size_t)net->n_params * 4, st));
  struct GradsBack { gi_net* net; float* g; ~GradsBack() { net->grads = g; } } grads_back{net, grads};
  net->grads = gbuf;
  // 3) tangent forward
  void* TZ = net->shared(net->oTZ);
  {
    const int64_t cnt = (int64_t)n * (H / 2) * (W / 2) * 64;
    GI_TRY(op_c1_gather(st, dt, vimg, net->params + net->dconv[1].w_off, net->shared(net->oTX[1]), n, H / 2, W / 2, 64, 64, 0, GI_ACT_NONE, 1.f));
    GI_TRY(op_mul_slope(st, dt, net->shared(net->oTX[1]), net->slot(s, net->oA[1]), A2(1, 0), cnt));
    GI_HIP(hipMemcpyAsync(A2(1, 1), net->slot(s, net->oA[1]), cnt * T, hipMemcpyDeviceToDevice, st));
  }
  for (int i = 2; i <= 4; ++i) {
    const Conv& c = net->dconv[i];
    const int Hs = H >> i, Ws = W >> i;
    const int64_t pix = (int64_t)n * Hs * Ws, cnt = pix * c.ca;
    void* TX = net->shared(net->oTX[i]);
    GI_TRY(gemm_run(net, 0, gemm_args(net, sl(A2(i - 1, 0), c.cb), packed_ptr(net, c), sl(TX, c.ca), n, Hs, Ws)));
    ActBnBwdArgs jt = act_bwd_args(sl(TX, c.ca), pix, GI_ACT_NONE);   // BatchNorm Jacobian applied to the tangent
    set_g1(jt, sl(TX, c.ca));
    jt.x = net->slot(s, net->oRd[i]);
    GI_TRY(act_bn_bwd(net, s, jt, TZ, &net->dbn[i]));
    GI_TRY(op_mul_slope(st, dt, TZ, net->slot(s, net->oA[i]), A2(i, 0), cnt));
    GI_HIP(hipMemcpyAsync(A2(i, 1), net->slot(s, net->oA[i]), cnt * T, hipMemcpyDeviceToDevice, st));
  }
  // head: phi = sum_n wl . (w5 * ta4)
  HeadArgs h;
  h.a4 = A2(4, 0); h.w5 = net->params + net->w5_off; h.wl = net->params + net->wl_off; h.bl = net->params + net->bl_off;
  h.h = th; h.out = ytmp; h.n = n; h.Hh = net->Hh; h.Wh = net->Wh; h.c = 512; h.sigmoid = 0;
  GI_TRY(op_head_forward(st, dt, h));
  // 4) reverse pass over the tangent graph (seed d(phi)/d(tz) = L; the Linear bias does not enter phi). dw5 / dwl: the head
  // kernels form them from the unscaled seed and the tangent ta4 / h (s), into fixed-order partials (no float atomics)
  HeadBwdArgs hb;
  hb.a4 = A2(4, 0); hb.w5 = h.w5; hb.wl = h.wl; hb.h = th; hb.out = ytmp; hb.dy = ones; hb.da4 = G2(4, 0);
  hb.dw5 = net->grads + net->w5_off; hb.dwl = net->grads + net->wl_off; hb.dbl = nullptr; hb.dh = dth;
  hb.n = n; hb.Hh = net->Hh; hb.Wh = net->Wh; hb.c = 512; hb.sigmoid = 0; hb.loss_scale = LS;
  hb.scratch = (float*)net->shared(net->oHw); hb.scratch_bytes = net->hw_bytes;
  GI_TRY(op_head_backward(st, dt, hb));
  GI_HIP(hipMemsetAsync(G2(4, 1), 0, (size_t)n * net->Hh * net->Wh * 512 * T, st));   // no primal gradient enters above the head
  char* D2 = net->shared(net->oD2);
  for (int i = 4; i >= 2; --i) {
    const Conv& c = net->dconv[i];
    const int Hs = H >> i, Ws = W >> i;
    const int64_t pix = (int64_t)n * Hs * Ws, half = pix * c.ca * T;
    // tangent-gradient chain: d(tx_i) = J_BN( slope * d(ta_i) )
    ActBnBwdArgs b = act_bwd_args(sl(net->slot(s, net->oA[i]), c.ca), pix, GI_ACT_LRELU);
    set_g1(b, sl(G2(i, 0), c.ca));
    b.x = net->slot(s, net->oRd[i]);
    GI_TRY(act_bn_bwd(net, s, b, D2, &net->dbn[i]));
    // primal chain: standard BatchNorm backward of the gradient arriving from the layer above (dgamma / dbeta: s * L, 1/L removed)
    set_g1(b, sl(G2(i, 1), c.ca));
    GI_TRY(act_bn_bwd(net, s, b, D2 + half, &net->dbn[i], 1));
    // dependence of the BatchNorm Jacobian on the primal input (dgamma: s * L, 1/L removed here)
    BNPtrs bp = bn_ptrs(net, s, net->dbn[i]);
    GI_TRY(op_bn_tangent_inject(st, dt, G2(i, 0), net->slot(s, net->oA[i]), net->shared(net->oTX[i]), net->slot(s, net->oRd[i]), D2 + half, pix,
                                c.ca, net->params + net->dbn[i].gamma_off, bp.mean, bp.inv, net->grads + net->dbn[i].gamma_off, iLS,
                                (float*)net->shared(net->oGPpart), (float*)net->shared(net->oGPsums)));
    // conv_i on the stacked 2n batch: [d(tx_i); dxp_i] x [ta_{i-1}; a_{i-1}] (both products s * L; wgrad removes L)
    GI_TRY(wgrad_run(net, wgrad_args(net, sl(D2, c.ca), sl(A2(i - 1, 0), c.cb), 2 * n, Hs, Ws, net->grads + c.w_off)));
    GI_TRY(gemm_run(net, 1, gemm_args(net, sl(D2, c.ca), phase_ptr(net, c), sl(G2(i - 1, 0), c.cb), 2 * n, Hs, Ws)));
  }
  {
    const int64_t pix = (int64_t)n * (H / 2) * (W / 2), half = pix * 64 * T;
    ActBnBwdArgs b = act_bwd_args(sl(net->slot(s, net->oA[1]), 64), pix, GI_ACT_LRELU);
    set_g1(b, sl(G2(1, 0), 64));
    GI_TRY(act_bn_bwd(net, s, b, D2));
    set_g1(b, sl(G2(1, 1), 64));
    GI_TRY(act_bn_bwd(net, s, b, D2 + half));
    // conv1: tangent half against v * s (L * s), primal half against xhat (s * L)
    GI_TRY(op_c1_wgrad(st, dt, D2, vimg, net->grads + net->dconv[1].w_off, n, H / 2, W / 2, 64, 64, 0, 0, iLS, 1.f, nullptr, (float*)net->shared(net->oPart), net->part_floats));
    GI_TRY(op_c1_wgrad(st, dt, D2 + half, (const float*)net->slot(s, net->oX), net->grads + net->dconv[1].w_off, n, H / 2, W / 2, 64, 64, 0, 0,
                       iLS, 1.f, nullptr, (float*)net->shared(net->oPart), net->part_floats));
  }
  // 5) bound gradients += private buffer * 1/s (spectral norm: projected through this forward's u, v, sigma on the way)
  if (net->sn) return sn_project(net, s, gbuf, grads, 0, net->n_params, sc + 1);
  GI_TRY(op_gp_unscale_add(st, gbuf, sc, grads, net->n_params));
  return GI_OK;
}

}  // namespace

extern "C" int gi_patchgan_gradient_penalty(gi_net* net, const float* xhat, int n, float lam, float* penalty_out) {
  GI_REQUIRE(net && net->bound && net->kind == 1, "gradient_penalty: bound discriminator handle required");
  GI_REQUIRE(xhat && n >= 1 && n <= net->max_n, "gradient_penalty: n=%d (max %d)", n, net->max_n);
  // the interpolates are ONE BatchNorm population whatever the stacked real|fake passes around this call use
  // (gi_net_set_bn_groups): the penalty's primal forward, its backward and the tangent passes all run with one group.
  // The tangent passes read conv4's activation: the penalty's primal forward materialises it (no fp16 head fusion there).
  const int groups = net->bn_groups, fuse_head = net->fuse_head;
  net->bn_groups = 1;
  net->fuse_head = 0;
  const int rc = patchgan_gradient_penalty(net, xhat, n, lam, penalty_out);
  net->bn_groups = groups;
  net->fuse_head = fuse_head;
  return rc;
}

// flat fp32 gradient buffer of a bound handle (comm.hip)
float* gi_net_grads_ptr(gi_net* net, int64_t* floats) {
  if (!net || !net->bound) return nullptr;
  if (floats) *floats = net->n_params;
  return net->grads;
}

extern "C" int gi_net_forward(gi_net* net, int slot, const float* x, float* y, int n) {
  GI_REQUIRE(net && net->bound, "net_forward: net not bound");
  GI_REQUIRE(x && y && n >= 1 && n <= net->max_n, "net_forward: n=%d (max %d)", n, net->max_n);
  GI_REQUIRE(slot >= 0 && slot < net->n_slots, "net_forward: slot=%d", slot);
  if (net->kind == 2) return gi_dcgan_forward(net->dc, net->ctx->stream, net->params, net->ws, slot, x, y, n);
  return net->kind == 0 ? unet_forward(net, slot, x, y, n) : patchgan_forward(net, slot, x, y, n);
}

namespace {
// saved activation (pixels x channels of an NHWC tensor, ld / coff) -> fp32 (n,c,hw). scale != null: src is the RAW
// convolution output of a layer whose normalisation + activation a consumer applies on the fly (C1Affine / HeadArgs::scale4):
// the same fma(x, scale, shift) and activation are applied here (image i of population i / n_per_group, vectors gstride apart)
template <typename T>
__global__ void __launch_bounds__(256) export_act_kernel(const T* __restrict__ src, int ld, int coff, float* __restrict__ out, int n, int c, int hw,
                                                         const float* __restrict__ scale, const float* __restrict__ shift, int act,
                                                         int n_per_group, int gstride) {
  const int64_t total = (int64_t)n * c * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int p = (int)(i % hw);
    const int64_t t = i / hw;
    const int ch = (int)(t % c);
    const int64_t img = t / c;
    float v = (float)src[(img * hw + p) * ld + coff + ch];
    if (scale) {
      const int g = n_per_group > 0 ? (int)(img / n_per_group) : 0;
      v = fmaf(v, scale[(int64_t)g * gstride + ch], shift[(int64_t)g * gstride + ch]);
      v = act == GI_ACT_RELU ? fmaxf(v, 0.f) : (act == GI_ACT_LRELU ? (v > 0.f ? v : 0.2f * v) : v);
      v = (float)(T)v;
    }
    out[i] = v;
  }
}
}  // namespace

// Debug: the split-K tile tickets of this network (igemm7 / igemm fix-up hand-off) that are NOT zero. Every launch leaves them zero (the
// last arriver of a tile resets its ticket); a non-zero ticket between launches means a launch was cut short and the next split-K
// layer would mis-count its arrivals. Synchronises the context's stream.
extern "C" int gi_net_debug_nonzero_tickets(gi_net* net, int* count) {
  GI_REQUIRE(net && net->bound && count, "debug_nonzero_tickets: net not bound / null output");
  *count = 0;
  if (net->oTickets < 0) return GI_OK;
  std::vector<unsigned> h(GI_IGEMM_TICKETS);
  GI_HIP(hipMemcpyAsync(h.data(), net->shared(net->oTickets), (size_t)GI_IGEMM_TICKETS * 4, hipMemcpyDeviceToHost, net->ctx->stream));
  GI_HIP(hipStreamSynchronize(net->ctx->stream));
  for (unsigned v : h) *count += v != 0;
  return GI_OK;
}

namespace {
// slot: a user slot, or a critic's gp_slot (gi_patchgan_gp_saved_activation)
int saved_activation(gi_net* net, int slot, int kind, int level, float* out_nchw, int64_t count) {
  GI_REQUIRE(net->slot_n[slot] > 0, "saved_activation: slot %d holds no forward", slot);
  GI_REQUIRE(!(net->kind == 0 && net->slot_inference[slot]), "saved_activation: slot %d holds an inference forward (nothing saved)", slot);
  const int n = net->slot_n[slot];
  const void* src = nullptr;
  int ld = 0, coff = 0, c = 0, hw = 0, act = GI_ACT_NONE, npg = 0, gstride = 0;
  const float* scale = nullptr; const float* shift = nullptr;
  if (net->kind == 0) {
    const int nd = net->nd;
    GI_REQUIRE((kind == 0 && level >= 1 && level <= nd) || (kind == 1 && level >= 1 && level <= nd - 1),
               "saved_activation: generator kind=%d level=%d (kind 0: 1..%d, kind 1: 1..%d)", kind, level, nd, nd - 1);
    c = net->ch[level]; hw = net->Hk[level] * net->Wk[level];
    if (kind == 0 && level == nd) { src = net->slot(slot, net->oE); ld = c; }
    else {
      src = net->slot(slot, net->oC[level]); ld = 2 * c; coff = kind ? c : 0;
      if (kind == 1 && level == 1 && net->slot_fused_u2[slot]) {   // never materialised: the head applies it on the fly
        BNPtrs p = bn_ptrs(net, slot, net->unorm[2]);
        src = net->slot(slot, net->oU[2]); ld = c; coff = 0; scale = p.scale; shift = p.shift; act = GI_ACT_RELU;
      }
    }
  } else {
    GI_REQUIRE(kind == 0 && level >= 1 && level <= 4, "saved_activation: discriminator kind=%d level=%d (kind 0, 1..4)", kind, level);
    const int chans[5] = {1, 64, 128, 256, 512};
    c = chans[level]; hw = (net->H >> level) * (net->W >> level); ld = c;
    src = net->slot(slot, net->oA[level]);
    if (level == 4 && net->slot_fused_u2[slot]) {
      BNPtrs p = bn_ptrs(net, slot, net->dbn[4]);
      src = net->slot(slot, net->oRd[4]); scale = p.scale; shift = p.shift; act = GI_ACT_LRELU;
      npg = n / net->slot_groups[slot]; gstride = 4 * 512;
    }
  }
  GI_REQUIRE(count == (int64_t)n * c * hw, "saved_activation: count %lld != n*c*h*w = %lld", (long long)count, (long long)n * c * hw);
  hipStream_t st = net->ctx->stream;
  if (net->dtype == GI_F16)
    hipLaunchKernelGGL(export_act_kernel<half_t>, dim3(grid1d(count)), dim3(256), 0, st, (const half_t*)src, ld, coff, out_nchw, n, c, hw, scale, shift,
                       act, npg, gstride);
  else
    hipLaunchKernelGGL(export_act_kernel<float>, dim3(grid1d(count)), dim3(256), 0, st, (const float*)src, ld, coff, out_nchw, n, c, hw, scale, shift,
                       act, npg, gstride);
  GI_LAUNCH_CHECK();
  return GI_OK;
}
}  // namespace

extern "C" int gi_net_saved_activation(gi_net* net, int slot, int kind, int level, float* out_nchw, int64_t count) {
  GI_REQUIRE(net && net->bound && out_nchw, "saved_activation: net not bound / null output");
  if (net->kind == 2) {
    GI_REQUIRE(slot >= 0 && slot < net->n_slots, "saved_activation: slot=%d", slot);
    return gi_dcgan_saved(net->dc, net->ctx->stream, net->ws, slot, kind, level, out_nchw, count);
  }
  GI_REQUIRE(slot >= 0 && slot < net->n_slots && net->slot_n[slot] > 0, "saved_activation: slot %d holds no forward", slot);
  return saved_activation(net, slot, kind, level, out_nchw, count);
}

extern "C" int gi_patchgan_gp_saved_activation(gi_net* net, int level, float* out_nchw, int64_t count) {
  GI_REQUIRE(net && net->bound && net->kind == 1 && out_nchw, "gp_saved_activation: bound discriminator handle / output required");
  GI_REQUIRE(net->slot_n[net->gp_slot] > 0, "gp_saved_activation: no gradient penalty has run on this handle");
  return saved_activation(net, net->gp_slot, 0, level, out_nchw, count);
}

extern "C" int gi_net_sn_read(gi_net* net, int slot, float* sigma6, float* eff_params, int64_t count) {
  GI_REQUIRE(net && net->bound && net->kind == 1 && net->sn, "sn_read: bound discriminator handle with spectral norm required");
  GI_REQUIRE(slot >= 0 && slot <= net->n_slots && net->slot_sn_gen[slot] > 0, "sn_read: slot %d holds no forward", slot);
  hipStream_t st = net->ctx->stream;
  if (sigma6) GI_HIP(hipMemcpyAsync(sigma6, sn_slot_sigma(net, slot), 6 * 4, hipMemcpyDeviceToDevice, st));
  if (eff_params) {
    GI_REQUIRE(count == net->n_params, "sn_read: count %lld != %lld parameter floats", (long long)count, (long long)net->n_params);
    GI_REQUIRE(net->sn_eff_gen == net->slot_sn_gen[slot], "sn_read: the effective parameters in the workspace belong to another forward");
    GI_HIP(hipMemcpyAsync(eff_params, net->shared(net->oSnEff), (size_t)count * 4, hipMemcpyDeviceToDevice, st));
  }
  return GI_OK;
}

// backward_joined for a critic with spectral norm whose slot holds a forward
static int backward_joined_sn(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad, int phase) {
  ParamsBack params_back{net, net->params};
  struct GradsBack { gi_net* net; float* g; ~GradsBack() { net->grads = g; } } grads_back{net, net->grads};
  const int64_t split = net->dconv[4].w_off, lo = phase == 1 ? split : 0, hi = phase == 2 ? split : net->n_params;
  GI_TRY(sn_enter(net, slot, false));
  if (need_wgrad) {
    float* priv = (float*)net->shared(net->oSnGrad);
    GI_HIP(hipMemsetAsync(priv + lo, 0, (size_t)(hi - lo) * 4, net->ctx->stream));
    net->grads = priv;
  }
  GI_TRY(side_begin(net, need_wgrad));
  const int rc = patchgan_backward(net, slot, dy, dx, need_wgrad, phase);
  const int rj = side_join(net);
  if (rc != GI_OK || rj != GI_OK) return rc != GI_OK ? rc : rj;
  if (need_wgrad) return sn_project(net, slot, net->grads, grads_back.g, lo, hi, nullptr);
  return GI_OK;
}

// weight gradients on the second stream (side_begin), joined before the caller sees the gradients
static int backward_joined(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad, int phase) {
  if (net->kind == 2)
    return gi_dcgan_backward(net->dc, net->ctx->stream, net->params, net->grads, net->ws, slot, dy, dx, need_wgrad, net->loss_scale, phase);
  // spectral norm: the backward differentiates the forward's effective weights (re-derived from the slot's sigma when a later
  // forward has replaced them) into the private buffer; after the join the projection folds that into the bound gradients
  if (net->sn && net->slot_n[slot] > 0) return backward_joined_sn(net, slot, dy, dx, need_wgrad, phase);
  GI_TRY(side_begin(net, need_wgrad));
  const int rc = net->kind == 0 ? unet_backward(net, slot, dy, dx, need_wgrad, phase) : patchgan_backward(net, slot, dy, dx, need_wgrad, phase);
  const int rj = side_join(net);
  return rc != GI_OK ? rc : rj;
}

extern "C" int gi_net_backward(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad) {
  GI_REQUIRE(net && net->bound, "net_backward: net not bound");
  GI_REQUIRE(dy, "net_backward: dy is null");
  GI_REQUIRE(slot >= 0 && slot < net->n_slots, "net_backward: slot=%d", slot);
  return backward_joined(net, slot, dy, dx, need_wgrad, 0);
}

extern "C" int gi_net_backward_phase(gi_net* net, int slot, const float* dy, float* dx, int need_wgrad, int phase) {
  GI_REQUIRE(net && net->bound, "net_backward_phase: net not bound");
  GI_REQUIRE(dy, "net_backward_phase: dy is null");
  GI_REQUIRE(slot >= 0 && slot < net->n_slots, "net_backward_phase: slot=%d", slot);
  GI_REQUIRE(phase >= 0 && phase <= 4, "net_backward_phase: phase=%d", phase);
  if (net->kind != 0 && phase >= 3) return GI_OK;   // discriminator: two phases
  return backward_joined(net, slot, dy, dx, need_wgrad, phase);
}

// first float of the gradient region completed by phase 1 (generator: the innermost up-conv weight; discriminator:
// the conv4 weight)
extern "C" int64_t gi_net_phase_split(gi_net* net) {
  if (!net) return GI_ERR_INVALID;
  if (net->kind == 2) return gi_dcgan_phase_split(net->dc);
  if (net->kind != 0) return net->dconv[4].w_off;
  return net->up[net->nd].w_off;
}
// generator: first float of the region completed by phase 3 (the level-5 down-conv weight); phases 3 + 4 == phase 2
extern "C" int64_t gi_net_phase_split2(gi_net* net) {
  if (!net) return GI_ERR_INVALID;
  if (net->kind != 0) return 0;
  return net->conv[net->nd < 5 ? net->nd : 5].w_off;
}
