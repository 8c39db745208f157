// The implicit-GEMM dispatch: gi_igemm_plan decides which kernel serves a layer (dtype -> mode -> family -> tile -> split) and
// op_igemm launches it. Candidates are tried in the order halo-resident kernels (igemm8 / igemm6 / igemm5) -> igemm3 -> igemm7 ->
// generic kernel; a candidate that does not serve the shape answers NEXT. DESIGN.md section 4 has the same order as a table.
#include "igemm_plan.h"

namespace {

constexpr int NEXT = 1;   // not this family: try the next candidate (never leaves this file)

// the name of a family's table row (igemm_plan.h)
#define GI_NAME3(V, A, B, NAME) case V: return NAME;
#define GI_NAME4(V, A, B, C, NAME) case V: return NAME;
#define GI_NAME_FN(FN, ROWS) const char* FN(int variant) { switch (variant) { ROWS } return ""; }
GI_NAME_FN(name3, GI_IGEMM3_KERNELS(GI_NAME3))
GI_NAME_FN(name5, GI_IGEMM5_KERNELS(GI_NAME3) GI_IGEMM5_DUAL_KERNEL(GI_NAME3))
GI_NAME_FN(name6, GI_IGEMM6_KERNELS(GI_NAME4))
GI_NAME_FN(name7, GI_IGEMM7_KERNELS(GI_NAME3) GI_IGEMM7_FOLD_NAMES(GI_NAME3))
GI_NAME_FN(name8, GI_IGEMM8_KERNELS(GI_NAME4))

// ---- igemm8 / igemm6 / igemm5 (igemm5.hip, igemm8.hip): a TH x TW patch of the small grid per workgroup, input halo resident in LDS
int plan_halo(int mode, const IgemmArgs& a, IgemmPlan& p) {
  if (!gi_is_pow2(a.Ws) || a.Ws < 8) return NEXT;
  const int TW = a.Ws < 32 ? a.Ws : 32, TH = 256 / TW;
  if (a.Hs % TH != 0) return NEXT;
  if (mode == 2 ? (TH + 2) * (TW + 2) > 384 : (TH + 1) * (TW + ((mode == 1 && a.cout % 128 != 0) ? 2 : 1)) > 320) return NEXT;   // the halo must fit its LDS rows
  int BN = (a.cout % 128 == 0) ? 128 : 64;
  const int nph = mode == 1 ? 4 : 1;
  const int mtiles = a.n * (a.Ws / TW) * (a.Hs / TH);
  if (mode != 2 && mtiles * (a.cout / BN) * nph < 128) return NEXT;   // too few tiles to fill 256 CUs: igemm7's split-K serves those layers
  if (mode == 0 && BN == 128 && mtiles * (a.cout / BN) < 256) {
    // 128..255 workgroups on 256 CUs (generator d4 at 256x256, bs=32): 64-wide N tiles double them
    if (gi_tune("GI_IGEMM5_NARROW", 1)) BN = 64;
  }
  const bool dual = mode == 1 && BN == 64;     // 64-channel N tiles: both px phases per workgroup (MODE 3)
  const int64_t in_px = (int64_t)a.n * a.Hs * a.Ws * (mode == 0 ? 4 : 1), out_px = (int64_t)a.n * a.Hs * a.Ws * (mode == 1 ? 4 : 1);
  GI_REQUIRE(in_px * a.ldin < (1ll << 31) && out_px * a.ldout < (1ll << 31), "igemm5: tensor too large for 32-bit offsets");
  GI_REQUIRE(!a.stat_acc || a.stat_pg == 0 || a.stat_pg % (a.Hs * a.Ws) == 0, "igemm5: stat_pg=%d must be whole images", a.stat_pg);
  if (a.mask) {
    GI_REQUIRE(a.ldmask % 8 == 0 && a.coffmask % 8 == 0 && out_px * a.ldmask < (1ll << 31), "igemm5: mask layout");
    GI_REQUIRE(!a.add || (a.ldadd % 8 == 0 && a.coffadd % 8 == 0 && out_px * a.ldadd < (1ll << 31)), "igemm5: add layout");
  }
  p.take_mask = a.mask != nullptr;
  p.mode = dual ? 3 : mode; p.bn = BN; p.dual = dual; p.relu = a.relu_in != 0;
  p.TH = TH; p.TW = TW; p.mtiles = mtiles; p.ntiles = a.cout / BN;
  p.grid = ((mtiles + 7) / 8) * 8 * p.ntiles * (dual ? 2 : nph);
  p.ntiles_out = mtiles * nph;
  p.stat_to_acc = a.stat_acc != nullptr;
  const int BNk = dual ? 128 : BN;             // columns of the workgroup tile
  const int epi = 256 * (BNk + 8) * 2 + 4 * BNk * 8;
  // igemm8 (igemm8.hip): the same tile on four waves, two workgroups per CU. GI_IGEMM8: 0 off, 1 (default) layers whose grid
  // gives every CU at least two workgroups (with one per CU half the wave slots stay empty: measured d3 / u4 / critic conv4,
  // 256 workgroups, 10 - 16 % slower than igemm6; every layer with >= 512 workgroups 3 - 16 % faster), 2 every eligible layer
  // GI_IGEMM6=0 (the first-generation halo kernels: no buffer-descriptor LDS-DMA anywhere) switches igemm8 off as well
  const int use6 = gi_opt(GI_OPT_IGEMM6), use8 = use6 ? gi_opt(GI_OPT_IGEMM8) : 0;
  const bool fits31 = in_px * a.ldin * 2 < (1ll << 31) && (int64_t)a.cout * (mode == 1 ? 4 : (mode == 2 ? 9 : 16)) * a.cin * 2 * (dual ? 2 : 1) < (1ll << 31);
  // (the 3x3 mode: 128-column tiles on 32-wide patches, no fused input ReLU; VGG-19 from conv2_1 to conv4_4)
  const bool take8 = use8 && (mode != 2 || (TW == 32 && !a.relu_in)) && (dual || BN == 128 || mode == 2) && a.cin % (mode == 0 ? 64 : 32) == 0 && TW >= 16 &&
      fits31 && !(mode == 0 && a.relu_in) && (use8 >= 2 || p.grid >= gi_tune("GI_IGEMM8_MINGRID", 512));
  // fused BatchNorm-backward reduction (the dual-px / 64-column tiles do not take it; nor a launch with a mask; a column range only igemm8)
  p.bwd_range = a.bwd_c > 0 && (a.bwd_c0 != 0 || a.bwd_c != a.cout);
  if (a.bwd_acc && !a.mask && mode != 2 && a.cout % 128 == 0 && BN == 128 && (!p.bwd_range || (take8 && a.bwd_c0 % 128 == 0 && a.bwd_c % 128 == 0 && a.bwd_c0 + a.bwd_c <= a.cout))) {
    const int64_t px_per_tile = 256 * (mode == 1 ? 4 : 1);          // output pixels per M tile over all phases
    GI_REQUIRE(a.bwd_ldx % 8 == 0 && out_px * a.bwd_ldx < (1ll << 31) && (a.bwd_pg == 0 || a.bwd_pg % px_per_tile == 0) && a.coffout == 0,
               "igemm5: fused BatchNorm-backward reduction: layout");
    p.take_bwd = true;
  }
  if (take8) {
    if (mode == 2 && a.pool2 && !a.mask && !a.stat_acc && !a.partials) {   // the pooled store: igemm8's 3x3 mode only
      GI_REQUIRE(a.coffout == 0 && (int64_t)a.n * (a.Hs / 2) * (a.Ws / 2) * a.ldout < (1ll << 31), "igemm8: pooled output layout");
      p.take_pool = true;
    }
    p.take_mask_bits = dual && !a.relu_in && a.mask && a.mask_bits && a.cout == 64 && !a.bias && a.act_out == GI_ACT_NONE && !a.stat_acc && !a.partials;
    p.take_c1w = p.take_mask_bits && a.c1w_part && a.c1w_img && mtiles % 8 == 0 && a.c1w_part_floats >= (int64_t)p.grid * 1024 &&
                 (int64_t)a.n * 16 * a.Hs * a.Ws < (1ll << 31);
    p.family = GI_FAM_IGEMM8;
    p.variant = mode == 2 ? (BN == 64 ? 7 : 6) : (dual ? 2 : mode) * 2 + (p.relu ? 1 : 0);
    // 4-tap modes: = the epilogue's 256 x 136 halves + 4 x 128 x 2 floats; 3x3 with 64 output channels (VGG conv1_2): 64-column weight stages
    p.lds_bytes = p.variant == 7 ? 2 * 22528 + 4 * 4096 : (mode == 2 ? 2 * 22528 : 2 * 20480) + 4 * 8192;
    p.lds_attr_bytes = p.lds_bytes;
    p.name = name8(p.variant);
  } else if (use6 && mode != 2 && fits31 && !(mode == 0 && a.relu_in)) {
    // GI_IGEMM6=0: the first-generation halo kernels (also the fallback beyond 2^31-byte tensors)
    const int lds6 = 2 * 320 * 128 + 4 * BNk * 128;
    p.family = GI_FAM_IGEMM6;
    p.variant = (dual ? 4 : (BN == 64 ? 2 : 0) + mode) * 2 + (p.relu ? 1 : 0);
    p.lds_bytes = lds6 > epi ? lds6 : epi;
    p.lds_attr_bytes = 160 * 1024;
    p.name = name6(p.variant);
  } else {
    const int ring = 2 * (mode == 2 ? 384 : 320) * 128 + 3 * BNk * 128;
    p.family = GI_FAM_IGEMM5;
    p.variant = dual ? 6 : (BN == 64 ? 3 : 0) + mode;
    p.lds_bytes = ring > epi ? ring : epi;
    p.lds_attr_bytes = 160 * 1024;
    p.name = name5(p.variant);
  }
  return GI_OK;
}

// ---- igemm3 (igemm3.hip): 256 x BN tiles, three-stage LDS-DMA ring, A gathered tap by tap
int plan_igemm3(int mode, const IgemmArgs& a, IgemmPlan& p) {
  const int M = a.n * a.Hs * a.Ws;
  const int nph = mode == 1 ? 4 : 1;
  int BN = (a.cout % 128 == 0) ? 128 : 64;
  if (mode != 2) {   // too few tiles to fill 256 CUs: the split-K kernels serve those layers
    const int tiles = ((M + 255) / 256) * (a.cout / BN) * nph;
    if (tiles < 128) return NEXT;
    // 128..255 tiles leave CUs idle (one 8-wave workgroup per CU): 64-wide N tiles double the workgroups
    if (gi_tune("GI_IGEMM3_NARROW", 1) && BN == 128 && tiles < 256) BN = 64;
  }
  GI_REQUIRE(!a.stat_acc || a.stat_pg == 0 || a.stat_pg % 256 == 0, "igemm3: stat_pg=%d must be a multiple of 256", a.stat_pg);
  const int64_t in_px = (int64_t)M * (mode == 0 ? 4 : 1), out_px = (int64_t)M * nph;
  GI_REQUIRE(in_px * a.ldin < (1ll << 31) && out_px * a.ldout < (1ll << 31), "igemm3: tensor too large for 32-bit offsets");
  p.family = GI_FAM_IGEMM3; p.mode = mode; p.bn = BN;
  p.variant = (BN == 64 ? 3 : 0) + mode;
  p.mtiles = (M + 255) / 256; p.ntiles = a.cout / BN;
  p.grid = ((p.mtiles + 7) / 8) * 8 * p.ntiles * nph;
  const int ring = 3 * (256 + BN) * 128, epi = 256 * (BN + 8) * 2 + 4 * BN * 8;
  p.lds_bytes = ring > epi ? ring : epi;
  p.lds_attr_bytes = 3 * (256 + 128) * 128;
  p.stat_to_acc = a.stat_acc != nullptr;
  p.ntiles_out = p.mtiles * nph;
  p.name = name3(p.variant);
  return GI_OK;
}

// ---- igemm7 (igemm7.hip): small-M layers, 128 x BN tiles, four-stage ring, split-K reduced by the last arriver of a tile
int plan_igemm7(int mode, const IgemmArgs& a, IgemmPlan& p) {
  if (a.cin % 64 != 0 || a.cout % 64 != 0) return NEXT;
  if (!gi_opt(GI_OPT_IGEMM7)) return NEXT;   // GI_IGEMM7=0: igemm.hip serves these layers
  int max_split = gi_tune("GI_IGEMM7_MAXSPLIT", 8);   // (measured: d7 20.6 us with 16 splits, 18.6 us with 8: the last arriver's tail)
  if (max_split < 1) max_split = 8;
  const int M = a.n * a.Hs * a.Ws;
  const int nph = mode == 1 ? 4 : 1;
  const int mtiles = (M + 127) / 128;
  int BN = (a.cout % 128 == 0 && mtiles * (a.cout / 128) * nph >= 64) ? 128 : 64;   // fewer than 64 tiles of 128 x 128: 64-wide N tiles
  {   // GI_IGEMM7_BN (ablation build): force the N tile
    const int force_bn = gi_tune("GI_IGEMM7_BN", 0);
    if (force_bn == 64 || (force_bn == 128 && a.cout % 128 == 0)) BN = force_bn;
  }
  const int ntiles = a.cout / BN;
  const int tiles = mtiles * ntiles * nph;
  const int nk = (mode == 1 ? 4 : 16) * a.cin / 64;
  int splitk = (256 + tiles - 1) / tiles;
  if (splitk > max_split) splitk = max_split;
  if (splitk > nk / 8) splitk = nk / 8;   // at least 8 K tiles per split (u7: 21.7 us with 4 tiles per split, 17.9 us with 8)
  if (splitk < 1) splitk = 1;
  const int kps = (nk + splitk - 1) / splitk;
  splitk = (nk + kps - 1) / kps;
  if (splitk > 1 && (!a.tickets || !a.ws || tiles > GI_IGEMM_TICKETS || a.ws_bytes < (int64_t)splitk * tiles * 128 * BN * 4)) return NEXT;
  // Folded normalisation (IgemmFold): taken when ONE workgroup can normalise a channel column in about the time the separate pass
  // spends before its first byte moves (a dependent launch + the accumulator reads: ~5 us): the column finisher reads and writes
  // out_pixels x BN halves at 60 - 100 GB/s (one CU, other workgroups' rows: guides/MI355X_MICROARCH.md "handoff-payload"), i.e.
  // ~1.5 us per 64 KiB each way. The column tickets are the last 32 of the GI_IGEMM_TICKETS words.
  constexpr int COL_TICKETS = 32;
  const int64_t out_pixels = (int64_t)M * nph;
  const int64_t col_bytes = out_pixels * BN * 2;
  p.fold = a.fold && gi_opt(GI_OPT_BN_FOLD) && a.stat_acc && a.fold->bn.groups == 1 && a.fold->bn.acc == a.stat_acc && a.tickets &&
           ntiles <= COL_TICKETS && tiles <= GI_IGEMM_TICKETS - COL_TICKETS && col_bytes <= (int64_t)gi_tune("GI_FOLD_MAX_KB", 256) * 1024 &&
           out_pixels * a.ldout * 2 < (1ll << 31) && out_pixels * a.fold->lddst * 2 < (1ll << 31) && a.ldout % 8 == 0 && a.coffout % 8 == 0 &&
           a.fold->lddst % 8 == 0 && a.fold->coffdst % 8 == 0 && (a.fold->act == GI_ACT_RELU || a.fold->act == GI_ACT_LRELU || a.fold->act == GI_ACT_NONE);
  GI_REQUIRE(!a.stat_acc || a.stat_pg == 0 || a.stat_pg % 128 == 0, "igemm7: stat_pg=%d must be a multiple of 128", a.stat_pg);
  GI_REQUIRE((int64_t)M * (mode == 0 ? 4 : 1) * a.ldin < (1ll << 31) && out_pixels * a.ldout < (1ll << 31), "igemm7: tensor too large for 32-bit offsets");
  p.family = GI_FAM_IGEMM7; p.mode = mode; p.bn = BN;
  p.variant = (BN == 64 ? 2 : 0) + mode;
  p.splitk = splitk; p.kt_per_split = kps;
  p.mtiles = mtiles; p.ntiles = ntiles;
  const int nyz = ntiles * nph * splitk;
  p.grid = mtiles >= 8 ? ((mtiles + 7) / 8) * 8 * nyz : mtiles * nyz;
  // shipped choice, measured on d5 / d6 / d7 / u7 / u6 at the headline batch (tools/r4_small.sh, profiles/r04_igemm7_variants.txt):
  // four stages and one split per tail iteration. A six-stage ring on the 64-column tiles (four K tiles in flight) ran 3 - 5 us
  // SLOWER per layer (the five-tile prologue burst of every CU delays the first tile by more than the deeper ring gains), two or
  // four splits of the tail in flight changed nothing (+-0.5 us): the tail's round trips are not what these launches wait for.
  p.nstg = gi_tune("GI_IGEMM7_NSTG", 4); p.pf = gi_tune("GI_IGEMM7_PF", 1);
  if (BN == 128 || p.nstg != 6) p.nstg = 4;
  if (p.pf != 2 && p.pf != 4) p.pf = 1;
  // waves per workgroup (kernel header): eight unless the folded normalisation is asked for (the four-wave kernel's) or GI_IGEMM7_WAVES=4
  p.nw = (p.fold || gi_opt(GI_OPT_IGEMM7_WAVES) == 4) ? 4 : 8;
  const int ring = p.nstg * (128 + BN) * 128, epi = 128 * (BN + 8) * 2 + 4 * BN * 8;
  p.lds_bytes = ring > epi ? ring : epi;
  p.lds_attr_bytes = 144 * 1024;
  p.stat_to_acc = a.stat_acc != nullptr;
  p.ntiles_out = mtiles * nph;
  p.name = name7(p.variant + (p.fold ? 4 : 0));
  return GI_OK;
}

// ---- the register-staged kernel of igemm.hip: every dtype and every shape the others leave; split-K for small M
int plan_generic(int dtype, int mode, const IgemmArgs& a, IgemmPlan& p) {
  if (dtype != GI_F16 && dtype != GI_F32) { gi_set_error("igemm: bad dtype %d", dtype); return GI_ERR_INVALID; }
  const bool f16 = dtype == GI_F16;
  const int EPC = f16 ? 8 : 4, BK = 8 * EPC;
  GI_REQUIRE(a.cin % BK == 0, "igemm: cin=%d must be a multiple of %d", a.cin, BK);
  GI_REQUIRE(a.cout % 64 == 0, "igemm: cout=%d must be a multiple of 64", a.cout);
  GI_REQUIRE(a.ldin % EPC == 0 && a.coffin % EPC == 0 && a.ldout % EPC == 0 && a.coffout % EPC == 0,
             "igemm: leading dims / channel offsets must be 16-byte aligned");
  const int phases = mode ? 4 : 1, M = a.n * a.Hs * a.Ws;
  const int nk = (mode ? 4 : 16) * a.cin / BK;
  const int64_t in_elems = (int64_t)M * (mode ? 1 : 4) * a.ldin, out_pixels = (int64_t)M * phases;
  GI_REQUIRE(in_elems < (1ll << 31) && out_pixels * a.ldout < (1ll << 31), "igemm: tensor too large for 32-bit offsets");
  const bool wide = (a.cout % 128 == 0);
  int BM = wide ? 128 : 256, BN = wide ? 128 : 64;
  int mt = (M + BM - 1) / BM, nt = a.cout / BN;
  int tiles = mt * nt * phases;
  int splitk = 1;
  // in-kernel fix-up: the last arriver reads splits x tile bytes on ONE CU (~100 GB/s), so the split count is capped
  // and very small M gets 128 x 64 tiles instead (twice the workgroups for the same tail)
  int fix_max = gi_tune("GI_IGEMM_FIX_MAXSPLIT", 8);
  if (fix_max < 2) fix_max = 8;
  // GI_IGEMM_FIXUP=0: finish-kernel path
  bool fixup = gi_opt(GI_OPT_IGEMM_FIXUP) && a.tickets && a.ws && a.force_splitk == 0 && tiles < 256 && nk >= 8;
  bool half_n = false;
  if (fixup) {
    if (wide && tiles * fix_max < 256) { half_n = true; BN = 64; nt = a.cout / BN; tiles = mt * nt * phases; }
    splitk = (256 + tiles - 1) / tiles;
    if (splitk > fix_max) splitk = fix_max;
    if (splitk > nk / 4) splitk = nk / 4;
    if (splitk < 1) splitk = 1;
    if (tiles > GI_IGEMM_TICKETS || a.ws_bytes < (int64_t)splitk * tiles * BM * BN * 4) {
      fixup = false; splitk = 1;
      if (half_n) { half_n = false; BN = 128; nt = a.cout / BN; tiles = mt * nt * phases; }
    }
  }
  if (fixup) {
  } else if (a.force_splitk > 0) splitk = a.force_splitk;
  else if (tiles < 256 && nk >= 8) {   // fewer workgroups than CUs: split the reduction
    splitk = (gi_tune("GI_IGEMM_SPLIT_BLOCKS", 384) + tiles - 1) / tiles;   // workgroups to aim for
    if (splitk > nk / 4) splitk = nk / 4;
    if (splitk > 64) splitk = 64;
    if (splitk < 1) splitk = 1;
  }
  if (splitk > 1 && (a.ws == nullptr || a.ws_bytes < out_pixels * a.cout * 4)) splitk = 1;
  p.kt_per_split = (nk + splitk - 1) / splitk;
  p.splitk = (nk + p.kt_per_split - 1) / p.kt_per_split;
  p.fixup = fixup && p.splitk > 1;
  p.finish_launch = p.splitk > 1 && !p.fixup;
  // scratch for one buffer per split: plain stores + a summing finish pass (deterministic, no memset);
  // otherwise fp32 atomics into a single zeroed buffer
  p.atomics_ws = p.finish_launch && a.ws_bytes < (int64_t)p.splitk * out_pixels * a.cout * 4;
  GI_REQUIRE(!a.stat_acc || a.stat_pg == 0 || a.stat_pg % 256 == 0, "igemm: stat_pg=%d must be a multiple of 256", a.stat_pg);
  p.family = GI_FAM_GENERIC; p.mode = mode ? 1 : 0; p.bn = BN; p.BM = BM; p.half_n = half_n;
  p.mtiles = mt; p.ntiles = nt; p.grid = mt * nt * phases * p.splitk;
  p.stat_to_acc = a.stat_acc != nullptr;
  p.ntiles_out = mt * phases;
  if (p.finish_launch) {
    const int RL = 256 / (a.cout / 4) > 0 ? 256 / (a.cout / 4) : 1;   // row lanes per block
    int rpb = 64;
    while (rpb > RL && (out_pixels + rpb - 1) / rpb < 256) rpb >>= 1;   // fill the chip on small tensors
    if (rpb < RL) rpb = RL;
    GI_REQUIRE(a.cout <= 1024, "igemm split-K finish: cout=%d > 1024", a.cout);
    p.finish_rows = rpb; p.finish_blocks = (int)((out_pixels + rpb - 1) / rpb);
    p.stat_to_acc = a.stat_acc && !a.partials;   // few rows per block: partial rows + finalize are cheaper there than 4 atomics per channel
    p.ntiles_out = p.finish_blocks;
  }
  p.name = f16 ? (p.fixup ? "igemm<f16,fixup>" : (p.splitk > 1 ? "igemm<f16,splitk>" : "igemm<f16>"))
               : (p.fixup ? "igemm<f32,fixup>" : (p.splitk > 1 ? "igemm<f32,splitk>" : "igemm<f32>"));
  return GI_OK;
}

}  // namespace

int gi_igemm_plan(int dtype, int mode, const IgemmArgs& a, IgemmPlan* p) {
  *p = IgemmPlan{};
  // mode 2 (VGG-19's 3x3 convolutions, fp16) enters below GI_IGEMM_VARIANT and knows the LDS-DMA kernels only.
  // GI_IGEMM_VARIANT: 3 = LDS-DMA kernels (default), 1 = the register-staged kernel only (what fp32 and a forced split always run)
  const bool dma = mode == 2 || (dtype == GI_F16 && a.force_splitk == 0 && gi_opt(GI_OPT_IGEMM_VARIANT) >= 3);
  int rc = NEXT;
  if (dma && a.cin % 64 == 0 && a.cout % 64 == 0 && a.cin <= 2048) {
    const int use5 = gi_opt(GI_OPT_IGEMM5);   // GI_IGEMM5: bit 0 / 1 / 2 = halo-resident kernel for mode 1 / 0 / 2 (default all)
    if ((mode == 1 && (use5 & 1)) || (mode == 0 && (use5 & 2)) || (mode == 2 && (use5 & 4))) rc = plan_halo(mode, a, *p);
    if (rc == NEXT) rc = plan_igemm3(mode, a, *p);
  }
  if (rc == NEXT && mode == 2) return GI_ERR_UNSUPPORTED;   // the caller (vgg.hip) reports the shape
  if (rc == NEXT && dma) rc = plan_igemm7(mode, a, *p);     // small-M layers: deep LDS-DMA ring + in-kernel split-K reduction
  if (rc == NEXT) rc = plan_generic(dtype, mode, a, *p);
  return rc;
}

// mode: 0 = Conv2d 4x4/s2/p1 gather, 1 = sub-pixel phases (ConvTranspose2d forward / Conv2d dgrad),
//       2 = Conv2d 3x3/s1/p1 (VGG features, fp16; weights [cout][9*cin], tap-major)
int op_igemm(hipStream_t st, int dtype, int mode, IgemmArgs& a) {
  IgemmPlan p;
  GI_TRY(gi_igemm_plan(dtype, mode, a, &p));
  switch (p.family) {
    case GI_FAM_IGEMM3: GI_TRY(launch_igemm3(st, p, a)); break;
    case GI_FAM_IGEMM5: case GI_FAM_IGEMM6: GI_TRY(launch_igemm5(st, p, a)); break;
    case GI_FAM_IGEMM7: GI_TRY(launch_igemm7(st, p, a)); break;
    case GI_FAM_IGEMM8: GI_TRY(launch_igemm8(st, p, a)); break;
    default: GI_TRY(launch_igemm(st, dtype, p, a)); break;
  }
  gi_note_kernel(p.name);
  if (p.fold) gi_note_fold();
  gi_igemm_returns(p, a);
  return GI_OK;
}

// the (returned) fields of IgemmArgs; a family leaves alone what it knows nothing about (callers pre-set those to 0)
void gi_igemm_returns(const IgemmPlan& p, IgemmArgs& a) {
  a.stat_used = p.stat_to_acc ? 1 : 0;
  a.ntiles_out = p.ntiles_out;
  if (p.family == GI_FAM_IGEMM7) a.fold_applied = p.fold ? 1 : 0;
  if (p.family == GI_FAM_IGEMM5 || p.family == GI_FAM_IGEMM6 || p.family == GI_FAM_IGEMM8) {
    if (p.take_mask) a.mask_applied = 1;
    if (p.take_bwd) a.bwd_applied = 1;
    a.c1w_applied = p.take_c1w ? 1 : 0; a.c1w_blocks = p.take_c1w ? p.grid : 0;
    a.pool_applied = p.take_pool ? 1 : 0;
  }
}
