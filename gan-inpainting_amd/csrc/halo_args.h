// Kernel arguments of the halo-resident implicit GEMMs (igemm5.hip: igemm5 / igemm6; igemm8.hip), filled by fill_halo_args below.
#pragma once
#include <stdlib.h>

#include "igemm_plan.h"

struct KP5 {
  const char* in;
  const char* w;      // [4 phases][cout][4*cin] (K order: tap, channel)
  char* out;
  const char* zero;
  const float* bias;
  float* partials;
  unsigned long long* stat_acc; int stat_pg, stat_reps;   // IgemmArgs::stat_acc
  int Hs, Ws, n;      // the small grid (MODE 1: input, MODE 0: output)
  int TH, TW;         // patch of the small grid, TH*TW = 256; TW a power of two
  int tiles_x, tiles_per_img, mtiles;
  int cin, ldin, coffin;
  int cout, ldout, coffout;
  int nchunk;         // cin / 64
  int relu_in, relu_cend, act_out;
  int ntiles;
  const char* mask; int ldmask, coffmask; float mask_slope;   // fused activation backward (IgemmArgs::mask)
  const char* add; int ldadd, coffadd;
  const unsigned long long* mask_bits;   // IgemmArgs::mask_bits (igemm8, MODE 3 only; else null)
  // IgemmArgs::c1w_* (igemm8, MODE 3 with mask_bits only): the weight gradient of the single-channel layer below, from the tile
  const float* c1w_img; float* c1w_part; float c1w_scale; int c1w_skip_out;
  // fused BatchNorm-backward reduction (IgemmArgs::bwd_*)
  const char* bwd_x; int bwd_ldx;
  const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; const float* bwd_inv; int bwd_stride;
  float bwd_slope;
  int bwd_c0, bwd_c;   // IgemmArgs::bwd_c0 / bwd_c (igemm8 only; igemm6: 0 / cout)
  unsigned long long* bwd_acc; int bwd_reps; int bwd_pg_tiles;   // bwd_pg_tiles: M tiles per BatchNorm population (0: one population)
  int pool;           // MODE 2: the epilogue stores the 2x2 max pool of the tile (IgemmArgs::pool2)
  int dbg_epi;        // builds with -DGI_ABLATION only (GI_EPI_DBG): 1 = all tiles store into one 64 KiB window (no HBM write burst)
};

// KP5 from the layer + its plan (plan_halo, igemm_plan.hip); GI_ERR_HIP without the zero page
static inline int fill_halo_args(KP5& kp, const IgemmPlan& p, const IgemmArgs& a) {
  kp = KP5{};
  kp.in = (const char*)a.in; kp.w = (const char*)a.w; kp.out = (char*)a.out; kp.zero = gi_igemm_zero_page();
  if (!kp.zero) { gi_set_error("igemm5: no zero page"); return GI_ERR_HIP; }
  kp.bias = a.bias; kp.partials = a.stat_acc ? nullptr : a.partials;
  kp.stat_acc = a.stat_acc; kp.stat_pg = a.stat_pg; kp.stat_reps = a.stat_reps > 0 ? a.stat_reps : 1;
  kp.Hs = a.Hs; kp.Ws = a.Ws; kp.n = a.n; kp.TH = p.TH; kp.TW = p.TW;
  kp.tiles_x = a.Ws / p.TW; kp.tiles_per_img = kp.tiles_x * (a.Hs / p.TH); kp.mtiles = p.mtiles;
  kp.cin = a.cin; kp.ldin = a.ldin; kp.coffin = a.coffin;
  kp.cout = a.cout; kp.ldout = a.ldout; kp.coffout = a.coffout;
  kp.nchunk = a.cin / 64;
  kp.relu_in = a.relu_in; kp.act_out = a.act_out;
  kp.relu_cend = a.relu_cend > 0 ? a.relu_cend : a.cin;
  kp.ntiles = p.ntiles;
  kp.mask = (const char*)a.mask; kp.ldmask = a.ldmask; kp.coffmask = a.coffmask; kp.mask_slope = a.mask_slope;
  kp.add = a.mask ? (const char*)a.add : nullptr; kp.ldadd = a.ldadd; kp.coffadd = a.coffadd;
  if (p.take_mask_bits) kp.mask_bits = a.mask_bits;
  if (p.take_c1w) { kp.c1w_img = a.c1w_img; kp.c1w_part = a.c1w_part; kp.c1w_scale = a.c1w_scale; kp.c1w_skip_out = a.c1w_skip_out; }
  kp.bwd_c = a.cout;
  if (p.take_bwd) {
    const int64_t px_per_tile = 256 * (p.mode == 0 ? 1 : 4);          // output pixels per M tile over all phases
    kp.bwd_x = (const char*)a.bwd_x; kp.bwd_ldx = a.bwd_ldx;
    kp.bwd_scale = a.bwd_scale; kp.bwd_shift = a.bwd_shift; kp.bwd_mean = a.bwd_mean; kp.bwd_inv = a.bwd_inv; kp.bwd_stride = a.bwd_stride;
    kp.bwd_slope = a.bwd_slope; kp.bwd_acc = a.bwd_acc; kp.bwd_reps = a.bwd_reps > 0 ? a.bwd_reps : 1;
    kp.bwd_pg_tiles = a.bwd_pg > 0 ? (int)(a.bwd_pg / px_per_tile) : 0;
    if (p.bwd_range) { kp.bwd_c0 = a.bwd_c0; kp.bwd_c = a.bwd_c; }
  }
  kp.pool = p.take_pool ? 1 : 0;
#ifdef GI_ABLATION
  { const char* e = getenv("GI_EPI_DBG"); if (e) kp.dbg_epi = atoi(e); }
#endif
  return GI_OK;
}
