// Which implicit-GEMM kernel serves a layer (igemm_plan.hip: the ONLY place that decides), and what the files that own the
// kernels need to launch it. op_igemm = gi_igemm_plan -> launch_igemmN (fills its kernel arguments from IgemmArgs + plan).
#pragma once
#include "common.h"

enum { GI_FAM_GENERIC = 0, GI_FAM_IGEMM3, GI_FAM_IGEMM5, GI_FAM_IGEMM6, GI_FAM_IGEMM7, GI_FAM_IGEMM8 };

struct IgemmPlan {
  int family;                  // GI_FAM_*
  int variant;                 // row of the family's kernel table below
  int mode, bn;                // kernel MODE (0 gather, 1 sub-pixel phases, 2 3x3 / s1, 3 both px phases per workgroup), N tile
  bool dual, relu;
  int nw, nstg, pf;            // igemm7: waves per workgroup; ring stages / tail prefetch (ablation build: GI_IGEMM7_NSTG / _PF)
  int BM; bool half_n;         // generic kernel: M tile, 128 x 64 tiles for very small M
  int splitk, kt_per_split;
  bool fixup, finish_launch, atomics_ws;   // generic split-K: last-arriver reduction | finish launch (per-split buffers | fp32 atomics)
  bool fold, take_mask, take_mask_bits, take_c1w, take_bwd, bwd_range, take_pool, stat_to_acc;
  int TH, TW, mtiles, ntiles, grid, lds_bytes, lds_attr_bytes, ntiles_out;
  int finish_rows, finish_blocks;          // generic finish launch
  const char* name;            // gi_note_kernel string
};
// GI_OK, or GI_ERR_INVALID with the message set; mode 2 (3x3 / s1): GI_ERR_UNSUPPORTED when no kernel serves the shape.
// Host arithmetic only: reads IgemmArgs (pointers for null-ness), gi_opt() and gi_tune().
int gi_igemm_plan(int dtype, int mode, const IgemmArgs& a, IgemmPlan* p);

// the (returned) fields of IgemmArgs from the plan
void gi_igemm_returns(const IgemmPlan& p, IgemmArgs& a);

int launch_igemm(hipStream_t st, int dtype, const IgemmPlan& p, const IgemmArgs& a);   // igemm.hip
int launch_igemm3(hipStream_t st, const IgemmPlan& p, const IgemmArgs& a);             // igemm3.hip
int launch_igemm5(hipStream_t st, const IgemmPlan& p, const IgemmArgs& a);             // igemm5.hip: igemm5 and igemm6
int launch_igemm7(hipStream_t st, const IgemmPlan& p, const IgemmArgs& a);             // igemm7.hip
int launch_igemm8(hipStream_t st, const IgemmPlan& p, const IgemmArgs& a);             // igemm8.hip
// the zero page padding taps read (igemm3.hip), for the current device; null: GI_ERR_HIP
const char* gi_igemm3_zero_page(int dev);
static inline const char* gi_igemm_zero_page() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? gi_igemm3_zero_page(dev) : nullptr; }

// Kernel tables, written once: X(variant, template arguments ..., name). The plan picks the row, the launcher instantiates it.
// (Rows are in the order the kernels have always been instantiated in: it is the order of the functions in the code object.)
#define GI_IGEMM3_KERNELS(X) /* (MODE, BN) */ \
  X(0, 0, 128, "igemm3<0,128>") X(1, 1, 128, "igemm3<1,128>") X(2, 2, 128, "igemm3<2,128>") \
  X(3, 0, 64, "igemm3<0,64>") X(4, 1, 64, "igemm3<1,64>") X(5, 2, 64, "igemm3<2,64>")
#define GI_IGEMM5_KERNELS(X) /* (MODE, BN) */ \
  X(0, 0, 128, "igemm5<0,128>") X(1, 1, 128, "igemm5<1,128>") X(2, 2, 128, "igemm5<2,128>") \
  X(3, 0, 64, "igemm5<0,64>") X(4, 1, 64, "igemm5<1,64>") X(5, 2, 64, "igemm5<2,64>")
#define GI_IGEMM5_DUAL_KERNEL(X) X(6, 3, 128, "igemm5<3,128>")
#define GI_IGEMM6_KERNELS(X) /* (MODE, BN, RELU); variant = (dual ? 4 : (BN == 64 ? 2 : 0) + mode) * 2 + relu */ \
  X(0, 0, 128, false, "igemm6<0,128>") X(2, 1, 128, false, "igemm6<1,128>") X(3, 1, 128, true, "igemm6<1,128,relu>") \
  X(4, 0, 64, false, "igemm6<0,64>") X(6, 1, 64, false, "igemm6<1,64>") X(7, 1, 64, true, "igemm6<1,64,relu>") \
  X(8, 3, 128, false, "igemm6<3,128>") X(9, 3, 128, true, "igemm6<3,128,relu>")
#define GI_IGEMM7_KERNELS(X) /* (PHASE, BN); + 4: with the folded normalisation */ \
  X(0, 0, 128, "igemm7<0,128>") X(1, 1, 128, "igemm7<1,128>") X(2, 0, 64, "igemm7<0,64>") X(3, 1, 64, "igemm7<1,64>")
#define GI_IGEMM7_FOLD_NAMES(X) X(4, 0, 128, "igemm7<0,128>+bn") X(5, 1, 128, "igemm7<1,128>+bn") X(6, 0, 64, "igemm7<0,64>+bn") X(7, 1, 64, "igemm7<1,64>+bn")
#define GI_IGEMM8_KERNELS(X) /* (MODE, RELU, BN); variant = (dual ? 2 : mode) * 2 + relu, 3x3: 6, with 64 output channels 7 */ \
  X(7, 2, false, 64, "igemm8<2,64>") X(0, 0, false, 128, "igemm8<0>") X(1, 0, true, 128, "igemm8<0,relu>") X(2, 1, false, 128, "igemm8<1>") \
  X(3, 1, true, 128, "igemm8<1,relu>") X(4, 3, false, 128, "igemm8<3>") X(5, 3, true, 128, "igemm8<3,relu>") X(6, 2, false, 128, "igemm8<2>")
