// irx — the plan of one gemm() call: which kernel runs it, with which tiles, K splits and tile order, and which of the
// requested epilogue features that kernel honours.  gemm_plan() is a pure function of the arguments and the option
// globals (no HIP call, no allocation; gemm_plan.cpp is host-only).  gemm() launches from the plan and every gemm_*
// query of ops.h reads the same plan, so a caller that sizes buffers from a query in a dry run (models.cpp) and the
// launch that follows cannot decide differently.
#pragma once
#include "ops.h"

namespace irx {

// ------------------------------------------------------------ constants the policy shares with the kernels
constexpr int kSplitCounters = 1 << 16;   // split-K arrival tickets per stream (gemm2.hip): tiles of an in-kernel reduction
constexpr int kRedGnRows = 64;   // rows per GroupNorm partial of splitk_reduce_gn_kernel (the 8x8-level convs: one image)
constexpr int kHaloWMax = 64;    // widest image row a halo tile takes (LDS: 2 x (BM + 2W) x 2BK B)
constexpr int kStripW = 32;      // strip halo tiles (HALO == 5 / 7): 8 rows x 32 columns
constexpr int kSkK = 320;        // the one K the streaming kernel (gemm_sk.hip) takes

enum GemmPath {
  GEMM_WAVE4 = 0,     // 4-wave kernel (gemm.hip)
  GEMM_WAVE4_SPLIT,   // ... with small-M K splits + the reduce kernel
  GEMM_SK,            // K = 320 streaming kernel (gemm_sk.hip)
  GEMM_HALO,          // large tiles, halo conv (gemm2.hip, HALO != 0)
  GEMM_LARGE,         // large tiles, dense / im2col (gemm2.hip)
};

struct GemmPlan {
  int path = GEMM_WAVE4;
  // gemm2_kernel instantiation (GEMM_HALO / GEMM_LARGE)
  int BM = 0, BN = 0, WM = 0, WN = 0, BK = 0, S = 0, HALO = 0;
  bool PP = false;
  // split-K: `per` K steps (of BK; halo: taps x slabs) per split, fp32 partials [batch * splits][Mp][Np] of ws_bytes,
  // reduced by the last arriving split (inkernel) or by the reduce kernel
  int splits = 1, per = 0, Mp = 0, Np = 0;
  bool inkernel = false;
  size_t ws_bytes = 0;
  // what gemm_workspace_bytes reports: an upper bound over the paths (the large-tile splits or the 4-wave kernel's
  // small-M splits, before the large-tile path's alignment exits)
  size_t ws_reserve = 0;
  // tile order and epilogue form (GemmArgs::vec_epilogue / nmajor / group_m)
  bool vec_epilogue = false;
  int nmajor = 0, group_m = 0;
  // the features the arguments request that this path honours (a feature not requested reads 0 / false)
  int gn_rows = 0;         // rows per GroupNorm partial (GemmArgs::gn_part; 0: none)
  bool ln_fold = false;    // folded LayerNorm (ln_rs / ln_part)
  bool ln_out = false;     // LayerNorm partials out (ln_out)
  bool bimg = false;       // per-image B / bias (b_rows)
  bool up2 = false;        // sub-pixel store (up2_w)
  bool geglu = false;      // fused GEGLU (geglu)
  bool gn_fused = false;   // GroupNorm-fused operand (gn_ab)
  bool large() const { return path == GEMM_HALO || path == GEMM_LARGE; }
};

GemmPlan gemm_plan(const GemmArgs& a);

// one integer per gemm2_kernel instantiation (the launcher's switch, gemm2.hip)
constexpr long gemm2_key(int BM, int BN, int WM, int WN, int BK, int S, int HALO, bool PP) {
  return ((((((long)BM * 1000 + BN) * 10 + WM) * 10 + WN) * 100 + BK) * 10 + S) * 100 + HALO * 2 + (PP ? 1 : 0);
}

// gemm2.hip: launches a GEMM_HALO / GEMM_LARGE plan
void gemm_large_tile(const GemmArgs& a, const GemmPlan& p, hipStream_t s);

}  // namespace irx
