// irx — tile / split / path policy of gemm(): gemm_plan() and the gemm_* queries that read it (gemm_plan.h).
// Host-only: no HIP call, no allocation; everything here is a function of the arguments and the options below.
#include "gemm_plan.h"

#include <algorithm>
#include <cmath>

namespace irx {

// ------------------------------------------------------------------ options (irx_set_option)
bool g_large_tiles = true;   // irx_set_option("large_tiles", 0) forces the 4-wave kernel (A/B tests)
int g_large_mask = 3;    // irx_set_option("large_mask", m): bit 0 dense GEMMs, bit 1 convs take the large tiles
int g_large_dense = 63;  // irx_set_option("large_dense", m): dense classes on large tiles: 1 N <= 1280, 2 head-split,
                         // GEGLU at K 4: 320, 16: 640, 32: >= 1280, 8 other
int g_small_splitk = 1;  // 1 (default): small-M, long-K 4-wave GEMMs in K splits + the reduce kernel
// irx_set_option("gemm_sk", m): 1 (default) the GEGLU projection only, 3 every K = 320 shape, 2 GEGLU on the one-wave-
// per-SIMD form, 0 none.  Measured (profiles/r03_kprof_sk_n.txt, M = 65536): GEGLU 179 vs 214 us on the large-tile
// kernel; the N = 320 / 960 projections 32 / 37 / 74 vs 27 / 34 / 66 us — one wave per SIMD with the B slice in
// registers leaves the MFMA pipe 14 % busy behind AGPR -> VGPR operand copies and the epilogue's VALU work
// (profiles/r03_pmc_sk_*.txt), so those stay on the large-tile kernel
int g_gemm_sk = 1;
int g_gemm_deep = 0;    // irx_set_option("gemm_deep", m): 0 two-stage BK 64, 1 BK-32 ring, 2 BK-64 3/4-stage ring
bool g_gemm_small = false;   // irx_set_option("gemm_small", 1): 4-wave 128x160 / 128x128 tiles for K <= kmax
int g_gemm_small_kmax = 1280;
int g_gemm_force = 0;            // irx_set_option("gemm_force", BM*100000 + BN*100 + splits): tuning sweeps
bool g_tile_256x320 = true;      // irx_set_option("tile_256x320", 0): no 256x320 tiles (A/B)
bool g_splitk_inkernel = true;   // irx_set_option("splitk_inkernel", 0): separate split-K reduce kernel (A/B)
int g_gemm_nmajor = 1;   // 0 M-major tile order, 1 N-major where B outweighs A (default), 2 always N-major
int g_gemm_group = 1;    // irx_set_option("gemm_group", 0): the M-major / N-major dense tile orders only (A/B);
                         // g >= 2: groups of g M tiles whatever the cost model says (tests)
// irx_set_option("gemm_pp", m): ping-pong main loops.  Non-zero (default 2): the lean dense form on whole 256x256
// tiles (the 32x32 / 16x16-level GEGLU projections: ff1 -12 / -14 % at the kbench shapes, 49.9 -> 46.5 ms/step in the
// bench; profiles/r04_kbench_gemm_pp_lean.txt) and the long-K two-source chains of gemm_pp_chain; 0: none (A/B)
int g_gemm_pp = 2;
// irx_set_option("gemm_pp2", m): the lean ping-pong loop on 256x128 / 128x256 tiles built for two resident 8-wave
// blocks per CU (72 KiB of LDS, <= 128 VGPRs): one block's ring fill, load waits and epilogue run beside the other's
// MFMA phases.  1 (default): the shapes of pair_tile() below; 0: none (A/B); 2 / 3: 256x128 / 128x256 wherever the
// kernel's conditions hold (kbench, tests: also K % 32 == 0 instead of K % 64 == 0)
int g_gemm_pp2 = 1;
int g_gemm_pp_chain = 1;   // irx_set_option("gemm_pp_chain", 0): the two-source 1x1 chains on the two-stage loop (A/B)
int g_conv1x1_dense = 1;   // irx_set_option("conv1x1_dense", 0): 1x1 convs on the im2col conv path (A/B)
int g_conv_halo = 1;     // irx_set_option("conv_halo", m): 0 im2col walk for every conv (A/B),
                         // 1 halo tiles where the grid fills the chip, 2 wherever they fit (tests)
int g_halo_split = 1;    // irx_set_option("halo_split", 0): no K-split halo tiles (A/B)
int g_halo_pipe = 1;     // irx_set_option("halo_pipe", 0): the round-2 halo main loop (A/B)
// irx_set_option("halo_strip", m): 0 no strip tiles (VAE / 768^2 convs on the im2col walk, A/B), 1 (default) strip
// tiles where whole-row tiles do not fit (W > 64 or no power of two), 2 strip tiles wherever the shape allows (tests:
// strips == rows bit for bit at W <= 64)
int g_halo_strip = 1;
int g_halo_up2 = 1;      // irx_set_option("halo_up2", 0): upsampler parity convs on the im2col walk (A/B)
int g_halo_mi = 1;       // irx_set_option("halo_mi", 0): the 8x8-level convs on the im2col walk (A/B)
int g_halo_group = 1;    // irx_set_option("halo_group", 0): M-major halo tile order (A/B)
int g_gn_fuse = 0;   // measured slower: the halo normalisation's VALU work does not hide under the MFMAs
int g_gn_parts = 1;      // 1: producers emit GroupNorm partial sums, the stats pass is skipped (0: A/B)
int g_gn_red_parts = 1;  // irx_set_option("gn_red_parts", 0): split-K reduce kernels do not emit GroupNorm partials (A/B)
int g_gn_fold = 1;       // 1: the transformer GroupNorm folded into per-image proj_in weights (0: gn_apply, A/B)
int g_ln_fold = 1;       // 1: 16-bit UNets fold LayerNorm into the following projections (read at model creation)
// transformer producers emit LayerNorm partials, the statistics pass is skipped: 0 off (A/B), 1 at C == 320 only (final
// pairs; the default), 2 at every width (C = 640 / 1280: per-tile partials merged by the consumer blocks — 2.2 ms/step
// faster in the same-box A/B, short of the 3 x spread the default asks for: DESIGN.md §22)
int g_ln_parts = 1;

namespace {

constexpr int kCUs = 256;
constexpr long kPairMinTiles = 2L * kCUs;   // two pair tiles (option gemm_pp2) per CU

struct Choice {
  int BM = 0, BN = 0, splits = 1, per = 0;
  bool small = false;   // 4-wave block, two resident per CU (short-K GEMMs: one block's prologue/epilogue
                        // overlaps the other's MFMA loop)
  bool pair = false;    // 8-wave ping-pong block, two resident per CU (pair_tile)
};

int step_k() { return g_gemm_deep == 1 ? 32 : 64; }   // K depth of one pipeline stage (eligibility granule)

// rows (M x batch) the policy plans for: image-indexed GEMMs at kCanonImages images (batch invariance)
long canon_rows(const GemmArgs& a) {
  const long rows = (long)a.M * a.batch;
  return a.imgs > 0 ? rows / a.imgs * kCanonImages : rows;
}
int canon_batch(const GemmArgs& a) { return (a.imgs > 0 && a.batch > 1) ? kCanonImages : a.batch; }

// K splits > 1: the last arriving split reduces in the kernel (and runs the full epilogue), else the reduce kernel.
// In-kernel reduction wins at 2 splits; with more, the serial last-arriver tail loses to the reduce kernel.
bool reduce_in_kernel(int splits, long tiles) { return g_splitk_inkernel && splits == 2 && tiles <= kSplitCounters; }

Choice choose(const GemmArgs& a) {
  Choice best;
  const int nk = std::max(1, a.K / step_k());   // (K < 64: the forced pair tiles of option gemm_pp2 only)
  if (g_gemm_small && g_gemm_deep == 0 && a.K <= g_gemm_small_kmax) {
    const int bn = (!a.geglu && a.N % 160 == 0) ? 160 : (a.N % 128 == 0 ? 128 : 0);
    if (bn) {
      best.BM = 128; best.BN = bn; best.small = true; best.splits = 1; best.per = nk;
      return best;
    }
  }
  if (g_gemm_force > 0 && g_gemm_deep == 0) {   // tuning sweeps: BM*100000 + BN*100 + splits
    const int BM = g_gemm_force / 100000, BN = (g_gemm_force / 100) % 1000, sp = g_gemm_force % 100;
    const bool ok = (BM == 256 || BM == 128 || (BM == 64 && BN == 320 && sp == 1 && !a.gn_part)) &&
                    (BN == 320 || BN == 256 || BN == 128) && a.N % BN == 0 &&
                    sp >= 1 && (sp == 1 || !((a.out_f32 && canon_batch(a) > 1) || a.geglu)) && (!a.geglu || BN % 128 == 0);
    if (ok) {
      best.BM = BM; best.BN = BN; best.splits = sp; best.per = (nk + sp - 1) / sp;
      if ((long)(sp - 1) * best.per < nk) return best;
    }
    best = Choice();
  }
  double best_score = -1.0;
  const int cands[7][2] = {{256, 320}, {256, 256}, {128, 320}, {256, 128}, {128, 256}, {128, 128}, {256, 160}};
  for (auto& c : cands) {
    const int BM = c[0], BN = c[1];
    if (BN == 160 && g_gemm_deep != 2) continue;
    if (BN == 320 && BM == 256 && (g_gemm_deep != 0 || !g_tile_256x320)) continue;
    if (a.N % BN != 0) continue;
    if (a.geglu && BN % 128 != 0) continue;      // tiles must hold whole (value, gate) block pairs
    const long tiles = (canon_rows(a) + BM - 1) / BM * (a.N / BN);
    // per-tile efficiency at full occupancy, calibrated on the batch-16 UNet / batch-8 VAE shapes
    // (scripts/gemm_sweep.py): the load path (L2 -> LDS-DMA) bounds the small tiles, 128x128 keeps two
    // blocks per CU resident (its prologue / epilogue overlap the other block's loop), 256x128 (4x2 waves)
    // loses to it everywhere measured
    const double eff = BM == 256 ? (BN >= 256 ? 1.0 : BN == 160 ? 0.9 : 0.65)
                                 : (BN == 320 ? 0.97 : BN == 256 ? 0.75 : 0.78);
    const int resident = (BM == 128 && BN == 128 && g_gemm_deep == 0) ? 2 : 1;
    const long cap = (long)kCUs * resident;
    for (int splits = 1; splits <= 8; splits *= 2) {
      if (splits > 1 && ((a.out_f32 && canon_batch(a) > 1) || a.geglu)) break;
      const int per = (nk + splits - 1) / splits;
      if (per * step_k() < 512 && splits > 1) break;    // keep >= 512 of K per split
      if ((long)(splits - 1) * per >= nk) break;        // no empty split
      const long blocks = tiles * splits;
      const double util = (double)blocks / ((double)((blocks + cap - 1) / cap) * cap);
      // split-K pays an fp32 partial write + read per split and a reduction tail, relatively more when
      // each split is short
      const double cost_split = splits > 1 ? (1.0 + 0.35 * std::log2((double)splits)) * (per < 16 ? 1.6 : 1.0) : 1.0;
      const double score = util * eff / cost_split;
      if (score > best_score + 1e-9) {
        best_score = score;
        best.BM = BM; best.BN = BN; best.splits = splits; best.per = per;
      }
    }
  }
  return best;
}

bool vec_ok(const GemmArgs& a) {
  return !a.out_f32 && a.N % 8 == 0 && a.ldc % 8 == 0 && ((uintptr_t)a.C % 16) == 0 &&
         (!a.residual || (a.ldr % 8 == 0 && ((uintptr_t)a.residual % 16) == 0)) &&
         (a.batch == 1 || (a.sC % 8 == 0 && (!a.residual || a.sR % 8 == 0)));
}

// What the two-per-CU ping-pong tiles (gemm2.hip, PAIR) compile out or never handle: convs, a second A source, K
// splits (the caller checks), per-image weights, row add, GroupNorm / LayerNorm partials, sub-pixel rows
bool pair_form(const GemmArgs& a) {
  return g_gemm_pp2 && g_gemm_pp && g_gemm_deep == 0 && !g_gemm_small && g_gemm_force == 0 && !a.conv && !a.A1 &&
         !a.b_rows && !a.rowadd && !a.gn_part && !a.gn_ab && !a.ln_out && !a.up2_w && a.K % 32 == 0;
}

// The pair tile (BM, BN) that replaces the choice `c` of a dense GEMM, or false.  A function of the canonical shape
// only (canon_rows, N, K, feature flags), never of the actual batch.
bool pair_tile(const GemmArgs& a, const Choice& c, int& BM, int& BN) {
  if (!pair_form(a)) return false;
  int bm = 256, bn = 128;   // (BM 256: the per-image row tile rules of the fused GEGLU / LayerNorm fold read as before)
  if (g_gemm_pp2 >= 2) {    // (forced: one K split whatever `choose` gave)
    if (g_gemm_pp2 == 3) { bm = 128; bn = 256; }
  } else {
    // the shapes that won their kbench: the fused GEGLU projections `choose` gave 256x256 tiles, from
    // one tile per CU (the GELU pass is the VALU work the partner block hides); the wide K >= 640 projections on
    // 128x320 tiles (q|k|v at 32^2) from two per CU.  Plain 256x256 calls (q|k|v at 16^2) did not resolve, N = 640
    // with 1.25 tiles per CU lost: both stay
    if (c.splits != 1 || a.K % 64 != 0) return false;
    const long tiles = canon_rows(a) / bm * (a.N / bn);
    const bool geglu = a.geglu && c.BM == 256 && c.BN == 256 && tiles >= kCUs;
    const bool wide = !a.geglu && c.BM == 128 && c.BN == 320 && a.K >= 640 && tiles >= kPairMinTiles;
    if (!geglu && !wide) return false;
  }
  if (a.M % bm != 0 || a.N % bn != 0) return false;
  BM = bm; BN = bn;
  return true;
}

bool eligible(const GemmArgs& a) {
  const int bk = (g_gemm_pp2 >= 2 && pair_form(a)) ? 32 : step_k();
  if (!(g_large_mask & (a.conv ? 2 : 1))) return false;   // (A/B: large tiles for dense GEMMs / convs only)
  if (!a.conv && g_large_dense != 63) {   // (diagnostics: dense classes on large tiles)
    const int cls = a.geglu ? (a.K <= 320 ? 4 : a.K <= 640 ? 16 : 32) : a.hs_L ? 2 : a.N <= 1280 ? 1 : 8;
    if (!(g_large_dense & cls)) return false;
  }
  if (a.hs_L && !vec_ok(a)) return false;  // head-split stores: the 16-byte LDS-staged epilogue only
  if (a.act != ACT_NONE) return false;   // activations are fused by the 4-wave kernel only (tiny GEMMs)
  // the unrolled scalar (non-16-byte) epilogue only scales and adds bias: row add / residual need vec rows
  if (!vec_ok(a) && (a.rowadd || a.residual)) return false;
  if (a.rowadd && (a.rowadd_ld % 4 != 0 || ((uintptr_t)a.rowadd % 16) != 0)) return false;
  if (!is16(a.dtype) || a.K % bk != 0 || a.ldb % 8 != 0) return false;
  if (canon_rows(a) < 512) return false;           // tiny outputs: the 64x64 4-wave tiles waste less
  if (a.geglu && (a.out_f32 || a.residual || a.batch != 1 || a.N % 128 != 0)) return false;
  if (a.conv) return !a.out_f32 && a.g.C0 % bk == 0 && a.g.C1 % bk == 0;
  if (a.A1 && (a.batch != 1 || a.kA1 % 64 != 0 || a.lda1 % 8 != 0 || ((uintptr_t)a.A1 % 16) != 0)) return false;
  return a.lda % 8 == 0 && (a.batch == 1 || a.sA % 8 == 0);
}

// K splits for a small-M GEMM on the 4-wave kernel (the CLIP text model's 154 rows, the time embedding's 2B rows): a
// few 64-column tiles over a long K leave most CUs idle (the CLIP fc2 [154 x 768 x 3072]: 36 blocks, 50 us).  Calls
// of M <= 256 rows only (the gate reads the actual M); among those the splits depend on N and K only, whole 64-deep K
// steps each, and not on the output layout (a head-split q|k|v projection takes the same splits as its row-major twin).
int small_splits(const GemmArgs& a) {
  if (!g_small_splitk || !is16(a.dtype) || a.conv || a.batch != 1 || a.geglu || a.A1 || a.up2_w) return 0;
  if (a.M > 256 || a.N % 8 || a.K < 1024 || a.N <= 16) return 0;
  if (a.out_f32 ? a.ldc % 4 != 0 : (a.ldc % 8 != 0 || ((uintptr_t)a.C % 16) != 0)) return 0;
  if (a.residual && (a.ldr % 8 != 0 || ((uintptr_t)a.residual % 16) != 0)) return 0;
  const long ctiles = (a.N + 63) / 64;
  if (ctiles >= 128) return 0;
  int sp = 1;
  while (sp < 8 && ctiles * sp * 2 <= 256 && a.K % (sp * 2 * 64) == 0 && a.K / (sp * 2) >= 256) sp *= 2;
  return sp > 1 ? sp : 0;
}

// Halo tiles of a 3x3 / stride-1 / pad-1 conv, or of one parity's 2x2 conv of a nearest-2x upsampler
// (GemmArgs::up2_*, pad (1 - a, 1 - b)); bn == 0: the halo path does not take the conv.  The decision does not depend
// on the parity.
struct Halo {
  int mode = 0;     // 1 = 256-pixel tiles of whole image rows (W in {16, 32, 64}), 2 = 8 x 32 strip tiles (W % 32 == 0,
                    // H % 8 == 0; HALO == 5 / 7), 3 = four whole 8x8 images per tile (HALO == 8 / 9)
  int bn = 0;       // BN 160 (UNet widths), else 128 (VAE widths 128 / 256 / 512; ping-pong loop only)
  int splits = 1;   // K splits (whole 64-channel slabs per split)
};

Halo plan_halo(const GemmArgs& a) {
  const ConvGeom& g = a.g;
  Halo h;
  if (!g_conv_halo || !a.conv || a.batch != 1 || a.geglu || a.out_f32 || !vec_ok(a)) return h;
  if (g.stride != 1) return h;
  if (a.up2_w) {   // (ping-pong loop only)
    if (!g_halo_up2 || !g_halo_pipe || a.gn_ab || g.KH != 2 || g.KW != 2 || (g.pad_t & ~1) || (g.pad_l & ~1)) return h;
  } else if (g.KH != 3 || g.KW != 3 || g.pad_t != 1 || g.pad_l != 1) {
    return h;
  }
  if (g.Hv != g.Hin || g.Wv != g.Win || g.Ho != g.Hin || g.Wo != g.Win) return h;
  if (g.C0 % 64 || g.C1 % 64 || g.C0 <= 0) return h;
  const int W = g.Win;
  if ((long)g.N * g.Hin * W != a.M) return h;
  const int slabs = (g.C0 + g.C1) / 64;
  const int bn = a.N % 160 == 0 ? 160 : (a.N % 128 == 0 && g_halo_pipe && !a.gn_ab) ? 128 : 0;
  // four whole 8x8 images per tile (HALO == 8, instantiated at BN 160: the UNet's 1280 channels): any image count (a
  // partial last tile), so the choice is batch-invariant like the others.  Whole slabs per split for about one block
  // per CU (the canonical 16 images: 4 row tiles x N / 160), reduced by the separate kernel
  if (W == 8 && g.Hin == 8 && g_halo_mi && g_halo_pipe && !a.gn_ab && a.M % 64 == 0) {
    if (bn != 160) return h;
    const long tiles = (canon_rows(a) + 255) / 256 * (a.N / bn);
    const int want = (int)std::max(1L, std::min(8L, (long)kCUs / std::max(1L, tiles)));
    const int per = (slabs + want - 1) / want;
    h.mode = 3; h.bn = bn; h.splits = (slabs + per - 1) / per;
    return h;
  }
  // (parity convs on row / strip tiles: whole 256-row tiles of one image, the sub-pixel GroupNorm partial blocks)
  if (a.up2_w && ((long)a.up2_h * a.up2_w) % 256) return h;
  if (a.M % 256) return h;
  const bool rows = W >= 16 && W <= kHaloWMax && !(W & (W - 1)) && 256 % W == 0 && g.Hin % (256 / W) == 0;
  // (strips: the ping-pong loop only, no GroupNorm-fused operand)
  const bool strips = g_halo_strip && g_halo_pipe && !a.gn_ab && W % kStripW == 0 && g.Hin % (256 / kStripW) == 0;
  const int mode = strips && (g_halo_strip == 2 || !rows) ? 2 : rows ? 1 : 0;
  if (!mode || !bn) return h;
  // the grid must fill the chip: alone (1 split), or with two K splits reduced in the kernel
  const long tiles = canon_rows(a) / 256 * (a.N / bn);
  int splits = 0;
  if (tiles >= kCUs || g_conv_halo >= 2) splits = 1;
  else if (g_halo_split && 2 * tiles >= kCUs && slabs >= 8 && reduce_in_kernel(2, tiles)) splits = 2;
  if (!splits) return h;
  if (a.up2_w && mode == 2 && bn != 128) return h;   // (strip parity convs: the VAE widths only, HALO == 7 at BN 128)
  // (GroupNorm-fused operand: one 512-element chunk of the (256 + 2W) x 8 halo per tap, taps 3..8)
  static_assert((256 + 2 * kHaloWMax) * 8 <= 512 * 6, "halo normalisation chunks");
  h.mode = mode; h.bn = bn; h.splits = splits;
  return h;
}

// Tile order of a halo conv (GemmArgs::group_m; scheduling only, no numeric effect).  One XCD runs q = tiles / 8
// consecutive logical tiles at once; in the M-major order they are q / tiles_n M tiles x all tiles_n N tiles, so at
// the 16x16 level (16 M tiles x 8 N tiles of a 1280-channel conv, 29.5 MB of weights) every XCD streams all of B.
// Grouped by g M tiles the range is g x q / g: per XCD ~ g halo slabs of A + q / g B panels (bytes (BM + 2W) Cin 2
// and BN K 2).  g minimises that sum; 0 keeps the M-major order when it is within 10 % of the best.
int halo_group_m(const GemmArgs& a, const Halo& h) {
  if (!g_halo_group) return 0;
  const long tiles_m = (a.M + 255) / 256, tiles_n = a.N / h.bn;
  if (tiles_n < 2) return 0;
  // logical tiles per XCD (xcd_remap ranges), of which one block per CU = 32 run at a time
  const long q = (tiles_m * tiles_n + 7) / 8, w = std::min(q, 32L);
  const double hpix = h.mode == 2 ? 10.0 * (kStripW + 2) : 256.0 + 2.0 * a.g.Wo;   // halo pixels per tile
  const double a_m = hpix * (a.g.C0 + a.g.C1) * 2.0, b_n = (double)h.bn * a.K * 2.0;
  auto cost = [&](long g) {   // A + B bytes of one XCD's w co-resident tiles in groups of g M tiles
    const bool whole = w >= g * tiles_n;   // (the window spans whole groups: w / tiles_n M tiles x every N tile)
    const long gm = whole ? (w + tiles_n - 1) / tiles_n : std::min(g, w);
    const long gn = whole ? tiles_n : (w + g - 1) / g;
    return gm * a_m + gn * b_n;
  };
  const double legacy = cost(std::max(1L, (w + tiles_n - 1) / tiles_n));   // M-major: w / tiles_n whole M rows
  long best_g = 0;
  double best = legacy;
  for (long g = 1; g <= tiles_m; g *= 2)
    if (cost(g) < best) { best = cost(g); best_g = g; }
  return best < 0.9 * legacy ? (int)best_g : 0;
}

// Tile order of a dense large-tile GEMM (scheduling only): the cost model of halo_group_m with A panel BM x K and B
// panel BN x K, over the 32 x `resident` tiles one XCD runs at once; 0 keeps the M-major / N-major order when the
// grouped one is not > 10 % better.  (The GEGLU projections at 32^2 / 16^2: every XCD streamed the whole 6.5 / 26 MB
// weight in the M-major / N-major orders.)
int dense_group_m(const GemmArgs& a, int bm, int bn, int resident, bool nmajor) {
  if (!g_gemm_group) return 0;
  const long tiles_m = (a.M + bm - 1) / bm, tiles_n = (a.N + bn - 1) / bn;
  if (tiles_n < 2 || tiles_m < 2) return 0;
  if (g_gemm_group >= 2) return (int)std::min((long)g_gemm_group, tiles_m);
  const long q = (tiles_m * tiles_n + 7) / 8, w = std::min(q, 32L * resident);
  const double a_m = (double)bm * a.K * 2.0, b_n = (double)bn * a.K * 2.0;
  auto cost = [&](long g) {
    const bool whole = w >= g * tiles_n;
    const long gm = whole ? (w + tiles_n - 1) / tiles_n : std::min(g, w);
    const long gn = whole ? tiles_n : (w + g - 1) / g;
    return gm * a_m + gn * b_n;
  };
  // the current order: M-major = groups of one whole M row block; N-major = a window of w M tiles x w / tiles_m N tiles
  const double legacy = nmajor ? std::min(w, tiles_m) * a_m + (double)((w + tiles_m - 1) / tiles_m) * b_n
                               : cost(std::max(1L, (w + tiles_n - 1) / tiles_n));
  long best_g = 0;
  double best = legacy;
  for (long g = 1; g <= tiles_m; g *= 2)
    if (cost(g) < best) { best = cost(g); best_g = g; }
  return best < 0.9 * legacy ? (int)best_g : 0;
}

void set_kernel(GemmPlan& p, int BM, int BN, int WM, int WN, int BK, int S, int HALO = 0, bool PP = false) {
  p.BM = BM; p.BN = BN; p.WM = WM; p.WN = WN; p.BK = BK; p.S = S; p.HALO = HALO; p.PP = PP;
}

// A halo conv: 256 x bn tiles of 4 x 2 waves, BK 64, three stages; HALO names the main loop
void plan_halo_launch(const GemmArgs& a, const Halo& h, GemmPlan& p) {
  p.path = GEMM_HALO;
  p.vec_epilogue = true;
  p.group_m = halo_group_m(a, h);
  const bool mi = h.mode == 3;
  int halo;
  if (mi) halo = a.up2_w ? 9 : 8;                  // four 8x8 images per tile (parity convs: 4 taps)
  else if (a.up2_w) halo = h.mode == 2 ? 7 : 6;    // upsampler parity convs: 4 taps per slab
  else if (h.mode == 2) halo = 5;                  // strip tiles (ping-pong main loop)
  else halo = g_halo_pipe && !a.gn_ab ? 2 : 1;     // ping-pong main loop / the lock-step loop (BN 160 only)
  set_kernel(p, 256, h.bn, 4, 2, 64, 3, halo);
  p.splits = h.splits;
  p.per = a.K / 64;
  if (h.splits > 1) {   // whole slabs per split, in-kernel last-arriver reduction (fp32 partials; 8x8: reduce kernel)
    const int slabs = (a.g.C0 + a.g.C1) / 64;
    p.per = (a.up2_w ? 4 : 9) * ((slabs + h.splits - 1) / h.splits);
    p.Mp = (a.M + 255) / 256 * 256;   // (whole row tiles of partials: a partial last tile stores all its rows)
    p.Np = a.N;
    p.ws_bytes = (size_t)h.splits * p.Mp * a.N * sizeof(float);
    p.inkernel = !mi;
  }
}

// The gemm2_kernel instantiation of a dense / im2col tile: waves, K depth of a stage and stages per main loop
bool large_kernel(const GemmArgs& a, const Choice& c, GemmPlan& p) {
  const int key = c.BM * 1000 + c.BN;
  const int wm = (c.BM == 256 && c.BN <= 160) ? 4 : 2, wn = 8 / wm;   // 256x128 / 256x160: 4 x 2 waves
  if (c.pair) {   // the lean ping-pong loop, two 8-wave blocks per CU (pair_tile)
    set_kernel(p, c.BM, c.BN, wm, wn, 32, 3, 0, true);
  } else if (c.BM == 64) {   // 64x320, 4 waves, BK 32, two stages (48 KiB of LDS: three blocks per CU)
    set_kernel(p, 64, 320, 1, 4, 32, 2);
  } else if (c.small) {   // 4 waves, two blocks per CU
    set_kernel(p, 128, c.BN, 2, 2, 64, 2);
  } else if (g_gemm_deep == 0 && g_gemm_pp && !a.conv && !a.ln_out && !a.b_rows &&
             (!a.A1 || g_gemm_pp_chain) &&   // (two-source A: the ping-pong loop only where the chain option allows it)
             ((c.BM == 256 && c.BN == 256) ||
              // the long-K two-source 1x1 convs (proj_out o ff.net.2 over (h | g), K = 5C): the ping-pong loop pays
              // where the K loop is long (unlike the K = 320 / 640 projections, which stay on the two-stage loop)
              (a.A1 && g_gemm_pp_chain && c.BN == 320 && (c.BM == 256 || c.BM == 128) && a.K >= 1024)) &&
             a.M % c.BM == 0 && a.N % c.BN == 0) {
    // the lean ping-pong loop: dense GEMMs on whole tiles, 3 stages of BK 32 (BK 64 would not fit these tiles)
    set_kernel(p, c.BM, c.BN, wm, wn, 32, 3, 0, true);
  } else if (g_gemm_deep == 2) {   // BK 64; a third (fourth) stage wherever it fits in 160 KiB
    if (key == 256320) return false;
    set_kernel(p, c.BM, c.BN, wm, wn, 64, (key == 256256 || key == 128320) ? 2 : key == 128128 ? 4 : 3);
  } else if (g_gemm_deep == 1) {   // BK 32 ring
    if (key == 256320 || c.BN == 160) return false;
    set_kernel(p, c.BM, c.BN, wm, wn, 32, key == 256256 ? 4 : key == 128128 ? 6 : 5);
  } else {
    if (c.BN == 160) return false;
    set_kernel(p, c.BM, c.BN, wm, wn, 64, 2);
  }
  return true;
}

// A dense / im2col GEMM on the large tiles `c`; false, with `p` untouched (the 4-wave kernel runs), where the epilogue
// forms do not fit
bool plan_large(const GemmArgs& a, const Choice& c0, GemmPlan& p) {
  Choice c = c0;
  if (pair_tile(a, c0, c.BM, c.BN)) {
    c.pair = true;
    c.splits = 1;
  } else if (a.K % step_k() != 0) {   // (eligible() let K % 32 == 0 through for the forced pair tiles only)
    return false;
  }
  const bool vec = vec_ok(a);
  if (a.geglu && !vec) return false;
  if (c.splits > 1) {
    if (!vec && !a.out_f32) return false;     // reduce kernel needs 16-byte output rows
    if (a.out_f32 && (a.ldc % 8 != 0 || a.N % 8 != 0)) return false;
  }
  if (!large_kernel(a, c, p)) return false;
  p.path = GEMM_LARGE;
  p.vec_epilogue = vec;
  // tile order (scheduling only, no numeric effect): N-major when the weights outweigh the activation rows, so that an
  // XCD's consecutive tiles re-use one B panel from its L2 instead of every XCD streaming all of B
  p.nmajor = g_gemm_nmajor == 2 || (g_gemm_nmajor == 1 && (long)a.N * a.batch > (long)a.M * a.batch);
  if (a.batch == 1 && !a.hs_L) {   // grouped order where it cuts an XCD's co-resident A + B bytes (GemmArgs::group_m)
    p.group_m = dense_group_m(a, c.BM, c.BN, (c.BM == 128 && c.BN == 128) || c.small || c.pair ? 2 : 1, p.nmajor);
    if (p.group_m) p.nmajor = 0;
  }
  p.splits = c.splits;
  // K steps per split: the choice counts steps of step_k(), the kernel steps of its BK
  p.per = c.pair ? a.K / p.BK : (c.splits > 1 ? c.per : a.K / step_k()) * (step_k() / p.BK);
  if (c.splits > 1) {
    p.Mp = (a.M + c.BM - 1) / c.BM * c.BM;
    p.Np = (a.N + c.BN - 1) / c.BN * c.BN;
    p.ws_bytes = (size_t)c.splits * a.batch * p.Mp * p.Np * sizeof(float);
    p.inkernel = reduce_in_kernel(c.splits, (long)(p.Mp / c.BM) * (p.Np / c.BN) * a.batch);
  }
  return true;
}

// a stand-in for a buffer a query asks about before it exists (never dereferenced)
template <typename T> T* requested() { return (T*)(uintptr_t)4096; }

}  // namespace

// The K = 320 streaming path: dense, 16-bit, one batch, no conv / split / activation / row add / GroupNorm
// partials; N a multiple of the 320-column slice (GEGLU: of 256 interleaved weight rows); 16-byte aligned rows.
// The decision depends only on the per-call shape (not on M), so it is the same for every batch size.
bool gemm_sk_eligible(const GemmArgs& a) {
  if (!g_gemm_sk || (!a.geglu && g_gemm_sk != 3) || !is16(a.dtype) || a.conv || a.out_f32 || a.batch != 1 || a.K != kSkK) return false;
  if (a.act != ACT_NONE || a.rowadd || a.gn_part || a.gn_ab || a.b_rows || a.ln_out) return false;
  if (a.A1 || a.up2_w) return false;   // (one A source of K columns; plain row-major output)
  if (a.res_rows) return false;        // (the residual DMA walks consecutive rows: no wrap, GemmArgs::res_rows)
  if (a.geglu ? (a.N % 256 != 0 || a.N / 2 / 128 > 32 || a.residual || a.hs_L || a.ldc % 4) : (a.N % 320 || a.N / 320 > 32))
    return false;
  if (a.lda % 8 || a.ldb % 8 || ((uintptr_t)a.A % 16) || ((uintptr_t)a.B % 16)) return false;
  if (((uintptr_t)a.C % 8) || (a.hs_L ? (a.hs_d % 4 || a.hs_C % 4) : a.ldc % 4)) return false;
  if (a.residual && (a.ldr % 4 || ((uintptr_t)a.residual % 8))) return false;
  if (a.hs_L && (a.residual || a.hs_L % 64)) return false;   // (a 64-row tile lies in one image)
  if ((a.ln_rs || a.ln_part) && (a.alpha != 1.f || a.M % 2)) return false;   // (statistics DMA'd as row pairs)
  if (a.ln_part && a.ln_T != 1) return false;   // (one producer partial per row: the K = 320 row)
  return a.M > 0;
}

GemmPlan gemm_plan(const GemmArgs& a) {
  GemmPlan p;
  const int small = small_splits(a);
  const size_t small_bytes = small ? (size_t)small * a.M * a.N * sizeof(float) : 0;
  p.ws_reserve = small_bytes;
  Halo h;
  Choice c;
  if (g_large_tiles && eligible(a)) {
    h = plan_halo(a);
    if (h.bn) {
      p.ws_reserve = h.splits > 1 ? (size_t)h.splits * ((a.M + 255) / 256 * 256) * a.N * sizeof(float) : 0;
    } else {
      c = choose(a);
      if (c.BM && c.splits > 1)
        p.ws_reserve = std::max(small_bytes, (size_t)c.splits * a.batch * ((a.M + c.BM - 1) / c.BM * c.BM) *
                                                 ((a.N + c.BN - 1) / c.BN * c.BN) * sizeof(float));
    }
    if (gemm_sk_eligible(a)) p.path = GEMM_SK;
    else if (h.bn) plan_halo_launch(a, h, p);
    else if (c.BM) plan_large(a, c, p);   // (may decline: the 4-wave kernel then)
  }
  if (p.path == GEMM_WAVE4 && small) {   // raw fp32 partials per K split, then the reduce kernel
    p.path = GEMM_WAVE4_SPLIT;
    p.splits = small;
    p.Mp = a.M; p.Np = a.N;
    p.ws_bytes = small_bytes;
  }

  // ---- which requested features the path honours
  const bool vec = p.vec_epilogue;
  // the kernel's own staged epilogue finishes every tile (no K splits, or the in-kernel reduction)
  const bool full_epi = p.large() && vec && (p.splits == 1 || p.inkernel);
  const bool one16 = a.batch == 1 && !a.out_f32;
  if (a.geglu) p.geglu = p.path == GEMM_SK ? vec_ok(a) : p.path == GEMM_LARGE && vec;
  // every store of the large-tile path goes through c_off (the 16-byte epilogue, the split-K reduce kernel, the halo
  // parity convs); the scalar epilogue, the 4-wave kernel and gemm_sk do not map rows
  if (a.up2_w) p.up2 = p.large() && vec && a.batch == 1 && !a.hs_L;
  if (a.gn_ab) p.gn_fused = g_gn_fuse && p.path == GEMM_HALO && p.HALO == 1;   // (the lock-step halo loop only)
  if (a.gn_part && g_gn_parts && p.large() && vec && one16 && !a.geglu && !a.hs_L) {
    if (p.splits > 1 && !p.inkernel)
      // splitk_reduce_gn_kernel applies one bias vector and assumes the plain m * ldc layout: no per-image weights /
      // bias, no sub-pixel rows
      p.gn_rows = (g_gn_red_parts && !a.up2_w && !a.b_rows && a.M % kRedGnRows == 0 && a.N % 64 == 0 && a.act == ACT_NONE)
                      ? kRedGnRows : 0;
    else if (p.path == GEMM_HALO)
      p.gn_rows = h.mode == 3 ? 0 : 256;   // (row / strip tiles: M % 256 == 0)
    else if (a.up2_w && ((long)a.up2_h * a.up2_w) % p.BM)
      p.gn_rows = 0;   // (a sub-pixel tile's rows in one image)
    else
      p.gn_rows = a.M % p.BM ? 0 : p.BM;
  }
  if (a.ln_rs || a.ln_part)
    p.ln_fold = !a.conv && a.alpha == 1.f && one16 && vec_ok(a) && (p.path == GEMM_SK || (p.path == GEMM_LARGE && full_epi));
  // LayerNorm partials out and per-image B / bias: the staged epilogue of the two-stage / lean ping-pong loops
  const bool staged = p.path == GEMM_LARGE && full_epi && !a.conv && one16 && !a.geglu && g_gemm_deep == 0;
  const bool ln_w_ok = a.ln_W == kLnGroup || a.ln_W == kLnGroupNarrow;
  if (a.ln_out && g_ln_parts && staged && !a.hs_L && !a.gn_part && ln_w_ok && a.N % a.ln_W == 0 &&
      !(a.ln_out_rs && a.N != a.ln_W)) {
    // one partial per tile and row: the tile as wide as the requested group — 320-column tiles (the 64x64 / 32x32-level
    // transformer projections) or the 8-wave 128x128 two-stage tile (C = 1280).  A call that gemm_sk takes without
    // the partials (option gemm_sk 3) stays there: its consumer runs the statistics pass
    GemmArgs bare = a;
    bare.ln_out = nullptr;
    const bool tile = a.ln_W == kLnGroup ? (p.BM == 256 || p.BM == 128)
                                         : (p.BM == 128 && p.WM * p.WN == 8 && !p.PP);
    p.ln_out = p.BN == a.ln_W && tile && !gemm_sk_eligible(bare);
  }
  // ... row tiles that never straddle two images
  if (a.b_rows > 0)   // (not the 4-wave 128-row tiles of option gemm_small)
    p.bimg = staged && !(p.WM == 2 && p.WN == 2) && a.M % a.b_rows == 0 && a.b_rows % p.BM == 0;
  return p;
}

// ------------------------------------------------------------------ queries: the plan of the call with the feature requested
size_t gemm_workspace_bytes(const GemmArgs& a) { return gemm_plan(a).ws_reserve; }

size_t gemm_small_split_bytes(const GemmArgs& a) {
  const int sp = small_splits(a);
  return sp ? (size_t)sp * a.M * a.N * sizeof(float) : 0;
}

int gemm_large_splits(const GemmArgs& a) {
  const GemmPlan p = gemm_plan(a);
  return p.large() ? p.splits : 0;
}

bool gemm_geglu_fusable(const GemmArgs& a) { return gemm_plan(a).geglu; }
bool gemm_up2_ok(const GemmArgs& a) { return gemm_plan(a).up2; }
bool gemm_bimg_ok(const GemmArgs& a) { return gemm_plan(a).bimg; }

int gemm_emits_gn_parts(const GemmArgs& a) {
  GemmArgs q = a;
  if (!q.gn_part) q.gn_part = requested<double>();
  return gemm_plan(q).gn_rows;
}

bool gemm_gn_fusable(const GemmArgs& a) {
  GemmArgs q = a;
  if (!q.gn_ab) q.gn_ab = requested<const float2>();
  return gemm_plan(q).gn_fused;
}

bool gemm_ln_foldable(const GemmArgs& a) {
  GemmArgs q = a;
  if (!q.ln_rs && !q.ln_part) q.ln_rs = requested<const float2>();
  return gemm_plan(q).ln_fold;
}

bool gemm_emits_ln_parts(const GemmArgs& a) {
  GemmArgs q = a;
  if (!q.ln_out) q.ln_out = requested<float2>();
  return gemm_plan(q).ln_out;
}

bool conv1x1_as_dense(GemmArgs& a) {
  const ConvGeom& g = a.g;
  if (!g_conv1x1_dense || !a.conv || !is16(a.dtype) || a.batch != 1 || a.gn_ab || a.up2_w || a.act != ACT_NONE) return false;
  if (g.KH != 1 || g.KW != 1 || g.stride != 1 || g.pad_t != 0 || g.pad_l != 0) return false;
  if (g.Hv != g.Hin || g.Wv != g.Win || g.Ho != g.Hin || g.Wo != g.Win) return false;
  GemmArgs d = a;
  d.conv = 0;
  d.g = ConvGeom();
  d.A = g.src0; d.lda = g.C0;
  d.A1 = g.C1 ? g.src1 : nullptr; d.lda1 = g.C1; d.kA1 = g.C1 ? g.C0 : 0;
  const int path = gemm_plan(d).path;
  if (path != GEMM_SK && path != GEMM_LARGE) return false;
  a = d;
  return true;
}

}  // namespace irx
