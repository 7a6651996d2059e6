// tile_select.h -- which compiled body runs a tile pass: the one selection rule of the library's launcher (tile_kernels.hip
// launch_tile) and of the host emulator (tests/emu/emu_tile.cpp), for Goldilocks and Montgomery primes (TileArgs::fc.p).
// Plain C++ (no HIP), so the emulator checks on the CPU exactly the choice the GPU makes.
//   GENERIC  the run-time-strided kernel of every pass size (KIND 0)
//   CFG      a RONK_CFG_TABLE / RONK_CFG_TABLE_DIST shape (tile_cfg_table.h; Montgomery: RONK_CFG_TABLE only)
//   HALF     the same shape with two-phase 32-bit LDS exchanges (Goldilocks)
//   FEAT     a RONK_CFG_TABLE_FEAT shape (Montgomery: only in the direction the feature occurs in)
//   WL_FULL / WL_HALF  ntt_tile_wl.h's 2^10 .. 2^12-row x 4-column passes (the half image: Goldilocks, 2^11 rows)
//   R4       the [16 . 4] . [8 | 16] round structure of the 2^9 / 2^10-row shapes (Goldilocks, opt-in)
#pragma once
#include <stdlib.h>

#include "ntt_tile.h"
#include "ntt_tile_wl.h"
#include "tile_cfg_table.h"

namespace ronk {

// every dispatch knob, read once per process
struct TileEnv {
  bool no_cfg = false;   // RONK_NO_CFG_KERNELS (set): the generic kernels only (experiments)
  int half_lds = -1;     // RONK_HALF_LDS: -1 the grid-size rule (use_half), 0 never, 1 always, 2 row passes only
  int wl = 1;            // RONK_WL: 0 off, 1 both passes, 2 column pass only, 3 row pass only
  bool wl_half = false;  // RONK_WL_HALF=1: the half-image WL form (Goldilocks, 2^11 rows)
  int wl_rows = 7;       // RONK_WL_ROWS: bit mask of the WL pass sizes (1 = 2^10 rows, 2 = 2^11, 4 = 2^12)
  bool r4mid = false;    // RONK_R4MID=1: the R4 round structure (opt-in, measured not faster: tile_kernels_r4.hip)
};

inline TileEnv tile_env_read() {
  const auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  TileEnv v;
  v.no_cfg = getenv("RONK_NO_CFG_KERNELS") != nullptr;
  v.half_lds = num("RONK_HALF_LDS", -1);
  v.wl = num("RONK_WL", 1);
  v.wl_half = num("RONK_WL_HALF", 0) != 0;
  v.wl_rows = num("RONK_WL_ROWS", 7);
  v.r4mid = num("RONK_R4MID", 0) != 0;
  return v;
}
inline const TileEnv& tile_env() {
  static const TileEnv v = tile_env_read();
  return v;
}

// does RONK_WL want the WL body for a pass of this kind?
inline bool tile_wl_wanted(const TileEnv& env, int kind) {
  return env.wl == 1 || (env.wl == 2 && kind != 2) || (env.wl == 3 && kind == 2);
}

// Two-phase 32-bit LDS exchanges (TileCfg::HALF, half the LDS image, kernels built for 6-8 waves per SIMD) pay when a
// pass has far more tiles than the chip holds at once: the workgroups of a CU drift into different phases and the
// additional resident ones fill the load / store phases of the others.  Measured (same box): 1024 x 2^16
// 0.493 -> 0.469 ms, 512 x 2^17 0.561 -> 0.514 ms; row passes with >= 2^10 rows get slower (2^22 x 16 pass 2: 402 -> 484 us)
// and a single transform (one tile per CU) only pays the extra barriers (51.4 -> 53.7 us), so:
//   default  column passes (KIND 1, 3) of any size and row passes (KIND 2) up to 2^9 rows, when the grid has at least
//            twice the threads the chip holds at four waves per SIMD (2 * 256 CUs * 1024)
//   RONK_HALF_LDS = 0 never, 1 always, 2 row passes only (experiments)
//   round 3 (planner: big batches keep 16384-coefficient tiles for 2^11-row passes; HBM-cold sweep, profiles/r03_half_rule_sweep.txt):
//            a 2^11-row x 8-column row pass owns a whole CU (136 KiB) -- there the half image pays as well (2^22 x 16: 21.5 k ->
//            22.5 k NTT/s); 2^10-row row passes stay on the full image (2^21 x 32: 49.9 k with the rule, 48.4 k all-half)
inline bool use_half(const TileEnv& env, const TileArgs& a, int logr, u32 grid, u32 block, int kind) {
  if (env.half_lds >= 0) return env.half_lds == 1 || (env.half_lds == 2 && kind == 2);
  if ((unsigned long long)grid * block < 2ull * 256 * 1024) return false;
  return kind != 2 || logr <= 9 || (logr == 11 && a.logc == 3);
}

// the instantiation tables (tile_cfg_table.h) as predicates
inline bool tile_cfg_listed(int logr, int logc, int kind) {
#define RONK_SEL_HAS(LR, LC, KD) if (logr == LR && logc == LC && kind == KD) return true;
  RONK_CFG_TABLE(RONK_SEL_HAS)
#undef RONK_SEL_HAS
  return false;
}
inline bool tile_dist_listed(int logr, int logc, int kind) {
#define RONK_SEL_HAS(LR, LC, KD) if (logr == LR && logc == LC && kind == KD) return true;
  RONK_CFG_TABLE_DIST(RONK_SEL_HAS)
#undef RONK_SEL_HAS
  return false;
}
inline bool tile_feat_listed(int logr, int logc, int kind, int feat) {
#define RONK_SEL_HAS(LR, LC, KD, FT) if (logr == LR && logc == LC && kind == KD && feat == FT) return true;
  RONK_CFG_TABLE_FEAT(RONK_SEL_HAS)
#undef RONK_SEL_HAS
  return false;
}

enum class TileForm { GENERIC, CFG, HALF, FEAT, WL_FULL, WL_HALF, R4 };
struct TileChoice {
  TileForm form = TileForm::GENERIC;
  int kind = 0;   // KIND of the shape (ntt_tile.h TileCfg); 0 for GENERIC
  int feat = 0;   // FEAT mask (FEAT only)
};

inline TileChoice select_tile(const TileArgs& a, int logr, bool inverse, u32 grid, u32 block, const TileEnv& env) {
  if (env.no_cfg) return {};
  const bool mont = a.fc.p != 0;   // Montgomery instantiations: no HALF, no R4, no DIST shapes, FEAT in one direction
  const bool r4 = env.r4mid && !mont;
  const int logc = (int)a.logc, feat = tile_features(a);
  // 2^10 / 2^11 / 2^12-row x 4-column passes (the two-lane plans of 2^20 .. 2^22, one transform of 2^20 / 2^21 / 2^23): one
  // wave-local and one cross-wave exchange, one barrier per pass (ntt_tile_wl.h).  Round 6, same box: two lanes at 2^22
  // 22.4 k -> 23.6 k NTT/s, one stream 58.5 -> 55.5 us.  The opt-in R4 structure wins at 2^10 rows.
  if (!feat && wl_logr_ok(logr) && logc == WL_LOGC && !(r4 && logr == 10) && ((env.wl_rows >> (logr - 10)) & 1)) {
    for (int kind : {1, 2, 3}) {
      if (!tile_wl_wanted(env, kind) || !tile_wl_matches(a, logr, kind)) continue;
      return {env.wl_half && !mont && logr == 11 ? TileForm::WL_HALF : TileForm::WL_FULL, kind, 0};
    }
  }
  // one kind after the other: a pass can match several (a column pass is a general twiddled pass, too), and the first kind
  // with an instantiation wins
  for (int kind : {1, 2, 3, 4, 5}) {
    if (!tile_cfg_matches(a, logr, logc, kind, feat)) continue;
    if (feat) {
      // Montgomery: padding limits belong to forward transforms (multiply operands, encode), the second operand and the
      // truncation to the multiply's inverse -- only that direction is instantiated
      if (tile_feat_listed(logr, logc, kind, feat) && (!mont || inverse == (feat != FEAT_IN_VALID))) return {TileForm::FEAT, kind, feat};
      continue;
    }
    if (mont) {
      if (tile_cfg_listed(logr, logc, kind)) return {TileForm::CFG, kind, 0};
      continue;
    }
    if (kind < 4 && tile_cfg_listed(logr, logc, kind) && use_half(env, a, logr, grid, block, kind)) return {TileForm::HALF, kind, 0};
    if (r4 && (logr == 9 || logr == 10) && tile_cfg_listed(logr, logc, kind) && cfg_r4(logr, logc, kind)) return {TileForm::R4, kind, 0};
    if (tile_cfg_listed(logr, logc, kind) || tile_dist_listed(logr, logc, kind)) return {TileForm::CFG, kind, 0};
  }
  return {};
}

// the emulator's name for a choice ("kernel=" in tests/emu/emu_tile.cpp's pass lines)
inline const char* tile_choice_label(const TileChoice& c) {
  static const char* const names[7][6] = {
      {"generic", "generic", "generic", "generic", "generic", "generic"},
      {"cfg:", "cfg:column/two-level", "cfg:row", "cfg:column/matrix", "cfg:general", "cfg:whole"},
      {"half:", "half:column/two-level", "half:row", "half:column/matrix", "half:general", "half:whole"},
      {"feat:", "feat:column/two-level", "feat:row", "feat:column/matrix", "feat:general", "feat:whole"},
      {"wl:", "wl:column/two-level", "wl:row", "wl:column/matrix", "wl:general", "wl:whole"},
      {"wl:", "wl:column/two-level", "wl:row", "wl:column/matrix", "wl:general", "wl:whole"},
      {"r4:", "r4:column/two-level", "r4:row", "r4:column/matrix", "r4:general", "r4:whole"}};
  return names[(int)c.form][c.kind >= 0 && c.kind <= 5 ? c.kind : 0];
}

}  // namespace ronk
