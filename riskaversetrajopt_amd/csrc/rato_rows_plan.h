// Launch geometry of the two row-parallel linearize kernels (drone_linearize_rows_kernel, car_linearize_rows_kernel):
// host-only, no HIP header, no getenv, no runtime call -- plain C++17 that the launchers (drone.hip, driving.hip), the
// rato_*_stats_in_launch queries and the rato_*_rows_plan queries (and through those the CPU tests) all share.
//
// A batch of M samples is n_tiles = ceil(M / 64) tiles (one sample per lane).  A launch takes one of three forms:
//   SPLIT   every tile dealt to `split` workgroups, each taking the row tasks congruent to its part (mod split): small
//           batches, so that the chip is filled;
//   STATIC  one tile per workgroup;
//   QUEUE   `workgroups` resident workgroups take units from a global counter: n_whole whole tiles first, then the last
//           n_tiles - n_whole tiles as `split` row-interleaved parts each.
// In every form the kernel runs n_units = n_whole + (n_tiles - n_whole) * split units.  The two systems' rules differ where
// each was measured on its own (the split condition, the queue grid, the tail defaults, n_whole's convention in the
// static form, the RATO_ROWS_DYNAMIC test): they are two functions on purpose.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rato_saa.h"

namespace rato_plan {

constexpr int TILE = 64;                    // samples per tile (one wave)
constexpr size_t LDS_MAX = 160 * 1024;      // LDS of a CU: what one workgroup of a row kernel may take
enum Form { SPLIT = RATO_ROWS_FORM_SPLIT, STATIC = RATO_ROWS_FORM_STATIC, QUEUE = RATO_ROWS_FORM_QUEUE };

// what the kernel's build fixes (-DRATO_DIAG, -DRATO_ROWS_NW, -DRATO_CROWS_NW): from the .hip file
struct Geometry {
  size_t lds_bytes;   // per workgroup, for this S
  int waves;          // per workgroup
};

// The A/B switches as integers; the initialisers are what an unset variable means.  The members are in the order of the
// `switches` array of rato_drone_rows_plan / rato_car_rows_plan.
struct DroneSwitches {
  int slots_per_cu = 0;   // RATO_ROWS_SLOTS_PER_CU: fewer workgroups per CU than the LDS allows (one per CU = 256 store streams)
  int small_split = 0;    // RATO_SMALL_SPLIT
  int dynamic = 1;        // RATO_ROWS_DYNAMIC: 0 = no queue (the bit-identity tests' base)
  int qslots = 0;         // RATO_ROWS_QSLOTS: queue workgroups, absolute
  int tail_split = 0;     // RATO_DYN_TAIL_SPLIT (1 = whole tiles only)
  int tail_tiles = 0;     // RATO_DYN_TAIL_TILES
};
struct CarSwitches {
  int slots_per_cu = 0;   // RATO_CAR_SLOTS_PER_CU
  int small_split = -1;   // RATO_CAR_SMALL_SPLIT
  int dynamic = 1;        // RATO_ROWS_DYNAMIC
  int tail_split = 1;     // RATO_CAR_TAIL_SPLIT
  int tail_tiles = -1;    // RATO_CAR_TAIL_TILES
};

inline int n_tiles(int32_t M) { return (M + TILE - 1) / TILE; }
// resident workgroups per CU: the LDS limit, 32 wave slots, at least 1
inline int per_cu(const Geometry& g) {
  int n = (int)(LDS_MAX / g.lds_bytes);
  if (n > 32 / g.waves) n = 32 / g.waves;
  return n < 1 ? 1 : n;
}
inline int max_split(int S) { return (S + 3) / 4 < 1 ? 1 : (S + 3) / 4; }   // keep >= 4 row tasks per workgroup

// The store policy of the row kernels (1: the Jacobian goes out as streaming stores): when the output cannot stay in the
// 256 MB memory-side cache anyway (>= 256 MB) and the batch's noise can (<= 128 MB).  nt_env: RATO_NT_STORES, 0 never /
// 1 by this rule / 2 always (A/B).  Drone M = 1e5, S = 50: 3 GB out, 60 MB in: yes.  Driving C5 shard (800 MB out, 40 MB
// in) -11.7 %; M = 1e6 (6.4 GB out, 320 MB in) ordinary stores (+2 % with streaming ones).
inline int streaming_stores(int nt_env, int64_t M, int S, int out_floats_per_pair, int in_floats_per_step) {
  const double out_bytes = (double)M * (double)((S * (S - 1)) >> 1) * out_floats_per_pair * 4.0;
  const double in_bytes = (double)M * S * in_floats_per_step * 4.0;
  return (nt_env == 2 || (nt_env == 1 && out_bytes >= 256e6 && in_bytes <= 128e6)) ? 1 : 0;
}

inline void finish(rato_rows_plan& r) {
  r.n_units = r.n_whole + (r.n_tiles - r.n_whole) * r.split;
  r.workgroups = r.form == QUEUE ? r.qslots : r.n_units;
}

// ---- drone.  queue_available = false: what the launcher falls back to when the pool hands out no queue (static form).
// In the static form n_whole = n_tiles; qslots is 0 outside the queue form.
inline rato_rows_plan drone_rows(const Geometry& g, int32_t M, int S, bool factored, int cus, const DroneSwitches& sw,
                                 bool queue_available) {
  rato_rows_plan r = {};
  r.n_tiles = n_tiles(M);
  r.per_cu = per_cu(g);
  if (sw.slots_per_cu >= 1 && sw.slots_per_cu < r.per_cu) r.per_cu = sw.slots_per_cu;
  r.slots = cus * r.per_cu;
  r.form = STATIC;
  r.split = 1;
  r.n_whole = r.n_tiles;
  // Small batches (fewer tiles than resident workgroup slots) deal each tile's row tasks out to `split` workgroups so
  // that the chip is filled (M = 1e4, S = 50: 81 -> 72 us).
  if (r.n_tiles < r.slots) {
    // Re-measured with the tiles on 2 MiB boundaries (RATO_SMALL_SPLIT sweep, kernel ms, products / factored):
    // M = 2000 (32 tiles): split 1 0.0439 / 0.0387, 2 0.0339 / 0.0336, 4 0.0342 / 0.0340, slots / n_tiles 0.0378 / 0.0376;
    // M = 5000: 1 0.0456 / 0.0397, 2 0.0389 / 0.0349, 4 0.0453 / 0.0387; M = 1e4 (C2): 1 0.0609, 2 0.0645, 3 0.0653;
    // M = 2e4: 1 0.1208 / 0.0632, 2 0.1213 / 0.0731 -> two parts while that still leaves one workgroup per CU, else none.
    r.split = sw.small_split > 0 ? sw.small_split : (2 * r.n_tiles <= cus ? 2 : 1);
    if (r.split > max_split(S)) r.split = max_split(S);
    if (r.split < 1) r.split = 1;
    if (r.split > 1) {
      r.form = SPLIT;
      r.n_whole = 0;
    }
  }
  // (Splitting the tiles of the last round of a STATIC grid was measured twice and rejected: every extra work unit
  // spends ~15-25 us staging and rolling out in one of only 512 LDS-limited slots -- profiles/README.md; M = 1e5:
  // 0.627 -> 0.648 ms.  So a large batch without a queue uses one workgroup per tile.)
  // Large batches: a grid that fills every slot once + a global tile counter (see the kernel).  Why: with one tile
  // per workgroup the timeline (tools/timeline.py, -DRATO_DIAG=4, M = 1e5) shows the workgroups with an even block
  // index -- every other XCD -- running their tiles in 145-151 us and the odd ones in 174-176 us, the hardware
  // having dealt the grid out to the XCDs in advance: the fast half of the chip is done at 500-518 us and idles
  // until the slow half finishes at 585-590 us.
  // Measured, same box, alternating (profiles/r02_ab_rows.txt): factored output -7 % at M = 1e5, -9 % at M = 1e6;
  // products output -1.5 % at M = 1e5, and -- since its tiles start on 2 MiB boundaries (rato_packed_tile_stride)
  // -- also at large batches: M = 4e5 2.148 / 2.147 ms against 2.176 / 2.213 static, M = 1e6 5.298 / 5.369 against
  // 5.344 / 5.477 (tools/ab_big_products.sh; with the tiles back to back the queue had cost +1.3 % / +5 % there).
  r.wants_queue = r.split == 1 && r.n_tiles > r.slots && sw.dynamic >= 1;
  if (r.wants_queue && queue_available) {
    r.form = QUEUE;
    // Products output, four or more rounds of tiles: ONE queue workgroup per CU (256 store streams instead of
    // 512) is as fast or faster than the two the LDS allows -- same box, alternating (tools/ab_slots.sh,
    // ab_slots2.sh), 2 -> 1 per CU: M = 1e5 0.5600 -> 0.5605 ms (noise read) / 0.5355 -> 0.5256 (regenerated),
    // 2e5 1.110 -> 1.102 / 1.050 -> 1.025, 1e6 5.425 -> 5.311 / 5.097 -> 5.025; at 5e4 +1.2 % / -1.2 %.
    // The factored output needs the second workgroup (its tiles are a third as long: 0.2455 -> 0.2648 ms).
    // RATO_ROWS_SLOTS_PER_CU overrides.
    r.qslots = sw.qslots > 0 ? sw.qslots : ((!factored && sw.slots_per_cu < 1 && r.n_tiles >= 1024) ? cus : r.slots);
    // Products output: the LAST tiles are handed out in row-interleaved parts (round 3: quarters of the last slots / 2
    // tiles; round 6: halves of the last `slots` tiles, below).
    // The drain at the end of the launch is bounded per workgroup (~19 GB/s each, whatever the residency), so
    // shorter last units shorten it; the re-staging they cost is paid while the chip is still full.  Same box,
    // alternating, 100 steps (tools/dyn_tail_sweep.sh): 0.5543-0.5576 -> 0.5415-0.5440 ms (-2.4 %, 0.704-0.708
    // of 8 TB/s); halves over the last 1024 tiles -1 %; thirds / sixths / eighths no better.  The factored
    // output loses with any split (its tiles are short already) and keeps whole tiles.
    // Round 6, re-measured on three boards (same board, alternating, kernel ms by events; tools/ab.sh): quarters over
    // the last 128 tiles (the round-3 choice) 0.5139 / 0.5076 / 0.5135, whole tiles 0.5117 / 0.5036 / 0.5117, HALVES
    // over the last 128 / 256 / 384 tiles 0.5059 / 0.4980 / 0.5004, 0.5067 / 0.5055 / 0.4986, 0.4984 / 0.5046 / 0.4969;
    // eighths 0.523-0.538.  Since the streaming stores (round 4) a re-staged unit costs more than it did (its noise is
    // no longer re-read from HBM by anyone else in between): halves over the last round of tiles are the default.
    int want_split = sw.tail_split > 0 ? sw.tail_split : (factored ? 1 : 2);
    const int want_tiles = sw.tail_tiles > 0 ? sw.tail_tiles : r.qslots;
    if (want_split > max_split(S)) want_split = max_split(S);
    if (want_split > 1 && want_tiles > 0) {
      r.split = want_split;
      // (RATO_ROWS_QSLOTS above the tile count: no tail at all.  Unclamped, n_tiles - qslots < 0 pushed n_whole past
      // n_tiles and the unit count below it: S = 90, M = 20,001 with 512 queue workgroups ran 114 of 313 tiles.)
      const int tail_max = r.n_tiles > r.qslots ? r.n_tiles - r.qslots : 0;
      r.n_whole = r.n_tiles - (want_tiles < tail_max ? want_tiles : tail_max);
    }
  }
  finish(r);
  return r;
}

// ---- driving.  In the split and static forms n_whole = 0 (every tile is dealt as `split` parts, split = 1 included);
// qslots is computed whatever the form.
inline rato_rows_plan car_rows(const Geometry& g, int32_t M, int S, int cus, const CarSwitches& sw, bool queue_available) {
  rato_rows_plan r = {};
  r.n_tiles = n_tiles(M);
  r.per_cu = per_cu(g);
  if (sw.slots_per_cu >= 1 && sw.slots_per_cu < r.per_cu) r.per_cu = sw.slots_per_cu;
  r.slots = cus * r.per_cu;
  // large batches: one workgroup per slot + a global tile queue (XCD load balance, see the kernel)
  r.wants_queue = sw.dynamic != 0 && r.n_tiles > r.slots;
  // At most two queue workgroups per CU even where the LDS allows more (S <= 33).  Measured when the S = 40 layout still
  // fitted three per CU: same box, alternating (tools/ab_car_slots.sh), 3 -> 2:
  // C5 shard (M = 125,000) 0.1923-0.1938 -> 0.1846-0.1877 ms (noise read), 0.1768-0.1771 -> 0.1728-0.1734 (regenerated);
  // M = 1e6 1.162-1.175 -> 1.158-1.163 / 1.105-1.108 -> 1.102-1.111; one per CU: +17 %.  RATO_CAR_SLOTS_PER_CU overrides.
  // Today S = 40 takes 16,208 floats (64,832 B) per workgroup: the LDS itself allows two per CU, 512 slots on 256 CUs.
  r.qslots = (sw.slots_per_cu < 1 && r.per_cu > 2) ? cus * 2 : r.slots;
  if (r.wants_queue && queue_available) {
    r.form = QUEUE;
    // the last `tail_tiles` tiles of the queue as `split` parts each (RATO_CAR_TAIL_SPLIT / RATO_CAR_TAIL_TILES).
    // OFF by default: unlike the drone's products output it does not pay here -- C5 shard (M = 125,000, 1954 tiles
    // on 768 slots when measured; 512 queue workgroups with today's LDS layout), same box, alternating
    // (tools/ab_car_tail.sh), kernel ms: whole tiles 0.1813-0.1816 | halves over
    // the last 384 / 768 tiles 0.1817-0.1823 / 0.1844-0.1856 | thirds 0.1904-0.1907 | quarters 0.1994-0.2012.
    r.split = sw.tail_split < 1 ? 1 : sw.tail_split;
    if (r.split > max_split(S)) r.split = max_split(S);
    int tail_tiles = sw.tail_tiles >= 0 ? sw.tail_tiles : r.qslots / 2;
    if (tail_tiles > r.n_tiles) tail_tiles = r.n_tiles;
    r.n_whole = r.split > 1 ? r.n_tiles - tail_tiles : r.n_tiles;
  } else {
    // small batches (fewer tiles than workgroup slots): every tile split over several workgroups (>= 4 row tasks each)
    r.split = 1;
    if (r.n_tiles < r.slots) {
      // C3 (M = 1e4: 157 tiles; 768 slots when measured, 512 with today's LDS layout: split 2 either way), same box,
      // alternating, kern_ms: split 1 / 2 / 3 / 4 = 0.0302-0.0307 /
      // 0.0279-0.0282 / 0.0270-0.0271 (one run 0.0411) / 0.0360-0.0361: every part rebuilds the fp64 ego tables and
      // re-stages the noise tile, so two parts per tile is where it stops paying reliably.
      r.split = sw.small_split >= 1 ? sw.small_split : (r.slots / r.n_tiles >= 2 ? 2 : 1);
      if (r.split > max_split(S)) r.split = max_split(S);
      if (r.split < 1) r.split = 1;
    }
    r.form = r.split > 1 ? SPLIT : STATIC;
    r.n_whole = 0;
  }
  finish(r);
  return r;
}

}  // namespace rato_plan
