// ma_damage_body.h -- the deaminated-fragment filter of a .maln (ma_hip -D, -e, -S, -f 95) as functions of one column, of one stretch
// of flat positions and of one record.  The reference has no such filter: the rule is this project's own ("Deaminated
// fragments"), defined on top of the substitution profile, whose event of a column (ma_prof_bin, ma_profile_body.h: d', i', j' already
// in the read's orientation) is all that is looked at:
//     5' hit at k = 1 .. 15      d' = k - 1,  (i', j') = (C, T)
//     3' hit at k = 1 .. 15      d' = 31 - k, (i', j') = (G, A) for a double-stranded library, (C, T) for a single-stranded one
// MIDDLE, deletions, `beyond` and `bad_code` columns and the columns of a record that is left out are never hits.
// Per record the smallest k of either end is kept as 16 - k (0 = no hit), so that a maximum over a zeroed array finds it.
//
// Plain C++ behind MIA_HD.  k_ma_damage_hits (mia_ma_damage_kernels.h) gives every lane a stretch of MA_DMG_LANE flat positions:
// ma_dmg_stretch is the shared walk (ma_flat_body.h) with this rule: it keeps the best hit of either end of the record it is in in
// registers and hands them to its caller when the walk leaves the record -- at most one call per record of the stretch, and none for
// a record without a hit.  k_ma_damage_molecules gives every lane a record: ma_dmg_record is the shared join of the halves of a read
// split at the origin (ma_molecule_body.h) with this rule: keep for N and the ends mode, and the molecule's class.  A host caller
// (tests/ma_damage_driver.cpp) runs the same code stretch by stretch and record by record.
#pragma once
#include <stdint.h>

#include "ma_molecule_body.h"
#include "ma_profile_body.h"

namespace mia {

constexpr int MA_DMG_LANE = MA_FLAT_LANE;
constexpr int MA_DMG_MAX_POS = 15;                                     // k and N lie in 1 .. 15
constexpr int MA_DMG_CLASSES = MA_DMG_MAX_POS + 1;                     // m5, m3 = 0 .. 15
constexpr int MA_DMG_HIST = 2 * MA_DMG_CLASSES * MA_DMG_CLASSES;       // hist[strand][m5][m3]
constexpr int MA_DMG_ORPHANS = MA_DMG_HIST, MA_DMG_KEPT = MA_DMG_ORPHANS + 1, MA_DMG_BINS = MA_DMG_KEPT + 1;   // 514: hist | orphans | kept records
constexpr int MA_DMG_ANY = 0, MA_DMG_5 = 1, MA_DMG_3 = 2, MA_DMG_BOTH = 3;
inline bool ma_dmg_mate_ok(const int64_t* mate, int64_t n) { return ma_mate_ok(mate, n); }   // (the name it had while it lived here)

MIA_HD inline bool ma_dmg_pos_ok(int n_pos) { return n_pos >= 1 && n_pos <= MA_DMG_MAX_POS; }
MIA_HD inline bool ma_dmg_mode_ok(int mode) { return mode >= MA_DMG_ANY && mode <= MA_DMG_BOTH; }

// What a column yields, from its bin of the profile: 0 = no hit, +k = a 5' hit at k, -k = a 3' hit at k.
MIA_HD inline int ma_dmg_hit(int bin, bool single_stranded) {
  if (bin < 0 || bin >= MA_PROF_COUNTS) return 0;                      // no event, a deletion, bad_code, beyond
  const int d = bin / (MA_PROF_CLASSES * MA_PROF_CLASSES), i = bin / MA_PROF_CLASSES % MA_PROF_CLASSES, j = bin % MA_PROF_CLASSES;
  const bool c_to_t = i == 1 && j == 3, g_to_a = i == 2 && j == 0;
  if (d < MA_PROF_MIDDLE) return c_to_t ? d + 1 : 0;
  if (d > MA_PROF_MIDDLE) return (single_stranded ? c_to_t : g_to_a) ? -(MA_PROF_DEPTHS - d) : 0;
  return 0;
}

// The stretch of flat positions base .. base + MA_DMG_LANE - 1 (base a multiple of MA_DMG_LANE): found(r, h5, h3) is called once for
// every record r of the stretch that has a hit there, h5 / h3 = 16 - (its smallest k at that end inside the stretch), 0 for none.
template <class Found>
MIA_HD inline void ma_dmg_stretch(const MaFlatView& v, bool single_stranded, int64_t base, Found&& found) {
  uint32_t h5 = 0, h3 = 0;
  ma_flat_stretch<false>(
      v, base,
      [&](const MaFlatColumn& c) {
        if (!c.used) return;
        const bool beyond = c.p >= v.L;
        const int hit = ma_dmg_hit(ma_prof_bin(beyond, beyond ? '\0' : v.ref[c.p], c.seq_ch, c.smp_ch, c.rc), single_stranded);
        const uint32_t val = (uint32_t)(MA_DMG_CLASSES - (hit < 0 ? -hit : hit));
        if (hit > 0 && val > h5) h5 = val;
        if (hit < 0 && val > h3) h3 = val;
      },
      [&](int64_t r, bool) {
        if (h5 | h3) found(r, h5, h3);
        h5 = h3 = 0;
      });
}

// The molecule stage's view: what the hits stage left per record, the pairing and the question asked.
struct MaDmgMolView {
  int64_t n;
  const uint8_t* revcom;     // [n]
  const uint8_t* use;        // [n] or NULL
  const int64_t* mate;       // [n] or NULL: MA_MOL_NONE, MA_MOL_ORPHAN or the other half (validated by the caller)
  const uint32_t* hit5;      // [n]: 16 - k of the record's smallest 5' hit, 0 for none
  const uint32_t* hit3;      // [n]
  int32_t n_pos, mode;
  uint8_t* pos5;             // [n] out
  uint8_t* pos3;             // [n] out
  uint8_t* keep;             // [n] out
};

MIA_HD inline bool ma_dmg_keep(int m5, int m3, int n_pos, int mode) {
  const bool k5 = m5 > 0 && m5 <= n_pos, k3 = m3 > 0 && m3 <= n_pos;
  return mode == MA_DMG_5 ? k5 : mode == MA_DMG_3 ? k3 : mode == MA_DMG_BOTH ? (k5 && k3) : (k5 || k3);
}
MIA_HD inline int ma_dmg_hist_bin(int strand, int m5, int m3) { return (strand * MA_DMG_CLASSES + m5) * MA_DMG_CLASSES + m3; }

// Record r: its own pos5 / pos3; and, where r is the lowest-numbered record of its molecule, the molecule's m5 / m3 over its records,
// keep to every record of it, and count(bin) for every bin the molecule adds to (its class if it counts, the orphans, the records kept).
template <class Count>
MIA_HD inline void ma_dmg_record(const MaDmgMolView& v, int64_t r, Count&& count) {
  uint32_t h5 = v.hit5[r], h3 = v.hit3[r];
  v.pos5[r] = (uint8_t)(h5 ? MA_DMG_CLASSES - h5 : 0);
  v.pos3[r] = (uint8_t)(h3 ? MA_DMG_CLASSES - h3 : 0);
  ma_molecule_join(
      v.mate, v.use, r, MA_DMG_ORPHANS, MA_DMG_KEPT,
      [&](int64_t m, int* bin) {
        if (m >= 0) {
          const uint32_t o5 = v.hit5[m], o3 = v.hit3[m];
          if (o5 > h5) h5 = o5;
          if (o3 > h3) h3 = o3;
        }
        const int m5 = h5 ? MA_DMG_CLASSES - (int)h5 : 0, m3 = h3 ? MA_DMG_CLASSES - (int)h3 : 0;
        const bool k = ma_dmg_keep(m5, m3, v.n_pos, v.mode);
        v.keep[r] = k ? 1 : 0;
        if (m >= 0) v.keep[m] = k ? 1 : 0;
        *bin = ma_dmg_hist_bin(v.revcom[r] != 0 ? 1 : 0, m5, m3);
        return k;
      },
      count);
}

// ---- the report (host) ------------------------------------------------------------------------------------------------------------
// Row N of -f 95 for one strand (0, 1; 2 = both): the molecules with 0 < m5 <= N, with 0 < m3 <= N, with both, with either.
inline void ma_dmg_row(const int64_t* hist, int strand, int n_pos, int64_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  for (int s = 0; s < 2; s++) {
    if (strand < 2 && s != strand) continue;
    for (int m5 = 0; m5 < MA_DMG_CLASSES; m5++)
      for (int m3 = 0; m3 < MA_DMG_CLASSES; m3++) {
        const int64_t c = hist[ma_dmg_hist_bin(s, m5, m3)];
        const bool k5 = m5 > 0 && m5 <= n_pos, k3 = m3 > 0 && m3 <= n_pos;
        if (k5) out[0] += c;
        if (k3) out[1] += c;
        if (k5 && k3) out[2] += c;
        if (k5 || k3) out[3] += c;
      }
  }
}

}  // namespace mia
