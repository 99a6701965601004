// ma_pmd_body.h -- the damage score of a .maln (ma_hip -L, -K, -S, -f 97) as functions of one column, of one stretch of flat positions
// and of one record.  The reference has no such step: the rule is this project's own ("Damage score"), defined on top of the
// substitution profile.  The primitive is a weight table w[31][5][5] (int32, units of 2^-16 nat), indexed exactly like `count` of the
// profile: a column whose event (ma_prof_bin, ma_profile_body.h: d', i', j' already in the read's orientation) is a count adds
// w[d'][i'][j'] to its record's score; deletions, `beyond` and `bad_code` columns and the columns of a record that is left out add
// nothing.  A molecule's score S is the sum over its records (halves paired by mate, as for the deaminated-fragment filter); it is kept
// when S >= threshold, and hist[strand][bin] counts the molecules by bin = clamp(floor(S / 32768) + 20, 0, 63), half a nat per bin.
//
// Plain C++ behind MIA_HD.  k_ma_score_cols (mia_ma_pmd_kernels.h) gives every lane a stretch of MA_PMD_LANE flat positions:
// ma_pmd_stretch is the shared walk (ma_flat_body.h) with this rule: it sums the weights of the record it is in in a register and hands
// the sum to its caller when the walk leaves the record -- at most one call per record of the stretch, and none for a sum of zero.
// k_ma_score_molecules gives every lane a record: ma_pmd_record is the shared join (ma_molecule_body.h) with this rule: it adds the
// halves, decides keep and names the molecule's bin.  A host caller (tests/ma_pmd_driver.cpp) runs the same code stretch by stretch
// and record by record.  The model that fills the table from four parameters (ma_pmd_model, host only) is at the end.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ma_damage_body.h"

namespace mia {

constexpr int MA_PMD_LANE = MA_FLAT_LANE;
constexpr int MA_PMD_WEIGHTS = MA_PROF_COUNTS;                         // 775: w[31][5][5]
constexpr int32_t MA_PMD_MAX_WEIGHT = 1 << 20;                         // |w| of an entry: 16 positions of a lane stay inside int32
constexpr int MA_PMD_HIST_BINS = 64, MA_PMD_HIST = 2 * MA_PMD_HIST_BINS;           // hist[strand][bin]
constexpr int MA_PMD_ORPHANS = MA_PMD_HIST, MA_PMD_KEPT = MA_PMD_ORPHANS + 1, MA_PMD_BINS = MA_PMD_KEPT + 1;   // 130: hist | orphans | kept records
constexpr int64_t MA_PMD_BIN_UNITS = 32768;                            // half a nat
constexpr int MA_PMD_BIN_ZERO = 20;                                    // the bin of 0 <= S < 32768

// every entry within +-MA_PMD_MAX_WEIGHT (host: the entry point's check)
inline bool ma_pmd_weights_ok(const int32_t* w) {
  for (int b = 0; b < MA_PMD_WEIGHTS; b++)
    if (w[b] > MA_PMD_MAX_WEIGHT || w[b] < -MA_PMD_MAX_WEIGHT) return false;
  return true;
}

// What a column adds: the entry of its bin of the profile; nothing for no event, a deletion, bad_code, beyond.
MIA_HD inline int32_t ma_pmd_weight(const int32_t* w, bool beyond, char ref_ch, char seq_ch, char smp_ch, bool rc) {
  const int bin = ma_prof_bin(beyond, ref_ch, seq_ch, smp_ch, rc);
  return bin < MA_PROF_COUNTS ? w[bin] : 0;
}

// The stretch of flat positions base .. base + MA_PMD_LANE - 1 (base a multiple of MA_PMD_LANE): found(r, sum) is called once for
// every record r of the stretch whose columns there add up to something other than zero (|sum| <= 16 * MA_PMD_MAX_WEIGHT).
template <class Found>
MIA_HD inline void ma_pmd_stretch(const MaFlatView& v, const int32_t* w, int64_t base, Found&& found) {
  int32_t sum = 0;
  ma_flat_stretch<false>(
      v, base,
      [&](const MaFlatColumn& c) {
        if (!c.used) return;
        const bool beyond = c.p >= v.L;
        sum += ma_pmd_weight(w, beyond, beyond ? '\0' : v.ref[c.p], c.seq_ch, c.smp_ch, c.rc);
      },
      [&](int64_t r, bool) {
        if (sum) found(r, sum);
        sum = 0;
      });
}

// The molecule stage's view: what the column stage left per record, the pairing and the threshold.
struct MaPmdMolView {
  int64_t n;
  const uint8_t* revcom;     // [n]
  const uint8_t* use;        // [n] or NULL
  const int64_t* mate;       // [n] or NULL: MA_MOL_NONE, MA_MOL_ORPHAN or the other half (validated by the caller)
  const int64_t* rec_score;  // [n]: the sum of the record's weights
  int64_t threshold;
  int64_t* mol_score;        // [n] out: the score of the record's molecule
  uint8_t* keep;             // [n] out
};

// bin = clamp(floor(S / 32768) + 20, 0, 63): a floor division, also for a negative S
MIA_HD inline int ma_pmd_bin(int64_t S) {
  int64_t q = S / MA_PMD_BIN_UNITS;
  if (S % MA_PMD_BIN_UNITS < 0) q--;
  q += MA_PMD_BIN_ZERO;
  return q < 0 ? 0 : q >= MA_PMD_HIST_BINS ? MA_PMD_HIST_BINS - 1 : (int)q;
}
MIA_HD inline int ma_pmd_hist_bin(int strand, int64_t S) { return strand * MA_PMD_HIST_BINS + ma_pmd_bin(S); }

// Record r, where it is the lowest-numbered record of its molecule: the molecule's S over its records, S and keep to every record of
// it, and count(bin) for every bin the molecule adds to (its bin if it counts, the orphans, the records kept).
template <class Count>
MIA_HD inline void ma_pmd_record(const MaPmdMolView& v, int64_t r, Count&& count) {
  ma_molecule_join(
      v.mate, v.use, r, MA_PMD_ORPHANS, MA_PMD_KEPT,
      [&](int64_t m, int* bin) {
        int64_t S = v.rec_score[r];
        if (m >= 0) S += v.rec_score[m];
        const bool k = S >= v.threshold;
        v.mol_score[r] = S;
        v.keep[r] = k ? 1 : 0;
        if (m >= 0) { v.mol_score[m] = S; v.keep[m] = k ? 1 : 0; }
        *bin = ma_pmd_hist_bin(v.revcom[r] != 0 ? 1 : 0, S);
        return k;
      },
      count);
}

// ---- the model and the report (host) ----------------------------------------------------------------------------------------------
// The table of a briggs-like damage model: a C of the reference is read as T with probability D_CT(d') = c0 + g(k) near an end, g(k) =
// p (1 - p)^(k - 1), k = d' + 1 from the 5' end (d' <= 14), 31 - d' from the 3' end (d' >= 16; a single-stranded library only); a G as
// A with D_GA(d') = c0 + g(31 - d') near the 3' end of a double-stranded library.  With the polymorphism rate pi and the error rate eps
// a match has likelihood L(D) = (1 - pi)(1 - eps)(1 - D) + (1 - pi) eps D + pi eps (1 - D), and the entries are the log likelihood
// ratios against D = 0 in units of 2^-16 nat, q(x) = floor(x * 65536 + 0.5):
//     w[d'][C][C] = q(ln(L(D_CT) / L(0)))    w[d'][C][T] = q(ln((1 - L(D_CT)) / (1 - L(0))))    (G, G) and (G, A) likewise with D_GA (ds)
// Every other entry is 0.  false for a parameter that is not finite or outside 0 < p < 1, 0 <= c0 < 1, 0 < pi < 1, 0 < eps < 1, for
// D >= 1 at some code, and for parameters so small that a ratio is no finite number.
inline bool ma_pmd_model(double p, double c0, double pi, double eps, bool single_stranded, int32_t* w) {
  if (!isfinite(p) || !isfinite(c0) || !isfinite(pi) || !isfinite(eps)) return false;
  if (!(p > 0.0 && p < 1.0 && c0 >= 0.0 && c0 < 1.0 && pi > 0.0 && pi < 1.0 && eps > 0.0 && eps < 1.0)) return false;
  auto like = [&](double D) { return (1.0 - pi) * (1.0 - eps) * (1.0 - D) + (1.0 - pi) * eps * D + pi * eps * (1.0 - D); };
  auto g = [&](int k) { return p * pow(1.0 - p, (double)(k - 1)); };
  auto q = [](double x, int32_t* out) {
    const double u = floor(x * 65536.0 + 0.5);
    if (!isfinite(u) || fabs(u) > 2147483647.0) return false;
    *out = (int32_t)u;
    return true;
  };
  for (int b = 0; b < MA_PMD_WEIGHTS; b++) w[b] = 0;
  const double L0 = like(0.0);
  for (int d = 0; d < MA_PROF_DEPTHS; d++) {
    const double g5 = d < MA_PROF_MIDDLE ? g(d + 1) : 0.0, g3 = d > MA_PROF_MIDDLE ? g(MA_PROF_DEPTHS - d) : 0.0;
    const double D_ct = c0 + g5 + (single_stranded ? g3 : 0.0), D_ga = c0 + g3;
    if (!(D_ct < 1.0) || !(D_ga < 1.0)) return false;
    int32_t* const wd = w + d * MA_PROF_CLASSES * MA_PROF_CLASSES;
    if (!q(log(like(D_ct) / L0), &wd[1 * MA_PROF_CLASSES + 1]) || !q(log((1.0 - like(D_ct)) / (1.0 - L0)), &wd[1 * MA_PROF_CLASSES + 3])) return false;
    if (single_stranded) continue;         // G rows carry no weight
    if (!q(log(like(D_ga) / L0), &wd[2 * MA_PROF_CLASSES + 2]) || !q(log((1.0 - like(D_ga)) / (1.0 - L0)), &wd[2 * MA_PROF_CLASSES + 0])) return false;
  }
  return true;
}

// the lower bound of a bin in nat (bin 0 has none), and row b of -f 97 for one strand (0, 1; 2 = both): the molecules in the bin, and
// those in this bin or above
inline double ma_pmd_bin_from(int b) { return (double)(b - MA_PMD_BIN_ZERO) / 2.0; }
inline void ma_pmd_row(const int64_t* hist, int strand, int b, int64_t out[2]) {
  out[0] = out[1] = 0;
  for (int s = 0; s < 2; s++) {
    if (strand < 2 && s != strand) continue;
    out[0] += hist[s * MA_PMD_HIST_BINS + b];
    for (int k = b; k < MA_PMD_HIST_BINS; k++) out[1] += hist[s * MA_PMD_HIST_BINS + k];
  }
}

}  // namespace mia
