// ma_profile_body.h -- the substitution profile of a .maln (ma_hip -f 9, -f 91) as functions of one column of one record.  The
// reference has no such report: the rule is this project's own ("Substitution profile").  A column c of a selected
// record (START, RC) with SEQ character s and SMP character m, on reference column p = START + c of L, is one event:
//     p >= L                     bin MA_PROF_BEYOND (the record of a circular assembly that ends on column L)
//     d = m - 'A' outside 0..30  bin MA_PROF_BAD
//     s == '-'                   bin MA_PROF_DEL + d'                      d' = RC ? 30 - d : d
//     else                       bin (d' * 5 + i') * 5 + j'                i, j = class of toupper(ref[p]), toupper(s): ACGT 0..3, else 4;
//                                                                          RC mirrors a class k < 4 to 3 - k (revcom_submat, src/pssm.c:53-91)
// The 808 bins are count[31][5][5] | del[31] | bad_code | beyond.
//
// Plain C++ behind MIA_HD.  k_ma_profile (mia_ma_profile_kernels.h) gives every lane a stretch of MA_PROF_LANE flat positions of
// the records' concatenated SEQ / SMP strings: ma_prof_stretch is the shared walk (ma_flat_body.h) that hands every position's bin
// to its caller; a host caller (tests/ma_profile_driver.cpp) runs the same code stretch by stretch.
// Labels and scores of the two reports (host/ma_main.cpp) are at the end.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "ma_flat_body.h"

namespace mia {

constexpr int MA_PROF_DEPTHS = 31, MA_PROF_CLASSES = 5, MA_PROF_MIDDLE = 15;
constexpr int MA_PROF_COUNTS = MA_PROF_DEPTHS * MA_PROF_CLASSES * MA_PROF_CLASSES;                 // 775
constexpr int MA_PROF_DEL = MA_PROF_COUNTS, MA_PROF_BAD = MA_PROF_DEL + MA_PROF_DEPTHS, MA_PROF_BEYOND = MA_PROF_BAD + 1, MA_PROF_BINS = MA_PROF_BEYOND + 1;   // 808
constexpr int MA_PROF_LANE = MA_FLAT_LANE;
// the view and the bisection under the names they had while they lived here (ma_flat_body.h has them now): callers written for those
using MaProfView = MaFlatView;
MIA_HD inline int64_t ma_prof_record_of(const MaFlatView& v, int64_t pos) { return ma_flat_record_of(v, pos); }
constexpr int MA_PROF_HOT = 4;             // (MIDDLE, X, X) for X in ACGT: where most events of a real assembly fall

MIA_HD inline int ma_prof_class(char c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}
MIA_HD inline int ma_prof_mirror(int k) { return k < 4 ? 3 - k : 4; }

// the bin of one column event; ref_ch is not looked at when `beyond`
MIA_HD inline int ma_prof_bin(bool beyond, char ref_ch, char seq_ch, char smp_ch, bool rc) {
  if (beyond) return MA_PROF_BEYOND;
  int d = (int)(unsigned char)smp_ch - 'A';
  if (d < 0 || d >= MA_PROF_DEPTHS) return MA_PROF_BAD;
  if (rc) d = MA_PROF_DEPTHS - 1 - d;
  if (seq_ch == '-') return MA_PROF_DEL + d;
  int i = ma_prof_class(ref_ch), j = ma_prof_class(seq_ch);
  if (rc) { i = ma_prof_mirror(i); j = ma_prof_mirror(j); }
  return (d * MA_PROF_CLASSES + i) * MA_PROF_CLASSES + j;
}

// 0 .. 3 for the bins (MIDDLE, X, X), X = A, C, G, T; -1 for every other bin (and for "no event", bin -1)
MIA_HD inline int ma_prof_hot(int bin) {
  const int k = bin - MA_PROF_MIDDLE * MA_PROF_CLASSES * MA_PROF_CLASSES;
  return k >= 0 && k < 4 * (MA_PROF_CLASSES + 1) && k % (MA_PROF_CLASSES + 1) == 0 ? k / (MA_PROF_CLASSES + 1) : -1;
}
MIA_HD inline int ma_prof_hot_bin(int h) { return MA_PROF_MIDDLE * MA_PROF_CLASSES * MA_PROF_CLASSES + h * (MA_PROF_CLASSES + 1); }

// The stretch of flat positions base .. base + MA_PROF_LANE - 1 (base a multiple of MA_PROF_LANE; the walk: ma_flat_body.h): emit(bin)
// is called MA_PROF_LANE times, in order, with the position's bin -- or with -1 for a position at or behind T and for a column of a
// record that is left out.  Every caller makes all MA_PROF_LANE calls whatever its base, so a wavefront's lanes reach each of them
// together.
template <class Emit>
MIA_HD inline void ma_prof_stretch(const MaFlatView& v, int64_t base, Emit&& emit) {
  ma_flat_stretch<true>(
      v, base,
      [&](const MaFlatColumn& c) {
        int bin = -1;
        if (c.live && c.used) {
          const bool beyond = c.p >= v.L;
          bin = ma_prof_bin(beyond, beyond ? '\0' : v.ref[c.p], c.seq_ch, c.smp_ch, c.rc);
        }
        emit(bin);
      },
      [](int64_t, bool) {});
}

// ---- the two reports (host) ---------------------------------------------------------------------------------------------------
// the labels of the shipped matrix files: 1 .. 15, MIDDLE, -15 .. -1
inline void ma_prof_label(int d, char out[16]) {
  if (d == MA_PROF_MIDDLE) snprintf(out, 16, "MIDDLE");
  else snprintf(out, 16, "%d", d < MA_PROF_MIDDLE ? d + 1 : d - MA_PROF_DEPTHS);
}

// The entry of a -f 91 matrix for ref class i (row = count[d][i][0 .. 3]) and read class j, in the reference's unit
// (find_phred_qscore reads a score as pow(2, score / 100); the flat match 200 = 100 * log2(1 / 0.25)):
// floor(100 * log2(((row[j] + alpha) / (N + 4 alpha)) / 0.25) + 0.5), N the row's sum.  A row without a count is the flat row.
// The quotient is at most 1 / 0.25 and, with a row sum below 2^63, at least 4 alpha / 2^63 (alpha <= 1): an entry lies in
// 100 * (log2(alpha) - 61) .. 200, that is -6 100 .. 200 for alpha = 1 and -26 100 .. 200 for alpha = MA_PROF_MIN_ALPHA -- inside
// the +-32 000 mia_hip_set_pssm accepts, so nothing is clamped.  A smaller alpha would leave that range (and a subnormal one the
// range of int; 4 alpha that overflows makes the quotient 0): ma_prof_alpha_ok refuses an alpha outside 1e-60 .. 1e60 along
// with alpha <= 0 and what is not finite.
constexpr double MA_PROF_MIN_ALPHA = 1e-60, MA_PROF_MAX_ALPHA = 1e60;
inline bool ma_prof_alpha_ok(double alpha) { return isfinite(alpha) && alpha >= MA_PROF_MIN_ALPHA && alpha <= MA_PROF_MAX_ALPHA; }
inline int ma_prof_score(const int64_t row[4], int i, int j, double alpha) {
  const int64_t N = row[0] + row[1] + row[2] + row[3];
  if (N == 0) return i == j ? 200 : -600;
  return (int)floor(100.0 * log2((((double)row[j] + alpha) / ((double)N + 4.0 * alpha)) / 0.25) + 0.5);
}

}  // namespace mia
