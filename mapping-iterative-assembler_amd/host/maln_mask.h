// maln_mask.h -- what ma_hip -E / -x does on the host around mia_hip_ma_mask ("End mask"): the option's two numbers, the
// record view the device made put back into the MalnFile, and the report of -f 96.  The decision -- which columns of which record
// stay, which pairs, which bases become N -- is the device's; emptied records leave through remove_records (maln_dedup.h), which
// also resets GAPS from the pairs that remain.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "maln_dedup.h"

namespace maln_text {

// -E n5[,n3]: whole numbers, n3 = n5 when only one is given.  false for anything else (the range is the library's to judge).
inline bool parse_mask_ends(const char* s, long* n5, long* n3) {
  char* end = nullptr;
  *n5 = strtol(s, &end, 10);
  if (end == s || *n5 < 0 || *n5 > 1000) return false;
  if (!*end) { *n3 = *n5; return true; }
  if (*end != ',') return false;
  const char* t = end + 1;
  *n3 = strtol(t, &end, 10);
  return end != t && !*end && *n3 >= 0 && *n3 <= 1000;
}

// What mia_hip_get_ma_mask handed out, in the record and pair order of flatten_records.
struct MaskResult {
  std::vector<int32_t> first, count, start, ins_pos;
  std::vector<int64_t> col_off;
  std::vector<uint8_t> pair_keep;
  std::string seq, smp;
  int64_t hist[2 * 2 * 16] = {0}, scalars[6] = {0};
};

// The masked file.  Trim mode: every record keeps columns first .. first + count - 1 and the pairs the device kept, at their new
// positions; a record with count 0 leaves; the records are sorted again, as reading the masked file would.  Substitution mode: the SEQ characters of columns START .. END are the device's.
inline void apply_mask(MalnFile* m, const MaskResult& r, bool substitute) {
  const size_t n = m->rec.size();
  std::vector<uint8_t> keep(n, 1);
  size_t e = 0;
  for (size_t k = 0; k < n; k++) {
    MalnRecord& a = m->rec[k];
    const size_t at = (size_t)r.col_off[k], cols = (size_t)r.count[k];
    if (substitute) {
      a.seq.assign(r.seq, at, cols);
      a.seq_raw.replace(0, cols, a.seq);
      e += a.ins_pos.size();
      continue;
    }
    keep[k] = cols ? 1 : 0;
    std::vector<int32_t> pos;
    std::vector<std::string> bases;
    for (size_t p = 0; p < a.ins_pos.size(); p++, e++)
      if (cols && r.pair_keep[e]) { pos.push_back(r.ins_pos[e]); bases.push_back(std::move(a.ins_seq[p])); }
    if (!cols) continue;
    a.ins_pos.swap(pos);
    a.ins_seq.swap(bases);
    a.end = a.start + r.first[k] + (int)cols - 1;
    a.start = r.start[k];
    a.seq.assign(r.seq, at, cols);
    a.smp.assign(r.smp, at, cols);
    a.seq_raw = a.seq;
    a.smp_raw = a.smp;
  }
  if (substitute) { flatten_records(m); return; }
  remove_records(m, keep);
  sort_records(m);                          // (START moved: the order read_ma would give the masked file)
  flatten_records(m);
}

// -f 96
inline void mask_report(FILE* out, int64_t n_in, const MaskResult& r, bool substitute, bool single_stranded) {
  fprintf(out, "# ma_hip end mask: %lld records, %lld kept, %lld %lld emptied, %lld inserts dropped, %lld gap columns stripped, mode %s, library %s\n", (long long)n_in,
          (long long)r.scalars[4], (long long)r.scalars[0], (long long)r.scalars[1], (long long)r.scalars[3], (long long)r.scalars[2], substitute ? "N" : "trim",
          single_stranded ? "ss" : "ds");
  fprintf(out, "# k\t5p+\t5p-\t3p+\t3p-\n");
  for (int k = 1; k <= 15; k++)
    fprintf(out, "%d\t%lld\t%lld\t%lld\t%lld\n", k, (long long)r.hist[(0 * 2 + 0) * 16 + k], (long long)r.hist[(1 * 2 + 0) * 16 + k], (long long)r.hist[(0 * 2 + 1) * 16 + k],
            (long long)r.hist[(1 * 2 + 1) * 16 + k]);
}

}  // namespace maln_text
