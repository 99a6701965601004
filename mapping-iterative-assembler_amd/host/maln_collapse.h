// maln_collapse.h -- what ma_hip -u -j does on the host around mia_hip_ma_collapse ("Duplicate consensus"): the SEQ strings
// the device decided put into the records that stay, NUM_INPUTS of those records, and the report of -f 98.  Which records stay, and
// GAPS, are the duplicate filter's (maln_dedup.h: remove_records follows).  The votes are the device's; NUM_INPUTS is summed here,
// because the library is not given it.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "maln_dedup.h"

namespace maln_text {

// What mia_hip_ma_dedup and mia_hip_get_ma_collapse handed out: keep and rep per FILE number, SEQ' in the order of flatten_records
struct CollapseResult {
  std::vector<uint8_t> keep;
  std::vector<int64_t> rep;
  std::string seq;
  int64_t hist[2 * 6 * 6] = {0};
  int64_t molecules = 0, clusters = 0, collapsed = 0, orphans = 0;
};

// vote per position in MalnFile::rec, as the library was given it.  Every kept record takes its columns of SEQ'; every record of a
// representative takes the sum of NUM_INPUTS over the whole or front records of its cluster's voting molecules (at most 2^31 - 1; as
// it was if nobody voted).  A cluster of one molecule keeps both, since it is its own only voter.  Orphans are no cluster.
inline void apply_collapse(MalnFile* m, const DedupInput& in, const CollapseResult& r, const std::vector<uint8_t>& vote) {
  const size_t n = m->rec.size();
  std::vector<int64_t> sum(n, 0);
  std::vector<uint8_t> voted(n, 0);
  auto whole_or_front = [&](size_t f) {
    const int64_t mt = in.mate[f];
    if (mt == -2) return false;
    return mt < 0 || in.start[f] > in.start[(size_t)mt] || (in.start[f] == in.start[(size_t)mt] && (int64_t)f < mt);
  };
  for (size_t f = 0; f < n; f++) {
    if (!whole_or_front(f) || !vote[in.at[f]]) continue;
    const size_t to = (size_t)r.rep[f];
    sum[to] += m->rec[in.at[f]].num_inputs;
    if (sum[to] > INT32_MAX) sum[to] = INT32_MAX;
    voted[to] = 1;
  }
  for (size_t f = 0; f < n; f++) {
    if (!r.keep[f]) continue;
    const size_t k = in.at[f];
    MalnRecord& a = m->rec[k];
    const size_t at = (size_t)m->col_off[k], cols = (size_t)(m->col_off[k + 1] - m->col_off[k]);
    a.seq.assign(r.seq, at, cols);
    a.seq_raw.replace(0, cols, a.seq);
    if (in.mate[f] != -2 && voted[(size_t)r.rep[f]]) a.num_inputs = (int)sum[(size_t)r.rep[f]];
  }
}

// -f 98
inline void collapse_report(FILE* out, const CollapseResult& r, long tolerance) {
  static const char* const sizes[6] = {"2", "3", "4", "5-8", "9-16", "17+"};
  fprintf(out, "# ma_hip duplicate consensus: %lld molecules, %lld clusters, %lld collapsed, %lld orphans, tolerance %ld\n", (long long)r.molecules,
          (long long)r.clusters, (long long)r.collapsed, (long long)r.orphans, tolerance);
  fprintf(out, "# size\tstrand\tclusters\tcolumns\tsplit\tto_base\tto_gap\tto_N\n");
  for (int b = 0; b < 6; b++)
    for (int strand = 0; strand < 2; strand++) {
      fprintf(out, "%s\t%c", sizes[b], strand ? '-' : '+');
      for (int k = 0; k < 6; k++) fprintf(out, "\t%lld", (long long)r.hist[(strand * 6 + b) * 6 + k]);
      fputc('\n', out);
    }
}

}  // namespace maln_text
