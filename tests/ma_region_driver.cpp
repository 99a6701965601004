// Host caller of the region view's shared code (csrc/ma_region_body.h: the functions k_ma_region_select and
// k_ma_region_render run on the device): reads a .maln as ma_hip does, selects the records that overlap the region and
// renders their rows on the CPU, and prints the record lines of `ma -f 6`.
//   ma_region_driver <file.maln> [<-R argument>]
#include <stdio.h>

#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_region_body.h"
#include "../mapping-iterative-assembler_amd/host/maln_text.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ma_region_driver <file.maln> [<start:end>]\n"); return 2; }
  maln_text::MalnFile m;
  maln_text::read_maln_file(argv[1], &m);
  int reg_start = 90, reg_end = 109, first = 0, last = -1;
  if (argc > 2) maln_text::parse_region(argv[2], &reg_start, &reg_end);
  maln_text::clamp_region(reg_start, reg_end, m.L, &first, &last);
  const int64_t n = (int64_t)m.start.size();
  // the pairs by record, as mia_hip_ma_tally lists them for the device
  std::vector<int32_t> rec_ins, ins_list;
  mia::ma_list_pairs(n, (int64_t)m.ins_record.size(), m.ins_record.data(), m.ins_pos.data(), &rec_ins, &ins_list);
  std::vector<int64_t> colmap(1, 0);
  for (int p = first; p <= last; p++) colmap.push_back(colmap.back() + mia::ma_region_gap(m.gaps[(size_t)p]) + 1);
  mia::MaRegionView v{n, m.start.data(), m.col_off.data(), m.seq.data(), rec_ins.data(), ins_list.data(), m.ins_pos.data(), m.ins_off.data(),
                      m.ins_bases.data(), m.gaps.data(), first, last, colmap.data()};
  std::string row((size_t)colmap.back(), '\0');
  for (int64_t r = 0; r < n; r++) {
    if (!mia::ma_region_overlaps(m.start[(size_t)r], mia::ma_region_end(v, r), first, last)) continue;
    mia::ma_region_row(v, r, &row[0], 0, 1);
    printf("%-20.20s %s\n", maln_text::region_label(m.rec[(size_t)r]).c_str(), row.c_str());
  }
  return 0;
}
