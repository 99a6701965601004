// Host caller of the shared code of the fragment-end context and the read lengths (csrc/ma_ends_body.h: what k_ma_ends runs on the
// device, a record per lane).
//   ma_ends_driver counts <file.maln> [A] [back]   reads a .maln as ma_hip does, lists the INS_POS pairs by record as mia_hip_ma_tally
//                                           does, runs ma_ends_record over every record (`back`: from the last to the first) and prints
//                                           the records that count and the 1 267 bins, one number per line.  Every array has the exact
//                                           size the device's has -- SEQ and the pairs' characters 16-byte aligned and as long as the next multiple of 16
//                                           behind their last character -- so a read past an end is seen.  ma_ends_bases is checked against a
//                                           loop over the characters for every record.
//   ma_ends_driver dashes                   ma_ends_bases over every offset 0 .. 47 and length 0 .. 80 of two texts, against a loop
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_ends_body.h"
#include "../mapping-iterative-assembler_amd/host/maln_text.h"

namespace {

using namespace mia;

struct Aligned {                           // exactly `bytes` bytes, 16-byte aligned
  char* p = nullptr;
  explicit Aligned(size_t bytes) { if (bytes && posix_memalign((void**)&p, 16, bytes)) p = nullptr; }
  ~Aligned() { free(p); }
};

size_t padded(int64_t T) { return (size_t)((T + MA_PROF_LANE - 1) / MA_PROF_LANE * MA_PROF_LANE); }

int64_t plain_bases(const char* seq, int64_t off, int64_t n) {
  int64_t k = 0;
  for (int64_t x = off; x < off + n; x++) k += seq[x] != '-' ? 1 : 0;
  return k;
}

int counts(const char* fn, bool use_dropped, bool back) {
  maln_text::MalnFile m;
  maln_text::read_maln_file(fn, &m);
  const int64_t n = (int64_t)m.start.size(), T = m.col_off[(size_t)n], n_ins = (int64_t)m.ins_record.size();
  // the pairs by record, as mia_hip_ma_tally lists them
  std::vector<int32_t> rec_ins, ins_list;
  ma_list_pairs(n, n_ins, m.ins_record.data(), m.ins_pos.data(), &rec_ins, &ins_list);
  Aligned seq(padded(T)), ref((size_t)m.L), ib(padded((int64_t)m.ins_bases.size()));
  if ((T && !seq.p) || !ref.p || (!m.ins_bases.empty() && !ib.p)) { fprintf(stderr, "no memory\n"); return 2; }
  if (T) { memset(seq.p, '-', padded(T)); memcpy(seq.p, m.seq.data(), (size_t)T); }      // ('-' behind the end: counted there, it would show)
  memcpy(ref.p, m.ref_seq.data(), (size_t)m.L);
  if (ib.p) { memset(ib.p, '-', padded((int64_t)m.ins_bases.size())); memcpy(ib.p, m.ins_bases.data(), m.ins_bases.size()); }
  std::vector<int32_t> start(m.start.begin(), m.start.end()), ins_pos(m.ins_pos.begin(), m.ins_pos.end());
  std::vector<uint8_t> revcom(m.revcom.begin(), m.revcom.end()), use((size_t)n), seg((size_t)n);
  std::vector<int64_t> col_off(m.col_off.begin(), m.col_off.end()), ins_off(m.ins_off.begin(), m.ins_off.end());
  int64_t n_used = 0;
  for (int64_t r = 0; r < n; r++) {
    use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
    seg[(size_t)r] = (uint8_t)m.rec[(size_t)r].segment;
    n_used += use[(size_t)r];
  }
  const MaEndsView v{n, m.L, start.data(), revcom.data(), col_off.data(), seq.p, rec_ins.data(), ins_list.data(), ins_pos.data(), ins_off.data(),
                     ib.p, ref.p, seg.data(), use.data()};
  std::vector<int64_t> bins((size_t)MA_ENDS_BINS, 0);
  for (int64_t i = 0; i < n; i++) {
    const int64_t r = back ? n - 1 - i : i;
    int events = 0;
    ma_ends_record(v, r, [&](int bin) {
      if (bin < 0 || bin >= MA_ENDS_BINS) { fprintf(stderr, "record %lld: bin %d\n", (long long)r, bin); exit(3); }
      bins[(size_t)bin]++;
      events++;
    });
    const int ends = (ma_ends_has(0, revcom[(size_t)r] != 0, (char)seg[(size_t)r]) ? 1 : 0) + (ma_ends_has(1, revcom[(size_t)r] != 0, (char)seg[(size_t)r]) ? 1 : 0);
    if (events != (use[(size_t)r] ? ends * MA_ENDS_POS + 1 : 0)) { fprintf(stderr, "record %lld: %d events\n", (long long)r, events); return 3; }
    const int64_t cols = col_off[(size_t)r + 1] - col_off[(size_t)r];
    if (ma_ends_bases(seq.p, col_off[(size_t)r], cols) != plain_bases(seq.p, col_off[(size_t)r], cols)) {
      fprintf(stderr, "record %lld: %lld bases by words, %lld one by one\n", (long long)r, (long long)ma_ends_bases(seq.p, col_off[(size_t)r], cols),
              (long long)plain_bases(seq.p, col_off[(size_t)r], cols));
      return 3;
    }
  }
  printf("%lld\n", (long long)n_used);
  for (int b = 0; b < MA_ENDS_BINS; b++) printf("%lld\n", (long long)bins[(size_t)b]);
  return 0;
}

int dashes() {
  const int64_t T = 128;
  Aligned a(padded(T)), b(padded(T));
  if (!a.p || !b.p) return 2;
  for (int64_t x = 0; x < T; x++) {
    a.p[x] = (x * 7 + x / 5) % 3 == 0 ? '-' : "ACGT,.\xad\x2c"[x % 8];        // '-' often; its neighbours in the code table and '-' + 0x80 too
    b.p[x] = '-';
  }
  int64_t checked = 0;
  for (const char* text : {(const char*)a.p, (const char*)b.p})
    for (int64_t off = 0; off < 48; off++)
      for (int64_t n = 0; n <= 80; n++, checked++)
        if (ma_ends_bases(text, off, n) != plain_bases(text, off, n)) { fprintf(stderr, "offset %lld, length %lld\n", (long long)off, (long long)n); return 3; }
  printf("%lld\n", (long long)checked);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "counts")) {
    bool all = false, back = false;
    for (int k = 3; k < argc; k++) { all = all || !strcmp(argv[k], "A"); back = back || !strcmp(argv[k], "back"); }
    return counts(argv[2], all, back);
  }
  if (argc >= 2 && !strcmp(argv[1], "dashes")) return dashes();
  fprintf(stderr, "usage: ma_ends_driver counts <file.maln> [A] [back] | dashes\n");
  return 2;
}
