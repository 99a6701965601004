// Host caller of the substitution profile's shared code (csrc/ma_profile_body.h: what k_ma_profile runs on the device).
//   ma_profile_driver bins <table>          the table holds records of six bytes: flags (bit 0 RC, bit 1 beyond), the reference's
//                                           character, the SEQ character, the SMP character, the bin as int16 (little endian);
//                                           every one is checked against ma_prof_bin; prints how many were
//   ma_profile_driver profile <file.maln> [A]   reads a .maln as ma_hip does and prints the records that count and the 808 bins, one
//                                           number per line.  The bins are made twice -- record by record and column by column,
//                                           and over the flat columns in stretches of MA_PROF_LANE as the kernel's lanes take them,
//                                           every stretch of every workgroup chunk, those behind the last column too -- and both
//                                           must agree.  SEQ and SMP lie in buffers that end where the kernel's may end.
//   ma_profile_driver scores <file>         lines "<alpha> <i> <c0> <c1> <c2> <c3>": prints the four scores of the row; then the labels
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_profile_body.h"
#include "../mapping-iterative-assembler_amd/host/maln_text.h"

namespace {

using namespace mia;

int check_bins(const char* fn) {
  std::string buf;
  if (!maln_text::slurp(fn, &buf) || buf.size() % 6) { fprintf(stderr, "cannot read %s as a table\n", fn); return 2; }
  for (size_t at = 0; at < buf.size(); at += 6) {
    const unsigned char* e = (const unsigned char*)buf.data() + at;
    const int want = (int)(int16_t)(uint16_t)(e[4] | (e[5] << 8));
    const int got = ma_prof_bin((e[0] & 2) != 0, (char)e[1], (char)e[2], (char)e[3], (e[0] & 1) != 0);
    if (got != want) {
      fprintf(stderr, "entry %zu: flags %d, reference %d, SEQ %d, SMP %d: bin %d, the table says %d\n", at / 6, e[0], e[1], e[2], e[3], got, want);
      return 1;
    }
  }
  printf("%zu\n", buf.size() / 6);
  return 0;
}

struct Aligned {                           // exactly `bytes` bytes, 16-byte aligned
  char* p = nullptr;
  explicit Aligned(size_t bytes) { if (bytes && posix_memalign((void**)&p, 16, bytes)) p = nullptr; }
  ~Aligned() { free(p); }
};

int profile(const char* fn, bool use_dropped) {
  maln_text::MalnFile m;
  maln_text::read_maln_file(fn, &m);
  const int64_t n = (int64_t)m.start.size(), T = m.col_off[(size_t)n];
  std::vector<uint8_t> use((size_t)n + 1, 1);
  int64_t n_used = 0;
  for (int64_t r = 0; r < n; r++) { use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0; n_used += use[(size_t)r]; }
  // record by record
  std::vector<int64_t> plain((size_t)MA_PROF_BINS, 0), flat((size_t)MA_PROF_BINS, 0);
  for (int64_t r = 0; r < n; r++) {
    if (!use[(size_t)r]) continue;
    for (int64_t x = m.col_off[(size_t)r]; x < m.col_off[(size_t)r + 1]; x++) {
      const int64_t p = (int64_t)m.start[(size_t)r] + (x - m.col_off[(size_t)r]);
      plain[(size_t)ma_prof_bin(p >= m.L, p >= m.L ? '\0' : m.ref_seq[(size_t)p], m.seq[(size_t)x], m.smp[(size_t)x], m.revcom[(size_t)r] != 0)]++;
    }
  }
  // over the flat columns
  const size_t padded = (size_t)((T + MA_PROF_LANE - 1) / MA_PROF_LANE * MA_PROF_LANE);
  Aligned seq(padded), smp(padded);
  Aligned ref((size_t)m.L);
  if ((padded && (!seq.p || !smp.p)) || !ref.p) { fprintf(stderr, "no memory\n"); return 2; }
  if (padded) { memset(seq.p, '?', padded); memset(smp.p, '?', padded); memcpy(seq.p, m.seq.data(), (size_t)T); memcpy(smp.p, m.smp.data(), (size_t)T); }
  memcpy(ref.p, m.ref_seq.data(), (size_t)m.L);
  std::vector<int32_t> start(m.start.begin(), m.start.end());           // (exact sizes: a read past the end is seen)
  std::vector<uint8_t> revcom(m.revcom.begin(), m.revcom.end()), use_n(use.begin(), use.begin() + n);
  std::vector<int64_t> col_off(m.col_off.begin(), m.col_off.end());
  const MaProfView v{n, T, m.L, start.data(), revcom.data(), col_off.data(), seq.p, smp.p, ref.p, use_n.data()};
  const int64_t chunk = 256 * MA_PROF_LANE, all = (T + chunk - 1) / chunk * chunk;
  int64_t calls = 0, hot = 0;
  for (int64_t base = 0; base < all; base += MA_PROF_LANE) {
    int k = 0;
    ma_prof_stretch(v, base, [&](int bin) {
      calls++;
      if (base + k >= T && bin != -1) { fprintf(stderr, "flat position %lld behind the last column has bin %d\n", (long long)(base + k), bin); exit(3); }
      if (bin >= 0) {
        flat[(size_t)bin]++;
        const int h = ma_prof_hot(bin);
        if (h >= 0) { hot++; if (ma_prof_hot_bin(h) != bin) { fprintf(stderr, "hot bin %d of %d\n", h, bin); exit(3); } }
      }
      k++;
    });
    if (k != MA_PROF_LANE) { fprintf(stderr, "stretch %lld made %d calls\n", (long long)base, k); return 3; }
    if (base < T && ma_prof_record_of(v, base) != (int64_t)(std::upper_bound(col_off.begin(), col_off.end(), base) - col_off.begin()) - 1) {
      fprintf(stderr, "flat position %lld: the bisection finds another record\n", (long long)base);
      return 3;
    }
  }
  for (int b = 0; b < MA_PROF_BINS; b++)
    if (flat[(size_t)b] != plain[(size_t)b]) { fprintf(stderr, "bin %d: %lld over the flat columns, %lld record by record\n", b, (long long)flat[(size_t)b], (long long)plain[(size_t)b]); return 3; }
  if (hot != flat[(size_t)ma_prof_hot_bin(0)] + flat[(size_t)ma_prof_hot_bin(1)] + flat[(size_t)ma_prof_hot_bin(2)] + flat[(size_t)ma_prof_hot_bin(3)]) { fprintf(stderr, "hot bins\n"); return 3; }
  printf("%lld\n", (long long)n_used);
  for (int b = 0; b < MA_PROF_BINS; b++) printf("%lld\n", (long long)flat[(size_t)b]);
  return 0;
}

int scores(const char* fn) {
  FILE* f = fopen(fn, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", fn); return 2; }
  double alpha;
  int i;
  long long c[4];
  while (fscanf(f, "%lf %d %lld %lld %lld %lld", &alpha, &i, &c[0], &c[1], &c[2], &c[3]) == 6) {
    const int64_t row[4] = {c[0], c[1], c[2], c[3]};
    if (!ma_prof_alpha_ok(alpha)) { printf("refused\n"); continue; }
    printf("%d %d %d %d\n", ma_prof_score(row, i, 0, alpha), ma_prof_score(row, i, 1, alpha), ma_prof_score(row, i, 2, alpha), ma_prof_score(row, i, 3, alpha));
  }
  fclose(f);
  for (int d = 0; d < MA_PROF_DEPTHS; d++) {
    char label[16];
    ma_prof_label(d, label);
    printf("%s\n", label);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "bins")) return check_bins(argv[2]);
  if (argc >= 3 && !strcmp(argv[1], "profile")) return profile(argv[2], argc >= 4 && !strcmp(argv[3], "A"));
  if (argc >= 3 && !strcmp(argv[1], "scores")) return scores(argv[2]);
  fprintf(stderr, "usage: ma_profile_driver bins <table> | profile <file.maln> [A] | scores <file>\n");
  return 2;
}
