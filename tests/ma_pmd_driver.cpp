// Host caller of the shared code of the damage score (csrc/ma_pmd_body.h: what the kernels of mia_ma_pmd_kernels.h run per lane):
// ma_pmd_stretch over every stretch of 16 flat positions, added into score[r] as the device's atomics do, then ma_pmd_record over every
// record, for every weight table and threshold of the input.  Every array ends where the device's may end -- SEQ and SMP on the next
// multiple of 16 behind their last character, everything else on its last element -- and is heap memory of its own, so that
// AddressSanitizer sees every index.  Beside it a loop record by record and column by column that shares ma_pmd_weight and
// ma_prof_bin alone; the two must agree.  The results are printed for the test to compare with its own restatement
// (tests/ma_pmd_ref.py), which shares nothing.
//
//   ma_pmd_driver <file>     file: "L n T", the reference, ">" + SEQ, ">" + SMP (flat), n lines "start rc use mate col_off_end", then
//                            "tables thresholds" and per table its 775 weights followed by its thresholds
//   output per table: "rec ..", then per threshold "threshold molecules kept orphans", keep as a string of 0 / 1 ("-" without records),
//   "mol .." and the bins of hist that are not zero as "bin count" pairs
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_pmd_body.h"
#include "ma_driver_util.h"

using namespace mia;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ma_pmd_driver <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  long long L = 0, n = 0, T = 0;
  if (fscanf(f, "%lld %lld %lld\n", &L, &n, &T) != 3) { fprintf(stderr, "bad header\n"); return 2; }
  const std::string ref_s = line_of(f), seq_s = line_of(f).substr(1), smp_s = line_of(f).substr(1);
  if ((long long)ref_s.size() != L || (long long)seq_s.size() != T || (long long)smp_s.size() != T) { fprintf(stderr, "bad strings\n"); return 2; }
  const size_t padded = (size_t)(T + MA_PMD_LANE - 1) / MA_PMD_LANE * MA_PMD_LANE;
  Exact<char> ref((size_t)L), seq(padded, 16), smp(padded, 16);
  Exact<int32_t> start((size_t)n), w(MA_PMD_WEIGHTS);
  Exact<uint8_t> revcom((size_t)n), use((size_t)n), keep((size_t)n);
  Exact<int64_t> col_off((size_t)n + 1), mate((size_t)n), rec((size_t)n), mol((size_t)n);
  memcpy(ref.p, ref_s.data(), (size_t)L);
  if (T) { memcpy(seq.p, seq_s.data(), (size_t)T); memcpy(smp.p, smp_s.data(), (size_t)T); }
  bool all_used = true;
  for (long long r = 0; r < n; r++) {
    long long s, rc, u, m, e;
    if (fscanf(f, "%lld %lld %lld %lld %lld", &s, &rc, &u, &m, &e) != 5) { fprintf(stderr, "bad record %lld\n", r); return 2; }
    start.p[r] = (int32_t)s; revcom.p[r] = (uint8_t)rc; use.p[r] = (uint8_t)u; mate.p[r] = m; col_off.p[r + 1] = e;
    all_used = all_used && u;
  }
  if (!ma_dmg_mate_ok(mate.p, n)) { fprintf(stderr, "bad mate\n"); return 2; }
  const uint8_t* use_arg = all_used ? nullptr : use.p;      // (as the library is called: NULL where every record counts)
  const MaProfView v(n, T, (int32_t)L, start.p, revcom.p, col_off.p, seq.p, smp.p, ref.p, use_arg);
  int n_tables = 0, n_thresholds = 0;
  if (fscanf(f, "%d %d", &n_tables, &n_thresholds) != 2) { fprintf(stderr, "bad table count\n"); return 2; }
  for (int t = 0; t < n_tables; t++) {
    for (int b = 0; b < MA_PMD_WEIGHTS; b++) {
      long long x;
      if (fscanf(f, "%lld", &x) != 1) { fprintf(stderr, "bad table %d\n", t); return 2; }
      w.p[b] = (int32_t)x;
    }
    if (!ma_pmd_weights_ok(w.p)) { fprintf(stderr, "a weight out of range\n"); return 2; }
    // the column stage: stretch by stretch, in an order of its own (last stretch first: a sum does not care)
    for (long long r = 0; r < n; r++) rec.p[r] = 0;
    long long calls = 0;
    for (long long base = (long long)padded - MA_PMD_LANE; base >= 0; base -= MA_PMD_LANE)
      ma_pmd_stretch(v, w.p, base, [&](int64_t r, int32_t sum) {
        calls++;
        if (r < 0 || r >= n || !sum || sum > MA_PMD_LANE * MA_PMD_MAX_WEIGHT || sum < -MA_PMD_LANE * MA_PMD_MAX_WEIGHT) { fprintf(stderr, "a call out of range\n"); exit(1); }
        rec.p[r] += sum;
      });
    if (calls > (long long)(padded / MA_PMD_LANE) + n) { fprintf(stderr, "more calls than a stretch per record allows\n"); return 1; }
    // record by record
    printf("rec");
    for (long long r = 0; r < n; r++) {
      int64_t s = 0;
      if (!use_arg || use_arg[r])
        for (int64_t x = col_off.p[r]; x < col_off.p[r + 1]; x++) {
          const int64_t p = (int64_t)start.p[r] + (x - col_off.p[r]);
          s += ma_pmd_weight(w.p, p >= L, p >= L ? '\0' : ref.p[p], seq.p[x], smp.p[x], revcom.p[r] != 0);
        }
      if (s != rec.p[r]) { fprintf(stderr, "record %lld (table %d): stretches %lld, columns %lld\n", r, t, (long long)rec.p[r], (long long)s); return 1; }
      printf(" %lld", (long long)s);
    }
    printf("\n");
    // the molecule stage
    for (int k = 0; k < n_thresholds; k++) {
      long long threshold;
      if (fscanf(f, "%lld", &threshold) != 1) { fprintf(stderr, "bad threshold\n"); return 2; }
      std::vector<int64_t> bins(MA_PMD_BINS, 0);
      for (long long r = 0; r < n; r++) { keep.p[r] = 255; mol.p[r] = INT64_MIN; }
      const MaPmdMolView mv{n, revcom.p, use_arg, mate.p, rec.p, threshold, mol.p, keep.p};
      for (long long r = n - 1; r >= 0; r--) ma_pmd_record(mv, r, [&](int bin) {
        if (bin < 0 || bin >= MA_PMD_BINS) { fprintf(stderr, "a bin out of range\n"); exit(1); }
        bins[(size_t)bin]++;
      });
      int64_t molecules = 0;
      for (int b = 0; b < MA_PMD_HIST; b++) molecules += bins[(size_t)b];
      printf("%lld %lld %lld %lld\n", threshold, (long long)molecules, (long long)bins[MA_PMD_KEPT], (long long)bins[MA_PMD_ORPHANS]);
      std::string ks;
      for (long long r = 0; r < n; r++) {
        if (keep.p[r] > 1 || mol.p[r] == INT64_MIN) { fprintf(stderr, "record %lld: keep or the molecule's score was not written\n", r); return 1; }
        ks += (char)('0' + keep.p[r]);
      }
      printf("%s\nmol", ks.empty() ? "-" : ks.c_str());
      for (long long r = 0; r < n; r++) printf(" %lld", (long long)mol.p[r]);
      printf("\nhist");
      for (int b = 0; b < MA_PMD_HIST; b++) if (bins[(size_t)b]) printf(" %d %lld", b, (long long)bins[(size_t)b]);
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
