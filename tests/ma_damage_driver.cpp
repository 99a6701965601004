// Host caller of the shared code of the deaminated-fragment filter (csrc/ma_damage_body.h: what the kernels of
// mia_ma_damage_kernels.h run per lane): ma_dmg_stretch over every stretch of 16 flat positions, into hit5 / hit3 by maximum as the
// device's atomics do, then ma_dmg_record over every record, for both libraries, N in 1, 2, 3, 15 and the four ends modes.  Every array
// ends where the device's may end -- SEQ and SMP on the next multiple of 16 behind their last character, everything else on its last
// element -- and is heap memory of its own, so that AddressSanitizer sees every index.  Beside it a loop record by record and column
// by column that shares ma_dmg_hit and ma_prof_bin alone; the two must agree.  The results are printed for the test to compare with
// its own restatement (tests/ma_damage_ref.py), which shares nothing.
//
//   ma_damage_driver <file>     file: "L n T", the reference, ">" + SEQ, ">" + SMP (flat), then n lines "start rc use mate col_off_end"
//   output per library (ds, ss): "pos5 ..", "pos3 ..", then per N and mode "N mode molecules kept orphans", keep as a string of 0 / 1
//   ("-" without records) and the bins of hist that are not zero as "bin count" pairs
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_damage_body.h"
#include "ma_driver_util.h"

using namespace mia;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: ma_damage_driver <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  long long L = 0, n = 0, T = 0;
  if (fscanf(f, "%lld %lld %lld\n", &L, &n, &T) != 3) { fprintf(stderr, "bad header\n"); return 2; }
  const std::string ref_s = line_of(f), seq_s = line_of(f).substr(1), smp_s = line_of(f).substr(1);
  if ((long long)ref_s.size() != L || (long long)seq_s.size() != T || (long long)smp_s.size() != T) { fprintf(stderr, "bad strings\n"); return 2; }
  const size_t padded = (size_t)(T + MA_DMG_LANE - 1) / MA_DMG_LANE * MA_DMG_LANE;
  Exact<char> ref((size_t)L), seq(padded, 16), smp(padded, 16);
  Exact<int32_t> start((size_t)n);
  Exact<uint8_t> revcom((size_t)n), use((size_t)n), pos5((size_t)n), pos3((size_t)n), keep((size_t)n);
  Exact<int64_t> col_off((size_t)n + 1), mate((size_t)n);
  Exact<uint32_t> hit5((size_t)n), hit3((size_t)n);
  memcpy(ref.p, ref_s.data(), (size_t)L);
  if (T) { memcpy(seq.p, seq_s.data(), (size_t)T); memcpy(smp.p, smp_s.data(), (size_t)T); }
  bool all_used = true;
  for (long long r = 0; r < n; r++) {
    long long s, rc, u, m, e;
    if (fscanf(f, "%lld %lld %lld %lld %lld", &s, &rc, &u, &m, &e) != 5) { fprintf(stderr, "bad record %lld\n", r); return 2; }
    start.p[r] = (int32_t)s; revcom.p[r] = (uint8_t)rc; use.p[r] = (uint8_t)u; mate.p[r] = m; col_off.p[r + 1] = e;
    all_used = all_used && u;
  }
  fclose(f);
  if (!ma_dmg_mate_ok(mate.p, n)) { fprintf(stderr, "bad mate\n"); return 2; }
  const uint8_t* use_arg = all_used ? nullptr : use.p;      // (as the library is called: NULL where every record counts)
  const MaProfView v(n, T, (int32_t)L, start.p, revcom.p, col_off.p, seq.p, smp.p, ref.p, use_arg);
  for (int ss = 0; ss < 2; ss++) {
    // the hits stage: stretch by stretch, in an order of its own (last stretch first: the maximum does not care)
    for (long long r = 0; r < n; r++) hit5.p[r] = hit3.p[r] = 0;
    long long calls = 0;
    for (long long base = (long long)padded - MA_DMG_LANE; base >= 0; base -= MA_DMG_LANE)
      ma_dmg_stretch(v, ss != 0, base, [&](int64_t r, uint32_t h5, uint32_t h3) {
        calls++;
        if (r < 0 || r >= n || (!h5 && !h3) || h5 >= (uint32_t)MA_DMG_CLASSES || h3 >= (uint32_t)MA_DMG_CLASSES) { fprintf(stderr, "a call out of range\n"); exit(1); }
        if (h5 > hit5.p[r]) hit5.p[r] = h5;
        if (h3 > hit3.p[r]) hit3.p[r] = h3;
      });
    if (calls > 2 * (long long)(padded / MA_DMG_LANE) + n) { fprintf(stderr, "more calls than a stretch per record allows\n"); return 1; }
    // record by record
    for (long long r = 0; r < n; r++) {
      int k5 = 0, k3 = 0;
      if (!use_arg || use_arg[r])
        for (int64_t x = col_off.p[r]; x < col_off.p[r + 1]; x++) {
          const int64_t p = (int64_t)start.p[r] + (x - col_off.p[r]);
          const int hit = ma_dmg_hit(ma_prof_bin(p >= L, p >= L ? '\0' : ref.p[p], seq.p[x], smp.p[x], revcom.p[r] != 0), ss != 0);
          if (hit > 0 && (!k5 || hit < k5)) k5 = hit;
          if (hit < 0 && (!k3 || -hit < k3)) k3 = -hit;
        }
      const int s5 = hit5.p[r] ? MA_DMG_CLASSES - (int)hit5.p[r] : 0, s3 = hit3.p[r] ? MA_DMG_CLASSES - (int)hit3.p[r] : 0;
      if (s5 != k5 || s3 != k3) { fprintf(stderr, "record %lld (library %d): stretches %d %d, columns %d %d\n", r, ss, s5, s3, k5, k3); return 1; }
    }
    // the molecule stage
    static const int grid_n[4] = {1, 2, 3, 15};
    for (int gi = 0; gi < 4; gi++)
      for (int mode = 0; mode < 4; mode++) {
        std::vector<int64_t> bins(MA_DMG_BINS, 0);
        for (long long r = 0; r < n; r++) pos5.p[r] = pos3.p[r] = keep.p[r] = 255;
        const MaDmgMolView mv{n, revcom.p, use_arg, mate.p, hit5.p, hit3.p, grid_n[gi], mode, pos5.p, pos3.p, keep.p};
        for (long long r = n - 1; r >= 0; r--) ma_dmg_record(mv, r, [&](int bin) {
          if (bin < 0 || bin >= MA_DMG_BINS) { fprintf(stderr, "a bin out of range\n"); exit(1); }
          bins[(size_t)bin]++;
        });
        if (gi == 0 && mode == 0) {
          printf("pos5"); for (long long r = 0; r < n; r++) printf(" %d", pos5.p[r]);
          printf("\npos3"); for (long long r = 0; r < n; r++) printf(" %d", pos3.p[r]);
          printf("\n");
        }
        int64_t molecules = 0;
        for (int b = 0; b < MA_DMG_HIST; b++) molecules += bins[(size_t)b];
        printf("%d %d %lld %lld %lld\n", grid_n[gi], mode, (long long)molecules, (long long)bins[MA_DMG_KEPT], (long long)bins[MA_DMG_ORPHANS]);
        std::string ks;
        for (long long r = 0; r < n; r++) {
          if (keep.p[r] > 1) { fprintf(stderr, "record %lld: keep was not written\n", r); return 1; }
          ks += (char)('0' + keep.p[r]);
        }
        printf("%s\nhist", ks.empty() ? "-" : ks.c_str());
        for (int b = 0; b < MA_DMG_HIST; b++) if (bins[(size_t)b]) printf(" %d %lld", b, (long long)bins[(size_t)b]);
        printf("\n");
      }
  }
  return 0;
}
