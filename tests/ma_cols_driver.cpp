// Host caller of the shared code of the strand-split column table (csrc/ma_cols_body.h: what k_ma_cols runs on the device).
//   ma_cols_driver <file.maln> [A] [back]   reads a .maln as ma_hip does and, tile by tile as a workgroup does, runs ma_cols_touches,
//                                           ma_cols_ends, ma_cols_part and ma_cols_walk (as 64 lanes, one after the other) over every record
//                                           (`back`: from the last to the first), and ma_cols_outside for tile 0, into a tile of 16 x
//                                           MA_COLS_TILE words that is added to the table as the kernel's flush does.  Every array has
//                                           the exact size the device's has -- SEQ 16-byte aligned and 16 bytes longer than its
//                                           characters, as mia_hip_ma_tally makes it -- so a read past an end is seen.  Prints the records that
//                                           count, n_events, beyond, ends_outside and the 16 x L words, one number per line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../mapping-iterative-assembler_amd/csrc/ma_cols_body.h"
#include "../mapping-iterative-assembler_amd/host/maln_text.h"

int main(int argc, char** argv) {
  using namespace mia;
  if (argc < 2) { fprintf(stderr, "usage: ma_cols_driver <file.maln> [A] [back]\n"); return 2; }
  bool use_dropped = false, back = false;
  for (int k = 2; k < argc; k++) { use_dropped = use_dropped || !strcmp(argv[k], "A"); back = back || !strcmp(argv[k], "back"); }
  maln_text::MalnFile m;
  maln_text::read_maln_file(argv[1], &m);
  const int64_t n = (int64_t)m.start.size(), chars = m.col_off[(size_t)n];
  const int32_t L = m.L;
  std::vector<int32_t> start(m.start.begin(), m.start.end());
  std::vector<uint8_t> revcom(m.revcom.begin(), m.revcom.end()), use((size_t)n), seg((size_t)n);
  std::vector<int64_t> col_off(m.col_off.begin(), m.col_off.end());
  char* seq = nullptr;                                       // (what lies behind the characters must not be counted: 'A' would show)
  if (posix_memalign((void**)&seq, 16, (size_t)chars + 16)) { fprintf(stderr, "no memory\n"); return 2; }
  memset(seq, 'A', (size_t)chars + 16);
  memcpy(seq, m.seq.data(), (size_t)chars);
  int64_t n_used = 0;
  for (int64_t r = 0; r < n; r++) {
    use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
    seg[(size_t)r] = (uint8_t)m.rec[(size_t)r].segment;
    n_used += use[(size_t)r];
  }
  const MaColsView v{n, L, start.data(), revcom.data(), col_off.data(), seq, seg.data(), use.data()};
  std::vector<int64_t> table((size_t)MA_COLS_WORDS * (size_t)L, 0);
  int64_t beyond = 0, outside = 0;
  for (int64_t tile = 0; tile < ma_cols_tiles(L); tile++) {
    std::vector<uint32_t> lds((size_t)MA_COLS_WORDS * MA_COLS_TILE, 0);
    auto add = [&](int word, int col) {
      if (word < 0 || word >= MA_COLS_WORDS || col < 0 || col >= MA_COLS_TILE || tile * MA_COLS_TILE + col >= L) {
        fprintf(stderr, "tile %lld: word %d, column %d\n", (long long)tile, word, col);
        exit(3);
      }
      lds[(size_t)word * MA_COLS_TILE + (size_t)col]++;
    };
    for (int64_t i = 0; i < n; i++) {
      const int64_t r = back ? n - 1 - i : i;
      if (!ma_cols_counts(v, r)) continue;
      if (tile == 0) ma_cols_outside(v, r, &beyond, &outside);
      if (!ma_cols_touches(start[(size_t)r], col_off[(size_t)r + 1] - col_off[(size_t)r], L, tile)) {
        // a record that does not touch the tile must have nothing to add to it
        MaColsPart none;
        if (ma_cols_part(v, r, tile, &none)) { fprintf(stderr, "record %lld has a column in tile %lld\n", (long long)r, (long long)tile); exit(3); }
        ma_cols_ends(v, r, tile, [&](int, int) { fprintf(stderr, "record %lld has an anchor in tile %lld\n", (long long)r, (long long)tile); exit(3); });
        continue;
      }
      ma_cols_ends(v, r, tile, add);
      MaColsPart part;
      if (!ma_cols_part(v, r, tile, &part)) continue;
      for (int lane = 0; lane < 64; lane++) ma_cols_walk(seq, part, lane, 64, add);
    }
    for (int w = 0; w < MA_COLS_WORDS; w++)
      for (int c = 0; c < MA_COLS_TILE; c++) {
        const int64_t p = tile * MA_COLS_TILE + c;
        if (lds[(size_t)w * MA_COLS_TILE + (size_t)c] && p < L) table[(size_t)w * (size_t)L + (size_t)p] += lds[(size_t)w * MA_COLS_TILE + (size_t)c];
      }
  }
  int64_t events = beyond;
  for (int64_t i = 0; i < (int64_t)MA_COLS_STARTS * L; i++) events += table[(size_t)i];
  printf("%lld\n%lld\n%lld\n%lld\n", (long long)n_used, (long long)events, (long long)beyond, (long long)outside);
  for (int64_t x : table) printf("%lld\n", (long long)x);
  free(seq);
  return 0;
}
