// ma_cols_body.h -- the strand-split column table of a .maln (ma_hip -f 42) as functions of one record and one tile of reference
// columns.  The rule is DESIGN.md's "Strand table (-f 42)": sixteen words per reference column p in 0 .. L-1,
//     0 .. 5    A C G T gap other of the columns of forward records         6 .. 11   the same of records stored reverse-complemented
//     12, 13    forward / reverse records that START on p, unless SEG is 'b'
//     14, 15    forward / reverse records that END on p, unless SEG is 'f'      (starts_f, starts_r, ends_f, ends_r of col_print_cons,
//                                                                                src/map_align.c:789-825)
// A record that counts, with s = START, n columns and e = s + n - 1, adds one to word (rc ? 6 : 0) + class(seq[c]) of column s + c
// for c = 0 .. n-1 -- the class of the exact character: 'A' 'C' 'G' 'T' -> 0 .. 3, '-' -> 4, anything else 5 -- and one to `beyond`
// instead when s + c >= L.  Its START is an event on column s and its END one on column e (a record without columns: e = s - 1); an
// anchor outside 0 .. L-1 adds one to `ends_outside` instead.
//
// Plain C++ behind MIA_HD.  The reference columns are cut into tiles of MA_COLS_TILE; a tile's sixteen words per column are what a
// workgroup of k_ma_cols (mia_ma_cols_kernels.h) holds in LDS.  ma_cols_touches says whether a record has anything to add to a tile,
// ma_cols_part which of its columns lie in it, ma_cols_walk hands the tile those columns (lanes over adjacent words of four columns),
// ma_cols_ends the record's anchors that lie in it, and ma_cols_outside counts what lies on no reference column; tile 0 takes those.
// A host caller (tests/ma_cols_driver.cpp) runs the same code record by record and tile by tile.
#pragma once
#include <stdint.h>

#include "ma_records.h"

namespace mia {

constexpr int MA_COLS_TILE = 512;          // reference columns of one tile: 16 words x 512 x 4 bytes = 32 KiB of LDS
constexpr int MA_COLS_WORDS = 16, MA_COLS_CLASSES = 6, MA_COLS_STARTS = 12, MA_COLS_ENDS = 14;

// The records (ma_records.h: seq is loaded in aligned words of four characters), the segments and the selection.
struct MaColsView : MaRecords {
  const uint8_t* segment;    // [n]: the SEG character; NULL = every record is whole
  const uint8_t* use;        // [n]: 0 = the record is left out; NULL = every record counts
  MaColsView(const MaRecords& recs, const uint8_t* segment, const uint8_t* use) : MaRecords(recs), segment(segment), use(use) {}
  // ... or from the arrays this export reads alone, for a caller that holds no more (the host drivers): the rest of MaRecords is null
  MaColsView(int64_t n, int32_t L, const int32_t* start, const uint8_t* revcom, const int64_t* col_off, const char* seq, const uint8_t* segment,
             const uint8_t* use)
      : MaRecords{n, L, start, revcom, col_off, seq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, segment(segment), use(use) {}
};

MIA_HD inline int ma_cols_class(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == '-' ? 4 : 5; }
MIA_HD inline int64_t ma_cols_tiles(int32_t L) { return ((int64_t)L + MA_COLS_TILE - 1) / MA_COLS_TILE; }
// the tile that holds reference column a, or -1 when a is no reference column
MIA_HD inline int64_t ma_cols_tile_of(int64_t a, int32_t L) { return a < 0 || a >= L ? -1 : a / MA_COLS_TILE; }

// The columns c of a record (s, n) that lie in `tile` and inside the reference: *c0 <= c < *c1; none when *c0 >= *c1.
MIA_HD inline void ma_cols_range(int64_t s, int64_t n, int32_t L, int64_t tile, int64_t* c0, int64_t* c1) {
  const int64_t t0 = tile * MA_COLS_TILE, t1 = t0 + MA_COLS_TILE < L ? t0 + MA_COLS_TILE : (int64_t)L;
  *c0 = t0 > s ? t0 - s : 0;
  *c1 = t1 - s < n ? t1 - s : n;
}

// has a record of n columns at START s anything to add to `tile`: a column, or one of its two anchors (whether the anchor counts is
// ma_cols_ends' to say)
MIA_HD inline bool ma_cols_touches(int64_t s, int64_t n, int32_t L, int64_t tile) {
  int64_t c0, c1;
  ma_cols_range(s, n, L, tile, &c0, &c1);
  return c0 < c1 || ma_cols_tile_of(s, L) == tile || ma_cols_tile_of(s + n - 1, L) == tile;
}

MIA_HD inline bool ma_cols_counts(const MaColsView& v, int64_t r) { return !v.use || v.use[r] != 0; }

// The part of a record that lies in a tile, as a workgroup lists it: the flat position in seq of its first column there, how many
// columns, the column in the tile of the first, and the strand -- twelve bytes.
struct MaColsPart {
  int64_t at;
  int32_t meta;              // len | col << 12 | rc << 24
};
static_assert(MA_COLS_TILE <= 2048, "MaColsPart packs a length and a column of up to 2048");
MIA_HD inline int ma_cols_part_len(int32_t meta) { return meta & 0xfff; }
MIA_HD inline int ma_cols_part_col(int32_t meta) { return (meta >> 12) & 0xfff; }
MIA_HD inline int ma_cols_part_strand(int32_t meta) { return (meta >> 24) & 1 ? MA_COLS_CLASSES : 0; }

// the part of record r in `tile`; false when it has no column there
MIA_HD inline bool ma_cols_part(const MaColsView& v, int64_t r, int64_t tile, MaColsPart* part) {
  const int64_t off = v.col_off[r], s = v.start[r];
  int64_t c0, c1;
  ma_cols_range(s, v.col_off[r + 1] - off, v.L, tile, &c0, &c1);
  if (c0 >= c1) return false;
  part->at = off + c0;
  part->meta = (int32_t)(c1 - c0) | (int32_t)(s + c0 - tile * MA_COLS_TILE) << 12 | (v.revcom[r] != 0 ? 1 : 0) << 24;
  return true;
}

// The columns of a part for lane `lane` of `lanes`: seq in aligned words of four characters, adjacent lanes on adjacent words, the
// characters of the first and the last word that are not the part's left out; add(word of the table, column in the tile) once per
// column.  seq is 4-byte aligned and readable up to the next multiple of four behind the part (mia_hip_ma_tally pads it).
template <class Add>
MIA_HD inline void ma_cols_walk(const char* seq, const MaColsPart& part, int lane, int lanes, Add&& add) {
  const int64_t at = part.at, end = at + ma_cols_part_len(part.meta);
  const int strand = ma_cols_part_strand(part.meta), col = ma_cols_part_col(part.meta);
  for (int64_t w = (at & ~(int64_t)3) + 4 * (int64_t)lane; w < end; w += 4 * (int64_t)lanes) {
    uint32_t x;
    __builtin_memcpy(&x, __builtin_assume_aligned(seq + w, 4), sizeof x);
    for (int q = 0; q < 4; q++, x >>= 8) {
      const int64_t pos = w + q;
      if (pos >= at && pos < end) add(strand + ma_cols_class((char)(x & 0xffu)), col + (int)(pos - at));
    }
  }
}

// The START and the END of record r, if they are events and lie in `tile`: add(word, column in the tile).
template <class Add>
MIA_HD inline void ma_cols_ends(const MaColsView& v, int64_t r, int64_t tile, Add&& add) {
  const int64_t s = v.start[r], e = s + (v.col_off[r + 1] - v.col_off[r]) - 1;
  const int rc = v.revcom[r] != 0 ? 1 : 0;
  const char seg = v.segment ? (char)v.segment[r] : 'n';
  if (seg != 'b' && ma_cols_tile_of(s, v.L) == tile) add(MA_COLS_STARTS + rc, (int)(s - tile * MA_COLS_TILE));
  if (seg != 'f' && ma_cols_tile_of(e, v.L) == tile) add(MA_COLS_ENDS + rc, (int)(e - tile * MA_COLS_TILE));
}

// What record r has on no reference column: its columns at or behind L, and its anchors outside 0 .. L-1.
MIA_HD inline void ma_cols_outside(const MaColsView& v, int64_t r, int64_t* beyond, int64_t* ends_outside) {
  const int64_t n = v.col_off[r + 1] - v.col_off[r], s = v.start[r], e = s + n - 1;
  const char seg = v.segment ? (char)v.segment[r] : 'n';
  const int64_t past = s + n - v.L;                          // columns s + c >= L
  if (past > 0) *beyond += past < n ? past : n;
  if (seg != 'b' && ma_cols_tile_of(s, v.L) < 0) *ends_outside += 1;
  if (seg != 'f' && ma_cols_tile_of(e, v.L) < 0) *ends_outside += 1;
}

}  // namespace mia
