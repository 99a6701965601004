// cull_body.h -- the cull's arithmetic that needs no GPU: records per read, the links a read will emit, and a block's first
// AlnSeq slot from k_slot_count's raw counts.  Plain C++ (tests/test_cull_body_cpu.py compiles it with g++); the kernels of
// mia_consensus_kernels.h use these very functions.
#pragma once
#include <stdint.h>

#ifndef MIA_HD
#if defined(__HIPCC__)
#define MIA_HD __host__ __device__
#else
#define MIA_HD
#endif
#endif

namespace mia {

// how a read's alignment maps onto AlnSeq records (src/mia_main.c:259-276, src/mia.c:1376-1438)
struct RecGeom {
  int start_w, end, split, ncols_f, ncols_b;
};
MIA_HD inline RecGeom rec_geom(int as, int ae, int L) {
  RecGeom g;
  g.start_w = as;
  g.end = ae > L ? ae - L : ae;
  g.split = as > g.end;
  g.ncols_f = g.split ? (L - as) : (g.end - as + 1);
  g.ncols_b = g.split ? g.end + 1 : 0;
  return g;
}

// AlnSeq records of a read: none while its strand is unknown, two when it is split at the origin
MIA_HD inline int cull_records(bool sk, int as, int ae, int L) { return sk ? (rec_geom(as, ae, L).split ? 2 : 1) : 0; }

// links the cull will emit for a read (kinds: see struct Links).  A strand-unknown read follows both pass-1 pointers; a
// strand-known read follows its back pointer only while it is NOT split (a split read overwrites the pointer instead).
// Everything this looks at exists before k_cull_records runs, and that kernel changes back_slot of split reads only: a
// count taken beforehand is exact.
// The kernels do not look at the two 8-byte pointers for this but at one mark byte per read, kept wherever a pointer is written
// (upload, mia_hip_set_back_slots, mia_hip_set_pass1_state, the cull's split reads): bit 0 = has a back pointer, bit 1 = has a pass-1
// front pointer.
MIA_HD inline int cull_link_mark(int64_t back_slot, int64_t front_slot0) { return (back_slot >= 0 ? 1 : 0) | (front_slot0 >= 0 ? 2 : 0); }
MIA_HD inline int cull_links_marked(bool sk, bool split, int mark) {
  if (!sk) return (mark & 1) + ((mark >> 1) & 1);
  return (!split && (mark & 1)) ? 1 : 0;
}
MIA_HD inline int cull_links(bool sk, bool split, int64_t back_slot, int64_t front_slot0) {
  return cull_links_marked(sk, split, cull_link_mark(back_slot, front_slot0));
}

// k_slot_count's raw counts, nb = blocks of 256 reads:
//   partial[0 .. nb)            records of block b
//   partial[nb .. nb + ng)      records of group g = sixteen blocks (ng = cull_groups(nb))
//   partial[nb + ng .. nb+2ng)  links of group g
MIA_HD inline int cull_groups(int nb) { return (nb + 15) >> 4; }
MIA_HD inline int64_t cull_partial_words(int64_t n) { const int64_t nb = (n + 255) / 256; return nb + 2 * ((nb + 15) / 16) + 8; }

// Thread t of `threads` takes its share of the three sums a block needs: the records before block `block` (its first slot
// is slot_base + that), the records of all blocks, the links of all blocks.  The shares of t = 0 .. threads - 1 add up to
// the sums; threads >= 16.
struct CullShare {
  int64_t pre, tot, links;
};
MIA_HD inline CullShare cull_share(const int64_t* partial, int nb, int block, int t, int threads) {
  const int ng = cull_groups(nb), myg = block >> 4;
  CullShare s = {0, 0, 0};
  // (the blocks of the own group first: on the GPU this load is then in flight together with the loop's)
  if (t < 16) {
    const int b = myg * 16 + t;
    if (b < block) s.pre = partial[b];
  }
  for (int g = t; g < ng; g += threads) {
    const int64_t v = partial[nb + g];
    s.tot += v;
    if (g < myg) s.pre += v;
    s.links += partial[nb + ng + g];
  }
  return s;
}

}  // namespace mia
