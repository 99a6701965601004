// ma_molecule_body.h -- the molecules of a .maln: how the two halves of a read that was split at the origin of a circular reference
// are paired (mate), and the join of the halves that the deaminated-fragment filter and the damage score share.
//
// mate[r] is MA_MOL_NONE (the record is a molecule of its own), MA_MOL_ORPHAN (a half without its other half) or the record number
// of its other half, whose mate is r; a NULL mate means MA_MOL_NONE for every record.  The duplicate filter reads the same encoding.
// The lower-numbered record of a molecule decides for it: it combines the halves' values, stores the outcome to both records (plain
// stores: no other caller writes them) and counts the molecule once -- in its class, where either half is selected; among the
// orphans; and every record of it among the records kept.
//
// Plain C++ behind MIA_HD.
#pragma once
#include <stdint.h>

#include "ma_records.h"                    // MIA_HD

namespace mia {

constexpr int64_t MA_MOL_NONE = -1, MA_MOL_ORPHAN = -2;

// mate[r]: MA_MOL_NONE, MA_MOL_ORPHAN, or another record whose mate is r
MIA_HD inline bool ma_mate_record_ok(const int64_t* mate, int64_t n, int64_t r) {
  const int64_t m = mate ? mate[r] : MA_MOL_NONE;
  return m == MA_MOL_NONE || m == MA_MOL_ORPHAN || (m >= 0 && m < n && m != r && mate[m] == r);
}
// ... for every r (host: the entry points' check)
inline bool ma_mate_ok(const int64_t* mate, int64_t n) {
  if (!mate) return true;
  for (int64_t r = 0; r < n; r++)
    if (!ma_mate_record_ok(mate, n, r)) return false;
  return true;
}

// Record r, where it is the lowest-numbered record of its molecule.  decide(m, &bin) does what differs between the callers: m >= 0 is
// the other half (else r is alone); it combines the halves' values, stores the per-record outputs to r (and m), names the molecule's
// class bin and returns keep.  count(bin) is then called for every bin the molecule adds to.
template <class Decide, class Count>
MIA_HD inline void ma_molecule_join(const int64_t* mate, const uint8_t* use, int64_t r, int orphans_bin, int kept_bin, Decide&& decide, Count&& count) {
  const int64_t m = mate ? mate[r] : MA_MOL_NONE;
  if (m >= 0 && m < r) return;             // the other half decides
  bool counts = !use || use[r] != 0;
  if (m >= 0) counts = counts || !use || use[m] != 0;
  int bin = 0;
  const bool k = decide(m, &bin);
  if (counts) {
    count(bin);
    if (m == MA_MOL_ORPHAN) count(orphans_bin);
  }
  if (k) { count(kept_bin); if (m >= 0) count(kept_bin); }
}

}  // namespace mia
