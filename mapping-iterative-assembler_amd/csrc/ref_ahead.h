// ref_ahead.h -- "reference ahead": may the tables that were prepared behind the last consensus stand in for the ones this call
// would make?  Plain C++17, no HIP: the two functions read their arguments and nothing else, so a CPU test
// (tests/test_ref_ahead_cpu.py) enumerates them.  mia_hip_iterate launches k_ref_prep for the string it has just returned (the
// shadow launch: second set of buffers, the idle half of the control block) and asks here, at the top of the next call, whether that
// work is the work the call wants.
#pragma once
#include <stdint.h>
#include <string.h>

namespace mia {

// Everything k_ref_prep's arguments are derived from, besides the characters themselves.  The shadow launch fills one from the string
// it was given; the next call fills one from its own arguments, by the same functions.
struct RefAheadKey {
  int32_t L = 0;                  // characters of the reference
  int32_t circular = 0;           // the wrap's length depends on it
  int64_t n_other = 0;            // characters that are no base
  int64_t kh_entries = 0;         // entries the N columns' spellings add to the 10-mer table
  uint32_t kslots = 0;            // slots of that table
  int32_t kwild = 0;              // N columns per 10-mer it spells out
  int64_t plane_words = 0, nib_words = 0;
  bool bits = false;              // the quick plan's bitmaps were made / are wanted
};

inline bool ref_ahead_same_key(const RefAheadKey& a, const RefAheadKey& b) {
  return a.L == b.L && a.circular == b.circular && a.n_other == b.n_other && a.kh_entries == b.kh_entries && a.kslots == b.kslots &&
         a.kwild == b.kwild && a.plane_words == b.plane_words && a.nib_words == b.nib_words && a.bits == b.bits;
}

// the string kept from the last return (built.L characters) is the one the new call brings: what was counted on it -- n_other,
// kh_entries -- holds for the new call as well and is not counted again
inline bool ref_ahead_same_string(const RefAheadKey& built, const char* kept, const char* new_ref, int32_t new_len, int32_t circular) {
  return kept && new_ref && new_len > 0 && new_len == built.L && (circular != 0) == (built.circular != 0) && memcmp(new_ref, kept, (size_t)new_len) == 0;
}

// HIT: same key, same string -- it compares the characters itself, whatever the caller has found out before (it asks
// ref_ahead_same_string once more to know whether the counts kept with the shadow launch may fill `want`: 16 KB, well under a
// microsecond).  Anything else is a miss and the call prepares its reference itself.
inline bool ref_ahead_hit(const RefAheadKey& built, const RefAheadKey& want, const char* kept, const char* new_ref) {
  return ref_ahead_same_key(built, want) && ref_ahead_same_string(built, kept, new_ref, want.L, want.circular);
}

}  // namespace mia
