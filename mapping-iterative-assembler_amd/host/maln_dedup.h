// maln_dedup.h -- what ma_hip -u and -D do on the host around mia_hip_ma_dedup and mia_hip_ma_damage ("Duplicate filter",
// "Deaminated fragments"): the pairing of the halves of reads split at the origin (IDs are strings), and the removal of the records
// that are not kept -- with their INS_POS pairs, and
// with GAPS recomputed the way cull_maln_from_fsdb does (src/mia.c:484-504).  Records are handed to the filter in FILE order
// (MalnRecord::file_no), because the rule's tie-break is the file index; read_maln_file has sorted them by then.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "maln_text.h"

namespace maln_text {

struct DedupInput {
  std::vector<size_t> at;                    // file number -> position in MalnFile::rec
  std::vector<int32_t> start, end, score;
  std::vector<uint8_t> revcom;
  std::vector<int64_t> mate;                 // -1 whole, -2 an orphan half, else the file number of the other half
};

// A record with SEG 'f' and an ID that ends in "_f" and a record with SEG 'b' and an ID that ends in "_b" are one molecule when the
// IDs are equal up to that last letter, the strands are equal, and that stem occurs once among the 'f' and once among the 'b' records
// of that strand.  Every other 'f' or 'b' record is an orphan.  The pairing works on POSITIONS in MalnFile::rec, so that it holds for
// a file some records of which are gone already: item i is the record rec[at[i]], and mate[i] is -1 (whole), -2 (an orphan half) or
// the item of the other half.  pairs (may be NULL): the (front item, back item) of every pair, ordered by strand and stem.
inline void pair_halves(const MalnFile& m, const std::vector<size_t>& at, std::vector<int64_t>* mate, std::vector<std::pair<int64_t, int64_t>>* pairs) {
  const size_t n = at.size();
  mate->assign(n, -1);
  std::map<std::pair<int, std::string>, std::pair<std::vector<int64_t>, std::vector<int64_t>>> stems;
  for (size_t i = 0; i < n; i++) {
    const MalnRecord& a = m.rec[at[i]];
    if (a.segment != 'f' && a.segment != 'b') continue;
    (*mate)[i] = -2;
    const size_t len = a.id.size();
    if (len < 2 || a.id[len - 2] != '_' || a.id[len - 1] != a.segment) continue;
    auto& lists = stems[{a.rc ? 1 : 0, a.id.substr(0, len - 1)}];
    (a.segment == 'f' ? lists.first : lists.second).push_back((int64_t)i);
  }
  for (const auto& s : stems) {
    if (s.second.first.size() != 1 || s.second.second.size() != 1) continue;
    const int64_t f = s.second.first[0], b = s.second.second[0];
    (*mate)[(size_t)f] = b;
    (*mate)[(size_t)b] = f;
    if (pairs) pairs->push_back({f, b});
  }
}

// ... with item i = position i: the record numbers of a mia_hip_ma_tally of the file as it stands
inline void pair_halves(const MalnFile& m, std::vector<int64_t>* mate) {
  std::vector<size_t> at(m.rec.size());
  for (size_t k = 0; k < at.size(); k++) at[k] = k;
  pair_halves(m, at, mate, nullptr);
}

// The duplicate filter's input, in FILE order (item = file number).  Returns false (and names the read in *why) if the front half of
// a pair does not start behind its back half: such halves do not lie across the origin of a circular reference.
inline bool dedup_input(const MalnFile& m, DedupInput* in, std::string* why) {
  const size_t n = m.rec.size();
  in->at.assign(n, 0);
  for (size_t k = 0; k < n; k++) {
    const int f = m.rec[k].file_no;
    if (f < 0 || (size_t)f >= n) { *why = "record numbers are inconsistent"; return false; }
    in->at[(size_t)f] = k;
  }
  in->start.resize(n); in->end.resize(n); in->score.resize(n); in->revcom.resize(n);
  for (size_t f = 0; f < n; f++) {
    const MalnRecord& a = m.rec[in->at[f]];
    in->start[f] = a.start; in->end[f] = a.end; in->score[f] = a.score; in->revcom[f] = a.rc ? 1 : 0;
  }
  std::vector<std::pair<int64_t, int64_t>> pairs;
  pair_halves(m, in->at, &in->mate, &pairs);
  for (const auto& p : pairs)
    if (in->start[(size_t)p.first] <= in->start[(size_t)p.second]) {
      const std::string& id = m.rec[in->at[(size_t)p.first]].id;
      *why = "the halves of " + id.substr(0, id.size() - 1) + " do not lie across the origin";
      return false;
    }
  return true;
}

// Removes every record r (position in MalnFile::rec) with keep[r] == 0, then resets GAPS: only columns i with GAPS[i] > 0 change, to
// the longest insert a remaining record with START < i <= END carries at i - START (of several pairs of one position the last given
// counts), 0 if there is none.  NUM_INPUTS and everything else of the remaining records stay as they are.
inline void remove_records(MalnFile* m, const std::vector<uint8_t>& keep) {
  std::vector<MalnRecord> left;
  for (size_t k = 0; k < m->rec.size(); k++) if (keep[k]) left.push_back(std::move(m->rec[k]));
  m->rec.swap(left);
  std::vector<int32_t> longest((size_t)m->L, 0);
  for (const MalnRecord& a : m->rec) {
    std::map<int32_t, size_t> last;
    for (size_t k = 0; k < a.ins_pos.size(); k++) last[a.ins_pos[k]] = k;
    for (const auto& e : last) {
      const long i = (long)a.start + e.first;
      if (e.first <= 0 || i > a.end || i >= m->L) continue;
      const int32_t len = (int32_t)a.ins_seq[e.second].size();
      if (len > longest[(size_t)i]) longest[(size_t)i] = len;
    }
  }
  for (int i = 0; i < m->L; i++) if (m->gaps[(size_t)i] > 0) m->gaps[(size_t)i] = longest[(size_t)i];
  flatten_records(m);
}

}  // namespace maln_text
