// maln_text.h -- reading the text of a .maln file the way the reference's read_ma does (src/map_alignment.c:384-607:
// fgets with MAX_LINE_LEN, sscanf "KEY %s" / "KEY %d", fscanf " %d %s" for the insert list), and writing it again the way
// write_ma does (:283-382; ma -m).  Shared by ma_hip and ccheck_hip; ccheck_hip keeps its own record layout, ma_hip's
// (MalnFile, read_maln_file, write_maln_file) is here so that a host-only caller can read and write a .maln the same way.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace maln_text {

constexpr int MAX_LINE_LEN = 1000000;   // src/params.h:22

struct Cursor {
  const char* p;
  const char* end;
  // fgets(line, MAX_LINE_LEN, f): at most MAX_LINE_LEN-1 characters, newline included
  bool line(std::string* out) {
    if (p >= end) { out->clear(); return false; }
    const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
    const char* stop = nl ? nl + 1 : end;
    if (stop - p > MAX_LINE_LEN - 1) stop = p + (MAX_LINE_LEN - 1);
    out->assign(p, stop);
    p = stop;
    return true;
  }
  void skip_ws() { while (p < end && isspace((unsigned char)*p)) p++; }
  bool literal(const char* lit) {   // fscanf(f, "LITERAL"): stops at the first mismatch
    for (; *lit; lit++) { if (p < end && *p == *lit) p++; else return false; }
    return true;
  }
  bool integer(long* v) {           // fscanf " %d"
    skip_ws();
    const char* q = p;
    if (q < end && (*q == '+' || *q == '-')) q++;
    if (q >= end || !isdigit((unsigned char)*q)) return false;
    char* e = nullptr;
    *v = strtol(p, &e, 10);
    p = e;
    return true;
  }
  bool token(std::string* t) {      // fscanf " %s"
    skip_ws();
    const char* q = p;
    while (q < end && !isspace((unsigned char)*q)) q++;
    if (q == p) return false;
    t->assign(p, q);
    p = q;
    return true;
  }
};

// sscanf(line, "KEY %s") / "KEY %d"
inline bool field(const std::string& line, const char* key, std::string* tok) {
  const size_t k = strlen(key);
  if (line.compare(0, k, key) != 0) return false;
  size_t i = k;
  while (i < line.size() && isspace((unsigned char)line[i])) i++;
  size_t j = i;
  while (j < line.size() && !isspace((unsigned char)line[j])) j++;
  if (j == i) return false;
  tok->assign(line, i, j - i);
  return true;
}
inline bool field_int(const std::string& line, const char* key, int* v) {
  std::string t;
  if (!field(line, key, &t)) return false;
  char* e = nullptr;
  long x = strtol(t.c_str(), &e, 10);
  if (e == t.c_str()) return false;
  *v = (int)x;
  return true;
}

inline void read_matrices(Cursor& c, int depth, int32_t sm[31][5][5]) {
  std::string line;
  for (int i = 0; i <= depth * 2 && i < 31; i++) {
    for (int row = 0; row <= 4; row++) {
      c.line(&line);
      int v[5] = {0, 0, 0, 0, 0};
      sscanf(line.c_str(), "%d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4]);
      for (int k = 0; k < 5; k++) sm[i][row][k] = v[k];
    }
    c.line(&line);   // blank line between matrices
  }
}


inline bool slurp(const char* fn, std::string* buf) {
  FILE* f = fopen(fn, "r");
  if (!f) return false;
  char chunk[1 << 16];
  size_t n;
  while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf->append(chunk, n);
  fclose(f);
  return true;
}

// ---- a whole .maln as ma reads it (read_ma, src/map_alignment.c:384-607) -------------------------------------------------
constexpr int PSSM_DEPTH = 15;   // src/params.h:21
constexpr int INIT_NUM_ALN_SEQS = 16000;   // src/params.h:69

struct MalnRecord {
  std::string id, desc;                       // desc: the DESC line behind "DESC " (src/map_alignment.c:551-552)
  int start = 0, end = 0, rc = 0, trimmed = 0, num_inputs = 1, score = 0, dropped = 0;
  char segment = 'n';
  int file_no = 0;                            // the record's place in the file (read_maln_file sorts the records)
  std::string seq, smp;                       // columns start .. end
  std::string seq_raw, smp_raw;               // the SEQ and SMP strings as read: write_ma writes them whole, ace_output counts strlen(SEQ)
  std::vector<int32_t> ins_pos;               // INS_POS pairs, in file order
  std::vector<std::string> ins_seq;
};

// The records flattened the way mia_hip_ma_tally takes them, in the order of `rec`.
struct MalnFile {
  std::string ref_id, ref_seq, ref_desc;
  int L = 0;
  int maln_siz = 0, ref_size = 0, depth = 15; // maln->size as read_ma leaves it, ref->size, fpsm->depth
  std::vector<int32_t> gaps;
  int32_t fpsm[31][5][5], rpsm[31][5][5];
  std::vector<MalnRecord> rec;
  std::vector<int32_t> start, ins_record, ins_pos;
  std::vector<uint8_t> revcom;
  std::vector<int64_t> col_off, ins_off;
  std::string seq, smp, ins_bases;
};

inline void maln_bad(const char* what, const char* fn) { fprintf(stderr, what, fn); exit(1); }

// sort_aln_frags (src/map_alignment.c:630-633, alnSeqCmp src/map_align.c:393-414): by start, then end.  glibc's qsort is a merge
// sort at these sizes, so records that compare equal keep their order.
inline void sort_records(MalnFile* m) {
  std::stable_sort(m->rec.begin(), m->rec.end(), [](const MalnRecord& a, const MalnRecord& b) { return a.start != b.start ? a.start < b.start : a.end < b.end; });
}

inline void flatten_records(MalnFile* m) {
  m->start.clear(); m->revcom.clear(); m->seq.clear(); m->smp.clear(); m->ins_record.clear(); m->ins_pos.clear(); m->ins_bases.clear();
  m->col_off.assign(1, 0);
  m->ins_off.assign(1, 0);
  for (size_t r = 0; r < m->rec.size(); r++) {
    const MalnRecord& a = m->rec[r];
    m->start.push_back(a.start);
    m->revcom.push_back(a.rc ? 1 : 0);
    m->seq += a.seq;
    m->smp += a.smp;
    m->col_off.push_back((int64_t)m->seq.size());
    for (size_t k = 0; k < a.ins_pos.size(); k++) {
      m->ins_record.push_back((int32_t)r);
      m->ins_pos.push_back(a.ins_pos[k]);
      m->ins_bases += a.ins_seq[k];
      m->ins_off.push_back((int64_t)m->ins_bases.size());
    }
  }
}

inline void read_maln_file(const char* fn, MalnFile* m) {
  std::string buf;
  if (!slurp(fn, &buf)) { fprintf(stderr, "Cannot open %s\n", fn); exit(1); }
  Cursor c{buf.data(), buf.data() + buf.size()};
  std::string line, tok;
  c.line(&line);
  if (line.find("/* map_alignment") == std::string::npos) maln_bad("%s does not look like a map_alignment input file\n", fn);
  int nas = 0, tmp = 0;
  c.line(&line); field_int(line, "MALN_NAS", &nas);
  c.line(&line);                       // MALN_SIZ: the record array doubles from INIT_NUM_ALN_SEQS until it is that large (:415-419)
  m->maln_siz = INIT_NUM_ALN_SEQS;
  if (field_int(line, "MALN_SIZ", &tmp)) while (m->maln_siz < tmp && m->maln_siz <= (1 << 29)) m->maln_siz *= 2;
  c.line(&line);                       // MALN_COC: overridden by -c (src/map_assembler.c:191)
  c.line(&line);
  if (line.find("__REFERENCE__") == std::string::npos) maln_bad("Do not see reference sequence header in %s\n", fn);
  c.line(&line); field(line, "ID", &m->ref_id);
  c.line(&line); m->ref_desc.clear(); field(line, "DESC", &m->ref_desc);
  c.line(&line); field_int(line, "LEN", &m->L);
  c.line(&line); m->ref_size = 0; field_int(line, "SIZE", &m->ref_size);
  c.line(&line); field(line, "SEQ", &m->ref_seq);
  if ((int)m->ref_seq.size() != m->L) {
    fprintf(stderr, "Reported length of reference sequence %d is not observed length %d\n", m->L, (int)m->ref_seq.size());
    exit(1);
  }
  c.literal("GAPS");
  m->gaps.assign((size_t)m->L, 0);
  for (int i = 0; i < m->L; i++) { long v = 0; if (c.integer(&v)) m->gaps[(size_t)i] = (int32_t)v; }
  while (c.p < c.end && *c.p != '\n') c.p++;
  if (c.p < c.end) c.p++;
  c.line(&line);
  if (line.find("__PSSM__") == std::string::npos) { fprintf(stderr, "Do not see __PSSM__ line in %s\n", fn); exit(2); }
  int depth = PSSM_DEPTH;
  c.line(&line); field_int(line, "DEPTH", &depth);
  m->depth = depth;
  c.line(&line);
  if (line.find("FPSM:") == std::string::npos) { fprintf(stderr, "Do not see the FPSM: in %s\n", fn); exit(2); }
  memset(m->fpsm, 0, sizeof m->fpsm);
  memset(m->rpsm, 0, sizeof m->rpsm);
  read_matrices(c, depth, m->fpsm);
  c.line(&line);
  if (line.find("RPSM:") == std::string::npos) { fprintf(stderr, "Do not see the RPSM: in %s\n", fn); exit(2); }
  read_matrices(c, depth, m->rpsm);
  c.line(&line);
  if (line.find("__ALNSEQS__") == std::string::npos) maln_bad("Do not see __ALNSEQS__ line in %s\n", fn);
  m->rec.clear();
  m->rec.reserve((size_t)(nas > 0 ? nas : 0));
  for (int r = 0; r < nas; r++) {
    MalnRecord a;
    a.file_no = r;
    std::string seq, smp;
    c.line(&line); field(line, "ID", &a.id);
    c.line(&line);                                  // DESC: what follows "DESC ", without the newline
    if (line.size() > 5) a.desc.assign(line, 5, line.size() - 6);
    c.line(&line); field_int(line, "SCORE", &a.score);
    c.line(&line);                                  // NUM_INPUTS, if there (else 1)
    if (field_int(line, "NUM_INPUTS", &a.num_inputs)) c.line(&line);
    field_int(line, "START", &a.start);
    c.line(&line); field_int(line, "END", &a.end);
    c.line(&line); field_int(line, "RC", &a.rc);
    c.line(&line); field_int(line, "TR", &a.trimmed);
    c.line(&line);                                  // DR, if there
    if (field_int(line, "DR", &tmp)) { a.dropped = tmp; c.line(&line); }
    if (field(line, "SEG", &tok)) a.segment = tok[0];
    c.line(&line); field(line, "SEQ", &seq);
    c.line(&line); field(line, "SMP", &smp);
    const int ncols = a.end - a.start + 1;
    if (ncols < 0 || (int)seq.size() < ncols || (int)smp.size() < ncols || a.start < 0) {
      fprintf(stderr, "record %d of %s: SEQ/SMP shorter than START..END\n", r, fn);
      exit(1);
    }
    a.seq.assign(seq, 0, (size_t)ncols);
    a.smp.assign(smp, 0, (size_t)ncols);
    a.seq_raw = std::move(seq);
    a.smp_raw = std::move(smp);
    c.literal("INS_POS");
    for (;;) {
      const char* save = c.p;
      long pos = 0;
      if (!c.integer(&pos)) break;                   // (white space already consumed, as fscanf does)
      if (!c.token(&tok)) { c.p = save; break; }
      a.ins_pos.push_back((int32_t)pos);
      a.ins_seq.push_back(tok);
    }
    m->rec.push_back(std::move(a));
  }
  sort_records(m);
  flatten_records(m);
}

// ---- ma -m (write_ma, src/map_alignment.c:283-382) ---------------------------------------------------------------------------
// Everything from the MALN_NAS line on, the records in the order of `rec` (sorted: ma sorts before it writes).  cons_code is
// ma's -c (src/map_assembler.c:191), not the file's MALN_COC.  A record's INS_POS pairs are written by ascending position, of
// several pairs of one position the last, and only positions inside its SEQ string: write_ma walks ins[0 .. strlen(seq)).
inline void maln_body_text(const MalnFile& m, int cons_code, std::string* out) {
  char num[64];
  auto put_int = [&](const char* key, long v) { snprintf(num, sizeof num, "%s%ld\n", key, v); *out += num; };
  put_int("MALN_NAS ", (long)m.rec.size());
  put_int("MALN_SIZ ", m.maln_siz);
  put_int("MALN_COC ", cons_code);
  *out += "__REFERENCE__\nID " + m.ref_id + "\nDESC " + m.ref_desc + "\n";
  put_int("LEN ", m.L);
  put_int("SIZE ", m.ref_size);
  *out += "SEQ " + m.ref_seq + "\nGAPS";
  for (int p = 0; p < m.L; p++) { snprintf(num, sizeof num, " %d", m.gaps[(size_t)p]); *out += num; }
  *out += "\n__PSSM__\n";
  put_int("DEPTH ", m.depth);
  for (int s = 0; s < 2; s++) {
    const int32_t (*sm)[5][5] = s ? m.rpsm : m.fpsm;
    *out += s ? "RPSM:\n" : "FPSM:\n";
    for (int i = 0; i <= m.depth * 2 && i < 31; i++) {
      for (int row = 0; row <= 4; row++) {
        snprintf(num, sizeof num, "%d %d %d %d %d\n", sm[i][row][0], sm[i][row][1], sm[i][row][2], sm[i][row][3], sm[i][row][4]);
        *out += num;
      }
      *out += "\n";
    }
  }
  *out += "__ALNSEQS__\n";
  for (const MalnRecord& a : m.rec) {
    *out += "ID " + a.id + "\nDESC " + a.desc + "\n";
    put_int("SCORE ", a.score);
    put_int("NUM_INPUTS ", a.num_inputs);
    put_int("START ", a.start);
    put_int("END ", a.end);
    put_int("RC ", a.rc ? 1 : 0);
    put_int("TR ", a.trimmed ? 1 : 0);
    put_int("DR ", a.dropped ? 1 : 0);
    *out += "SEG ";
    *out += a.segment;
    *out += "\nSEQ " + a.seq_raw + "\nSMP " + a.smp_raw + "\nINS_POS";
    std::map<int32_t, size_t> last;                 // position -> the last pair given for it
    for (size_t k = 0; k < a.ins_pos.size(); k++)
      if (a.ins_pos[k] >= 0 && (size_t)a.ins_pos[k] < a.seq_raw.size()) last[a.ins_pos[k]] = k;
    for (const auto& e : last) { snprintf(num, sizeof num, " %d ", e.first); *out += num; *out += a.ins_seq[e.second]; }
    *out += "\n";
  }
}

inline bool write_maln_file(const char* fn, const MalnFile& m, int cons_code) {
  FILE* f = fopen(fn, "w");
  if (!f) { fprintf(stderr, "%s\n", fn); perror("Cannot open file"); return false; }
  time_t t = time(NULL);
  std::string text = "/* map_alignment [V1.0] */ ";
  text += asctime(localtime(&t));
  maln_body_text(m, cons_code, &text);
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return (fclose(f) == 0) && ok;
}

// ---- ma -R (parse_region, src/map_assembler.c:73-82) and print_region's clamp (src/map_align.c:561-567) --------------------
// sscanf "%d:%d": what does not parse keeps its default; the reference's swap assigns the smaller value to both ends.
inline void parse_region(const char* s, int* reg_start, int* reg_end) {
  sscanf(s, "%d:%d", reg_start, reg_end);
  if (*reg_start > *reg_end) { *reg_start = *reg_end; *reg_end = *reg_start; }
}
// 1-based inclusive region -> 0-based inclusive columns first .. last inside a reference of L columns (first > last: empty)
inline void clamp_region(int reg_start, int reg_end, int L, int* first, int* last) {
  if (reg_start < 1) reg_start = 1;
  if (reg_end > L) reg_end = L;
  *first = reg_start - 1;
  *last = reg_end - 1;
}

// the id print_region shows for a record: ID, then t|_ (trimmed), r|_ (reverse complement) and %02d of num_inputs -- of which
// read_id[4] = '\0' keeps two characters (src/map_align.c:664-681)
inline std::string region_label(const MalnRecord& a) {
  char num[16];
  snprintf(num, sizeof num, "%02d", a.num_inputs);
  std::string id = a.id;
  id += a.trimmed ? 't' : '_';
  id += a.rc ? 'r' : '_';
  id.append(num, 0, 2);
  return id;
}

}  // namespace maln_text
