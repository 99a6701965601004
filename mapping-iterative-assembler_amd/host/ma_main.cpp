// ma_hip -- the reference's `ma` report tool (/root/reference/src/map_assembler.c): -f 1 (clustalw, the default), -f 2 (line
// format), -f 5 (assembled sequence as FASTA), -f 41 and -f 4 (per-column table), -f 6 and -f 61 (the fragments of a region,
// -R), -f 7 (ACE export, every record in full), -f 8 (SAM, which the reference does not have: the reads as aligned to the reference), -f 9 and -f 91 (the substitution profile of the
// assembly, which the reference does not have either: substitution counts by distance from the read's ends, and a -s matrix made
// from them; -P pseudocount, -A dropped records too), -f 92 and -f 93 (which the reference does not have either: the reference bases around the places where reads
// begin and end, and the reads' lengths per strand), -f 95 (the damage classes of the molecules), -f 42 (likewise this tool's own: -f 41's base counts per
// strand, and the records that start and end on every column per strand, which are format 3's columns 5-8) and -m (the .maln written again, sorted, with -c and -I applied).  The .maln text is parsed exactly as read_ma does (host/maln_text.h); the add_base loops of show_consensus /
// find_ins_cons run on the GPU (mia_hip_ma_tally, every record counts, dropped or not), and so do the selection and the
// rows of the region view (mia_hip_ma_region), the padded reads of the ACE export (mia_hip_ma_ace) and CIGAR, SEQ and NM of the SAM
// export (mia_hip_ma_sam) and the counts of the substitution profile (mia_hip_ma_profile) and of the two
// fragment reports (mia_hip_ma_ends) and the strand table (mia_hip_ma_cols); calling, phred score and
// printing follow src/map_alignment.c:107-220, src/map_align.c:152-227,294-391,543-759 and src/io.c:756-913,929-1085.  Format 3
// (the summary of format 2 plus a table per column: coverage, and the records that start and that end there on either strand,
// src/map_align.c:761-849, src/map_alignment.c:635-653) stays outside; its four strand columns are part of -f 42.
// -u removes duplicate molecules in front of all of it (the reference has the rule in mia -u, not in ma): the
// halves of reads split at the origin are paired here (host/maln_dedup.h), the clusters are formed on the GPU (mia_hip_ma_dedup), the
// records that are not kept leave with their inserts and GAPS is reset as cull_maln_from_fsdb does (src/mia.c:484-504).
// -D N keeps only the molecules that carry a deamination signature themselves ("Deaminated fragments": a C read as T within N
// positions of the 5' end, a G read as A -- -S: a C read as T -- within N of the 3' end; -e says which ends must show it): it runs behind
// -u and in front of everything else, the per-record decision is made on the GPU (mia_hip_ma_damage) over the records of a tally of the
// file as it stands, and the records that are not kept leave as for -u.  -f 95 prints the molecules' damage classes.
// -E n5[,n3] masks the reads' ends behind -u and -D and in front of everything else ("End mask"): the columns whose depth code
// lies within n5 positions of the read's 5' end or n3 of its 3' end leave the record (with -x: a T there at the 5' end, an A -- -S: a T --
// at the 3' end becomes N), so that the consensus is not called from deaminated bases.  The new record view is made on the GPU
// (mia_hip_ma_mask) and put back into the file here (host/maln_mask.h); -f 96 prints what left.
// -L T keeps only the molecules whose damage score reaches T nat ("Damage score": a likelihood ratio of post-mortem damage
// against none, summed over every C and G column of the read, from the model -K p,c0,pi,eps fills a weight table with; -S: a
// single-stranded library): behind -u and -D and in front of -E, scored on the GPU (mia_hip_ma_score) over the records of a tally of the
// file as it stands; the records that are not kept leave as for -u.  -f 97 prints the molecules' scores as a histogram.
// -j (with -u) makes the copy that stays the consensus of its cluster ("Duplicate consensus"; the reference's idea is mia -C,
// collapse_FSDB, src/mia.c:140-233, on raw reads with qualities -- a .maln holds none, so the rule is this tool's own): the whole file is
// tallied first, the clusters are formed as for -u, every molecule of a cluster of two or more votes base by base on the columns of the
// representative's records on the GPU (mia_hip_ma_collapse; a dropped copy does not vote), and the new SEQ strings and NUM_INPUTS go
// into the records that stay (host/maln_collapse.h) before the others leave.  -f 98 prints what the votes changed.
// No CPU fallback.
#include <ctype.h>
#include <float.h>
#include <getopt.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mia_hip.h"
#include "maln_text.h"
#include "maln_dedup.h"
#include "maln_mask.h"
#include "maln_collapse.h"
#include "../csrc/ma_ace_body.h"
#include "../csrc/ma_sam_body.h"
#include "../csrc/ma_profile_body.h"
#include "../csrc/ma_ends_body.h"
#include "../csrc/ma_cols_body.h"
#include "../csrc/ma_dedup_body.h"
#include "../csrc/ma_damage_body.h"
#include "../csrc/ma_mask_body.h"
#include "../csrc/ma_pmd_body.h"

namespace {

constexpr int FASTA_LINE_WIDTH = 60, CLUSTALW_LINE_WIDTH = 60;   // src/params.h:19-20
using namespace maln_text;
typedef MalnFile Maln;

void help() {
  printf("ma_hip -M <maln input file>\n   -c <consensus code>\n   -f <output format: 1, 2, 4, 41, 42, 5, 6, 61, 7, 8, 9, 91, 92, 93, 95, 96, 97 or 98>\n   -R <REGION_START:REGION_END>\n"
         "   -I <ID to assign to assembly sequence>\n   -C colour format 6 output\n   -m <maln output file>\n"
         "   -P <pseudocount of format 91, default 1>\n   -A count dropped records too (formats 42, 9, 91, 92, 93, 95 and 97)\n"
         "   -u remove duplicate molecules first\n   -t <tolerance of -u in columns, 0 .. 100, default 0>\n"
         "   -j with -u: the copy that stays becomes the consensus of its cluster\n"
         "   -D <N: keep only deaminated fragments, a hit within N = 1 .. 15 positions of a read end>\n"
         "   -e <ends of -D that must show a hit: 5, 3, any (default) or both>\n   -S single-stranded library (-D, -L, formats 95 and 97, -x)\n"
         "   -L <T: keep only the molecules whose damage score is at least T nat>\n"
         "   -K <p,c0,pi,eps: the damage model of -L and format 97, default 0.3,0.01,0.001,0.000333333>\n"
         "   -E <n5[,n3]: mask n5 positions at the reads' 5' end and n3 (default n5) at their 3' end, 0 .. 15, not both 0>\n"
         "   -x with -E: do not trim, write N over the bases deamination makes\n"
         "ma_hip reports from a .maln file written by mia, as the reference's ma does: the alignment of consensus and reference\n"
         "(-f 1 clustalw, the default; -f 2 one line each plus coverage), the per-column table (-f 41 all positions, -f 4\n"
         "positions that differ from the reference), the assembled sequence (-f 5), and the reference, the consensus and every\n"
         "fragment of a region (-f 6, as multi-FASTA -f 61; -R, default 90:109).  Tallies, the selection of the fragments and\n"
         "their rows are computed on the MI355X, and so are the padded reads of the ACE export (-f 7).  -m writes the .maln\n"
         "again: records sorted, -c and -I applied.  -f 8 writes the records as SAM (one line each, aligned to the reference;\n"
         "CIGAR, SEQ and NM come from the MI355X; the reference's ma has no such format).  -f 9 prints the substitution profile of\n"
         "the assembly: per distance from the read's 5' end (1..15), MIDDLE and distance from its 3' end (-15..-1) how often a\n"
         "reference base was read as which base, the deletions, and the columns with an N or another code (C>T at the first\n"
         "and G>A at the last positions is the damage of ancient DNA); -f 91 prints a substitution matrix made from these counts,\n"
         "a file for mia -s (100 * log2 of the share of each read base per reference base over 0.25, -P added to every count).\n"
         "-f 92 prints the fragmentation context: for the 5' and the 3' ends of the reads the reference bases at the ten positions\n"
         "in front of (-10..-1) and behind (+1..+10) each end, in the read's orientation (an excess of purines at 5' -1 is the\n"
         "depurination of ancient DNA); -f 93 prints the distribution of the reads' lengths per strand.  A read split at the\n"
         "origin gives only its true ends and no length.\n"
         "-f 42 prints the strand table: a line per reference column (-R: of that region only) with the A, C, G, T, gap and other\n"
         "columns of the forward (+) and of the reverse (-) records there, and the records that start and that end on it per strand\n"
         "(damage shows as C>T on + and G>A on -; a variant shows on both; many starts on one column of one strand are duplicates).\n"
         "Dropped records do not count unless -A is given; the counts come from the MI355X.\n"
         "-u removes duplicates before anything else is computed, by the rule of mia -u: molecules (a read split at the origin is one)\n"
         "with the same strand, start and end are one cluster -- with -t N, also those within N columns of the cluster's first in\n"
         "start and in end -- and only the best-scoring molecule of the cluster's first coordinates stays; GAPS shrinks to the inserts\n"
         "of what is left, and every format and -m see the smaller file.  Clusters are formed on the MI355X.\n"
         "-D N keeps only the molecules that are deaminated themselves, behind -u and in front of everything else: a reference C read as T at\n"
         "one of the first N positions of the read (a 5' hit), or a reference G read as A at one of its last N positions (a 3' hit; -S, a\n"
         "single-stranded library: a C read as T there too), positions as mia scored them (1 .. 15 from either end), in the read's\n"
         "orientation; a read split at the origin is one molecule.  -e 5 asks for a 5' hit, -e 3 for a 3' hit, -e both for both, -e any\n"
         "(the default) for either.  What is not kept leaves as for -u, and the consensus is called from the deaminated fragments alone\n"
         "(-D 1 -e 3 -f 9 prints the 5' profile of the fragments deaminated at their 3' end).  The decision is made on the MI355X.\n"
         "-f 95 prints the damage classes of the file as it stands behind -u and -D: for N = 1 .. 15 the molecules with a 5' hit within N,\n"
         "with a 3' hit within N, with both and with either, on the forward strand, the reverse strand and both.\n"
         "-E n5[,n3] masks the reads' ends behind -u and -D and in front of everything else: a column belongs to a read's 5' end when the\n"
         "position mia scored it at (1 .. 15 from either end, in the read's orientation) is at most n5, to its 3' end when it is at most n3.\n"
         "Those columns at either end of a record leave it, with the '-' columns next to them; START, END and the inserts' positions move,\n"
         "an insert in front of the new first column leaves, a record that keeps no base leaves the file, GAPS shrinks as for -u.  With -x\n"
         "nothing leaves: a T at the 5' end and an A (-S: a T) at the 3' end, in the read's orientation, become N.  Every format and -m see\n"
         "the masked file; formats 92, 93, 95 and 97 describe real fragment ends and refuse -E.  The mask is made on the MI355X.  -f 96 prints\n"
         "what the mask took: per position 1 .. 15 the columns removed (-x: set to N) at the 5' and 3' ends of forward and reverse records.\n"
         "-L T keeps only the molecules whose damage score is at least T nat, behind -u and -D and in front of -E.  The score is a log\n"
         "likelihood ratio of post-mortem damage against none over all of the read: every reference C read as C or T, and every reference G\n"
         "read as G or A (-S: C columns only), in the read's orientation, adds a weight that depends on its position as mia scored it.  -K\n"
         "sets the model the weights come from: C>T with probability c0 + p (1-p)^(k-1) at position k from the 5' end (G>A likewise from\n"
         "the 3' end; -S: C>T at both ends), polymorphism rate pi, error rate eps.  A read split at the origin is one molecule.  What is not\n"
         "kept leaves as for -u.  The score is summed on the MI355X.  -f 97 prints the scores of the file as it stands behind -u, -D and -L:\n"
         "per strand and for both the molecules in every half-nat bin from -10 to 21.5 nat, and those in this bin or above.\n"
         "-j (with -u) does not throw the other copies' information away: every molecule of a cluster of two or more votes, base by base,\n"
         "on the columns of the copy that stays.  A, C, G, T and '-' are votes ('-' not at a record's first and last column), anything else is\n"
         "none, a dropped copy does not vote.  One character strictly ahead replaces the column (the copy's own lower case survives when it\n"
         "wins); when several tie the copy's own stays if it is one of them, otherwise the column becomes N.  NUM_INPUTS becomes the sum over\n"
         "the voting copies; inserted bases, depth codes and everything else stay the kept copy's.  It runs before -D, -L and -E, so that an\n"
         "error in one copy is not taken for damage.  The votes are counted on the MI355X.  -f 98 prints, per cluster size (2, 3, 4, 5-8, 9-16,\n"
         "17+) and strand, the clusters, the columns with a vote, those not unanimous and those changed to a base, to '-' and to N.\n"
         "Format 3 (format 2's summary plus\n"
         "a table of coverage and of the records that start and end at every column) is outside the accelerated path.\n");
}

void read_ma(const char* fn, Maln* m) { read_maln_file(fn, m); }

// find_phred_qscore, src/map_align.c:152-205
int phred(int sA, int sC, int sG, int sT) {
  int best, nb[3];
  if (sA >= sC && sA >= sG && sA >= sT) { best = sA; nb[0] = sC; nb[1] = sG; nb[2] = sT; }
  else if (sC >= sG && sC >= sT) { best = sC; nb[0] = sA; nb[1] = sG; nb[2] = sT; }
  else if (sG >= sT) { best = sG; nb[0] = sA; nb[1] = sC; nb[2] = sT; }
  else { best = sT; nb[0] = sA; nb[1] = sC; nb[2] = sG; }
  double p_best = pow(2, ((double)best / 100));
  double p_nbs[3];
  for (int i = 0; i < 3; i++) p_nbs[i] = pow(2, ((double)nb[i] / 100));
  double p_correct = p_best / (p_nbs[0] + p_nbs[1] + p_nbs[2]);
  if (p_correct >= DBL_MAX) p_correct = DBL_MAX;
  return 10 * log10(p_correct);
}

struct Counts { int As, Cs, Gs, Ts, gaps, cov, sA, sC, sG, sT; };

// find_consensus, src/map_align.c:294-391 (the call AND frac_agree)
char find_consensus(const Counts& b, int cons_code, double* frac) {
  if (b.cov == 0) { *frac = 0.0; return 'N'; }
  if (((double)b.gaps / (double)b.cov) >= (double)(50 / 100.0)) { *frac = ((double)b.gaps / (double)b.cov); return '-'; }
  int top = b.sA, second = INT_MIN;
  char base = 'A';
  *frac = ((double)b.As / (double)b.cov);
  if (b.sC >= top) { second = top; top = b.sC; base = 'C'; *frac = ((double)b.Cs / (double)b.cov); } else second = b.sC;
  if (b.sG >= top) { second = top; top = b.sG; base = 'G'; *frac = ((double)b.Gs / (double)b.cov); } else if (b.sG >= second) second = b.sG;
  if (b.sT >= top) { second = top; top = b.sT; base = 'T'; *frac = ((double)b.Ts / (double)b.cov); } else if (b.sT >= second) second = b.sT;
  if (cons_code == 2) return (top >= 0 || (top - 2400) > second) ? base : 'N';
  return (top >= -399) ? base : 'N';
}

void show_single_pos(int ref_pos, char ref_base, char cons_base, const Counts& b, double frac) {   // src/map_align.c:208-227
  printf("%d %c %c %d %d %d %d %d %d %d %d %d %d %d %0.3f\n", ref_pos, ref_base, cons_base, b.cov, b.As, b.Cs, b.Gs, b.Ts, b.gaps, b.sA, b.sC,
         b.sG, b.sT, phred(b.sA, b.sC, b.sG, b.sT), frac);
}

// fasta_aln_print, src/io.c:953-973
void fasta_aln_print(const char* seq, size_t len, const std::string& id) {
  printf(">%s\n", id.c_str());
  size_t i = 0;
  for (; i + FASTA_LINE_WIDTH <= len; i += FASTA_LINE_WIDTH) {
    for (size_t k = 0; k < (size_t)FASTA_LINE_WIDTH; k++) fputc(seq[i + k] == ' ' ? 'X' : seq[i + k], stdout);
    fputc('\n', stdout);
  }
  for (; i < len; i++) fputc(seq[i] == ' ' ? 'X' : seq[i], stdout);
  fputc('\n', stdout);
}

// clustalw_print_cons, src/io.c:976-1029
void clustalw_print_cons(const std::string& cons, const std::string& aln_ref, const std::string& ref_id) {
  std::string ref_start = ref_id.substr(0, 15);
  ref_start.resize(17, ' ');
  printf("CLUSTAL W (1.8) multiple sequence alignment\n");
  for (size_t at = 0; at < cons.size(); at += CLUSTALW_LINE_WIDTH) {
    const std::string r = aln_ref.substr(at, CLUSTALW_LINE_WIDTH);
    std::string c = cons.substr(at, CLUSTALW_LINE_WIDTH);
    for (char& ch : c) if (ch == ' ') ch = 'X';
    printf("%s%s\nConsensus        %s\n                 ", ref_start.c_str(), r.c_str(), c.c_str());
    for (size_t i = 0; i < c.size(); i++) fputc(i < r.size() && r[i] == c[i] ? '*' : ' ', stdout);
    printf("\n\n\n");
  }
}

// color_print, src/io.c:1044-1085
void color_print(const char* s, size_t len) {
  for (size_t i = 0; i < len; i++) {
    switch (s[i]) {
      case 'a': case 'A': printf("\33[37;42m"); break;
      case 'c': case 'C': printf("\33[37;44m"); break;
      case 'g': case 'G': printf("\33[37;40m"); break;
      case 't': case 'T': printf("\33[37;41m"); break;
      case '-': printf("\33[47;30m"); break;
      default: printf("\33[0m");
    }
    fputc(s[i], stdout);
  }
  printf("\33[0m\n");
}

// Output of the ACE export: one buffer, written out whenever it has grown past a few megabytes
struct Out {
  std::string buf;
  void flush() { if (!buf.empty()) { fwrite(buf.data(), 1, buf.size(), stdout); buf.clear(); } }
  void room() { if (buf.size() > ((size_t)4 << 20)) flush(); }
  void fmt(const char* f, ...) __attribute__((format(printf, 2, 3))) {
    char line[1024];
    va_list ap;
    va_start(ap, f);
    const int k = vsnprintf(line, sizeof line, f, ap);
    va_end(ap);
    if (k > 0) buf.append(line, (size_t)k < sizeof line ? (size_t)k : sizeof line - 1);
  }
};

// the consensus block of ace_output (src/io.c:780-793, 893-906): lines of 50, '-' as '*', ' ' as 'X', the remainder line even when empty
void ace_consensus(Out& o, const std::string& cons) {
  size_t at = o.buf.size(), line_pos = 0;
  o.buf.resize(at + cons.size() + cons.size() / 50 + 1);
  for (char c : cons) {
    o.buf[at++] = c == '-' ? '*' : (c == ' ' ? 'X' : c);
    if (++line_pos == 50) { o.buf[at++] = '\n'; line_pos = 0; }
  }
  o.buf[at++] = '\n';
}

// ace_output, src/io.c:756-913: everything but the padded reads, which come from the device already cut into lines
void ace_print(const Maln& m, const std::string& cons, const std::vector<int64_t>& af_pos, const std::vector<int64_t>& padded_len,
               const std::vector<int64_t>& body_off, const std::string& body) {
  Out o;
  const size_t n = m.rec.size();
  const long long number_bases = (long long)cons.size();   // get_consensus_length: gaps[0] is 0 here, so it is the string's length
  o.fmt("AS %d %zu\n\n", 1, n + 1);
  o.buf += "CO " + m.ref_id;
  o.fmt(" %lld %zu %d %c\n", number_bases, n + 1, 1, 'U');
  ace_consensus(o, cons);
  o.buf += "\nBQ\n";
  for (size_t i = 0; i < cons.size(); i++) {
    if (cons[i] != '-') o.buf += "40 ";
    if (i % 50 == 0) o.buf += '\n';
  }
  o.buf += "\n\nAF FAKE_READ-IGNORE_ME U 1\n";
  for (size_t r = 0; r < n; r++) {
    o.buf += "AF " + m.rec[r].id;
    o.fmt(" %c %lld\n", m.rec[r].rc ? 'C' : 'U', (long long)af_pos[r]);
    o.room();
  }
  o.fmt("\nBS 1 %lld FAKE_READ-IGNORE_ME\n\n", number_bases);
  for (size_t r = 0; r < n; r++) {
    const MalnRecord& a = m.rec[r];
    // strlen(aln_seq->seq) + gaps: what the SEQ string held behind column END counts, though it is not printed
    const long long len = (long long)padded_len[r] + ((long long)a.seq_raw.size() - (long long)a.seq.size());
    o.buf += "RD " + a.id;
    o.fmt(" %lld 0 0\n", len);
    o.buf.append(body, (size_t)body_off[r], (size_t)(body_off[r + 1] - body_off[r]));
    o.fmt("\nQA 1 %lld 1 %lld\n", len, len);
    o.buf += "DS CHROMAT_FILE: " + a.id + " PHD_FILE: " + a.id + "_FAKE.phd TIME: Tue Feb 21 15:42:35 1984\n\n";
    o.room();
  }
  o.fmt("RD FAKE_READ-IGNORE_ME %lld 0 0\n", number_bases);
  ace_consensus(o, cons);
  o.fmt("\n\nQA 1 %lld 1 %lld\n", number_bases, number_bases);
  o.buf += "DS CHROMAT_FILE: FAKE_READ PHD_FILE: FAKE_READ_FAKE.phd TIME: Tue Feb 21 23:23:23 1984\n";
  o.flush();
}

// SAM (-f 8): header, and per record everything in front of and behind the body the device made (fields 6-10)
void sam_print(const Maln& m, const std::vector<int32_t>& nm, const std::vector<int64_t>& body_off, const std::string& body) {
  Out o;
  o.buf += "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:" + m.ref_id;
  o.fmt("\tLN:%d\n@PG\tID:ma_hip\tPN:ma_hip\n", m.L);
  for (size_t r = 0; r < m.rec.size(); r++) {
    const MalnRecord& a = m.rec[r];
    o.buf += a.id;
    o.fmt("\t%d\t", (a.rc ? 16 : 0) + (a.dropped ? 512 : 0) + (a.segment == 'b' ? 2048 : 0));
    o.buf += m.ref_id;
    o.fmt("\t%d\t255\t", a.start + 1);
    o.buf.append(body, (size_t)body_off[r], (size_t)(body_off[r + 1] - body_off[r]));
    o.fmt("\t*\tAS:i:%d\tNM:i:%d\tXN:i:%d\tXS:A:%c\tXT:i:%d\n", a.score, nm[r], a.num_inputs, a.segment, a.trimmed ? 1 : 0);
    o.room();
  }
  o.flush();
}

// -f 9: the counts as a table, a line per depth code
void profile_table(int64_t n_used, int64_t n_events, const int64_t* count, const int64_t* del, int64_t bad_code, int64_t beyond) {
  Out o;
  o.fmt("# ma_hip substitution profile: %lld records, %lld columns, %lld bad depth codes, %lld columns beyond the reference\n", (long long)n_used,
        (long long)n_events, (long long)bad_code, (long long)beyond);
  o.buf += "# position";
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) o.fmt("\t%c>%c", "ACGT"[i], "ACGT"[j]);
  o.buf += "\tdel\tother\n";
  for (int d = 0; d < mia::MA_PROF_DEPTHS; d++) {
    char label[16];
    mia::ma_prof_label(d, label);
    o.buf += label;
    const int64_t* c = count + d * 25;
    int64_t other = 0;
    for (int i = 0; i < 5; i++) for (int j = 0; j < 5; j++) {
      if (i < 4 && j < 4) o.fmt("\t%lld", (long long)c[i * 5 + j]); else other += c[i * 5 + j];
    }
    o.fmt("\t%lld\t%lld\n", (long long)del[d], (long long)other);
  }
  o.flush();
}

// -f 91: the counts as a matrix file in the layout of matrices/ancient.submat.txt, which read_pssm (src/io.c:408-503) reads
void profile_matrix(const int64_t* count, double alpha) {
  Out o;
  for (int d = 0; d < mia::MA_PROF_DEPTHS; d++) {
    char label[16];
    mia::ma_prof_label(d, label);
    o.fmt("# Matrix for position: %s\n", label);
    for (int i = 0; i < 4; i++) {
      const int64_t* c = count + (d * 5 + i) * 5;
      for (int j = 0; j < 4; j++) o.fmt("%d\t", mia::ma_prof_score(c, i, j, alpha));
      o.buf += '\n';
    }
    o.buf += '\n';
  }
  o.flush();
}

// -f 92: the reference's classes around the reads' ends, a line per end and position
void ends_table(int64_t n_used, int64_t n5, int64_t n3, const int64_t* ctx_count) {
  Out o;
  o.fmt("# ma_hip fragment ends: %lld records, %lld 5' ends, %lld 3' ends\n", (long long)n_used, (long long)n5, (long long)n3);
  o.buf += "# end\tposition\tA\tC\tG\tT\tother\toutside\n";
  for (int end = 0; end < 2; end++)
    for (int p = 0; p < mia::MA_ENDS_POS; p++) {
      o.fmt("%s\t%+d", end ? "3p" : "5p", mia::ma_ends_k(p));
      for (int c = 0; c < mia::MA_ENDS_CLASSES; c++) o.fmt("\t%lld", (long long)ctx_count[mia::ma_ends_ctx_bin(end, p, c)]);
      o.buf += '\n';
    }
  o.flush();
}

// -f 93: the lengths of the whole records per strand, from the shortest to the longest that occurs
void lengths_table(const int64_t* len_count, int64_t halves) {
  const int64_t* fwd = len_count;
  const int64_t* rev = len_count + mia::MA_ENDS_LENS;
  int64_t whole = 0;
  int lo = mia::MA_ENDS_MAX_LEN, hi = -1;
  for (int l = 0; l <= mia::MA_ENDS_MAX_LEN; l++) {
    whole += fwd[l] + rev[l];
    if (l < mia::MA_ENDS_MAX_LEN && fwd[l] + rev[l] > 0) { if (lo > l) lo = l; hi = l; }
  }
  const int64_t longer = fwd[mia::MA_ENDS_MAX_LEN] + rev[mia::MA_ENDS_MAX_LEN];
  Out o;
  o.fmt("# ma_hip read lengths: %lld whole records, %lld halves of reads split at the origin (not counted), %lld longer than %d\n", (long long)whole,
        (long long)halves, (long long)longer, mia::MA_ENDS_MAX_LEN - 1);
  o.buf += "# length\tforward\treverse\n";
  for (int l = lo; l <= hi; l++) o.fmt("%d\t%lld\t%lld\n", l, (long long)fwd[l], (long long)rev[l]);
  if (longer > 0) o.fmt(">%d\t%lld\t%lld\n", mia::MA_ENDS_MAX_LEN - 1, (long long)fwd[mia::MA_ENDS_MAX_LEN], (long long)rev[mia::MA_ENDS_MAX_LEN]);
  o.flush();
}

// -f 42: the sixteen words of the reference columns first .. last
void cols_table(const Maln& m, int64_t n_used, int64_t n_events, int64_t beyond, int64_t ends_outside, const int32_t* cols, int first, int last) {
  Out o;
  o.fmt("# ma_hip strand table: %lld records, %lld columns, %lld beyond the reference, %lld ends outside it\n", (long long)n_used, (long long)n_events,
        (long long)beyond, (long long)ends_outside);
  o.buf += "# position\treference\tA+\tC+\tG+\tT+\tgap+\tother+\tA-\tC-\tG-\tT-\tgap-\tother-\tstarts+\tstarts-\tends+\tends-\n";
  for (int p = first; p <= last; p++) {
    o.fmt("%d\t%c", p + 1, m.ref_seq[(size_t)p]);
    for (int w = 0; w < mia::MA_COLS_WORDS; w++) o.fmt("\t%d", cols[(size_t)w * (size_t)m.L + (size_t)p]);
    o.buf += '\n';
    o.room();
  }
  o.flush();
}

// -f 95: the damage classes, from hist[strand][m5][m3] alone
void damage_table(int64_t n_molecules, int64_t orphans, int64_t n_used, bool single_stranded, const int64_t* hist) {
  Out o;
  o.fmt("# ma_hip damage classes: %lld molecules, %lld orphan halves, %lld records, library %s\n", (long long)n_molecules, (long long)orphans,
        (long long)n_used, single_stranded ? "ss" : "ds");
  o.buf += "# N";
  for (const char* strand : {"+", "-", ""}) for (const char* what : {"5p", "3p", "both", "either"}) o.fmt("\t%s%s", what, strand);
  o.buf += '\n';
  for (int n_pos = 1; n_pos <= mia::MA_DMG_MAX_POS; n_pos++) {
    o.fmt("%d", n_pos);
    for (int strand = 0; strand < 3; strand++) {
      int64_t row[4];
      mia::ma_dmg_row(hist, strand, n_pos, row);
      for (int k = 0; k < 4; k++) o.fmt("\t%lld", (long long)row[k]);
    }
    o.buf += '\n';
  }
  o.flush();
}

// -f 97: the molecules' scores per bin, from hist[strand][bin] alone
void score_table(int64_t n_molecules, int64_t orphans, int64_t n_used, bool single_stranded, const double model[4], const int64_t* hist) {
  Out o;
  o.fmt("# ma_hip damage scores: %lld molecules, %lld orphan halves, %lld records, library %s, p %g c0 %g pi %g eps %g\n", (long long)n_molecules,
        (long long)orphans, (long long)n_used, single_stranded ? "ss" : "ds", model[0], model[1], model[2], model[3]);
  o.buf += "# from\t+\t-\tall\tfrom+\tfrom-\tfrom_all\n";
  for (int b = 0; b < mia::MA_PMD_HIST_BINS; b++) {
    if (b == 0) o.buf += "-inf"; else o.fmt("%.1f", mia::ma_pmd_bin_from(b));
    int64_t row[3][2];
    for (int strand = 0; strand < 3; strand++) mia::ma_pmd_row(hist, strand, b, row[strand]);
    for (int k = 0; k < 2; k++) for (int strand = 0; strand < 3; strand++) o.fmt("\t%lld", (long long)row[strand][k]);
    o.buf += '\n';
  }
  o.flush();
}

// -K p,c0,pi,eps: four numbers and nothing else
bool parse_model(const char* s, double out[4]) {
  for (int k = 0; k < 4; k++) {
    char* end = nullptr;
    out[k] = strtod(s, &end);
    if (end == s || *end != (k < 3 ? ',' : '\0')) return false;
    s = end + 1;
  }
  return true;
}

void die(mia_hip_ctx* g, const char* what) {
  fprintf(stderr, "%s: %s\n", what, g ? mia_hip_last_error(g) : "no context");
  exit(1);
}

}  // namespace

int main(int argc, char* argv[]) {
  std::string ma_in_fn, assign_id, ma_out_fn;
  bool id_assigned = false, in_ma = false, any_arg = false, out_ma = false;
  int cons_scheme = 1, out_format = 1, gpu = 0, reg_start = 90, reg_end = 109;
  bool in_color = false, use_dropped = false, region_given = false, dedup = false, tol_given = false, collapse = false;
  long tolerance = 0, damage_n = 0;
  bool damage = false, ends_given = false, single_stranded = false;
  int ends_mode = mia::MA_DMG_ANY;
  bool mask = false, mask_ok = false, substitute = false;
  long mask_n5 = 0, mask_n3 = 0;
  bool score = false, score_ok = false, model_given = false, model_ok = false;
  double score_nat = 0.0, model[4] = {0.3, 0.01, 0.001, 0.001 / 3};
  double score_int = -1.0, score_slo = -1.0, alpha = 1.0;
  int ich;
  // the reference's option string (src/map_assembler.c:113) plus -g <gpu>, -P <pseudocount>, -A, -u, -t <tolerance>, -D <N>, -e <ends>, -S, -E <n5[,n3]>, -x, -L <T>, -K <p,c0,pi,eps> and -j
  while ((ich = getopt(argc, argv, "I:c:i:f:R:s:m:M:Cb:s:dg:P:Aut:D:e:SE:xL:K:j")) != -1) {
    switch (ich) {
      case 'I': assign_id = optarg; id_assigned = true; break;
      case 'c': cons_scheme = atoi(optarg); any_arg = true; break;
      case 'i': any_arg = true; break;                 // parsed and never used by the reference either
      case 'f': out_format = atoi(optarg); any_arg = true; break;
      case 'R': parse_region(optarg, &reg_start, &reg_end); region_given = true; any_arg = true; break;
      case 's': score_slo = atof(optarg); any_arg = true; break;
      case 'b': score_int = atof(optarg); any_arg = true; break;
      case 'C': in_color = true; break;
      case 'm': ma_out_fn = optarg; out_ma = true; any_arg = true; break;
      case 'M': ma_in_fn = optarg; in_ma = true; any_arg = true; break;
      case 'd': any_arg = true; break;
      case 'g': gpu = atoi(optarg); break;
      case 'P': { char* end = nullptr; alpha = strtod(optarg, &end); if (end == optarg || *end) alpha = NAN; } break;
      case 'A': use_dropped = true; break;
      case 'u': dedup = true; any_arg = true; break;
      case 't': { char* end = nullptr; tolerance = strtol(optarg, &end, 10); if (end == optarg || *end) tolerance = -1; tol_given = true; } break;
      case 'D': { char* end = nullptr; damage_n = strtol(optarg, &end, 10); if (end == optarg || *end) damage_n = -1; damage = true; any_arg = true; } break;
      case 'e':
        ends_given = true;
        ends_mode = !strcmp(optarg, "any") ? mia::MA_DMG_ANY : !strcmp(optarg, "5") ? mia::MA_DMG_5 : !strcmp(optarg, "3") ? mia::MA_DMG_3 : !strcmp(optarg, "both") ? mia::MA_DMG_BOTH : -1;
        break;
      case 'S': single_stranded = true; break;
      case 'E': mask = true; mask_ok = parse_mask_ends(optarg, &mask_n5, &mask_n3); any_arg = true; break;
      case 'x': substitute = true; break;
      case 'j': collapse = true; break;
      case 'L': { char* end = nullptr; score_nat = strtod(optarg, &end); score_ok = end != optarg && !*end && isfinite(score_nat) && fabs(score_nat) <= 1e12; score = true; any_arg = true; } break;
      case 'K': model_given = true; model_ok = parse_model(optarg, model); break;
      default: help(); exit(0);
    }
  }
  if (!any_arg || ((score_slo == -1) && (score_int != -1)) || ((score_slo != -1) && (score_int == -1)) || !in_ma) { help(); exit(0); }
  if (out_format != 1 && out_format != 2 && out_format != 5 && out_format != 4 && out_format != 41 && out_format != 42 && out_format != 6 && out_format != 61 && out_format != 7 && out_format != 8 && out_format != 9 && out_format != 91 && out_format != 92 && out_format != 93 && out_format != 95 && out_format != 96 && out_format != 97 && out_format != 98) {
    fprintf(stderr, "output format %d is outside the MI355X-accelerated path (formats 1, 2, 4, 41, 5, 6, 61 and 7 are, and 42, 8, 9, 91, 92, 93, 95, 96, 97 and 98, which the reference does not have); use the reference's ma\n", out_format);
    exit(1);
  }
  if (out_format == 91 && !mia::ma_prof_alpha_ok(alpha)) {
    fprintf(stderr, "ma_hip: -P must be a number from %g to %g\n", mia::MA_PROF_MIN_ALPHA, mia::MA_PROF_MAX_ALPHA);
    exit(1);
  }
  if (tol_given && !dedup) { fprintf(stderr, "ma_hip: -t is the tolerance of -u, which is not given\n"); exit(1); }
  if (tolerance < 0 || tolerance > mia::MA_DEDUP_MAX_TOL) { fprintf(stderr, "ma_hip: -t must be a whole number from 0 to %d\n", mia::MA_DEDUP_MAX_TOL); exit(1); }
  if (collapse && !dedup) { fprintf(stderr, "ma_hip: -j is the consensus of the clusters of -u, which is not given\n"); exit(1); }
  if (out_format == 98 && !collapse) { fprintf(stderr, "ma_hip: -f 98 is the report of -j, which is not given\n"); exit(1); }
  if (ends_given && !damage) { fprintf(stderr, "ma_hip: -e names the ends of -D, which is not given\n"); exit(1); }
  if (substitute && !mask) { fprintf(stderr, "ma_hip: -x is the substitution mode of -E, which is not given\n"); exit(1); }
  if (out_format == 96 && !mask) { fprintf(stderr, "ma_hip: -f 96 is the report of -E, which is not given\n"); exit(1); }
  if (mask && (!mask_ok || !mia::ma_mask_args_ok((int)mask_n5, (int)mask_n3, mia::MA_MASK_TRIM, 0))) {
    fprintf(stderr, "ma_hip: -E must be n5 or n5,n3: whole numbers from 0 to %d, not both 0\n", mia::MA_MASK_MAX_POS);
    exit(1);
  }
  if (mask && (out_format == 92 || out_format == 93 || out_format == 95 || out_format == 97)) {
    fprintf(stderr, "ma_hip: -f %d describes real fragment ends and cannot follow -E, which masks them\n", out_format);
    exit(1);
  }
  if (single_stranded && !damage && out_format != 95 && !substitute && !score && out_format != 97) { fprintf(stderr, "ma_hip: -S is the library type of -D and of -f 95, neither of which is given\n"); exit(1); }
  if (damage && !mia::ma_dmg_pos_ok((int)(damage_n < 0 || damage_n > 1000 ? -1 : damage_n))) {
    fprintf(stderr, "ma_hip: -D must be a whole number from 1 to %d\n", mia::MA_DMG_MAX_POS);
    exit(1);
  }
  if (ends_given && ends_mode < 0) { fprintf(stderr, "ma_hip: -e (the ends of -D) must be 5, 3, any or both\n"); exit(1); }
  if (model_given && !score && out_format != 97) { fprintf(stderr, "ma_hip: -K is the damage model of -L and of -f 97, neither of which is given\n"); exit(1); }
  if (score && !score_ok) { fprintf(stderr, "ma_hip: -L must be a finite decimal number, the least damage score in nat\n"); exit(1); }
  if (model_given && !model_ok) { fprintf(stderr, "ma_hip: -K must be p,c0,pi,eps: four numbers, the damage model of -L and of -f 97\n"); exit(1); }
  std::vector<int32_t> weights((size_t)mia::MA_PMD_WEIGHTS, 0);
  if ((score || out_format == 97) &&
      (mia_hip_ma_pmd_table(model[0], model[1], model[2], model[3], single_stranded ? 1 : 0, weights.data()) != MIA_HIP_OK || !mia::ma_pmd_weights_ok(weights.data()))) {
    fprintf(stderr, "ma_hip: -K must hold 0 < p < 1, 0 <= c0 < 1, 0 < pi < 1, 0 < eps < 1 and c0 + p < 1, and give weights of at most 16 nat\n");
    exit(1);
  }
  Maln m;
  read_ma(ma_in_fn.c_str(), &m);
  if (id_assigned) m.ref_id = assign_id.substr(0, 256);
  mia_hip_ctx* g = nullptr;
  auto open_gpu = [&]() {
    if (!g && mia_hip_create(&g, gpu) != MIA_HIP_OK) { fprintf(stderr, "ma_hip: no usable MI355X (gfx950) device %d; there is no CPU fallback\n", gpu); exit(1); }
  };
  // the file as it stands goes to the device: the PSSMs and the records (mia_hip_ma_tally, which also validates them)
  auto tally_file = [&]() {
    open_gpu();
    if (mia_hip_set_pssm(g, &m.fpsm[0][0][0], &m.rpsm[0][0][0]) != MIA_HIP_OK) die(g, "set_pssm");
    if (mia_hip_ma_tally(g, m.L, m.gaps.data(), (int64_t)m.start.size(), m.start.data(), m.revcom.data(), m.col_off.data(), m.seq.data(), m.smp.data(),
                         (int64_t)m.ins_record.size(), m.ins_record.data(), m.ins_pos.data(), m.ins_off.data(), m.ins_bases.data()) != MIA_HIP_OK)
      die(g, "ma_tally");
  };
  CollapseResult collapsed;
  if (dedup) {
    // the duplicate filter, in front of everything: clusters over all records (dropped or not) on the device, then -u takes out what
    // is not kept and every check and report below sees the smaller file
    DedupInput in;
    std::string why;
    if (!dedup_input(m, &in, &why)) { fprintf(stderr, "ma_hip: %s has no duplicate filter: %s\n", ma_in_fn.c_str(), why.c_str()); exit(1); }
    open_gpu();
    if (collapse) tally_file();                        // -j: the votes are read from the tallied records of the whole file
    const int64_t n_all = (int64_t)m.rec.size();
    int64_t n_molecules = 0, n_clusters = 0;
    std::vector<uint8_t> keep_file((size_t)n_all + 1, 1), keep((size_t)n_all);
    if (mia_hip_ma_dedup(g, m.L, n_all, in.start.data(), in.end.data(), in.revcom.data(), in.score.data(), in.mate.data(), (int32_t)tolerance, &n_molecules,
                         &n_clusters) != MIA_HIP_OK)
      die(g, "ma_dedup");
    if (mia_hip_get_ma_dedup(g, keep_file.data(), nullptr, nullptr, nullptr) != MIA_HIP_OK) die(g, "get_ma_dedup");
    for (int64_t f = 0; f < n_all; f++) keep[in.at[(size_t)f]] = keep_file[(size_t)f];
    if (collapse) {
      // the duplicate consensus: the clusters' votes on the device, SEQ' and NUM_INPUTS into the records that stay, then -u as ever
      std::vector<int64_t> rec_of((size_t)n_all + 1, 0);
      std::vector<uint8_t> vote((size_t)n_all + 1, 1);
      for (int64_t f = 0; f < n_all; f++) rec_of[(size_t)f] = (int64_t)in.at[(size_t)f];
      for (int64_t k = 0; k < n_all; k++) vote[(size_t)k] = m.rec[(size_t)k].dropped ? 0 : 1;
      collapsed.keep.assign(keep_file.begin(), keep_file.end());
      collapsed.rep.assign((size_t)n_all + 1, 0);
      collapsed.molecules = n_molecules; collapsed.clusters = n_clusters;
      if (mia_hip_get_ma_dedup(g, nullptr, collapsed.rep.data(), nullptr, &collapsed.orphans) != MIA_HIP_OK) die(g, "get_ma_dedup");
      if (mia_hip_ma_collapse(g, rec_of.data(), vote.data(), &collapsed.collapsed, nullptr) != MIA_HIP_OK) die(g, "ma_collapse");
      collapsed.seq.assign(m.seq.size() + 1, '\0');
      if (mia_hip_get_ma_collapse(g, &collapsed.seq[0], (int64_t)m.seq.size(), nullptr, collapsed.hist) != MIA_HIP_OK) die(g, "get_ma_collapse");
      apply_collapse(&m, in, collapsed, vote);
    }
    remove_records(&m, keep);
  }
  if (damage) {
    // the deaminated-fragment filter, behind -u and in front of everything else: the decision per molecule over all records (dropped
    // or not) on the device, then what is not kept leaves as for -u
    tally_file();
    std::vector<int64_t> mate;
    pair_halves(m, &mate);
    std::vector<uint8_t> keep(m.rec.size() + 1, 0);
    if (mia_hip_ma_damage(g, m.ref_seq.data(), nullptr, mate.data(), (int32_t)damage_n, single_stranded ? 1 : 0, ends_mode, nullptr, nullptr) != MIA_HIP_OK)
      die(g, "ma_damage");
    if (mia_hip_get_ma_damage(g, nullptr, nullptr, keep.data(), nullptr, nullptr) != MIA_HIP_OK) die(g, "get_ma_damage");
    keep.resize(m.rec.size());
    remove_records(&m, keep);
  }
  if (score) {
    // the damage score filter, behind -u and -D and in front of the mask: the score per molecule over all records (dropped or not) on
    // the device, then what stays below the threshold leaves as for -u
    tally_file();
    std::vector<int64_t> mate;
    pair_halves(m, &mate);
    std::vector<uint8_t> keep(m.rec.size() + 1, 0);
    if (mia_hip_ma_score(g, m.ref_seq.data(), nullptr, mate.data(), weights.data(), (int64_t)floor(score_nat * 65536.0 + 0.5), nullptr, nullptr) != MIA_HIP_OK)
      die(g, "ma_score");
    if (mia_hip_get_ma_score(g, nullptr, nullptr, keep.data(), nullptr, nullptr) != MIA_HIP_OK) die(g, "get_ma_score");
    keep.resize(m.rec.size());
    remove_records(&m, keep);
  }
  MaskResult masked;
  const int64_t mask_n_in = (int64_t)m.rec.size();
  if (mask) {
    // the end mask, behind -u and -D and in front of everything else: the new record view is made on the device from a tally of the
    // file as it stands, put back into the file here, and what is emptied leaves as for -u
    tally_file();
    const int64_t n_rec = (int64_t)m.start.size(), n_pairs = (int64_t)m.ins_record.size();
    int64_t cols_kept = 0;
    if (mia_hip_ma_mask(g, (int32_t)mask_n5, (int32_t)mask_n3, substitute ? mia::MA_MASK_N : mia::MA_MASK_TRIM, substitute && single_stranded ? 1 : 0, nullptr,
                        &cols_kept) != MIA_HIP_OK)
      die(g, "ma_mask");
    masked.first.resize((size_t)n_rec + 1); masked.count.resize((size_t)n_rec + 1); masked.start.resize((size_t)n_rec + 1);
    masked.col_off.resize((size_t)n_rec + 1); masked.pair_keep.resize((size_t)n_pairs + 1); masked.ins_pos.resize((size_t)n_pairs + 1);
    masked.seq.assign((size_t)cols_kept + 1, '\0'); masked.smp.assign((size_t)cols_kept + 1, '\0');
    if (mia_hip_get_ma_mask(g, masked.first.data(), masked.count.data(), masked.start.data(), masked.col_off.data(), &masked.seq[0], &masked.smp[0], cols_kept,
                            masked.pair_keep.data(), masked.ins_pos.data(), masked.hist, masked.scalars) != MIA_HIP_OK)
      die(g, "get_ma_mask");
    apply_mask(&m, masked, substitute);
  }
  if (out_format == 8 && !mia::ma_sam_gaps_ok(m.gaps.data(), m.L)) {
    fprintf(stderr, "ma_hip: %s has no SAM export: its GAPS line holds a negative value\n", ma_in_fn.c_str());
    exit(1);
  }
  if (out_format == 7 && !mia::ma_ace_gaps_ok(m.gaps.data(), m.L)) {
    fprintf(stderr, "ma_hip: %s has no ACE export: its GAPS line opens insert columns in front of column 0 or holds a negative value\n", ma_in_fn.c_str());
    exit(1);
  }
  // write_ma (src/map_assembler.c:214-217): after whatever report -f selected
  auto finish = [&](mia_hip_ctx* ctx) {
    mia_hip_destroy(ctx);
    if (out_ma) { fflush(stdout); if (!write_maln_file(ma_out_fn.c_str(), m, cons_scheme)) exit(1); }
    return 0;
  };

  tally_file();
  const int64_t n = (int64_t)m.start.size();
  const int L = m.L;
  if (out_format == 8) {
    int64_t n_rec = 0, body_bytes = 0;
    if (mia_hip_ma_sam(g, m.ref_seq.data(), &n_rec, &body_bytes) != MIA_HIP_OK) die(g, "ma_sam");
    if (n_rec != n) { fprintf(stderr, "ma_hip: the export holds %lld records, the file %lld\n", (long long)n_rec, (long long)n); exit(1); }
    std::vector<int32_t> nm((size_t)n_rec + 1);
    std::vector<int64_t> body_off((size_t)n_rec + 1);
    std::string body((size_t)body_bytes + 1, '\0');
    if (mia_hip_get_ma_sam(g, nm.data(), body_off.data(), &body[0], body_bytes) != MIA_HIP_OK) die(g, "get_ma_sam");
    sam_print(m, nm, body_off, body);
    return finish(g);
  }
  if (out_format == 9 || out_format == 91) {
    std::vector<uint8_t> use((size_t)n + 1, 1);
    for (int64_t r = 0; r < n; r++) use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
    int64_t n_used = 0, n_events = 0, bad_code = 0, beyond = 0;
    std::vector<int64_t> count((size_t)mia::MA_PROF_COUNTS), del((size_t)mia::MA_PROF_DEPTHS);
    if (mia_hip_ma_profile(g, m.ref_seq.data(), use.data(), &n_used, &n_events) != MIA_HIP_OK) die(g, "ma_profile");
    if (mia_hip_get_ma_profile(g, count.data(), del.data(), &bad_code, &beyond) != MIA_HIP_OK) die(g, "get_ma_profile");
    if (out_format == 9) profile_table(n_used, n_events, count.data(), del.data(), bad_code, beyond);
    else profile_matrix(count.data(), alpha);
    return finish(g);
  }
  if (out_format == 92 || out_format == 93) {
    std::vector<uint8_t> use((size_t)n + 1, 1), seg((size_t)n + 1, 'n');
    for (int64_t r = 0; r < n; r++) {
      use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
      seg[(size_t)r] = (uint8_t)m.rec[(size_t)r].segment;
    }
    int64_t n_used = 0, n5 = 0, n3 = 0, halves = 0;
    std::vector<int64_t> ctx_count((size_t)mia::MA_ENDS_CTX), len_count((size_t)2 * mia::MA_ENDS_LENS);
    if (mia_hip_ma_ends(g, m.ref_seq.data(), seg.data(), use.data(), &n_used, &n5, &n3) != MIA_HIP_OK) die(g, "ma_ends");
    if (mia_hip_get_ma_ends(g, ctx_count.data(), len_count.data(), &halves) != MIA_HIP_OK) die(g, "get_ma_ends");
    if (out_format == 92) ends_table(n_used, n5, n3, ctx_count.data());
    else lengths_table(len_count.data(), halves);
    return finish(g);
  }
  if (out_format == 96) {
    mask_report(stdout, mask_n_in, masked, substitute, substitute && single_stranded);
    fflush(stdout);
    return finish(g);
  }
  if (out_format == 98) {
    collapse_report(stdout, collapsed, tolerance);
    fflush(stdout);
    return finish(g);
  }
  if (out_format == 95) {
    std::vector<uint8_t> use((size_t)n + 1, 1);
    int64_t n_used = 0;
    for (int64_t r = 0; r < n; r++) n_used += use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
    std::vector<int64_t> mate, hist((size_t)mia::MA_DMG_HIST);
    pair_halves(m, &mate);
    int64_t n_molecules = 0, orphans = 0;
    if (mia_hip_ma_damage(g, m.ref_seq.data(), use.data(), mate.data(), mia::MA_DMG_MAX_POS, single_stranded ? 1 : 0, mia::MA_DMG_ANY, &n_molecules, nullptr) != MIA_HIP_OK)
      die(g, "ma_damage");
    if (mia_hip_get_ma_damage(g, nullptr, nullptr, nullptr, hist.data(), &orphans) != MIA_HIP_OK) die(g, "get_ma_damage");
    damage_table(n_molecules, orphans, n_used, single_stranded, hist.data());
    return finish(g);
  }
  if (out_format == 97) {
    std::vector<uint8_t> use((size_t)n + 1, 1);
    int64_t n_used = 0;
    for (int64_t r = 0; r < n; r++) n_used += use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
    std::vector<int64_t> mate, hist((size_t)mia::MA_PMD_HIST);
    pair_halves(m, &mate);
    int64_t n_molecules = 0, orphans = 0;
    if (mia_hip_ma_score(g, m.ref_seq.data(), use.data(), mate.data(), weights.data(), 0, &n_molecules, nullptr) != MIA_HIP_OK) die(g, "ma_score");
    if (mia_hip_get_ma_score(g, nullptr, nullptr, nullptr, hist.data(), &orphans) != MIA_HIP_OK) die(g, "get_ma_score");
    score_table(n_molecules, orphans, n_used, single_stranded, model, hist.data());
    return finish(g);
  }
  if (out_format == 42) {
    std::vector<uint8_t> use((size_t)n + 1, 1), seg((size_t)n + 1, 'n');
    for (int64_t r = 0; r < n; r++) {
      use[(size_t)r] = use_dropped || !m.rec[(size_t)r].dropped ? 1 : 0;
      seg[(size_t)r] = (uint8_t)m.rec[(size_t)r].segment;
    }
    int64_t n_used = 0, n_events = 0, beyond = 0, ends_outside = 0;
    std::vector<int32_t> cols((size_t)mia::MA_COLS_WORDS * (size_t)L);
    if (mia_hip_ma_cols(g, seg.data(), use.data(), &n_used, &n_events, &beyond, &ends_outside) != MIA_HIP_OK) die(g, "ma_cols");
    if (mia_hip_get_ma_cols(g, cols.data()) != MIA_HIP_OK) die(g, "get_ma_cols");
    int first = 0, last = L - 1;                       // every column, unless -R names a region (format 6's default does not apply)
    if (region_given) clamp_region(reg_start, reg_end, L, &first, &last);
    cols_table(m, n_used, n_events, beyond, ends_outside, cols.data(), first, last);
    return finish(g);
  }
  if (out_format == 5) {
    // fasta_print_cons of the called columns (src/io.c:929-951); '-' calls are not printed
    int64_t total_gaps = 0;
    for (int p = 0; p < L; p++) total_gaps += m.gaps[(size_t)p];
    std::string cons((size_t)L + (size_t)total_gaps + 16, '\0');
    int64_t clen = 0;
    if (mia_hip_consensus(g, cons_scheme, &cons[0], (int64_t)cons.size(), &clen) != MIA_HIP_OK) die(g, "consensus");
    printf(">%s\n", m.ref_id.c_str());
    int64_t i = 0;
    for (; i + FASTA_LINE_WIDTH <= clen; i += FASTA_LINE_WIDTH) { fwrite(&cons[(size_t)i], 1, FASTA_LINE_WIDTH, stdout); fputc('\n', stdout); }
    fwrite(&cons[(size_t)i], 1, (size_t)(clen - i), stdout);
    fputc('\n', stdout);
    return finish(g);
  }
  // the other formats: BaseCounts of every column from the device, calls and the double-valued columns here
  std::vector<int32_t> tally((size_t)MIA_HIP_TALLY_WORDS * (size_t)(L + 1)), dgaps((size_t)L + 1), ins_off((size_t)L + 1);
  {
    std::string scratch((size_t)L * 2 + (1 << 20), '\0');
    int64_t clen = 0;
    if (mia_hip_consensus(g, cons_scheme, &scratch[0], (int64_t)scratch.size(), &clen) != MIA_HIP_OK) die(g, "consensus");
  }
  if (mia_hip_get_tally(g, tally.data(), dgaps.data()) != MIA_HIP_OK) die(g, "get_tally");
  int64_t slots = 0;
  if (mia_hip_get_ins_tally(g, ins_off.data(), nullptr, 0, &slots) != MIA_HIP_OK) die(g, "get_ins_tally");
  std::vector<int32_t> ins_tally((size_t)slots * 9 + 9);
  if (slots > 0 && mia_hip_get_ins_tally(g, nullptr, ins_tally.data(), slots, nullptr) != MIA_HIP_OK) die(g, "get_ins_tally");
  const size_t Lp = (size_t)L + 1;
  auto word = [&](int w, int p) { return tally[(size_t)w * Lp + (size_t)p]; };
  if (out_format != 4 && out_format != 41) {
    // consensus, gapped reference and coverage of columns first .. last as show_consensus (formats 1, 2: the whole reference, no
    // insert columns in front of column 0) and print_region (formats 6, 61: those too) build them
    const bool region = out_format == 6 || out_format == 61;
    int first = 0, last = L - 1;
    if (region) clamp_region(reg_start, reg_end, L, &first, &last);
    std::string cons, aln_ref;
    std::vector<int> cov;
    for (int p = first; p <= last; p++) {
      const int gp = m.gaps[(size_t)p] > 0 ? m.gaps[(size_t)p] : 0;
      if (gp > 0 && (p > 0 || region)) {              // find_ins_cons (src/map_align.c:444-510); no record spans column 0
        const int span = p > 0 ? word(10 /* T_SPAN */, p) : 0;
        for (int j = 0; j < gp; j++) {
          static const int32_t none[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
          const int32_t* t = p > 0 ? &ins_tally[(size_t)(ins_off[(size_t)p] + j) * 9] : none;
          Counts b{t[0], t[1], t[2], t[3], span - t[4], span, t[5], t[6], t[7], t[8]};
          double frac = 0.0;
          cons += find_consensus(b, cons_scheme, &frac);
          aln_ref += '-';
          cov.push_back(span);
        }
      }
      Counts b{word(0, p), word(1, p), word(2, p), word(3, p), word(4, p), word(5, p), word(6, p), word(7, p), word(8, p), word(9, p)};
      double frac = 0.0;
      cons += find_consensus(b, cons_scheme, &frac);
      aln_ref += m.ref_seq[(size_t)p];
      cov.push_back(b.cov);
    }
    if (out_format == 7) {
      // ace_output, src/io.c:756-913: cons is get_consensus' string; the padded reads of all records come from the device
      int64_t n_rec = 0, body_bytes = 0;
      if (mia_hip_ma_ace(g, &n_rec, &body_bytes) != MIA_HIP_OK) die(g, "ma_ace");
      std::vector<int64_t> af_pos((size_t)n_rec + 1), padded_len((size_t)n_rec + 1), body_off((size_t)n_rec + 1);
      std::string body((size_t)body_bytes + 1, '\0');
      if (mia_hip_get_ma_ace(g, af_pos.data(), padded_len.data(), body_off.data(), &body[0], body_bytes) != MIA_HIP_OK) die(g, "get_ma_ace");
      if (n_rec != n) { fprintf(stderr, "ma_hip: the export holds %lld records, the file %lld\n", (long long)n_rec, (long long)n); exit(1); }
      ace_print(m, cons, af_pos, padded_len, body_off, body);
    } else if (out_format == 1) clustalw_print_cons(cons, aln_ref, m.ref_id);
    else if (out_format == 2) {                       // line_print_cons, src/io.c:1032-1042
      printf("Consensus, %s, coverage:\n%s\n%s\n", m.ref_id.c_str(), cons.c_str(), aln_ref.c_str());
      for (int c : cov) printf("%d ", c);
      printf("\n");
    } else {
      // print_region, src/map_align.c:635-750: the rows of the overlapping records come from the device
      int64_t n_rows = 0, width = 0;
      if (mia_hip_ma_region(g, first, last, &n_rows, &width) != MIA_HIP_OK) die(g, "ma_region");
      if (width != (int64_t)aln_ref.size()) { fprintf(stderr, "ma_hip: the region's rows are %lld wide, its reference line %zu\n", (long long)width, aln_ref.size()); exit(1); }
      std::vector<int64_t> rows((size_t)n_rows + 1);
      std::string text((size_t)(n_rows * width) + 1, '\0');
      if (mia_hip_get_ma_region(g, rows.data(), &text[0], n_rows) != MIA_HIP_OK) die(g, "get_ma_region");
      if (out_format == 61) {
        fasta_aln_print(aln_ref.data(), aln_ref.size(), m.ref_id);
        fasta_aln_print(cons.data(), cons.size(), "Consensus");
      } else if (in_color) {
        printf("%-20.20s ", m.ref_id.c_str());
        color_print(aln_ref.data(), aln_ref.size());
        printf("%-20.20s ", "Consensus");
        color_print(cons.data(), cons.size());
      } else {
        printf("%-20.20s %s\n%-20s %s\n", m.ref_id.c_str(), aln_ref.c_str(), "Consensus", cons.c_str());
      }
      for (int64_t i = 0; i < n_rows; i++) {
        const std::string label = region_label(m.rec[(size_t)rows[(size_t)i]]);
        const char* row = text.data() + (size_t)(i * width);
        if (out_format == 61) fasta_aln_print(row, (size_t)width, label);
        else {
          printf("%-20.20s ", label.c_str());
          if (in_color) color_print(row, (size_t)width);
          else { fwrite(row, 1, (size_t)width, stdout); fputc('\n', stdout); }
        }
      }
    }
    return finish(g);
  }
  for (int p = 0; p < L; p++) {
    if (m.gaps[(size_t)p] > 0 && p > 0) {           // find_ins_cons (src/map_align.c:444-510)
      const int span = word(10 /* T_SPAN */, p);
      for (int j = 0; j < m.gaps[(size_t)p]; j++) {
        const int32_t* t = &ins_tally[(size_t)(ins_off[(size_t)p] + j) * 9];
        Counts b{t[0], t[1], t[2], t[3], span - t[4], span, t[5], t[6], t[7], t[8]};
        double frac = 0.0;
        const char cb = find_consensus(b, cons_scheme, &frac);
        if (out_format == 41 || cb != '-') show_single_pos(p, '-', cb, b, frac);
      }
    }
    Counts b{word(0, p), word(1, p), word(2, p), word(3, p), word(4, p), word(5, p), word(6, p), word(7, p), word(8, p), word(9, p)};
    double frac = 0.0;
    const char cb = find_consensus(b, cons_scheme, &frac);
    if (out_format == 41 || m.ref_seq[(size_t)p] != cb) show_single_pos(p, m.ref_seq[(size_t)p], cb, b, frac);
  }
  return finish(g);
}
