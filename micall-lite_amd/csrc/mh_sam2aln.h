// mh_sam2aln.h -- state of the sam2aln stage shared by its host half
// (mh_s2a_host.cpp: remap.csv parse, matchmaker, CSV output) and its device
// half (mh_sam2aln.hip: merge, grouping).  See mh_sam2aln.hip for the map
// onto micall/core/sam2aln.py.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "mh_gunzip.h"
#include "mh_internal.h"

namespace mh {

enum { S2A_OK = 0, S2A_UNMATCHED = 1, S2A_BADCIGAR = 2, S2A_2REFS = 3, S2A_MANYNS = 4,
       S2A_EMPTY = 5 };

// apply_cigar's verdict on a row's CIGAR (sam2aln.py:113-151)
enum { CIG_OK = 0, CIG_STAR = 1, CIG_INVALID = 2, CIG_UNSUPPORTED = 3, CIG_LONG = 4,
       CIG_SHORT = 5 };

constexpr int S2A_MAX_CUTS = 8;  // q-cutoffs of one call (SAM2ALN_Q_CUTOFFS, sam2aln.py:25)

// k_s2a_merge's launch (s2a_run; reported by mh_test_sam2aln_info).  A wave
// keeps both mates in reference coordinates in LDS: wave_bytes =
// S2A_SPAN_BYTES * span_cap + S2A_OP_BYTES * (ops_cap + 1), rounded up to 16
constexpr size_t S2A_LDS_BYTES = 160 * 1024;   // dynamic LDS of one block at most
constexpr int64_t S2A_BLOCK_CAP = 256 * 64;    // blocks of one launch at most
constexpr int S2A_WPB = 4;                     // waves per block while they fit in S2A_LDS_BYTES
constexpr uint64_t S2A_MIN_TABLE = 1024;       // slots of the grouping table at least
constexpr int S2A_SPAN_BYTES = 4;              // c0 q0 c1 q1: a byte each per reference position
constexpr int S2A_OP_BYTES = 16;               // reference and read offset (int32) per op and mate

struct S2AShard;                 // sam2aln split over the ranks of a job (mh_s2a_shard.cpp)
void s2a_shard_free(S2AShard *sh);

// aligned.csv's data rows in file order (s2a_order): the printed groups, one
// per (rname, q-cutoff) that has rows, and per row its index into uniq
struct S2AOrder {
    bool valid = false;
    std::vector<int32_t> g_name, g_qcut;   // per group: index into names, the cutoff
    std::vector<int64_t> g_first;          // per group (+ end): its first row
    std::vector<uint64_t> g_total;         // per group: the sum of its rows' counts
    std::vector<int32_t> rows;             // per row: k of uniq[2k], uniq[2k + 1]
};

// The row arrays the device half reads.  dev: they are on the device already
// (k_s2a_stage wrote them) and span[r] is row r's reference span; without it
// they are uploaded from S and the spans come from S.cig
struct S2ADevRows {
    const uint8_t *seq, *qual;
    const int64_t *soff;
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int32_t *span;                // host: S2AState::d_spanins per row
};

// soft-clip counts of the last call (mh_sam2aln_clipping), counted on the
// first request from the rows and units the merge left on the device
enum { CLIP_NONE = 0, CLIP_ROWS = 1, CLIP_DONE = 2 };
constexpr int64_t S2A_CLIP_MAX_WINDOW = (int64_t)1 << 26;   // positions of one reference

struct S2AClip {
    int state = CLIP_NONE;              // CLIP_ROWS: s2a_run's arrays stand, nothing counted yet
    S2ADevRows rows{};                  // what s2a_run's kernels read
    std::vector<int32_t> name;          // per (reference, position) with a count > 0, by
    std::vector<int64_t> pos;           //   (name as Python sorts str, pos): index into
    std::vector<int32_t> count;         //   S2AState::names, 1-based position, units
    std::string text;                   // clipping.csv, formatted on first use
    bool text_valid = false;
    int64_t *d_lo = nullptr, *d_base = nullptr;              // per reference: window start, offset in d_diff
    int32_t *d_wlen = nullptr, *d_diff = nullptr, *d_idx = nullptr, *d_cnt = nullptr,
            *d_n = nullptr;                                  // d_n: pairs per reference, then the error flag
};

// mate concordance of the last call (mh_sam2aln_concordance), counted on the
// first request from the same rows and units: per consensus position the
// paired units whose mates both align it and how they disagree there, and per
// (read, cycle) and (read, quality) the bases compared and found different
enum { CONC_OVERLAP = 0, CONC_MISMATCH = 1, CONC_INDEL = 2, CONC_NOCALL = 3, CONC_UNRESOLVED = 4,
       CONC_PLANES = 5 };

struct S2AConc {
    bool done = false;
    std::vector<int32_t> name;          // per (reference, position) with overlap > 0, by (name as
    std::vector<int64_t> pos;           //   Python sorts str, pos): index into S2AState::names, position
    std::vector<int32_t> count;         // CONC_PLANES per row
    std::vector<int64_t> reads;         // per key with compared > 0, in file order: read, by (0 cycle,
                                        //   1 quality), value, compared, mismatch
    std::string text[2];                // concordance.csv, cycle_concordance.csv, formatted on first use
    bool text_valid[2] = {false, false};
    int64_t *d_lo = nullptr, *d_base = nullptr;              // per reference: window start, offset in a plane
    int32_t *d_wlen = nullptr, *d_acc = nullptr, *d_idx = nullptr, *d_cnt = nullptr,
            *d_n = nullptr;                                  // d_n: rows per reference, then the error flag
    uint8_t *d_orient = nullptr;                             // per merge unit: k_s2a_conc's orientation bits
    unsigned long long *d_rd = nullptr;                      // the per-read sums (64-bit)
};

// strand support of the last call (mh_sam2aln_strand), counted on the first
// request from the same rows, units and merge results: per (reference,
// q-cutoff, position) and merged character (A, C, G, T, '-') the units with a
// supporting mate on the forward strand, on the reverse strand, and on both
constexpr int STRAND_KEYS = 15;                              // character * 3 + (0 fwd only, 1 rev only, 2 both)
constexpr int64_t S2A_STRAND_MAX_BYTES = (int64_t)1 << 30;   // the class planes in HBM at most

struct S2AStrand {
    bool done = false;
    std::vector<int32_t> name, qcut;    // per row, by (name as Python sorts str, the call's cutoff order,
    std::vector<int64_t> pos;           //   pos): index into S2AState::names, the cutoff, 1-based position
    std::vector<int32_t> count;         // STRAND_KEYS per row: A_fwd, A_rev, A_both, C_fwd, ... del_both
    std::string text;                   // strand.csv, formatted on first use
    bool text_valid = false;
    int64_t *d_lo = nullptr, *d_base = nullptr;              // per reference: window start, offset in a plane
    int32_t *d_wlen = nullptr, *d_acc = nullptr, *d_idx = nullptr, *d_cnt = nullptr,
            *d_n = nullptr;                                  // d_n: rows per (cutoff, reference), then the error flag
    uint8_t *d_orient = nullptr;                             // per merge unit: bit 0 row1 reversed, bit 1 row2
};

// merged insertions of the last call (mh_sam2aln_conseq_ins), counted on the
// first request from the same rows and units.  One record per (listed unit,
// consensus key); one entry per (record, q-cutoff): entry = record * n_cut + k
struct S2AInsRec {
    int32_t unit, key;                  // merge unit; 0-based consensus coordinate the insertion precedes
    int32_t len1, len2;                 // inserted bytes of mate 1 and mate 2 (0: none); both 0: unused record
    int64_t src1, src2;                 // their first byte in seq / qual
    int64_t boff;                       // the record's first merged byte, per cutoff
};

struct S2AIns {
    bool done = false;
    // conseq_ins.csv's rows in file order
    std::vector<int32_t> name, cut, count;   // index into S2AState::names, index into q_cutoffs, units
    std::vector<int64_t> pos, soff;          // the key; the string's place in strings (+ end)
    std::string strings;
    // per (name, cutoff, key) the sum over strings, in the same order
    std::vector<int32_t> t_name, t_cut, t_count;
    std::vector<int64_t> t_pos;
    std::string text;                   // conseq_ins.csv, formatted on first use
    bool text_valid = false;
    int32_t *d_list = nullptr, *d_res = nullptr, *d_rref = nullptr, *d_tcnt = nullptr, *d_trep = nullptr,
            *d_uniq = nullptr, *d_ctr = nullptr;
    int64_t *d_recoff = nullptr, *d_byteoff = nullptr, *d_slot = nullptr, *d_goff = nullptr;
    S2AInsRec *d_rec = nullptr;
    uint64_t *d_h = nullptr, *d_tkey = nullptr;
    uint8_t *d_out = nullptr, *d_gather = nullptr;
};

struct S2AState {
    // ---- rows of the last remap.csv (host) ----
    int64_t n_rows = 0;
    TextBuf qpool;                      // qnames back to back (not zero-filled)
    std::vector<int64_t> qoff;
    std::vector<int32_t> qlen;
    TextBuf cpool;                      // CIGAR texts (for error messages)
    std::vector<int64_t> coff;
    std::vector<int32_t> clen;
    std::vector<int8_t> cstate;         // CIG_*
    std::vector<int32_t> rid;           // rname id into rnames
    std::vector<std::string> rnames;
    std::vector<int32_t> flag, pos;     // pos INT32_MIN: not an integer
    std::vector<uint8_t> qshort;        // qual shorter than seq
    TextBuf seq, qual;                  // concatenated, qual padded to seq length
    std::vector<int64_t> soff;
    std::vector<int32_t> slen;
    std::vector<int32_t> cig_off, n_cig;
    std::vector<uint32_t> cig;          // (len << 4) | op of usable CIGARs
    // ---- units in matchmaker order ----
    std::vector<int64_t> u1, u2;        // rows; u2 = -1 for None
    std::vector<int8_t> ucause;         // host-decided cause, -1 = merged on the device
    std::vector<int8_t> upaired;        // is_paired of row1
    std::vector<int64_t> merge_of_unit; // index into the device merge list, -1 if none
    std::vector<int32_t> name_id;       // per unit: index into names
    std::vector<std::string> names;     // rnames in first-seen order over units
    // q-cutoffs of the call, distinct, in the caller's order (sam2aln.py:391).
    // One merge entry per (merge unit m, cutoff k): entry = m * n_cut + k
    std::vector<int32_t> q_cutoffs{15};
    // ---- device ----
    uint8_t *d_seq = nullptr, *d_qual = nullptr, *d_out = nullptr, *d_gather = nullptr;
    int64_t *d_soff = nullptr, *d_units = nullptr, *d_slot = nullptr, *d_goff = nullptr;
    int32_t *d_pos = nullptr, *d_cigoff = nullptr, *d_ncig = nullptr, *d_uref = nullptr,
            *d_res = nullptr, *d_tcnt = nullptr, *d_trep = nullptr, *d_uniq = nullptr,
            *d_ctr = nullptr;
    uint32_t *d_cig = nullptr;
    uint64_t *d_h = nullptr, *d_tkey = nullptr;
    // per read, written by k_s2a_stage (mh_sam2aln_resident): FLAG, the
    // index of RNAME (-1: '*') and reference span << 2 | reversed << 1 | has an I op
    // (-1: unmapped)
    int32_t *d_flag = nullptr, *d_samref = nullptr, *d_spanins = nullptr;
    int64_t staged_reads = -1;          // reads whose SEQ / QUAL d_seq / d_qual hold as staged; -1 none
    std::unordered_map<const void *, size_t> dcap;   // bytes allocated behind each device pointer (grow-only)
    // ---- results of the device pass ----
    int64_t n_merge = 0, n_unique = 0;
    std::vector<int32_t> res;           // per entry: status, offset, body_len, strip_len
    std::vector<int32_t> uniq;          // rep entry, count
    std::vector<int64_t> uniq_off;      // offsets into gathered
    TextBuf gathered;                   // bodies of the distinct sequences (not zero-filled)
    // ---- formatted outputs (cached between the size query and the copy) ----
    std::vector<std::string> out_cache[3];   // the text as pieces, in order
    int out_valid = 0;
    S2AOrder order;                     // aligned.csv's row order, built on first use
    // true from the end of a whole (un-sharded) call that succeeded until
    // the next call starts: the device arrays then hold what the host ones do
    bool complete = false;
    // crc32 and size of aligned.csv as mh_sam2aln_write last wrote it (-1: not written)
    uint32_t wr_crc = 0;
    int64_t wr_bytes = -1;
    // ---- host timings of the last call (ms) ----
    double t_parse = 0, t_device = 0, t_format[3] = {0, 0, 0};
    S2AClip clip;
    S2AIns ins;
    S2AConc conc;
    S2AStrand strand;
    // shape of the last k_s2a_merge launch, kept for mh_test_sam2aln_info
    // (host bookkeeping; nothing reads it otherwise).  wpb and blocks stay 0
    // when the call was refused before the launch
    struct Info {
        int span_cap = 0, ops_cap = 0, wave_bytes = 0, wpb = 0, n_cut = 0;
        int64_t blocks = 0, n_merge = 0, tsize = 0;
    } info;
    // ---- this rank's part of a sharded sam2aln ----
    S2AShard *shard = nullptr;
    ~S2AState() { if (shard) s2a_shard_free(shard); }
};

// failed.csv's manyNs of merge unit m: any of its entries failed the prop_N
// test (parse_sam keeps one failure cause per pair, sam2aln.py:381-389)
inline bool s2a_many_ns(const S2AState &S, int64_t m)
{
    const int64_t nc = (int64_t)S.q_cutoffs.size();
    for (int64_t e = m * nc; e < (m + 1) * nc; ++e)
        if (S.res[4 * e] == S2A_MANYNS) return true;
    return false;
}

// Every call that rebuilds S starts here: a new serial (mh_sam2aln_serial),
// nothing of the last call's results stands any more.
inline void s2a_begin(Ctx &c, S2AState &S)
{
    ++c.s2a_serial;
    S.complete = false;
    S.order = S2AOrder();
    S.wr_bytes = -1;
    S.n_merge = S.n_unique = 0;
    S.res.clear();
    S.clip.state = CLIP_NONE;
    S.clip.text_valid = false;
    S.ins.done = S.ins.text_valid = false;
    S.conc.done = S.conc.text_valid[0] = S.conc.text_valid[1] = false;
    S.strand.done = S.strand.text_valid = false;
    for (auto &o : S.out_cache) std::vector<std::string>().swap(o);
    S.out_valid = 0;
}

// host half: the header row of text, then its records (body_lo >= 0: only
// the records in bytes [body_lo, body_hi) of text, both record boundaries)
int s2a_parse(S2AState &S, const char *text, int64_t len, int64_t body_lo = -1, int64_t body_hi = -1);
// insert.csv (which 1) or failed.csv (2) rows of units [u0, u1)
int s2a_format_units(const S2AState &S, int which, int64_t u0, int64_t u1, bool head_row,
                     std::vector<std::string> &out);
// aligned.csv's row order into S.order (kept until the next call rebuilds S):
// the formatter and mh_a2c_load_resident both read the rows from it
void s2a_order(S2AState &S);
int s2a_format(S2AState &S, int which, std::vector<std::string> &out);
// the same text written to fd from offset while it is formatted; 0 or errno.
// crc (may be null): the crc32 of the bytes written, from the pieces' own
int s2a_format_write(S2AState &S, int which, int fd, int64_t offset, int64_t *written,
                     uint32_t *crc = nullptr);
// device half (S2ADevRows above)
int s2a_run(Ctx &c, S2AState &S, double max_prop_n, const S2ADevRows *dev = nullptr);
// k_s2a_clip and k_s2a_clip_scan over the units of the last s2a_run, once per
// call: S.clip's (name, pos, count) lists
int s2a_clip_run(Ctx &c, S2AState &S);
// k_s2a_ins_rec, k_s2a_ins_merge and the grouping over the units of the last
// s2a_run that hold an I op, once per call: S.ins's rows and totals
int s2a_ins_run(Ctx &c, S2AState &S);
// k_s2a_conc and k_s2a_conc_scan over the paired units of the last s2a_run,
// once per call: S.conc's position rows and read table
int s2a_conc_run(Ctx &c, S2AState &S);
// k_s2a_strand and k_s2a_strand_scan over the units of the last s2a_run whose
// merge entries are S2A_OK, once per call: S.strand's rows
int s2a_strand_run(Ctx &c, S2AState &S);
// Units, failure causes, group names and QNAMEs of the resident rows (one
// per read, in read order) instead of s2a_parse: S.pos, S.flag, S.n_cig,
// S.cig_off and S.cig hold the rows as k_s2a_stage wrote them; sam_ref[r]
// indexes refnames (-1: '*'), span_ins[r] as S2ADevRows::span.  1 when the
// rows cannot stand for matchmaker's pairing of the file (mates with two
// QNAMEs, an unpaired QNAME that may repeat): the caller parses the file.
int s2a_units_resident(Ctx &c, S2AState &S, int n_refs, const char *const *refnames,
                       const std::vector<int32_t> &sam_ref, const std::vector<int32_t> &span_ins);

}  // namespace mh
