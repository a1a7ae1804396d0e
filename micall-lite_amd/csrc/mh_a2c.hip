// mh_a2c.hip -- the per-read half of aln2counts (micall/core/aln2counts.py)
// on gfx950, over the rows of aligned.csv (sam2aln's distinct merged reads
// with their counts) resident in HBM.
//
//   k_a2c_count   SequenceReport._count_reads (:115-172) with
//                 SeedAmino.count_aminos / SeedNucleotide.count_nucleotides
//                 (:595-606, :636-645).  Work unit: a chunk of <= 1024 rows of
//                 one bin; a bin is 21 consecutive codons of one (refname,
//                 qcut) group.  A wave takes a row, lane 21 f + c codon c of
//                 the bin in reading frame f (63 lanes: the three frames read
//                 the same bytes in one load instruction, so every row is
//                 fetched once per bin, not once per frame): the three
//                 characters of the frame- and
//                 offset-padded read ('-' outside it, :155-157), the amino
//                 acid from the codon table, then LDS counters per (codon,
//                 amino acid) and per (codon, position, base): a count and
//                 the first row that touched it.  The first row is the
//                 Counter insertion order that most_common() breaks ties by
//                 (:624, :668).  One global atomic per touched counter
//                 flushes the chunk.
//   k_a2c_detail  the codons k_a2c_count drops because they translate to no
//                 amino acid, sorted into X / partial / del over the same
//                 chunks and lanes; run only when mh_a2c_codon_detail asks
//                 (amino_detail.csv; the rule: tests/amino_detail_oracle.py).
//   k_a2c_stage, k_a2c_bin_count / _scan / _fill
//                 the rows and the bin lists built on the device from the
//                 results sam2aln left there (mh_a2c_load_resident): what the
//                 host half below builds from the text of aligned.csv.
//   k_a2c_ins_*   the read loop of InsertionWriter.write (:786-795): per
//                 (insert range, row) the framed slice [3 left, 3 right) of
//                 the read, rejected when it starts in the padding, holds '-'
//                 or 'n' or no whole codon, and translated (k_a2c_ins_hash:
//                 a key per pair); every member of a group of equal strings
//                 is compared with the group's first row (k_a2c_ins_verify:
//                 a collision is an error, never a merge) and the distinct
//                 strings are gathered for the host (k_a2c_ins_gather).
//   k_a2c_var_*   the nucleotide variants of the coordinate regions (the loop
//                 of :346-375, the report of :537-549): per (region, row) the
//                 padded row clipped to the region's window, hashed, verified
//                 and gathered a wavefront per pair, and each region's
//                 greatest by (count, sequence) picked on the device (see
//                 the section at the end of this file).
//   k_a2c_tab_count, k_a2c_tab_compact
//                 the grouping both of them share (A2CTable): the keyed
//                 pairs of a call in an open-addressing table, per distinct
//                 key the summed count and the first row, then the occupied
//                 slots as entries.  a2c_group_strings is its host side.
//   k_a2c_link, k_a2c_link_compact
//                 linked amino acids (mh_a2c_link, the section at the end of
//                 this file): per (set of codons, row) the row's codon classes
//                 at the set's codons as one exact key, grouped by
//                 k_a2c_tab_count.
//   k_a2c_gram_bits, k_a2c_gram_pairs
//                 pairwise covariation (mh_a2c_gram, the last section of this
//                 file): per column of the call one bit per row, "the row's
//                 codon class here is in the column's mask", then the weighted
//                 Gram matrix of the bit columns by popcount over the planes
//                 of the row counts.
// Host half (below the kernels): aligned.csv as csv.DictReader reads it,
// consecutive (refname, qcut) groups (itertools.groupby, :884-887), the
// codon extent of every frame, the bin lists.
// Bit-for-bit specification: oracle/og_aln2counts.py.
#include <algorithm>
#include <atomic>
#include <charconv>
#include <chrono>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "mh_gunzip.h"
#include "mh_internal.h"
#include "mh_sam2aln.h"
#include "mh_text.h"

namespace mh {

constexpr int A2C_W = 21;                       // codons per bin (x 3 frames = 63 lanes)
constexpr int A2C_LANES = 3 * A2C_W;
constexpr int A2C_CHUNK = 1024;                 // rows per workgroup
constexpr int A2C_NAA = 21;                     // AMINO_ALPHABET
constexpr int A2C_STRIDE = A2C_NAA + 18;        // per codon: 21 amino acids, 3 x 6 bases
constexpr int A2C_CELLS = A2C_LANES * A2C_STRIDE;   // counters per bin (3 frames)
constexpr int A2C_SLOTS = 4;
constexpr uint32_t A2C_NONE = 0xffffffffu;
constexpr int64_t A2C_MAX_SPAN = 1 << 28;
// Read characters: A C G T N - are classes 0-5; 'n' (the gap between the
// mates: no base, an 'N' to translate, :642-645) is 6; anything else is 7.
enum { A2C_DASH = 5, A2C_GAP = 6, A2C_BAD = 7 };
static const char A2C_CODES[] = "ACDEFGHIKLMNPQRSTVWY*?-";   // amino-acid codes 0..22
__constant__ char c_a2c_codes[24] = "ACDEFGHIKLMNPQRSTVWY*?-";

struct A2CRow {
    int64_t soff;      // first seq byte in the uploaded text
    int32_t len;       // seq length
    int32_t off;       // offset column
    uint32_t cnt;      // count column
    uint32_t local;    // row index within its group
};

struct A2CChunk {
    int32_t bin, codon0;
    int64_t beg, end;  // slice of bin_rows
};

// One distinct string of a class: an amino-acid string of an insert range
// (mh_a2c_inserts), a clipped sequence of a coordinate region
// (mh_a2c_variants).
struct A2CDistinct {
    int32_t cls;       // the range; the index among the call's regions with a cut above 0
    uint32_t first;    // first row that produced it: on the device its index among the
                       // call's rows, in A2CState::entries its number within the group
    int32_t len;       // codons of the amino-acid string; bytes of the clipped sequence
    int32_t pad;
    unsigned long long count;
};

struct A2CState {
    // host
    int64_t n_rows = 0, n_bins = 0;
    std::vector<A2CRow> rows;
    std::vector<int64_t> g_first;             // n_groups + 1
    std::vector<std::string> g_ref, g_qcut;
    std::vector<int32_t> g_ncod;              // 3 per group
    std::vector<int64_t> g_bin0;              // n_groups + 1
    std::vector<uint32_t> h_cnt, h_first;     // [bin][frame * 21 + codon][39]
    int8_t code[512];
    uint8_t cls[256];
    std::string pool;                         // row text when it is not the caller's CSV
    // device
    uint8_t *d_text = nullptr, *d_cls = nullptr;
    int8_t *d_code = nullptr;
    A2CRow *d_rows = nullptr;
    int32_t *d_bin_rows = nullptr;
    A2CChunk *d_chunks = nullptr;
    uint32_t *d_cnt = nullptr, *d_first = nullptr;
    // mh_a2c_codon_detail: the chunks of the last load that counted, and the
    // X / partial / del counters k_a2c_detail makes of them on the first request
    size_t n_chunks = 0;
    bool counted = false, det_ready = false;
    uint32_t *d_det = nullptr;
    std::vector<uint32_t> h_det;              // [bin][frame * 21 + codon][3]
    // mh_a2c_load_resident: the rows were built on the device (rows is
    // empty; every group's first row has local 0) from these uploads
    bool dev_rows = false;
    int32_t *d_order = nullptr, *d_gfirst = nullptr, *d_gbin0 = nullptr, *d_ncod = nullptr;
    unsigned long long *d_bstart = nullptr, *d_bcur = nullptr;
    // insertion strings of the last mh_a2c_inserts, in (range, first row) order
    std::vector<A2CDistinct> entries;
    std::string aminos;                       // one line per entry
    std::string ins_rows;                     // mh_a2c_insert_rows text (size query, then copy)
    std::unordered_map<const void *, size_t> dcap;   // bytes behind each device pointer (grow-only)
    // kept variants of the last mh_a2c_variants, in report order
    std::vector<A2CDistinct> var_entries;
    std::vector<int32_t> var_region;          // the caller's region index of each
    std::string var_text;                     // their clipped sequences, back to back
    int64_t var_stats[4] = {0, 0, 0, 0};      // pairs kept, entries, tied at a cut, text bytes fetched
    double t_var = 0;
    // entries of the last mh_a2c_link, in report order
    std::vector<int32_t> link_set;            // the caller's set index of each
    std::vector<int64_t> link_count;
    std::string link_text;                    // one haplotype per line
    std::vector<int64_t> link_cov;            // per set of the call
    int64_t link_stats[3] = {0, 0, 0};        // pairs that counted, distinct entries, entries fetched
    double t_link = 0;
    // figures of the last mh_a2c_gram: rows, row words, count planes, distinct (frame, codon), tiles
    int64_t gram_stats[5] = {0, 0, 0, 0, 0};
    double t_gram = 0;
    double t_parse = 0, t_count = 0, t_ins = 0;
    // a part of aligned.csv held between mh_a2c_part_open and _count (mapped)
    const char *part_text = nullptr;          // (null for an empty file)
    size_t part_len = 0;
    bool part_open = false;                   // mh_a2c_part_open done, not counted yet
    int64_t part_b0 = 0, part_b1 = 0;         // the part's bytes of the text
    std::vector<int64_t> part_first;          // local groups' first rows (+ end)
};

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
struct A2CCountArgs {
    const uint8_t *text;
    const A2CRow *rows;
    const int32_t *bin_rows;
    const A2CChunk *chunks;
    const int8_t *code;   // 512: codon of classes (c0, c1, c2) at 64 c0 + 8 c1 + c2
    const uint8_t *cls;   // 256
    uint32_t *cnt, *first;
};

__global__ __launch_bounds__(256) void k_a2c_count(A2CCountArgs A)
{
    __shared__ uint32_t s_cnt[A2C_CELLS], s_first[A2C_CELLS];
    __shared__ int8_t s_code[512];
    __shared__ uint8_t s_cls[256];
    const A2CChunk ch = A.chunks[blockIdx.x];
    for (int i = threadIdx.x; i < A2C_CELLS; i += 256) {
        s_cnt[i] = 0;
        s_first[i] = A2C_NONE;
    }
    s_code[threadIdx.x] = A.code[threadIdx.x];
    s_code[threadIdx.x + 256] = A.code[threadIdx.x + 256];
    s_cls[threadIdx.x] = A.cls[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int f = lane / A2C_W;                  // this lane's frame and codon
    const int j = ch.codon0 + lane - A2C_W * f;
    // lane stride 39 words: odd, so the lanes of a wave hit distinct banks
    uint32_t *cc = s_cnt + lane * A2C_STRIDE, *cf = s_first + lane * A2C_STRIDE;
    for (int64_t i = ch.beg + (threadIdx.x >> 6); i < ch.end; i += 4) {
        if (lane >= A2C_LANES) continue;
        const A2CRow R = A.rows[A.bin_rows[i]];
        // codons offset // 3 .. ceil((frame + offset + len) / 3) - 1 (:155-160)
        if (j < R.off / 3 || j >= (f + R.off + R.len + 2) / 3) continue;
        const int q0 = 3 * j - f - R.off;
        const uint8_t *s = A.text + R.soff;
        int c[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int q = q0 + t;
            c[t] = (q >= 0 && q < R.len) ? s_cls[s[q]] : A2C_DASH;
        }
        const int a = s_code[64 * c[0] + 8 * c[1] + c[2]];
        if (a < A2C_NAA) {
            atomicAdd(&cc[a], R.cnt);
            atomicMin(&cf[a], R.local);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (c[t] < A2C_GAP) {
                const int k = A2C_NAA + 6 * t + c[t];
                atomicAdd(&cc[k], R.cnt);
                atomicMin(&cf[k], R.local);
            }
    }
    __syncthreads();
    const size_t base = (size_t)ch.bin * A2C_CELLS;
    for (int i = threadIdx.x; i < A2C_CELLS; i += 256) {
        const uint32_t fr = s_first[i];
        if (fr == A2C_NONE) continue;
        if (s_cnt[i]) atomicAdd(&A.cnt[base + i], s_cnt[i]);
        atomicMin(&A.first[base + i], fr);
    }
}

// ---- the codons k_a2c_count leaves out (amino_detail.csv) -----------------
// A codon whose translation is not one of the 21 letters is counted nowhere
// by k_a2c_count.  k_a2c_detail walks the same chunks with the same lanes and
// sorts those codons: all three characters '-' of the read itself (not the
// padding around it) is a deletion; no base at all (padding, the gap between
// the mates) is nothing; a '-' or 'n' beside a base is a partial codon; three
// of A C G T N are an ambiguous one.  Per lane three LDS counters (stride 3:
// odd, distinct banks), no first row; one global atomic per non-zero counter
// flushes the chunk.
constexpr int A2C_DET = 3;                              // X, partial, del
constexpr int A2C_DET_CELLS = A2C_LANES * A2C_DET;      // counters per bin (3 frames)
enum { A2C_DET_X = 0, A2C_DET_PARTIAL = 1, A2C_DET_DEL = 2 };

struct A2CDetailArgs {
    const uint8_t *text;
    const A2CRow *rows;
    const int32_t *bin_rows;
    const A2CChunk *chunks;
    const int8_t *code;
    const uint8_t *cls;
    uint32_t *det;        // [bin][frame * 21 + codon][3]
};

__global__ __launch_bounds__(256) void k_a2c_detail(A2CDetailArgs A)
{
    __shared__ uint32_t s_det[A2C_DET_CELLS];
    __shared__ int8_t s_code[512];
    __shared__ uint8_t s_cls[256];
    const A2CChunk ch = A.chunks[blockIdx.x];
    if (threadIdx.x < A2C_DET_CELLS) s_det[threadIdx.x] = 0;
    s_code[threadIdx.x] = A.code[threadIdx.x];
    s_code[threadIdx.x + 256] = A.code[threadIdx.x + 256];
    s_cls[threadIdx.x] = A.cls[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int f = lane / A2C_W;
    const int j = ch.codon0 + lane - A2C_W * f;
    uint32_t *cc = s_det + lane * A2C_DET;
    for (int64_t i = ch.beg + (threadIdx.x >> 6); i < ch.end; i += 4) {
        if (lane >= A2C_LANES) continue;
        const A2CRow R = A.rows[A.bin_rows[i]];
        if (j < R.off / 3 || j >= (f + R.off + R.len + 2) / 3) continue;
        const int q0 = 3 * j - f - R.off;
        const uint8_t *s = A.text + R.soff;
        int c[3], inside = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int q = q0 + t;
            const bool in = q >= 0 && q < R.len;
            c[t] = in ? s_cls[s[q]] : A2C_DASH;
            inside += in;
        }
        if (s_code[64 * c[0] + 8 * c[1] + c[2]] < A2C_NAA) continue;     // amino.csv's own
        const int dashes = (c[0] == A2C_DASH) + (c[1] == A2C_DASH) + (c[2] == A2C_DASH);
        const int bases = (c[0] < A2C_DASH) + (c[1] < A2C_DASH) + (c[2] < A2C_DASH);
        int k;
        if (dashes == 3 && inside == 3) k = A2C_DET_DEL;
        else if (bases == 0) continue;
        else k = bases == 3 ? A2C_DET_X : A2C_DET_PARTIAL;
        atomicAdd(&cc[k], R.cnt);
    }
    __syncthreads();
    if (threadIdx.x < A2C_DET_CELLS && s_det[threadIdx.x])
        atomicAdd(&A.det[(size_t)ch.bin * A2C_DET_CELLS + threadIdx.x], s_det[threadIdx.x]);
}

// The bins of its group a row reaches: every codon of every frame it touches
// (frame 2 reaches furthest) lies in bins b0 .. b1.
__host__ __device__ inline void a2c_row_bins(int off, int len, int &b0, int &b1)
{
    b0 = (off / 3) / A2C_W;
    b1 = ((2 + off + len + 2) / 3 - 1) / A2C_W;
}

// ---- rows and bin lists from sam2aln's resident results -------------------
constexpr int A2C_TEAM = 16;            // lanes sharing one row's bytes (16 B each per load)
constexpr int A2C_STAGE_GROUPS = 64;    // groups of one block's rows reduced in LDS
constexpr int A2C_LDS_BINS = 1024;      // bins of one block's rows counted in LDS

struct A2CStageArgs {
    const int32_t *order;    // per row of aligned.csv: k of uniq
    const int32_t *gfirst;   // n_groups + 1: first row of each group
    const int64_t *goff;     // per k: where its body starts in text
    const int32_t *res;      // per merge entry: status, offset, body length, stripped length
    const int32_t *uniq;     // per k: representative entry, count
    const uint8_t *text;     // the slot's copy of the bodies (16 spare bytes behind them)
    const uint8_t *cls;
    A2CRow *rows;
    int32_t *ncod;           // 3 per group (zeroed), then one word: a byte of class A2C_BAD seen
    int32_t n_rows, n_groups, per_block;
};

// the group g with gfirst[g] <= i < gfirst[g + 1] (no group is empty)
__device__ __forceinline__ int a2c_group_of(const int32_t *gfirst, int n_groups, int64_t i)
{
    int lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (gfirst[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Row i of aligned.csv as a2c_row reads it from the text: its A2CRow, its
// bytes tested against cls, its codons added to its group's extent per frame
// (a2c_layout).  A block takes per_block consecutive rows, a team of 16
// lanes a row: each lane tests 16 bytes of one aligned load, so a row of a
// few hundred bytes is one or two loads of the team.  The extents of the
// block's first A2C_STAGE_GROUPS groups are reduced in LDS and leave the
// block as one atomicMax per group and frame.
__global__ __launch_bounds__(256) void k_a2c_stage(A2CStageArgs A)
{
    __shared__ uint8_t s_cls[256];
    __shared__ int s_hi[3 * A2C_STAGE_GROUPS];
    __shared__ int s_g0;
    const int64_t r0 = (int64_t)blockIdx.x * A.per_block;
    const int64_t r1 = r0 + A.per_block < A.n_rows ? r0 + A.per_block : A.n_rows;
    s_cls[threadIdx.x] = A.cls[threadIdx.x];
    if (threadIdx.x < 3 * A2C_STAGE_GROUPS) s_hi[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_g0 = a2c_group_of(A.gfirst, A.n_groups, r0);
    __syncthreads();
    const int team = threadIdx.x / A2C_TEAM, tl = threadIdx.x % A2C_TEAM;
    int g = s_g0;
    bool bad = false;
    for (int64_t i = r0 + team; i < r1; i += 256 / A2C_TEAM) {
        while (i >= A.gfirst[g + 1]) ++g;
        const int k = A.order[i];
        const int rep = A.uniq[2 * k];
        A2CRow R;
        R.soff = A.goff[k];
        R.len = A.res[4 * (int64_t)rep + 3];
        R.off = A.res[4 * (int64_t)rep + 1];
        R.cnt = (uint32_t)A.uniq[2 * k + 1];
        R.local = (uint32_t)(i - A.gfirst[g]);
        if (tl == 0) {
            A.rows[i] = R;
            const int lo = R.off / 3, gl = g - s_g0;
            for (int f = 0; f < 3; ++f) {
                const int hi = (f + R.off + R.len + 2) / 3;
                if (hi <= lo) continue;
                if (gl < A2C_STAGE_GROUPS) atomicMax(&s_hi[3 * gl + f], hi);
                else atomicMax(&A.ncod[3 * g + f], hi);
            }
        }
        const int64_t b = R.soff, e = R.soff + R.len;
        for (int64_t p = (b & ~(int64_t)15) + 16 * tl; p < e; p += 16 * A2C_TEAM) {
            const uint4 w = *reinterpret_cast<const uint4 *>(A.text + p);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint32_t ch = (ww[q >> 2] >> (8 * (q & 3))) & 0xffu;
                if (p + q >= b && p + q < e && s_cls[ch] == A2C_BAD) bad = true;
            }
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&A.ncod[3 * A.n_groups], 1);
    __syncthreads();
    if (threadIdx.x < 3 * A2C_STAGE_GROUPS && s_hi[threadIdx.x] > 0)
        atomicMax(&A.ncod[3 * (s_g0 + threadIdx.x / 3) + threadIdx.x % 3], s_hi[threadIdx.x]);
}

struct A2CBinArgs {
    const A2CRow *rows;
    const int32_t *gfirst, *gbin0;    // n_groups + 1 each: first row, first bin of each group
    int32_t n_rows, n_groups;
    unsigned long long *cnt;          // k_a2c_bin_count: rows per bin (zeroed)
    unsigned long long *cur;          // k_a2c_bin_fill: the next free place of each bin's list
    int32_t *bin_rows;
    unsigned long long total;         // places in bin_rows
};

// the bins [b0, b1] (numbered over all groups) of row i, the empty range
// past the last row; g0 = the first bin of the group of the block's first row
__device__ __forceinline__ void a2c_bins_of(const A2CBinArgs &A, int64_t i, int &b0, int &b1, int *g0)
{
    b0 = 0;
    b1 = -1;
    if (i >= A.n_rows) return;
    const int g = a2c_group_of(A.gfirst, A.n_groups, i);
    const A2CRow R = A.rows[i];
    a2c_row_bins(R.off, R.len, b0, b1);
    b0 += A.gbin0[g];
    b1 += A.gbin0[g];
    if (b1 >= A.gbin0[g + 1]) b1 = A.gbin0[g + 1] - 1;   // (its group's extent covers the row)
    if (g0) *g0 = A.gbin0[g];
}

// Rows per bin.  A million rows of one group share some fifty bins, and
// atomics on one global address serialise, so a block of 256 consecutive
// rows counts into an LDS table of the A2C_LDS_BINS bins from its first
// row's group on (1024 bins = 21 504 codons: several groups of a block, or
// one 64 kb reference) and adds each touched bin to the global count once;
// bins past the table are counted in global memory directly.
__global__ __launch_bounds__(256) void k_a2c_bin_count(A2CBinArgs A)
{
    __shared__ uint32_t s_n[A2C_LDS_BINS];
    __shared__ int s_b0;
    for (int k = threadIdx.x; k < A2C_LDS_BINS; k += 256) s_n[k] = 0;
    int b0, b1;
    a2c_bins_of(A, (int64_t)blockIdx.x * 256 + threadIdx.x, b0, b1, threadIdx.x == 0 ? &s_b0 : nullptr);
    __syncthreads();
    for (int b = b0; b <= b1; ++b) {
        if (b - s_b0 < A2C_LDS_BINS) atomicAdd(&s_n[b - s_b0], 1u);
        else atomicAdd(&A.cnt[b], 1ull);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < A2C_LDS_BINS; k += 256)
        if (s_n[k]) atomicAdd(&A.cnt[s_b0 + k], (unsigned long long)s_n[k]);
}

// start[b] = cnt[0] + .. + cnt[b - 1] for b = 0 .. n (one block)
__global__ __launch_bounds__(1024) void k_a2c_bin_scan(const unsigned long long *cnt,
                                                       unsigned long long *start, int n)
{
    __shared__ unsigned long long s[1024];
    const int per = (n + 1023) / 1024;
    const int64_t a0 = (int64_t)threadIdx.x * per;
    const int a = a0 < n ? (int)a0 : n, b = a0 + per < n ? (int)(a0 + per) : n;
    unsigned long long sum = 0;
    for (int i = a; i < b; ++i) sum += cnt[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long v = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = s[threadIdx.x] - sum;
    for (int i = a; i < b; ++i) {
        start[i] = run;
        run += cnt[i];
    }
    if (threadIdx.x == 1023) start[n] = s[1023];
}

// The bin lists: the block counts as k_a2c_bin_count does, takes its range
// of every touched bin's list with one global atomicAdd, and its rows take
// their places inside the ranges through the LDS counts.  The order of the
// rows of a bin is free (k_a2c_count adds counts and takes the least row).
__global__ __launch_bounds__(256) void k_a2c_bin_fill(A2CBinArgs A)
{
    __shared__ uint32_t s_n[A2C_LDS_BINS];
    __shared__ unsigned long long s_at[A2C_LDS_BINS];
    __shared__ int s_b0;
    for (int k = threadIdx.x; k < A2C_LDS_BINS; k += 256) s_n[k] = 0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int b0, b1;
    a2c_bins_of(A, i, b0, b1, threadIdx.x == 0 ? &s_b0 : nullptr);
    __syncthreads();
    for (int b = b0; b <= b1; ++b)
        if (b - s_b0 < A2C_LDS_BINS) atomicAdd(&s_n[b - s_b0], 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < A2C_LDS_BINS; k += 256)
        if (s_n[k]) {
            s_at[k] = atomicAdd(&A.cur[s_b0 + k], (unsigned long long)s_n[k]);
            s_n[k] = 0;
        }
    __syncthreads();
    for (int b = b0; b <= b1; ++b) {
        const unsigned long long at = b - s_b0 < A2C_LDS_BINS
                                          ? s_at[b - s_b0] + atomicAdd(&s_n[b - s_b0], 1u)
                                          : atomicAdd(&A.cur[b], 1ull);
        if (at < A.total) A.bin_rows[at] = (int32_t)i;
    }
}

// ---- the distinct strings of the (class, row) pairs of one call ------------
// Pair p = cls * n_rows + row.  A hash kernel of the caller writes h[p], the
// key of the pair's string (0: the pair produces none), and counts the keyed
// pairs in ctr[0]; an open-addressing table of at least twice that many
// slots then holds per key the summed count of its rows and the first of
// them (k_a2c_tab_count); a verify kernel of the caller compares every pair
// with its slot's first row (ctr[1]: pairs that differ, an error of the
// call); the occupied slots leave as entries (k_a2c_tab_compact, ctr[2]).
struct A2CTable {
    const A2CRow *rows;      // the rows of the call: its group's, or a rank's part of them
    int64_t n_rows, n_pairs;
    uint64_t *h;
    uint64_t *tkey;          // 0 = free
    unsigned long long *tcnt;
    uint32_t *tfirst;        // index in rows
    int32_t *tclass;
    uint64_t mask;
    A2CDistinct *entries;
    unsigned long long *ctr;
};

__device__ __forceinline__ uint64_t a2c_slot(uint64_t h, uint64_t mask)
{
    return ((h * 0x9e3779b97f4a7c15ull) >> 20) & mask;
}

__device__ __forceinline__ unsigned long long a2c_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ void a2c_table_add(const A2CTable &T, uint64_t h, int cls, unsigned long long cnt, uint32_t first)
{
    const TableSlot c = table_claim(T.tkey, T.mask, a2c_slot(h, T.mask), h);
    if (c.created) T.tclass[c.slot] = cls;
    atomicAdd(&T.tcnt[c.slot], cnt);
    atomicMin(&T.tfirst[c.slot], first);
}

constexpr int A2C_COMBINE = 4;           // rounds of equal-key combining in a wave

// A thread per pair.  Equal keys of a wave are combined first (the dominant
// string is most of every wave, and atomics on one address serialise): for
// A2C_COMBINE rounds the lanes holding the lowest active lane's key add their
// counts up and take their least row, and that lane alone goes to the table;
// what is left goes lane by lane.
__global__ __launch_bounds__(256) void k_a2c_tab_count(A2CTable T)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t h = 0;
    uint32_t idx = 0;
    unsigned long long cnt = 0;
    int cls = 0;
    if (p < T.n_pairs) {
        h = T.h[p];
        idx = (uint32_t)(p % T.n_rows);
        cls = (int)(p / T.n_rows);
        if (h) cnt = T.rows[idx].cnt;
    }
    bool todo = h != 0;
    for (int round = 0; round < A2C_COMBINE; ++round) {
        const unsigned long long act = __ballot(todo);
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const uint64_t k = __shfl((unsigned long long)h, leader);
        const bool mine = todo && h == k;
        const unsigned long long sum = a2c_wave_sum(mine ? cnt : 0ull);
        uint32_t mn = mine ? idx : A2C_NONE;
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const uint32_t o = __shfl_xor(mn, d);
            mn = o < mn ? o : mn;
        }
        if (lane == leader) a2c_table_add(T, h, cls, sum, mn);
        todo = todo && !mine;
    }
    if (todo) a2c_table_add(T, h, cls, cnt, idx);
}

// The occupied slots as entries, one counter atomic per wave.  Args derives
// from A2CTable and gives a2c_entry_len(A, cls, first): the entry's len.
template <class Args>
__global__ __launch_bounds__(256) void k_a2c_tab_compact(Args A)
{
    const int lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool used = s <= A.mask && A.tkey[s] != 0;
    const unsigned long long b = __ballot(used);
    if (!b) return;
    unsigned long long base = 0;
    const int leader = __ffsll((long long)b) - 1;
    if (lane == leader) base = atomicAdd(&A.ctr[2], (unsigned long long)__popcll(b));
    base = __shfl(base, leader);
    if (!used) return;
    A2CDistinct e;
    e.cls = A.tclass[s];
    e.first = A.tfirst[s];
    e.count = A.tcnt[s];
    e.pad = 0;
    e.len = a2c_entry_len(A, e.cls, e.first);
    A.entries[base + __popcll(b & ((1ull << lane) - 1))] = e;
}

struct A2CInsArgs : A2CTable {
    const uint8_t *text;
    const int8_t *code;
    const uint8_t *cls;
    const int32_t *left, *right;
    int frame;
};

// The framed slice of one read for one range (:787-791): read indices
// [lo, lo + 3 n) of its whole codons, or false when the slice starts in the
// '-' padding, is empty, holds '-' or 'n', or translates to nothing.
// scan = false gives the indices without reading the bytes: only for a row
// that k_a2c_ins_hash already keyed for this range (an entry's first row),
// which therefore passed the scan.
__device__ bool a2c_slice(const A2CInsArgs &A, const A2CRow &R, int rg, int &lo, int &n, bool scan = true)
{
    const int64_t s = 3LL * A.left[rg] - A.frame - R.off;
    int64_t e = 3LL * A.right[rg] - A.frame - R.off;
    if (e > R.len) e = R.len;
    if (s < 0 || e - s < 3) return false;
    const uint8_t *p = A.text + R.soff;
    for (int64_t q = s; scan && q < e; ++q) {
        const uint8_t c = A.cls[p[q]];
        if (c == A2C_DASH || c == A2C_GAP) return false;
    }
    lo = (int)s;
    n = (int)((e - s) / 3);
    return true;
}

__device__ __forceinline__ int a2c_codon(const A2CInsArgs &A, const uint8_t *p, int q)
{
    return A.code[64 * A.cls[p[q]] + 8 * A.cls[p[q + 1]] + A.cls[p[q + 2]]];
}

__device__ __forceinline__ uint64_t a2c_mix(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the codons of an entry's string (k_a2c_tab_compact)
__device__ __forceinline__ int a2c_entry_len(const A2CInsArgs &A, int rg, uint32_t first)
{
    int lo = 0, n = 0;
    a2c_slice(A, A.rows[first], rg, lo, n, false);
    return n;
}

__global__ __launch_bounds__(256) void k_a2c_ins_hash(A2CInsArgs A)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (p < A.n_pairs) {
        const int rg = (int)(p / A.n_rows);
        const A2CRow R = A.rows[p % A.n_rows];
        int lo, n;
        uint64_t h = 0;
        if (a2c_slice(A, R, rg, lo, n)) {
            const uint8_t *s = A.text + R.soff;
            h = a2c_mix(0x243f6a8885a308d3ull + (uint64_t)rg);
            for (int k = 0; k < n; ++k) h = a2c_mix(h ^ (uint64_t)(a2c_codon(A, s, lo + 3 * k) + 1));
            h = a2c_mix(h ^ ((uint64_t)n << 32)) | 1ull;
            ok = true;
        }
        A.h[p] = h;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&A.ctr[0], (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void k_a2c_ins_verify(A2CInsArgs A)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pairs) return;
    const uint64_t h = A.h[p];
    if (!h) return;
    const int rg = (int)(p / A.n_rows);
    const uint64_t s = table_find(A.tkey, A.mask, a2c_slot(h, A.mask), h);
    const A2CRow R = A.rows[p % A.n_rows], F = A.rows[A.tfirst[s]];
    int lo = 0, n = 0, flo = 0, fn = 0;
    bool same = A.tclass[s] == rg && a2c_slice(A, R, rg, lo, n) && a2c_slice(A, F, rg, flo, fn) &&
                n == fn;
    const uint8_t *pr = A.text + R.soff, *pf = A.text + F.soff;
    for (int k = 0; same && k < n; ++k)
        same = a2c_codon(A, pr, lo + 3 * k) == a2c_codon(A, pf, flo + 3 * k);
    if (!same) atomicAdd(&A.ctr[1], 1ull);
}

// amino-acid strings of the (sorted) entries, each followed by '\n'
__global__ __launch_bounds__(256) void k_a2c_ins_gather(A2CInsArgs A, const A2CDistinct *ent,
                                                        const int64_t *eoff, int64_t n_ent,
                                                        char *out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_ent) return;
    const A2CDistinct e = ent[k];
    const A2CRow F = A.rows[e.first];
    const uint8_t *s = A.text + F.soff;
    int lo = 0, n = 0;
    a2c_slice(A, F, e.cls, lo, n, false);
    char *o = out + eoff[k];
    for (int c = 0; c < e.len; ++c) o[c] = c_a2c_codes[a2c_codon(A, s, lo + 3 * c)];
    o[e.len] = '\n';
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static void a2c_free_device(A2CState &S)
{
    hipFree(S.d_text); hipFree(S.d_cls); hipFree(S.d_code); hipFree(S.d_rows);
    hipFree(S.d_bin_rows); hipFree(S.d_chunks); hipFree(S.d_cnt); hipFree(S.d_first);
    hipFree(S.d_order); hipFree(S.d_gfirst); hipFree(S.d_gbin0); hipFree(S.d_ncod);
    hipFree(S.d_bstart); hipFree(S.d_bcur); hipFree(S.d_det);
    S.d_det = nullptr;
    S.counted = S.det_ready = false;
    S.d_order = S.d_gfirst = S.d_gbin0 = S.d_ncod = nullptr;
    S.d_bstart = S.d_bcur = nullptr;
    S.d_text = S.d_cls = nullptr;
    S.d_code = nullptr;
    S.d_rows = nullptr;
    S.d_bin_rows = nullptr;
    S.d_chunks = nullptr;
    S.d_cnt = S.d_first = nullptr;
    S.dcap.clear();
}

// byte classes and the codon table from the caller's translations of the 216
// codons over A C G T N - (micall_amd/translation.py codon_chars)
static int a2c_tables(A2CState &S, const char *codon_chars)
{
    if (!codon_chars || strlen(codon_chars) != 216) {
        set_error("aln2counts: codon_chars must hold 216 translations");
        return -3;
    }
    memset(S.cls, A2C_BAD, sizeof(S.cls));
    const char *alpha = "ACGTN-";
    for (int k = 0; k < 6; ++k) S.cls[(uint8_t)alpha[k]] = (uint8_t)k;
    S.cls[(uint8_t)'n'] = A2C_GAP;
    for (int c0 = 0; c0 < 8; ++c0)
        for (int c1 = 0; c1 < 8; ++c1)
            for (int c2 = 0; c2 < 8; ++c2) {
                // count_aminos upper-cases the codon: 'n' translates as 'N'
                const int m0 = c0 == A2C_GAP ? 4 : c0, m1 = c1 == A2C_GAP ? 4 : c1,
                          m2 = c2 == A2C_GAP ? 4 : c2;
                int8_t v = 22;
                if (m0 < 6 && m1 < 6 && m2 < 6) {
                    const char ch = codon_chars[36 * m0 + 6 * m1 + m2];
                    const char *hit = ch ? strchr(A2C_CODES, ch) : nullptr;
                    if (!hit) {
                        set_error("aln2counts: codon translation '%c' is not an amino-acid code", ch);
                        return -3;
                    }
                    v = (int8_t)(hit - A2C_CODES);
                }
                S.code[64 * c0 + 8 * c1 + c2] = v;
            }
    return 0;
}

struct A2CKey {
    const char *p;
    int32_t n;
};

struct A2CPart {
    const char *beg, *end;
    std::vector<A2CRow> rows;
    std::vector<A2CKey> kref, kqcut;
    std::deque<std::string> pool;      // unquoted keys and seqs (quoted input only)
    int64_t err_row = -1;
    std::string err;
};

enum { COL_REF, COL_QCUT, COL_COUNT, COL_OFFSET, COL_SEQ, N_COLS };

// One data row into P (fields as [begin, end) views); false on an error.
static bool a2c_row(A2CPart &P, const char *const *fb, const char *const *fe, const int *col,
                    const char *base, const uint8_t *cls)
{
    int64_t cnt = 0, off = 0;
    if (!py_int(std::string_view(fb[col[COL_COUNT]], (size_t)(fe[col[COL_COUNT]] - fb[col[COL_COUNT]])), cnt)) {
        P.err = "invalid literal for int() with base 10 in column count";
        return false;
    }
    if (!py_int(std::string_view(fb[col[COL_OFFSET]], (size_t)(fe[col[COL_OFFSET]] - fb[col[COL_OFFSET]])), off)) {
        P.err = "invalid literal for int() with base 10 in column offset";
        return false;
    }
    if (cnt < 0 || cnt > (int64_t)UINT32_MAX) { P.err = "count outside 0 .. 2**32-1"; return false; }
    if (off < 0 || off > A2C_MAX_SPAN) { P.err = "offset outside 0 .. 2**28"; return false; }
    const char *sb = fb[col[COL_SEQ]], *se = fe[col[COL_SEQ]];
    if (se - sb > A2C_MAX_SPAN) { P.err = "seq longer than 2**28"; return false; }
    for (const char *c = sb; c < se; ++c)
        if (cls[(uint8_t)*c] == A2C_BAD) {
            P.err = std::string("character '") + *c + "' in seq is not one of A C G T N - n";
            return false;
        }
    A2CRow R;
    R.soff = sb - base;
    R.len = (int32_t)(se - sb);
    R.off = (int32_t)off;
    R.cnt = (uint32_t)cnt;
    R.local = 0;
    P.rows.push_back(R);
    P.kref.push_back({fb[col[COL_REF]], (int32_t)(fe[col[COL_REF]] - fb[col[COL_REF]])});
    P.kqcut.push_back({fb[col[COL_QCUT]], (int32_t)(fe[col[COL_QCUT]] - fb[col[COL_QCUT]])});
    return true;
}

// unquoted text: every field is a view into the text
static void a2c_parse_part(A2CPart &P, const int *col, int need, const char *base,
                           const uint8_t *cls)
{
    std::vector<const char *> fb(need), fe(need);
    const char *p = P.beg;
    int64_t row = 0;
    while (p < P.end) {
        int nf = 0;
        const char *s = p;
        for (;;) {
            const char *q = s;
            while (q < P.end && *q != ',' && *q != '\n' && *q != '\r') ++q;
            if (nf < need) { fb[nf] = s; fe[nf] = q; }
            ++nf;
            if (q < P.end && *q == ',') { s = q + 1; continue; }
            if (q < P.end && *q == '\r') ++q;
            if (q < P.end && *q == '\n') ++q;
            p = q;
            break;
        }
        if (nf == 1 && fb[0] == fe[0]) continue;             // blank line: DictReader skips it
        if (nf < need) { P.err_row = row; P.err = "row has fewer fields than the header"; return; }
        if (!a2c_row(P, fb.data(), fe.data(), col, base, cls)) { P.err_row = row; return; }
        ++row;
    }
}

// quoted text (rare): fields unescaped into P.pool; seqs are copied too, so
// the rows point into the state's pool instead of the caller's text
static void a2c_parse_quoted(A2CPart &P, const int *col, int need, const uint8_t *cls,
                             std::string &seqpool)
{
    std::vector<std::string_view> f;
    std::deque<std::string> scratch;
    std::vector<const char *> fb(need), fe(need);
    const char *p = P.beg;
    int64_t row = 0;
    while (csv_views(p, P.end, f, scratch)) {
        if (f.size() == 1 && f[0].empty()) continue;
        if ((int)f.size() < need) { P.err_row = row; P.err = "row has fewer fields than the header"; return; }
        for (int k = 0; k < need; ++k) {
            P.pool.emplace_back(f[k]);
            fb[k] = P.pool.back().data();
            fe[k] = fb[k] + P.pool.back().size();
        }
        const size_t seq_at = seqpool.size();
        seqpool.append(f[col[COL_SEQ]]);
        if (!a2c_row(P, fb.data(), fe.data(), col, fb[col[COL_SEQ]], cls)) { P.err_row = row; return; }
        P.rows.back().soff = (int64_t)seq_at;
        ++row;
    }
}

// Per-group codon extents, bins, bin row lists and chunks.
// preset: g_ncod and every row's `local` were set by the caller (a part of
// a sharded job: the job's codon extents and row numbers within the group)
static int a2c_layout(A2CState &S, std::vector<int32_t> &bin_rows, std::vector<A2CChunk> &chunks,
                      bool preset = false)
{
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (!preset) S.g_ncod.assign(3 * ng, 0);
    S.g_bin0.assign(ng + 1, 0);
    if (S.n_rows >= INT32_MAX) { set_error("aln2counts: more than 2**31 rows"); return -3; }
    for (int64_t g = 0; g < ng; ++g) {
        int32_t *nc = &S.g_ncod[3 * g];
        if (preset) {
            const int top = std::max(nc[0], std::max(nc[1], nc[2]));
            S.g_bin0[g + 1] = S.g_bin0[g] + (top + A2C_W - 1) / A2C_W;
            continue;
        }
        uint64_t total = 0;
        for (int64_t r = S.g_first[g]; r < S.g_first[g + 1]; ++r) {
            A2CRow &R = S.rows[r];
            R.local = (uint32_t)(r - S.g_first[g]);
            total += R.cnt;
            const int lo = R.off / 3;
            for (int f = 0; f < 3; ++f) {
                const int hi = (f + R.off + R.len + 2) / 3;
                if (hi > lo && hi > nc[f]) nc[f] = hi;
            }
        }
        if (total > UINT32_MAX) {
            set_error("aln2counts: the counts of group %lld add up to more than 2**32-1", (long long)g);
            return -3;
        }
        const int top = std::max(nc[0], std::max(nc[1], nc[2]));
        S.g_bin0[g + 1] = S.g_bin0[g] + (top + A2C_W - 1) / A2C_W;
    }
    S.n_bins = S.g_bin0[ng];
    std::vector<int64_t> start(S.n_bins + 1, 0);
    for (int64_t g = 0; g < ng; ++g)
        for (int64_t r = S.g_first[g]; r < S.g_first[g + 1]; ++r) {
            const A2CRow &R = S.rows[r];
            int r0, r1;
            a2c_row_bins(R.off, R.len, r0, r1);
            for (int64_t b = S.g_bin0[g] + r0; b <= S.g_bin0[g] + r1; ++b) ++start[b + 1];
        }
    for (int64_t b = 0; b < S.n_bins; ++b) start[b + 1] += start[b];
    bin_rows.assign(start[S.n_bins], 0);
    std::vector<int64_t> cur(start.begin(), start.end() - 1);
    for (int64_t g = 0; g < ng; ++g)
        for (int64_t r = S.g_first[g]; r < S.g_first[g + 1]; ++r) {
            const A2CRow &R = S.rows[r];
            int r0, r1;
            a2c_row_bins(R.off, R.len, r0, r1);
            for (int64_t b = S.g_bin0[g] + r0; b <= S.g_bin0[g] + r1; ++b) bin_rows[cur[b]++] = (int32_t)r;
        }
    chunks.clear();
    for (int64_t g = 0; g < ng; ++g)
        for (int64_t b = S.g_bin0[g]; b < S.g_bin0[g + 1]; ++b)
            for (int64_t i = start[b]; i < start[b + 1]; i += A2C_CHUNK)
                chunks.push_back({(int32_t)b, (int32_t)((b - S.g_bin0[g]) * A2C_W), i,
                                  std::min<int64_t>(i + A2C_CHUNK, start[b + 1])});
    return 0;
}

template <class T>
static int a2c_reserve(A2CState &S, T *&p, size_t bytes)
{
    // kept between calls, reallocated only to grow (hipFree waits for the device)
    size_t &cap = S.dcap[(const void *)&p];
    if (p && cap >= bytes) return 0;
    hipFree(p);
    p = nullptr;
    cap = 0;
    MH_HIP(hipMalloc(&p, bytes > 0 ? bytes : 1));
    cap = bytes;
    return 0;
}

template <class T>
static int a2c_upload(A2CState &S, T *&dst, const T *src, size_t n, hipStream_t s)
{
    if (int st = a2c_reserve(S, dst, sizeof(T) * n)) return st;
    if (n) MH_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, s));
    return 0;
}

static int a2c_count_chunks(Ctx &c, A2CState &S, size_t n_chunks);

// upload the rows, count every group on the device, fetch the counters
static int a2c_count(Ctx &c, A2CState &S, const char *text, int64_t text_len, bool preset = false)
{
    std::vector<int32_t> bin_rows;
    std::vector<A2CChunk> chunks;
    if (int st = a2c_layout(S, bin_rows, chunks, preset)) return st;
    hipStream_t s = c.stream;
    if (int st = a2c_upload(S, S.d_text, (const uint8_t *)text, (size_t)text_len, s)) return st;
    if (int st = a2c_upload(S, S.d_rows, S.rows.data(), S.rows.size(), s)) return st;
    if (int st = a2c_upload(S, S.d_bin_rows, bin_rows.data(), bin_rows.size(), s)) return st;
    if (int st = a2c_upload(S, S.d_chunks, chunks.data(), chunks.size(), s)) return st;
    if (int st = a2c_upload(S, S.d_code, S.code, 512, s)) return st;
    if (int st = a2c_upload(S, S.d_cls, S.cls, 256, s)) return st;
    return a2c_count_chunks(c, S, chunks.size());
}

// k_a2c_count over the n_chunks chunks on the device (rows, bin lists, text
// and tables are there), the counters fetched
static int a2c_count_chunks(Ctx &c, A2CState &S, size_t n_chunks)
{
    hipStream_t s = c.stream;
    const size_t cells = (size_t)S.n_bins * A2C_CELLS;
    S.counted = S.det_ready = false;
    S.n_chunks = n_chunks;
    if (int st = a2c_reserve(S, S.d_cnt, sizeof(uint32_t) * cells)) return st;
    if (int st = a2c_reserve(S, S.d_first, sizeof(uint32_t) * cells)) return st;
    if (cells) {
        MH_HIP(hipMemsetAsync(S.d_cnt, 0, sizeof(uint32_t) * cells, s));
        MH_HIP(hipMemsetAsync(S.d_first, 0xff, sizeof(uint32_t) * cells, s));
    }
    if (n_chunks) {
        A2CCountArgs a{S.d_text, S.d_rows, S.d_bin_rows, S.d_chunks, S.d_code, S.d_cls,
                       S.d_cnt, S.d_first};
        const int p0 = prof_begin(c, "k_a2c_count");
        hipLaunchKernelGGL(k_a2c_count, dim3((unsigned)n_chunks), dim3(256), 0, s, a);
        prof_end(c, p0);
        MH_HIP(hipGetLastError());
    }
    S.h_cnt.resize(cells);
    S.h_first.resize(cells);
    if (cells) {
        MH_HIP(hipMemcpyAsync(S.h_cnt.data(), S.d_cnt, sizeof(uint32_t) * cells,
                              hipMemcpyDeviceToHost, s));
        MH_HIP(hipMemcpyAsync(S.h_first.data(), S.d_first, sizeof(uint32_t) * cells,
                              hipMemcpyDeviceToHost, s));
    }
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    S.counted = true;
    return 0;
}

// k_a2c_detail over the chunks the last load left on the device, one launch
// for all groups of the slot; the counters fetched
static int a2c_detail_run(Ctx &c, A2CState &S)
{
    hipStream_t s = c.stream;
    const size_t cells = (size_t)S.n_bins * A2C_DET_CELLS;
    if (int st = a2c_reserve(S, S.d_det, sizeof(uint32_t) * cells)) return st;
    if (cells) MH_HIP(hipMemsetAsync(S.d_det, 0, sizeof(uint32_t) * cells, s));
    if (S.n_chunks) {
        A2CDetailArgs a{S.d_text, S.d_rows, S.d_bin_rows, S.d_chunks, S.d_code, S.d_cls, S.d_det};
        const int p0 = prof_begin(c, "k_a2c_detail");
        hipLaunchKernelGGL(k_a2c_detail, dim3((unsigned)S.n_chunks), dim3(256), 0, s, a);
        prof_end(c, p0);
        MH_HIP(hipGetLastError());
    }
    S.h_det.resize(cells);
    if (cells)
        MH_HIP(hipMemcpyAsync(S.h_det.data(), S.d_det, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    S.det_ready = true;
    return 0;
}

static int a2c_parse_csv(A2CState &S, const char *text, int64_t len, bool &use_pool,
                         int64_t body_lo = -1, int64_t body_hi = -1)
{
    const char *p = text, *end = text + len;
    std::vector<std::string> head;
    S.rows.clear();
    S.dev_rows = false;
    S.g_first.assign(1, 0);
    S.g_ref.clear();
    S.g_qcut.clear();
    S.pool.clear();
    use_pool = false;
    if (!csv_record(p, end, head)) return 0;             // empty file: no rows
    if (body_lo >= 0) {      // one part of the body: the records of [body_lo, body_hi)
        p = text + std::max<int64_t>(body_lo, p - text);
        end = text + std::max<int64_t>(body_hi, p - text);
    }
    static const char *const want[N_COLS] = {"refname", "qcut", "count", "offset", "seq"};
    int col[N_COLS];
    int need = 0;
    csv_columns(head, want, N_COLS, col);
    for (int k = 0; k < N_COLS; ++k) need = std::max(need, col[k] + 1);
    const int64_t body = end - p;
    const bool quoted = memchr(p, '"', (size_t)body) != nullptr;
    for (int k = 0; k < N_COLS; ++k)
        if (col[k] < 0) {
            // DictReader only fails when a row is read: row['refname'] -> KeyError
            const char *q = p;
            while (q < end && (*q == '\n' || *q == '\r')) ++q;
            if (q == end) return 0;
            set_error("aligned csv: KeyError: '%s'", want[k]);
            return -3;
        }
    int nt = quoted ? 1 : s2a_threads();
    if (body < (int64_t)nt * (1 << 20)) nt = (int)std::max<int64_t>(1, body >> 20);
    const std::vector<const char *> cut = csv_cuts(p, end, nt);
    std::vector<A2CPart> parts(nt);
    for (int t = 0; t < nt; ++t) { parts[t].beg = cut[t]; parts[t].end = cut[t + 1]; }
    if (quoted) {
        use_pool = true;
        a2c_parse_quoted(parts[0], col, need, S.cls, S.pool);
    } else {
        par_for(nt, [&](int t) { a2c_parse_part(parts[t], col, need, text, S.cls); });
    }
    int64_t base = 0;
    for (auto &P : parts) {
        if (P.err_row >= 0) {
            set_error("aligned csv row %lld: %s", (long long)(base + P.err_row + 1), P.err.c_str());
            return -3;
        }
        base += (int64_t)P.rows.size();
    }
    S.n_rows = base;
    S.rows.resize(base);
    int64_t o = 0;
    A2CKey pr{nullptr, -1}, pq{nullptr, -1};
    for (auto &P : parts) {
        memcpy(S.rows.data() + o, P.rows.data(), sizeof(A2CRow) * P.rows.size());
        for (size_t i = 0; i < P.rows.size(); ++i) {
            const A2CKey &kr = P.kref[i], &kq = P.kqcut[i];
            const bool same = kr.n == pr.n && kq.n == pq.n && !memcmp(kr.p, pr.p, kr.n) &&
                              !memcmp(kq.p, pq.p, kq.n);
            if (!same) {
                if (o + (int64_t)i > 0) S.g_first.push_back(o + (int64_t)i);
                S.g_ref.emplace_back(kr.p, kr.n);
                S.g_qcut.emplace_back(kq.p, kq.n);
                pr = kr;
                pq = kq;
            }
        }
        o += (int64_t)P.rows.size();
    }
    if (S.n_rows) S.g_first.push_back(S.n_rows);
    // the key views of the last part may point into its pool: the group
    // names were copied above, so the parts can go
    return 0;
}

static A2CState *a2c_state(Ctx &c, int slot)
{
    if (!c.a2c) c.a2c = new A2CState *[A2C_SLOTS]();
    if (!c.a2c[slot]) c.a2c[slot] = new A2CState();
    return c.a2c[slot];
}

void a2c_free(Ctx &c)
{
    if (!c.a2c) return;
    for (int k = 0; k < A2C_SLOTS; ++k)
        if (c.a2c[k]) {
            if (c.a2c[k]->part_text) unmap_text_file(c.a2c[k]->part_text, c.a2c[k]->part_len);
            a2c_free_device(*c.a2c[k]);
            delete c.a2c[k];
        }
    delete[] c.a2c;
    c.a2c = nullptr;
}

static void a2c_clear_link(A2CState &S)
{
    S.link_set.clear();
    S.link_count.clear();
    S.link_text.clear();
    S.link_cov.clear();
    for (int k = 0; k < 3; ++k) S.link_stats[k] = 0;
    S.t_link = 0;
}

static void a2c_clear_gram(A2CState &S)
{
    for (int k = 0; k < 5; ++k) S.gram_stats[k] = 0;
    S.t_gram = 0;
}

static void a2c_clear_inserts(A2CState &S)
{
    S.entries.clear();
    S.aminos.clear();
    S.var_entries.clear();
    S.var_region.clear();
    S.var_text.clear();
    a2c_clear_link(S);
    a2c_clear_gram(S);
}

// The device memory of one call: every allocation is freed when the holder
// goes, however the call returns (move-only, as its unique_ptrs are).
struct A2CDevFree {
    void operator()(void *p) const { hipFree(p); }
};
struct A2CDevMem {
    std::vector<std::unique_ptr<void, A2CDevFree>> held;
    template <class T> hipError_t alloc(T *&p, size_t n)
    {
        p = nullptr;
        const hipError_t e = hipMalloc(&p, sizeof(T) * n);
        if (e == hipSuccess) held.emplace_back(p);
        return e;
    }
};

// The middle of mh_a2c_inserts and mh_a2c_variants: a.h is filled and
// ctr[0] (on the host) counts its keys.  Sizes, allocates and clears the
// table, groups (k_a2c_tab_count), verifies with the caller's kernel, compacts
// and reads the counters back: a.entries[0 .. ctr[2]) are on the device in no
// particular order.  who: the calling function, for a failure's text; label:
// the profile names of the three launches (a name repeated takes them under
// one bracket).  -4 with the caller's message when distinct strings share a
// key.
template <class Args>
static int a2c_group_strings(Ctx &c, A2CDevMem &mem, Args &a, unsigned long long *ctr,
                             void (*verify)(Args), unsigned verify_blocks, const char *who,
                             const char *const label[3], const char *collision)
{
    hipStream_t s = c.stream;
    uint64_t tsize = 1024;
    while (tsize < 2 * ctr[0]) tsize <<= 1;
    hipError_t e = mem.alloc(a.tkey, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tcnt, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tfirst, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tclass, tsize);
    if (e == hipSuccess) e = mem.alloc(a.entries, ctr[0]);
    if (e == hipSuccess) e = hipMemsetAsync(a.tkey, 0, sizeof(uint64_t) * tsize, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.tcnt, 0, sizeof(unsigned long long) * tsize, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.tfirst, 0xff, sizeof(uint32_t) * tsize, s);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + " table").c_str());
    a.mask = tsize - 1;
    const dim3 pair_blocks((unsigned)((a.n_pairs + 255) / 256)), slot_blocks((unsigned)((tsize + 255) / 256));
    int p = prof_begin(c, label[0]);
    auto next = [&](int k) {
        if (strcmp(label[k], label[k - 1]) == 0) return;
        prof_end(c, p);
        p = prof_begin(c, label[k]);
    };
    hipLaunchKernelGGL(k_a2c_tab_count, pair_blocks, dim3(256), 0, s, static_cast<const A2CTable &>(a));
    next(1);
    hipLaunchKernelGGL(verify, dim3(verify_blocks), dim3(256), 0, s, a);
    next(2);
    hipLaunchKernelGGL(k_a2c_tab_compact<Args>, slot_blocks, dim3(256), 0, s, a);
    prof_end(c, p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, a.ctr, 3 * sizeof(*ctr), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, label[0]);
    if (ctr[1]) {
        set_error("%s", collision);
        return -4;
    }
    return 0;
}

}  // namespace mh

using namespace mh;

extern "C" int mh_a2c_load_csv(mh_ctx *ctx, int slot, const char *text, int64_t len,
                               const char *codon_chars, int64_t *n_groups)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || (!text && len) || len < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_inserts(S);
    S.counted = S.det_ready = false;
    if (S.part_text) {       // a part left open by a sharded load that fell back
        unmap_text_file(S.part_text, S.part_len);
        S.part_text = nullptr;
        S.part_open = false;
    }
    auto t0 = std::chrono::steady_clock::now();
    if (int st = a2c_tables(S, codon_chars)) return st;
    bool use_pool = false;
    int st = 0;
    try {   // a parser thread's bad_alloc arrives here (par_for)
        st = a2c_parse_csv(S, text ? text : "", len, use_pool);
    } catch (const std::exception &e) {
        set_error("mh_a2c_load_csv: out of memory (%s)", e.what());
        st = -2;
    }
    if (st) {
        S.rows.clear();
        S.g_first.assign(1, 0);
        return st;
    }
    S.t_parse = ms_since(t0);
    auto t1 = std::chrono::steady_clock::now();
    st = use_pool ? a2c_count(c, S, S.pool.data(), (int64_t)S.pool.size())
                  : a2c_count(c, S, text ? text : "", len);
    if (st) {
        S.rows.clear();
        S.g_first.assign(1, 0);
        return st;
    }
    S.t_count = ms_since(t1);
    if (n_groups) *n_groups = (int64_t)S.g_first.size() - 1;
    return 0;
}

extern "C" int mh_a2c_load_file(mh_ctx *ctx, int slot, int fd, const char *codon_chars, int64_t *n_groups)
{
    if (!ctx || fd < 0) return -3;
    const char *text = nullptr;
    size_t len = 0;
    if (int st = map_text_file(fd, &text, &len)) return st;
    const int rc = mh_a2c_load_csv(ctx, slot, text, (int64_t)len, codon_chars, n_groups);
    unmap_text_file(text, len);
    return rc;
}

// The rows of aligned.csv from the results sam2aln left on the device: see
// micall_hip.h.  1: the caller loads the file (whose errors are then the
// file path's own).
static int a2c_load_resident(Ctx &c, A2CState &S, int64_t *n_groups)
{
    if (!c.s2a || !c.s2a->complete) return 1;
    S2AState &Q = *c.s2a;
    auto t0 = std::chrono::steady_clock::now();
    s2a_order(Q);
    const S2AOrder &O = Q.order;
    const int64_t ng = (int64_t)O.g_name.size(), n = O.g_first.back();
    const int64_t ne = Q.n_merge * (int64_t)Q.q_cutoffs.size();
    const int64_t text_len = Q.n_unique ? Q.uniq_off[(size_t)Q.n_unique] : 0;
    if (n >= INT32_MAX) return 1;
    if (n && (!Q.d_gather || !Q.d_goff || !Q.d_res || !Q.d_uniq || text_len <= 0)) return 1;
    for (int64_t g = 0; g < ng; ++g) {
        const std::string &name = Q.names[(size_t)O.g_name[g]];
        if (name.find_first_of("\",\r\n") != std::string::npos) return 1;
        if (O.g_total[g] > UINT32_MAX) return 1;
        // two runs of one (refname, qcut) side by side are one group of the file
        if (g && O.g_qcut[g] == O.g_qcut[g - 1] && name == Q.names[(size_t)O.g_name[g - 1]]) return 1;
    }
    // the limits a2c_row checks, and every index the kernels follow
    const int nt = std::max(1, std::min(s2a_threads(), (int)(n >> 16) + 1));
    std::atomic<int> off_limits(0), broken(0);
    par_for(nt, [&](int t) {
        for (int64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
            const int64_t k = O.rows[(size_t)i];
            if (k < 0 || k >= Q.n_unique) { broken = 1; return; }
            const int64_t rep = Q.uniq[2 * k];
            if (rep < 0 || rep >= ne) { broken = 1; return; }
            const int64_t off = Q.res[4 * rep + 1], len = Q.res[4 * rep + 3];
            if (len < 0 || len > Q.uniq_off[(size_t)k + 1] - Q.uniq_off[(size_t)k] || Q.uniq[2 * k + 1] < 0) {
                broken = 1;
                return;
            }
            if (off < 0 || off > A2C_MAX_SPAN || len > A2C_MAX_SPAN) { off_limits = 1; return; }
        }
    });
    if (broken) {
        set_error("mh_a2c_load_resident: the sam2aln results are inconsistent");
        return -3;
    }
    if (off_limits) return 1;
    S.rows.clear();
    S.dev_rows = true;
    S.n_rows = n;
    S.pool.clear();
    S.g_first = O.g_first;
    S.g_ref.clear();
    S.g_qcut.clear();
    for (int64_t g = 0; g < ng; ++g) {
        S.g_ref.push_back(Q.names[(size_t)O.g_name[g]]);
        S.g_qcut.push_back(std::to_string(O.g_qcut[g]));
    }
    S.g_ncod.assign(3 * (size_t)ng, 0);
    S.g_bin0.assign((size_t)ng + 1, 0);
    S.n_bins = 0;
    hipStream_t s = c.stream;
    if (int st = a2c_upload(S, S.d_code, S.code, 512, s)) return st;
    if (int st = a2c_upload(S, S.d_cls, S.cls, 256, s)) return st;
    size_t n_chunks = 0;
    auto t1 = t0;
    if (n) {
        // ---- staging: the bodies into the slot, the rows, the codon extents ----
        std::vector<int32_t> gfirst(O.g_first.begin(), O.g_first.end());
        if (int st = a2c_upload(S, S.d_order, O.rows.data(), (size_t)n, s)) return st;
        if (int st = a2c_upload(S, S.d_gfirst, gfirst.data(), gfirst.size(), s)) return st;
        if (int st = a2c_reserve(S, S.d_text, (size_t)text_len + 16)) return st;
        if (int st = a2c_reserve(S, S.d_rows, sizeof(A2CRow) * (size_t)n)) return st;
        if (int st = a2c_reserve(S, S.d_ncod, sizeof(int32_t) * (3 * (size_t)ng + 1))) return st;
        MH_HIP(hipMemcpyAsync(S.d_text, Q.d_gather, (size_t)text_len, hipMemcpyDeviceToDevice, s));
        MH_HIP(hipMemsetAsync(S.d_text + text_len, 0, 16, s));
        MH_HIP(hipMemsetAsync(S.d_ncod, 0, sizeof(int32_t) * (3 * (size_t)ng + 1), s));
        int64_t per_block = (n + 2047) / 2048;
        per_block = std::max<int64_t>(256 / A2C_TEAM, (per_block + 15) & ~(int64_t)15);
        A2CStageArgs a{S.d_order, S.d_gfirst, Q.d_goff, Q.d_res, Q.d_uniq, S.d_text, S.d_cls, S.d_rows,
                       S.d_ncod, (int32_t)n, (int32_t)ng, (int32_t)per_block};
        const int p0 = prof_begin(c, "k_a2c_stage");
        hipLaunchKernelGGL(k_a2c_stage, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, s, a);
        prof_end(c, p0);
        MH_HIP(hipGetLastError());
        std::vector<int32_t> ncod(3 * (size_t)ng + 1);
        MH_HIP(hipMemcpyAsync(ncod.data(), S.d_ncod, sizeof(int32_t) * ncod.size(), hipMemcpyDeviceToHost, s));
        MH_HIP(hipStreamSynchronize(s));
        prof_flush(c);
        if (ncod[3 * (size_t)ng]) return 1;     // a byte the file path names in its error
        S.t_parse = ms_since(t0);
        t1 = std::chrono::steady_clock::now();
        // ---- layout: bins per group, rows per bin, the bin lists, the chunks ----
        std::vector<int32_t> gbin0((size_t)ng + 1, 0);
        for (int64_t g = 0; g < ng; ++g) {
            const int32_t *nc = &ncod[3 * (size_t)g];
            for (int f = 0; f < 3; ++f) S.g_ncod[3 * (size_t)g + f] = nc[f];
            const int top = std::max(nc[0], std::max(nc[1], nc[2]));
            S.g_bin0[(size_t)g + 1] = S.g_bin0[(size_t)g] + (top + A2C_W - 1) / A2C_W;
            if (S.g_bin0[(size_t)g + 1] >= INT32_MAX) return 1;
            gbin0[(size_t)g + 1] = (int32_t)S.g_bin0[(size_t)g + 1];
        }
        S.n_bins = S.g_bin0[(size_t)ng];
        const size_t nb = (size_t)S.n_bins;
        if (int st = a2c_upload(S, S.d_gbin0, gbin0.data(), gbin0.size(), s)) return st;
        if (int st = a2c_reserve(S, S.d_bstart, sizeof(unsigned long long) * (nb + 1))) return st;
        if (int st = a2c_reserve(S, S.d_bcur, sizeof(unsigned long long) * (nb + 1))) return st;
        MH_HIP(hipMemsetAsync(S.d_bcur, 0, sizeof(unsigned long long) * (nb + 1), s));
        A2CBinArgs b{S.d_rows, S.d_gfirst, S.d_gbin0, (int32_t)n, (int32_t)ng, S.d_bcur, nullptr, nullptr, 0};
        const unsigned row_blocks = (unsigned)((n + 255) / 256);
        const int p1 = prof_begin(c, "k_a2c_bin_count");
        hipLaunchKernelGGL(k_a2c_bin_count, dim3(row_blocks), dim3(256), 0, s, b);
        prof_end(c, p1);
        const int p2 = prof_begin(c, "k_a2c_bin_scan");
        hipLaunchKernelGGL(k_a2c_bin_scan, dim3(1), dim3(1024), 0, s, S.d_bcur, S.d_bstart, (int)nb);
        prof_end(c, p2);
        MH_HIP(hipGetLastError());
        std::vector<unsigned long long> start(nb + 1);
        MH_HIP(hipMemcpyAsync(start.data(), S.d_bstart, sizeof(unsigned long long) * (nb + 1),
                              hipMemcpyDeviceToHost, s));
        // the lists are filled from copies of the starts
        MH_HIP(hipMemcpyAsync(S.d_bcur, S.d_bstart, sizeof(unsigned long long) * (nb + 1),
                              hipMemcpyDeviceToDevice, s));
        MH_HIP(hipStreamSynchronize(s));
        std::vector<A2CChunk> chunks;
        for (int64_t g = 0; g < ng; ++g)
            for (int64_t bin = S.g_bin0[(size_t)g]; bin < S.g_bin0[(size_t)g + 1]; ++bin)
                for (int64_t i = (int64_t)start[(size_t)bin]; i < (int64_t)start[(size_t)bin + 1]; i += A2C_CHUNK)
                    chunks.push_back({(int32_t)bin, (int32_t)((bin - S.g_bin0[(size_t)g]) * A2C_W), i,
                                      std::min<int64_t>(i + A2C_CHUNK, (int64_t)start[(size_t)bin + 1])});
        n_chunks = chunks.size();
        if (int st = a2c_reserve(S, S.d_bin_rows, sizeof(int32_t) * (size_t)start[nb])) return st;
        if (int st = a2c_upload(S, S.d_chunks, chunks.data(), chunks.size(), s)) return st;
        b.cnt = nullptr;
        b.cur = S.d_bcur;
        b.bin_rows = S.d_bin_rows;
        b.total = start[nb];
        const int p3 = prof_begin(c, "k_a2c_bin_fill");
        hipLaunchKernelGGL(k_a2c_bin_fill, dim3(row_blocks), dim3(256), 0, s, b);
        prof_end(c, p3);
        MH_HIP(hipGetLastError());
    } else {
        S.t_parse = ms_since(t0);
        t1 = std::chrono::steady_clock::now();
    }
    if (int st = a2c_count_chunks(c, S, n_chunks)) return st;
    S.t_count = ms_since(t1);
    if (n_groups) *n_groups = ng;
    return 0;
}

extern "C" int mh_a2c_load_resident(mh_ctx *ctx, int slot, const char *codon_chars, int64_t *n_groups)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_inserts(S);
    S.counted = S.det_ready = false;
    if (S.part_text) {       // a part left open by a sharded load that fell back
        unmap_text_file(S.part_text, S.part_len);
        S.part_text = nullptr;
        S.part_open = false;
    }
    if (int st = a2c_tables(S, codon_chars)) return st;
    int st = 0;
    try {
        st = a2c_load_resident(c, S, n_groups);
    } catch (const std::exception &e) {
        set_error("mh_a2c_load_resident: out of memory (%s)", e.what());
        st = -2;
    }
    if (st) {                // nothing of a load that did not finish stands
        S.rows.clear();
        S.dev_rows = false;
        S.n_rows = 0;
        S.g_first.assign(1, 0);
        S.g_ref.clear();
        S.g_qcut.clear();
    }
    return st;
}

extern "C" int mh_a2c_load_rows(mh_ctx *ctx, int slot, int64_t n_rows, const char *pool,
                                int64_t pool_len, const int64_t *seq_off, const int32_t *seq_len,
                                const int64_t *offset, const int64_t *count, int64_t n_groups,
                                const int64_t *group_first, const char *codon_chars)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || n_rows < 0 || pool_len < 0 || n_groups < 0 ||
        (n_rows && (!pool || !seq_off || !seq_len || !offset || !count)) || !group_first)
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_inserts(S);
    S.counted = S.det_ready = false;
    auto t0 = std::chrono::steady_clock::now();
    if (int st = a2c_tables(S, codon_chars)) return st;
    if (group_first[0] != 0 || group_first[n_groups] != n_rows) {
        set_error("mh_a2c_load_rows: group_first must run from 0 to n_rows");
        return -3;
    }
    S.rows.assign(n_rows, A2CRow{});
    S.dev_rows = false;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (seq_off[r] < 0 || seq_len[r] < 0 || seq_off[r] + seq_len[r] > pool_len ||
            seq_len[r] > A2C_MAX_SPAN) {
            set_error("mh_a2c_load_rows: row %lld: seq outside the pool", (long long)r);
            return -3;
        }
        if (count[r] < 0 || count[r] > (int64_t)UINT32_MAX) {
            set_error("mh_a2c_load_rows: row %lld: count outside 0 .. 2**32-1", (long long)r);
            return -3;
        }
        if (offset[r] < 0 || offset[r] > A2C_MAX_SPAN) {
            set_error("mh_a2c_load_rows: row %lld: offset outside 0 .. 2**28", (long long)r);
            return -3;
        }
        for (int32_t k = 0; k < seq_len[r]; ++k) {
            const char ch = pool[seq_off[r] + k];
            if (S.cls[(uint8_t)ch] == A2C_BAD) {
                set_error("mh_a2c_load_rows: row %lld: character '%c' is not one of A C G T N - n",
                          (long long)r, ch);
                return -3;
            }
        }
        S.rows[r] = A2CRow{seq_off[r], seq_len[r], (int32_t)offset[r], (uint32_t)count[r], 0};
    }
    S.n_rows = n_rows;
    S.g_first.assign(group_first, group_first + n_groups + 1);
    for (int64_t g = 0; g < n_groups; ++g)
        if (group_first[g + 1] < group_first[g]) {
            set_error("mh_a2c_load_rows: group_first must not decrease");
            return -3;
        }
    S.g_ref.assign(n_groups, std::string());
    S.g_qcut.assign(n_groups, std::string());
    S.t_parse = ms_since(t0);
    auto t1 = std::chrono::steady_clock::now();
    if (int st = a2c_count(c, S, pool ? pool : "", pool_len)) {
        S.rows.clear();
        S.g_first.assign(1, 0);
        return st;
    }
    S.t_count = ms_since(t1);
    return 0;
}

extern "C" int mh_a2c_group(mh_ctx *ctx, int slot, int64_t g, int64_t *info5, char *names,
                            size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !info5) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_group: no group %lld", (long long)g); return -3; }
    info5[0] = S.g_first[g];
    info5[1] = S.g_first[g + 1] - S.g_first[g];
    for (int f = 0; f < 3; ++f) info5[2 + f] = S.g_ncod[3 * g + f];
    const std::string &r = S.g_ref[g], &q = S.g_qcut[g];
    const size_t need = r.size() + 1 + q.size();
    if (used) *used = need;
    if (names) {
        if (cap < need) { set_error("mh_a2c_group: buffer too small"); return -2; }
        memcpy(names, r.data(), r.size());
        names[r.size()] = '\0';
        memcpy(names + r.size() + 1, q.data(), q.size());
    }
    return 0;
}

extern "C" int mh_a2c_counts(mh_ctx *ctx, int slot, int64_t g, int frame, uint32_t *aa_count,
                             uint32_t *aa_first, uint32_t *nuc_count, uint32_t *nuc_first)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || frame < 0 || frame > 2) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_counts: no group %lld", (long long)g); return -3; }
    const int n = S.g_ncod[3 * g + frame];
    if (n && (!aa_count || !aa_first || !nuc_count || !nuc_first)) return -3;
    for (int j = 0; j < n; ++j) {
        const size_t at = (size_t)(S.g_bin0[g] + j / A2C_W) * A2C_CELLS +
                          (size_t)(A2C_W * frame + j % A2C_W) * A2C_STRIDE;
        memcpy(aa_count + (size_t)j * A2C_NAA, &S.h_cnt[at], 4 * A2C_NAA);
        memcpy(aa_first + (size_t)j * A2C_NAA, &S.h_first[at], 4 * A2C_NAA);
        memcpy(nuc_count + (size_t)j * 18, &S.h_cnt[at + A2C_NAA], 4 * 18);
        memcpy(nuc_first + (size_t)j * 18, &S.h_first[at + A2C_NAA], 4 * 18);
    }
    return 0;
}

extern "C" int mh_a2c_codon_detail(mh_ctx *ctx, int slot, int64_t g, int frame, uint32_t *xpd)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || frame < 0 || frame > 2) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    if (!S.counted) { set_error("mh_a2c_codon_detail: nothing is loaded in slot %d", slot); return -3; }
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_codon_detail: no group %lld", (long long)g); return -3; }
    const int n = S.g_ncod[3 * g + frame];
    if (n && !xpd) return -3;
    if (!S.det_ready) {
        MH_HIP(hipSetDevice(c.device));
        int st = 0;
        try {
            st = a2c_detail_run(c, S);
        } catch (const std::exception &e) {
            set_error("mh_a2c_codon_detail: out of memory (%s)", e.what());
            st = -2;
        }
        if (st) return st;
    }
    for (int j = 0; j < n; ++j) {
        const size_t at = (size_t)(S.g_bin0[g] + j / A2C_W) * A2C_DET_CELLS +
                          (size_t)(A2C_W * frame + j % A2C_W) * A2C_DET;
        memcpy(xpd + (size_t)j * A2C_DET, &S.h_det[at], 4 * A2C_DET);
    }
    return 0;
}

// mh_a2c_inserts past its checks: the entries of the group's np > 0 (range,
// row) pairs and their strings into S
static int a2c_inserts_run(Ctx &c, A2CState &S, int64_t g, int frame, int n_ranges,
                           const int32_t *left, const int32_t *right)
{
    static const char *const label[3] = {"k_a2c_ins", "k_a2c_ins", "k_a2c_ins"};
    const int64_t nr = S.g_first[g + 1] - S.g_first[g], np = nr * n_ranges;
    const unsigned pair_blocks = (unsigned)((np + 255) / 256);
    hipStream_t s = c.stream;
    A2CDevMem mem;
    A2CInsArgs a{};
    int32_t *d_lr;
    A2CDistinct *d_sorted;
    int64_t *d_eoff;
    char *d_out;
    unsigned long long ctr[3] = {0, 0, 0};
    std::vector<int32_t> lr(2 * (size_t)n_ranges);
    for (int k = 0; k < n_ranges; ++k) { lr[k] = left[k]; lr[n_ranges + k] = right[k]; }
    hipError_t e = mem.alloc(d_lr, lr.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_lr, lr.data(), sizeof(int32_t) * lr.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = mem.alloc(a.h, (size_t)np);
    if (e == hipSuccess) e = mem.alloc(a.ctr, 3);
    if (e == hipSuccess) e = hipMemsetAsync(a.ctr, 0, sizeof(ctr), s);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_inserts alloc");
    a.text = S.d_text;
    a.rows = S.d_rows + S.g_first[g];
    a.code = S.d_code;
    a.cls = S.d_cls;
    a.left = d_lr;
    a.right = d_lr + n_ranges;
    a.n_rows = nr;
    a.n_pairs = np;
    a.frame = frame;
    {
        const int p0 = prof_begin(c, label[0]);
        hipLaunchKernelGGL(k_a2c_ins_hash, dim3(pair_blocks), dim3(256), 0, s, a);
        prof_end(c, p0);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "k_a2c_ins_hash");
    if (ctr[0] == 0) return 0;
    if (int rc = a2c_group_strings(c, mem, a, ctr, k_a2c_ins_verify, pair_blocks, "mh_a2c_inserts", label,
                                   "aln2counts: insertion-string hash collision (distinct strings share a key)"))
        return rc;
    std::vector<A2CDistinct> ent(ctr[2]);
    e = copy_sync(c, ent.data(), a.entries, sizeof(A2CDistinct) * ent.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_inserts fetch");
    // InsertionWriter order: ranges in order, then Counter insertion order
    std::sort(ent.begin(), ent.end(), [](const A2CDistinct &x, const A2CDistinct &y) {
        return x.cls != y.cls ? x.cls < y.cls : x.first < y.first;
    });
    std::vector<int64_t> eoff(ent.size() + 1);
    eoff[0] = 0;
    for (size_t k = 0; k < ent.size(); ++k) eoff[k + 1] = eoff[k] + ent[k].len + 1;
    S.aminos.assign((size_t)eoff.back(), '\0');
    e = mem.alloc(d_sorted, ent.size());
    if (e == hipSuccess) e = mem.alloc(d_eoff, eoff.size());
    if (e == hipSuccess) e = mem.alloc(d_out, (size_t)eoff.back());
    if (e == hipSuccess) e = hipMemcpyAsync(d_sorted, ent.data(), sizeof(A2CDistinct) * ent.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_eoff, eoff.data(), sizeof(int64_t) * eoff.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_inserts gather");
    hipLaunchKernelGGL(k_a2c_ins_gather, dim3((unsigned)((ent.size() + 255) / 256)), dim3(256), 0, s,
                       a, d_sorted, d_eoff, (int64_t)ent.size(), d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&S.aminos[0], d_out, (size_t)eoff.back(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "k_a2c_ins_gather");
    // first rows leave as row numbers within the whole group.  This relies on
    // local being contiguous over a call's rows, rows[i].local ==
    // rows[0].local + i, as a2c_layout and mh_a2c_part_count number them (a
    // rank's part of a group starts at the rows of the ranks before; rows
    // built on the device are whole groups, from 0)
    const uint32_t base = S.dev_rows ? 0 : S.rows[(size_t)S.g_first[g]].local;
    for (A2CDistinct &x : ent) x.first += base;
    S.entries = std::move(ent);
    return 0;
}

extern "C" int mh_a2c_inserts(mh_ctx *ctx, int slot, int64_t g, int frame, int n_ranges,
                              const int32_t *left, const int32_t *right, int64_t *n_entries)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || frame < 0 || frame > 2 || n_ranges < 0 ||
        (n_ranges && (!left || !right)))
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_inserts(S);
    if (n_entries) *n_entries = 0;
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_inserts: no group %lld", (long long)g); return -3; }
    for (int k = 0; k < n_ranges; ++k)
        if (left[k] < 0 || right[k] < left[k] || right[k] > (1 << 27)) {
            set_error("mh_a2c_inserts: bad range %d..%d", left[k], right[k]);
            return -3;
        }
    if ((S.g_first[g + 1] - S.g_first[g]) * n_ranges == 0) return 0;
    auto t0 = std::chrono::steady_clock::now();
    const int rc = a2c_inserts_run(c, S, g, frame, n_ranges, left, right);
    prof_flush(c);
    S.t_ins += ms_since(t0);
    if (rc) a2c_clear_inserts(S);
    else if (n_entries) *n_entries = (int64_t)S.entries.size();
    return rc;
}

extern "C" int mh_a2c_insert_entries(mh_ctx *ctx, int slot, int32_t *range, int64_t *count,
                                     uint32_t *first, char *aminos, size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    for (size_t k = 0; k < S.entries.size(); ++k) {
        if (range) range[k] = S.entries[k].cls;
        if (count) count[k] = (int64_t)S.entries[k].count;
        if (first) first[k] = S.entries[k].first;
    }
    if (used) *used = S.aminos.size();
    if (aminos) {
        if (cap < S.aminos.size()) { set_error("mh_a2c_insert_entries: buffer too small"); return -2; }
        memcpy(aminos, S.aminos.data(), S.aminos.size());
    }
    return 0;
}

extern "C" int mh_a2c_insert_rows(mh_ctx *ctx, int slot, const char *lead, int n_ranges,
                                  const int32_t *left, const int32_t *target, const char *eol,
                                  char *buf, size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !lead || !eol || !used || n_ranges < 0 ||
        (n_ranges && (!left || !target)))
        return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    if (!buf) {
        // InsertionWriter.write's rows: lead, left codon + 1, the amino-acid
        // string, its count, the coordinate position (blank when none)
        std::string &o = S.ins_rows;
        o.clear();
        const size_t ll = strlen(lead), el = strlen(eol);
        o.reserve(S.entries.size() * (ll + el + 24) + S.aminos.size());
        const char *am = S.aminos.data(), *am_end = am + S.aminos.size();
        char num[24];
        auto put = [&](long long v) {
            auto r = std::to_chars(num, num + sizeof num, v);
            o.append(num, (size_t)(r.ptr - num));
        };
        for (size_t k = 0; k < S.entries.size(); ++k) {
            const char *nl = (const char *)memchr(am, '\n', (size_t)(am_end - am));
            if (!nl) { set_error("mh_a2c_insert_rows: entry strings out of step"); return -3; }
            const int r = S.entries[k].cls;
            if (r < 0 || r >= n_ranges) { set_error("mh_a2c_insert_rows: range %d out of %d", r, n_ranges); return -3; }
            o.append(lead, ll);
            put((long long)left[r] + 1);
            o.push_back(',');
            o.append(am, (size_t)(nl - am));
            o.push_back(',');
            put((long long)S.entries[k].count);
            o.push_back(',');
            if (target[r] != INT32_MIN) put(target[r]);
            o.append(eol, el);
            am = nl + 1;
        }
        *used = o.size();
        return 0;
    }
    *used = S.ins_rows.size();
    if (cap < S.ins_rows.size()) { set_error("mh_a2c_insert_rows: buffer too small"); return -2; }
    memcpy(buf, S.ins_rows.data(), S.ins_rows.size());
    std::string().swap(S.ins_rows);
    return 0;
}

extern "C" int mh_a2c_timing(mh_ctx *ctx, int slot, double *ms3)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !ms3) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    ms3[0] = S.t_parse;
    ms3[1] = S.t_count;
    ms3[2] = S.t_ins;
    S.t_ins = 0;
    return 0;
}

// ---------------------------------------------------------------------------
// aln2counts split over the ranks of a job.  The reference counts every row
// of aligned.csv into per-(refname, qcut) Counters (aln2counts.py:115-172),
// in file order; the counts are sums and the first row a Counter saw is a
// minimum, so rank r counts the rows in its share of the file's bytes and
// the caller adds the ranks' counters up (and takes the minimum of their
// first rows): mh_a2c_part_open parses the share, mh_a2c_part_groups reports
// its runs of (refname, qcut), mh_a2c_part_count lays out the job's groups
// (codon extents, row numbers within a group from the ranks before) and
// counts, mh_a2c_part_counters hands the counters out and takes the sums
// back.  The insertion strings of InsertionWriter.write (:786-795) are the
// same kind of reduction: mh_a2c_insert_export / mh_a2c_insert_merge.
// ---------------------------------------------------------------------------
static int64_t a2c_line_start(const char *t, int64_t lo, int64_t hi, int64_t x)
{
    if (x <= lo) return lo;
    if (x >= hi) return hi;
    if (t[x - 1] == '\n') return x;
    const char *q = (const char *)memchr(t + x, '\n', (size_t)(hi - x));
    return q ? (q - t) + 1 : hi;
}

extern "C" int mh_a2c_part_open(mh_ctx *ctx, int slot, int fd, int part, int parts,
                                const char *codon_chars, int64_t *info3)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || fd < 0 || parts < 1 || part < 0 || part >= parts ||
        !info3)
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_inserts(S);
    S.counted = S.det_ready = false;
    if (S.part_text) { unmap_text_file(S.part_text, S.part_len); S.part_text = nullptr; }
    S.part_open = false;
    if (int st = a2c_tables(S, codon_chars)) return st;
    const char *text = nullptr;
    size_t len = 0;
    if (int st = map_text_file(fd, &text, &len)) return st;   // 1: '\r' in it
    auto t0 = std::chrono::steady_clock::now();
    const char *p = text, *end = text + len;
    std::vector<std::string> head;
    int64_t lo = 0, hi = (int64_t)len;
    if (csv_record(p, end, head)) lo = p - text;
    const int64_t b0 = a2c_line_start(text, lo, hi, lo + (hi - lo) * part / parts);
    const int64_t b1 = a2c_line_start(text, lo, hi, lo + (hi - lo) * (part + 1) / parts);
    // a quoted field (a refname with a comma) is parsed on one thread into a
    // pool; the split is kept to unquoted files
    if (memchr(text + b0, '"', (size_t)(b1 - b0))) { unmap_text_file(text, len); return 1; }
    bool use_pool = false;
    int st = 0;
    try {
        st = a2c_parse_csv(S, text, (int64_t)len, use_pool, b0, b1);
    } catch (const std::exception &e) {
        set_error("aligned csv: out of memory (%s)", e.what());
        st = -2;
    }
    if (st || use_pool) {
        unmap_text_file(text, len);
        S.rows.clear();
        S.g_first.assign(1, 0);
        return st ? st : 1;
    }
    S.part_text = text;
    S.part_len = len;
    S.part_open = true;
    S.part_b0 = b0;
    S.part_b1 = b1;
    S.part_first = S.g_first;
    S.t_parse = ms_since(t0);
    info3[0] = S.n_rows;
    info3[1] = (int64_t)S.g_first.size() - 1;
    info3[2] = b1 - b0;
    return 0;
}

extern "C" int mh_a2c_part_groups(mh_ctx *ctx, int slot, char *keys, size_t cap, size_t *used,
                                  int64_t *rows, int32_t *ncod3, int64_t *total)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !used) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    const int64_t ng = (int64_t)S.part_first.size() - 1;
    size_t need = 0;
    for (int64_t g = 0; g < ng; ++g) need += S.g_ref[g].size() + S.g_qcut[g].size() + 2;
    *used = need;
    if (!keys) return 0;
    if (cap < need || !rows || !ncod3 || !total) { set_error("mh_a2c_part_groups: buffer too small"); return -2; }
    for (int64_t g = 0; g < ng; ++g) {
        memcpy(keys, S.g_ref[g].data(), S.g_ref[g].size());
        keys += S.g_ref[g].size();
        *keys++ = '\x1f';
        memcpy(keys, S.g_qcut[g].data(), S.g_qcut[g].size());
        keys += S.g_qcut[g].size();
        *keys++ = '\n';
        int32_t nc[3] = {0, 0, 0};
        uint64_t tot = 0;
        for (int64_t r = S.part_first[g]; r < S.part_first[g + 1]; ++r) {
            const A2CRow &R = S.rows[r];
            tot += R.cnt;
            const int l = R.off / 3;
            for (int f = 0; f < 3; ++f) {
                const int h = (f + R.off + R.len + 2) / 3;
                if (h > l && h > nc[f]) nc[f] = h;
            }
        }
        rows[g] = S.part_first[g + 1] - S.part_first[g];
        for (int f = 0; f < 3; ++f) ncod3[3 * g + f] = nc[f];
        total[g] = (int64_t)tot;
    }
    return 0;
}

extern "C" int mh_a2c_part_count(mh_ctx *ctx, int slot, int64_t n_groups, const char *keys,
                                 const int64_t *gid, const int32_t *ncod3, const int64_t *row_base,
                                 int64_t *cells)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || n_groups < 0 || (n_groups && (!keys || !ncod3)) ||
        !cells)
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    if (!S.part_open) { set_error("mh_a2c_part_count: no part open"); return -3; }
    const int64_t nl = (int64_t)S.part_first.size() - 1;
    if (nl && (!gid || !row_base)) return -3;
    for (int64_t k = 0; k < nl; ++k)
        if (gid[k] < 0 || gid[k] >= n_groups || (k && gid[k] <= gid[k - 1])) {
            set_error("mh_a2c_part_count: group ids out of order");
            return -3;
        }
    // the job's groups, this part's rows in them (global row numbers within
    // a group for the first-row counters)
    std::vector<std::string> ref, qcut;
    const char *p = keys;
    for (int64_t g = 0; g < n_groups; ++g) {
        const char *us = strchr(p, '\x1f'), *nlp = us ? strchr(us, '\n') : nullptr;
        if (!us || !nlp) { set_error("mh_a2c_part_count: malformed group keys"); return -3; }
        ref.emplace_back(p, (size_t)(us - p));
        qcut.emplace_back(us + 1, (size_t)(nlp - us - 1));
        p = nlp + 1;
    }
    std::vector<int64_t> first((size_t)n_groups + 1, 0);
    {
        int64_t k = 0, at = 0;
        for (int64_t g = 0; g < n_groups; ++g) {
            first[(size_t)g] = at;
            if (k < nl && gid[k] == g) {
                for (int64_t r = S.part_first[k]; r < S.part_first[k + 1]; ++r)
                    S.rows[r].local = (uint32_t)(row_base[k] + (r - S.part_first[k]));
                at = S.part_first[k + 1];
                ++k;
            }
        }
        first[(size_t)n_groups] = at;
    }
    S.g_first.swap(first);
    S.g_ref.swap(ref);
    S.g_qcut.swap(qcut);
    S.g_ncod.assign(ncod3, ncod3 + 3 * n_groups);
    auto t1 = std::chrono::steady_clock::now();
    int st = 0;
    try {
        // only the part's bytes go to the device: row offsets from b0
        for (A2CRow &R : S.rows) R.soff -= S.part_b0;
        st = a2c_count(c, S, S.part_text + S.part_b0, S.part_b1 - S.part_b0, true);
    } catch (const std::exception &e) {
        set_error("aln2counts: out of memory (%s)", e.what());
        st = -2;
    }
    unmap_text_file(S.part_text, S.part_len);
    S.part_text = nullptr;
    S.part_len = 0;
    S.part_open = false;
    if (st) {
        S.rows.clear();
        S.g_first.assign(1, 0);
        return st;
    }
    S.t_count = ms_since(t1);
    *cells = (int64_t)S.h_cnt.size();
    return 0;
}

extern "C" int mh_a2c_part_counters(mh_ctx *ctx, int slot, int set, uint32_t *cnt, uint32_t *first)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !cnt || !first) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    const size_t n = S.h_cnt.size();
    if (set) {
        memcpy(S.h_cnt.data(), cnt, 4 * n);
        memcpy(S.h_first.data(), first, 4 * n);
    } else {
        memcpy(cnt, S.h_cnt.data(), 4 * n);
        memcpy(first, S.h_first.data(), 4 * n);
    }
    return 0;
}

// insertion entries on the wire: range, first row, codons, string length,
// count, then the string, padded to 8
struct A2CWireEntry {
    int32_t range;
    uint32_t first;
    int32_t n_codons;
    int32_t slen;
    unsigned long long count;
};

extern "C" int mh_a2c_insert_export(mh_ctx *ctx, int slot, uint8_t *buf, size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !used) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    size_t need = 0;
    const char *am = S.aminos.data(), *am_end = am + S.aminos.size();
    std::vector<std::pair<const char *, size_t>> str;
    for (size_t k = 0; k < S.entries.size(); ++k) {
        const char *nl = (const char *)memchr(am, '\n', (size_t)(am_end - am));
        if (!nl) { set_error("mh_a2c_insert_export: entry strings out of step"); return -3; }
        str.emplace_back(am, (size_t)(nl - am));
        need += sizeof(A2CWireEntry) + ((str.back().second + 7) & ~(size_t)7);
        am = nl + 1;
    }
    *used = need;
    if (!buf) return 0;
    if (cap < need) { set_error("mh_a2c_insert_export: buffer too small"); return -2; }
    memset(buf, 0, need);
    for (size_t k = 0; k < S.entries.size(); ++k) {
        const A2CDistinct &e = S.entries[k];
        A2CWireEntry w{e.cls, e.first, e.len, (int32_t)str[k].second, e.count};
        memcpy(buf, &w, sizeof w);
        memcpy(buf + sizeof w, str[k].first, str[k].second);
        buf += sizeof w + ((str[k].second + 7) & ~(size_t)7);
    }
    return 0;
}

// every rank's entries of one insertion call: equal (range, string) added
// up, the first row the least, in (range, first row) order
extern "C" int mh_a2c_insert_merge(mh_ctx *ctx, int slot, const uint8_t *buf, int64_t len,
                                   int64_t *n_entries)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || (!buf && len) || len < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    std::map<std::pair<int32_t, std::string>, A2CDistinct> merged;
    int64_t at = 0;
    while (at < len) {
        if (len - at < (int64_t)sizeof(A2CWireEntry)) { set_error("mh_a2c_insert_merge: malformed"); return -3; }
        A2CWireEntry w;
        memcpy(&w, buf + at, sizeof w);
        const int64_t sz = (int64_t)(sizeof w + (((size_t)w.slen + 7) & ~(size_t)7));
        if (w.slen < 0 || len - at < sz) { set_error("mh_a2c_insert_merge: malformed"); return -3; }
        std::string key((const char *)buf + at + sizeof w, (size_t)w.slen);
        auto it = merged.find({w.range, key});
        if (it == merged.end()) {
            merged.emplace(std::make_pair(w.range, std::move(key)), A2CDistinct{w.range, w.first, w.n_codons, 0, w.count});
        } else {
            it->second.count += w.count;
            it->second.first = std::min(it->second.first, w.first);
        }
        at += sz;
    }
    std::vector<std::pair<const std::string *, A2CDistinct>> v;
    for (auto &kv : merged) v.push_back({&kv.first.second, kv.second});
    std::sort(v.begin(), v.end(), [](const auto &x, const auto &y) {
        return x.second.cls != y.second.cls ? x.second.cls < y.second.cls
                                                : x.second.first < y.second.first;
    });
    S.entries.clear();
    S.aminos.clear();
    for (auto &x : v) {
        S.entries.push_back(x.second);
        S.aminos += *x.first;
        S.aminos.push_back('\n');
    }
    if (n_entries) *n_entries = (int64_t)S.entries.size();
    return 0;
}

// ---------------------------------------------------------------------------
// Nucleotide variants of the coordinate regions of one run: the loop
// SequenceReport.read runs per region over every row (aln2counts.py:346-375)
// and the report write_nuc_variants (:537-549) was meant to write.  Per
// (region, row) the row padded with '-' to its offset is clipped to the
// region's window [start, end) (Python slice rules), kept when twice its
// bytes other than '-' exceed the coordinate reference's length, and equal
// clipped sequences (byte identity, the length included) add their counts up.
// A region's report is its max_variants largest by (count, sequence).
//   k_a2c_var_hash     a wavefront per pair: the lanes stride the window 64
//                      bytes at a time (the padding is synthesised), each
//                      keeps the sum of a per-(position, byte) mix and the
//                      wave adds the sums up; the length and the region go
//                      into the key.  A pair whose row cannot hold enough
//                      bytes of the window is rejected before any is read.
//   k_a2c_tab_count    (shared with the insertion strings, profiled here as
//                      k_a2c_var_count) the keys grouped: count and first row.
//   k_a2c_var_verify   a wavefront per pair: its window against the window
//                      of its entry's first row, byte for byte; a mismatch is
//                      an error of the call, never a merged count.
//   k_a2c_tab_compact  (shared, profiled as k_a2c_var_compact) the occupied
//                      slots as entries.
//   k_a2c_var_select   a block per (slice of entries, region), max_variants
//                      rounds: the largest count among the entries not kept
//                      yet, then among the entries tied at it the greatest
//                      sequence by successive 8-byte big-endian chunks (bytes
//                      past the end are 0, so a proper prefix sorts below the
//                      longer one).  A region's greatest entries are among
//                      its slices' greatest, so a second launch of a block
//                      per region picks from those.  The cut, ties included,
//                      is decided here: only fixed-size records of the kept
//                      entries go to the host.
//   k_a2c_var_tied     how many entries share a region's last kept count (the
//                      "tied at the cut" figure of the stats).
//   k_a2c_var_gather   the text of the kept entries, padding materialised.
// ---------------------------------------------------------------------------
namespace mh {

constexpr int A2C_VAR_SLICE = 2048;      // entries a block of the first selection level takes

struct A2CVarArgs : A2CTable {
    const uint8_t *text;
    const int64_t *win;          // per region: start, end, reference length, max_variants
    int key_bits;
};

// clipped = ('-' * off + seq)[start:end]: padded positions [lo, hi)
__device__ __forceinline__ void a2c_var_clip(const A2CRow &R, int64_t start, int64_t end,
                                             int64_t &lo, int64_t &hi)
{
    const int64_t L = (int64_t)R.off + R.len;
    lo = start < L ? start : L;
    hi = end < L ? end : L;
    if (hi < lo) hi = lo;
}

// the byte at padded position pos < off + len
__device__ __forceinline__ uint32_t a2c_var_byte(const uint8_t *text, const A2CRow &R, int64_t pos)
{
    return pos < R.off ? (uint32_t)'-' : (uint32_t)text[R.soff + (pos - R.off)];
}

__global__ __launch_bounds__(256) void k_a2c_var_hash(A2CVarArgs A)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    unsigned long long kept = 0;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < A.n_pairs; p += n_waves) {
        const int rg = (int)(p / A.n_rows);
        const A2CRow R = A.rows[p % A.n_rows];
        const int64_t *w = A.win + 4 * rg;
        int64_t lo, hi;
        a2c_var_clip(R, w[0], w[1], lo, hi);
        const int64_t rlo = lo > R.off ? lo : R.off;     // the read's own bytes: [rlo, hi)
        uint64_t key = 0;
        if (2 * (hi - rlo) > w[2]) {
            uint64_t part = 0;
            int64_t bases = 0;
            for (int64_t q0 = lo; q0 < hi; q0 += 64) {
                const int64_t q = q0 + lane;
                const bool in = q < hi;
                const uint32_t ch = in ? a2c_var_byte(A.text, R, q) : (uint32_t)'-';
                if (in) part += a2c_mix(((uint64_t)(q - lo) << 8) | ch);
                bases += __popcll(__ballot(in && ch != (uint32_t)'-'));
            }
            if (2 * bases > w[2]) {
                part = a2c_wave_sum(part);
                const uint64_t h = a2c_mix(part ^ a2c_mix(((uint64_t)(hi - lo) << 20) ^ (uint64_t)rg));
                key = A.key_bits >= 64 ? (h | 1ull) : (((h & ((1ull << A.key_bits) - 1)) << 1) | 1ull);
                ++kept;
            }
        }
        if (lane == 0) A.h[p] = key;
    }
    if (lane == 0 && kept) atomicAdd(&A.ctr[0], kept);
}

__global__ __launch_bounds__(256) void k_a2c_var_verify(A2CVarArgs A)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    unsigned long long wrong = 0;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < A.n_pairs; p += n_waves) {
        const uint64_t h = A.h[p];
        if (!h) continue;
        const int rg = (int)(p / A.n_rows);
        const uint32_t idx = (uint32_t)(p % A.n_rows);
        const uint64_t s = table_find(A.tkey, A.mask, a2c_slot(h, A.mask), h);
        const uint32_t fidx = A.tfirst[s];
        bool bad = A.tclass[s] != rg;
        if (!bad && fidx != idx) {
            const A2CRow R = A.rows[idx], F = A.rows[fidx];
            const int64_t *w = A.win + 4 * rg;
            int64_t lo, hi, flo, fhi;
            a2c_var_clip(R, w[0], w[1], lo, hi);
            a2c_var_clip(F, w[0], w[1], flo, fhi);
            bad = hi - lo != fhi - flo;
            if (!bad)
                for (int64_t i = lane; i < hi - lo; i += 64)
                    bad = bad || a2c_var_byte(A.text, R, lo + i) != a2c_var_byte(A.text, F, flo + i);
        }
        if (__any(bad)) ++wrong;
    }
    if (lane == 0 && wrong) atomicAdd(&A.ctr[1], wrong);
}

// the bytes of an entry's clipped sequence (k_a2c_tab_compact)
__device__ __forceinline__ int a2c_entry_len(const A2CVarArgs &A, int rg, uint32_t first)
{
    int64_t lo, hi;
    a2c_var_clip(A.rows[first], A.win[4 * rg], A.win[4 * rg + 1], lo, hi);
    return (int)(hi - lo);
}

// bytes [j, j + 8) of an entry's clipped sequence, big-endian, 0 past its end
__device__ uint64_t a2c_var_chunk(const A2CVarArgs &A, const A2CDistinct &e, int64_t j)
{
    const A2CRow F = A.rows[e.first];
    int64_t lo, hi;
    a2c_var_clip(F, A.win[4 * e.cls], A.win[4 * e.cls + 1], lo, hi);
    uint64_t key = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b)
        key = (key << 8) | (j + b < e.len ? (uint64_t)a2c_var_byte(A.text, F, lo + j + b) : 0ull);
    return key;
}

// The greatest entries of region blockIdx.y among src[b0, b1), in order, into
// out + slot * cap (slot = region * gridDim.x + blockIdx.x), at most
// min(max_variants, cap) of them.  Two levels: every slice of A2C_VAR_SLICE
// entries keeps its own greatest (gridDim.x slices, seg_stride 0); the
// region's greatest are among those, so one block per region then picks from
// the slices' picks (gridDim.x 1, the region's segment of seg_stride
// entries; unused places hold region -1).  state per entry: 0 free, 1 kept,
// 2 tied at the round's count and still the greatest on every chunk compared.
__global__ __launch_bounds__(1024) void k_a2c_var_select(A2CVarArgs A, const A2CDistinct *src, int64_t n_src,
                                                         int64_t slice, int64_t seg_stride, uint8_t *state,
                                                         int64_t cap, A2CDistinct *out, int32_t *n_out,
                                                         unsigned long long *last_out)
{
    __shared__ unsigned long long s_best, s_key;
    __shared__ unsigned int s_has, s_alive, s_pick;
    const int rg = blockIdx.y, tid = threadIdx.x;
    const int64_t b0 = (int64_t)rg * seg_stride + (int64_t)blockIdx.x * slice;
    const int64_t b1 = b0 + slice < n_src ? b0 + slice : n_src;
    const int64_t slot = (int64_t)rg * gridDim.x + blockIdx.x;
    const int64_t m = A.win[4 * rg + 3] < cap ? A.win[4 * rg + 3] : cap;
    int64_t got = 0;
    unsigned long long last = 0;
    for (; got < m; ++got) {
        if (tid == 0) { s_best = 0; s_has = 0; s_alive = 0; }
        __syncthreads();
        unsigned long long best = 0;
        bool has = false;
        for (int64_t e = b0 + tid; e < b1; e += 1024)
            if (src[e].cls == rg && state[e] != 1) {
                has = true;
                best = src[e].count > best ? src[e].count : best;
            }
        if (has) {
            atomicMax(&s_best, best);
            s_has = 1;
        }
        __syncthreads();
        if (!s_has) break;
        best = s_best;
        unsigned int n = 0;
        for (int64_t e = b0 + tid; e < b1; e += 1024)
            if (src[e].cls == rg && state[e] != 1) {
                const bool tied = src[e].count == best;
                state[e] = tied ? 2 : 0;
                n += tied;
            }
        if (n) atomicAdd(&s_alive, n);
        __syncthreads();
        unsigned int alive = s_alive;
        for (int64_t j = 0; alive > 1; j += 8) {
            __syncthreads();
            if (tid == 0) { s_key = 0; s_alive = 0; }
            __syncthreads();
            unsigned long long top = 0;
            for (int64_t e = b0 + tid; e < b1; e += 1024)
                if (state[e] == 2 && src[e].cls == rg) {
                    const unsigned long long k = a2c_var_chunk(A, src[e], j);
                    top = k > top ? k : top;
                }
            if (top) atomicMax(&s_key, top);
            __syncthreads();
            top = s_key;
            n = 0;
            for (int64_t e = b0 + tid; e < b1; e += 1024)
                if (state[e] == 2 && src[e].cls == rg) {
                    if (a2c_var_chunk(A, src[e], j) == top) ++n;
                    else state[e] = 0;
                }
            if (n) atomicAdd(&s_alive, n);
            __syncthreads();
            alive = s_alive;
            if (top == 0) break;      // every one ended: equal sequences (one entry each: not reached)
        }
        __syncthreads();
        if (tid == 0) s_pick = 0xffffffffu;
        __syncthreads();
        for (int64_t e = b0 + tid; e < b1; e += 1024)
            if (state[e] == 2 && src[e].cls == rg) atomicMin(&s_pick, (unsigned int)(e - b0));
        __syncthreads();
        const int64_t pick = b0 + s_pick;
        for (int64_t e = b0 + tid; e < b1; e += 1024)
            if (state[e] == 2 && src[e].cls == rg) state[e] = e == pick ? 1 : 0;
        if (tid == 0) out[slot * cap + got] = src[pick];
        last = best;
        __syncthreads();
    }
    if (tid == 0) {
        n_out[slot] = (int32_t)got;
        last_out[slot] = last;
    }
}

// eq[region] = entries of the region whose count is last[region] (the count
// of its last kept entry): more of them than were kept means the cut fell
// inside a tie.  One atomic per wave and region met.
__global__ __launch_bounds__(256) void k_a2c_var_tied(A2CVarArgs A, int64_t n_ent,
                                                      const unsigned long long *last,
                                                      unsigned long long *eq)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int rg = -1;
    if (e < n_ent && A.entries[e].count == last[A.entries[e].cls]) rg = A.entries[e].cls;
    for (;;) {
        const unsigned long long act = __ballot(rg >= 0);
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const int r = __shfl(rg, leader);
        const unsigned long long same = __ballot(rg == r);
        if (lane == leader) atomicAdd(&eq[r], (unsigned long long)__popcll(same));
        if (rg == r) rg = -1;
    }
}

// a wavefront per kept entry: its clipped sequence at out + off[k]
__global__ __launch_bounds__(256) void k_a2c_var_gather(A2CVarArgs A, const A2CDistinct *kept,
                                                        const int64_t *off, int64_t n, char *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const A2CDistinct e = kept[k];
    const A2CRow F = A.rows[e.first];
    int64_t lo, hi;
    a2c_var_clip(F, A.win[4 * e.cls], A.win[4 * e.cls + 1], lo, hi);
    for (int64_t i = lane; i < e.len; i += 64) out[off[k] + i] = (char)a2c_var_byte(A.text, F, lo + i);
}

}  // namespace mh

// mh_a2c_variants past its checks: win / which are the na regions with a cut
// above 0 (four values each; the caller's index of each), np > 0 pairs
static int a2c_variants_run(Ctx &c, A2CState &S, int64_t g, const std::vector<int64_t> &win,
                            const std::vector<int32_t> &which, int key_bits, int64_t *n_kept)
{
    static const char *const label[3] = {"k_a2c_var_count", "k_a2c_var_verify", "k_a2c_var_compact"};
    const int na = (int)which.size();
    const int64_t nr = S.g_first[g + 1] - S.g_first[g], np = nr * na;
    hipStream_t s = c.stream;
    A2CDevMem mem;
    int64_t *d_win, *d_toff;
    unsigned long long *d_last;
    int32_t *d_nkept;
    A2CDistinct *d_kept, *d_cand = nullptr;
    uint8_t *d_state;
    char *d_out;
    A2CVarArgs a{};
    unsigned long long ctr[3] = {0, 0, 0};
    std::vector<int64_t> toff;
    std::vector<unsigned long long> last_eq;    // per region: its last kept count, entries with it
    int64_t cap2 = 0;                           // places per region in kept
    std::vector<int32_t> nk((size_t)na, 0);
    std::vector<A2CDistinct> kept;
    const unsigned wave_blocks = (unsigned)std::min<int64_t>((np + 3) / 4, 8192);
    hipError_t e = mem.alloc(d_win, win.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_win, win.data(), sizeof(int64_t) * win.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = mem.alloc(a.h, (size_t)np);
    if (e == hipSuccess) e = mem.alloc(a.ctr, 3);
    if (e == hipSuccess) e = hipMemsetAsync(a.ctr, 0, sizeof(ctr), s);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_variants alloc");
    a.text = S.d_text;
    a.rows = S.d_rows + S.g_first[g];
    a.win = d_win;
    a.n_rows = nr;
    a.n_pairs = np;
    a.key_bits = key_bits;
    {
        const int p0 = prof_begin(c, "k_a2c_var_hash");
        hipLaunchKernelGGL(k_a2c_var_hash, dim3(wave_blocks), dim3(256), 0, s, a);
        prof_end(c, p0);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "k_a2c_var_hash");
    S.var_stats[0] = (int64_t)ctr[0];
    if (ctr[0] == 0) return 0;
    if (int rc = a2c_group_strings(c, mem, a, ctr, k_a2c_var_verify, wave_blocks, "mh_a2c_variants", label,
                                   "aln2counts: variant hash collision (distinct clipped sequences share a key)"))
        return rc;
    S.var_stats[1] = (int64_t)ctr[2];
    // ---- the cut: every slice's greatest entries, then each region's among those ----
    {
        const int64_t n_ent = (int64_t)ctr[2];
        int64_t most = 0;
        for (int k = 0; k < na; ++k) most = std::max(most, win[4 * (size_t)k + 3]);
        const int64_t n_slices = (n_ent + A2C_VAR_SLICE - 1) / A2C_VAR_SLICE;
        const int64_t cap1 = std::min<int64_t>(most, A2C_VAR_SLICE), seg = n_slices * cap1;
        const int64_t n_cand = n_slices > 1 ? (int64_t)na * seg : 0;
        cap2 = std::min<int64_t>(most, n_slices > 1 ? seg : n_ent);
        const size_t slots = (size_t)na * (size_t)std::max<int64_t>(n_slices, 1);
        e = mem.alloc(d_state, (size_t)(n_ent + n_cand));
        if (e == hipSuccess) e = hipMemsetAsync(d_state, 0, (size_t)(n_ent + n_cand), s);
        if (e == hipSuccess) e = mem.alloc(d_kept, (size_t)na * (size_t)cap2);
        if (e == hipSuccess) e = mem.alloc(d_nkept, 2 * slots);
        if (e == hipSuccess) e = mem.alloc(d_last, 2 * slots + (size_t)na);
        if (e == hipSuccess) e = hipMemsetAsync(d_last, 0, sizeof(unsigned long long) * (2 * slots + (size_t)na), s);
        if (e == hipSuccess && n_cand) e = mem.alloc(d_cand, (size_t)n_cand);
        if (e == hipSuccess && n_cand) e = hipMemsetAsync(d_cand, 0xff, sizeof(A2CDistinct) * (size_t)n_cand, s);
        if (e != hipSuccess) return hip_fail(e, "mh_a2c_variants select");
        // d_nkept / d_last: [0, slots) the regions' results, [slots, 2 slots) the slices'
        const int p0 = prof_begin(c, "k_a2c_var_select");
        if (n_slices > 1) {
            hipLaunchKernelGGL(k_a2c_var_select, dim3((unsigned)n_slices, (unsigned)na), dim3(1024), 0, s, a,
                               a.entries, n_ent, (int64_t)A2C_VAR_SLICE, (int64_t)0, d_state, cap1, d_cand,
                               d_nkept + slots, d_last + slots);
            hipLaunchKernelGGL(k_a2c_var_select, dim3(1, (unsigned)na), dim3(1024), 0, s, a, d_cand, n_cand,
                               seg, seg, d_state + n_ent, cap2, d_kept, d_nkept, d_last);
        } else {
            hipLaunchKernelGGL(k_a2c_var_select, dim3(1, (unsigned)na), dim3(1024), 0, s, a, a.entries, n_ent,
                               n_ent, (int64_t)0, d_state, cap2, d_kept, d_nkept, d_last);
        }
        prof_end(c, p0);
        const int p1 = prof_begin(c, "k_a2c_var_tied");
        hipLaunchKernelGGL(k_a2c_var_tied, dim3((unsigned)((n_ent + 255) / 256)), dim3(256), 0, s, a, n_ent,
                           d_last, d_last + 2 * slots);
        prof_end(c, p1);
        e = hipGetLastError();
        kept.resize((size_t)na * (size_t)cap2);
        last_eq.resize(2 * (size_t)na);
        if (e == hipSuccess) e = hipMemcpyAsync(nk.data(), d_nkept, sizeof(int32_t) * (size_t)na, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && !kept.empty())
            e = hipMemcpyAsync(kept.data(), d_kept, sizeof(A2CDistinct) * kept.size(), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(last_eq.data(), d_last, sizeof(unsigned long long) * (size_t)na, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(last_eq.data() + na, d_last + 2 * slots, sizeof(unsigned long long) * (size_t)na, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "k_a2c_var_select");
    }
    // ---- the kept entries' text: their summed lengths and nothing else ----
    {
        std::vector<A2CDistinct> order;
        for (int k = 0; k < na; ++k) {
            if (nk[(size_t)k] < 0 || nk[(size_t)k] > cap2) {
                set_error("mh_a2c_variants: the selection is inconsistent");
                return -3;
            }
            int64_t at_last = 0;
            for (int32_t i = 0; i < nk[(size_t)k]; ++i) {
                order.push_back(kept[(size_t)k * (size_t)cap2 + i]);
                S.var_region.push_back(which[(size_t)k]);
                at_last += order.back().count == last_eq[(size_t)k];
            }
            // a cut inside a tie: entries left out that share the last kept count
            if (nk[(size_t)k] == win[4 * (size_t)k + 3] && (int64_t)last_eq[(size_t)na + k] > at_last)
                S.var_stats[2] += (int64_t)last_eq[(size_t)na + k];
            if (n_kept) n_kept[which[(size_t)k]] = nk[(size_t)k];
        }
        toff.assign(order.size() + 1, 0);
        for (size_t k = 0; k < order.size(); ++k) toff[k + 1] = toff[k] + order[k].len;
        S.var_text.assign((size_t)toff.back(), '\0');
        if (toff.back() > 0) {
            e = mem.alloc(d_toff, toff.size());
            if (e == hipSuccess) e = mem.alloc(d_out, (size_t)toff.back());
            if (e == hipSuccess) e = hipMemcpyAsync(d_toff, toff.data(), sizeof(int64_t) * toff.size(), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_kept, order.data(), sizeof(A2CDistinct) * order.size(), hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "mh_a2c_variants gather");
            const int p0 = prof_begin(c, "k_a2c_var_gather");
            hipLaunchKernelGGL(k_a2c_var_gather, dim3((unsigned)((order.size() + 3) / 4)), dim3(256), 0, s,
                               a, d_kept, d_toff, (int64_t)order.size(), d_out);
            prof_end(c, p0);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&S.var_text[0], d_out, (size_t)toff.back(), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hip_fail(e, "k_a2c_var_gather");
            S.var_stats[3] = toff.back();
        }
        S.var_entries = std::move(order);
    }
    return 0;
}

extern "C" int mh_a2c_variants(mh_ctx *ctx, int slot, int64_t g, int n_regions, const int64_t *start,
                               const int64_t *end, const int64_t *ref_len, const int64_t *max_variants,
                               int key_bits, int64_t *n_kept)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || n_regions < 1 || !start || !end || !ref_len ||
        !max_variants || key_bits < 8 || key_bits > 64)
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    S.var_entries.clear();
    S.var_region.clear();
    S.var_text.clear();
    for (int k = 0; k < 4; ++k) S.var_stats[k] = 0;
    S.t_var = 0;
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_variants: no group %lld", (long long)g); return -3; }
    std::vector<int64_t> win;       // the regions with a cut above 0
    std::vector<int32_t> which;
    for (int k = 0; k < n_regions; ++k) {
        if (start[k] < 0 || end[k] < 0 || ref_len[k] < 0 || max_variants[k] < 0 ||
            start[k] > 4 * A2C_MAX_SPAN || end[k] > 4 * A2C_MAX_SPAN) {
            set_error("mh_a2c_variants: bad window %lld..%lld of region %d", (long long)start[k],
                      (long long)end[k], k);
            return -3;
        }
        if (n_kept) n_kept[k] = 0;
        if (max_variants[k] == 0) continue;
        which.push_back(k);
        win.insert(win.end(), {start[k], end[k], ref_len[k], max_variants[k]});
    }
    const int64_t np = (S.g_first[g + 1] - S.g_first[g]) * (int64_t)which.size();
    if (np == 0) return 0;
    if (np >= (int64_t)1 << 32) { set_error("mh_a2c_variants: more than 2**32 (region, row) pairs"); return -3; }
    auto t0 = std::chrono::steady_clock::now();
    const int rc = a2c_variants_run(c, S, g, win, which, key_bits, n_kept);
    prof_flush(c);
    S.t_var = ms_since(t0);
    if (rc) {
        S.var_entries.clear();
        S.var_region.clear();
        S.var_text.clear();
        if (n_kept) for (int k = 0; k < n_regions; ++k) n_kept[k] = 0;
    }
    return rc;
}

extern "C" int mh_a2c_variant_entries(mh_ctx *ctx, int slot, int32_t *region, int64_t *count,
                                      int32_t *len, char *seqs, size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    for (size_t k = 0; k < S.var_entries.size(); ++k) {
        if (region) region[k] = S.var_region[k];
        if (count) count[k] = (int64_t)S.var_entries[k].count;
        if (len) len[k] = S.var_entries[k].len;
    }
    if (used) *used = S.var_text.size();
    if (seqs) {
        if (cap < S.var_text.size()) { set_error("mh_a2c_variant_entries: buffer too small"); return -2; }
        memcpy(seqs, S.var_text.data(), S.var_text.size());
    }
    return 0;
}

extern "C" int mh_a2c_variant_stats(mh_ctx *ctx, int slot, int64_t *stats4, double *ms)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !stats4) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    for (int k = 0; k < 4; ++k) stats4[k] = S.var_stats[k];
    if (ms) *ms = S.t_var;
    return 0;
}

// ---------------------------------------------------------------------------
// Linked amino acids: per (set of codons, row) the haplotype the row reads at
// the set's codons, equal haplotypes of a set added up (the rule:
// tests/linkage_oracle.py).  A codon's character is k_a2c_detail's class of
// it: one of the 21 letters, X, '?' (partial), '-' (del); a row with a blank
// codon in a set does not count for the set.
//   k_a2c_link          a wavefront per row, lane = one (set, position) slot
//                       of the pass: the row is read once for all sets.  The
//                       key of a pair is the haplotype itself, 5 bits per
//                       position (codes 1..24, so no key is 0) and the set's
//                       index within the pass in bits 60..63; the lanes of a
//                       set OR their shifted codes together with a segmented
//                       shuffle.  A set whose first or last codon lies
//                       outside the row's codon extent is rejected before a
//                       byte is read.  Per-set coverage leaves as one 64-bit
//                       atomic per set and block.
//   k_a2c_tab_count     (shared) the keys grouped; the keys are exact, so no
//                       verify kernel follows.
//   k_a2c_link_compact  the occupied slots with count >= min_count as (key,
//                       count) records; the distinct ones are counted too.
// More sets than a pass holds (A2C_LINK_SETS sets, A2C_LINK_SLOTS lanes) go
// in further passes.
// ---------------------------------------------------------------------------
namespace mh {

constexpr int A2C_LINK_MAX = 12;         // codons per set: 12 x 5 bits
constexpr int A2C_LINK_SETS = 16;        // sets per pass: 4 bits of the key
constexpr int A2C_LINK_SLOTS = 64;       // (set, position) slots per pass: the lanes of a wave
constexpr int A2C_LINK_BITS = 5;
constexpr int32_t A2C_LINK_FAR = 1 << 29;   // a codon beyond every row (offset, length <= 2^28)
// haplotype characters of the codes 1..24: the 21 letters, X, partial, del
static const char A2C_LINK_CHARS[] = "\0ACDEFGHIKLMNPQRSTVWY*X?-";
enum { A2C_LINK_X = 22, A2C_LINK_PARTIAL = 23, A2C_LINK_DEL = 24 };

struct A2CLinkSlot {
    int32_t codon;
    int8_t set, pos, len, frame;     // set within the pass, position within the set, the set's codons
};

struct A2CLinkRec {
    uint64_t key;
    unsigned long long count;
};

struct A2CLinkArgs : A2CTable {
    const uint8_t *text;
    const int8_t *code;
    const uint8_t *cls;
    const A2CLinkSlot *slots;
    int n_slots;
    unsigned long long *cov;         // per set of the pass
};

__global__ __launch_bounds__(256) void k_a2c_link(A2CLinkArgs A)
{
    __shared__ int8_t s_code[512];
    __shared__ uint8_t s_cls[256];
    __shared__ unsigned long long s_cov[A2C_LINK_SETS];
    s_code[threadIdx.x] = A.code[threadIdx.x];
    s_code[threadIdx.x + 256] = A.code[threadIdx.x + 256];
    s_cls[threadIdx.x] = A.cls[threadIdx.x];
    if (threadIdx.x < A2C_LINK_SETS) s_cov[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool live = lane < A.n_slots;
    A2CLinkSlot L{0, 0, 0, 1, 0};
    if (live) L = A.slots[lane];
    // the set's first and last codon, from the lanes that hold them
    const int k_first = __shfl(L.codon, lane - L.pos), k_last = __shfl(L.codon, lane - L.pos + L.len - 1);
    const int shift = A2C_LINK_BITS * L.pos;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    unsigned long long cov = 0, kept = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < A.n_rows; r += n_waves) {
        const A2CRow R = A.rows[r];
        unsigned long long v = 0;
        int ok = 0;
        // codons offset // 3 .. ceil((frame + offset + len) / 3) - 1 hold bytes of the row
        if (live && k_first >= R.off / 3 && k_last < (L.frame + R.off + R.len + 2) / 3) {
            const int q0 = 3 * L.codon - L.frame - R.off;
            const uint8_t *s = A.text + R.soff;
            int c[3], inside = 0;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int q = q0 + t;
                const bool in = q >= 0 && q < R.len;
                c[t] = in ? s_cls[s[q]] : A2C_DASH;
                inside += in;
            }
            const int a = s_code[64 * c[0] + 8 * c[1] + c[2]];
            const int dashes = (c[0] == A2C_DASH) + (c[1] == A2C_DASH) + (c[2] == A2C_DASH);
            const int bases = (c[0] < A2C_DASH) + (c[1] < A2C_DASH) + (c[2] < A2C_DASH);
            int k = 0;                                   // blank
            if (a < A2C_NAA) k = a + 1;
            else if (dashes == 3 && inside == 3) k = A2C_LINK_DEL;
            else if (bases == 3) k = A2C_LINK_X;
            else if (bases) k = A2C_LINK_PARTIAL;
            v = (unsigned long long)k << shift;
            ok = k != 0;
        }
        // the lanes of a set, towards its first: codes ORed, not-blank flags ANDed
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const unsigned long long ov = __shfl_down(v, d);
            const int ook = __shfl_down(ok, d);
            if (L.pos + d < L.len) {
                v |= ov;
                ok &= ook;
            }
        }
        if (live && L.pos == 0) {
            A.h[(int64_t)L.set * A.n_rows + r] = ok ? (v | ((unsigned long long)L.set << 60)) : 0ull;
            if (ok) {
                cov += R.cnt;
                ++kept;
            }
        }
    }
    if (cov) atomicAdd(&s_cov[L.set], cov);
    kept = a2c_wave_sum(kept);
    if (lane == 0 && kept) atomicAdd(&A.ctr[0], kept);
    __syncthreads();
    if (threadIdx.x < A2C_LINK_SETS && s_cov[threadIdx.x]) atomicAdd(&A.cov[threadIdx.x], s_cov[threadIdx.x]);
}

// The occupied slots: ctr[1] counts them, those with count >= min_count
// leave as records (ctr[2]); one counter atomic each per wave.
__global__ __launch_bounds__(256) void k_a2c_link_compact(A2CTable T, unsigned long long min_count,
                                                          A2CLinkRec *out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool used = s <= T.mask && T.tkey[s] != 0;
    const bool keep = used && T.tcnt[s] >= min_count;
    const unsigned long long bu = __ballot(used), bk = __ballot(keep);
    if (!bu) return;
    unsigned long long base = 0;
    const int leader = __ffsll((long long)bu) - 1;
    if (lane == leader) {
        atomicAdd(&T.ctr[1], (unsigned long long)__popcll(bu));
        if (bk) base = atomicAdd(&T.ctr[2], (unsigned long long)__popcll(bk));
    }
    base = __shfl(base, leader);
    if (keep) out[base + __popcll(bk & ((1ull << lane) - 1))] = A2CLinkRec{T.tkey[s], T.tcnt[s]};
}

struct A2CLinkEntry {
    int32_t set;
    int64_t count;
    char hap[A2C_LINK_MAX];
    int len;
};

// One pass of mh_a2c_link: the sets [s0, s1) of the call over the nr > 0 rows
// of group g; entries and coverage appended to ent / S.link_cov.
static int a2c_link_pass(Ctx &c, A2CState &S, int64_t g, int s0, int s1, const int32_t *set_first,
                         const int32_t *frame, const int32_t *codon, int64_t min_count,
                         std::vector<A2CLinkEntry> &ent)
{
    const int ns = s1 - s0;
    const int64_t nr = S.g_first[g + 1] - S.g_first[g], np = nr * ns;
    hipStream_t s = c.stream;
    A2CDevMem mem;
    A2CLinkArgs a{};
    A2CLinkSlot *d_slots;
    A2CLinkRec *d_rec;
    unsigned long long ctr[3] = {0, 0, 0};
    std::vector<A2CLinkSlot> slots;
    for (int k = s0; k < s1; ++k)
        for (int i = set_first[k]; i < set_first[k + 1]; ++i)
            slots.push_back({std::min(codon[i], A2C_LINK_FAR), (int8_t)(k - s0), (int8_t)(i - set_first[k]),
                             (int8_t)(set_first[k + 1] - set_first[k]), (int8_t)frame[k]});
    hipError_t e = mem.alloc(d_slots, slots.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_slots, slots.data(), sizeof(A2CLinkSlot) * slots.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = mem.alloc(a.h, (size_t)np);
    if (e == hipSuccess) e = mem.alloc(a.ctr, 3);
    if (e == hipSuccess) e = mem.alloc(a.cov, A2C_LINK_SETS);
    if (e == hipSuccess) e = hipMemsetAsync(a.ctr, 0, sizeof(ctr), s);
    if (e == hipSuccess) e = hipMemsetAsync(a.cov, 0, sizeof(unsigned long long) * A2C_LINK_SETS, s);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_link alloc");
    a.text = S.d_text;
    a.rows = S.d_rows + S.g_first[g];
    a.code = S.d_code;
    a.cls = S.d_cls;
    a.slots = d_slots;
    a.n_slots = (int)slots.size();
    a.n_rows = nr;
    a.n_pairs = np;
    {
        const int p0 = prof_begin(c, "k_a2c_link");
        hipLaunchKernelGGL(k_a2c_link, dim3((unsigned)std::min<int64_t>((nr + 3) / 4, 8192)), dim3(256), 0, s, a);
        prof_end(c, p0);
    }
    unsigned long long cov[A2C_LINK_SETS];
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cov, a.cov, sizeof(cov), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "k_a2c_link");
    for (int k = 0; k < ns; ++k) S.link_cov[(size_t)(s0 + k)] = (int64_t)cov[k];
    S.link_stats[0] += (int64_t)ctr[0];
    if (ctr[0] == 0) return 0;
    // ---- the table: twice the keyed pairs, as a2c_group_strings sizes it ----
    uint64_t tsize = 1024;
    while (tsize < 2 * ctr[0]) tsize <<= 1;
    e = mem.alloc(a.tkey, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tcnt, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tfirst, tsize);
    if (e == hipSuccess) e = mem.alloc(a.tclass, tsize);
    if (e == hipSuccess) e = mem.alloc(d_rec, std::min<uint64_t>(ctr[0], tsize));
    if (e == hipSuccess) e = hipMemsetAsync(a.tkey, 0, sizeof(uint64_t) * tsize, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.tcnt, 0, sizeof(unsigned long long) * tsize, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.tfirst, 0xff, sizeof(uint32_t) * tsize, s);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_link table");
    a.mask = tsize - 1;
    {
        const int p0 = prof_begin(c, "k_a2c_link_count");
        hipLaunchKernelGGL(k_a2c_tab_count, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s,
                           static_cast<const A2CTable &>(a));
        prof_end(c, p0);
        const int p1 = prof_begin(c, "k_a2c_link_compact");
        hipLaunchKernelGGL(k_a2c_link_compact, dim3((unsigned)((tsize + 255) / 256)), dim3(256), 0, s,
                           static_cast<const A2CTable &>(a), (unsigned long long)min_count, d_rec);
        prof_end(c, p1);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, a.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "k_a2c_link_count");
    S.link_stats[1] += (int64_t)ctr[1];
    S.link_stats[2] += (int64_t)ctr[2];
    std::vector<A2CLinkRec> rec(ctr[2]);
    e = copy_sync(c, rec.data(), d_rec, sizeof(A2CLinkRec) * rec.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "mh_a2c_link fetch");
    for (const A2CLinkRec &r : rec) {
        A2CLinkEntry x{};
        const int k = (int)(r.key >> 60);
        if (k >= ns) { set_error("mh_a2c_link: the table is inconsistent"); return -3; }
        x.set = s0 + k;
        x.count = (int64_t)r.count;
        x.len = set_first[x.set + 1] - set_first[x.set];
        for (int i = 0; i < x.len; ++i) {
            const int code = (int)((r.key >> (A2C_LINK_BITS * i)) & 31);
            if (code < 1 || code > A2C_LINK_DEL) { set_error("mh_a2c_link: the table is inconsistent"); return -3; }
            x.hap[i] = A2C_LINK_CHARS[code];
        }
        ent.push_back(x);
    }
    return 0;
}

}  // namespace mh

extern "C" int mh_a2c_link(mh_ctx *ctx, int slot, int64_t g, int n_sets, const int32_t *set_first,
                           const int32_t *frame, const int32_t *codon, int64_t min_count,
                           int64_t *n_entries)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || n_sets < 1 || !set_first || !frame || !codon ||
        min_count < 1)
        return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_link(S);
    if (n_entries) *n_entries = 0;
    if (!S.counted) { set_error("mh_a2c_link: nothing is loaded in slot %d", slot); return -3; }
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_link: no group %lld", (long long)g); return -3; }
    if (set_first[0] != 0) { set_error("mh_a2c_link: set_first must start at 0"); return -3; }
    for (int k = 0; k < n_sets; ++k) {
        const int64_t n = (int64_t)set_first[k + 1] - set_first[k];
        if (n < 1 || n > A2C_LINK_MAX) {
            set_error("mh_a2c_link: set %d has %lld codons (1 .. %d)", k, (long long)n, A2C_LINK_MAX);
            return -3;
        }
        if (frame[k] < 0 || frame[k] > 2) { set_error("mh_a2c_link: set %d: frame %d", k, frame[k]); return -3; }
        for (int i = set_first[k]; i < set_first[k + 1]; ++i)
            if (codon[i] < 0) { set_error("mh_a2c_link: set %d: negative codon", k); return -3; }
    }
    auto t0 = std::chrono::steady_clock::now();
    const int64_t nr = S.g_first[g + 1] - S.g_first[g];
    int rc = 0;
    try {
        S.link_cov.assign((size_t)n_sets, 0);
        std::vector<A2CLinkEntry> ent;
        // a pass: at most A2C_LINK_SETS sets, A2C_LINK_SLOTS codons, 2^32 - 1 (set, row) pairs
        const int most = (int)std::max<int64_t>(1, std::min<int64_t>(A2C_LINK_SETS, nr ? 0xffffffffll / nr : A2C_LINK_SETS));
        for (int s0 = 0; nr && s0 < n_sets && !rc;) {
            int s1 = s0;
            while (s1 < n_sets && s1 - s0 < most && set_first[s1 + 1] - set_first[s0] <= A2C_LINK_SLOTS) ++s1;
            rc = a2c_link_pass(c, S, g, s0, s1, set_first, frame, codon, min_count, ent);
            s0 = s1;
        }
        if (!rc) {
            // report order: sets as given, count descending, haplotype bytes ascending
            std::sort(ent.begin(), ent.end(), [](const A2CLinkEntry &x, const A2CLinkEntry &y) {
                if (x.set != y.set) return x.set < y.set;
                if (x.count != y.count) return x.count > y.count;
                return memcmp(x.hap, y.hap, A2C_LINK_MAX) < 0;
            });
            for (const A2CLinkEntry &x : ent) {
                S.link_set.push_back(x.set);
                S.link_count.push_back(x.count);
                S.link_text.append(x.hap, (size_t)x.len);
                S.link_text.push_back('\n');
            }
        }
    } catch (const std::exception &ex) {
        set_error("mh_a2c_link: out of memory (%s)", ex.what());
        rc = -2;
    }
    prof_flush(c);
    S.t_link = ms_since(t0);
    if (rc) {
        const double t = S.t_link;
        a2c_clear_link(S);
        S.t_link = t;
    } else if (n_entries) {
        *n_entries = (int64_t)S.link_set.size();
    }
    return rc;
}

extern "C" int mh_a2c_link_entries(mh_ctx *ctx, int slot, int32_t *set, int64_t *count,
                                   char *haplotypes, size_t cap, size_t *used)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    for (size_t k = 0; k < S.link_set.size(); ++k) {
        if (set) set[k] = S.link_set[k];
        if (count) count[k] = S.link_count[k];
    }
    if (used) *used = S.link_text.size();
    if (haplotypes) {
        if (cap < S.link_text.size()) { set_error("mh_a2c_link_entries: buffer too small"); return -2; }
        memcpy(haplotypes, S.link_text.data(), S.link_text.size());
    }
    return 0;
}

extern "C" int mh_a2c_link_stats(mh_ctx *ctx, int slot, int64_t *coverage, int64_t *stats3, double *ms)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !stats3) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    if (coverage) for (size_t k = 0; k < S.link_cov.size(); ++k) coverage[k] = S.link_cov[k];
    for (int k = 0; k < 3; ++k) stats3[k] = S.link_stats[k];
    if (ms) *ms = S.t_link;
    return 0;
}

// ---------------------------------------------------------------------------
// Pairwise covariation: the weighted Gram matrix of bit columns (the rule:
// tests/covariation_oracle.py).  A column is (frame, codon, mask); it holds a
// row when the row's linkage code there (1..24 of A2C_LINK_CHARS, 0 blank) has
// its bit set in the mask.  gram[i][j] = the summed cnt of the rows both hold.
//   k_a2c_gram_bits   lane = row, a wavefront per 64 consecutive rows of the
//                     group (a row word).  The columns come sorted by (frame,
//                     codon): every distinct site is classified once, as
//                     k_a2c_link classifies (extent rejection before any byte
//                     is read), and each of its columns is one mask test and
//                     one __ballot.  Lane c % 64 keeps the ballot of column c,
//                     so 64 columns of a word leave in one coalesced store:
//                     bits[word][column], the layout k_a2c_gram_pairs stages.
//                     The same ballots make the count planes,
//                     planes[word][k] = bit k of cnt over the word's rows, and
//                     the set of planes that occur at all.
//   k_a2c_gram_pairs  a block owns a 64 x 64 tile of column pairs, on or above
//                     the diagonal, and every gridDim.y-th slice of
//                     A2C_GRAM_SLICE row words; the tile's 128 column slices
//                     and the planes are staged in LDS, a thread holds a 4 x 4
//                     block of pairs.  Per plane that occurs the thread sums
//                     popcount(a & b & plane) over the slice in 32 bits, then
//                     shifts the sum into its 64-bit accumulators; one 64-bit
//                     atomicAdd per non-zero cell ends the block.  The host
//                     mirrors the upper triangle.
// ---------------------------------------------------------------------------
namespace mh {

constexpr int A2C_GRAM_MAX = 512;        // columns of a call
constexpr int A2C_GRAM_SLICE = 32;       // row words of a slice: 2048 rows
constexpr uint32_t A2C_GRAM_CODES = (1u << (A2C_LINK_DEL + 1)) - 2;   // bits 1..24

struct A2CGramSite {
    int32_t codon, frame, first, end;    // columns [first, end) of the sorted order read this site
};

struct A2CGramArgs {
    const uint8_t *text;
    const A2CRow *rows;
    const int8_t *code;
    const uint8_t *cls;
    const A2CGramSite *sites;
    const uint32_t *mask;                // per sorted column
    int n_sites, n_cols, np;             // np: the columns padded to a multiple of 64
    int64_t n_rows, n_words;
    unsigned long long *bits;            // [n_words][np]
    unsigned long long *planes;          // [n_words][32]
    uint32_t *plane_set;                 // bit k: some row of the group has bit k of cnt
    unsigned long long *gram;            // [np][np]
};

__global__ __launch_bounds__(256) void k_a2c_gram_bits(A2CGramArgs A)
{
    __shared__ int8_t s_code[512];
    __shared__ uint8_t s_cls[256];
    __shared__ A2CGramSite s_site[A2C_GRAM_MAX];
    __shared__ uint32_t s_mask[A2C_GRAM_MAX];
    s_code[threadIdx.x] = A.code[threadIdx.x];
    s_code[threadIdx.x + 256] = A.code[threadIdx.x + 256];
    s_cls[threadIdx.x] = A.cls[threadIdx.x];
    for (int i = threadIdx.x; i < A.n_sites; i += 256) s_site[i] = A.sites[i];
    for (int i = threadIdx.x; i < A.n_cols; i += 256) s_mask[i] = A.mask[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    uint32_t seen = 0;                   // lane k < 32: plane k occurred in a word of this wave
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < A.n_words; w += n_waves) {
        const int64_t r = w * 64 + lane;
        const bool live = r < A.n_rows;
        A2CRow R{0, 0, 0, 0, 0};
        if (live) R = A.rows[r];
        unsigned long long mine = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const unsigned long long b = __ballot((R.cnt >> k) & 1);
            if (lane == k) mine = b;
        }
        if (lane < 32) {
            A.planes[w * 32 + lane] = mine;
            seen |= mine != 0;
        }
        const uint8_t *s = A.text + R.soff;
        unsigned long long *out = A.bits + w * A.np;
        mine = 0;
        for (int i = 0; i < A.n_sites; ++i) {
            const A2CGramSite L = s_site[i];
            int k = 0;                                       // blank
            // codons offset // 3 .. ceil((frame + offset + len) / 3) - 1 hold bytes of the row
            if (live && L.codon >= R.off / 3 && L.codon < (L.frame + R.off + R.len + 2) / 3) {
                const int q0 = 3 * L.codon - L.frame - R.off;
                int c[3], inside = 0;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int q = q0 + t;
                    const bool in = q >= 0 && q < R.len;
                    c[t] = in ? s_cls[s[q]] : A2C_DASH;
                    inside += in;
                }
                const int a = s_code[64 * c[0] + 8 * c[1] + c[2]];
                const int dashes = (c[0] == A2C_DASH) + (c[1] == A2C_DASH) + (c[2] == A2C_DASH);
                const int bases = (c[0] < A2C_DASH) + (c[1] < A2C_DASH) + (c[2] < A2C_DASH);
                if (a < A2C_NAA) k = a + 1;
                else if (dashes == 3 && inside == 3) k = A2C_LINK_DEL;
                else if (bases == 3) k = A2C_LINK_X;
                else if (bases) k = A2C_LINK_PARTIAL;
            }
            for (int col = L.first; col < L.end; ++col) {    // wave-uniform
                const unsigned long long b = __ballot((s_mask[col] >> k) & 1);   // no mask has bit 0
                if (lane == (col & 63)) mine = b;
                if ((col & 63) == 63) {
                    out[col - 63 + lane] = mine;
                    mine = 0;
                }
            }
        }
        // the last, partly filled 64 columns: zeros past n_cols
        if (A.n_cols & 63) out[(A.n_cols & ~63) + lane] = mine;
    }
    if (lane < 32 && seen) atomicOr(A.plane_set, 1u << lane);
}

__global__ __launch_bounds__(256) void k_a2c_gram_pairs(A2CGramArgs A)
{
    __shared__ unsigned long long s_a[A2C_GRAM_SLICE][64], s_b[A2C_GRAM_SLICE][64], s_p[A2C_GRAM_SLICE][32];
    // tile blockIdx.x of the upper triangle, rows of tiles first
    const int side = A.np / 64;
    int ti = 0, t = (int)blockIdx.x;
    while (t >= side - ti) {
        t -= side - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint32_t plane_set = *A.plane_set;
    const int64_t n_slices = (A.n_words + A2C_GRAM_SLICE - 1) / A2C_GRAM_SLICE;
    unsigned long long acc[4][4] = {};
    for (int64_t sl = blockIdx.y; sl < n_slices; sl += gridDim.y) {
        const int64_t w0 = sl * A2C_GRAM_SLICE;
        __syncthreads();
        for (int i = threadIdx.x; i < A2C_GRAM_SLICE * 64; i += 256) {
            const int64_t w = w0 + (i >> 6);
            const bool in = w < A.n_words;
            s_a[i >> 6][i & 63] = in ? A.bits[w * A.np + 64 * ti + (i & 63)] : 0ull;
            s_b[i >> 6][i & 63] = in ? A.bits[w * A.np + 64 * tj + (i & 63)] : 0ull;
        }
        for (int i = threadIdx.x; i < A2C_GRAM_SLICE * 32; i += 256) {
            const int64_t w = w0 + (i >> 5);
            s_p[i >> 5][i & 31] = w < A.n_words ? A.planes[w * 32 + (i & 31)] : 0ull;
        }
        __syncthreads();
        for (uint32_t m = plane_set; m; m &= m - 1) {
            const int k = __ffs((int)m) - 1;
            // a slice is 64 * A2C_GRAM_SLICE = 2048 rows, so a plane's sum over it is at
            // most 2048: 32 bits hold it.  Shifted by k <= 31 it is below 2^43, and a
            // cell's total is at most the group's summed cnt, below 2^32 * 2^31 rows.
            uint32_t part[4][4] = {};
            for (int w = 0; w < A2C_GRAM_SLICE; ++w) {
                const unsigned long long p = s_p[w][k];
                unsigned long long b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = s_b[w][tx + 16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned long long a = s_a[w][ty + 16 * i] & p;
#pragma unroll
                    for (int j = 0; j < 4; ++j) part[i][j] += (uint32_t)__popcll(a & b[j]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (unsigned long long)part[i][j] << k;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (acc[i][j])
                atomicAdd(&A.gram[(size_t)(64 * ti + ty + 16 * i) * A.np + 64 * tj + tx + 16 * j], acc[i][j]);
}

}  // namespace mh

extern "C" int mh_a2c_gram(mh_ctx *ctx, int slot, int64_t g, int n_cols, const int32_t *frame,
                           const int32_t *codon, const uint32_t *mask, int64_t *gram)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    A2CState &S = *a2c_state(c, slot);
    a2c_clear_gram(S);
    if (n_cols < 1 || n_cols > A2C_GRAM_MAX) {
        set_error("mh_a2c_gram: %d columns (1 .. %d)", n_cols, A2C_GRAM_MAX);
        return -3;
    }
    if (!frame || !codon || !mask || !gram) return -3;
    if (!S.counted) { set_error("mh_a2c_gram: nothing is loaded in slot %d", slot); return -3; }
    const int64_t ng = (int64_t)S.g_first.size() - 1;
    if (g < 0 || g >= ng) { set_error("mh_a2c_gram: no group %lld", (long long)g); return -3; }
    for (int k = 0; k < n_cols; ++k) {
        if (frame[k] < 0 || frame[k] > 2) { set_error("mh_a2c_gram: column %d: frame %d", k, frame[k]); return -3; }
        if (codon[k] < 0) { set_error("mh_a2c_gram: column %d: negative codon", k); return -3; }
        if (!mask[k] || (mask[k] & ~A2C_GRAM_CODES)) {
            set_error("mh_a2c_gram: column %d: mask 0x%x (bits 1 .. %d, not 0)", k, mask[k], (int)A2C_LINK_DEL);
            return -3;
        }
    }
    auto t0 = std::chrono::steady_clock::now();
    const int64_t nr = S.g_first[g + 1] - S.g_first[g], nw = (nr + 63) / 64;
    const int np = (n_cols + 63) / 64 * 64, side = np / 64, tiles = side * (side + 1) / 2;
    memset(gram, 0, sizeof(int64_t) * (size_t)n_cols * n_cols);
    int rc = 0;
    try {
        // the columns by (frame, codon): equal sites share one classification
        std::vector<int> order(n_cols);
        for (int k = 0; k < n_cols; ++k) order[k] = k;
        std::sort(order.begin(), order.end(), [&](int x, int y) {
            if (frame[x] != frame[y]) return frame[x] < frame[y];
            if (codon[x] != codon[y]) return codon[x] < codon[y];
            return x < y;
        });
        std::vector<A2CGramSite> sites;
        std::vector<uint32_t> masks(n_cols);
        for (int k = 0; k < n_cols; ++k) {
            const int x = order[k];
            masks[k] = mask[x];
            if (k && frame[x] == frame[order[k - 1]] && codon[x] == codon[order[k - 1]]) sites.back().end = k + 1;
            else sites.push_back({std::min(codon[x], A2C_LINK_FAR), frame[x], k, k + 1});
        }
        S.gram_stats[0] = nr;
        S.gram_stats[1] = nw;
        S.gram_stats[3] = (int64_t)sites.size();
        S.gram_stats[4] = tiles;
        if (nr) {
            hipStream_t s = c.stream;
            A2CDevMem mem;
            A2CGramArgs a{};
            A2CGramSite *d_sites;
            uint32_t *d_mask;
            hipError_t e = mem.alloc(d_sites, sites.size());
            if (e == hipSuccess) e = mem.alloc(d_mask, masks.size());
            if (e == hipSuccess) e = mem.alloc(a.bits, (size_t)nw * np);
            if (e == hipSuccess) e = mem.alloc(a.planes, (size_t)nw * 32);
            if (e == hipSuccess) e = mem.alloc(a.plane_set, 1);
            if (e == hipSuccess) e = mem.alloc(a.gram, (size_t)np * np);
            if (e == hipSuccess) e = hipMemcpyAsync(d_sites, sites.data(), sizeof(A2CGramSite) * sites.size(), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_mask, masks.data(), sizeof(uint32_t) * masks.size(), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemsetAsync(a.plane_set, 0, sizeof(uint32_t), s);
            if (e == hipSuccess) e = hipMemsetAsync(a.gram, 0, sizeof(unsigned long long) * np * np, s);
            if (e != hipSuccess) {
                a2c_clear_gram(S);
                return hip_fail(e, "mh_a2c_gram alloc");
            }
            a.text = S.d_text;
            a.rows = S.d_rows + S.g_first[g];
            a.code = S.d_code;
            a.cls = S.d_cls;
            a.sites = d_sites;
            a.mask = d_mask;
            a.n_sites = (int)sites.size();
            a.n_cols = n_cols;
            a.np = np;
            a.n_rows = nr;
            a.n_words = nw;
            const int64_t n_slices = (nw + A2C_GRAM_SLICE - 1) / A2C_GRAM_SLICE;
            {
                const int p0 = prof_begin(c, "k_a2c_gram_bits");
                hipLaunchKernelGGL(k_a2c_gram_bits, dim3((unsigned)std::min<int64_t>((nw + 3) / 4, 8192)), dim3(256), 0, s, a);
                prof_end(c, p0);
                // about 2048 blocks: each tile's slices shared out over gridDim.y of them
                const unsigned ny = (unsigned)std::min<int64_t>(n_slices, std::max(1, 2048 / tiles));
                const int p1 = prof_begin(c, "k_a2c_gram_pairs");
                hipLaunchKernelGGL(k_a2c_gram_pairs, dim3((unsigned)tiles, ny), dim3(256), 0, s, a);
                prof_end(c, p1);
            }
            std::vector<unsigned long long> full((size_t)np * np);
            uint32_t plane_set = 0;
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(full.data(), a.gram, sizeof(unsigned long long) * full.size(), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(&plane_set, a.plane_set, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = hip_fail(e, "k_a2c_gram");
            S.gram_stats[2] = __builtin_popcount(plane_set);
            // the upper triangle of the sorted order, mirrored, in the caller's order
            for (int x = 0; x < n_cols && !rc; ++x)
                for (int y = x; y < n_cols; ++y) {
                    const int64_t v = (int64_t)full[(size_t)x * np + y];
                    gram[(size_t)order[x] * n_cols + order[y]] = v;
                    gram[(size_t)order[y] * n_cols + order[x]] = v;
                }
        }
    } catch (const std::exception &ex) {
        set_error("mh_a2c_gram: out of memory (%s)", ex.what());
        rc = -2;
    }
    prof_flush(c);
    const double t = ms_since(t0);
    if (rc) {
        a2c_clear_gram(S);
        memset(gram, 0, sizeof(int64_t) * (size_t)n_cols * n_cols);
    }
    S.t_gram = t;
    return rc;
}

extern "C" int mh_a2c_gram_stats(mh_ctx *ctx, int slot, int64_t *stats, double *ms)
{
    if (!ctx || slot < 0 || slot >= A2C_SLOTS || !stats) return -3;
    Ctx &c = *ctx_of(ctx);
    A2CState &S = *a2c_state(c, slot);
    for (int k = 0; k < 5; ++k) stats[k] = S.gram_stats[k];
    if (ms) *ms = S.t_gram;
    return 0;
}
