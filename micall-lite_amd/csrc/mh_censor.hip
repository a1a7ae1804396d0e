// mh_censor.hip -- censor_fastq.censor (micall/core/censor_fastq.py:32-102)
// on gfx950, behind mh_censor_fastq / mh_censor_staged / mh_censor_output /
// mh_censor_write:
//   host      the FASTQ text: gunzipped from a buffer (libdeflate, else
//             zlib) or taken from a staged FASTQ (mh_fastq_open_part: the
//             file mmap'd, its gzip members inflated in parallel), into a
//             buffer that is not zero-filled; line starts found in parallel
//             (memchr, two passes: counts, then positions); records parsed
//             in parallel, tile + read direction from each header exactly as
//             :59-63 parse them, bad (tile, cycle) set from the caller
//   k_censor  one wave64 per read: the bases / qualities of bad cycles
//             become 'N' / '#' in place, the trailing run of bad cycles is
//             dropped (the reference only flushes pending Ns before a good
//             cycle, :66-74, :78-90), and every quality score is summed for
//             the summary (:80-82) -- per-block sums, one atomic per block
//   k_trim    only with adapters set (mh_censor_set_adapters; no such step
//             in the reference, bin/micall:133 names it): one wave64 per
//             read, the censored sequence line against each 3' adapter of
//             its read direction by a semi-global unit-cost edit distance
//             (lane l = adapter row l + 1, skewed along the read); the
//             kept lengths are lowered to the leftmost match's start
//   k_primer  only with primers set (mh_censor_set_primers): one wave64 per
//             read, lane l takes the primers l, l + 64, ... of its read
//             direction, each anchored at the read's first base by Myers'
//             bit-vector edit distance (the primer's rows in one 64-bit
//             word, one column per read base); the winner's end is the
//             record's lead, the bases the writer drops at the front
//   k_primer3 only with 3' primers set (mh_censor_set_primers3): one wave64
//             per read, the same lanes and words, the read scanned from its
//             last kept base backwards to its lead against the reversed
//             primers, so that a column's index is the number of bases cut;
//             a search state (the whole primer, starting at the cut) and a
//             partial state (the read ends inside the primer) per lane; the
//             winner lowers the record's kept lengths
//   host      records rewritten (header and '+' lines verbatim) and, for
//             gzip output, compressed, in blocks of ~8 MB of records on
//             every host thread, sequence and quality lines from their lead
//             to their kept length (one gzip member per block: the member
//             boundaries depend on the input only, not on the thread count);
//             the output is written with pwrite (mh_censor_write) or copied
//             out (mh_censor_output)
#include <sys/types.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "mh_fastq.h"
#include "mh_gunzip.h"
#include "mh_internal.h"

namespace mh {

constexpr int TRIM_MAXADAPT = 8;     // adapters per read direction
constexpr int TRIM_MAXLEN = 64;      // adapter bases: one lane per adapter row
constexpr int TRIM_MAXREAD = 65535;  // read bases: a match's start is 16 bits of a DP cell

// the adapters as k_trim reads them: slot = direction * TRIM_MAXADAPT + index,
// direction 0 for the records of read 1 (sign +1), 1 for all others
struct TrimTab {
    int32_t n[2];
    int32_t min_overlap;
    int32_t len[2 * TRIM_MAXADAPT];
    int32_t max_err[TRIM_MAXLEN + 1];   // errors allowed in a match of i adapter bases
    uint8_t seq[2 * TRIM_MAXADAPT][TRIM_MAXLEN];
};

constexpr int PRIMER_MAX = 256;     // primers per read direction
constexpr int PRIMER_MINLEN = 8;    // primer bases: the rows of one 64-bit word
constexpr int PRIMER_MAXLEN = 64;
constexpr int PRIMER_MAXCOL = 127;  // read columns looked at: 7 bits of the key, two loads a lane

// the primers as k_primer reads them, slot = direction * PRIMER_MAX + index:
// eq[d][c][k] has bit i set where primer k of direction d holds base "ACGT"[c]
// at i; cols[d] is the largest len + err of the direction's list
struct PrimerTab {
    int32_t n[2];
    int32_t cols[2];
    int32_t len[2 * PRIMER_MAX];
    int32_t err[2 * PRIMER_MAX];   // errors allowed in the whole primer
    uint64_t eq[2][4][PRIMER_MAX];
};

// the 3' primers as k_primer3 reads them: p.eq holds the masks of the
// REVERSED primers (bit i set where the primer holds the base at m - 1 - i),
// p.err the errors allowed in the whole primer, p.cols is not used;
// max_err[b] is the budget of a partial match that removes b bases
struct Primer3Tab {
    PrimerTab p;
    int32_t min_overlap;
    int32_t max_err[PRIMER_MAXLEN + 1];
};

struct CensorState {
    TextBuf text;                           // the FASTQ (censored in place)
    // per record: line starts (header, seq, '+', qual); the header line is
    // [h0, s0), the '+' line [o0, q0), both with their newline
    std::vector<int64_t> h0, s0, o0, q0;
    std::vector<int32_t> sl, ql;            // seq / qual lengths, trailing whitespace stripped
    std::vector<int32_t> tile, sign;        // tile id (-1: no bad cycle) / +1, -1
    std::vector<int32_t> keep;              // 2 per record: kept seq / qual length
    std::vector<int32_t> lead;              // per record, only with primers set: bases dropped in front
    int64_t base_count = 0, score_sum = 0;
    TextBuf out;                            // the censored file (gzip members or text)
    // set: the blocks are written to sink_fd from sink_pos as they are made
    // (mh_censor_staged_write) instead of collected in out
    int sink_fd = -1;
    int64_t sink_pos = 0;
    int sink_err = 0;
    double t_host_in = 0, t_device = 0, t_host_out = 0;
    // device buffers, grown on demand and kept between calls
    uint8_t *d_text = nullptr;
    int64_t *d_s0 = nullptr, *d_q0 = nullptr;
    int32_t *d_sl = nullptr, *d_ql = nullptr, *d_tile = nullptr, *d_sign = nullptr, *d_keep = nullptr;
    uint32_t *d_bad = nullptr;
    unsigned long long *d_sums = nullptr;
    int64_t cap_text = 0, cap_rec = 0, cap_bad = 0;
    // 3' adapters of the following calls (mh_censor_set_adapters) and what
    // the last call trimmed, per direction * TRIM_MAXADAPT + adapter
    bool trim_on = false;
    TrimTab trim{};
    int64_t trim_reads[2 * TRIM_MAXADAPT] = {}, trim_bases[2 * TRIM_MAXADAPT] = {};
    TrimTab *d_trim = nullptr;
    unsigned long long *d_tstat = nullptr;   // reads[16], bases[16]
    // 5' primers of the following calls (mh_censor_set_primers) and what the
    // last call trimmed, per direction * PRIMER_MAX + primer
    bool primer_on = false;
    PrimerTab primer{};
    int64_t primer_reads[2 * PRIMER_MAX] = {}, primer_bases[2 * PRIMER_MAX] = {};
    PrimerTab *d_primer = nullptr;
    int32_t *d_lead = nullptr;
    unsigned long long *d_pstat = nullptr;   // reads[512], bases[512]
    // 3' primers of the following calls (mh_censor_set_primers3) and what the
    // last call trimmed, per direction * PRIMER_MAX + primer
    bool primer3_on = false;
    std::unique_ptr<Primer3Tab> primer3;
    int64_t primer3_reads[2 * PRIMER_MAX] = {}, primer3_bases[2 * PRIMER_MAX] = {};
    Primer3Tab *d_primer3 = nullptr;
    unsigned long long *d_p3stat = nullptr;  // reads[512], bases[512]
};

static void censor_free_device(CensorState &C)
{
    hipFree(C.d_text); hipFree(C.d_s0); hipFree(C.d_q0); hipFree(C.d_sl); hipFree(C.d_ql);
    hipFree(C.d_tile); hipFree(C.d_sign); hipFree(C.d_keep); hipFree(C.d_bad); hipFree(C.d_sums);
    hipFree(C.d_trim); hipFree(C.d_tstat);
    C.d_trim = nullptr; C.d_tstat = nullptr;
    hipFree(C.d_primer); hipFree(C.d_lead); hipFree(C.d_pstat);
    C.d_primer = nullptr; C.d_lead = nullptr; C.d_pstat = nullptr;
    hipFree(C.d_primer3); hipFree(C.d_p3stat);
    C.d_primer3 = nullptr; C.d_p3stat = nullptr;
    C.d_text = nullptr; C.d_s0 = C.d_q0 = nullptr;
    C.d_sl = C.d_ql = C.d_tile = C.d_sign = C.d_keep = nullptr;
    C.d_bad = nullptr; C.d_sums = nullptr;
    C.cap_text = C.cap_rec = C.cap_bad = 0;
}

void censor_free(Ctx &c)
{
    if (c.censor) censor_free_device(*c.censor);
    delete c.censor;
    c.censor = nullptr;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
struct CensorArgs {
    uint8_t *text;
    const int64_t *s0, *q0;
    const int32_t *sl, *ql, *tile, *sign;
    int64_t n;
    const uint32_t *bad;     // per bad tile: bitmap over cycles -maxc .. maxc
    int maxc, words;         // words per tile bitmap
    int32_t *keep;
    unsigned long long *sums;   // [0] score sum (two's complement), [1] bases
};

__device__ __forceinline__ bool censor_bad(const CensorArgs &A, int t, int cyc)
{
    if (t < 0 || cyc < -A.maxc || cyc > A.maxc) return false;
    const int b = cyc + A.maxc;
    return (A.bad[(int64_t)t * A.words + (b >> 5)] >> (b & 31)) & 1u;
}

__global__ __launch_bounds__(256) void k_censor(CensorArgs A)
{
    __shared__ long long part_sum[4];
    __shared__ long long part_n[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long ssum = 0, nb = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < A.n; r += (int64_t)gridDim.x * 4) {
        const int t = A.tile[r], sg = A.sign[r];
        // bases
        int last = 0;
        uint8_t *s = A.text + A.s0[r];
        for (int i = lane; i < A.sl[r]; i += 64) {
            if (censor_bad(A, t, sg * (i + 1))) s[i] = 'N';
            else last = i + 1;
        }
        for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
        const int keep_s = last;
        // qualities (summed before censoring)
        last = 0;
        uint8_t *q = A.text + A.q0[r];
        for (int i = lane; i < A.ql[r]; i += 64) {
            ssum += (long long)q[i] - 33;
            if (censor_bad(A, t, sg * (i + 1))) q[i] = '#';
            else last = i + 1;
        }
        nb += A.ql[r] > lane ? (A.ql[r] - lane + 63) / 64 : 0;
        for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
        if (lane == 0) {
            A.keep[2 * r] = keep_s;
            A.keep[2 * r + 1] = last;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ssum += __shfl_xor(ssum, o, 64);
        nb += __shfl_xor(nb, o, 64);
    }
    if (lane == 0) { part_sum[wv] = ssum; part_n[wv] = nb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = 0, b = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { a += part_sum[w]; b += part_n[w]; }
        if (a) atomicAdd(&A.sums[0], (unsigned long long)a);
        if (b) atomicAdd(&A.sums[1], (unsigned long long)b);
    }
}

// ---- k_trim: 3' adapters ---------------------------
// For an adapter a (m bases) and the read r (n bases: the sequence line as
// k_censor left it, cut to its kept length), cell (i, j) holds
// K = cost << 16 | origin: the smallest unit-cost edit distance between
// a[:i] and any r[s:j], and the smallest s that attains it,
//   K[i][j] = min(K[i-1][j-1] + (a[i-1] != r[j-1]) << 16,
//                 K[i-1][j] + 1 << 16, K[i][j-1] + 1 << 16),
//   K[0][j] = j, K[i][0] = i << 16.
// Candidates are (m, j) for every j with cost <= max_err[m], and (i, n) for
// min_overlap <= i < m with cost <= max_err[i]; over the adapters of the
// record's direction the smallest origin wins, then the smaller cost, the
// larger i, the lower adapter index, which is the order of the 31-bit key
//   origin << 15 | cost << 9 | (64 - i) << 3 | adapter
// (a candidate's cost is below 64: max_err[i] < i <= 64).
//
// One wave per read.  Lane l owns row l + 1 and at step t stands in column
// t - l + 1, so "up" is the lane below's cell of the step before (one lane
// shift) and "diagonal" the value shifted in the step before that; lane 0
// takes row 0's K[0][t + 1] = t + 1.  The read's bytes walk up the lanes by
// the same shift: 64 of them are loaded at a time, one block ahead, and lane
// 0 takes byte t of the block in hand each step.
struct TrimArgs {
    const uint8_t *text;
    const int64_t *s0;
    const int32_t *sign;
    int64_t n;
    int32_t *keep;
    const TrimTab *tab;
    unsigned long long *stat;   // [slot] reads, [16 + slot] bases
};

// lane l <- lane l - 1 (lane 0 takes `first`)
__device__ __forceinline__ uint32_t trim_shift_up(uint32_t first, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138, 0xF, 0xF, false);
}

__global__ __launch_bounds__(256) void k_trim(TrimArgs A)
{
    constexpr int NS = 2 * TRIM_MAXADAPT;
    __shared__ unsigned long long part[4][2 * NS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TrimTab &T = *A.tab;
    const int min_ov = __builtin_amdgcn_readfirstlane(T.min_overlap);
    unsigned long long my_reads = 0, my_bases = 0;   // lane k < NS: of slot k
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < A.n; r += (int64_t)gridDim.x * 4) {
        const int dir = __builtin_amdgcn_readfirstlane(A.sign[r] == 1 ? 0 : 1);
        const int n = __builtin_amdgcn_readfirstlane(A.keep[2 * r]);
        const int na = __builtin_amdgcn_readfirstlane(T.n[dir]);
        // a longer read is left alone: the host fails the call for it
        if (n <= 0 || n > TRIM_MAXREAD || na <= 0) continue;
        const uint8_t *rd = A.text + A.s0[r];
        auto block = [&](int p) { return p + lane < n ? (uint32_t)rd[p + lane] : 0u; };
        uint32_t best = ~0u;
        for (int k = 0; k < na; ++k) {
            const int slot = dir * TRIM_MAXADAPT + k;
            const int m = __builtin_amdgcn_readfirstlane(T.len[slot]);
            const bool row = lane < m;
            const uint32_t ab = T.seq[slot][lane];
            // a cell is within the row's error budget when it is <= vmax
            const uint32_t vmax = (uint32_t)T.max_err[lane + 1] << 16 | 0xffffu;
            const uint32_t ktail = (uint32_t)(63 - lane) << 3 | (uint32_t)k;
            // of a cell with its halves swapped (origin above cost)
            auto key = [&](uint32_t w) { return (w >> 16) << 15 | (w & 0xffffu) << 9 | ktail; };
            const bool last = lane == m - 1;
            uint32_t cur = (uint32_t)(lane + 1) << 16, diag = (uint32_t)lane << 16;
            uint32_t rb = 0, full = ~0u;   // full: the least swapped cell of row m within budget
            uint32_t nxt = block(0);
            const int steps = n + m - 1;
            for (int t0 = 0; t0 < steps; t0 += 64) {
                const uint32_t blk = nxt;
                nxt = block(t0 + 64);
                auto step = [&](int q) {
                    const int t = t0 + q;
                    rb = trim_shift_up((uint32_t)__builtin_amdgcn_readlane((int)blk, q), rb);
                    const uint32_t up = trim_shift_up((uint32_t)(t + 1), cur);
                    const uint32_t v = min(diag + (ab != rb ? 0x10000u : 0u), min(up, cur) + 0x10000u);
                    diag = up;
                    // column j = t - lane + 1 is in 1 .. n (selects, no branch)
                    const bool act = row && (uint32_t)(t - lane) < (uint32_t)n;
                    cur = act ? v : cur;
                    const uint32_t swapped = v >> 16 | v << 16;
                    full = min(full, act && last && v <= vmax ? swapped : ~0u);
                };
                // four steps a turn (the shifts keep the compiler from
                // unrolling): a step past the last one finds no row active
                const int qn = min(64, (steps - t0 + 3) & ~3);
                for (int q = 0; q < qn; q += 4) {
                    step(q);
                    step(q + 1);
                    step(q + 2);
                    step(q + 3);
                }
            }
            // lane m - 1 holds the best full match, a lane below it its
            // prefix's cell at the read's end
            if (last) best = min(best, full == ~0u ? ~0u : key(full));
            else if (row && lane + 1 >= min_ov && cur <= vmax) best = min(best, key(cur >> 16 | cur << 16));
        }
        for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, 64));
        if (best == ~0u) continue;
        const int s = (int)(best >> 15);
        const int slot = dir * TRIM_MAXADAPT + (int)(best & 7u);
        if (lane == 0) {
            A.keep[2 * r] = s;
            A.keep[2 * r + 1] = min(A.keep[2 * r + 1], s);
        }
        if (lane == slot) { ++my_reads; my_bases += (unsigned long long)(n - s); }
    }
    if (lane < NS) { part[wv][lane] = my_reads; part[wv][NS + lane] = my_bases; }
    __syncthreads();
    if (threadIdx.x < 2 * NS) {
        unsigned long long a = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) a += part[w][threadIdx.x];
        if (a) atomicAdd(&A.stat[threadIdx.x], a);
    }
}

// ---- k_primer: anchored 5' primers ------------------
// For a primer p (m bases) and the read r (n bases: the sequence line as
// k_censor and k_trim left it), D(j) is the unit-cost edit distance between
// all of p and r[0:j]; (k, j) is a candidate when D(j) <= err[k].  Over the
// primers of the record's direction the larger m - D wins, then the smaller
// D, the larger j, the lower primer index, which is the order of the key
//   (64 - (m - D)) << 21 | D << 15 | (127 - j) << 8 | k
// (1 <= m - D <= 64 and D < 64 as err < m <= 64; j <= m + err <= 127).
//
// One wave per read.  The read's first cols = min(n, largest m + err of the
// list) bytes sit in two VGPRs, byte j of them is broadcast to every lane
// through an SGPR each column.  Lane l takes the primers l, l + 64, ...: the
// column of the DP table over its primer's rows as Myers' vertical delta
// words (pv, mv), with Hyyro's boundary for a distance from the read's start
// (the horizontal delta shifted into row 0 is +1: D[0][j] = j, not 0), and
// the cell of row m followed as a score.  D(j) >= |j - m|, so the columns a
// lane runs past its own m + err hold no candidate.
struct PrimerArgs {
    const uint8_t *text;
    const int64_t *s0;
    const int32_t *sign;
    int64_t n;
    const int32_t *keep;
    int32_t *lead;
    const PrimerTab *tab;
    unsigned long long *stat;   // [slot] reads, [2 * PRIMER_MAX + slot] bases
};

__global__ __launch_bounds__(256) void k_primer(PrimerArgs A)
{
    constexpr int NS = 2 * PRIMER_MAX;
    // what this block's reads lost, per slot: a block takes far fewer than
    // 2^32 / PRIMER_MAXCOL reads
    __shared__ uint32_t part[2 * NS];
    for (int i = threadIdx.x; i < 2 * NS; i += blockDim.x) part[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const PrimerTab &T = *A.tab;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < A.n; r += (int64_t)gridDim.x * 4) {
        const int dir = __builtin_amdgcn_readfirstlane(A.sign[r] == 1 ? 0 : 1);
        const int n = __builtin_amdgcn_readfirstlane(A.keep[2 * r]);
        const int np = __builtin_amdgcn_readfirstlane(T.n[dir]);
        const int cols = min(n, min(__builtin_amdgcn_readfirstlane(T.cols[dir]), PRIMER_MAXCOL));
        const uint8_t *rd = A.text + A.s0[r];
        const uint32_t b0 = lane < cols ? (uint32_t)rd[lane] : 0u;
        const uint32_t b1 = lane + 64 < cols ? (uint32_t)rd[lane + 64] : 0u;
        uint32_t best = ~0u;
        for (int k0 = 0; k0 < np && cols > 0; k0 += 64) {
            const bool act = k0 + lane < np;
            const int k = act ? k0 + lane : 0;
            const int m = T.len[dir * PRIMER_MAX + k];
            const uint64_t eq_a = T.eq[dir][0][k], eq_c = T.eq[dir][1][k];
            const uint64_t eq_g = T.eq[dir][2][k], eq_t = T.eq[dir][3][k];
            const uint64_t top = 1ull << (m - 1);
            uint64_t pv = ~0ull, mv = 0;
            // lim: the least D so far, from the budget down; at: its last column
            int score = m, lim = T.err[dir * PRIMER_MAX + k], at = 0;
            auto column = [&](int j, uint32_t c) {
                const uint64_t eq = c == 'A' ? eq_a : c == 'C' ? eq_c : c == 'G' ? eq_g : c == 'T' ? eq_t : 0ull;
                const uint64_t xv = eq | mv;
                const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
                uint64_t ph = mv | ~(xh | pv);
                uint64_t mh = pv & xh;
                score += (ph & top ? 1 : 0) - (mh & top ? 1 : 0);
                ph = ph << 1 | 1ull;
                mh <<= 1;
                pv = mh | ~(xv | ph);
                mv = ph & xv;
                const bool hit = score <= lim;
                lim = hit ? score : lim;
                at = hit ? j : at;
            };
            const int c0 = min(cols, 64);
            for (int j = 0; j < c0; ++j) column(j + 1, (uint32_t)__builtin_amdgcn_readlane((int)b0, j));
            for (int j = 64; j < cols; ++j) column(j + 1, (uint32_t)__builtin_amdgcn_readlane((int)b1, j - 64));
            if (act && at)
                best = min(best, (uint32_t)(64 - (m - lim)) << 21 | (uint32_t)lim << 15 |
                                     (uint32_t)(PRIMER_MAXCOL - at) << 8 | (uint32_t)k);
        }
        for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o, 64));
        if (lane == 0) {
            const int j = best == ~0u ? 0 : PRIMER_MAXCOL - (int)(best >> 8 & 127u);
            A.lead[r] = j;
            if (j) {
                const int slot = dir * PRIMER_MAX + (int)(best & 255u);
                atomicAdd(&part[slot], 1u);
                atomicAdd(&part[NS + slot], (uint32_t)j);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * NS; i += blockDim.x)
        if (part[i]) atomicAdd(&A.stat[i], (unsigned long long)part[i]);
}

// ---- k_primer3: 3' primers --------------------------
// The text is x = r[lead:n] (n the kept length, lead k_primer's or 0), the
// pattern a primer p of m bases, b the bases cut from the end.  On the
// reversed strings (q = p reversed, t = x reversed), column b of
//   A: A[0][j] = 0, A[i][0] = i   F(b) = A[m][b]: all of p against r[n-b:e],
//                                 the best e -- the primer starts at the cut
//   B: B[0][j] = j, B[i][0] = 0   G(b) = B[m][b]: the best prefix of p against
//                                 all of r[n-b:n] -- the read ends in the primer
// Candidates are (k, b), 1 <= b <= len(x), with F(b) <= E[m] (L = m, D = F) and
// (k, b), min_overlap <= b <= min(len(x), m - 1), with G(b) <= E[b] (L = b,
// D = G); the larger L - D wins, then the smaller D, the larger b, the lower
// primer index, which is the order of the 37-bit key
//   (64 - (L - D)) << 30 | D << 24 | (65535 - b) << 8 | k
// (1 <= L - D <= 64 and D < 64 as E[i] < i <= 64; b <= 65535).
//
// One wave per read, lane l takes the primers l, l + 64, ... as k_primer
// does; every round of 64 primers scans the read again.  The scan runs from
// the read's last kept base backwards: 64 bytes are loaded at a time in
// reversed order, one block ahead, and each column's byte is broadcast from
// the block in hand through an SGPR, so the column loop holds no load.  Both
// states step on the same byte and the same mask of the reversed primer: A
// with Myers' search boundary (pv = ~0, mv = 0, a horizontal delta of 0 into
// row 0), B with pv = mv = 0 and a horizontal delta of +1 into row 0.  B can
// hold a candidate only for b <= m - 1 <= 63, so it runs in the first
// min(len(x), 63) columns alone.  Of a lane's full candidates the least F,
// then the largest b, is the one its key can win with (m is the lane's own);
// its partial candidates differ in L, so their order is kept in a 19-bit key
// of the same fields.
struct Primer3Args {
    const uint8_t *text;
    const int64_t *s0;
    const int32_t *sign;
    int64_t n;
    int32_t *keep;
    const int32_t *lead;        // null without 5' primers
    const Primer3Tab *tab;
    unsigned long long *stat;   // [slot] reads, [2 * PRIMER_MAX + slot] bases
};

__global__ __launch_bounds__(256) void k_primer3(Primer3Args A)
{
    constexpr int NS = 2 * PRIMER_MAX;
    // what this block's reads lost, per slot (a cut is up to 65 535 bases)
    __shared__ unsigned long long part[2 * NS];
    for (int i = threadIdx.x; i < 2 * NS; i += blockDim.x) part[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const Primer3Tab &T = *A.tab;
    const int min_ov = __builtin_amdgcn_readfirstlane(T.min_overlap);
    // lane b: the budget of a partial match that removes b bases (b <= 63)
    const int ev = T.max_err[lane];
    for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < A.n; r += (int64_t)gridDim.x * 4) {
        const int dir = __builtin_amdgcn_readfirstlane(A.sign[r] == 1 ? 0 : 1);
        const int n = __builtin_amdgcn_readfirstlane(A.keep[2 * r]);
        const int np = __builtin_amdgcn_readfirstlane(T.p.n[dir]);
        const int ld = A.lead ? min(max(__builtin_amdgcn_readfirstlane(A.lead[r]), 0), n) : 0;
        const int len = n - ld;
        // a longer read is left alone: the host fails the call for it
        if (len <= 0 || n > TRIM_MAXREAD || np <= 0) continue;
        // column b looks at end[-b]; lane l of block(p) holds column p + l + 1's byte
        const uint8_t *end = A.text + A.s0[r] + n;
        auto block = [&](int p) { return p + lane < len ? (uint32_t)end[-(p + lane) - 1] : 0u; };
        const int cb = min(len, 63);
        uint64_t best = ~0ull;
        for (int k0 = 0; k0 < np; k0 += 64) {
            const bool act = k0 + lane < np;
            const int k = act ? k0 + lane : 0;
            const int m = T.p.len[dir * PRIMER_MAX + k];
            const uint64_t eq_a = T.p.eq[dir][0][k], eq_c = T.p.eq[dir][1][k];
            const uint64_t eq_g = T.p.eq[dir][2][k], eq_t = T.p.eq[dir][3][k];
            const uint64_t top = 1ull << (m - 1);
            auto mask = [&](uint32_t c) {
                return c == 'A' ? eq_a : c == 'C' ? eq_c : c == 'G' ? eq_g : c == 'T' ? eq_t : 0ull;
            };
            // A: lim is the least F so far, from the budget down; at: its last column
            uint64_t pa = ~0ull, ma = 0;
            int sa = m, lim = T.p.err[dir * PRIMER_MAX + k], at = 0;
            auto column_a = [&](int b, uint64_t eq) {
                const uint64_t xv = eq | ma;
                const uint64_t xh = (((eq & pa) + pa) ^ pa) | eq;
                uint64_t ph = ma | ~(xh | pa);
                uint64_t mh = pa & xh;
                sa += (ph & top ? 1 : 0) - (mh & top ? 1 : 0);
                ph <<= 1;
                mh <<= 1;
                pa = mh | ~(xv | ph);
                ma = ph & xv;
                const bool hit = sa <= lim;
                lim = hit ? sa : lim;
                at = hit ? b : at;
            };
            // B: the least (64 - (b - G)) << 12 | G << 6 | (63 - b) over its candidates
            uint64_t pb = 0, mb = 0;
            int sb = 0;
            uint32_t part_key = ~0u;
            auto column_b = [&](int b, uint64_t eq, int budget) {
                const uint64_t xv = eq | mb;
                const uint64_t xh = (((eq & pb) + pb) ^ pb) | eq;
                uint64_t ph = mb | ~(xh | pb);
                uint64_t mh = pb & xh;
                sb += (ph & top ? 1 : 0) - (mh & top ? 1 : 0);
                ph = ph << 1 | 1ull;
                mh <<= 1;
                pb = mh | ~(xv | ph);
                mb = ph & xv;
                const uint32_t key = (uint32_t)(64 - (b - sb)) << 12 | (uint32_t)sb << 6 | (uint32_t)(63 - b);
                part_key = min(part_key, b < m && sb <= budget ? key : ~0u);
            };
            uint32_t nxt = block(0);
            for (int t0 = 0; t0 < len; t0 += 64) {
                const uint32_t blk = nxt;
                nxt = block(t0 + 64);
                const int qn = min(64, len - t0);
                int q = 0;
                if (t0 == 0)
                    for (; q < cb; ++q) {
                        const uint64_t eq = mask((uint32_t)__builtin_amdgcn_readlane((int)blk, q));
                        // below min_overlap no cost is within the budget
                        const int budget = q + 1 >= min_ov ? __builtin_amdgcn_readlane(ev, q + 1) : -1;
                        column_a(q + 1, eq);
                        column_b(q + 1, eq, budget);
                    }
                for (; q < qn; ++q)
                    column_a(t0 + q + 1, mask((uint32_t)__builtin_amdgcn_readlane((int)blk, q)));
            }
            if (act && at)
                best = min(best, (uint64_t)(64 - (m - lim)) << 30 | (uint64_t)lim << 24 |
                                     (uint64_t)(TRIM_MAXREAD - at) << 8 | (uint64_t)k);
            if (act && part_key != ~0u)
                best = min(best, (uint64_t)(part_key >> 6) << 24 |
                                     (uint64_t)(TRIM_MAXREAD - 63 + (int)(part_key & 63u)) << 8 | (uint64_t)k);
        }
        for (int o = 32; o > 0; o >>= 1)
            best = min(best, (uint64_t)__shfl_xor((unsigned long long)best, o, 64));
        if (lane == 0 && best != ~0ull) {
            const int b = TRIM_MAXREAD - (int)(best >> 8 & 0xffffu);
            const int slot = dir * PRIMER_MAX + (int)(best & 255u);
            A.keep[2 * r] = n - b;
            A.keep[2 * r + 1] = min(A.keep[2 * r + 1], n - b);
            atomicAdd(&part[slot], 1ull);
            atomicAdd(&part[NS + slot], (unsigned long long)b);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * NS; i += blockDim.x)
        if (part[i]) atomicAdd(&A.stat[i], part[i]);
}


// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static inline bool py_space(unsigned char c)
{
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f);
}

using TileMap = std::unordered_map<std::string_view, int>;

// records of the FASTQ text: 4 lines each (itertools.zip_longest, :57)
static int split_records(CensorState &C, const TileMap &tiles)
{
    const char *T = C.text.data();
    const int64_t n = (int64_t)C.text.size();
    const int nt = std::max(1, std::min<int>(s2a_threads(), (int)(n >> 20) + 1));
    // newlines per chunk, then every line start at its place: 0, and the byte
    // after every newline that is not the text's last byte
    std::vector<int64_t> cnt((size_t)nt + 1, 0);
    auto chunk = [&](int t, int64_t &a, int64_t &b) { a = n * t / nt; b = n * (t + 1) / nt; };
    par_for(nt, [&](int t) {
        int64_t a, b, k = 0;
        chunk(t, a, b);
        for (const char *p = T + a, *e = T + b; p < e;) {
            const char *q = (const char *)memchr(p, '\n', (size_t)(e - p));
            if (!q) break;
            ++k;
            p = q + 1;
        }
        cnt[(size_t)t + 1] = k;
    });
    for (int t = 0; t < nt; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
    const int64_t nl = n == 0 ? 0 : 1 + cnt[(size_t)nt] - (T[n - 1] == '\n' ? 1 : 0);
    if (nl % 4) {
        set_error("censor: FASTQ has %lld lines, not a multiple of 4", (long long)nl);
        return -3;
    }
    std::unique_ptr<int64_t[]> starts(new int64_t[(size_t)std::max<int64_t>(nl, 1)]);
    if (nl) starts[0] = 0;
    par_for(nt, [&](int t) {
        int64_t a, b, k = 1 + cnt[(size_t)t];
        chunk(t, a, b);
        for (const char *p = T + a, *e = T + b; p < e;) {
            const char *q = (const char *)memchr(p, '\n', (size_t)(e - p));
            if (!q) break;
            const int64_t at = (int64_t)(q - T) + 1;
            if (at < n) starts[(size_t)k++] = at;
            p = q + 1;
        }
    });
    const int64_t nr = nl / 4;
    C.h0.resize(nr); C.s0.resize(nr); C.o0.resize(nr); C.q0.resize(nr);
    C.sl.resize(nr); C.ql.resize(nr); C.tile.resize(nr); C.sign.resize(nr);
    const int rt = std::max(1, std::min<int>(nt, (int)(nr >> 12) + 1));
    std::vector<int> bad((size_t)rt, 0);
    std::vector<int64_t> bad_rec((size_t)rt, -1);
    auto line_end = [&](int64_t k) { return k + 1 < nl ? starts[(size_t)k + 1] : n; };   // after '\n'
    auto stripped = [&](int64_t a, int64_t e) {
        while (e > a && py_space((unsigned char)T[e - 1])) --e;
        return (int32_t)(e - a);
    };
    par_for(rt, [&](int t) {
        for (int64_t r = nr * t / rt; r < nr * (t + 1) / rt; ++r) {
            const int64_t k = 4 * r;
            const int64_t ha = starts[(size_t)k], he = starts[(size_t)k + 1];
            C.h0[r] = ha;
            C.s0[r] = he;
            C.o0[r] = starts[(size_t)k + 2];
            C.q0[r] = starts[(size_t)k + 3];
            C.sl[r] = stripped(he, C.o0[r]);
            C.ql[r] = stripped(C.q0[r], line_end(k + 3));
            // ident.split(' ') -> fields[0].split(':')[4] (tile),
            // fields[1].split(':')[0] (read direction); the line keeps its '\n'
            const char *h = T + ha;
            const int64_t hn = he - ha;
            const char *spp = (const char *)memchr(h, ' ', (size_t)hn);
            if (!spp) { bad[(size_t)t] = 1; bad_rec[(size_t)t] = r; break; }
            const int64_t sp = spp - h;
            int64_t f = 0, colon = 0;
            while (f < sp && colon < 4) { if (h[f] == ':') ++colon; ++f; }
            if (colon < 4) { bad[(size_t)t] = 2; bad_rec[(size_t)t] = r; break; }
            int64_t g = f;
            while (g < sp && h[g] != ':') ++g;
            int64_t d = sp + 1, de = d;
            while (de < hn && h[de] != ' ' && h[de] != ':') ++de;
            C.sign[r] = (de - d == 1 && h[d] == '1') ? 1 : -1;
            auto it = tiles.find(std::string_view(h + f, (size_t)(g - f)));
            C.tile[r] = it == tiles.end() ? -1 : it->second;
        }
    });
    for (int t = 0; t < rt; ++t)
        if (bad[(size_t)t]) {
            set_error(bad[(size_t)t] == 1 ? "censor: header of record %lld has no space (ValueError)"
                                          : "censor: header of record %lld has no tile field (IndexError)",
                      (long long)(bad_rec[(size_t)t] + 1));
            return -3;
        }
    return 0;
}

// k_censor over the records: the text up, censored in place, down again
static int censor_run(Ctx &c, CensorState &C, const TileMap &tid, int n_bad, const char *const *tiles,
                      const int32_t *cycles)
{
    const int64_t nr = (int64_t)C.h0.size();
    C.keep.assign(2 * (size_t)nr, 0);
    C.base_count = C.score_sum = 0;
    std::fill(std::begin(C.trim_reads), std::end(C.trim_reads), 0);
    std::fill(std::begin(C.trim_bases), std::end(C.trim_bases), 0);
    std::fill(std::begin(C.primer_reads), std::end(C.primer_reads), 0);
    std::fill(std::begin(C.primer_bases), std::end(C.primer_bases), 0);
    std::fill(std::begin(C.primer3_reads), std::end(C.primer3_reads), 0);
    std::fill(std::begin(C.primer3_bases), std::end(C.primer3_bases), 0);
    C.lead.clear();
    if (nr == 0) return 0;
    if (C.primer_on) C.lead.assign((size_t)nr, 0);
    // bad-cycle bitmaps per bad tile id, over the cycles of the reads
    int maxc = 1;
    for (int64_t r = 0; r < nr; ++r) maxc = std::max(maxc, std::max(C.sl[r], C.ql[r]));
    const int words = (2 * maxc + 1 + 31) / 32;
    std::vector<uint32_t> bm((size_t)std::max(1, (int)tid.size()) * words, 0u);
    for (int k = 0; k < n_bad; ++k) {
        const int c0 = cycles[k];
        if (c0 < -maxc || c0 > maxc) continue;
        const int b = c0 + maxc;
        bm[(size_t)tid.at(std::string_view(tiles[k])) * words + (b >> 5)] |= 1u << (b & 31);
    }
    hipStream_t s = c.stream;
    int st = 0;
    auto H = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && !st) st = hip_fail(e, what);
        return st == 0;
    };
    CensorState &D = C;
    if ((int64_t)C.text.size() + 1 > D.cap_text) {
        hipFree(D.d_text);
        D.d_text = nullptr;
        D.cap_text = (int64_t)C.text.size() + 1;
        H(hipMalloc(&D.d_text, D.cap_text), "hipMalloc text");
    }
    if (nr > D.cap_rec) {
        hipFree(D.d_s0); hipFree(D.d_q0); hipFree(D.d_sl); hipFree(D.d_ql);
        hipFree(D.d_tile); hipFree(D.d_sign); hipFree(D.d_keep); hipFree(D.d_lead);
        D.d_lead = nullptr;
        D.cap_rec = nr;
        H(hipMalloc(&D.d_s0, 8 * nr), "hipMalloc");
        H(hipMalloc(&D.d_q0, 8 * nr), "hipMalloc");
        H(hipMalloc(&D.d_sl, 4 * nr), "hipMalloc");
        H(hipMalloc(&D.d_ql, 4 * nr), "hipMalloc");
        H(hipMalloc(&D.d_tile, 4 * nr), "hipMalloc");
        H(hipMalloc(&D.d_sign, 4 * nr), "hipMalloc");
        H(hipMalloc(&D.d_keep, 8 * nr), "hipMalloc");
    }
    if ((int64_t)bm.size() > D.cap_bad) {
        hipFree(D.d_bad);
        D.cap_bad = (int64_t)bm.size();
        H(hipMalloc(&D.d_bad, 4 * bm.size()), "hipMalloc");
    }
    if (!D.d_sums) H(hipMalloc(&D.d_sums, 16), "hipMalloc");
    constexpr size_t tstat_bytes = 2 * 2 * TRIM_MAXADAPT * sizeof(unsigned long long);
    if (C.trim_on && !D.d_trim) H(hipMalloc(&D.d_trim, sizeof(TrimTab)), "hipMalloc");
    if (C.trim_on && !D.d_tstat) H(hipMalloc(&D.d_tstat, tstat_bytes), "hipMalloc");
    constexpr size_t pstat_bytes = 2 * 2 * PRIMER_MAX * sizeof(unsigned long long);
    if (C.primer_on && !D.d_primer) H(hipMalloc(&D.d_primer, sizeof(PrimerTab)), "hipMalloc");
    if (C.primer_on && !D.d_pstat) H(hipMalloc(&D.d_pstat, pstat_bytes), "hipMalloc");
    if (C.primer_on && !D.d_lead) H(hipMalloc(&D.d_lead, 4 * D.cap_rec), "hipMalloc");
    if (C.primer3_on && !D.d_primer3) H(hipMalloc(&D.d_primer3, sizeof(Primer3Tab)), "hipMalloc");
    if (C.primer3_on && !D.d_p3stat) H(hipMalloc(&D.d_p3stat, pstat_bytes), "hipMalloc");
    if (st) { censor_free_device(D); return st; }
    H(hipMemcpyAsync(D.d_text, C.text.data(), C.text.size(), hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_s0, C.s0.data(), 8 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_q0, C.q0.data(), 8 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_sl, C.sl.data(), 4 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_ql, C.ql.data(), 4 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_tile, C.tile.data(), 4 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_sign, C.sign.data(), 4 * nr, hipMemcpyHostToDevice, s), "H2D");
    H(hipMemcpyAsync(D.d_bad, bm.data(), 4 * bm.size(), hipMemcpyHostToDevice, s), "H2D");
    H(hipMemsetAsync(D.d_sums, 0, 16, s), "memset");
    CensorArgs a{D.d_text, D.d_s0, D.d_q0, D.d_sl, D.d_ql, D.d_tile, D.d_sign, nr, D.d_bad, maxc,
                 words, D.d_keep, D.d_sums};
    int64_t blocks = (nr + 3) / 4;
    if (blocks > 256 * 64) blocks = 256 * 64;
    if (!st) {
        const int pk = prof_begin(c, "k_censor");
        hipLaunchKernelGGL(k_censor, dim3((unsigned)blocks), dim3(256), 0, s, a);
        prof_end(c, pk);
        H(hipGetLastError(), "k_censor");
    }
    unsigned long long tstat[2 * 2 * TRIM_MAXADAPT] = {};
    if (C.trim_on && !st) {   // on the censored text, before it goes down
        H(hipMemcpyAsync(D.d_trim, &C.trim, sizeof(TrimTab), hipMemcpyHostToDevice, s), "H2D");
        H(hipMemsetAsync(D.d_tstat, 0, tstat_bytes, s), "memset");
        TrimArgs ta{D.d_text, D.d_s0, D.d_sign, nr, D.d_keep, D.d_trim, D.d_tstat};
        if (!st) {
            const int pk = prof_begin(c, "k_trim");
            hipLaunchKernelGGL(k_trim, dim3((unsigned)blocks), dim3(256), 0, s, ta);
            prof_end(c, pk);
            H(hipGetLastError(), "k_trim");
        }
        H(hipMemcpyAsync(tstat, D.d_tstat, tstat_bytes, hipMemcpyDeviceToHost, s), "D2H");
    }
    std::vector<unsigned long long> pstat;
    if (C.primer_on && !st) {   // on what k_censor and k_trim kept
        pstat.assign(2 * 2 * PRIMER_MAX, 0);
        H(hipMemcpyAsync(D.d_primer, &C.primer, sizeof(PrimerTab), hipMemcpyHostToDevice, s), "H2D");
        H(hipMemsetAsync(D.d_pstat, 0, pstat_bytes, s), "memset");
        PrimerArgs pa{D.d_text, D.d_s0, D.d_sign, nr, D.d_keep, D.d_lead, D.d_primer, D.d_pstat};
        if (!st) {
            const int pk = prof_begin(c, "k_primer");
            hipLaunchKernelGGL(k_primer, dim3((unsigned)blocks), dim3(256), 0, s, pa);
            prof_end(c, pk);
            H(hipGetLastError(), "k_primer");
        }
        H(hipMemcpyAsync(pstat.data(), D.d_pstat, pstat_bytes, hipMemcpyDeviceToHost, s), "D2H");
        H(hipMemcpyAsync(C.lead.data(), D.d_lead, 4 * nr, hipMemcpyDeviceToHost, s), "D2H");
    }
    std::vector<unsigned long long> p3stat;
    if (C.primer3_on && !st) {   // on what the three passes before kept, behind k_primer's lead
        p3stat.assign(2 * 2 * PRIMER_MAX, 0);
        H(hipMemcpyAsync(D.d_primer3, C.primer3.get(), sizeof(Primer3Tab), hipMemcpyHostToDevice, s), "H2D");
        H(hipMemsetAsync(D.d_p3stat, 0, pstat_bytes, s), "memset");
        Primer3Args pa{D.d_text, D.d_s0, D.d_sign, nr, D.d_keep, C.primer_on ? D.d_lead : nullptr,
                       D.d_primer3, D.d_p3stat};
        if (!st) {
            const int pk = prof_begin(c, "k_primer3");
            hipLaunchKernelGGL(k_primer3, dim3((unsigned)blocks), dim3(256), 0, s, pa);
            prof_end(c, pk);
            H(hipGetLastError(), "k_primer3");
        }
        H(hipMemcpyAsync(p3stat.data(), D.d_p3stat, pstat_bytes, hipMemcpyDeviceToHost, s), "D2H");
    }
    unsigned long long sums[2] = {0, 0};
    H(hipMemcpyAsync(C.text.data(), D.d_text, C.text.size(), hipMemcpyDeviceToHost, s), "D2H");
    H(hipMemcpyAsync(C.keep.data(), D.d_keep, 8 * nr, hipMemcpyDeviceToHost, s), "D2H");
    H(hipMemcpyAsync(sums, D.d_sums, 16, hipMemcpyDeviceToHost, s), "D2H");
    H(hipStreamSynchronize(s), "sync");
    if (st) return st;
    prof_flush(c);
    C.score_sum = (long long)sums[0];
    C.base_count = (long long)sums[1];
    if (C.trim_on || C.primer3_on) {
        // k_trim and k_primer3 leave a read past their cap alone (its kept
        // length is still k_censor's): such a read fails the call
        if (maxc > TRIM_MAXREAD)
            for (int64_t r = 0; r < nr; ++r)
                if (C.keep[2 * r] > TRIM_MAXREAD) {
                    const char *h = C.text.data() + C.h0[r];
                    const int hl = (int)std::min<int64_t>(C.s0[r] - C.h0[r], 80);
                    int e = 0;
                    while (e < hl && !py_space((unsigned char)h[e])) ++e;
                    set_error("censor: record %lld (%.*s) keeps %d bases, adapter trimming takes reads "
                              "of at most %d", (long long)(r + 1), e, h, (int)C.keep[2 * r], TRIM_MAXREAD);
                    return -3;
                }
        for (int k = 0; k < 2 * TRIM_MAXADAPT; ++k) {
            C.trim_reads[k] = (int64_t)tstat[k];
            C.trim_bases[k] = (int64_t)tstat[2 * TRIM_MAXADAPT + k];
        }
    }
    if (C.primer_on)
        for (int k = 0; k < 2 * PRIMER_MAX; ++k) {
            C.primer_reads[k] = (int64_t)pstat[(size_t)k];
            C.primer_bases[k] = (int64_t)pstat[(size_t)(2 * PRIMER_MAX + k)];
        }
    if (C.primer3_on)
        for (int k = 0; k < 2 * PRIMER_MAX; ++k) {
            C.primer3_reads[k] = (int64_t)p3stat[(size_t)k];
            C.primer3_bases[k] = (int64_t)p3stat[(size_t)(2 * PRIMER_MAX + k)];
        }
    return 0;
}

// The censored records, rewritten (header and '+' lines verbatim, seq and
// qual from their lead, if primers are set, to their kept length, each line
// ending in '\n') and, for gzip,
// deflated, in blocks of records of about CENSOR_BLOCK input bytes, one gzip
// member per block; the blocks are made by every host thread in turn and
// placed into C.out by their precomputed offsets.
constexpr int64_t CENSOR_BLOCK = (int64_t)8 << 20;

static int censor_emit(CensorState &C, int dst_gzip)
{
    const int64_t nr = (int64_t)C.h0.size();
    const int64_t n = (int64_t)C.text.size();
    std::vector<int64_t> bstart{0};
    for (int64_t r = 0, base = 0; r < nr; ++r) {
        if (C.h0[r] - base >= CENSOR_BLOCK) { bstart.push_back(r); base = C.h0[r]; }
    }
    if (nr > 0) bstart.push_back(nr);
    const int64_t nb = (int64_t)bstart.size() - 1;
    if (nb <= 0) {
        C.out.clear();
        if (dst_gzip) {   // an empty FASTQ still makes one (empty) gzip member
            if (gzip_member("", 0, C.out, 1)) { set_error("censor: deflate failed"); return -2; }
        }
        if (C.sink_fd >= 0 && C.out.size()) {
            if (const int e = write_all_at(C.sink_fd, C.out.data(), C.out.size(), C.sink_pos)) {
                set_error("censor: write failed (%s)", strerror(e));
                return -4;
            }
            C.sink_pos += (int64_t)C.out.size();
            C.out.clear();
        }
        return 0;
    }
    std::vector<TextBuf> part((size_t)nb);
    std::atomic<int64_t> next(0);
    std::atomic<int> err(0);
    const char *T = C.text.data();
    const int32_t *lead = C.lead.empty() ? nullptr : C.lead.data();
    const bool stream = C.sink_fd >= 0;
    // streamed: thread 0 writes the blocks in order as the others finish them
    const int nt = std::max(stream ? 2 : 1, std::min<int>(s2a_threads(), (int)nb + (stream ? 1 : 0)));
    std::unique_ptr<std::atomic<int>[]> done(new std::atomic<int>[(size_t)nb]);
    for (int64_t b = 0; b < nb; ++b) done[b].store(0);
    std::atomic<int> dead(0);   // a block maker failed: the writer stops waiting
    auto write_blocks = [&]() {
        for (int64_t b = 0; b < nb; ++b) {
            while (!done[b].load(std::memory_order_acquire) && !dead) std::this_thread::yield();
            if (dead || err) return;
            TextBuf &blk = part[(size_t)b];
            if ((C.sink_err = write_all_at(C.sink_fd, blk.data(), blk.size(), C.sink_pos))) { dead = 1; return; }
            C.sink_pos += (int64_t)blk.size();
            blk.release();
        }
    };
    par_for(nt, [&](int t) {
        if (stream && t == 0) { write_blocks(); return; }
        TextBuf raw;
        struct Dead {   // a throw out of a block maker releases the writer
            std::atomic<int> &d;
            bool ok = false;
            ~Dead() { if (!ok) d = 1; }
        } guard{dead};
        for (int64_t b; !dead && (b = next.fetch_add(1)) < nb;) {
            const int64_t r0 = bstart[(size_t)b], r1 = bstart[(size_t)b + 1];
            const int64_t in_end = r1 < nr ? C.h0[r1] : n;
            TextBuf &dst = dst_gzip ? raw : part[(size_t)b];
            dst.resize((size_t)(in_end - C.h0[r0] + 2 * (r1 - r0)));
            char *o = dst.data();
            for (int64_t r = r0; r < r1; ++r) {
                const size_t hl = (size_t)(C.s0[r] - C.h0[r]), pl = (size_t)(C.q0[r] - C.o0[r]);
                const size_t ks = (size_t)C.keep[2 * r], kq = (size_t)C.keep[2 * r + 1];
                // a lead is at most the kept sequence length
                const size_t ls = lead ? std::min((size_t)lead[r], ks) : 0, lq = std::min(ls, kq);
                memcpy(o, T + C.h0[r], hl); o += hl;
                memcpy(o, T + C.s0[r] + ls, ks - ls); o += ks - ls;
                *o++ = '\n';
                memcpy(o, T + C.o0[r], pl); o += pl;
                memcpy(o, T + C.q0[r] + lq, kq - lq); o += kq - lq;
                *o++ = '\n';
            }
            dst.resize((size_t)(o - dst.data()));
            if (dst_gzip && gzip_member(raw.data(), raw.size(), part[(size_t)b], 1)) { err = 1; dead = 1; }
            done[b].store(1, std::memory_order_release);
        }
        guard.ok = true;
    });
    if (err) { set_error("censor: deflate failed"); return -2; }
    if (stream) {
        if (C.sink_err) { set_error("censor: write failed (%s)", strerror(C.sink_err)); return -4; }
        return 0;
    }
    std::vector<size_t> off((size_t)nb + 1, 0);
    for (int64_t b = 0; b < nb; ++b) off[(size_t)b + 1] = off[(size_t)b] + part[(size_t)b].size();
    C.out.resize(off[(size_t)nb]);
    next = 0;
    par_for(nt, [&](int) {
        for (int64_t b; (b = next.fetch_add(1)) < nb;) {
            memcpy(C.out.data() + off[(size_t)b], part[(size_t)b].data(), part[(size_t)b].size());
            part[(size_t)b].release();
        }
    });
    return 0;
}

// one FASTQ text (moved into C.text) through split, k_censor and the rewrite
static int censor_text(Ctx &c, CensorState &C, int n_bad, const char *const *tiles,
                       const int32_t *cycles, int dst_gzip, std::chrono::steady_clock::time_point t0)
{
    TileMap tid;
    for (int k = 0; k < n_bad; ++k) tid.emplace(std::string_view(tiles[k]), (int)tid.size());
    if (int st = split_records(C, tid)) return st;
    C.t_host_in = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    if (int st = censor_run(c, C, tid, n_bad, tiles, cycles)) return st;
    C.t_device = ms_since(t1);
    const auto t2 = std::chrono::steady_clock::now();
    const int st = censor_emit(C, dst_gzip);
    C.t_host_out = ms_since(t2);
    // the text and record tables are not needed past the call: freed on a
    // detached thread (a GB-sized free is tens of ms)
    auto *old = new TextBuf();
    old->swap(C.text);
    std::thread([old]() { delete old; }).detach();
    return st;
}

// censor_text with an allocation failure (here or in a worker) as status -2
static int censor_text_guarded(Ctx &c, CensorState &C, int n_bad, const char *const *tiles,
                               const int32_t *cycles, int dst_gzip,
                               std::chrono::steady_clock::time_point t0)
{
    try {
        return censor_text(c, C, n_bad, tiles, cycles, dst_gzip, t0);
    } catch (const std::exception &e) {
        set_error("censor: out of memory (%s)", e.what());
        return -2;
    }
}

static bool censor_args_ok(mh_ctx *ctx, int n_bad, const char *const *tiles, const int32_t *cycles)
{
    return ctx && n_bad >= 0 && (!n_bad || (tiles && cycles));
}

}  // namespace mh

using namespace mh;

extern "C" int mh_censor_fastq(mh_ctx *ctx, const uint8_t *src, int64_t len, int src_gzip,
                               int n_bad, const char *const *tiles, const int32_t *cycles,
                               int dst_gzip, int64_t *base_count, int64_t *score_sum)
{
    if (!censor_args_ok(ctx, n_bad, tiles, cycles) || (len && !src) || len < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    C.out.clear();
    C.base_count = C.score_sum = 0;
    C.t_host_in = C.t_device = C.t_host_out = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (src_gzip) {
        std::string why;
        if (gunzip_buffer(src, len, C.text, why)) {
            set_error("censor: %s", why.c_str());
            return -3;
        }
    } else {
        try {
            C.text.assign((const char *)src, (size_t)len);
        } catch (const std::exception &) {
            set_error("censor: out of memory");
            return -2;
        }
    }
    if (int st = censor_text_guarded(c, C, n_bad, tiles, cycles, dst_gzip, t0)) { C.out.clear(); return st; }
    if (base_count) *base_count = C.base_count;
    if (score_sum) *score_sum = C.score_sum;
    return 0;
}

extern "C" int mh_censor_staged(mh_ctx *ctx, mh_fastq *fq, int n_bad, const char *const *tiles,
                                const int32_t *cycles, int dst_gzip, int64_t *out_bytes,
                                int64_t *base_count, int64_t *score_sum)
{
    if (!censor_args_ok(ctx, n_bad, tiles, cycles) || !fq) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    C.out.clear();
    C.base_count = C.score_sum = 0;
    C.t_host_in = C.t_device = C.t_host_out = 0;
    const auto t0 = std::chrono::steady_clock::now();
    TextBuf text = take_fastq_text(fq);
    C.text.swap(text);
    if (int st = censor_text_guarded(c, C, n_bad, tiles, cycles, dst_gzip, t0)) { C.out.clear(); return st; }
    if (out_bytes) *out_bytes = (int64_t)C.out.size();
    if (base_count) *base_count = C.base_count;
    if (score_sum) *score_sum = C.score_sum;
    return 0;
}

extern "C" int mh_censor_staged_write(mh_ctx *ctx, mh_fastq *fq, int n_bad, const char *const *tiles,
                                      const int32_t *cycles, int dst_gzip, int fd, int64_t offset,
                                      int64_t *written, int64_t *base_count, int64_t *score_sum)
{
    if (!censor_args_ok(ctx, n_bad, tiles, cycles) || !fq || fd < 0 || offset < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    C.out.clear();
    C.base_count = C.score_sum = 0;
    C.t_host_in = C.t_device = C.t_host_out = 0;
    C.sink_fd = fd;
    C.sink_pos = offset;
    C.sink_err = 0;
    const auto t0 = std::chrono::steady_clock::now();
    TextBuf text = take_fastq_text(fq);
    C.text.swap(text);
    const int st = censor_text_guarded(c, C, n_bad, tiles, cycles, dst_gzip, t0);
    C.sink_fd = -1;
    if (st) return st;
    if (written) *written = C.sink_pos - offset;
    if (base_count) *base_count = C.base_count;
    if (score_sum) *score_sum = C.score_sum;
    return 0;
}

extern "C" int mh_censor_output(mh_ctx *ctx, char *buf, size_t cap, size_t *used)
{
    if (!ctx || !used) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) { set_error("mh_censor_output: no censor results"); return -3; }
    CensorState &C = *c.censor;
    *used = C.out.size();
    if (!buf) return 0;
    if (cap < C.out.size()) { set_error("mh_censor_output: buffer too small"); return -2; }
    if (C.out.size()) memcpy(buf, C.out.data(), C.out.size());
    C.out.release();
    return 0;
}

extern "C" int mh_censor_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written)
{
    if (!ctx || fd < 0 || offset < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) { set_error("mh_censor_write: no censor results"); return -3; }
    CensorState &C = *c.censor;
    if (const int e = write_all_at(fd, C.out.data(), C.out.size(), offset)) {
        set_error("mh_censor_write: write failed (%s)", strerror(e));
        return -4;
    }
    if (written) *written = (int64_t)C.out.size();
    C.out.release();
    return 0;
}

extern "C" int mh_censor_timing(mh_ctx *ctx, double *ms3)
{
    if (!ctx || !ms3) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) { set_error("mh_censor_timing: no censor results"); return -3; }
    ms3[0] = c.censor->t_host_in;
    ms3[1] = c.censor->t_device;
    ms3[2] = c.censor->t_host_out;
    return 0;
}

extern "C" int mh_censor_set_adapters(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                                      const char *const *seqs2, int min_overlap,
                                      const int32_t *max_errors)
{
    if (!ctx) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    std::fill(std::begin(C.trim_reads), std::end(C.trim_reads), 0);
    std::fill(std::begin(C.trim_bases), std::end(C.trim_bases), 0);
    if (n1 == 0 && n2 == 0) { C.trim_on = false; return 0; }
    TrimTab T{};
    const int n[2] = {n1, n2};
    const char *const *seqs[2] = {seqs1, seqs2};
    for (int d = 0; d < 2; ++d) {
        if (n[d] < 0 || n[d] > TRIM_MAXADAPT || (n[d] && !seqs[d])) {
            set_error("censor: %d adapters for read direction %d (0 to %d)", n[d], d + 1, TRIM_MAXADAPT);
            return -3;
        }
        T.n[d] = n[d];
        for (int k = 0; k < n[d]; ++k) {
            const char *a = seqs[d][k];
            const size_t m = a ? strnlen(a, TRIM_MAXLEN + 1) : 0;
            if (m < 3 || m > (size_t)TRIM_MAXLEN || strspn(a, "ACGT") != m) {
                set_error("censor: adapter %d of read direction %d is not 3 to %d bases of ACGT", k, d + 1,
                          TRIM_MAXLEN);
                return -3;
            }
            T.len[d * TRIM_MAXADAPT + k] = (int32_t)m;
            memcpy(T.seq[d * TRIM_MAXADAPT + k], a, m);
        }
    }
    if (min_overlap < 1) { set_error("censor: min_overlap %d is below 1", min_overlap); return -3; }
    T.min_overlap = min_overlap;
    if (!max_errors) { set_error("censor: no error table"); return -3; }
    for (int i = 0; i <= TRIM_MAXLEN; ++i) {
        // an error rate below 1 allows fewer than i errors in i bases
        if (max_errors[i] < 0 || max_errors[i] >= std::max(i, 1)) {
            set_error("censor: %d errors allowed in %d adapter bases", (int)max_errors[i], i);
            return -3;
        }
        T.max_err[i] = max_errors[i];
    }
    C.trim = T;
    C.trim_on = true;
    return 0;
}

extern "C" int mh_censor_trim_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases)
{
    if (!ctx || !reads || !bases) return -3;
    Ctx &c = *ctx_of(ctx);
    for (int k = 0; k < 2 * TRIM_MAXADAPT; ++k) {
        reads[k] = c.censor ? c.censor->trim_reads[k] : 0;
        bases[k] = c.censor ? c.censor->trim_bases[k] : 0;
    }
    return 0;
}

extern "C" int mh_censor_set_primers(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                                     const char *const *seqs2, const int32_t *max_errors)
{
    if (!ctx) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    std::fill(std::begin(C.primer_reads), std::end(C.primer_reads), 0);
    std::fill(std::begin(C.primer_bases), std::end(C.primer_bases), 0);
    if (n1 == 0 && n2 == 0) { C.primer_on = false; return 0; }
    if (!max_errors) { set_error("censor: no error table"); return -3; }
    for (int i = 0; i <= PRIMER_MAXLEN; ++i) {
        // the fields of k_primer's key: fewer than i errors in i bases, the
        // last column i + errors within PRIMER_MAXCOL
        if (max_errors[i] < 0 || max_errors[i] >= std::max(i, 1) || i + max_errors[i] > PRIMER_MAXCOL) {
            set_error("censor: %d errors allowed in %d primer bases", (int)max_errors[i], i);
            return -3;
        }
    }
    std::unique_ptr<PrimerTab> T(new PrimerTab());
    const int n[2] = {n1, n2};
    const char *const *seqs[2] = {seqs1, seqs2};
    for (int d = 0; d < 2; ++d) {
        if (n[d] < 0 || n[d] > PRIMER_MAX || (n[d] && !seqs[d])) {
            set_error("censor: %d primers for read direction %d (0 to %d)", n[d], d + 1, PRIMER_MAX);
            return -3;
        }
        T->n[d] = n[d];
        for (int k = 0; k < n[d]; ++k) {
            const char *p = seqs[d][k];
            const size_t m = p ? strnlen(p, PRIMER_MAXLEN + 1) : 0;
            if (m < (size_t)PRIMER_MINLEN || m > (size_t)PRIMER_MAXLEN || strspn(p, "ACGT") != m) {
                set_error("censor: primer %d of read direction %d (%.70s) is not %d to %d bases of ACGT", k, d + 1,
                          p ? p : "", PRIMER_MINLEN, PRIMER_MAXLEN);
                return -3;
            }
            const int slot = d * PRIMER_MAX + k;
            T->len[slot] = (int32_t)m;
            T->err[slot] = max_errors[m];
            T->cols[d] = std::max(T->cols[d], (int32_t)m + max_errors[m]);
            for (size_t i = 0; i < m; ++i)
                T->eq[d][strchr("ACGT", p[i]) - "ACGT"][k] |= (uint64_t)1 << i;
        }
    }
    C.primer = *T;
    C.primer_on = true;
    return 0;
}

extern "C" int mh_censor_primer_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases)
{
    if (!ctx || !reads || !bases) return -3;
    Ctx &c = *ctx_of(ctx);
    for (int k = 0; k < 2 * PRIMER_MAX; ++k) {
        reads[k] = c.censor ? c.censor->primer_reads[k] : 0;
        bases[k] = c.censor ? c.censor->primer_bases[k] : 0;
    }
    return 0;
}

extern "C" int mh_censor_set_primers3(mh_ctx *ctx, int n1, const char *const *seqs1, int n2,
                                      const char *const *seqs2, int min_overlap,
                                      const int32_t *max_errors)
{
    if (!ctx) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.censor) c.censor = new CensorState();
    CensorState &C = *c.censor;
    std::fill(std::begin(C.primer3_reads), std::end(C.primer3_reads), 0);
    std::fill(std::begin(C.primer3_bases), std::end(C.primer3_bases), 0);
    if (n1 == 0 && n2 == 0) { C.primer3_on = false; return 0; }
    if (min_overlap < 1 || min_overlap > PRIMER_MAXLEN) {
        set_error("censor: 3' primer min_overlap %d is not in 1 to %d", min_overlap, PRIMER_MAXLEN);
        return -3;
    }
    if (!max_errors) { set_error("censor: no error table"); return -3; }
    std::unique_ptr<Primer3Tab> T(new Primer3Tab());
    T->min_overlap = min_overlap;
    for (int i = 0; i <= PRIMER_MAXLEN; ++i) {
        // the fields of k_primer3's key: fewer than i errors in i bases
        if (max_errors[i] < 0 || max_errors[i] >= std::max(i, 1)) {
            set_error("censor: %d errors allowed in %d 3' primer bases", (int)max_errors[i], i);
            return -3;
        }
        T->max_err[i] = max_errors[i];
    }
    const int n[2] = {n1, n2};
    const char *const *seqs[2] = {seqs1, seqs2};
    for (int d = 0; d < 2; ++d) {
        if (n[d] < 0 || n[d] > PRIMER_MAX || (n[d] && !seqs[d])) {
            set_error("censor: %d 3' primers for read direction %d (0 to %d)", n[d], d + 1, PRIMER_MAX);
            return -3;
        }
        T->p.n[d] = n[d];
        for (int k = 0; k < n[d]; ++k) {
            const char *p = seqs[d][k];
            const size_t m = p ? strnlen(p, PRIMER_MAXLEN + 1) : 0;
            if (m < (size_t)PRIMER_MINLEN || m > (size_t)PRIMER_MAXLEN || strspn(p, "ACGT") != m) {
                set_error("censor: 3' primer %d of read direction %d (%.70s) is not %d to %d bases of ACGT", k,
                          d + 1, p ? p : "", PRIMER_MINLEN, PRIMER_MAXLEN);
                return -3;
            }
            const int slot = d * PRIMER_MAX + k;
            T->p.len[slot] = (int32_t)m;
            T->p.err[slot] = max_errors[m];
            // the scan runs backwards: row i of the column is base m - 1 - i
            for (size_t i = 0; i < m; ++i)
                T->p.eq[d][strchr("ACGT", p[m - 1 - i]) - "ACGT"][k] |= (uint64_t)1 << i;
        }
    }
    C.primer3 = std::move(T);
    C.primer3_on = true;
    return 0;
}

extern "C" int mh_censor_primer3_stats(mh_ctx *ctx, int64_t *reads, int64_t *bases)
{
    if (!ctx || !reads || !bases) return -3;
    Ctx &c = *ctx_of(ctx);
    for (int k = 0; k < 2 * PRIMER_MAX; ++k) {
        reads[k] = c.censor ? c.censor->primer3_reads[k] : 0;
        bases[k] = c.censor ? c.censor->primer3_bases[k] : 0;
    }
    return 0;
}
