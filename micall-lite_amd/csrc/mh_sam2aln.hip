// mh_sam2aln.hip -- sam2aln on gfx950: the read-pair merge and the count of
// identical merged sequences that micall/core/sam2aln.py:395-478 runs in
// Python over remap.csv, behind mh_sam2aln_csv / mh_sam2aln_output.
//
//   host   remap.csv -> rows (DictReader), matchmaker (sam2aln.py:291-312),
//          the row-level failure causes of parse_sam (:340-348) and the
//          apply_cigar checks that raise (:113-151); insert.csv / failed.csv
//          text and the final ordering of aligned.csv (:465-478)
//   k_s2a_merge   one wave64 per pair: apply_cigar of both mates into LDS
//                 once, then for each of the call's n_cut q-cutoffs (:391-402)
//                 merge_pairs (no insertions, :156-237) lane-parallel, the
//                 prop_N test (:381-385), the merged sequence written to HBM
//                 and hashed (two 64-bit position-keyed sums).  One "merge
//                 entry" is (pair, cutoff k): entry = pair * n_cut + k
//   k_s2a_count   one thread per entry: open-addressing table keyed by
//                 the hash, count + first entry per distinct sequence of a
//                 group (rname, cutoff)
//   k_s2a_verify  one wave per entry: every member of a group is
//                 compared byte for byte with the group's first member
//                 (a hash collision is reported, never merged silently)
//   k_s2a_gather  distinct sequences copied out for the host's sort
//   k_s2a_stage   mh_sam2aln_resident: the rows k_s2a_merge reads, built from
//                 the resident packed reads and the last mapping pass's
//                 records instead of parsed from remap.csv and uploaded
//   k_s2a_clip, k_s2a_clip_scan   only when mh_sam2aln_clipping asks: the
//                 positions each merged unit soft-clips and no mate aligns,
//                 counted per reference (clipping.csv; no reference code)
//   k_s2a_ins_rec, k_s2a_ins_merge, k_s2a_ins_tab   only when
//                 mh_sam2aln_conseq_ins asks: the mates' insertions keyed by
//                 consensus position, merged as merge_inserts does
//                 (sam2aln.py:240-273) and counted per distinct string
//                 (conseq_ins.csv)
//   k_s2a_conc, k_s2a_conc_scan   only when mh_sam2aln_concordance asks: where
//                 the two mates of a unit both align and how often they
//                 disagree, per consensus position and per read cycle and
//                 quality (concordance.csv, cycle_concordance.csv; no
//                 reference code)
//   k_s2a_strand, k_s2a_strand_scan   only when mh_sam2aln_strand asks: per
//                 position and merged base the units whose supporting mate is
//                 forward, reversed or both (strand.csv; no reference code)
// Bit-for-bit specification: the reference itself (tests/golden/e2e/*/aligned.csv
// etc. were produced by running micall.core.sam2aln on the same remap.csv).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "mh_gunzip.h"
#include "mh_sam2aln.h"
#include "mh_text.h"

namespace mh {

static void s2a_free_device(S2AState &S)
{
    hipFree(S.d_seq); hipFree(S.d_qual); hipFree(S.d_out); hipFree(S.d_gather);
    hipFree(S.d_soff); hipFree(S.d_units); hipFree(S.d_slot); hipFree(S.d_goff);
    hipFree(S.d_pos); hipFree(S.d_cigoff); hipFree(S.d_ncig);
    hipFree(S.d_uref); hipFree(S.d_res); hipFree(S.d_tcnt); hipFree(S.d_trep);
    hipFree(S.d_uniq); hipFree(S.d_ctr); hipFree(S.d_cig); hipFree(S.d_h); hipFree(S.d_tkey);
    hipFree(S.d_flag); hipFree(S.d_samref); hipFree(S.d_spanins);
    S.d_flag = S.d_samref = S.d_spanins = nullptr;
    S.staged_reads = -1;
    S.d_seq = S.d_qual = S.d_out = S.d_gather = nullptr;
    S.d_soff = S.d_units = S.d_slot = S.d_goff = nullptr;
    S.d_pos = S.d_cigoff = S.d_ncig = S.d_uref = S.d_res = S.d_tcnt = S.d_trep =
        S.d_uniq = S.d_ctr = nullptr;
    S.d_cig = nullptr;
    S.d_h = S.d_tkey = nullptr;
    S2AClip &K = S.clip;
    hipFree(K.d_lo); hipFree(K.d_base); hipFree(K.d_wlen); hipFree(K.d_diff); hipFree(K.d_idx);
    hipFree(K.d_cnt); hipFree(K.d_n);
    K.d_lo = K.d_base = nullptr;
    K.d_wlen = K.d_diff = K.d_idx = K.d_cnt = K.d_n = nullptr;
    K.state = CLIP_NONE;
    S2AIns &I = S.ins;
    hipFree(I.d_list); hipFree(I.d_res); hipFree(I.d_rref); hipFree(I.d_tcnt); hipFree(I.d_trep);
    hipFree(I.d_uniq); hipFree(I.d_ctr); hipFree(I.d_recoff); hipFree(I.d_byteoff); hipFree(I.d_slot);
    hipFree(I.d_goff); hipFree(I.d_rec); hipFree(I.d_h); hipFree(I.d_tkey); hipFree(I.d_out);
    hipFree(I.d_gather);
    I.d_list = I.d_res = I.d_rref = I.d_tcnt = I.d_trep = I.d_uniq = I.d_ctr = nullptr;
    I.d_recoff = I.d_byteoff = I.d_slot = I.d_goff = nullptr;
    I.d_rec = nullptr;
    I.d_h = I.d_tkey = nullptr;
    I.d_out = I.d_gather = nullptr;
    I.done = false;
    S2AConc &Q = S.conc;
    hipFree(Q.d_lo); hipFree(Q.d_base); hipFree(Q.d_wlen); hipFree(Q.d_acc); hipFree(Q.d_idx);
    hipFree(Q.d_cnt); hipFree(Q.d_n); hipFree(Q.d_orient); hipFree(Q.d_rd);
    Q.d_lo = Q.d_base = nullptr;
    Q.d_wlen = Q.d_acc = Q.d_idx = Q.d_cnt = Q.d_n = nullptr;
    Q.d_orient = nullptr;
    Q.d_rd = nullptr;
    Q.done = false;
    S2AStrand &T = S.strand;
    hipFree(T.d_lo); hipFree(T.d_base); hipFree(T.d_wlen); hipFree(T.d_acc); hipFree(T.d_idx);
    hipFree(T.d_cnt); hipFree(T.d_n); hipFree(T.d_orient);
    T.d_lo = T.d_base = nullptr;
    T.d_wlen = T.d_acc = T.d_idx = T.d_cnt = T.d_n = nullptr;
    T.d_orient = nullptr;
    T.done = false;
    S.dcap.clear();
}

void s2a_free(Ctx &c)
{
    if (!c.s2a) return;
    s2a_free_device(*c.s2a);
    delete c.s2a;
    c.s2a = nullptr;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
struct S2AArgs {
    const uint8_t *seq, *qual;
    const int64_t *soff;
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int64_t *units;     // per merge unit: row1, row2 (-1: single)
    const int32_t *uref;
    const int64_t *slot;      // byte offset of each entry's output slot in out
    int64_t n;
    int n_cut;                // merge entry e = unit * n_cut + k
    unsigned char cut[S2A_MAX_CUTS];   // q_cutoff + 33 of cutoff k
    double max_prop_n;
    int span_cap, ops_cap, wave_bytes;
    uint8_t *out;
    int32_t *res;             // 4 per entry
    uint64_t *h;              // 2 per entry
    int32_t *ctr;             // [0] error
};

__device__ __forceinline__ int s2a_scan(int v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct Mate {
    int row, pad, rf, len;   // len = pad + reference span
    char *c, *q;             // LDS: c[t], q[t] for t < rf
};

// merge_pairs (sam2aln.py:186-230) at padded position i, for every cutoff at
// once; seq1 = a, seq2 = b (the longer padded read); single = no mate.  The
// merged character is thr > cut ? ch : 'N' for every cut, with (ch, thr)
// fixed for the pair (q and cut compared as bytes, cut = q_cutoff + 33):
//   - cutoff-independent characters ('-', 'n', the 'N' of a quality tie, an
//     unpaired read) get thr = S2A_ALWAYS, above every cut (cut <= 93 + 33);
//   - mates agree:  q1 > cut || q2 > cut          ==  max(q1, q2) > cut;
//   - mates disagree by >= 5:  q1 > max(q2, cut) ? c1 : q2 > max(q1, cut) ? c2 : 'N'.
//     With q1 > q2 the second test is false, so it is q1 > cut ? c1 : 'N';
//     with q2 > q1 the first is false, so it is q2 > cut ? c2 : 'N';
//   - past the shorter mate: q2 > cut ? c2 : 'N'.
constexpr unsigned char S2A_ALWAYS = 255;

__device__ __forceinline__ void s2a_pos(int i, const Mate &a, const Mate &b, bool single,
                                        int rev_start, char &ch, unsigned char &thr)
{
    char c2 = '-';
    unsigned char q2 = '!';
    if (i >= b.pad && i < b.len) { c2 = b.c[i - b.pad]; q2 = (unsigned char)b.q[i - b.pad]; }
    ch = c2;
    thr = S2A_ALWAYS;
    if (single) return;
    if (i < a.len) {
        char c1 = '-';
        unsigned char q1 = '!';
        if (i >= a.pad) { c1 = a.c[i - a.pad]; q1 = (unsigned char)a.q[i - a.pad]; }
        if (c1 == c2) {
            if (c1 != '-') thr = q1 > q2 ? q1 : q2;
            return;
        }
        const int dq = (int)q2 - (int)q1;
        if (dq >= 5) { thr = q2; return; }
        if (dq <= -5) { ch = c1; thr = q1; return; }
        ch = 'N';
        return;
    }
    if (c2 == '-') { ch = i >= rev_start ? '-' : 'n'; return; }
    thr = q2;
}

// NC: compile-time bound on A.n_cut (1, 2, 4 or 8), so that the per-cutoff
// accumulators below are registers, never scratch memory.  Everything up to
// and including the forward / reverse start scans runs once per pair; each
// cutoff then costs one compare per position.
//
// offset and stripped length are computed per cutoff (first[k], last[k]),
// not shared.  A '-' that apply_cigar or the padding wrote can never win a
// cutoff-dependent position -- its quality is ' ' or '!', above no cut >= '!'
// -- but the parser admits any byte in the seq column, and a '-' the read
// itself holds comes with the read's own quality: it wins (a gap) at a low
// cutoff and is 'N' at a higher one, which moves first and last.
template <int NC>
__global__ __launch_bounds__(256) void k_s2a_merge(S2AArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    unsigned char *wb = smem + (size_t)wv * A.wave_bytes;
    char *cq = (char *)wb;                                     // c0 q0 c1 q1, span_cap each
    int32_t *opref = (int32_t *)(wb + 4 * (size_t)A.span_cap); // ops_cap + 1 per mate
    int32_t *opread = opref + 2 * (A.ops_cap + 1);
    const int n_cut = NC == 1 ? 1 : A.n_cut;
    unsigned char cut[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) cut[k] = A.cut[k];

    for (int64_t u = (int64_t)blockIdx.x * wpb + wv; u < A.n; u += (int64_t)gridDim.x * wpb) {
        const int64_t rows[2] = {A.units[2 * u], A.units[2 * u + 1]};
        const int nm = rows[1] >= 0 ? 2 : 1;
        // every loop over the mates is unrolled: mt[k] with a run-time k
        // would put the array in scratch memory (80 B per lane, ~5 GB of
        // HBM writes per launch at C2)
        Mate mt[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            mt[k].row = -1; mt[k].pad = 0; mt[k].rf = 0; mt[k].len = 0;
            mt[k].c = cq + 2 * k * A.span_cap;
            mt[k].q = cq + (2 * k + 1) * A.span_cap;
        }
        // ---- apply_cigar (sam2aln.py:84-153): op offsets by a lane-parallel
        // scan, then the read expanded into reference coordinates ----
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nm) break;
            const int64_t r = rows[k];
            const int nc = A.n_cig[r];
            const uint32_t *ops = A.cig + A.cig_off[r];
            int32_t *oref = opref + k * (A.ops_cap + 1), *ord = opread + k * (A.ops_cap + 1);
            int rf0 = 0, rd0 = 0;
            for (int o0 = 0; o0 < nc; o0 += 64) {
                const int o = o0 + lane;
                int dref = 0, dread = 0, isd = 0;
                if (o < nc) {
                    const uint32_t op = ops[o];
                    const int n = (int)(op >> 4), t = (int)(op & 15);
                    if (t == MH_OP_M) { dref = n; dread = n; }
                    else if (t == MH_OP_D) { dref = n; isd = 1; }
                    else dread = n;                      // I, S (checked on the host)
                }
                const int iref = s2a_scan(dref, lane), iread = s2a_scan(dread, lane);
                if (o < nc) {
                    oref[o] = rf0 + iref - dref;
                    ord[o] = isd ? -1 : rd0 + iread - dread;
                }
                rf0 += __shfl(iref, 63, 64);
                rd0 += __shfl(iread, 63, 64);
            }
            if (lane == 0) { oref[nc] = rf0; ord[nc] = rd0; }
            const int p = A.pos[r] - 1;
            mt[k].row = (int)r;
            mt[k].pad = p > 0 ? p : 0;
            mt[k].rf = rf0;
            mt[k].len = mt[k].pad + rf0;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nm) break;
            const int64_t r = rows[k];
            const int32_t *oref = opref + k * (A.ops_cap + 1), *ord = opread + k * (A.ops_cap + 1);
            const uint8_t *s = A.seq + A.soff[r], *q = A.qual + A.soff[r];
            for (int t = lane; t < mt[k].rf; t += 64) {
                int o = 0;
                while (oref[o + 1] <= t) ++o;
                const int rd = ord[o];
                char c = '-', qq = ' ';
                if (rd >= 0) {
                    const int x = rd + (t - oref[o]);
                    c = (char)s[x];
                    qq = (char)q[x];
                }
                mt[k].c[t] = c;
                mt[k].q[t] = qq;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        // ---- merge_pairs roles: seq1 = row1 unless it is longer ----
        const bool single = nm == 1;
        Mate a = mt[0], b = mt[0];
        if (!single) {
            if (mt[0].len > mt[1].len) { a = mt[1]; b = mt[0]; }
            else { a = mt[0]; b = mt[1]; }
        }
        const int len2 = b.len;
        // is_reverse_started: first i with seq2[i] != '-'; is_forward_started:
        // first i < len(seq1) where not both are '-'
        int rev_start = 1 << 30, fwd_start = 1 << 30;
        if (!single) {
            for (int i0 = 0; i0 < len2; i0 += 64) {
                const int i = i0 + lane;
                int rs = 1 << 30, fs = 1 << 30;
                if (i < len2) {
                    const char c2 = (i >= b.pad) ? b.c[i - b.pad] : '-';
                    if (c2 != '-') rs = i;
                    if (i < a.len) {
                        const char c1 = (i >= a.pad) ? a.c[i - a.pad] : '-';
                        if (!(c1 == '-' && c2 == '-')) fs = i;
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    rs = min(rs, __shfl_xor(rs, o, 64));
                    fs = min(fs, __shfl_xor(fs, o, 64));
                }
                rev_start = min(rev_start, rs);
                fwd_start = min(fwd_start, fs);
                if (rev_start < (1 << 30) && (fwd_start < (1 << 30) || i0 + 64 >= a.len)) break;
            }
        }
        const bool fwd = single || fwd_start < a.len;
        // mseq[j] = merged char at i = j + i0 (the forward read never
        // starting drops positions < len(seq1), sam2aln.py:191-195)
        const int ibase = fwd ? 0 : a.len;
        const int mlen = len2 - ibase;
        // ---- per cutoff: offset (leading '-'), last non-'-', count of 'N' ----
        int first[NC], last[NC], nN[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { first[k] = 1 << 30; last[k] = -1; nN[k] = 0; }
        for (int j0 = 0; j0 < mlen; j0 += 64) {
            const int j = j0 + lane;
            if (j < mlen) {
                const int i = j + ibase;
                char ch = '-';
                unsigned char thr = S2A_ALWAYS;
                if (single || !fwd || i >= fwd_start) s2a_pos(i, a, b, single, rev_start, ch, thr);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const char m = thr > cut[k] ? ch : 'N';
                    if (m != '-') { first[k] = min(first[k], j); last[k] = max(last[k], j); }
                    nN[k] += m == 'N';
                }
            }
        }
        int status[NC], off[NC], blen[NC];
        uint64_t h1[NC], h2[NC];
        int lo = 1 << 30;           // smallest offset of the cutoffs that passed
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            for (int o = 32; o > 0; o >>= 1) {
                first[k] = min(first[k], __shfl_xor(first[k], o, 64));
                last[k] = max(last[k], __shfl_xor(last[k], o, 64));
                nN[k] += __shfl_xor(nN[k], o, 64);
            }
            status[k] = S2A_OK;
            if (last[k] < 0) {
                status[k] = S2A_EMPTY;   // len(mseq.strip('-')) == 0: ZeroDivisionError in the reference
            } else {
                const double prop = (double)nN[k] / (double)(last[k] - first[k] + 1);
                if (prop > A.max_prop_n) status[k] = S2A_MANYNS;
            }
            off[k] = status[k] == S2A_EMPTY ? 0 : first[k];
            blen[k] = status[k] == S2A_EMPTY ? 0 : mlen - first[k];
            h1[k] = h2[k] = 0;
            if (k < n_cut && status[k] == S2A_OK) lo = min(lo, off[k]);
        }
        // ---- the bodies of the cutoffs that passed, each into its entry's
        // slot, and their hashes: (ch, thr) once per position ----
        const int64_t e0 = u * n_cut;
        int64_t slot[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) slot[k] = k < n_cut ? A.slot[e0 + k] : 0;
        for (int j0 = lo; j0 < mlen; j0 += 64) {
            const int j = j0 + lane;
            if (j < mlen) {
                const int i = j + ibase;
                char ch = '-';
                unsigned char thr = S2A_ALWAYS;
                if (single || !fwd || i >= fwd_start) s2a_pos(i, a, b, single, rev_start, ch, thr);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    if (k < n_cut && status[k] == S2A_OK && j >= off[k]) {
                        const char m = thr > cut[k] ? ch : 'N';
                        const int jj = j - off[k];
                        A.out[slot[k] + jj] = (uint8_t)m;
                        const uint64_t k1 = mix64(2ull * (uint64_t)jj + 1ull) | 1ull;
                        const uint64_t k2 = mix64((uint64_t)jj ^ 0x5bd1e995ull << 32) | 1ull;
                        h1[k] += k1 * (uint64_t)(uint8_t)m;
                        h2[k] += k2 * (uint64_t)(uint8_t)m;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= n_cut) break;
            if (status[k] == S2A_OK) {
                for (int o = 32; o > 0; o >>= 1) {
                    h1[k] += __shfl_xor(h1[k], o, 64);
                    h2[k] += __shfl_xor(h2[k], o, 64);
                }
                // the group of a sequence is (rname, cutoff): equal bodies at
                // two cutoffs are two rows of aligned.csv
                const uint64_t grp = (uint64_t)(uint32_t)A.uref[u] * (uint64_t)n_cut + (uint64_t)k;
                const uint64_t meta = (grp << 40) ^ ((uint64_t)(uint32_t)off[k] << 20) ^
                                      (uint64_t)(uint32_t)blen[k];
                h1[k] = mix64(h1[k] ^ mix64(meta));
                h2[k] = mix64(h2[k] + 0x2545f4914f6cdd1dull * mix64(meta + 7));
            }
            if (lane == 0) {
                const int64_t e = e0 + k;
                A.res[4 * e] = status[k];
                A.res[4 * e + 1] = off[k];
                A.res[4 * e + 2] = blen[k];
                A.res[4 * e + 3] = last[k] < 0 ? 0 : last[k] - first[k] + 1;
                A.h[2 * e] = h1[k];
                A.h[2 * e + 1] = h2[k];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the grouping key of a hash: the hash itself (never 0) in the product; a
// test narrows it to key_bits < 64 bits (mh_test_set_sam2aln), shifted and
// made odd as k_a2c_var_hash does, so that distinct sequences share keys
__device__ __forceinline__ uint64_t s2a_key(uint64_t h1, int key_bits = 64)
{
    if (key_bits >= 64) return h1 ? h1 : 1ull;
    return ((h1 & ((1ull << key_bits) - 1)) << 1) | 1ull;
}

__global__ __launch_bounds__(256) void k_s2a_count(const int32_t *res, const uint64_t *h, int64_t n,
                                                   uint64_t *tkey, int32_t *tcnt, int32_t *trep,
                                                   uint64_t mask, int key_bits)
{
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n;
         u += (int64_t)gridDim.x * blockDim.x) {
        if (res[4 * u] != S2A_OK) continue;
        const uint64_t key = s2a_key(h[2 * u], key_bits);
        const uint64_t s = table_claim(tkey, mask, key & mask, key).slot;
        atomicAdd(&tcnt[s], 1);
        atomicMin(&trep[s], (int32_t)u);
    }
}

__global__ __launch_bounds__(256) void k_s2a_verify(const int32_t *res, const uint64_t *h,
                                                    const int32_t *uref, const int64_t *slot,
                                                    const uint8_t *out, int64_t n, int n_cut,
                                                    const uint64_t *tkey, const int32_t *trep,
                                                    uint64_t mask, int32_t *ctr, int key_bits)
{
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    for (int64_t u = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); u < n;
         u += (int64_t)gridDim.x * wpb) {
        if (res[4 * u] != S2A_OK) continue;
        const uint64_t key = s2a_key(h[2 * u], key_bits);
        const int64_t r = trep[table_find(tkey, mask, key & mask, key)];
        if (r == u) continue;
        // same group: same rname and same cutoff (entry = unit * n_cut + k)
        bool bad = h[2 * r + 1] != h[2 * u + 1] || uref[r / n_cut] != uref[u / n_cut] ||
                   r % n_cut != u % n_cut ||
                   res[4 * r + 1] != res[4 * u + 1] || res[4 * r + 2] != res[4 * u + 2];
        if (!bad) {
            const uint8_t *x = out + slot[u], *y = out + slot[r];
            int diff = 0;
            for (int j = lane; j < res[4 * u + 2]; j += 64) diff |= x[j] != y[j];
            bad = __any(diff);
        }
        if (bad && lane == 0) atomicExch(&ctr[0], 1);
    }
}

__global__ __launch_bounds__(256) void k_s2a_compact(const uint64_t *tkey, const int32_t *tcnt,
                                                     const int32_t *trep, uint64_t size,
                                                     int32_t *uniq, int32_t *ctr)
{
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < size;
         s += (uint64_t)gridDim.x * blockDim.x) {
        if (!tkey[s]) continue;
        const int idx = atomicAdd(&ctr[1], 1);
        uniq[2 * idx] = trep[s];
        uniq[2 * idx + 1] = tcnt[s];
    }
}

__global__ __launch_bounds__(256) void k_s2a_gather(const int32_t *uniq, const int64_t *goff,
                                                    const int32_t *res, const int64_t *slot,
                                                    const uint8_t *out, int64_t n_uniq,
                                                    uint8_t *dst)
{
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    for (int64_t k = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); k < n_uniq;
         k += (int64_t)gridDim.x * wpb) {
        const int64_t r = uniq[2 * k];
        const int bl = res[4 * r + 2];
        const uint8_t *src = out + slot[r];
        for (int j = lane; j < bl; j += 64) dst[goff[k] + j] = src[j];
    }
}

// ---------------------------------------------------------------------------
// k_s2a_stage: the resident reads and records as the rows of remap.csv.
// For read r the SEQ and QUAL bytes format_row prints (ACGTN, reversed and
// complemented on the reverse strand of a mapped read) go to seq / qual at
// the read's own padded offset R.off[r] (a multiple of 32, so S2AArgs.soff
// is R.off and every 16-byte store is aligned); POS, the CIGAR's place in the
// mapping pass's pool, FLAG and RNAME's index go to the row arrays, and the
// reference span (M + D), the strand and "has an I op" to span_ins for the
// host's slots.
//
// 16 lanes per read, one 16-base chunk per lane and step: a chunk is one
// 2-bit word, half an N-mask word and 16 quality bytes in, two 16-byte
// stores out, and the 16 lanes of a read write 256 consecutive bytes.  A
// reversed chunk reads its 16 source bases backwards from the read's end
// (an unaligned window over two words, shifted into place) and writes
// forwards like any other.
// ---------------------------------------------------------------------------
struct StageArgs {
    DevReads R;
    const Rec *rec;
    const uint32_t *pool;
    uint8_t *seq, *qual;
    int32_t *pos, *cig_off, *n_cig, *flag, *sam_ref, *span_ins;
};

// 16 2-bit codes (base i at bits 2i) and their N bits -> 16 ASCII bytes
__device__ __forceinline__ uint4 s2a_ascii16(uint32_t codes, uint32_t nm)
{
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = 4 * k + b;
            uint32_t ch = (0x54474341u >> (8 * ((codes >> (2 * i)) & 3u))) & 0xffu;   // "ACGT"
            if ((nm >> i) & 1u) ch = 'N';
            v |= ch << (8 * b);
        }
        w[k] = v;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bytes s .. s + 7 of the 16 bytes (x, y), s in 0..7
__device__ __forceinline__ uint64_t s2a_funnel(uint64_t x, uint64_t y, int s)
{
    return s ? (x >> (8 * s)) | (y << (64 - 8 * s)) : x;
}

__global__ __launch_bounds__(256) void k_s2a_stage(StageArgs A)
{
    const int sub = threadIdx.x & 15;
    const int64_t ngrp = (int64_t)gridDim.x * 16;
    for (int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < A.R.n; r += ngrp) {
        const Rec *a = A.rec + r;
        const int ref = a->ref, ncg = ref >= 0 ? a->n_cigar : 0, coff = a->cig_off;
        const bool rev = ref >= 0 && a->rev;
        const int L = A.R.len[r];
        const int64_t off = A.R.off[r];
        // ---- reference span and insertion flag: the read's ops over its lanes ----
        int span = 0, ins = 0;
        for (int o = sub; o < ncg; o += 16) {
            const uint32_t op = A.pool[coff + o];
            const int t = (int)(op & 15);
            if (t == MH_OP_M || t == MH_OP_D) span += (int)(op >> 4);
            ins |= t == MH_OP_I;
        }
        for (int o = 8; o > 0; o >>= 1) {
            span += __shfl_xor(span, o, 16);
            ins |= __shfl_xor(ins, o, 16);
        }
        if (sub == 0) {
            A.pos[r] = a->sam_pos;
            A.cig_off[r] = coff;
            A.n_cig[r] = ncg;
            A.flag[r] = a->flag;
            A.sam_ref[r] = a->sam_ref;
            A.span_ins[r] = ref >= 0 ? (span << 2 | (rev ? 2 : 0) | ins) : -1;
        }
        // ---- SEQ and QUAL, 16 bases per lane ----
        const uint32_t *w2 = A.R.seq2 + (off >> 4), *wn = A.R.nmask + (off >> 5);
        const uint8_t *q = A.R.qual + off;
        const int nch = (L + 15) >> 4;
        for (int j = sub; j < nch; j += 16) {
            uint32_t codes, nm;
            uint4 qv;
            if (!rev) {
                codes = w2[j];
                nm = (wn[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                qv = *(const uint4 *)(q + 16 * j);
            } else {
                // output bases 16j .. 16j+15 are source bases lo+15 .. lo, lo >= -15
                const int lo = L - 16 - 16 * j;
                const int qw = (lo + 16) >> 4, sh = lo & 15;
                const uint32_t cl = qw >= 1 ? w2[qw - 1] : 0u, chh = w2[qw];
                uint32_t x = (uint32_t)((((uint64_t)chh << 32) | cl) >> (2 * sh));
                x = __brev(x);                                           // base order reversed,
                x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u); // each code's bits back in order
                codes = ~x;                                              // complement: 3 - code
                const int qn = (lo + 32) >> 5, shn = (lo + 32) & 31;
                const uint32_t ml = qn >= 1 ? wn[qn - 1] : 0u, mh = wn[qn];
                nm = __brev((uint32_t)((((uint64_t)mh << 32) | ml) >> shn) & 0xffffu) >> 16;
                const uint4 z = make_uint4(0, 0, 0, 0);
                const uint4 va = qw >= 1 ? *(const uint4 *)(q + 16 * (qw - 1)) : z;
                const uint4 vb = *(const uint4 *)(q + 16 * qw);
                const uint64_t a0 = (uint64_t)va.y << 32 | va.x, a1 = (uint64_t)va.w << 32 | va.z;
                const uint64_t b0 = (uint64_t)vb.y << 32 | vb.x, b1 = (uint64_t)vb.w << 32 | vb.z;
                const bool up = sh >= 8;
                const int s8 = sh & 7;
                const uint64_t r0 = s2a_funnel(up ? a1 : a0, up ? b0 : a1, s8);
                const uint64_t r1 = s2a_funnel(up ? b0 : a1, up ? b1 : b0, s8);
                const uint64_t o0 = __builtin_bswap64(r1), o1 = __builtin_bswap64(r0);
                qv = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
            }
            *(uint4 *)(A.seq + off + 16 * j) = s2a_ascii16(codes, nm);
            *(uint4 *)(A.qual + off + 16 * j) = qv;
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// a device buffer of at least `bytes` behind p: kept between calls and
// reallocated only to grow (a hipFree waits for the device, and large
// allocations map pages: both once per size, not once per call)
template <class T>
static int dev_reserve(S2AState &S, T *&p, size_t bytes)
{
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
static int s2a_upload(S2AState &S, T *&dst, const std::vector<T> &v, hipStream_t s)
{
    if (int st = dev_reserve(S, dst, sizeof(T) * v.size())) return st;
    if (!v.empty()) MH_HIP(hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s));
    return 0;
}

template <class Bytes>
static int s2a_upload_bytes(S2AState &S, uint8_t *&dst, const Bytes &v, hipStream_t s)
{
    if (int st = dev_reserve(S, dst, v.size())) return st;
    if (!v.empty()) MH_HIP(hipMemcpyAsync(dst, v.data(), v.size(), hipMemcpyHostToDevice, s));
    return 0;
}

// apply_cigar's checks on one row (sam2aln.py:113-151): the regex, the
// supported ops and the read length; the reference raises RuntimeError.
int s2a_run(Ctx &c, S2AState &S, double max_prop_n, const S2ADevRows *dev)
{
    hipStream_t s = c.stream;
    const int64_t nu = (int64_t)S.u1.size();
    std::vector<int64_t> mu;      // row pairs of merged units
    std::vector<int32_t> mref;
    std::vector<int64_t> slot;    // one per entry
    const int nc = (int)S.q_cutoffs.size();
    int64_t total = 0;
    int span_cap = 1, ops_cap = 1;
    for (int64_t u = 0; u < nu; ++u) {
        if (S.ucause[u] >= 0) continue;
        const int64_t r1 = S.u1[u], r2 = S.upaired[u] ? S.u2[u] : -1;
        S.merge_of_unit[u] = (int64_t)mref.size();
        mu.push_back(r1);
        mu.push_back(r2);
        mref.push_back(S.name_id[u]);
        // slot: at most max(len) - min(pad) merged characters
        int hi = 0, lo = 1 << 30;
        for (int64_t r : {r1, r2}) {
            if (r < 0) continue;
            int rf = dev ? dev->span[r] >> 2 : 0;
            for (int o = 0; !dev && o < S.n_cig[r]; ++o) {
                const uint32_t op = S.cig[S.cig_off[r] + o];
                if ((op & 15) == MH_OP_M || (op & 15) == MH_OP_D) rf += (int)(op >> 4);
            }
            const int pad = S.pos[r] - 1 > 0 ? S.pos[r] - 1 : 0;
            hi = std::max(hi, pad + rf);
            lo = std::min(lo, pad);
            span_cap = std::max(span_cap, rf);
            ops_cap = std::max(ops_cap, S.n_cig[r]);
        }
        for (int k = 0; k < nc; ++k) {
            slot.push_back(total);
            total += std::max(0, hi - lo);
        }
    }
    S.n_merge = (int64_t)mref.size();
    S.n_unique = 0;
    S.res.clear();
    S.uniq.clear();
    S.uniq_off.clear();
    S.gathered.clear();
    if (S.n_merge == 0) {
        S.clip.state = CLIP_ROWS;    // no unit to count: clipping.csv is its header
        return 0;
    }
    if (S.n_merge * nc > 0x7f7f7f7f) {   // entries are int32 in the table and in uniq
        set_error("sam2aln: %lld pairs at %d q-cutoffs are too many merge entries",
                  (long long)S.n_merge, nc);
        return -3;
    }
    span_cap = (span_cap + 15) & ~15;
    const int wave_bytes = ((S2A_SPAN_BYTES * span_cap + S2A_OP_BYTES * (ops_cap + 1)) + 15) & ~15;
    int wpb = S2A_WPB;
    while (wpb > 1 && (size_t)wpb * wave_bytes > S2A_LDS_BYTES) --wpb;
    S.info = S2AState::Info();
    S.info.span_cap = span_cap;
    S.info.ops_cap = ops_cap;
    S.info.wave_bytes = wave_bytes;
    S.info.n_merge = S.n_merge;
    S.info.n_cut = nc;
    if ((size_t)wave_bytes > S2A_LDS_BYTES) {
        set_error("sam2aln: reference span %d too long for LDS", span_cap);
        return -3;
    }
    if (!dev) {
        S.staged_reads = -1;     // d_seq / d_qual hold the file's rows from here on
        if (int st = s2a_upload_bytes(S, S.d_seq, S.seq, s)) return st;
        if (int st = s2a_upload_bytes(S, S.d_qual, S.qual, s)) return st;
        if (int st = s2a_upload(S, S.d_soff, S.soff, s)) return st;
        if (int st = s2a_upload(S, S.d_pos, S.pos, s)) return st;
        if (int st = s2a_upload(S, S.d_cigoff, S.cig_off, s)) return st;
        if (int st = s2a_upload(S, S.d_ncig, S.n_cig, s)) return st;
        if (int st = s2a_upload(S, S.d_cig, S.cig, s)) return st;
    }
    if (int st = s2a_upload(S, S.d_units, mu, s)) return st;
    if (int st = s2a_upload(S, S.d_uref, mref, s)) return st;
    if (int st = s2a_upload(S, S.d_slot, slot, s)) return st;
    const int64_t nm = S.n_merge, ne = nm * nc;   // pairs, entries
    uint64_t tsize = S2A_MIN_TABLE;
    while (tsize < (uint64_t)(2 * ne)) tsize <<= 1;
    if (int st = dev_reserve(S, S.d_out, total > 0 ? (size_t)total : 1)) return st;
    if (int st = dev_reserve(S, S.d_res, sizeof(int32_t) * 4 * ne)) return st;
    if (int st = dev_reserve(S, S.d_h, sizeof(uint64_t) * 2 * ne)) return st;
    if (int st = dev_reserve(S, S.d_ctr, sizeof(int32_t) * 4)) return st;
    if (int st = dev_reserve(S, S.d_tkey, sizeof(uint64_t) * tsize)) return st;
    if (int st = dev_reserve(S, S.d_tcnt, sizeof(int32_t) * tsize)) return st;
    if (int st = dev_reserve(S, S.d_trep, sizeof(int32_t) * tsize)) return st;
    if (int st = dev_reserve(S, S.d_uniq, sizeof(int32_t) * 2 * ne)) return st;
    MH_HIP(hipMemsetAsync(S.d_ctr, 0, sizeof(int32_t) * 4, s));
    MH_HIP(hipMemsetAsync(S.d_tkey, 0, sizeof(uint64_t) * tsize, s));
    MH_HIP(hipMemsetAsync(S.d_tcnt, 0, sizeof(int32_t) * tsize, s));
    MH_HIP(hipMemsetAsync(S.d_trep, 0x7f, sizeof(int32_t) * tsize, s));

    S2AArgs a{dev ? dev->seq : S.d_seq, dev ? dev->qual : S.d_qual, dev ? dev->soff : S.d_soff,
              dev ? dev->pos : S.d_pos, dev ? dev->cig_off : S.d_cigoff,
              dev ? dev->n_cig : S.d_ncig, dev ? dev->cig : S.d_cig, S.d_units, S.d_uref,
              S.d_slot, nm, nc, {}, max_prop_n, span_cap, ops_cap,
              wave_bytes, S.d_out, S.d_res, S.d_h, S.d_ctr};
    for (int k = 0; k < nc; ++k) a.cut[k] = (unsigned char)(S.q_cutoffs[k] + 33);
    int64_t blocks = (nm + wpb - 1) / wpb;
    if (blocks > S2A_BLOCK_CAP) blocks = S2A_BLOCK_CAP;
    // mh_test_set_sam2aln: fewer blocks (a wave then takes several units in
    // turn) and a narrowed grouping key; 0 and 64 in the product
    const int64_t max_blocks = c.test_caps.s2a_max_blocks;
    const int key_bits = c.test_caps.s2a_key_bits;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    S.info.wpb = wpb;
    S.info.blocks = blocks;
    S.info.tsize = (int64_t)tsize;
    // the instance whose compile-time bound is the next power of two >= nc
    void (*merge)(S2AArgs) = nc == 1 ? k_s2a_merge<1> : nc == 2 ? k_s2a_merge<2>
                             : nc <= 4 ? k_s2a_merge<4> : k_s2a_merge<8>;
    MH_HIP(hipFuncSetAttribute((const void *)merge,
                               hipFuncAttributeMaxDynamicSharedMemorySize, wpb * wave_bytes));
    const int p0 = prof_begin(c, "k_s2a_merge");
    hipLaunchKernelGGL(merge, dim3((unsigned)blocks), dim3(64 * wpb), wpb * wave_bytes, s, a);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    int64_t tb = (ne + 255) / 256;
    if (tb > 65536) tb = 65536;
    const int p1 = prof_begin(c, "k_s2a_group");
    hipLaunchKernelGGL(k_s2a_count, dim3((unsigned)tb), dim3(256), 0, s, S.d_res, S.d_h, ne,
                       S.d_tkey, S.d_tcnt, S.d_trep, tsize - 1, key_bits);
    int64_t vb = (ne + 3) / 4;
    if (vb > 256 * 64) vb = 256 * 64;
    hipLaunchKernelGGL(k_s2a_verify, dim3((unsigned)vb), dim3(256), 0, s, S.d_res, S.d_h, S.d_uref,
                       S.d_slot, S.d_out, ne, nc, S.d_tkey, S.d_trep, tsize - 1, S.d_ctr, key_bits);
    int64_t cb = (int64_t)((tsize + 255) / 256);
    if (cb > 65536) cb = 65536;
    hipLaunchKernelGGL(k_s2a_compact, dim3((unsigned)cb), dim3(256), 0, s, S.d_tkey, S.d_tcnt,
                       S.d_trep, tsize, S.d_uniq, S.d_ctr);
    prof_end(c, p1);
    MH_HIP(hipGetLastError());
    int32_t ctr[4];
    MH_HIP(hipMemcpyAsync(ctr, S.d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    if (ctr[0]) {
        set_error("sam2aln: merged-sequence hash collision (distinct sequences share a key)");
        return -4;
    }
    S.n_unique = ctr[1];
    S.res.resize(4 * ne);
    S.uniq.resize(2 * (size_t)S.n_unique);
    MH_HIP(hipMemcpyAsync(S.res.data(), S.d_res, sizeof(int32_t) * 4 * ne, hipMemcpyDeviceToHost, s));
    if (S.n_unique)
        MH_HIP(hipMemcpyAsync(S.uniq.data(), S.d_uniq, sizeof(int32_t) * 2 * S.n_unique,
                              hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    for (int64_t e = 0; e < ne; ++e)
        if (S.res[4 * e] == S2A_EMPTY) {
            set_error("sam2aln: merged sequence of unit %lld is all gaps (float division by zero)",
                      (long long)(e / nc));
            return -3;
        }
    // gather the distinct bodies
    S.uniq_off.resize(S.n_unique + 1);
    int64_t g = 0;
    for (int64_t k = 0; k < S.n_unique; ++k) {
        S.uniq_off[k] = g;
        g += S.res[4 * (int64_t)S.uniq[2 * k] + 2];
    }
    S.uniq_off[S.n_unique] = g;
    S.gathered.resize((size_t)g);
    if (S.n_unique && g) {
        if (int st = s2a_upload(S, S.d_goff, S.uniq_off, s)) return st;
        if (int st = dev_reserve(S, S.d_gather, (size_t)g)) return st;
        int64_t gb = (S.n_unique + 3) / 4;
        if (gb > 256 * 64) gb = 256 * 64;
        hipLaunchKernelGGL(k_s2a_gather, dim3((unsigned)gb), dim3(256), 0, s, S.d_uniq, S.d_goff,
                           S.d_res, S.d_slot, S.d_out, S.n_unique, S.d_gather);
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(&S.gathered[0], S.d_gather, (size_t)g, hipMemcpyDeviceToHost, s));
        MH_HIP(hipStreamSynchronize(s));
    }
    prof_flush(c);
    // d_units / d_uref and these rows stand until the next call: s2a_clip_run
    S.clip.rows = dev ? *dev : S2ADevRows{S.d_seq, S.d_qual, S.d_soff, S.d_pos, S.d_cigoff, S.d_ncig,
                                          S.d_cig, nullptr};
    S.clip.state = CLIP_ROWS;
    return 0;
}

// ---------------------------------------------------------------------------
// Soft-clip counts (clipping.csv; DESIGN.md section 6, "Soft-clip counts").
// Per read with 1-based POS p: lead = the S ops before the first other op,
// trail = every other S op, span = M + D; clipped = [p - lead, p) and
// [p + span, p + span + trail), mapped = [p, p + span).  A merged unit adds 1
// at every position some mate clips and no mate aligns.
//
// k_s2a_clip       one thread per unit: the <= 12 interval ends of its mates,
//                  and at each distinct end x the step in(x) - in(x - 1) of
//                  "clipped and not mapped" (+1 where it begins, -1 where it
//                  ends) added to the reference's difference array at
//                  x - lo[ref].  An amplicon puts nearly every unit's steps on
//                  the same few addresses, so a block first sums them in an
//                  LDS table keyed by the array index (CLIP_SLOTS slots,
//                  CLIP_PROBES probes, then straight to HBM) and flushes one
//                  atomic per slot it used.  Integer adds: no order matters.
// k_s2a_clip_scan  one block per reference: the running sum over its window
//                  in chunks of the block's size (wave scans, wave totals in
//                  LDS, a carry between chunks), and the non-zero sums
//                  compacted in position order by a second scan of flags.
// ---------------------------------------------------------------------------
constexpr int CLIP_SLOTS = 1024;    // LDS table of k_s2a_clip (12 KiB a block)
constexpr int CLIP_PROBES = 8;
constexpr int CLIP_UNITS_PER_THREAD = 16;

struct ClipArgs {
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int64_t *units;     // per merge unit: row1, row2 (-1: single)
    const int32_t *uref;
    int64_t n;
    const int64_t *lo, *base; // per reference: first position of its window, its offset in diff
    const int32_t *wlen;      // per reference: positions in its window (diff holds wlen + 1)
    int32_t *diff;
    int32_t *err;             // set when a step falls outside its window
    int lds;                  // 0: every step straight to HBM (measurements)
};

struct ClipUnit {
    int64_t cl[4], ch[4];     // clipped [cl, ch): lead and trail of each mate
    int64_t ml[2], mh[2];     // mapped [ml, mh)
};

__device__ __forceinline__ void clip_read(const ClipArgs &A, int64_t r, ClipUnit &U, int k)
{
    const int nc = A.n_cig[r];
    const uint32_t *ops = A.cig + A.cig_off[r];
    int64_t lead = 0, trail = 0, span = 0;
    bool head = true;
    for (int o = 0; o < nc; ++o) {
        const uint32_t op = ops[o];
        const int64_t n = (int64_t)(op >> 4);
        const int t = (int)(op & 15);
        if (t == MH_OP_S) {
            if (head) lead += n; else trail += n;
        } else {
            head = false;
            if (t == MH_OP_M || t == MH_OP_D) span += n;
        }
    }
    const int64_t p = A.pos[r];
    U.cl[2 * k] = p - lead;       U.ch[2 * k] = p;
    U.cl[2 * k + 1] = p + span;   U.ch[2 * k + 1] = p + span + trail;
    U.ml[k] = p;                  U.mh[k] = p + span;
}

__device__ __forceinline__ int clip_in(const ClipUnit &U, int64_t y)
{
    bool c = false, m = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) c |= y >= U.cl[k] && y < U.ch[k];
#pragma unroll
    for (int k = 0; k < 2; ++k) m |= y >= U.ml[k] && y < U.mh[k];
    return c && !m;
}

__device__ __forceinline__ void clip_add(const ClipArgs &A, unsigned long long *tkey, int32_t *tval,
                                         int ref, int64_t x, int d)
{
    const int64_t idx = x - A.lo[ref];
    if (idx < 0 || idx > (int64_t)A.wlen[ref]) {   // the host sized the window from the same rows
        atomicExch(A.err, 1);
        return;
    }
    const int64_t g = A.base[ref] + idx;
    if (A.lds) {
        const unsigned long long key = (unsigned long long)g + 1ull;
        unsigned s = (unsigned)hash_key(key) & (CLIP_SLOTS - 1);
        for (int t = 0; t < CLIP_PROBES; ++t, s = (s + 1) & (CLIP_SLOTS - 1)) {
            const unsigned long long old = atomicCAS(&tkey[s], 0ull, key);
            if (old == 0ull || old == key) {
                atomicAdd(&tval[s], d);
                return;
            }
        }
    }
    atomicAdd(&A.diff[g], d);
}

__global__ __launch_bounds__(256) void k_s2a_clip(ClipArgs A)
{
    __shared__ unsigned long long tkey[CLIP_SLOTS];
    __shared__ int32_t tval[CLIP_SLOTS];
    for (int s = threadIdx.x; s < CLIP_SLOTS; s += blockDim.x) { tkey[s] = 0ull; tval[s] = 0; }
    __syncthreads();
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < A.n;
         u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r1 = A.units[2 * u], r2 = A.units[2 * u + 1];
        ClipUnit U;
        clip_read(A, r1, U, 0);
        if (r2 >= 0) {
            clip_read(A, r2, U, 1);
        } else {
            U.cl[2] = U.ch[2] = U.cl[3] = U.ch[3] = U.ml[1] = U.mh[1] = 0;   // empty
        }
        const int ref = A.uref[u];
        // every index below is a constant once unrolled: e[] stays in registers
        int64_t e[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) { e[k] = U.cl[k]; e[4 + k] = U.ch[k]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) { e[8 + k] = U.ml[k]; e[10 + k] = U.mh[k]; }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            bool dup = false;
#pragma unroll
            for (int j = 0; j < i; ++j) dup |= e[j] == e[i];
            const int d = clip_in(U, e[i]) - clip_in(U, e[i] - 1);
            if (!dup && d) clip_add(A, tkey, tval, ref, e[i], d);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CLIP_SLOTS; s += blockDim.x)
        if (tkey[s] && tval[s]) atomicAdd(&A.diff[tkey[s] - 1ull], tval[s]);
}

__global__ __launch_bounds__(1024) void k_s2a_clip_scan(const int64_t *base, const int32_t *wlen,
                                                        int32_t *diff, int32_t *idx_out,
                                                        int32_t *cnt_out, int32_t *n_out)
{
    __shared__ int32_t wsum[16], wnz[16];
    const int ref = blockIdx.x;
    const int64_t b = base[ref];
    const int n = wlen[ref] + 1;           // 0 for a reference without units (wlen -1)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int carry = 0, outn = 0;
    for (int i0 = 0; i0 < n; i0 += blockDim.x) {
        const int i = i0 + (int)threadIdx.x;
        const int v = i < n ? diff[b + i] : 0;
        const int s = s2a_scan(v, lane);
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < nw; ++w) { const int t = wsum[w]; pre += w < wv ? t : 0; tot += t; }
        const int cov = carry + pre + s;
        const int nz = i < n && cov != 0;
        const int f = s2a_scan(nz, lane);
        if (lane == 63) wnz[wv] = f;
        __syncthreads();
        int pre2 = 0, tot2 = 0;
        for (int w = 0; w < nw; ++w) { const int t = wnz[w]; pre2 += w < wv ? t : 0; tot2 += t; }
        if (i < n) diff[b + i] = cov;
        if (nz) {
            const int k = outn + pre2 + f - 1;     // < n: one pair per position at most
            idx_out[b + k] = i;
            cnt_out[b + k] = cov;
        }
        carry += tot;
        outn += tot2;
        __syncthreads();                   // wsum / wnz are rewritten by the next chunk
    }
    if (threadIdx.x == 0) n_out[ref] = outn;
}

int s2a_clip_run(Ctx &c, S2AState &S)
{
    S2AClip &K = S.clip;
    if (K.state == CLIP_DONE) return 0;
    if (K.state != CLIP_ROWS) {
        set_error("sam2aln clipping: no rows of a sam2aln call are on the device");
        return -3;
    }
    // the resident rows' CIGARs are the mapping pass's pool itself
    if (S.n_merge && K.rows.cig != S.d_cig && (!c.map.valid || K.rows.cig != c.map.pool)) {
        set_error("sam2aln clipping: the mapping pass the rows came from is gone");
        return -3;
    }
    K.name.clear(); K.pos.clear(); K.count.clear();
    K.text_valid = false;
    const int nref = (int)S.names.size();
    const int64_t nu = (int64_t)S.u1.size();
    // ---- each reference's window from its units' rows: POS - lead .. POS + span + trail ----
    std::vector<int64_t> lo((size_t)nref, INT64_MAX), hi((size_t)nref, INT64_MIN);
    for (int64_t u = 0; u < nu; ++u) {
        if (S.ucause[u] >= 0) continue;
        const int g = S.name_id[u];
        for (int64_t r : {S.u1[u], S.upaired[u] ? S.u2[u] : (int64_t)-1}) {
            if (r < 0) continue;
            int64_t lead = 0, rest = 0;
            bool head = true;
            for (int o = 0; o < S.n_cig[r]; ++o) {
                const uint32_t op = S.cig[S.cig_off[r] + o];
                const int t = (int)(op & 15);
                if (t == MH_OP_S && head) { lead += op >> 4; continue; }
                head = false;
                if (t == MH_OP_S || t == MH_OP_M || t == MH_OP_D) rest += op >> 4;
            }
            lo[g] = std::min(lo[g], (int64_t)S.pos[r] - lead);
            hi[g] = std::max(hi[g], (int64_t)S.pos[r] + rest);
        }
    }
    std::vector<int64_t> base((size_t)nref + 1, 0);
    std::vector<int32_t> wlen((size_t)nref, -1);
    for (int g = 0; g < nref; ++g) {
        if (lo[g] > hi[g]) { lo[g] = 0; base[g + 1] = base[g]; continue; }
        if (hi[g] - lo[g] > S2A_CLIP_MAX_WINDOW) {
            set_error("sam2aln clipping: the rows of %s span positions %lld to %lld, more than %lld",
                      S.names[g].c_str(), (long long)lo[g], (long long)hi[g],
                      (long long)S2A_CLIP_MAX_WINDOW);
            return -3;
        }
        wlen[g] = (int32_t)(hi[g] - lo[g]);
        base[g + 1] = base[g] + wlen[g] + 1;
    }
    const int64_t total = base[nref];
    if (S.n_merge == 0 || total == 0) { K.state = CLIP_DONE; return 0; }
    hipStream_t s = c.stream;
    if (int st = s2a_upload(S, K.d_lo, lo, s)) return st;
    if (int st = s2a_upload(S, K.d_base, base, s)) return st;
    if (int st = s2a_upload(S, K.d_wlen, wlen, s)) return st;
    if (int st = dev_reserve(S, K.d_diff, sizeof(int32_t) * (size_t)total)) return st;
    if (int st = dev_reserve(S, K.d_idx, sizeof(int32_t) * (size_t)total)) return st;
    if (int st = dev_reserve(S, K.d_cnt, sizeof(int32_t) * (size_t)total)) return st;
    if (int st = dev_reserve(S, K.d_n, sizeof(int32_t) * ((size_t)nref + 1))) return st;
    MH_HIP(hipMemsetAsync(K.d_diff, 0, sizeof(int32_t) * (size_t)total, s));
    MH_HIP(hipMemsetAsync(K.d_n, 0, sizeof(int32_t) * ((size_t)nref + 1), s));
    static const bool lds = !(getenv("MICALL_CLIP_LDS") && *getenv("MICALL_CLIP_LDS") == '0');
    ClipArgs a{K.rows.pos, K.rows.cig_off, K.rows.n_cig, K.rows.cig, S.d_units, S.d_uref, S.n_merge,
               K.d_lo, K.d_base, K.d_wlen, K.d_diff, K.d_n + nref, lds ? 1 : 0};
    int64_t blocks = (S.n_merge + 256 * CLIP_UNITS_PER_THREAD - 1) / (256 * CLIP_UNITS_PER_THREAD);
    if (blocks > 4096) blocks = 4096;
    const int p0 = prof_begin(c, "k_s2a_clip");
    hipLaunchKernelGGL(k_s2a_clip, dim3((unsigned)blocks), dim3(256), 0, s, a);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    const int p1 = prof_begin(c, "k_s2a_clip_scan");
    hipLaunchKernelGGL(k_s2a_clip_scan, dim3((unsigned)nref), dim3(1024), 0, s, K.d_base, K.d_wlen,
                       K.d_diff, K.d_idx, K.d_cnt, K.d_n);
    prof_end(c, p1);
    MH_HIP(hipGetLastError());
    std::vector<int32_t> n_out((size_t)nref + 1);
    MH_HIP(hipMemcpyAsync(n_out.data(), K.d_n, sizeof(int32_t) * n_out.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    if (n_out[nref]) {
        set_error("sam2aln clipping: a clipped position fell outside its reference's window");
        return -4;
    }
    // ---- the pairs of each reference, references as Python sorts str ----
    std::vector<int> order((size_t)nref);
    for (int g = 0; g < nref; ++g) order[g] = g;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return S.names[x] < S.names[y]; });
    std::vector<int64_t> at((size_t)nref + 1, 0);
    for (int k = 0; k < nref; ++k) {
        const int g = order[k];
        if (n_out[g] < 0 || n_out[g] > wlen[g] + 1) {
            set_error("sam2aln clipping: %d positions counted in a window of %d", n_out[g], wlen[g] + 1);
            return -4;
        }
        at[k + 1] = at[k] + n_out[g];
    }
    std::vector<int32_t> idx((size_t)at[nref]);
    K.count.resize((size_t)at[nref]);
    for (int k = 0; k < nref; ++k) {
        const int g = order[k];
        if (!n_out[g]) continue;
        const size_t nb = sizeof(int32_t) * (size_t)n_out[g];
        MH_HIP(hipMemcpyAsync(idx.data() + at[k], K.d_idx + base[g], nb, hipMemcpyDeviceToHost, s));
        MH_HIP(hipMemcpyAsync(K.count.data() + at[k], K.d_cnt + base[g], nb, hipMemcpyDeviceToHost, s));
    }
    MH_HIP(hipStreamSynchronize(s));
    K.name.resize(idx.size());
    K.pos.resize(idx.size());
    for (int k = 0; k < nref; ++k)
        for (int64_t j = at[k]; j < at[k + 1]; ++j) {
            K.name[j] = order[k];
            K.pos[j] = lo[order[k]] + idx[j];
        }
    K.state = CLIP_DONE;
    return 0;
}

// clipping.csv of S.clip's lists: refname,pos,count
static void s2a_clip_text(S2AState &S)
{
    S2AClip &K = S.clip;
    if (K.text_valid) return;
    std::string &o = K.text;
    o.assign("refname,pos,count\n");
    for (size_t j = 0; j < K.name.size(); ++j) {
        const std::string &rn = S.names[K.name[j]];
        csv_field(o, rn.data(), rn.size());
        o.push_back(',');
        o += std::to_string((long long)K.pos[j]);
        o.push_back(',');
        o += std::to_string(K.count[j]);
        o.push_back('\n');
    }
    K.text_valid = true;
}

// the counts of the context's last sam2aln call, counted now if not yet
static int s2a_clip_of(mh_ctx *ctx, const char *what, bool text, S2AState **out)
{
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("%s: no sam2aln results", what); return -3; }
    MH_HIP(hipSetDevice(c.device));
    try {
        if (int st = s2a_clip_run(c, *c.s2a)) return st;
        if (text) s2a_clip_text(*c.s2a);
    } catch (const std::exception &e) {
        c.s2a->clip.text_valid = false;
        set_error("%s: out of memory (%s)", what, e.what());
        return -2;
    }
    *out = c.s2a;
    return 0;
}

// ---------------------------------------------------------------------------
// Mate concordance (concordance.csv, cycle_concordance.csv; DESIGN.md section
// 6, "Mate concordance").  A paired unit that reaches the merge is expanded as
// apply_cigar expands it; at every position y both mates map (M or D) it adds
// 1 to overlap and, when the mates' bytes differ, 1 to one of mismatch, indel,
// nocall, and 1 to unresolved when their qualities are closer than 5.  Where
// both mates hold a read base other than 'N', each adds 1 to compared (and to
// mismatch when the bytes differ) at its (read, cycle) and (read, quality).
//
// k_s2a_conc       one wave per unit: the op offsets of both mates by the
//                  merge's lane-parallel scan (in LDS), then the intersection
//                  of the two mapped intervals 64 positions at a time, each
//                  lane looking both mates' bytes up in seq / qual.  overlap is
//                  two steps into the reference's difference array (plane 0);
//                  the four sparse classes are planes 1..4 of the same array.
//                  Steps and classes go through the block's LDS table (keyed
//                  by plane and index, CONC_SLOTS slots, CONC_PROBES probes,
//                  then straight to HBM) and are flushed with one atomic per
//                  used slot.  The per-read table is dense in LDS (32-bit)
//                  while a read's slots fit in CONC_READ_LDS, and flushed once
//                  per block with 64-bit adds; a longer read's adds go
//                  straight to the 64-bit table in HBM.  Integer adds only.
// k_s2a_conc_scan  one block per reference: the running sum of plane 0 as
//                  k_s2a_clip_scan runs it, and the positions with overlap > 0
//                  compacted in position order with their five counts.
// ---------------------------------------------------------------------------
constexpr int CONC_SLOTS = 1024;      // LDS table of k_s2a_conc (12 KiB a block)
constexpr int CONC_PROBES = 8;
constexpr int CONC_WPB = 4;
constexpr int CONC_READ_LDS = 2048;   // slots (cycles + 256 qualities) of one read kept in LDS at most
constexpr int CONC_UNITS_PER_WAVE = 16;  // a block's flush is one atomic per used slot: shared by 64 units
constexpr int64_t CONC_BLOCK_CAP = 1024;

struct ConcArgs {
    const uint8_t *seq, *qual;
    const int64_t *soff;
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int64_t *units;     // per merge unit: row1, row2 (-1: single)
    const int32_t *uref;
    const uint8_t *orient;    // per merge unit: bit 0 row1 is read 2, bit 1 row1 is reversed; bits 2, 3 row2
    int64_t n;
    const int64_t *lo, *base; // per reference: first position of its window, its offset in a plane
    const int32_t *wlen;      // per reference: positions in its window (a plane holds wlen + 1)
    int64_t total;            // entries of one plane
    int32_t *acc;             // CONC_PLANES planes
    unsigned long long *rd;   // [compared, mismatch][read][stride]: slot = cycle, or max_len + 1 + quality byte
    int stride, max_len, rd_lds, ops_cap;
    int32_t *err;             // set when a position or a cycle falls outside its table
};

__device__ __forceinline__ void conc_add(const ConcArgs &A, unsigned long long *tkey, int32_t *tval,
                                         int plane, int64_t g, int d)
{
    const int64_t at = (int64_t)plane * A.total + g;
    const unsigned long long key = (unsigned long long)at + 1ull;
    unsigned s = (unsigned)hash_key(key) & (CONC_SLOTS - 1);
    for (int t = 0; t < CONC_PROBES; ++t, s = (s + 1) & (CONC_SLOTS - 1)) {
        const unsigned long long old = atomicCAS(&tkey[s], 0ull, key);
        if (old == 0ull || old == key) {
            atomicAdd(&tval[s], d);
            return;
        }
    }
    atomicAdd(&A.acc[at], d);
}

__device__ __forceinline__ void conc_read_add(const ConcArgs &A, uint32_t *rl, int read, int slot,
                                              bool differ)
{
    const int i = read * A.stride + slot;
    if (A.rd_lds) {
        atomicAdd(&rl[i], 1u);
        if (differ) atomicAdd(&rl[2 * A.stride + i], 1u);
    } else {
        atomicAdd(&A.rd[i], 1ull);
        if (differ) atomicAdd(&A.rd[2 * A.stride + i], 1ull);
    }
}

// the op offsets of row r as k_s2a_merge scans them: oref[o], ord[o] = the
// reference and read offset op o starts at (ord -1: a D op), one past the
// last op the totals.  Returns the reference span; read_len = the read bases
__device__ __forceinline__ int conc_ops(const ConcArgs &A, int64_t r, int32_t *oref, int32_t *ord,
                                        int lane, int &read_len)
{
    const int nc = A.n_cig[r];
    const uint32_t *ops = A.cig + A.cig_off[r];
    int rf0 = 0, rd0 = 0;
    for (int o0 = 0; o0 < nc; o0 += 64) {
        const int o = o0 + lane;
        int dref = 0, dread = 0, isd = 0;
        if (o < nc) {
            const uint32_t op = ops[o];
            const int n = (int)(op >> 4), t = (int)(op & 15);
            if (t == MH_OP_M) { dref = n; dread = n; }
            else if (t == MH_OP_D) { dref = n; isd = 1; }
            else dread = n;                      // I, S (checked on the host)
        }
        const int iref = s2a_scan(dref, lane), iread = s2a_scan(dread, lane);
        if (o < nc) {
            oref[o] = rf0 + iref - dref;
            ord[o] = isd ? -1 : rd0 + iread - dread;
        }
        rf0 += __shfl(iref, 63, 64);
        rd0 += __shfl(iread, 63, 64);
    }
    if (lane == 0) { oref[nc] = rf0; ord[nc] = rd0; }
    read_len = rd0;
    return rf0;
}

// the mate's byte, quality and read index (-1: deleted) at offset t of its span
__device__ __forceinline__ void conc_at(const int32_t *oref, const int32_t *ord, const uint8_t *s,
                                        const uint8_t *q, int t, int read_len, unsigned char &c,
                                        unsigned char &qq, int &x)
{
    int o = 0;
    while (oref[o + 1] <= t) ++o;
    const int rd = ord[o];
    c = '-'; qq = ' '; x = -1;
    if (rd >= 0) {
        const int i = rd + (t - oref[o]);
        if (i < read_len) { x = i; c = s[i]; qq = q[i]; }
    }
}

__global__ __launch_bounds__(64 * CONC_WPB) void k_s2a_conc(ConcArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long tkey[CONC_SLOTS];
    __shared__ int32_t tval[CONC_SLOTS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    const int nrl = A.rd_lds ? 4 * A.stride : 0;
    uint32_t *rl = (uint32_t *)smem;
    int32_t *wops = (int32_t *)(smem + (((size_t)nrl * 4 + 15) & ~(size_t)15)) +
                    (size_t)wv * 4 * (A.ops_cap + 1);
    // named, not indexed by a run-time mate: nothing here lives in scratch memory
    int32_t *oref0 = wops, *ord0 = wops + (A.ops_cap + 1);
    int32_t *oref1 = wops + 2 * (A.ops_cap + 1), *ord1 = wops + 3 * (A.ops_cap + 1);
    for (int s = threadIdx.x; s < CONC_SLOTS; s += blockDim.x) { tkey[s] = 0ull; tval[s] = 0; }
    for (int s = threadIdx.x; s < nrl; s += blockDim.x) rl[s] = 0u;
    __syncthreads();

    for (int64_t u = (int64_t)blockIdx.x * wpb + wv; u < A.n; u += (int64_t)gridDim.x * wpb) {
        const int64_t r0 = A.units[2 * u], r1 = A.units[2 * u + 1];
        if (r1 < 0) continue;                         // an unpaired unit: nothing to compare
        int len0, len1;
        const int rf0 = conc_ops(A, r0, oref0, ord0, lane, len0);
        const int rf1 = conc_ops(A, r1, oref1, ord1, lane, len1);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t p0 = A.pos[r0], p1 = A.pos[r1];
        const int64_t lo = p0 > p1 ? p0 : p1;
        const int64_t hi = p0 + rf0 < p1 + rf1 ? p0 + rf0 : p1 + rf1;
        if (hi > lo) {
            const int ref = A.uref[u];
            const int64_t w0 = A.lo[ref], gb = A.base[ref];
            if (lo < w0 || hi - w0 > (int64_t)A.wlen[ref]) {   // the host sized the window from the same rows
                if (lane == 0) atomicExch(A.err, 1);
            } else {
                if (lane == 0) {
                    conc_add(A, tkey, tval, CONC_OVERLAP, gb + (lo - w0), 1);
                    conc_add(A, tkey, tval, CONC_OVERLAP, gb + (hi - w0), -1);
                }
                const int ob = A.orient[u];
                const int read0 = ob & 1, rev0 = (ob >> 1) & 1, read1 = (ob >> 2) & 1, rev1 = (ob >> 3) & 1;
                const uint8_t *s0 = A.seq + A.soff[r0], *q0 = A.qual + A.soff[r0];
                const uint8_t *s1 = A.seq + A.soff[r1], *q1 = A.qual + A.soff[r1];
                for (int64_t y0 = lo; y0 < hi; y0 += 64) {
                    const int64_t y = y0 + lane;
                    if (y >= hi) continue;
                    unsigned char c0, c1, b0, b1;
                    int x0, x1;
                    conc_at(oref0, ord0, s0, q0, (int)(y - p0), len0, c0, b0, x0);
                    conc_at(oref1, ord1, s1, q1, (int)(y - p1), len1, c1, b1, x1);
                    const bool differ = c0 != c1;
                    if (differ) {
                        const int cls = (c0 == 'N' || c1 == 'N') ? CONC_NOCALL
                                        : (c0 == '-' || c1 == '-') ? CONC_INDEL : CONC_MISMATCH;
                        conc_add(A, tkey, tval, cls, gb + (y - w0), 1);
                        const int dq = (int)b0 - (int)b1;
                        if (dq > -5 && dq < 5) conc_add(A, tkey, tval, CONC_UNRESOLVED, gb + (y - w0), 1);
                    }
                    if (x0 >= 0 && x1 >= 0 && c0 != 'N' && c1 != 'N') {
                        const int cy0 = rev0 ? len0 - x0 : x0 + 1, cy1 = rev1 ? len1 - x1 : x1 + 1;
                        if (cy0 < 1 || cy0 > A.max_len || cy1 < 1 || cy1 > A.max_len) {
                            atomicExch(A.err, 1);
                        } else {
                            conc_read_add(A, rl, read0, cy0, differ);
                            conc_read_add(A, rl, read0, A.max_len + 1 + b0, differ);
                            conc_read_add(A, rl, read1, cy1, differ);
                            conc_read_add(A, rl, read1, A.max_len + 1 + b1, differ);
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();              // the next unit rewrites the op offsets
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CONC_SLOTS; s += blockDim.x)
        if (tkey[s] && tval[s]) atomicAdd(&A.acc[tkey[s] - 1ull], tval[s]);
    for (int s = threadIdx.x; s < nrl; s += blockDim.x)
        if (rl[s]) atomicAdd(&A.rd[s], (unsigned long long)rl[s]);
}

__global__ __launch_bounds__(1024) void k_s2a_conc_scan(const int64_t *base, const int32_t *wlen,
                                                        int64_t total, const int32_t *acc,
                                                        int32_t *idx_out, int32_t *cnt_out, int32_t *n_out)
{
    __shared__ int32_t wsum[16], wnz[16];
    const int ref = blockIdx.x;
    const int64_t b = base[ref];
    const int n = wlen[ref] + 1;           // 0 for a reference without paired units (wlen -1)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int carry = 0, outn = 0;
    for (int i0 = 0; i0 < n; i0 += blockDim.x) {
        const int i = i0 + (int)threadIdx.x;
        const int v = i < n ? acc[b + i] : 0;
        const int s = s2a_scan(v, lane);
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < nw; ++w) { const int t = wsum[w]; pre += w < wv ? t : 0; tot += t; }
        const int cov = carry + pre + s;
        const int nz = i < n && cov != 0;
        const int f = s2a_scan(nz, lane);
        if (lane == 63) wnz[wv] = f;
        __syncthreads();
        int pre2 = 0, tot2 = 0;
        for (int w = 0; w < nw; ++w) { const int t = wnz[w]; pre2 += w < wv ? t : 0; tot2 += t; }
        if (nz) {
            const int64_t k = b + outn + pre2 + f - 1;     // < b + n: one row per position at most
            idx_out[k] = i;
            cnt_out[k] = cov;
#pragma unroll
            for (int pl = 1; pl < CONC_PLANES; ++pl) cnt_out[pl * total + k] = acc[pl * total + b + i];
        }
        carry += tot;
        outn += tot2;
        __syncthreads();                   // wsum / wnz are rewritten by the next chunk
    }
    if (threadIdx.x == 0) n_out[ref] = outn;
}

int s2a_conc_run(Ctx &c, S2AState &S)
{
    S2AConc &Q = S.conc;
    if (Q.done) return 0;
    if (S.clip.state == CLIP_NONE) {
        set_error("sam2aln concordance: no rows of a sam2aln call are on the device");
        return -3;
    }
    const S2ADevRows &rows = S.clip.rows;
    if (S.n_merge && rows.cig != S.d_cig && (!c.map.valid || rows.cig != c.map.pool)) {
        set_error("sam2aln concordance: the mapping pass the rows came from is gone");
        return -3;
    }
    if (S.n_merge && rows.soff != S.d_soff && (rows.soff != c.reads.off || S.staged_reads != c.reads.n)) {
        set_error("sam2aln concordance: the resident reads the rows came from are gone");
        return -3;
    }
    Q.name.clear(); Q.pos.clear(); Q.count.clear(); Q.reads.clear();
    Q.text_valid[0] = Q.text_valid[1] = false;
    const int nref = (int)S.names.size();
    const int64_t nu = (int64_t)S.u1.size();
    // ---- per paired unit its orientation bits; each reference's window from
    // its paired units' mapped intervals; the longest read and CIGAR ----
    std::vector<uint8_t> orient((size_t)S.n_merge, 0);
    std::vector<int64_t> lo((size_t)nref, INT64_MAX), hi((size_t)nref, INT64_MIN);
    int max_len = 0, ops_cap = 1;
    int64_t paired = 0, span_max = 1;
    for (int64_t u = 0; S.n_merge && u < nu; ++u) {
        if (S.ucause[u] >= 0 || !S.upaired[u] || S.u2[u] < 0) continue;
        const int g = S.name_id[u];
        int bits = 0, k = 0;
        for (int64_t r : {S.u1[u], S.u2[u]}) {
            // the read's length is its CIGAR's read bases, as the kernel takes it
            // (S.slen holds it only for the rows insert.csv quotes on the resident route)
            int64_t span = 0, bases = 0;
            for (int o = 0; o < S.n_cig[r]; ++o) {
                const uint32_t op = S.cig[S.cig_off[r] + o];
                if ((op & 15) == MH_OP_M || (op & 15) == MH_OP_D) span += op >> 4;
                if ((op & 15) != MH_OP_D) bases += op >> 4;
            }
            lo[g] = std::min(lo[g], (int64_t)S.pos[r]);
            hi[g] = std::max(hi[g], (int64_t)S.pos[r] + span);
            span_max = std::max(span_max, span);
            max_len = (int)std::max<int64_t>(max_len, bases);
            ops_cap = std::max(ops_cap, S.n_cig[r]);
            bits |= (((S.flag[r] & 0x40) ? 0 : 1) | ((S.flag[r] & 0x10) ? 2 : 0)) << (2 * k++);
        }
        orient[(size_t)S.merge_of_unit[u]] = (uint8_t)bits;
        ++paired;
    }
    std::vector<int64_t> base((size_t)nref + 1, 0);
    std::vector<int32_t> wlen((size_t)nref, -1);
    for (int g = 0; g < nref; ++g) {
        if (lo[g] > hi[g]) { lo[g] = 0; base[g + 1] = base[g]; continue; }
        if (hi[g] - lo[g] > S2A_CLIP_MAX_WINDOW) {
            set_error("sam2aln concordance: the rows of %s span positions %lld to %lld, more than %lld",
                      S.names[g].c_str(), (long long)lo[g], (long long)hi[g],
                      (long long)S2A_CLIP_MAX_WINDOW);
            return -3;
        }
        wlen[g] = (int32_t)(hi[g] - lo[g]);
        base[g + 1] = base[g] + wlen[g] + 1;
    }
    const int64_t total = base[nref];
    if (paired == 0 || total == 0) { Q.done = true; return 0; }
    const int stride = max_len + 1 + 256;
    const int rd_lds = stride <= CONC_READ_LDS ? 1 : 0;
    const size_t rd_bytes = rd_lds ? (((size_t)4 * stride * 4 + 15) & ~(size_t)15) : 0;
    const size_t wave_bytes = (size_t)16 * (ops_cap + 1);
    int wpb = CONC_WPB;
    while (wpb > 1 && rd_bytes + wpb * wave_bytes > S2A_LDS_BYTES - 16 * 1024) --wpb;
    if (rd_bytes + wave_bytes > S2A_LDS_BYTES - 16 * 1024) {
        set_error("sam2aln concordance: a read with %d CIGAR ops is too many for LDS", ops_cap);
        return -3;
    }
    hipStream_t s = c.stream;
    if (int st = s2a_upload(S, Q.d_orient, orient, s)) return st;
    if (int st = s2a_upload(S, Q.d_lo, lo, s)) return st;
    if (int st = s2a_upload(S, Q.d_base, base, s)) return st;
    if (int st = s2a_upload(S, Q.d_wlen, wlen, s)) return st;
    if (int st = dev_reserve(S, Q.d_acc, sizeof(int32_t) * CONC_PLANES * (size_t)total)) return st;
    if (int st = dev_reserve(S, Q.d_idx, sizeof(int32_t) * (size_t)total)) return st;
    if (int st = dev_reserve(S, Q.d_cnt, sizeof(int32_t) * CONC_PLANES * (size_t)total)) return st;
    if (int st = dev_reserve(S, Q.d_n, sizeof(int32_t) * ((size_t)nref + 1))) return st;
    if (int st = dev_reserve(S, Q.d_rd, sizeof(unsigned long long) * 4 * (size_t)stride)) return st;
    MH_HIP(hipMemsetAsync(Q.d_acc, 0, sizeof(int32_t) * CONC_PLANES * (size_t)total, s));
    MH_HIP(hipMemsetAsync(Q.d_n, 0, sizeof(int32_t) * ((size_t)nref + 1), s));
    MH_HIP(hipMemsetAsync(Q.d_rd, 0, sizeof(unsigned long long) * 4 * (size_t)stride, s));
    ConcArgs a{rows.seq, rows.qual, rows.soff, rows.pos, rows.cig_off, rows.n_cig, rows.cig,
               S.d_units, S.d_uref, Q.d_orient, S.n_merge, Q.d_lo, Q.d_base, Q.d_wlen, total,
               Q.d_acc, Q.d_rd, stride, max_len, rd_lds, ops_cap, Q.d_n + nref};
    int64_t blocks = (S.n_merge + wpb * CONC_UNITS_PER_WAVE - 1) / (wpb * CONC_UNITS_PER_WAVE);
    if (blocks > CONC_BLOCK_CAP) blocks = CONC_BLOCK_CAP;
    // a block's 32-bit LDS sums stay below 2^31: a unit adds at most its overlap to one
    // slot, and a block takes at most n_merge / blocks + wpb units
    const int64_t need = (S.n_merge * span_max >> 30) + 1;
    if (blocks < need) blocks = need;
    const int64_t max_blocks = c.test_caps.s2a_max_blocks;
    if (max_blocks > 0 && blocks > max_blocks && need <= max_blocks) blocks = max_blocks;
    const size_t dyn = rd_bytes + wpb * wave_bytes;
    MH_HIP(hipFuncSetAttribute((const void *)k_s2a_conc, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)dyn));
    const int p0 = prof_begin(c, "k_s2a_conc");
    hipLaunchKernelGGL(k_s2a_conc, dim3((unsigned)blocks), dim3(64 * wpb), dyn, s, a);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    const int p1 = prof_begin(c, "k_s2a_conc_scan");
    hipLaunchKernelGGL(k_s2a_conc_scan, dim3((unsigned)nref), dim3(1024), 0, s, Q.d_base, Q.d_wlen, total,
                       Q.d_acc, Q.d_idx, Q.d_cnt, Q.d_n);
    prof_end(c, p1);
    MH_HIP(hipGetLastError());
    std::vector<int32_t> n_out((size_t)nref + 1);
    std::vector<unsigned long long> rd((size_t)4 * stride);
    MH_HIP(hipMemcpyAsync(n_out.data(), Q.d_n, sizeof(int32_t) * n_out.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(rd.data(), Q.d_rd, sizeof(unsigned long long) * rd.size(),
                          hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    if (n_out[nref]) {
        set_error("sam2aln concordance: a position or a cycle fell outside its table");
        return -4;
    }
    // ---- the rows of each reference, references as Python sorts str ----
    std::vector<int> order((size_t)nref);
    for (int g = 0; g < nref; ++g) order[g] = g;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return S.names[x] < S.names[y]; });
    std::vector<int64_t> at((size_t)nref + 1, 0);
    for (int k = 0; k < nref; ++k) {
        const int g = order[k];
        if (n_out[g] < 0 || n_out[g] > wlen[g] + 1) {
            set_error("sam2aln concordance: %d positions counted in a window of %d", n_out[g], wlen[g] + 1);
            return -4;
        }
        at[k + 1] = at[k] + n_out[g];
    }
    const size_t nrow = (size_t)at[nref];
    std::vector<int32_t> idx(nrow), planes(CONC_PLANES * nrow);
    for (int k = 0; k < nref; ++k) {
        const int g = order[k];
        if (!n_out[g]) continue;
        const size_t nb = sizeof(int32_t) * (size_t)n_out[g];
        MH_HIP(hipMemcpyAsync(idx.data() + at[k], Q.d_idx + base[g], nb, hipMemcpyDeviceToHost, s));
        for (int pl = 0; pl < CONC_PLANES; ++pl)
            MH_HIP(hipMemcpyAsync(planes.data() + pl * nrow + at[k], Q.d_cnt + pl * total + base[g], nb,
                                  hipMemcpyDeviceToHost, s));
    }
    MH_HIP(hipStreamSynchronize(s));
    Q.name.resize(nrow);
    Q.pos.resize(nrow);
    Q.count.resize(CONC_PLANES * nrow);
    for (int k = 0; k < nref; ++k)
        for (int64_t j = at[k]; j < at[k + 1]; ++j) {
            Q.name[j] = order[k];
            Q.pos[j] = lo[order[k]] + idx[j];
            for (int pl = 0; pl < CONC_PLANES; ++pl) Q.count[CONC_PLANES * j + pl] = planes[pl * nrow + j];
        }
    // ---- the read table's keys with compared > 0: read, then cycles, then qualities ----
    for (int read = 0; read < 2; ++read)
        for (int by = 0; by < 2; ++by) {
            const int s0 = by ? max_len + 1 : 1, s1 = by ? stride : max_len + 1;
            for (int sl = s0; sl < s1; ++sl) {
                const unsigned long long cmp = rd[(size_t)read * stride + sl];
                if (!cmp) continue;
                const int64_t value = by ? sl - (max_len + 1) - 33 : sl;
                Q.reads.insert(Q.reads.end(), {(int64_t)read + 1, (int64_t)by, value, (int64_t)cmp,
                                               (int64_t)rd[(size_t)(2 + read) * stride + sl]});
            }
        }
    Q.done = true;
    return 0;
}

// concordance.csv (which 0) or cycle_concordance.csv (1) of S.conc's lists
static void s2a_conc_text(S2AState &S, int which)
{
    S2AConc &Q = S.conc;
    if (Q.text_valid[which]) return;
    std::string &o = Q.text[which];
    if (which == 0) {
        o.assign("refname,pos,overlap,mismatch,indel,nocall,unresolved\n");
        for (size_t j = 0; j < Q.name.size(); ++j) {
            const std::string &rn = S.names[Q.name[j]];
            csv_field(o, rn.data(), rn.size());
            o.push_back(',');
            o += std::to_string((long long)Q.pos[j]);
            for (int pl = 0; pl < CONC_PLANES; ++pl) {
                o.push_back(',');
                o += std::to_string(Q.count[CONC_PLANES * j + pl]);
            }
            o.push_back('\n');
        }
    } else {
        o.assign("read,by,value,compared,mismatch\n");
        for (size_t j = 0; j + 4 < Q.reads.size(); j += 5) {
            o += std::to_string((long long)Q.reads[j]);
            o += Q.reads[j + 1] ? ",quality," : ",cycle,";
            o += std::to_string((long long)Q.reads[j + 2]);
            o.push_back(',');
            o += std::to_string((long long)Q.reads[j + 3]);
            o.push_back(',');
            o += std::to_string((long long)Q.reads[j + 4]);
            o.push_back('\n');
        }
    }
    Q.text_valid[which] = true;
}

// the concordance of the context's last sam2aln call, counted now if not yet
static int s2a_conc_of(mh_ctx *ctx, const char *what, int which, S2AState **out)
{
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("%s: no sam2aln results", what); return -3; }
    if (which > 1) { set_error("%s: which must be 0 (positions) or 1 (reads)", what); return -3; }
    MH_HIP(hipSetDevice(c.device));
    try {
        if (int st = s2a_conc_run(c, *c.s2a)) return st;
        if (which >= 0) s2a_conc_text(*c.s2a, which);
    } catch (const std::exception &e) {
        c.s2a->conc.done = c.s2a->conc.text_valid[0] = c.s2a->conc.text_valid[1] = false;
        set_error("%s: out of memory (%s)", what, e.what());
        return -2;
    }
    *out = c.s2a;
    return 0;
}

// ---------------------------------------------------------------------------
// Strand support (strand.csv; DESIGN.md section 6, "Strand support").  A unit
// counts at the cutoffs at which its merge entry is S2A_OK.  At index j of its
// merged string (position y = j + 1) with merged character m in "ACGT-", a
// mate supports m when its own expansion holds the byte m at y; the unit adds
// 1 to m_fwd / m_rev when a supporting mate is forward / reversed and to
// m_both when both hold.
//
// k_s2a_strand       one wave per unit, the mates expanded into LDS as
//                    k_s2a_merge expands them, (ch, thr) of every position from
//                    the merge's own s2a_pos.  With the cutoffs sorted, a
//                    position passes the first p of them and the unit is OK at
//                    a set of them (from res, not assumed monotone): when that
//                    set is the first nok cutoffs, the position makes ONE add,
//                    to class min(p, nok) of key = character * 3 + (fwd only,
//                    rev only, both); the count at sorted cutoff k is the sum of
//                    the classes above k.  Any other OK set adds +1 / -1 at the
//                    ends of its runs, straight to HBM.  The one add goes to the
//                    block's LDS window: STRAND_KEYS * classes planes of `win`
//                    positions from the address win0 of the call's densest
//                    stretch, 16-bit counters two to a word, laid out so that a
//                    wave's 64 consecutive positions fall into 64 different
//                    words and banks.  A unit adds at most 1 to a counter and
//                    the host sizes the grid so that a block takes fewer than
//                    65536 units: no half carries into the other.  Adds outside
//                    the window go straight to HBM.  The block flushes one
//                    atomic per used counter.  Integer adds only.
// k_s2a_strand_scan  one block per (reference, cutoff): the classes above the
//                    cutoff summed per key, fwd = fwd only + both, rev = rev
//                    only + both, and the positions with any count compacted in
//                    position order as k_s2a_clip_scan compacts them.
// ---------------------------------------------------------------------------
constexpr int STRAND_WPB = 16;
constexpr int STRAND_UNITS_PER_WAVE = 32;     // a block's flush is shared by 512 units at least
constexpr int64_t STRAND_BLOCK_CAP = 256;     // one block a CU: each flushes up to a window of atomics
constexpr int64_t STRAND_BLOCK_UNITS = 65535; // units of one block at most: what a 16-bit counter holds

struct StrandArgs {
    const uint8_t *seq, *qual;
    const int64_t *soff;
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int64_t *units;     // per merge unit: row1, row2 (-1: single)
    const int32_t *uref;
    const uint8_t *orient;    // per merge unit: bit 0 row1 is reversed, bit 1 row2
    const int32_t *res;       // the merge's 4 per entry: status first
    int64_t n;
    int n_cut;
    unsigned char cut[S2A_MAX_CUTS];    // q_cutoff + 33, ascending
    unsigned char entry[S2A_MAX_CUTS];  // the call's index of sorted cutoff k
    int span_cap, ops_cap, wave_bytes;
    const int64_t *lo, *base; // per reference: first padded index of its window, its offset in a plane
    const int32_t *wlen;      // per reference: indexes in its window
    int64_t total;            // entries of one plane
    int64_t win0;             // first address of the LDS window
    int win;                  // its positions, a multiple of 128
    int32_t *acc;             // n_cut * STRAND_KEYS planes: (class - 1) * STRAND_KEYS + key
    int32_t *err;             // set when a position falls outside its window
};

__global__ __launch_bounds__(64 * STRAND_WPB) void k_s2a_strand(StrandArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    const int half = A.win >> 1;                                // words of one plane
    const int nword = A.n_cut * STRAND_KEYS * half;
    uint32_t *cnt = (uint32_t *)smem;
    unsigned char *wb = smem + (size_t)nword * 4 + (size_t)wv * A.wave_bytes;
    char *cq = (char *)wb;                                     // c0 q0 c1 q1, span_cap each
    int32_t *opref = (int32_t *)(wb + 4 * (size_t)A.span_cap); // ops_cap + 1 per mate
    int32_t *opread = opref + 2 * (A.ops_cap + 1);
    for (int s = threadIdx.x; s < nword; s += blockDim.x) cnt[s] = 0u;
    __syncthreads();

    for (int64_t u = (int64_t)blockIdx.x * wpb + wv; u < A.n; u += (int64_t)gridDim.x * wpb) {
        // the cutoffs (sorted) at which the unit is OK
        int en = 0;                                // lane k < n_cut: the entry of sorted cutoff k
#pragma unroll
        for (int k = 0; k < S2A_MAX_CUTS; ++k) en = lane == k ? A.entry[k] : en;
        const bool isok = lane < A.n_cut && A.res[4 * (u * A.n_cut + en)] == S2A_OK;
        const unsigned okm = (unsigned)__ballot(isok);
        if (!okm) continue;
        const int nok = __popc(okm);
        const bool prefix = okm == (1u << nok) - 1u;
        const int64_t rows[2] = {A.units[2 * u], A.units[2 * u + 1]};
        const int nm = rows[1] >= 0 ? 2 : 1;
        // named mates, every loop over them unrolled (see k_s2a_merge)
        Mate mt[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            mt[k].row = -1; mt[k].pad = 0; mt[k].rf = 0; mt[k].len = 0;
            mt[k].c = cq + 2 * k * A.span_cap;
            mt[k].q = cq + (2 * k + 1) * A.span_cap;
        }
        // ---- apply_cigar as k_s2a_merge runs it ----
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nm) break;
            const int64_t r = rows[k];
            const int nc = A.n_cig[r];
            const uint32_t *ops = A.cig + A.cig_off[r];
            int32_t *oref = opref + k * (A.ops_cap + 1), *ord = opread + k * (A.ops_cap + 1);
            int rf0 = 0, rd0 = 0;
            for (int o0 = 0; o0 < nc; o0 += 64) {
                const int o = o0 + lane;
                int dref = 0, dread = 0, isd = 0;
                if (o < nc) {
                    const uint32_t op = ops[o];
                    const int n = (int)(op >> 4), t = (int)(op & 15);
                    if (t == MH_OP_M) { dref = n; dread = n; }
                    else if (t == MH_OP_D) { dref = n; isd = 1; }
                    else dread = n;                      // I, S (checked on the host)
                }
                const int iref = s2a_scan(dref, lane), iread = s2a_scan(dread, lane);
                if (o < nc) {
                    oref[o] = rf0 + iref - dref;
                    ord[o] = isd ? -1 : rd0 + iread - dread;
                }
                rf0 += __shfl(iref, 63, 64);
                rd0 += __shfl(iread, 63, 64);
            }
            if (lane == 0) { oref[nc] = rf0; ord[nc] = rd0; }
            const int p = A.pos[r] - 1;
            mt[k].row = (int)r;
            mt[k].pad = p > 0 ? p : 0;
            mt[k].rf = rf0;
            mt[k].len = mt[k].pad + rf0;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nm) break;
            const int64_t r = rows[k];
            const int32_t *oref = opref + k * (A.ops_cap + 1), *ord = opread + k * (A.ops_cap + 1);
            const uint8_t *s = A.seq + A.soff[r], *q = A.qual + A.soff[r];
            for (int t = lane; t < mt[k].rf; t += 64) {
                int o = 0;
                while (oref[o + 1] <= t) ++o;
                const int rd = ord[o];
                char c = '-', qq = ' ';
                if (rd >= 0) {
                    const int x = rd + (t - oref[o]);
                    c = (char)s[x];
                    qq = (char)q[x];
                }
                mt[k].c[t] = c;
                mt[k].q[t] = qq;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        // ---- merge_pairs roles and starts, as k_s2a_merge takes them ----
        const bool single = nm == 1;
        const int ob = A.orient[u];
        Mate a = mt[0], b = mt[0];
        bool reva = ob & 1, revb = ob & 1;
        if (!single) {
            if (mt[0].len > mt[1].len) { a = mt[1]; b = mt[0]; reva = ob & 2; }
            else { a = mt[0]; b = mt[1]; revb = ob & 2; }
        }
        const int len2 = b.len;
        int rev_start = 1 << 30, fwd_start = 1 << 30;
        if (!single) {
            for (int i0 = 0; i0 < len2; i0 += 64) {
                const int i = i0 + lane;
                int rs = 1 << 30, fs = 1 << 30;
                if (i < len2) {
                    const char c2 = (i >= b.pad) ? b.c[i - b.pad] : '-';
                    if (c2 != '-') rs = i;
                    if (i < a.len) {
                        const char c1 = (i >= a.pad) ? a.c[i - a.pad] : '-';
                        if (!(c1 == '-' && c2 == '-')) fs = i;
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    rs = min(rs, __shfl_xor(rs, o, 64));
                    fs = min(fs, __shfl_xor(fs, o, 64));
                }
                rev_start = min(rev_start, rs);
                fwd_start = min(fwd_start, fs);
                if (rev_start < (1 << 30) && (fwd_start < (1 << 30) || i0 + 64 >= a.len)) break;
            }
        }
        const bool fwd = single || fwd_start < a.len;
        const int ibase = fwd ? 0 : a.len;
        const int mlen = len2 - ibase;
        const int ref = A.uref[u];
        const int64_t w0 = A.lo[ref], gb = A.base[ref];
        const int wl = A.wlen[ref];
        // no mate holds a byte below the smaller pad: nothing supports there
        const int jlo = (single ? b.pad : min(a.pad, b.pad)) & ~63;
        for (int j0 = jlo; j0 < mlen; j0 += 64) {
            const int j = j0 + lane;
            if (j >= mlen) continue;
            const int i = j + ibase;
            char ch = '-';
            unsigned char thr = S2A_ALWAYS;
            if (single || !fwd || i >= fwd_start) s2a_pos(i, a, b, single, rev_start, ch, thr);
            const int mi = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : ch == '-' ? 4 : -1;
            if (mi < 0) continue;
            // support is looked up at y = j + 1, padded index j, whatever ibase
            const bool sa = !single && j >= a.pad && j < a.len && a.c[j - a.pad] == ch;
            const bool sb = j >= b.pad && j < b.len && b.c[j - b.pad] == ch;
            const bool sf = (sa && !reva) || (sb && !revb), sr = (sa && reva) || (sb && revb);
            if (!sf && !sr) continue;
            const int key = mi * 3 + (sf && sr ? 2 : sr ? 1 : 0);
            int p = 0;
#pragma unroll
            for (int k = 0; k < S2A_MAX_CUTS; ++k) p += k < A.n_cut && thr > A.cut[k];
            const int64_t rel = (int64_t)j - w0;
            if (rel < 0 || rel > (int64_t)wl) {          // the host sized the window from the same rows
                atomicExch(A.err, 1);
                continue;
            }
            const int64_t g = gb + rel;
            if (prefix) {
                const int cls = min(p, nok);
                if (cls < 1) continue;
                const int plane = (cls - 1) * STRAND_KEYS + key;
                const int64_t x = g - A.win0;
                if (x >= 0 && x < (int64_t)A.win) {
                    const int xi = (int)x;
                    atomicAdd(&cnt[plane * half + ((xi >> 7) << 6) + (xi & 63)], 1u << (((xi >> 6) & 1) << 4));
                } else {
                    atomicAdd(&A.acc[(int64_t)plane * A.total + g], 1);
                }
            } else {
                // runs of counted cutoffs [s, e): +1 to class e, -1 to class s
#pragma unroll
                for (int k = 0; k < S2A_MAX_CUTS; ++k) {
                    const bool in = k < p && ((okm >> k) & 1u);
                    const bool before = k > 0 && k - 1 < p && ((okm >> (k - 1)) & 1u);
                    const bool after = k + 1 < p && ((okm >> (k + 1)) & 1u);
                    if (in && !after) atomicAdd(&A.acc[(int64_t)(k * STRAND_KEYS + key) * A.total + g], 1);
                    if (in && !before && k > 0)
                        atomicAdd(&A.acc[(int64_t)((k - 1) * STRAND_KEYS + key) * A.total + g], -1);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();              // the next unit rewrites the expansion
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nword; s += blockDim.x) {
        const uint32_t v = cnt[s];
        if (!v) continue;
        const int plane = s / half, r = s - plane * half;
        const int64_t g = A.win0 + ((int64_t)(r >> 6) << 7) + (r & 63);
        int32_t *dst = A.acc + (int64_t)plane * A.total;
        if (v & 0xffffu) atomicAdd(&dst[g], (int32_t)(v & 0xffffu));      // g + 64 < total where the high half counted
        if (v >> 16) atomicAdd(&dst[g + 64], (int32_t)(v >> 16));
    }
}

__global__ __launch_bounds__(1024) void k_s2a_strand_scan(const int64_t *base, const int32_t *wlen,
                                                          int64_t total, int n_cut, int nref,
                                                          const int32_t *acc, int32_t *idx_out,
                                                          int32_t *cnt_out, int32_t *n_out,
                                                          const unsigned char *rank_of)
{
    __shared__ int32_t wnz[16];
    const int ref = blockIdx.x, kk = blockIdx.y;   // kk: the call's cutoff index
    const int k0 = rank_of[kk];                    // classes k0 + 1 .. n_cut pass it
    const int64_t b = base[ref];
    const int n = wlen[ref] + 1;           // 0 for a reference without units (wlen -1)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t ob = (int64_t)kk * STRAND_KEYS * total;
    int outn = 0;
    for (int i0 = 0; i0 < n; i0 += blockDim.x) {
        const int i = i0 + (int)threadIdx.x;
        int32_t v[STRAND_KEYS];
        int any = 0;
#pragma unroll
        for (int key = 0; key < STRAND_KEYS; ++key) {
            int s = 0;
            if (i < n)
                for (int cl = k0; cl < n_cut; ++cl) s += acc[(int64_t)(cl * STRAND_KEYS + key) * total + b + i];
            v[key] = s;
            any |= s;
        }
        const int nz = any != 0;
        const int f = s2a_scan(nz, lane);
        if (lane == 63) wnz[wv] = f;
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < nw; ++w) { const int t = wnz[w]; pre += w < wv ? t : 0; tot += t; }
        if (nz) {
            const int64_t k = b + outn + pre + f - 1;      // < b + n: one row per position at most
            idx_out[(int64_t)kk * total + k] = i;
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const int both = v[3 * m + 2];
                cnt_out[ob + (int64_t)(3 * m) * total + k] = v[3 * m] + both;
                cnt_out[ob + (int64_t)(3 * m + 1) * total + k] = v[3 * m + 1] + both;
                cnt_out[ob + (int64_t)(3 * m + 2) * total + k] = both;
            }
        }
        outn += tot;
        __syncthreads();                   // wnz is rewritten by the next chunk
    }
    if (threadIdx.x == 0) n_out[kk * nref + ref] = outn;
}

int s2a_strand_run(Ctx &c, S2AState &S)
{
    S2AStrand &T = S.strand;
    if (T.done) return 0;
    if (S.clip.state == CLIP_NONE) {
        set_error("sam2aln strand: no rows of a sam2aln call are on the device");
        return -3;
    }
    const S2ADevRows &rows = S.clip.rows;
    if (S.n_merge && rows.cig != S.d_cig && (!c.map.valid || rows.cig != c.map.pool)) {
        set_error("sam2aln strand: the mapping pass the rows came from is gone");
        return -3;
    }
    if (S.n_merge && rows.soff != S.d_soff && (rows.soff != c.reads.off || S.staged_reads != c.reads.n)) {
        set_error("sam2aln strand: the resident reads the rows came from are gone");
        return -3;
    }
    T.name.clear(); T.qcut.clear(); T.pos.clear(); T.count.clear();
    T.text_valid = false;
    const int nref = (int)S.names.size();
    const int nc = (int)S.q_cutoffs.size();
    const int64_t nu = (int64_t)S.u1.size();
    if (S.n_merge == 0 || nref == 0) { T.done = true; return 0; }
    // ---- per unit its strand bits; each reference's window of padded indexes
    // from its units' rows; the adds per 64 addresses, for the LDS window ----
    std::vector<uint8_t> orient((size_t)S.n_merge, 0);
    std::vector<int64_t> lo((size_t)nref, INT64_MAX), hi((size_t)nref, INT64_MIN);
    std::vector<int64_t> ulo((size_t)S.n_merge, 0), uhi((size_t)S.n_merge, 0);
    for (int64_t u = 0; u < nu; ++u) {
        if (S.ucause[u] >= 0) continue;
        const int g = S.name_id[u];
        const int64_t m = S.merge_of_unit[u];
        int bits = 0, k = 0;
        int64_t l = INT64_MAX, h = 0;
        for (int64_t r : {S.u1[u], S.upaired[u] ? S.u2[u] : (int64_t)-1}) {
            if (r < 0) continue;
            int64_t span = 0;
            for (int o = 0; o < S.n_cig[r]; ++o) {
                const uint32_t op = S.cig[S.cig_off[r] + o];
                if ((op & 15) == MH_OP_M || (op & 15) == MH_OP_D) span += op >> 4;
            }
            const int64_t pad = S.pos[r] - 1 > 0 ? S.pos[r] - 1 : 0;
            l = std::min(l, pad);
            h = std::max(h, pad + span);
            bits |= ((S.flag[r] & 0x10) ? 1 : 0) << k++;
        }
        orient[(size_t)m] = (uint8_t)bits;
        ulo[(size_t)m] = l;
        uhi[(size_t)m] = h;
        lo[g] = std::min(lo[g], l);
        hi[g] = std::max(hi[g], h);
    }
    std::vector<int64_t> base((size_t)nref + 1, 0);
    std::vector<int32_t> wlen((size_t)nref, -1);
    for (int g = 0; g < nref; ++g) {
        if (lo[g] > hi[g]) { lo[g] = 0; base[g + 1] = base[g]; continue; }
        if (hi[g] - lo[g] > S2A_CLIP_MAX_WINDOW) {
            set_error("sam2aln strand: the rows of %s span positions %lld to %lld, more than %lld",
                      S.names[g].c_str(), (long long)lo[g] + 1, (long long)hi[g],
                      (long long)S2A_CLIP_MAX_WINDOW);
            return -3;
        }
        wlen[g] = (int32_t)(hi[g] - lo[g]);
        base[g + 1] = base[g] + wlen[g] + 1;
    }
    // a plane is padded to whole 128-address groups: the flush's high halves stay inside it
    const int64_t total = (base[nref] + 127) & ~(int64_t)127;
    const int64_t planes = (int64_t)nc * STRAND_KEYS;
    // acc, and idx + cnt of the compaction, int32 each
    if ((2 * planes + nc) * total * (int64_t)sizeof(int32_t) > S2A_STRAND_MAX_BYTES) {
        set_error("sam2aln strand: %lld positions at %d q-cutoffs need more than %lld bytes of counters",
                  (long long)base[nref], nc, (long long)S2A_STRAND_MAX_BYTES);
        return -3;
    }
    // ---- the launch: the waves' expansions as the merge sized them, the rest
    // of the block's LDS for the window ----
    const int span_cap = S.info.span_cap, ops_cap = S.info.ops_cap, wave_bytes = S.info.wave_bytes;
    int wpb = STRAND_WPB;
    while (wpb > 1 && (size_t)wpb * wave_bytes + 128 * 2 * (size_t)planes > S2A_LDS_BYTES) --wpb;
    if ((size_t)wpb * wave_bytes + 128 * 2 * (size_t)planes > S2A_LDS_BYTES) {
        set_error("sam2aln strand: reference span %d too long for LDS", span_cap);
        return -3;
    }
    int64_t win = (int64_t)((S2A_LDS_BYTES - (size_t)wpb * wave_bytes) / (2 * (size_t)planes)) & ~(int64_t)127;
    if (win > total) win = total;
    // the window starts where a stretch of `win` addresses takes the most adds
    int64_t win0 = 0;
    if (win < total) {
        const int64_t nb = total >> 7, wb = win >> 7;
        std::vector<int64_t> mass((size_t)nb + 1, 0);
        for (int64_t u = 0; u < nu; ++u) {
            if (S.ucause[u] >= 0) continue;
            const int64_t m = S.merge_of_unit[u];
            const int g = S.name_id[u];
            const int64_t mid = base[g] + (ulo[(size_t)m] + uhi[(size_t)m]) / 2 - lo[g];
            mass[(size_t)(mid >> 7)] += uhi[(size_t)m] - ulo[(size_t)m];
        }
        int64_t run = 0, best = -1;
        for (int64_t x = 0; x < nb; ++x) {
            run += mass[(size_t)x];
            if (x >= wb) run -= mass[(size_t)(x - wb)];
            if (x >= wb - 1 && run > best) { best = run; win0 = (x - wb + 1) << 7; }
        }
    }
    hipStream_t s = c.stream;
    std::vector<unsigned char> order((size_t)nc), rank_of((size_t)nc);
    for (int k = 0; k < nc; ++k) order[k] = (unsigned char)k;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return S.q_cutoffs[x] < S.q_cutoffs[y]; });
    for (int k = 0; k < nc; ++k) rank_of[order[k]] = (unsigned char)k;
    if (int st = s2a_upload(S, T.d_orient, orient, s)) return st;
    if (int st = s2a_upload(S, T.d_lo, lo, s)) return st;
    if (int st = s2a_upload(S, T.d_base, base, s)) return st;
    if (int st = s2a_upload(S, T.d_wlen, wlen, s)) return st;
    if (int st = dev_reserve(S, T.d_acc, sizeof(int32_t) * (size_t)(planes * total))) return st;
    if (int st = dev_reserve(S, T.d_idx, sizeof(int32_t) * (size_t)(nc * total))) return st;
    if (int st = dev_reserve(S, T.d_cnt, sizeof(int32_t) * (size_t)(planes * total))) return st;
    // rows per (cutoff, reference), the error flag, then the cutoffs' ranks as bytes
    const size_t n_words = (size_t)nc * nref + 1;
    if (int st = dev_reserve(S, T.d_n, sizeof(int32_t) * (n_words + 2))) return st;
    MH_HIP(hipMemsetAsync(T.d_acc, 0, sizeof(int32_t) * (size_t)(planes * total), s));
    MH_HIP(hipMemsetAsync(T.d_n, 0, sizeof(int32_t) * n_words, s));
    unsigned char *d_rank = (unsigned char *)(T.d_n + n_words);
    MH_HIP(hipMemcpyAsync(d_rank, rank_of.data(), (size_t)nc, hipMemcpyHostToDevice, s));
    StrandArgs a{rows.seq, rows.qual, rows.soff, rows.pos, rows.cig_off, rows.n_cig, rows.cig,
                 S.d_units, S.d_uref, T.d_orient, S.d_res, S.n_merge, nc, {}, {}, span_cap, ops_cap,
                 wave_bytes, T.d_lo, T.d_base, T.d_wlen, total, win0, (int)win, T.d_acc,
                 T.d_n + (n_words - 1)};
    for (int k = 0; k < nc; ++k) {
        a.cut[k] = (unsigned char)(S.q_cutoffs[order[k]] + 33);
        a.entry[k] = order[k];
    }
    int64_t blocks = (S.n_merge + wpb * STRAND_UNITS_PER_WAVE - 1) / (wpb * STRAND_UNITS_PER_WAVE);
    if (blocks > STRAND_BLOCK_CAP) blocks = STRAND_BLOCK_CAP;
    const int64_t max_blocks = c.test_caps.s2a_max_blocks;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    // a 16-bit counter of a block cannot wrap: a unit adds at most 1 to it, and a
    // block of `blocks` takes at most ceil(ceil(n / wpb) / blocks) * wpb units
    while (((S.n_merge + wpb - 1) / wpb + blocks - 1) / blocks * wpb > STRAND_BLOCK_UNITS) ++blocks;
    const size_t dyn = (size_t)planes * (size_t)win * 2 + (size_t)wpb * wave_bytes;
    MH_HIP(hipFuncSetAttribute((const void *)k_s2a_strand, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)dyn));
    const int p0 = prof_begin(c, "k_s2a_strand");
    hipLaunchKernelGGL(k_s2a_strand, dim3((unsigned)blocks), dim3(64 * wpb), dyn, s, a);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    const int p1 = prof_begin(c, "k_s2a_strand_scan");
    hipLaunchKernelGGL(k_s2a_strand_scan, dim3((unsigned)nref, (unsigned)nc), dim3(1024), 0, s, T.d_base,
                       T.d_wlen, total, nc, nref, T.d_acc, T.d_idx, T.d_cnt, T.d_n, d_rank);
    prof_end(c, p1);
    MH_HIP(hipGetLastError());
    std::vector<int32_t> n_out(n_words);
    MH_HIP(hipMemcpyAsync(n_out.data(), T.d_n, sizeof(int32_t) * n_words, hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    if (n_out[n_words - 1]) {
        set_error("sam2aln strand: a position fell outside its reference's window");
        return -4;
    }
    // ---- rows: references as Python sorts str, the call's cutoffs, positions ----
    std::vector<int> names((size_t)nref);
    for (int g = 0; g < nref; ++g) names[g] = g;
    std::sort(names.begin(), names.end(), [&](int x, int y) { return S.names[x] < S.names[y]; });
    std::vector<int64_t> at((size_t)nref * nc + 1, 0);
    for (int k = 0; k < nref; ++k)
        for (int kk = 0; kk < nc; ++kk) {
            const int g = names[k], n = n_out[(size_t)kk * nref + g];
            if (n < 0 || n > wlen[g] + 1) {
                set_error("sam2aln strand: %d positions counted in a window of %d", n, wlen[g] + 1);
                return -4;
            }
            at[(size_t)k * nc + kk + 1] = at[(size_t)k * nc + kk] + n;
        }
    const size_t nrow = (size_t)at[(size_t)nref * nc];
    std::vector<int32_t> idx(nrow), cnt(STRAND_KEYS * nrow);
    for (int k = 0; k < nref; ++k)
        for (int kk = 0; kk < nc; ++kk) {
            const int g = names[k], n = n_out[(size_t)kk * nref + g];
            if (!n) continue;
            const int64_t first = at[(size_t)k * nc + kk];
            const size_t nb = sizeof(int32_t) * (size_t)n;
            MH_HIP(hipMemcpyAsync(idx.data() + first, T.d_idx + (int64_t)kk * total + base[g], nb,
                                  hipMemcpyDeviceToHost, s));
            for (int key = 0; key < STRAND_KEYS; ++key)
                MH_HIP(hipMemcpyAsync(cnt.data() + key * nrow + first,
                                      T.d_cnt + ((int64_t)kk * STRAND_KEYS + key) * total + base[g], nb,
                                      hipMemcpyDeviceToHost, s));
        }
    MH_HIP(hipStreamSynchronize(s));
    T.name.resize(nrow);
    T.qcut.resize(nrow);
    T.pos.resize(nrow);
    T.count.resize(STRAND_KEYS * nrow);
    for (int k = 0; k < nref; ++k)
        for (int kk = 0; kk < nc; ++kk)
            for (int64_t j = at[(size_t)k * nc + kk]; j < at[(size_t)k * nc + kk + 1]; ++j) {
                T.name[j] = names[k];
                T.qcut[j] = S.q_cutoffs[kk];
                T.pos[j] = lo[names[k]] + idx[j] + 1;
                for (int key = 0; key < STRAND_KEYS; ++key) T.count[STRAND_KEYS * j + key] = cnt[key * nrow + j];
            }
    T.done = true;
    return 0;
}

// strand.csv of S.strand's rows
static void s2a_strand_text(S2AState &S)
{
    S2AStrand &T = S.strand;
    if (T.text_valid) return;
    std::string &o = T.text;
    o.assign("refname,qcut,pos,A_fwd,A_rev,A_both,C_fwd,C_rev,C_both,G_fwd,G_rev,G_both,"
             "T_fwd,T_rev,T_both,del_fwd,del_rev,del_both\n");
    for (size_t j = 0; j < T.name.size(); ++j) {
        const std::string &rn = S.names[T.name[j]];
        csv_field(o, rn.data(), rn.size());
        o.push_back(',');
        o += std::to_string(T.qcut[j]);
        o.push_back(',');
        o += std::to_string((long long)T.pos[j]);
        for (int key = 0; key < STRAND_KEYS; ++key) {
            o.push_back(',');
            o += std::to_string(T.count[STRAND_KEYS * j + key]);
        }
        o.push_back('\n');
    }
    T.text_valid = true;
}

// the strand support of the context's last sam2aln call, counted now if not yet
static int s2a_strand_of(mh_ctx *ctx, const char *what, bool text, S2AState **out)
{
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("%s: no sam2aln results", what); return -3; }
    MH_HIP(hipSetDevice(c.device));
    try {
        if (int st = s2a_strand_run(c, *c.s2a)) return st;
        if (text) s2a_strand_text(*c.s2a);
    } catch (const std::exception &e) {
        c.s2a->strand.done = c.s2a->strand.text_valid = false;
        set_error("%s: out of memory (%s)", what, e.what());
        return -2;
    }
    *out = c.s2a;
    return 0;
}

// ---------------------------------------------------------------------------
// Merged insertions (conseq_ins.csv; DESIGN.md section 6, "Merged
// insertions").  Per read, walking the CIGAR with ref = POS - 1 and left = 0:
// an I op of n > 0 bytes is the insertion (seq, qual)[left, left + n) at key
// ref, the last I op of a key standing for it.  A unit's keys are the union
// of its mates'; per cutoff the string of a key is merge_inserts'
// (sam2aln.py:240-273), and a unit counts at the cutoffs whose merge entry is
// S2A_OK.
//
// k_s2a_ins_rec    one wave per listed unit (the host lists the units with an
//                  I op): the ops of each mate over the lanes, ref / left by
//                  s2a_scan, the I ops compacted into a per-mate LDS list
//                  (keys never decrease along a read, so equal keys are
//                  neighbours and the last of a run stands).  One record slot
//                  per list element: mate 1's standing elements with mate 2's
//                  partner (binary search), then mate 2's without a partner;
//                  the others stay unused (both lengths 0).  The merged bytes
//                  of a unit's records are placed by a scan of max(len1, len2).
// k_s2a_ins_merge  one wave per record, every cutoff at once: min(qual) of
//                  each mate by wave reduction, merge_pairs' (character,
//                  threshold) once per position, and per kept cutoff the
//                  bytes into the entry's slot and two position-keyed sums
//                  mixed with (reference, cutoff, key, length).
// k_s2a_ins_tab    a thread per entry into the table (table_claim), equal
//                  keys of a wave combined first.
// k_s2a_verify, k_s2a_compact and k_s2a_gather then run unchanged on the
// entries: res = (status, key, length, 0) per entry, rref per record.
// ---------------------------------------------------------------------------
struct InsRecArgs {
    const int64_t *soff;
    const int32_t *pos, *cig_off, *n_cig;
    const uint32_t *cig;
    const int64_t *units;
    const int32_t *list;      // merge units with an I op
    const int64_t *rec_off;   // per listed unit (+ end): its first record slot
    const int64_t *byte_off;  // per listed unit: its first merged byte
    int64_t n_list;
    int icap, wave_bytes;     // I ops of one read at most; LDS bytes of a wave
    S2AInsRec *rec;
};

// the I ops (n > 0) of row r into key / left / len, in op order; their number
__device__ __forceinline__ int ins_ops(const InsRecArgs &A, int64_t r, int lane, int32_t *key,
                                       int32_t *left, int32_t *len)
{
    const int nc = A.n_cig[r];
    const uint32_t *ops = A.cig + A.cig_off[r];
    int rf0 = A.pos[r] - 1, rd0 = 0, cnt = 0;
    for (int o0 = 0; o0 < nc; o0 += 64) {
        const int o = o0 + lane;
        int dref = 0, dread = 0, n = 0, isi = 0;
        if (o < nc) {
            const uint32_t op = ops[o];
            const int t = (int)(op & 15);
            n = (int)(op >> 4);
            if (t == MH_OP_M) { dref = n; dread = n; }
            else if (t == MH_OP_D) dref = n;
            else dread = n;                              // I, S (checked on the host)
            isi = t == MH_OP_I && n > 0;
        }
        const int iref = s2a_scan(dref, lane), iread = s2a_scan(dread, lane), ii = s2a_scan(isi, lane);
        const int j = cnt + ii - 1;
        if (isi && j < A.icap) {
            key[j] = rf0 + iref - dref;
            left[j] = rd0 + iread - dread;
            len[j] = n;
        }
        rf0 += __shfl(iref, 63, 64);
        rd0 += __shfl(iread, 63, 64);
        cnt += __shfl(ii, 63, 64);
    }
    return cnt < A.icap ? cnt : A.icap;
}

// the last element of the sorted key[0, n) that equals k, -1 for none
__device__ __forceinline__ int ins_find(const int32_t *key, int n, int k)
{
    int lo = 0, hi = n;                                  // first element > k
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo > 0 && key[lo - 1] == k ? lo - 1 : -1;
}

__global__ __launch_bounds__(256) void k_s2a_ins_rec(InsRecArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpb = blockDim.x >> 6;
    int32_t *wb = (int32_t *)(smem + (size_t)wv * A.wave_bytes);
    int32_t *key1 = wb, *left1 = wb + A.icap, *len1 = wb + 2 * A.icap;
    int32_t *key2 = wb + 3 * A.icap, *left2 = wb + 4 * A.icap, *len2 = wb + 5 * A.icap;
    for (int64_t i = (int64_t)blockIdx.x * wpb + wv; i < A.n_list; i += (int64_t)gridDim.x * wpb) {
        const int m = A.list[i];
        const int64_t r1 = A.units[2 * (int64_t)m], r2 = A.units[2 * (int64_t)m + 1];
        const int n1 = ins_ops(A, r1, lane, key1, left1, len1);
        const int n2 = r2 >= 0 ? ins_ops(A, r2, lane, key2, left2, len2) : 0;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int64_t s1 = A.soff[r1], s2 = r2 >= 0 ? A.soff[r2] : 0;
        const int64_t rec0 = A.rec_off[i];
        // the host counted the same I ops: never more slots than it reserved
        int nslot = (int)(A.rec_off[i + 1] - rec0);
        if (nslot > n1 + n2) nslot = n1 + n2;
        int64_t bytes = A.byte_off[i];
        for (int j0 = 0; j0 < nslot; j0 += 64) {
            const int j = j0 + lane;
            S2AInsRec R{m, 0, 0, 0, 0, 0, 0};
            if (j < n1) {
                if (j + 1 >= n1 || key1[j + 1] != key1[j]) {
                    R.key = key1[j];
                    R.len1 = len1[j];
                    R.src1 = s1 + left1[j];
                    const int p = ins_find(key2, n2, R.key);
                    if (p >= 0) { R.len2 = len2[p]; R.src2 = s2 + left2[p]; }
                }
            } else if (j < nslot) {
                const int t = j - n1;
                if ((t + 1 >= n2 || key2[t + 1] != key2[t]) && ins_find(key1, n1, key2[t]) < 0) {
                    R.key = key2[t];
                    R.len2 = len2[t];
                    R.src2 = s2 + left2[t];
                }
            }
            const int L = R.len1 > R.len2 ? R.len1 : R.len2;
            const int run = s2a_scan(L, lane);
            R.boff = bytes + run - L;
            if (j < nslot) A.rec[rec0 + j] = R;
            bytes += __shfl(run, 63, 64);
        }
        // slots past the I ops found (none, unless the host's count differs)
        for (int64_t j = rec0 + nslot + lane; j < A.rec_off[i + 1]; j += 64)
            A.rec[j] = S2AInsRec{m, 0, 0, 0, 0, 0, 0};
        __builtin_amdgcn_wave_barrier();
    }
}

struct InsMergeArgs {
    const uint8_t *seq, *qual;
    const S2AInsRec *rec;
    int64_t n_rec;
    int n_cut;
    unsigned char cut[S2A_MAX_CUTS];
    const int32_t *mres;      // the merge's res: 4 per (unit, cutoff)
    const int32_t *uref;
    uint8_t *out;
    int32_t *res;             // 4 per entry: status, key, length, 0
    int32_t *rref;            // per record: its reference
    int64_t *slot;            // per entry: its bytes in out
    uint64_t *h;              // 2 per entry
    int32_t *ctr;             // [2]: the least unit with a '-' among its inserted bytes
};

constexpr int S2A_INS_SKIP = -1;   // status of an entry that is no row

template <int NC>
__global__ __launch_bounds__(256) void k_s2a_ins_merge(InsMergeArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int n_cut = NC == 1 ? 1 : A.n_cut;
    unsigned char cut[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) cut[k] = A.cut[k];
    for (int64_t r = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); r < A.n_rec;
         r += (int64_t)gridDim.x * wpb) {
        const S2AInsRec R = A.rec[r];
        const int64_t e0 = r * n_cut;
        const int L = R.len1 > R.len2 ? R.len1 : R.len2;
        // ---- min(qual) of each mate's insertion; a '-' is refused ----
        int min1 = 256, min2 = 256, dash = 0;
        for (int j = lane; j < R.len1; j += 64) {
            min1 = min(min1, (int)A.qual[R.src1 + j]);
            dash |= A.seq[R.src1 + j] == '-';
        }
        for (int j = lane; j < R.len2; j += 64) {
            min2 = min(min2, (int)A.qual[R.src2 + j]);
            dash |= A.seq[R.src2 + j] == '-';
        }
        for (int o = 32; o > 0; o >>= 1) {
            min1 = min(min1, __shfl_xor(min1, o, 64));
            min2 = min(min2, __shfl_xor(min2, o, 64));
        }
        const bool refused = __any(dash);
        if (refused && lane == 0) atomicMin(&A.ctr[2], R.unit);
        // ---- merge_pairs' roles: seq1 = a is the shorter string, mate 1 on a tie ----
        const bool swap = R.len1 > R.len2;
        const int64_t sa = swap ? R.src2 : R.src1, sb = swap ? R.src1 : R.src2;
        const int la = swap ? R.len2 : R.len1;
        // per cutoff: 0 no row, 1 mate 1's string alone, 2 the merged string
        int mode[NC], elen[NC];
        int64_t slot[NC];
        uint64_t h1[NC], h2[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            mode[k] = 0;
            if (k < n_cut && L > 0 && !refused &&
                A.mres[4 * ((int64_t)R.unit * n_cut + k)] == S2A_OK) {
                if (R.len2 > 0 && min2 > (int)cut[k]) mode[k] = 2;
                else if (R.len1 > 0 && min1 > (int)cut[k]) mode[k] = 1;
            }
            elen[k] = mode[k] == 2 ? L : mode[k] == 1 ? R.len1 : 0;
            slot[k] = (int64_t)n_cut * R.boff + (int64_t)k * L;
            h1[k] = h2[k] = 0;
        }
        for (int j = lane; j < L; j += 64) {
            char ch = 0, c1 = 0;
            unsigned char thr = S2A_ALWAYS;
            if (R.len2 > 0) {                            // (ch, thr) as in s2a_pos, no gaps
                ch = (char)A.seq[sb + j];
                thr = A.qual[sb + j];
                if (j < la) {
                    const char ca = (char)A.seq[sa + j];
                    const unsigned char qa = A.qual[sa + j];
                    if (ca == ch) {
                        thr = qa > thr ? qa : thr;
                    } else {
                        const int dq = (int)thr - (int)qa;
                        if (dq <= -5) { ch = ca; thr = qa; }
                        else if (dq < 5) { ch = 'N'; thr = S2A_ALWAYS; }
                    }
                }
            }
            if (j < R.len1) c1 = (char)A.seq[R.src1 + j];
            const uint64_t k1 = mix64(2ull * (uint64_t)j + 1ull) | 1ull;
            const uint64_t k2 = mix64((uint64_t)j ^ 0x5bd1e995ull << 32) | 1ull;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                if (j < elen[k]) {
                    const char mch = mode[k] == 2 ? (thr > cut[k] ? ch : 'N') : c1;
                    A.out[slot[k] + j] = (uint8_t)mch;
                    h1[k] += k1 * (uint64_t)(uint8_t)mch;
                    h2[k] += k2 * (uint64_t)(uint8_t)mch;
                }
            }
        }
        const int ref = A.uref[R.unit];
        if (lane == 0) A.rref[r] = ref;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (k >= n_cut) break;
            for (int o = 32; o > 0; o >>= 1) {
                h1[k] += __shfl_xor(h1[k], o, 64);
                h2[k] += __shfl_xor(h2[k], o, 64);
            }
            const uint64_t grp = (uint64_t)(uint32_t)ref * (uint64_t)n_cut + (uint64_t)k;
            const uint64_t meta = mix64(grp) ^ ((uint64_t)(uint32_t)R.key << 32) ^
                                  (uint64_t)(uint32_t)elen[k];
            h1[k] = mix64(h1[k] ^ mix64(meta));
            h2[k] = mix64(h2[k] + 0x2545f4914f6cdd1dull * mix64(meta + 7));
            if (lane == 0) {
                const int64_t e = e0 + k;
                A.res[4 * e] = mode[k] ? S2A_OK : S2A_INS_SKIP;
                A.res[4 * e + 1] = R.key;
                A.res[4 * e + 2] = elen[k];
                A.res[4 * e + 3] = 0;
                A.slot[e] = slot[k];
                A.h[2 * e] = h1[k];
                A.h[2 * e + 1] = h2[k];
            }
        }
    }
}

// A thread per entry.  An amplicon puts most of a wave's entries on one
// (position, string), and atomics on one address serialise: for
// INS_COMBINE rounds the lanes that hold the lowest active lane's key are
// counted by a ballot and that lane alone goes to the table (entries rise
// with the lane, so it is also the least of them); what is left goes lane by
// lane.  combine 0: every entry on its own (measurements).
constexpr int INS_COMBINE = 4;

__global__ __launch_bounds__(256) void k_s2a_ins_tab(const int32_t *res, const uint64_t *h, int64_t n,
                                                     uint64_t *tkey, int32_t *tcnt, int32_t *trep,
                                                     uint64_t mask, int combine, int key_bits)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key = 0;
    bool todo = false;
    if (e < n && res[4 * e] == S2A_OK) { key = s2a_key(h[2 * e], key_bits); todo = true; }
    for (int round = 0; combine && round < INS_COMBINE; ++round) {
        const unsigned long long act = __ballot(todo);
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const uint64_t k = __shfl((unsigned long long)key, leader, 64);
        const bool mine = todo && key == k;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) {
            const uint64_t s = table_claim(tkey, mask, key & mask, key).slot;
            atomicAdd(&tcnt[s], (int32_t)__popcll(same));
            atomicMin(&trep[s], (int32_t)e);
        }
        todo = todo && !mine;
    }
    if (todo) {
        const uint64_t s = table_claim(tkey, mask, key & mask, key).slot;
        atomicAdd(&tcnt[s], 1);
        atomicMin(&trep[s], (int32_t)e);
    }
}

static void s2a_ins_clear(S2AIns &I)
{
    I.done = I.text_valid = false;
    I.name.clear(); I.cut.clear(); I.count.clear(); I.pos.clear(); I.soff.assign(1, 0);
    I.strings.clear();
    I.t_name.clear(); I.t_cut.clear(); I.t_count.clear(); I.t_pos.clear();
}

int s2a_ins_run(Ctx &c, S2AState &S)
{
    S2AIns &I = S.ins;
    if (I.done) return 0;
    if (S.clip.state == CLIP_NONE) {
        set_error("sam2aln conseq_ins: no rows of a sam2aln call are on the device");
        return -3;
    }
    const S2ADevRows &rows = S.clip.rows;
    if (S.n_merge && rows.cig != S.d_cig && (!c.map.valid || rows.cig != c.map.pool)) {
        set_error("sam2aln conseq_ins: the mapping pass the rows came from is gone");
        return -3;
    }
    if (S.n_merge && rows.soff != S.d_soff && (rows.soff != c.reads.off || S.staged_reads != c.reads.n)) {
        set_error("sam2aln conseq_ins: the resident reads the rows came from are gone");
        return -3;
    }
    s2a_ins_clear(I);
    const int nc = (int)S.q_cutoffs.size();
    const int64_t nu = (int64_t)S.u1.size();
    // ---- the units with an I op, their record slots (one per I op) and
    // merged bytes (the I ops' lengths: at least the sum of max(len1, len2)) ----
    std::vector<int32_t> list;
    std::vector<int64_t> list_unit, rec_off(1, 0), byte_off(1, 0);
    int icap = 1;
    for (int64_t u = 0; S.n_merge && u < nu; ++u) {
        if (S.ucause[u] >= 0) continue;
        int64_t nrec = 0, nbytes = 0;
        for (int64_t r : {S.u1[u], S.upaired[u] ? S.u2[u] : (int64_t)-1}) {
            if (r < 0) continue;
            int ni = 0;
            for (int o = 0; o < S.n_cig[r]; ++o) {
                const uint32_t op = S.cig[S.cig_off[r] + o];
                if ((op & 15) == MH_OP_I && (op >> 4) > 0) { ++ni; nbytes += op >> 4; }
            }
            icap = std::max(icap, ni);
            nrec += ni;
        }
        if (!nrec) continue;
        list.push_back((int32_t)S.merge_of_unit[u]);
        list_unit.push_back(u);
        rec_off.push_back(rec_off.back() + nrec);
        byte_off.push_back(byte_off.back() + nbytes);
    }
    const int64_t nl = (int64_t)list.size(), nrec = rec_off.back(), ne = nrec * nc;
    const int64_t nbytes = byte_off.back() * nc;
    if (nl == 0) { I.done = true; return 0; }
    if (ne > 0x7f7f7f7f) {               // entries are int32 in the table and in uniq
        set_error("sam2aln conseq_ins: %lld insertions at %d q-cutoffs are too many entries",
                  (long long)nrec, nc);
        return -3;
    }
    const int wave_bytes = (6 * 4 * icap + 15) & ~15;
    int wpb = 4;
    while (wpb > 1 && (size_t)wpb * wave_bytes > 64 * 1024) --wpb;
    if ((size_t)wave_bytes > 160 * 1024) {
        set_error("sam2aln conseq_ins: a read with %d insertions is too many for LDS", icap);
        return -3;
    }
    hipStream_t s = c.stream;
    if (int st = s2a_upload(S, I.d_list, list, s)) return st;
    if (int st = s2a_upload(S, I.d_recoff, rec_off, s)) return st;
    if (int st = s2a_upload(S, I.d_byteoff, byte_off, s)) return st;
    uint64_t tsize = 1024;
    while (tsize < (uint64_t)(2 * ne)) tsize <<= 1;
    if (int st = dev_reserve(S, I.d_rec, sizeof(S2AInsRec) * (size_t)nrec)) return st;
    if (int st = dev_reserve(S, I.d_rref, sizeof(int32_t) * (size_t)nrec)) return st;
    if (int st = dev_reserve(S, I.d_out, (size_t)nbytes)) return st;
    if (int st = dev_reserve(S, I.d_res, sizeof(int32_t) * 4 * (size_t)ne)) return st;
    if (int st = dev_reserve(S, I.d_slot, sizeof(int64_t) * (size_t)ne)) return st;
    if (int st = dev_reserve(S, I.d_h, sizeof(uint64_t) * 2 * (size_t)ne)) return st;
    if (int st = dev_reserve(S, I.d_ctr, sizeof(int32_t) * 4)) return st;
    if (int st = dev_reserve(S, I.d_tkey, sizeof(uint64_t) * tsize)) return st;
    if (int st = dev_reserve(S, I.d_tcnt, sizeof(int32_t) * tsize)) return st;
    if (int st = dev_reserve(S, I.d_trep, sizeof(int32_t) * tsize)) return st;
    if (int st = dev_reserve(S, I.d_uniq, sizeof(int32_t) * 2 * (size_t)ne)) return st;
    static const int32_t ctr0[4] = {0, 0, INT32_MAX, 0};
    MH_HIP(hipMemcpyAsync(I.d_ctr, ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    MH_HIP(hipMemsetAsync(I.d_tkey, 0, sizeof(uint64_t) * tsize, s));
    MH_HIP(hipMemsetAsync(I.d_tcnt, 0, sizeof(int32_t) * tsize, s));
    MH_HIP(hipMemsetAsync(I.d_trep, 0x7f, sizeof(int32_t) * tsize, s));

    InsRecArgs ra{rows.soff, rows.pos, rows.cig_off, rows.n_cig, rows.cig, S.d_units, I.d_list,
                  I.d_recoff, I.d_byteoff, nl, icap, wave_bytes, I.d_rec};
    int64_t rb = (nl + wpb - 1) / wpb;
    if (rb > 256 * 64) rb = 256 * 64;
    MH_HIP(hipFuncSetAttribute((const void *)k_s2a_ins_rec, hipFuncAttributeMaxDynamicSharedMemorySize,
                               wpb * wave_bytes));
    const int p0 = prof_begin(c, "k_s2a_ins_rec");
    hipLaunchKernelGGL(k_s2a_ins_rec, dim3((unsigned)rb), dim3(64 * wpb), wpb * wave_bytes, s, ra);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    InsMergeArgs ma{rows.seq, rows.qual, I.d_rec, nrec, nc, {}, S.d_res, S.d_uref, I.d_out, I.d_res,
                    I.d_rref, I.d_slot, I.d_h, I.d_ctr};
    for (int k = 0; k < nc; ++k) ma.cut[k] = (unsigned char)(S.q_cutoffs[k] + 33);
    void (*merge)(InsMergeArgs) = nc == 1 ? k_s2a_ins_merge<1> : nc == 2 ? k_s2a_ins_merge<2>
                                  : nc <= 4 ? k_s2a_ins_merge<4> : k_s2a_ins_merge<8>;
    int64_t mb = (nrec + 3) / 4;
    if (mb > 256 * 64) mb = 256 * 64;
    const int p1 = prof_begin(c, "k_s2a_ins_merge");
    hipLaunchKernelGGL(merge, dim3((unsigned)mb), dim3(256), 0, s, ma);
    prof_end(c, p1);
    MH_HIP(hipGetLastError());
    static const bool combine = !(getenv("MICALL_INS_COMBINE") && *getenv("MICALL_INS_COMBINE") == '0');
    const int64_t tb = (ne + 255) / 256;     // a thread per entry: ne <= 0x7f7f7f7f
    const int key_bits = c.test_caps.s2a_key_bits;   // mh_test_set_sam2aln; 64 in the product
    const int p2 = prof_begin(c, "k_s2a_ins_tab");
    hipLaunchKernelGGL(k_s2a_ins_tab, dim3((unsigned)tb), dim3(256), 0, s, I.d_res, I.d_h, ne, I.d_tkey,
                       I.d_tcnt, I.d_trep, tsize - 1, combine ? 1 : 0, key_bits);
    prof_end(c, p2);
    MH_HIP(hipGetLastError());
    int64_t vb = (ne + 3) / 4;
    if (vb > 256 * 64) vb = 256 * 64;
    const int p3 = prof_begin(c, "k_s2a_ins_group");
    hipLaunchKernelGGL(k_s2a_verify, dim3((unsigned)vb), dim3(256), 0, s, I.d_res, I.d_h, I.d_rref,
                       I.d_slot, I.d_out, ne, nc, I.d_tkey, I.d_trep, tsize - 1, I.d_ctr, key_bits);
    int64_t cb = (int64_t)((tsize + 255) / 256);
    if (cb > 65536) cb = 65536;
    hipLaunchKernelGGL(k_s2a_compact, dim3((unsigned)cb), dim3(256), 0, s, I.d_tkey, I.d_tcnt, I.d_trep,
                       tsize, I.d_uniq, I.d_ctr);
    prof_end(c, p3);
    MH_HIP(hipGetLastError());
    int32_t ctr[4];
    MH_HIP(hipMemcpyAsync(ctr, I.d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    prof_flush(c);
    if (ctr[2] != INT32_MAX) {
        int64_t u = -1;
        for (int64_t k = 0; k < nl; ++k)
            if (list[k] == ctr[2]) u = list_unit[k];
        const int64_t r = u >= 0 ? S.u1[u] : -1;
        set_error("sam2aln conseq_ins: read %.*s has a '-' among its inserted bases",
                  r >= 0 ? (int)S.qlen[r] : 1, r >= 0 ? S.qpool.data() + S.qoff[r] : "?");
        return -3;
    }
    if (ctr[0]) {
        set_error("sam2aln conseq_ins: insertion hash collision (distinct insertions share a key)");
        return -4;
    }
    const int64_t nq = ctr[1];
    if (nq < 0 || nq > ne) {
        set_error("sam2aln conseq_ins: %lld distinct insertions of %lld entries", (long long)nq, (long long)ne);
        return -4;
    }
    if (nq == 0) { I.done = true; return 0; }
    std::vector<int32_t> uniq(2 * (size_t)nq), res(4 * (size_t)ne), rref((size_t)nrec);
    MH_HIP(hipMemcpyAsync(uniq.data(), I.d_uniq, sizeof(int32_t) * uniq.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(res.data(), I.d_res, sizeof(int32_t) * res.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(rref.data(), I.d_rref, sizeof(int32_t) * rref.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> goff((size_t)nq + 1, 0);
    for (int64_t k = 0; k < nq; ++k) {
        const int64_t e = uniq[2 * k];
        if (e < 0 || e >= ne || res[4 * e] != S2A_OK || res[4 * e + 2] <= 0) {
            set_error("sam2aln conseq_ins: distinct insertion %lld names no entry", (long long)k);
            return -4;
        }
        goff[k + 1] = goff[k] + res[4 * e + 2];
    }
    std::string bytes((size_t)goff[nq], '\0');
    if (int st = s2a_upload(S, I.d_goff, goff, s)) return st;
    if (int st = dev_reserve(S, I.d_gather, bytes.size())) return st;
    int64_t gb = (nq + 3) / 4;
    if (gb > 256 * 64) gb = 256 * 64;
    hipLaunchKernelGGL(k_s2a_gather, dim3((unsigned)gb), dim3(256), 0, s, I.d_uniq, I.d_goff, I.d_res,
                       I.d_slot, I.d_out, nq, I.d_gather);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&bytes[0], I.d_gather, bytes.size(), hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    // ---- file order: references as Python sorts str, cutoff, position,
    // count descending, string as bytes ----
    std::vector<int64_t> order((size_t)nq);
    for (int64_t k = 0; k < nq; ++k) order[k] = k;
    auto name_of = [&](int64_t k) -> const std::string & { return S.names[rref[uniq[2 * k] / nc]]; };
    auto str_of = [&](int64_t k) {
        return std::string_view(bytes.data() + goff[k], (size_t)(goff[k + 1] - goff[k]));
    };
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const int64_t ex = uniq[2 * x], ey = uniq[2 * y];
        if (const int d = name_of(x).compare(name_of(y))) return d < 0;
        const int qx = S.q_cutoffs[ex % nc], qy = S.q_cutoffs[ey % nc];
        if (qx != qy) return qx < qy;
        if (res[4 * ex + 1] != res[4 * ey + 1]) return res[4 * ex + 1] < res[4 * ey + 1];
        if (uniq[2 * x + 1] != uniq[2 * y + 1]) return uniq[2 * x + 1] > uniq[2 * y + 1];
        return str_of(x) < str_of(y);
    });
    for (int64_t k : order) {
        const int64_t e = uniq[2 * k];
        I.name.push_back(rref[e / nc]);
        I.cut.push_back((int32_t)(e % nc));
        I.pos.push_back(res[4 * e + 1]);
        I.count.push_back(uniq[2 * k + 1]);
        I.strings.append(str_of(k));
        I.soff.push_back((int64_t)I.strings.size());
        if (!I.t_name.empty() && I.t_name.back() == I.name.back() && I.t_cut.back() == I.cut.back() &&
            I.t_pos.back() == I.pos.back()) {
            I.t_count.back() += I.count.back();
        } else {
            I.t_name.push_back(I.name.back());
            I.t_cut.push_back(I.cut.back());
            I.t_pos.push_back(I.pos.back());
            I.t_count.push_back(I.count.back());
        }
    }
    I.done = true;
    return 0;
}

// conseq_ins.csv of S.ins's rows: refname,qcut,pos,insert,count
static void s2a_ins_text(S2AState &S)
{
    S2AIns &I = S.ins;
    if (I.text_valid) return;
    std::string &o = I.text;
    o.assign("refname,qcut,pos,insert,count\n");
    for (size_t j = 0; j < I.name.size(); ++j) {
        const std::string &rn = S.names[I.name[j]];
        csv_field(o, rn.data(), rn.size());
        o.push_back(',');
        o += std::to_string(S.q_cutoffs[I.cut[j]]);
        o.push_back(',');
        o += std::to_string((long long)I.pos[j]);
        o.push_back(',');
        csv_field(o, I.strings.data() + I.soff[j], (size_t)(I.soff[j + 1] - I.soff[j]));
        o.push_back(',');
        o += std::to_string(I.count[j]);
        o.push_back('\n');
    }
    I.text_valid = true;
}

// the insertions of the context's last sam2aln call, counted now if not yet
static int s2a_ins_of(mh_ctx *ctx, const char *what, bool text, S2AState **out)
{
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("%s: no sam2aln results", what); return -3; }
    MH_HIP(hipSetDevice(c.device));
    try {
        if (int st = s2a_ins_run(c, *c.s2a)) return st;
        if (text) s2a_ins_text(*c.s2a);
    } catch (const std::exception &e) {
        c.s2a->ins.done = c.s2a->ins.text_valid = false;
        set_error("%s: out of memory (%s)", what, e.what());
        return -2;
    }
    *out = c.s2a;
    return 0;
}

}  // namespace mh

using namespace mh;

// the list of q-cutoffs of a call: 1..S2A_MAX_CUTS distinct values in 0..93
static int s2a_check_cutoffs(int n_cut, const int32_t *q_cutoffs)
{
    if (n_cut < 1 || n_cut > S2A_MAX_CUTS || !q_cutoffs) {
        set_error("sam2aln: %d q-cutoffs (1..%d are supported)", n_cut, S2A_MAX_CUTS);
        return -3;
    }
    for (int k = 0; k < n_cut; ++k) {
        if (q_cutoffs[k] < 0 || q_cutoffs[k] > 93) {
            set_error("sam2aln: q-cutoff %d outside 0..93", (int)q_cutoffs[k]);
            return -3;
        }
        for (int j = 0; j < k; ++j)
            if (q_cutoffs[j] == q_cutoffs[k]) {
                set_error("sam2aln: q-cutoff %d given twice", (int)q_cutoffs[k]);
                return -3;
            }
    }
    return 0;
}

extern "C" int mh_sam2aln_csv_q(mh_ctx *ctx, const char *text, int64_t len, int n_cut,
                                const int32_t *q_cutoffs, double max_prop_n, int64_t *n_units)
{
    if (!ctx || (!text && len) || len < 0) return -3;
    if (int st = s2a_check_cutoffs(n_cut, q_cutoffs)) return st;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.s2a) c.s2a = new S2AState();
    S2AState &S = *c.s2a;
    S.q_cutoffs.assign(q_cutoffs, q_cutoffs + n_cut);
    s2a_begin(c, S);
    S.staged_reads = -1;
    auto t0 = std::chrono::steady_clock::now();
    int pst = 0;
    try {
        pst = s2a_parse(S, text ? text : "", len);
    } catch (const std::exception &e) {
        set_error("remap csv: out of memory (%s)", e.what());
        pst = -2;
    }
    if (pst) {
        S.u1.clear();
        return pst;
    }
    auto t1 = std::chrono::steady_clock::now();
    if (int st = s2a_run(c, S, max_prop_n)) {
        S.u1.clear();
        return st;
    }
    auto t2 = std::chrono::steady_clock::now();
    S.t_parse = std::chrono::duration<double, std::milli>(t1 - t0).count();
    S.t_device = std::chrono::duration<double, std::milli>(t2 - t1).count();
    S.complete = true;
    if (n_units) *n_units = (int64_t)S.u1.size();
    return 0;
}

extern "C" int mh_sam2aln_csv(mh_ctx *ctx, const char *text, int64_t len, int q_cutoff,
                              double max_prop_n, int64_t *n_units)
{
    const int32_t q = q_cutoff;
    return mh_sam2aln_csv_q(ctx, text, len, 1, &q, max_prop_n, n_units);
}

// the row arrays of every resident read from the records of the last mapping
// pass (k_s2a_stage), their host copies in S and in sam_ref / span_ins
static int s2a_stage(Ctx &c, S2AState &S, std::vector<int32_t> &sam_ref, std::vector<int32_t> &span_ins)
{
    hipStream_t s = c.stream;
    const DevReads &R = c.reads;
    const int64_t n = R.n;
    const size_t rows = sizeof(int32_t) * (size_t)(n > 0 ? n : 1);
    S.staged_reads = -1;
    if (int st = dev_reserve(S, S.d_seq, (size_t)R.total_bases + 64)) return st;
    if (int st = dev_reserve(S, S.d_qual, (size_t)R.total_bases + 64)) return st;
    if (int st = dev_reserve(S, S.d_pos, rows)) return st;
    if (int st = dev_reserve(S, S.d_cigoff, rows)) return st;
    if (int st = dev_reserve(S, S.d_ncig, rows)) return st;
    if (int st = dev_reserve(S, S.d_flag, rows)) return st;
    if (int st = dev_reserve(S, S.d_samref, rows)) return st;
    if (int st = dev_reserve(S, S.d_spanins, rows)) return st;
    S.n_rows = n;
    S.pos.resize(n); S.cig_off.resize(n); S.n_cig.resize(n); S.flag.resize(n);
    sam_ref.resize(n); span_ins.resize(n);
    const int64_t used = c.map.last_cigar < c.map.pool_cap ? c.map.last_cigar : c.map.pool_cap;
    S.cig.resize(used > 0 ? (size_t)used : 0);
    if (n == 0) return 0;
    StageArgs a{R, c.map.rec, c.map.pool, S.d_seq, S.d_qual, S.d_pos, S.d_cigoff, S.d_ncig,
                S.d_flag, S.d_samref, S.d_spanins};
    int64_t blocks = (n + 15) / 16;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    const int p0 = prof_begin(c, "k_s2a_stage");
    hipLaunchKernelGGL(k_s2a_stage, dim3((unsigned)blocks), dim3(256), 0, s, a);
    prof_end(c, p0);
    MH_HIP(hipGetLastError());
    const size_t nb = sizeof(int32_t) * (size_t)n;
    MH_HIP(hipMemcpyAsync(S.pos.data(), S.d_pos, nb, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(S.cig_off.data(), S.d_cigoff, nb, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(S.n_cig.data(), S.d_ncig, nb, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(S.flag.data(), S.d_flag, nb, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(sam_ref.data(), S.d_samref, nb, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(span_ins.data(), S.d_spanins, nb, hipMemcpyDeviceToHost, s));
    if (used > 0)
        MH_HIP(hipMemcpyAsync(S.cig.data(), c.map.pool, sizeof(uint32_t) * (size_t)used,
                              hipMemcpyDeviceToHost, s));
    MH_HIP(hipStreamSynchronize(s));
    S.staged_reads = n;
    return 0;
}

extern "C" int mh_sam2aln_resident(mh_ctx *ctx, int n_refs, const char *const *refnames, int n_cut,
                                   const int32_t *q_cutoffs, double max_prop_n, int64_t *n_units)
{
    if (!ctx || n_refs < 0 || (n_refs > 0 && !refnames)) return -3;
    if (int st = s2a_check_cutoffs(n_cut, q_cutoffs)) return st;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.map.valid || c.map.n_reads != c.reads.n) {
        set_error("mh_sam2aln_resident: no mapping pass is resident (call mh_map)");
        return -3;
    }
    if ((int64_t)c.names.size() != c.reads.n) {
        set_error("mh_sam2aln_resident: no read names are resident");
        return -3;
    }
    if (n_refs != c.map.n_refs) {
        set_error("mh_sam2aln_resident: %d reference names for a pass over %d references", n_refs,
                  c.map.n_refs);
        return -3;
    }
    if (!c.s2a) c.s2a = new S2AState();
    S2AState &S = *c.s2a;
    S.q_cutoffs.assign(q_cutoffs, q_cutoffs + n_cut);
    s2a_begin(c, S);
    S.u1.clear();
    std::vector<int32_t> sam_ref, span_ins;
    int st = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto t1 = t0, t2 = t0;
    try {
        st = s2a_stage(c, S, sam_ref, span_ins);
        t1 = std::chrono::steady_clock::now();
        if (!st) st = s2a_units_resident(c, S, n_refs, refnames, sam_ref, span_ins);
        t2 = std::chrono::steady_clock::now();
        if (!st) {
            const S2ADevRows dev{S.d_seq, S.d_qual, c.reads.off, S.d_pos, S.d_cigoff, S.d_ncig,
                                 c.map.pool, span_ins.data()};
            st = s2a_run(c, S, max_prop_n, &dev);
        }
    } catch (const std::exception &e) {
        set_error("mh_sam2aln_resident: out of memory (%s)", e.what());
        st = -2;
    }
    if (st) {
        S.u1.clear();
        return st;
    }
    const auto t3 = std::chrono::steady_clock::now();
    S.t_parse = std::chrono::duration<double, std::milli>(t2 - t1).count();
    S.t_device = std::chrono::duration<double, std::milli>((t1 - t0) + (t3 - t2)).count();
    S.complete = true;
    if (n_units) *n_units = (int64_t)S.u1.size();
    return 0;
}

extern "C" int mh_sam2aln_resident_rows(mh_ctx *ctx, int64_t first, int64_t n, int32_t *len,
                                        uint8_t *seq, uint8_t *qual, size_t cap, size_t *used)
{
    if (!ctx || !used || first < 0 || n < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    MH_HIP(hipSetDevice(c.device));
    if (!c.s2a || c.s2a->staged_reads < 0 || c.s2a->staged_reads != c.reads.n) {
        set_error("mh_sam2aln_resident_rows: no rows staged by mh_sam2aln_resident");
        return -3;
    }
    if (first + n > c.reads.n) { set_error("mh_sam2aln_resident_rows: row range out of bounds"); return -3; }
    const S2AState &S = *c.s2a;
    std::vector<int64_t> off((size_t)n);
    std::vector<int32_t> ln((size_t)n);
    if (n > 0) {
        MH_HIP(copy_sync(c, off.data(), c.reads.off + first, sizeof(int64_t) * (size_t)n,
                         hipMemcpyDeviceToHost));
        MH_HIP(copy_sync(c, ln.data(), c.reads.len + first, sizeof(int32_t) * (size_t)n,
                         hipMemcpyDeviceToHost));
    }
    size_t total = 0;
    for (int64_t k = 0; k < n; ++k) total += (size_t)ln[k];
    *used = total;
    if (!seq || !qual || !len) return 0;
    if (cap < total) { set_error("mh_sam2aln_resident_rows: buffer too small"); return -2; }
    if (n == 0) return 0;
    const int64_t lo = off[0], hi = off[n - 1] + ln[n - 1];
    std::vector<uint8_t> hs((size_t)(hi - lo) + 1), hq((size_t)(hi - lo) + 1);
    if (hi > lo) {
        MH_HIP(copy_sync(c, hs.data(), S.d_seq + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
        MH_HIP(copy_sync(c, hq.data(), S.d_qual + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
    }
    size_t at = 0;
    for (int64_t k = 0; k < n; ++k) {
        len[k] = ln[k];
        memcpy(seq + at, hs.data() + (off[k] - lo), (size_t)ln[k]);
        memcpy(qual + at, hq.data() + (off[k] - lo), (size_t)ln[k]);
        at += (size_t)ln[k];
    }
    return 0;
}

extern "C" int mh_sam2aln_file_q(mh_ctx *ctx, int fd, int n_cut, const int32_t *q_cutoffs,
                                 double max_prop_n, int64_t *n_units)
{
    if (!ctx || fd < 0) return -3;
    if (int st = s2a_check_cutoffs(n_cut, q_cutoffs)) return st;
    const char *text = nullptr;
    size_t len = 0;
    if (int st = map_text_file(fd, &text, &len)) return st;
    const int rc = mh_sam2aln_csv_q(ctx, text, (int64_t)len, n_cut, q_cutoffs, max_prop_n, n_units);
    unmap_text_file(text, len);
    return rc;
}

extern "C" int mh_sam2aln_file(mh_ctx *ctx, int fd, int q_cutoff, double max_prop_n, int64_t *n_units)
{
    const int32_t q = q_cutoff;
    return mh_sam2aln_file_q(ctx, fd, 1, &q, max_prop_n, n_units);
}

extern "C" int mh_sam2aln_write(mh_ctx *ctx, int which, int fd, int64_t offset, int64_t *written)
{
    if (!ctx || which < 0 || which > 2 || fd < 0 || offset < 0) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("mh_sam2aln_write: no sam2aln results"); return -3; }
    if (!(c.s2a->out_valid & (1 << which))) {
        // not formatted yet (no size query before): formatted and written
        // together, the writes overlapping the formatting
        S2AState &S = *c.s2a;
        auto t0 = std::chrono::steady_clock::now();
        int err = 0;
        int64_t n = 0;
        uint32_t crc = 0;
        if (which == 0) S.wr_bytes = -1;
        try {
            err = s2a_format_write(S, which, fd, offset, &n, which == 0 ? &crc : nullptr);
        } catch (const std::exception &e) {
            set_error("mh_sam2aln_write: out of memory (%s)", e.what());
            return -2;
        }
        S.t_format[which] = std::chrono::duration<double, std::milli>(
                                std::chrono::steady_clock::now() - t0).count();
        if (err) { set_error("mh_sam2aln_write: write failed (%s)", strerror(err)); return -4; }
        if (written) *written = n;
        if (which == 0) { S.wr_crc = crc; S.wr_bytes = n; }
        return 0;
    }
    size_t used = 0;
    if (int st = mh_sam2aln_output(ctx, which, nullptr, 0, &used)) return st;
    S2AState &S = *ctx_of(ctx)->s2a;
    int64_t pos = offset;
    uint32_t crc = 0;
    if (which == 0) S.wr_bytes = -1;
    for (const std::string &piece : S.out_cache[which]) {
        if (const int e = write_all_at(fd, piece.data(), piece.size(), pos)) {
            set_error("mh_sam2aln_write: write failed (%s)", strerror(e));
            return -4;
        }
        if (which == 0) crc = crc32_join(crc, crc32_update(0, piece.data(), piece.size()), (int64_t)piece.size());
        pos += (int64_t)piece.size();
    }
    if (written) *written = pos - offset;
    if (which == 0) { S.wr_crc = crc; S.wr_bytes = pos - offset; }
    std::vector<std::string>().swap(S.out_cache[which]);
    S.out_valid &= ~(1 << which);
    return 0;
}

extern "C" int mh_sam2aln_written(mh_ctx *ctx, int which, uint32_t *crc, int64_t *bytes)
{
    if (!ctx || which != 0 || !crc || !bytes) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a || c.s2a->wr_bytes < 0) {
        set_error("mh_sam2aln_written: aligned.csv was not written by mh_sam2aln_write");
        return -3;
    }
    *crc = c.s2a->wr_crc;
    *bytes = c.s2a->wr_bytes;
    return 0;
}

extern "C" int mh_sam2aln_serial(mh_ctx *ctx, int64_t *serial)
{
    if (!ctx || !serial) return -3;
    *serial = ctx_of(ctx)->s2a_serial;
    return 0;
}

extern "C" int mh_sam2aln_output(mh_ctx *ctx, int which, char *buf, size_t cap, size_t *used)
{
    if (!ctx || which < 0 || which > 2 || !used) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("mh_sam2aln_output: no sam2aln results"); return -3; }
    S2AState &S = *c.s2a;
    std::vector<std::string> &out = S.out_cache[which];
    if (!(S.out_valid & (1 << which))) {
        auto t0 = std::chrono::steady_clock::now();
        try {
            s2a_format(S, which, out);
        } catch (const std::exception &e) {
            std::vector<std::string>().swap(out);
            set_error("mh_sam2aln_output: out of memory (%s)", e.what());
            return -2;
        }
        S.t_format[which] = std::chrono::duration<double, std::milli>(
                                std::chrono::steady_clock::now() - t0).count();
        S.out_valid |= 1 << which;
    }
    size_t total = 0;
    for (const std::string &p : out) total += p.size();
    *used = total;
    if (!buf) return 0;
    if (cap < total) { set_error("mh_sam2aln_output: buffer too small"); return -2; }
    for (const std::string &p : out) { memcpy(buf, p.data(), p.size()); buf += p.size(); }
    std::vector<std::string>().swap(out);   // handed over: free the cached text
    S.out_valid &= ~(1 << which);
    return 0;
}

extern "C" int mh_sam2aln_clipping(mh_ctx *ctx, char *buf, size_t cap, size_t *used)
{
    if (!ctx || !used) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_clip_of(ctx, "mh_sam2aln_clipping", true, &S)) return st;
    const std::string &t = S->clip.text;
    *used = t.size();
    if (!buf) return 0;
    if (cap < t.size()) { set_error("mh_sam2aln_clipping: buffer too small"); return -2; }
    memcpy(buf, t.data(), t.size());
    return 0;
}

extern "C" int mh_sam2aln_clipping_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written)
{
    if (!ctx || fd < 0 || offset < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_clip_of(ctx, "mh_sam2aln_clipping_write", true, &S)) return st;
    const std::string &t = S->clip.text;
    if (const int e = write_all_at(fd, t.data(), t.size(), offset)) {
        set_error("mh_sam2aln_clipping_write: write failed (%s)", strerror(e));
        return -4;
    }
    if (written) *written = (int64_t)t.size();
    return 0;
}

extern "C" int mh_sam2aln_clip_counts(mh_ctx *ctx, int32_t *name_id, int64_t *pos, int32_t *count,
                                      int64_t cap, int64_t *n)
{
    if (!ctx || !n || cap < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_clip_of(ctx, "mh_sam2aln_clip_counts", false, &S)) return st;
    const S2AClip &K = S->clip;
    *n = (int64_t)K.name.size();
    if (!name_id || !pos || !count) return 0;
    if (cap < *n) { set_error("mh_sam2aln_clip_counts: buffer too small"); return -2; }
    if (*n) {
        memcpy(name_id, K.name.data(), sizeof(int32_t) * K.name.size());
        memcpy(pos, K.pos.data(), sizeof(int64_t) * K.pos.size());
        memcpy(count, K.count.data(), sizeof(int32_t) * K.count.size());
    }
    return 0;
}

extern "C" int mh_sam2aln_concordance(mh_ctx *ctx, int which, char *buf, size_t cap, size_t *used)
{
    if (!ctx || !used || which < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_conc_of(ctx, "mh_sam2aln_concordance", which, &S)) return st;
    const std::string &t = S->conc.text[which];
    *used = t.size();
    if (!buf) return 0;
    if (cap < t.size()) { set_error("mh_sam2aln_concordance: buffer too small"); return -2; }
    memcpy(buf, t.data(), t.size());
    return 0;
}

extern "C" int mh_sam2aln_concordance_write(mh_ctx *ctx, int which, int fd, int64_t offset,
                                            int64_t *written)
{
    if (!ctx || which < 0 || fd < 0 || offset < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_conc_of(ctx, "mh_sam2aln_concordance_write", which, &S)) return st;
    const std::string &t = S->conc.text[which];
    if (const int e = write_all_at(fd, t.data(), t.size(), offset)) {
        set_error("mh_sam2aln_concordance_write: write failed (%s)", strerror(e));
        return -4;
    }
    if (written) *written = (int64_t)t.size();
    return 0;
}

extern "C" int mh_sam2aln_conc_counts(mh_ctx *ctx, int32_t *name_id, int64_t *pos, int32_t *counts5,
                                      int64_t cap, int64_t *n, int64_t *reads5, int64_t read_cap,
                                      int64_t *read_n)
{
    if (!ctx || !n || !read_n || cap < 0 || read_cap < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_conc_of(ctx, "mh_sam2aln_conc_counts", -1, &S)) return st;
    const S2AConc &Q = S->conc;
    *n = (int64_t)Q.name.size();
    *read_n = (int64_t)(Q.reads.size() / 5);
    if (!name_id || !pos || !counts5 || !reads5) return 0;
    if (cap < *n || read_cap < *read_n) { set_error("mh_sam2aln_conc_counts: buffer too small"); return -2; }
    if (*n) {
        memcpy(name_id, Q.name.data(), sizeof(int32_t) * Q.name.size());
        memcpy(pos, Q.pos.data(), sizeof(int64_t) * Q.pos.size());
        memcpy(counts5, Q.count.data(), sizeof(int32_t) * Q.count.size());
    }
    if (*read_n) memcpy(reads5, Q.reads.data(), sizeof(int64_t) * Q.reads.size());
    return 0;
}

extern "C" int mh_sam2aln_strand(mh_ctx *ctx, char *buf, size_t cap, size_t *used)
{
    if (!ctx || !used) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_strand_of(ctx, "mh_sam2aln_strand", true, &S)) return st;
    const std::string &t = S->strand.text;
    *used = t.size();
    if (!buf) return 0;
    if (cap < t.size()) { set_error("mh_sam2aln_strand: buffer too small"); return -2; }
    memcpy(buf, t.data(), t.size());
    return 0;
}

extern "C" int mh_sam2aln_strand_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written)
{
    if (!ctx || fd < 0 || offset < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_strand_of(ctx, "mh_sam2aln_strand_write", true, &S)) return st;
    const std::string &t = S->strand.text;
    if (const int e = write_all_at(fd, t.data(), t.size(), offset)) {
        set_error("mh_sam2aln_strand_write: write failed (%s)", strerror(e));
        return -4;
    }
    if (written) *written = (int64_t)t.size();
    return 0;
}

extern "C" int mh_sam2aln_strand_counts(mh_ctx *ctx, int32_t *name_id, int32_t *qcut, int64_t *pos,
                                        int32_t *counts15, int64_t cap, int64_t *n)
{
    if (!ctx || !n || cap < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_strand_of(ctx, "mh_sam2aln_strand_counts", false, &S)) return st;
    const S2AStrand &T = S->strand;
    *n = (int64_t)T.name.size();
    if (!name_id || !qcut || !pos || !counts15) return 0;
    if (cap < *n) { set_error("mh_sam2aln_strand_counts: buffer too small"); return -2; }
    if (*n) {
        memcpy(name_id, T.name.data(), sizeof(int32_t) * T.name.size());
        memcpy(qcut, T.qcut.data(), sizeof(int32_t) * T.qcut.size());
        memcpy(pos, T.pos.data(), sizeof(int64_t) * T.pos.size());
        memcpy(counts15, T.count.data(), sizeof(int32_t) * T.count.size());
    }
    return 0;
}

extern "C" int mh_sam2aln_conseq_ins(mh_ctx *ctx, char *buf, size_t cap, size_t *used)
{
    if (!ctx || !used) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_ins_of(ctx, "mh_sam2aln_conseq_ins", true, &S)) return st;
    const std::string &t = S->ins.text;
    *used = t.size();
    if (!buf) return 0;
    if (cap < t.size()) { set_error("mh_sam2aln_conseq_ins: buffer too small"); return -2; }
    memcpy(buf, t.data(), t.size());
    return 0;
}

extern "C" int mh_sam2aln_conseq_ins_write(mh_ctx *ctx, int fd, int64_t offset, int64_t *written)
{
    if (!ctx || fd < 0 || offset < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_ins_of(ctx, "mh_sam2aln_conseq_ins_write", true, &S)) return st;
    const std::string &t = S->ins.text;
    if (const int e = write_all_at(fd, t.data(), t.size(), offset)) {
        set_error("mh_sam2aln_conseq_ins_write: write failed (%s)", strerror(e));
        return -4;
    }
    if (written) *written = (int64_t)t.size();
    return 0;
}

extern "C" int mh_sam2aln_ins_counts(mh_ctx *ctx, int32_t *name_id, int32_t *cut_index, int64_t *pos,
                                     int32_t *count, int64_t cap, int64_t *n)
{
    if (!ctx || !n || cap < 0) return -3;
    S2AState *S = nullptr;
    if (int st = s2a_ins_of(ctx, "mh_sam2aln_ins_counts", false, &S)) return st;
    const S2AIns &I = S->ins;
    *n = (int64_t)I.t_name.size();
    if (!name_id || !cut_index || !pos || !count) return 0;
    if (cap < *n) { set_error("mh_sam2aln_ins_counts: buffer too small"); return -2; }
    if (*n) {
        memcpy(name_id, I.t_name.data(), sizeof(int32_t) * I.t_name.size());
        memcpy(cut_index, I.t_cut.data(), sizeof(int32_t) * I.t_cut.size());
        memcpy(pos, I.t_pos.data(), sizeof(int64_t) * I.t_pos.size());
        memcpy(count, I.t_count.data(), sizeof(int32_t) * I.t_count.size());
    }
    return 0;
}

extern "C" int mh_sam2aln_timing(mh_ctx *ctx, double *ms5)
{
    if (!ctx || !ms5) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("mh_sam2aln_timing: no sam2aln results"); return -3; }
    const S2AState &S = *c.s2a;
    ms5[0] = S.t_parse;
    ms5[1] = S.t_device;
    for (int k = 0; k < 3; ++k) ms5[2 + k] = S.t_format[k];
    return 0;
}

extern "C" int mh_test_sam2aln_info(mh_ctx *ctx, int64_t *out16)
{
    if (!out16) { set_error("mh_test_sam2aln_info: no output array"); return -3; }
    const int64_t consts[7] = {S2A_LDS_BYTES, S2A_BLOCK_CAP, S2A_WPB, S2A_MIN_TABLE, S2A_MAX_CUTS,
                               S2A_SPAN_BYTES, S2A_OP_BYTES};
    for (int k = 0; k < 16; ++k) out16[k] = k < 7 ? consts[k] : 0;
    if (!ctx) return 0;
    const Ctx &c = *ctx_of(ctx);
    out16[15] = c.test_caps.s2a_key_bits;
    if (!c.s2a) return 0;
    const S2AState::Info &I = c.s2a->info;
    out16[7] = I.span_cap;
    out16[8] = I.ops_cap;
    out16[9] = I.wave_bytes;
    out16[10] = I.wpb;
    out16[11] = I.blocks;
    out16[12] = I.n_merge;
    out16[13] = I.n_cut;
    out16[14] = I.tsize;
    return 0;
}

extern "C" int mh_test_set_sam2aln(mh_ctx *ctx, int key_bits, int64_t max_blocks)
{
    if (!ctx || key_bits < 8 || key_bits > 64 || max_blocks < 0) {
        set_error("mh_test_set_sam2aln: key_bits outside 8..64 or max_blocks < 0");
        return -3;
    }
    TestCaps &t = ctx_of(ctx)->test_caps;
    t.s2a_key_bits = key_bits;
    t.s2a_max_blocks = max_blocks;
    return 0;
}

extern "C" int mh_sam2aln_stats(mh_ctx *ctx, int64_t *out4)
{
    if (!ctx || !out4) return -3;
    Ctx &c = *ctx_of(ctx);
    if (!c.s2a) { set_error("mh_sam2aln_stats: no sam2aln results"); return -3; }
    const S2AState &S = *c.s2a;
    int64_t nfail = 0;
    for (int64_t u = 0; u < (int64_t)S.u1.size(); ++u)
        if (S.ucause[u] >= 0 || s2a_many_ns(S, S.merge_of_unit[u])) ++nfail;
    out4[0] = (int64_t)S.u1.size();
    out4[1] = S.n_merge;
    out4[2] = S.n_unique;
    out4[3] = nfail;
    return 0;
}
