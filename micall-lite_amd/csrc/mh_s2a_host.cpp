// mh_s2a_host.cpp -- host half of the sam2aln stage (see mh_sam2aln.hip):
//   s2a_parse   remap.csv as csv.DictReader reads it (sam2aln.py:298), in
//               parallel chunks split at record boundaries; matchmaker
//               (:291-312); parse_sam's row-level causes (:340-348) and the
//               apply_cigar checks that raise (:113-151)
//   s2a_units_resident  the same units, causes and names for rows that are
//               the resident reads and records (mh_sam2aln_resident): no text
//   s2a_format  aligned.csv (:459-478), insert.csv (:357-380, :446-447),
//               failed.csv (:387-389, :449-450) as DictWriter writes them
// Threads: min(16, hardware threads, OMP_NUM_THREADS); output is identical
// for any thread count.
#include <algorithm>
#include <memory>
#include <cerrno>
#include <unistd.h>
#include <atomic>
#include <charconv>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "mh_sam2aln.h"
#include "mh_text.h"

namespace mh {

static const char *const S2A_CAUSE[] = {"", "unmatched", "badCigar", "2refs", "manyNs", ""};

constexpr int MAXCOLS = 64;   // columns a remap.csv record may have

static uint64_t hash_bytes(const char *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= (uint8_t)p[i]; h *= 1099511628211ull; }
    return h ^ (h >> 29);
}

// CIGAR -> ops + apply_cigar's verdict for a read of length L
static int8_t cigar_ops(const char *c, size_t n, int64_t L, std::vector<uint32_t> &ops)
{
    ops.clear();
    if (n == 1 && c[0] == '*') return CIG_STAR;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && c[j] >= '0' && c[j] <= '9') ++j;
        if (j == i || j >= n || !strchr("MIDNSHPX=", c[j]) || c[j] == '\0') return CIG_INVALID;
        i = j + 1;
    }
    int64_t left = 0;
    for (size_t i = 0; i < n;) {
        uint64_t v = 0;
        size_t j = i;
        while (c[j] >= '0' && c[j] <= '9') { v = v * 10 + (uint64_t)(c[j] - '0'); ++j; }
        uint32_t code;
        switch (c[j]) {
        case 'M': code = MH_OP_M; left += (int64_t)v; break;
        case 'I': code = MH_OP_I; left += (int64_t)v; break;
        case 'S': code = MH_OP_S; left += (int64_t)v; break;
        case 'D': code = MH_OP_D; break;
        default: return CIG_UNSUPPORTED;
        }
        if (left > L) return CIG_LONG;
        ops.push_back(((uint32_t)v << 4) | code);
        i = j + 1;
    }
    return left < L ? CIG_SHORT : CIG_OK;
}

struct Part {
    const char *beg = nullptr, *end = nullptr;
    int64_t rows = 0;
    TextBuf qpool, cpool, seq, qual;
    std::vector<int64_t> qoff, coff, soff;
    std::vector<int32_t> qlen, clen, slen, flag, pos, cig_off, n_cig, rid;
    std::vector<uint64_t> qhash;
    std::vector<int8_t> cstate;
    std::vector<uint8_t> qshort;
    std::vector<uint32_t> cig;
    std::vector<std::string> rnames;
    int err = 0;
    int64_t err_row = 0;
    std::string err_msg;
};

static void parse_part(Part &P, const int *col)
{
    std::vector<std::string_view> f;
    std::deque<std::string> scratch;
    std::unordered_map<std::string, int> rmap;
    std::vector<uint32_t> ops;
    const char *p = P.beg;
    int need = 0;
    for (int k = 0; k < 11; ++k) need = std::max(need, col[k] + 1);
    {   // upper bounds from the part's bytes (a row's seq and qual are under
        // half its bytes each; C2 rows are ~600 bytes): no regrowth copies
        const size_t bytes = (size_t)(P.end - P.beg);
        P.seq.reserve(bytes / 2 + 64);
        P.qual.reserve(bytes / 2 + 64);
        P.qpool.reserve(bytes / 4 + 64);
        P.cpool.reserve(bytes / 8 + 64);
        const size_t rows = bytes / 256 + 16;
        P.qoff.reserve(rows); P.coff.reserve(rows); P.soff.reserve(rows); P.qlen.reserve(rows);
        P.clen.reserve(rows); P.slen.reserve(rows); P.flag.reserve(rows); P.pos.reserve(rows);
        P.cig_off.reserve(rows); P.n_cig.reserve(rows); P.rid.reserve(rows); P.qhash.reserve(rows);
        P.cstate.reserve(rows); P.qshort.reserve(rows);
    }
    while (csv_views(p, P.end, f, scratch)) {
        if (f.size() > (size_t)MAXCOLS) {
            P.err = 1; P.err_row = P.rows; P.err_msg = "more than 64 columns";
            return;
        }
        if (f.size() == 1 && f[0].empty()) continue;          // blank line
        if ((int)f.size() < need) {
            P.err = 1; P.err_row = P.rows; P.err_msg = "short row";
            return;
        }
        const std::string_view q = f[col[0]], rn = f[col[2]], cg = f[col[5]], sq = f[col[9]],
                               ql = f[col[10]];
        int32_t fl = 0, ps = 0;
        if (!py_int32(f[col[1]], fl)) {
            P.err = 1; P.err_row = P.rows; P.err_msg = "flag is not an integer";
            return;
        }
        P.flag.push_back(fl);
        P.pos.push_back(py_int32(f[col[3]], ps) ? ps : INT32_MIN);
        P.qoff.push_back((int64_t)P.qpool.size());
        P.qlen.push_back((int32_t)q.size());
        P.qpool.append(q.data(), q.size());
        P.qhash.push_back(hash_bytes(q.data(), q.size()));
        auto it = rmap.find(std::string(rn));
        if (it == rmap.end()) {
            it = rmap.emplace(std::string(rn), (int)P.rnames.size()).first;
            P.rnames.emplace_back(rn);
        }
        P.rid.push_back(it->second);
        P.coff.push_back((int64_t)P.cpool.size());
        P.clen.push_back((int32_t)cg.size());
        P.cpool.append(cg.data(), cg.size());
        P.cstate.push_back(cigar_ops(cg.data(), cg.size(), (int64_t)sq.size(), ops));
        P.cig_off.push_back((int32_t)P.cig.size());
        P.n_cig.push_back(P.cstate.back() == CIG_OK ? (int32_t)ops.size() : 0);
        if (P.cstate.back() == CIG_OK) P.cig.insert(P.cig.end(), ops.begin(), ops.end());
        P.soff.push_back((int64_t)P.seq.size());
        P.slen.push_back((int32_t)sq.size());
        P.seq.append(sq.data(), sq.size());
        P.qshort.push_back(ql.size() < sq.size());
        if (ql.size() >= sq.size()) P.qual.append(ql.data(), sq.size());
        else {
            P.qual.append(ql.data(), ql.size());
            const size_t at = P.qual.size();
            P.qual.resize(at + (sq.size() - ql.size()));
            memset(P.qual.data() + at, '!', sq.size() - ql.size());
        }
        ++P.rows;
    }
}

static std::string cigar_text(const S2AState &S, int64_t r)
{
    return std::string(S.cpool.data() + S.coff[r], (size_t)S.clen[r]);
}

// the RuntimeError apply_cigar raises for row r, as the reference words it
static int row_error(const S2AState &S, int64_t r)
{
    const std::string cg = cigar_text(S, r);
    switch (S.cstate[r]) {
    case CIG_INVALID: set_error("Invalid CIGAR string: '%s'.", cg.c_str()); return -3;
    case CIG_UNSUPPORTED: {
        // the first token that is not M/I/D/S (sam2aln.py:141-143)
        size_t i = 0;
        while (i < cg.size()) {
            size_t j = i;
            while (cg[j] >= '0' && cg[j] <= '9') ++j;
            if (!strchr("MIDS", cg[j])) break;
            i = j + 1;
        }
        size_t j = i;
        while (j < cg.size() && cg[j] >= '0' && cg[j] <= '9') ++j;
        set_error("Unsupported CIGAR token: '%s'.", cg.substr(i, j + 1 - i).c_str());
        return -3;
    }
    case CIG_LONG: set_error("CIGAR string '%s' is too long for sequence.", cg.c_str()); return -3;
    case CIG_SHORT: set_error("CIGAR string '%s' is too short for sequence.", cg.c_str()); return -3;
    default: break;
    }
    if (S.pos[r] == INT32_MIN) { set_error("invalid literal for int() in pos of row %lld", (long long)r + 1); return -3; }
    if (S.qshort[r]) { set_error("string index out of range (qual shorter than seq, row %lld)", (long long)r + 1); return -3; }
    return 0;
}

// MH_S2A_TRACE=1: phase times of s2a_parse to stderr
static void s2a_mark(std::chrono::steady_clock::time_point t0, const char *what)
{
    static const bool on = getenv("MH_S2A_TRACE") && *getenv("MH_S2A_TRACE") == '1';
    if (on)
        fprintf(stderr, "s2a_parse %s %.1f ms\n", what,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

int s2a_parse(S2AState &S, const char *text, int64_t len, int64_t body_lo, int64_t body_hi)
{
    const auto tp = std::chrono::steady_clock::now();
    const char *p = text, *end = text + len;
    std::vector<std::string> head;
    if (!csv_record(p, end, head)) {
        set_error("remap csv: empty");
        return -3;
    }
    if (body_lo >= 0) {       // one part of the body: records [body_lo, body_hi)
        if (body_lo < p - text || body_hi < body_lo || body_hi > len) {
            set_error("remap csv: bad part bounds");
            return -3;
        }
        p = text + body_lo;
        end = text + body_hi;
    }
    const char *want[11] = {"qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext",
                            "tlen", "seq", "qual"};
    int col[11];
    csv_columns(head, want, 11, col);
    for (int k = 0; k < 11; ++k)
        if (col[k] < 0) {
            if (k == 4 || k == 6 || k == 7 || k == 8) { col[k] = 0; continue; }   // unused
            set_error("remap csv: missing column %s", want[k]);
            return -3;
        }
    // ---- split the body at record ends ----
    const int64_t body = end - p;
    int nt = s2a_threads();
    if (body < (int64_t)nt * (1 << 20)) nt = (int)std::max<int64_t>(1, body >> 20);
    const std::vector<const char *> cut = csv_cuts(p, end, nt);
    std::vector<Part> parts(nt);
    for (int t = 0; t < nt; ++t) { parts[t].beg = cut[t]; parts[t].end = cut[t + 1]; }
    s2a_mark(tp, "split");
    par_for(nt, [&](int t) { parse_part(parts[t], col); });
    s2a_mark(tp, "parts");
    int64_t base = 0;
    for (auto &P : parts) {
        if (P.err) {
            set_error("remap csv: row %lld: %s", (long long)(base + P.err_row + 1), P.err_msg.c_str());
            return -3;
        }
        base += P.rows;
    }
    // ---- concatenate the parts ----
    const int64_t nr = base;
    S.n_rows = nr;
    std::vector<int64_t> r0(nt + 1, 0), q0(nt + 1, 0), c0(nt + 1, 0), s0(nt + 1, 0), g0(nt + 1, 0);
    for (int t = 0; t < nt; ++t) {
        r0[t + 1] = r0[t] + parts[t].rows;
        q0[t + 1] = q0[t] + (int64_t)parts[t].qpool.size();
        c0[t + 1] = c0[t] + (int64_t)parts[t].cpool.size();
        s0[t + 1] = s0[t] + (int64_t)parts[t].seq.size();
        g0[t + 1] = g0[t] + (int64_t)parts[t].cig.size();
    }
    // rnames: global ids in part order of first appearance
    std::unordered_map<std::string, int> gid;
    S.rnames.clear();
    std::vector<std::vector<int32_t>> remap_id(nt);
    for (int t = 0; t < nt; ++t)
        for (auto &n : parts[t].rnames) {
            auto it = gid.emplace(n, (int)S.rnames.size());
            if (it.second) S.rnames.push_back(n);
            remap_id[t].push_back(it.first->second);
        }
    S.qpool.resize((size_t)q0[nt]); S.cpool.resize((size_t)c0[nt]);
    S.seq.resize((size_t)s0[nt]); S.qual.resize((size_t)s0[nt]);
    S.qoff.resize(nr); S.qlen.resize(nr); S.coff.resize(nr); S.clen.resize(nr);
    S.cstate.resize(nr); S.rid.resize(nr); S.flag.resize(nr); S.pos.resize(nr);
    S.qshort.resize(nr); S.soff.resize(nr); S.slen.resize(nr); S.cig_off.resize(nr);
    S.n_cig.resize(nr); S.cig.resize((size_t)g0[nt]);
    std::vector<uint64_t> qhash(nr);
    par_for(nt, [&](int t) {
        const Part &P = parts[t];
        const int64_t b = r0[t];
        memcpy(&S.qpool[q0[t]], P.qpool.data(), P.qpool.size());
        memcpy(&S.cpool[c0[t]], P.cpool.data(), P.cpool.size());
        memcpy(&S.seq[s0[t]], P.seq.data(), P.seq.size());
        memcpy(&S.qual[s0[t]], P.qual.data(), P.qual.size());
        if (!P.cig.empty()) memcpy(&S.cig[g0[t]], P.cig.data(), 4 * P.cig.size());
        for (int64_t i = 0; i < P.rows; ++i) {
            S.qoff[b + i] = P.qoff[i] + q0[t];
            S.qlen[b + i] = P.qlen[i];
            S.coff[b + i] = P.coff[i] + c0[t];
            S.clen[b + i] = P.clen[i];
            S.cstate[b + i] = P.cstate[i];
            S.rid[b + i] = remap_id[t][P.rid[i]];
            S.flag[b + i] = P.flag[i];
            S.pos[b + i] = P.pos[i];
            S.qshort[b + i] = P.qshort[i];
            S.soff[b + i] = P.soff[i] + s0[t];
            S.slen[b + i] = P.slen[i];
            S.cig_off[b + i] = (int32_t)(P.cig_off[i] + g0[t]);
            S.n_cig[b + i] = P.n_cig[i];
            qhash[b + i] = P.qhash[i];
        }
    });
    {   // the parts' buffers freed off the clock (GB-sized frees take tens of ms)
        auto *old = new std::vector<Part>(std::move(parts));
        std::thread([old]() { delete old; }).detach();
    }
    s2a_mark(tp, "concat");
    // ---- matchmaker (sam2aln.py:291-312): open addressing on qname ----
    uint64_t cap = 1024;
    while (cap < (uint64_t)(2 * nr + 2)) cap <<= 1;
    std::vector<int64_t> slot_row(cap, -1);   // row waiting for its mate
    std::vector<int64_t> pend_of_row(nr, -1);
    std::vector<std::pair<int64_t, bool>> pend;
    pend.reserve((size_t)nr);
    S.u1.clear(); S.u2.clear();
    S.u1.reserve((size_t)nr / 2 + 1); S.u2.reserve((size_t)nr / 2 + 1);
    auto same = [&](int64_t a, int64_t b) {
        return S.qlen[a] == S.qlen[b] &&
               memcmp(S.qpool.data() + S.qoff[a], S.qpool.data() + S.qoff[b], (size_t)S.qlen[a]) == 0;
    };
    for (int64_t r = 0; r < nr; ++r) {
        uint64_t s = qhash[r] & (cap - 1);
        int64_t hit = -1;
        uint64_t tomb = ~0ull;
        while (slot_row[s] != -1) {
            const int64_t o = slot_row[s];
            if (o == -2) { if (tomb == ~0ull) tomb = s; }
            else if (qhash[o] == qhash[r] && same(o, r)) { hit = (int64_t)s; break; }
            s = (s + 1) & (cap - 1);
        }
        if (hit >= 0) {
            const int64_t o = slot_row[hit];
            pend[pend_of_row[o]].second = false;
            S.u1.push_back(o);
            S.u2.push_back(r);
            slot_row[hit] = -2;   // tombstone
        } else {
            slot_row[tomb != ~0ull ? tomb : s] = r;
            pend_of_row[r] = (int64_t)pend.size();
            pend.push_back({r, true});
        }
    }
    for (auto &o : pend) if (o.second) { S.u1.push_back(o.first); S.u2.push_back(-1); }
    s2a_mark(tp, "matchmaker");
    // ---- parse_sam's early causes and the rname order ----
    const int64_t nu = (int64_t)S.u1.size();
    S.ucause.assign(nu, -1);
    S.upaired.assign(nu, 0);
    S.merge_of_unit.assign(nu, -1);
    S.name_id.assign(nu, 0);
    S.names.clear();
    std::vector<int32_t> nid_of_rid(S.rnames.size(), -1);
    for (int64_t u = 0; u < nu; ++u) {
        const int64_t r1 = S.u1[u], r2 = S.u2[u];
        int32_t &n = nid_of_rid[S.rid[r1]];
        if (n < 0) { n = (int32_t)S.names.size(); S.names.push_back(S.rnames[S.rid[r1]]); }
        S.name_id[u] = n;
        const int paired = S.flag[r1] & 1;
        S.upaired[u] = (int8_t)paired;
        int cause = -1;
        if (paired && r2 < 0) cause = S2A_UNMATCHED;
        else if (S.cstate[r1] == CIG_STAR || (r2 >= 0 && S.cstate[r2] == CIG_STAR)) cause = S2A_BADCIGAR;
        else if (paired && S.rid[r1] != S.rid[r2]) cause = S2A_2REFS;
        S.ucause[u] = (int8_t)cause;
        if (cause < 0) {
            if (int st = row_error(S, r1)) return st;
            if (paired)
                if (int st = row_error(S, r2)) return st;
        }
    }
    s2a_mark(tp, "causes");
    return 0;
}

// ---------------------------------------------------------------------------
// output
// ---------------------------------------------------------------------------
static void put_int(std::string &out, long long v)
{
    char b[24];
    auto r = std::to_chars(b, b + sizeof b, v);
    out.append(b, (size_t)(r.ptr - b));
}

template <class Cmp>
static void parallel_sort(std::vector<int64_t> &v, Cmp cmp, int nt)
{
    const size_t n = v.size();
    if (nt <= 1 || n < 65536) { std::sort(v.begin(), v.end(), cmp); return; }
    std::vector<size_t> b(nt + 1);
    for (int t = 0; t <= nt; ++t) b[t] = n * (size_t)t / (size_t)nt;
    par_for(nt, [&](int t) { std::sort(v.begin() + b[t], v.begin() + b[t + 1], cmp); });
    for (int w = 1; w < nt; w *= 2) {
        std::vector<std::pair<int, int>> jobs;
        for (int t = 0; t + w < nt; t += 2 * w) jobs.push_back({t, std::min(t + 2 * w, nt)});
        par_for((int)jobs.size(), [&](int j) {
            const int a = jobs[j].first, m = a + w, z = jobs[j].second;
            std::inplace_merge(v.begin() + b[a], v.begin() + b[m], v.begin() + b[z], cmp);
        });
    }
}

// the pieces fn(t, range) writes for nt ranges of [0, n), appended in order
using Pieces = std::vector<std::string>;

// Where an output's text goes, in order: collected as pieces (out), or
// written to fd from pos (pwrite) as each piece is finished.
struct TextSink {
    Pieces *out = nullptr;
    int fd = -1;
    int64_t pos = 0;
    int err = 0;    // errno of a failed write
    // the crc32 of everything put so far, kept when want_crc: joined from the
    // pieces' own (piece_crc: computed by the thread that formatted the piece)
    bool want_crc = false;
    uint32_t crc = 0;
    void put(std::string &s, const uint32_t *piece_crc = nullptr)
    {
        if (want_crc)
            crc = crc32_join(crc, piece_crc ? *piece_crc : crc32_update(0, s.data(), s.size()),
                             (int64_t)s.size());
        if (out) {
            if (!s.empty()) out->push_back(std::move(s));
            return;
        }
        if (!err && !(err = write_all_at(fd, s.data(), s.size(), pos))) pos += (int64_t)s.size();
        std::string().swap(s);
    }
};

// fn(text, a, b) formats items [a, b) of n.  Collected: one piece per
// thread.  Streamed: jobs of STREAM_ROWS items on nt - 1 formatting threads
// while this thread writes the finished jobs in order, so the writing of a
// GB-sized output overlaps its formatting.
constexpr int64_t STREAM_ROWS = 4096;
static void parallel_text(int64_t n, int nt, TextSink &sink,
                          const std::function<void(std::string &, int64_t, int64_t)> &fn)
{
    if (n < 4096) nt = 1;
    if (sink.out) {
        std::vector<std::string> piece(nt);
        par_for(nt, [&](int t) { fn(piece[t], n * t / nt, n * (t + 1) / nt); });
        for (auto &x : piece) sink.put(x);
        return;
    }
    const int64_t nj = (n + STREAM_ROWS - 1) / STREAM_ROWS;
    if (nt <= 1 || nj <= 1) {
        std::string one;
        fn(one, 0, n);
        sink.put(one);
        return;
    }
    std::vector<std::string> buf((size_t)nj);
    std::vector<uint32_t> crc(sink.want_crc ? (size_t)nj : 0);
    std::unique_ptr<std::atomic<int>[]> done(new std::atomic<int>[(size_t)nj]);
    for (int64_t j = 0; j < nj; ++j) done[j].store(0);
    std::atomic<int64_t> next(0);
    std::atomic<int> failed(0);
    // thread 0 (the caller) writes; threads 1 .. format.  Should a thread not
    // start, its formatting runs here before the writing (par_for).
    par_for(std::max(1, nt - 1) + 1, [&](int t) {
        if (t) {
            try {
                for (int64_t j; !failed && (j = next.fetch_add(1)) < nj;) {
                    fn(buf[(size_t)j], j * STREAM_ROWS, std::min(n, (j + 1) * STREAM_ROWS));
                    if (sink.want_crc)
                        crc[(size_t)j] = crc32_update(0, buf[(size_t)j].data(), buf[(size_t)j].size());
                    done[j].store(1, std::memory_order_release);
                }
            } catch (...) {
                failed = 1;   // the writer stops waiting; par_for rethrows
                throw;
            }
            return;
        }
        for (int64_t j = 0; j < nj && !failed && !sink.err; ++j) {
            while (!done[j].load(std::memory_order_acquire) && !failed) std::this_thread::yield();
            if (failed) break;
            sink.put(buf[(size_t)j], sink.want_crc ? &crc[(size_t)j] : nullptr);
        }
        failed = 1;   // a write error: the formatters stop at their next job
    });
}

// aligned.csv's row order (sam2aln.py:459-478): per rname in first-seen order
// and per q-cutoff, the distinct merged sequences sorted by (count, gap
// prefix, sequence), all descending; groups without rows are left out
void s2a_order(S2AState &S)
{
    S2AOrder &O = S.order;
    if (O.valid) return;
    O = S2AOrder();
    const int nt = s2a_threads();
    const int nn = (int)S.names.size(), nc = (int)S.q_cutoffs.size();
    std::vector<int32_t> mref(S.n_merge);
    for (int64_t u = 0; u < (int64_t)S.u1.size(); ++u)
        if (S.merge_of_unit[u] >= 0) mref[S.merge_of_unit[u]] = S.name_id[u];
    // one group per (rname, cutoff k).  A rname's groups come in the order in
    // which each cutoff first received a passing sequence (the reference's
    // region[qcut] is created on first use, sam2aln.py:446-452): by the first
    // merge unit that is OK at k -- merge units are in matchmaker order --
    // then by k, the order within one pair (:391)
    std::vector<std::vector<int64_t>> by((size_t)nn * nc);
    for (int64_t k = 0; k < S.n_unique; ++k) {
        const int64_t e = S.uniq[2 * k];
        by[(size_t)mref[e / nc] * nc + e % nc].push_back(k);
    }
    std::vector<int64_t> first_ok((size_t)nn * nc, INT64_MAX);
    for (int64_t e = 0; e < S.n_merge * nc; ++e)
        if (S.res[4 * e] == S2A_OK) {
            int64_t &f = first_ok[(size_t)mref[e / nc] * nc + e % nc];
            f = std::min(f, e / nc);
        }
    std::vector<int> order((size_t)nn * nc);
    for (int g = 0; g < nn * nc; ++g) order[g] = g;
    for (int r = 0; r < nn; ++r)
        std::sort(order.begin() + (size_t)r * nc, order.begin() + (size_t)(r + 1) * nc,
                  [&](int x, int y) { return first_ok[x] != first_ok[y] ? first_ok[x] < first_ok[y] : x < y; });
    auto cmp = [&](int64_t x, int64_t y) {
        const int64_t rx = S.uniq[2 * x], ry = S.uniq[2 * y];
        const int cx = S.uniq[2 * x + 1], cy = S.uniq[2 * y + 1];
        if (cx != cy) return cx > cy;
        const int ox = S.res[4 * rx + 1], oy = S.res[4 * ry + 1];
        if (ox != oy) return ox > oy;
        const int64_t lx = S.uniq_off[x + 1] - S.uniq_off[x], ly = S.uniq_off[y + 1] - S.uniq_off[y];
        const int c = memcmp(S.gathered.data() + S.uniq_off[x], S.gathered.data() + S.uniq_off[y],
                             (size_t)std::min(lx, ly));
        if (c != 0) return c > 0;
        return lx > ly;
    };
    // the order of cmp in two passes: by (count, offset) -- one 64-bit key,
    // cheap to compare -- then each run of equal keys by its sequence, the
    // runs sorted in parallel (no serial merge of memcmp comparisons)
    std::vector<uint64_t> key((size_t)S.n_unique);
    par_for(nt, [&](int t) {
        for (int64_t k = S.n_unique * t / nt; k < S.n_unique * (t + 1) / nt; ++k)
            key[(size_t)k] = (uint64_t)(uint32_t)S.uniq[2 * k + 1] << 32 |
                             (uint32_t)(S.res[4 * S.uniq[2 * k] + 1] ^ (int32_t)0x80000000);
    });
    auto by_key = [&](int64_t x, int64_t y) { return key[(size_t)x] > key[(size_t)y]; };
    O.rows.resize((size_t)S.n_unique);
    O.g_first.assign(1, 0);
    for (int g : order) {
        auto &v = by[g];
        if (v.empty()) continue;
        parallel_sort(v, by_key, nt);
        std::vector<size_t> runs{0};
        for (size_t i = 1; i < v.size(); ++i)
            if (key[(size_t)v[i]] != key[(size_t)v[i - 1]]) runs.push_back(i);
        runs.push_back(v.size());
        std::atomic<size_t> next_run(0);
        par_for(nt, [&](int) {
            for (size_t j; (j = next_run.fetch_add(1)) + 1 < runs.size();)
                if (runs[j + 1] - runs[j] > 1) std::sort(v.begin() + runs[j], v.begin() + runs[j + 1], cmp);
        });
        const int64_t at = O.g_first.back(), n = (int64_t)v.size();
        const int np = n < 65536 ? 1 : nt;
        std::vector<uint64_t> part((size_t)np, 0);
        par_for(np, [&](int t) {
            uint64_t sum = 0;
            for (int64_t i = n * t / np; i < n * (t + 1) / np; ++i) {
                O.rows[(size_t)(at + i)] = (int32_t)v[(size_t)i];
                sum += (uint32_t)S.uniq[2 * v[(size_t)i] + 1];
            }
            part[(size_t)t] = sum;
        });
        uint64_t total = 0;
        for (uint64_t x : part) total += x;
        O.g_name.push_back(g / nc);
        O.g_qcut.push_back(S.q_cutoffs[g % nc]);
        O.g_total.push_back(total);
        O.g_first.push_back(at + n);
        std::vector<int64_t>().swap(v);
    }
    O.valid = true;
}

// aligned.csv: the rows of S.order; seq written without its leading /
// trailing gaps
static void s2a_aligned(S2AState &S, TextSink &out)
{
    const int nt = s2a_threads();
    {
        std::string head("refname,qcut,rank,count,offset,seq\n");
        out.put(head);
    }
    s2a_order(S);
    const S2AOrder &O = S.order;
    for (size_t g = 0; g < O.g_name.size(); ++g) {
        const int32_t qcut = O.g_qcut[g];
        const int32_t *v = O.rows.data() + O.g_first[g];
        const std::string &name = S.names[(size_t)O.g_name[g]];
        std::string ref;
        csv_field(ref, name.data(), name.size());
        const size_t row_guess = ref.size() + 40 + (S.n_unique ? (size_t)(S.gathered.size() / S.n_unique) : 0);
        parallel_text(O.g_first[g + 1] - O.g_first[g], nt, out, [&](std::string &o, int64_t a, int64_t b) {
            o.reserve(o.size() + (size_t)(b - a) * row_guess);
            for (int64_t rank = a; rank < b; ++rank) {
                const int64_t k = v[rank], rep = S.uniq[2 * k];
                o += ref;
                o.push_back(',');
                put_int(o, qcut);
                o.push_back(',');
                put_int(o, rank);
                o.push_back(',');
                put_int(o, S.uniq[2 * k + 1]);
                o.push_back(',');
                put_int(o, S.res[4 * rep + 1]);
                o.push_back(',');
                o.append(S.gathered.data() + S.uniq_off[k], (size_t)S.res[4 * rep + 3]);
                o.push_back('\n');
            }
        });
    }
}

// insert.csv rows of parse_sam (sam2aln.py:357-380): every I op of the
// mates of a unit that reached apply_cigar, at pos - 1 + read offset
static void s2a_inserts(const S2AState &S, TextSink &out, int64_t u0, int64_t u1, bool head_row)
{
    if (head_row) {
        std::string head("qname,fwd_rev,refname,pos,insert,qual\n");
        out.put(head);
    }
    parallel_text(u1 - u0, s2a_threads(), out, [&](std::string &o, int64_t a, int64_t b) {
        for (int64_t u = u0 + a; u < u0 + b; ++u) {
            if (S.ucause[u] >= 0) continue;
            const int64_t r1 = S.u1[u];
            for (int k = 0; k < (S.upaired[u] ? 2 : 1); ++k) {
                const int64_t r = k ? S.u2[u] : r1;
                int64_t left = 0;
                for (int x = 0; x < S.n_cig[r]; ++x) {
                    const uint32_t op = S.cig[S.cig_off[r] + x];
                    const int n = (int)(op >> 4), t = (int)(op & 15);
                    if (t == MH_OP_I) {
                        csv_field(o, S.qpool.data() + S.qoff[r1], (size_t)S.qlen[r1]);
                        o += (S.flag[r] & 0x40) ? ",F," : ",R,";
                        const std::string &rn = S.rnames[S.rid[r1]];
                        csv_field(o, rn.data(), rn.size());
                        o.push_back(',');
                        put_int(o, (long long)S.pos[r] - 1 + left);
                        o.push_back(',');
                        csv_field(o, S.seq.data() + S.soff[r] + left, (size_t)n);
                        o.push_back(',');
                        csv_field(o, S.qual.data() + S.soff[r] + left, (size_t)n);
                        o.push_back('\n');
                    }
                    if (t == MH_OP_M || t == MH_OP_I || t == MH_OP_S) left += n;
                }
            }
        }
    });
}

static void s2a_failed(const S2AState &S, TextSink &out, int64_t u0, int64_t u1, bool head_row)
{
    if (head_row) {
        std::string head("qname,cause\n");
        out.put(head);
    }
    parallel_text(u1 - u0, s2a_threads(), out, [&](std::string &o, int64_t a, int64_t b) {
        for (int64_t u = u0 + a; u < u0 + b; ++u) {
            int cause = S.ucause[u];
            if (cause < 0 && s2a_many_ns(S, S.merge_of_unit[u])) cause = S2A_MANYNS;
            if (cause < 0) continue;
            const int64_t r1 = S.u1[u];
            csv_field(o, S.qpool.data() + S.qoff[r1], (size_t)S.qlen[r1]);
            o.push_back(',');
            o += S2A_CAUSE[cause];
            o.push_back('\n');
        }
    });
}

static void s2a_emit(S2AState &S, int which, TextSink &sink)
{
    const int64_t nu = (int64_t)S.u1.size();
    if (which == 0) s2a_aligned(S, sink);
    else if (which == 1) s2a_inserts(S, sink, 0, nu, true);
    else s2a_failed(S, sink, 0, nu, true);
}

int s2a_format_units(const S2AState &S, int which, int64_t u0, int64_t u1, bool head_row,
                     std::vector<std::string> &out)
{
    out.clear();
    TextSink sink;
    sink.out = &out;
    if (which == 1) s2a_inserts(S, sink, u0, u1, head_row);
    else s2a_failed(S, sink, u0, u1, head_row);
    return 0;
}

int s2a_format(S2AState &S, int which, std::vector<std::string> &out)
{
    out.clear();
    TextSink sink;
    sink.out = &out;
    s2a_emit(S, which, sink);
    return 0;
}

int s2a_format_write(S2AState &S, int which, int fd, int64_t offset, int64_t *written, uint32_t *crc)
{
    TextSink sink;
    sink.fd = fd;
    sink.pos = offset;
    sink.want_crc = crc != nullptr;
    s2a_emit(S, which, sink);
    if (written) *written = sink.pos - offset;
    if (crc) *crc = sink.crc;
    return sink.err;
}

// ---------------------------------------------------------------------------
// units of the resident rows (mh_sam2aln_resident)
// ---------------------------------------------------------------------------
// What s2a_parse derives from remap.csv, for a file that holds every
// resident read once in read order: matchmaker (sam2aln.py:291-312) pairs
// rows by QNAME, so with mates interleaved unit p is rows (2p, 2p + 1) as
// long as the two mates share their QNAME, and unpaired reads with distinct
// QNAMEs are all left over, in read order, as (row, None).
int s2a_units_resident(Ctx &c, S2AState &S, int n_refs, const char *const *refnames,
                       const std::vector<int32_t> &sam_ref, const std::vector<int32_t> &span_ins)
{
    const auto tp = std::chrono::steady_clock::now();
    const NameTable &names = c.names;
    const int64_t nr = S.n_rows;
    const bool paired = c.reads.paired != 0;
    const int nt = std::max(1, std::min(s2a_threads(), (int)(nr >> 14) + 1));
    // ---- may the rows stand for matchmaker's units? ----
    std::atomic<int> differs(0);
    if (paired) {
        par_for(nt, [&](int t) {
            for (int64_t p = (nr / 2) * t / nt; p < (nr / 2) * (t + 1) / nt; ++p)
                if (names[2 * p] != names[2 * p + 1]) { differs = 1; return; }
        });
    } else {
        // distinct QNAMEs: no two equal hashes (equal hashes of two distinct
        // names send the call to the file path too, which is always right)
        std::vector<int64_t> h((size_t)nr);
        par_for(nt, [&](int t) {
            for (int64_t r = nr * t / nt; r < nr * (t + 1) / nt; ++r)
                h[(size_t)r] = (int64_t)hash_bytes(names[r].data(), names[r].size());
        });
        parallel_sort(h, [](int64_t a, int64_t b) { return a < b; }, nt);
        for (int64_t r = 1; r < nr; ++r)
            if (h[(size_t)r] == h[(size_t)r - 1]) { differs = 1; break; }
    }
    if (differs) return 1;
    s2a_mark(tp, "resident pairing");
    // ---- QNAMEs and RNAMEs (every per-row array is written by the threads below) ----
    S.qpool.resize(names.pool.size());
    S.qoff.resize(nr); S.qlen.resize(nr); S.rid.resize(nr);
    S.coff.resize(nr); S.clen.resize(nr); S.cpool.clear();
    S.cstate.resize(nr); S.qshort.resize(nr);
    S.soff.resize(nr); S.slen.resize(nr);
    // RNAME ids as the parser gives them: equal names share one id; '*' last
    S.rnames.clear();
    std::unordered_map<std::string, int> gid;
    std::vector<int32_t> rid_of_ref((size_t)n_refs + 1);
    for (int k = 0; k <= n_refs; ++k) {
        const std::string name(k < n_refs ? refnames[k] : "*");
        auto it = gid.emplace(name, (int)S.rnames.size());
        if (it.second) S.rnames.push_back(name);
        rid_of_ref[k] = it.first->second;
    }
    std::atomic<int> bad_ref(0);
    par_for(nt, [&](int t) {
        const size_t q0 = names.pool.size() * (size_t)t / (size_t)nt,
                     q1 = names.pool.size() * (size_t)(t + 1) / (size_t)nt;
        if (q1 > q0) memcpy(S.qpool.data() + q0, names.pool.data() + q0, q1 - q0);
        for (int64_t r = nr * t / nt; r < nr * (t + 1) / nt; ++r) {
            S.coff[r] = 0; S.clen[r] = 0; S.qshort[r] = 0; S.soff[r] = 0; S.slen[r] = 0;
            S.qoff[r] = names.off[r];
            S.qlen[r] = (int32_t)(names.off[r + 1] - names.off[r]);
            const int32_t sr = sam_ref[r];
            if (sr >= n_refs) { bad_ref = 1; return; }
            S.rid[r] = rid_of_ref[sr >= 0 ? sr : n_refs];
            S.cstate[r] = span_ins[r] < 0 ? CIG_STAR : CIG_OK;
        }
    });
    if (bad_ref) {
        set_error("mh_sam2aln_resident: a record names a reference outside the %d given", n_refs);
        return -3;
    }
    s2a_mark(tp, "resident rows");
    // ---- units, parse_sam's early causes and the rname order ----
    const int64_t nu = paired ? nr / 2 : nr;
    S.u1.resize(nu); S.u2.resize(nu);
    S.ucause.assign(nu, -1);
    S.upaired.assign(nu, 0);
    S.merge_of_unit.assign(nu, -1);
    S.name_id.assign(nu, 0);
    S.names.clear();
    std::vector<int32_t> nid_of_rid(S.rnames.size(), -1);
    for (int64_t u = 0; u < nu; ++u) {
        const int64_t r1 = paired ? 2 * u : u, r2 = paired ? 2 * u + 1 : -1;
        S.u1[u] = r1;
        S.u2[u] = r2;
        int32_t &n = nid_of_rid[S.rid[r1]];
        if (n < 0) { n = (int32_t)S.names.size(); S.names.push_back(S.rnames[S.rid[r1]]); }
        S.name_id[u] = n;
        const int pr = S.flag[r1] & 1;
        S.upaired[u] = (int8_t)pr;
        int cause = -1;
        if (pr && r2 < 0) cause = S2A_UNMATCHED;
        else if (S.cstate[r1] == CIG_STAR || (r2 >= 0 && S.cstate[r2] == CIG_STAR)) cause = S2A_BADCIGAR;
        else if (pr && S.rid[r1] != S.rid[r2]) cause = S2A_2REFS;
        S.ucause[u] = (int8_t)cause;
    }
    s2a_mark(tp, "resident units");
    // ---- SEQ / QUAL on the host: only the rows insert.csv quotes from ----
    std::vector<int64_t> ins_rows;
    int64_t text = 0;
    for (int64_t r = 0; r < nr; ++r) {
        if (span_ins[r] < 0 || !(span_ins[r] & 1)) continue;
        const int L = host_read_text(c, r, false, nullptr, nullptr);
        if (L < 0) {
            set_error("mh_sam2aln_resident: the reads' text is not kept on the host");
            return -3;
        }
        ins_rows.push_back(r);
        S.soff[r] = text;
        S.slen[r] = L;
        text += L;
    }
    S.seq.resize((size_t)text);
    S.qual.resize((size_t)text);
    const int64_t ni = (int64_t)ins_rows.size();
    par_for(std::max(1, std::min(nt, (int)(ni >> 10) + 1)), [&](int t) {
        const int n = std::max(1, std::min(nt, (int)(ni >> 10) + 1));
        for (int64_t k = ni * t / n; k < ni * (t + 1) / n; ++k) {
            const int64_t r = ins_rows[(size_t)k];
            host_read_text(c, r, (span_ins[r] & 2) != 0, S.seq.data() + S.soff[r], S.qual.data() + S.soff[r]);
        }
    });
    s2a_mark(tp, "resident insert rows");
    return 0;
}

}  // namespace mh
