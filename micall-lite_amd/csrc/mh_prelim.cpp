// mh_prelim.cpp -- prelim.csv text to pileup rows on the host:
// csv.DictReader semantics for the 11 SAM columns prelim_map writes
// (prelim_map.py:142-151), remap.matchmaker (remap.py:853-889) over the rows
// whose rname is in the @SQ set, then compact reference ids.  Plain C++, no
// device part: it is also compiled alone, with the sanitizers, by
// tests/test_csv_readers_host.py.
#include "mh_prelim.h"

#include <algorithm>
#include <cstring>
#include <deque>
#include <string_view>
#include <unordered_map>

#include "mh_text.h"

namespace mh {

void set_error(const char *fmt, ...);

namespace {

// the rows of one block of the text (a host thread's share)
struct Block {
    std::vector<int32_t> flag, ref, pos, cig_off, n_cigar, len, maxm, name_id;
    std::vector<uint32_t> cigar;
    std::vector<int64_t> off;
    std::vector<uint8_t> seq, qual;
    std::vector<std::string_view> qname;   // into the text, or into `own`
    std::deque<std::string> own;           // qnames that were unescaped
    std::vector<std::string> unknown;      // rnames outside @SQ, first seen first: name_id -1 - k
    bool short_row = false;
};

void parse_block(Block &B, const char *p, const char *end, const int *col, int ncol,
                 const std::unordered_map<std::string, int> &refidx)
{
    std::vector<std::string_view> f;
    std::deque<std::string> scratch;
    std::vector<uint32_t> ops;
    std::unordered_map<std::string, int> unknown;
    std::string last_rname;
    int last_id = 0;
    bool have_last = false;
    B.flag.reserve((size_t)((end - p) / 500 + 16));
    while (csv_views(p, end, f, scratch)) {
        if (f.size() == 1 && f[0].empty()) continue;   // blank line: DictReader skips it
        if ((int)f.size() < ncol) { B.short_row = true; return; }
        // rows come grouped by rname: look a name up only when it changes
        if (!have_last || f[(size_t)col[2]] != last_rname) {
            last_rname.assign(f[(size_t)col[2]]);
            have_last = true;
            const auto it = refidx.find(last_rname);
            if (it != refidx.end()) {
                last_id = it->second;
            } else {
                const auto u = unknown.emplace(last_rname, (int)B.unknown.size());
                if (u.second) B.unknown.push_back(last_rname);
                last_id = -1 - u.first->second;
            }
        }
        const int flag = sv_atoi(f[(size_t)col[1]]);
        int maxm = 0;
        ops.clear();
        // an invalid or over-long CIGAR is the single op 3: it fails if it is used
        if (!(flag & 4) && (!parse_cigar_ops(f[(size_t)col[5]], ops, maxm) || ops.size() > MH_MAXOPS))
            ops.assign(1, 3u);
        B.cig_off.push_back((int32_t)B.cigar.size());
        B.cigar.insert(B.cigar.end(), ops.begin(), ops.end());
        B.n_cigar.push_back((int32_t)ops.size());
        B.flag.push_back(flag);
        B.ref.push_back(last_id < 0 ? -1 : last_id);
        B.name_id.push_back(last_id);
        B.pos.push_back(sv_atoi(f[(size_t)col[3]]));
        B.maxm.push_back(maxm);
        const std::string_view seq = f[(size_t)col[9]], qual = f[(size_t)col[10]];
        B.off.push_back((int64_t)B.seq.size());
        B.len.push_back((int32_t)seq.size());
        B.seq.insert(B.seq.end(), seq.begin(), seq.end());
        const size_t nq = std::min(qual.size(), seq.size());
        B.qual.insert(B.qual.end(), qual.begin(), qual.begin() + nq);
        B.qual.insert(B.qual.end(), seq.size() - nq, (uint8_t)'J');
        const std::string_view qname = f[(size_t)col[0]];
        const size_t k = (size_t)col[0];
        if (k < scratch.size() && qname.data() == scratch[k].data()) {   // unescaped: scratch is reused
            B.own.emplace_back(qname);
            B.qname.emplace_back(B.own.back());
        } else {
            B.qname.push_back(qname);
        }
    }
}

template <class T>
void place(std::vector<T> &dst, const std::vector<T> &src, int64_t at)
{
    std::copy(src.begin(), src.end(), dst.begin() + at);
}

}  // namespace

int prelim_parse(const char *text, int64_t len, int n_refs, const char *const *refnames, int threads,
                 PrelimRows &R, std::string &err)
{
    R = PrelimRows{};
    std::unordered_map<std::string, int> refidx;
    for (int r = 0; r < n_refs; ++r) refidx.emplace(refnames[r], r);
    const char *p = text, *end = text + (len > 0 ? len : 0);
    std::vector<std::string> head;
    if (!csv_record(p, end, head)) { err = "prelim csv: empty"; return -3; }
    static const char *const want[11] = {"qname", "flag", "rname", "pos", "mapq", "cigar", "rnext",
                                         "pnext", "tlen", "seq", "qual"};
    int col[11], ncol = 11;   // fields a row needs: up to the last column used
    csv_columns(head, want, 11, col);
    for (int k = 0; k < 11; ++k) {
        if (col[k] < 0) { err = std::string("prelim csv: missing column ") + want[k]; return -3; }
        ncol = std::max(ncol, col[k] + 1);
    }
    // rows parsed on host threads in blocks cut at record ends, placed in order
    const int nt = threads > 0 ? threads : std::max(1, std::min(s2a_threads(), (int)((end - p) >> 22) + 1));
    const std::vector<const char *> cut = csv_cuts(p, end, nt);
    std::vector<Block> part((size_t)nt);
    par_for(nt, [&](int t) { parse_block(part[(size_t)t], cut[(size_t)t], cut[(size_t)t + 1], col, ncol, refidx); });
    std::vector<int64_t> rb((size_t)nt + 1, 0), cb((size_t)nt + 1, 0), sb((size_t)nt + 1, 0);
    std::unordered_map<std::string, int> unknown;   // ids in first-seen order over the file
    for (int t = 0; t < nt; ++t) {
        Block &B = part[(size_t)t];
        if (B.short_row) { err = "prelim csv: short row"; return -3; }
        rb[(size_t)t + 1] = rb[(size_t)t] + (int64_t)B.flag.size();
        cb[(size_t)t + 1] = cb[(size_t)t] + (int64_t)B.cigar.size();
        sb[(size_t)t + 1] = sb[(size_t)t] + (int64_t)B.seq.size();
        std::vector<int> global;
        for (const std::string &u : B.unknown) {
            const auto g = unknown.emplace(u, (int)R.unknown.size());
            if (g.second) R.unknown.push_back(u);
            global.push_back(g.first->second);
        }
        for (int32_t &id : B.name_id)
            if (id < 0) id = -1 - global[(size_t)(-1 - id)];
    }
    const int64_t nr = rb[(size_t)nt];
    std::vector<int32_t> ref((size_t)nr), maxm((size_t)nr), name_id((size_t)nr);
    std::vector<std::string_view> qname((size_t)nr);
    R.flag.resize((size_t)nr); R.pos.resize((size_t)nr); R.cig_off.resize((size_t)nr);
    R.n_cigar.resize((size_t)nr); R.len.resize((size_t)nr); R.off.resize((size_t)nr);
    R.cigar.resize((size_t)cb[(size_t)nt]); R.seq.resize((size_t)sb[(size_t)nt]);
    R.qual.resize((size_t)sb[(size_t)nt]);
    par_for(nt, [&](int t) {
        const Block &B = part[(size_t)t];
        const int64_t r0 = rb[(size_t)t], c0 = cb[(size_t)t], s0 = sb[(size_t)t];
        place(R.flag, B.flag, r0); place(ref, B.ref, r0); place(R.pos, B.pos, r0);
        place(R.n_cigar, B.n_cigar, r0); place(maxm, B.maxm, r0); place(name_id, B.name_id, r0);
        place(R.len, B.len, r0); place(qname, B.qname, r0);
        place(R.cigar, B.cigar, c0); place(R.seq, B.seq, s0); place(R.qual, B.qual, s0);
        for (size_t i = 0; i < B.flag.size(); ++i) {
            R.cig_off[(size_t)r0 + i] = B.cig_off[i] + (int32_t)c0;
            R.off[(size_t)r0 + i] = B.off[i] + s0;
        }
    });
    matchmake(nr, [&](int64_t row) { return qname[(size_t)row]; },
              [&](int64_t row) { return ref[(size_t)row] >= 0; }, R.units);
    // compact reference ids: only references some unit row names, in @SQ
    // order (keeps the dense counters small); rows outside @SQ are never
    // paired and get compact id 0 (unused)
    std::vector<int32_t> compact((size_t)(n_refs > 0 ? n_refs : 1), -1);
    for (const int64_t row : R.units)
        if (row >= 0) compact[(size_t)ref[(size_t)row]] = 0;
    for (int r = 0; r < n_refs; ++r)
        if (compact[(size_t)r] == 0) { compact[(size_t)r] = (int32_t)R.present.size(); R.present.push_back(r); }
    R.ref.resize((size_t)nr);
    R.info.resize(4 * (size_t)nr);
    for (size_t i = 0; i < (size_t)nr; ++i) {
        R.ref[i] = ref[i] >= 0 && compact[(size_t)ref[i]] >= 0 ? compact[(size_t)ref[i]] : 0;
        R.info[4 * i] = name_id[i];
        R.info[4 * i + 1] = R.flag[i];
        R.info[4 * i + 2] = maxm[i];
        R.info[4 * i + 3] = R.ref[i];
    }
    return 0;
}

}  // namespace mh

extern "C" int mh_prelim_parse(const char *text, int64_t len, int n_refs, const char *const *refnames,
                               int threads, mh_prelim_sizes *sizes, int32_t *flag, int32_t *ref,
                               int32_t *pos, int32_t *cigar_off, int32_t *n_cigar, uint32_t *cigar,
                               int64_t *seq_off, int32_t *seq_len, uint8_t *seq, uint8_t *qual,
                               int64_t *units, int32_t *info, int32_t *present, char *unknown)
{
    if ((!text && len > 0) || len < 0 || n_refs < 0 || (n_refs > 0 && !refnames) || threads < 0 || !sizes)
        return -3;
    mh::PrelimRows R;
    std::string err;
    if (int st = mh::prelim_parse(text, len, n_refs, refnames, threads, R, err)) {
        mh::set_error("%s", err.c_str());
        return st;
    }
    std::string all;
    for (const std::string &u : R.unknown) { all += u; all.push_back('\n'); }
    sizes->n_rows = (int64_t)R.flag.size();
    sizes->n_units = (int64_t)R.units.size() / 2;
    sizes->n_cigar = (int64_t)R.cigar.size();
    sizes->n_bases = (int64_t)R.seq.size();
    sizes->n_present = (int32_t)R.present.size();
    sizes->unknown_bytes = all.size();
    if (!flag || !ref || !pos || !cigar_off || !n_cigar || !cigar || !seq_off || !seq_len || !seq ||
        !qual || !units || !info || !present || !unknown)
        return 0;
    auto put = [](void *dst, const void *src, size_t bytes) { if (bytes) std::memcpy(dst, src, bytes); };
    const size_t n = R.flag.size();
    put(flag, R.flag.data(), 4 * n);
    put(ref, R.ref.data(), 4 * n);
    put(pos, R.pos.data(), 4 * n);
    put(cigar_off, R.cig_off.data(), 4 * n);
    put(n_cigar, R.n_cigar.data(), 4 * n);
    put(cigar, R.cigar.data(), 4 * R.cigar.size());
    put(seq_off, R.off.data(), 8 * n);
    put(seq_len, R.len.data(), 4 * n);
    put(seq, R.seq.data(), R.seq.size());
    put(qual, R.qual.data(), R.qual.size());
    put(units, R.units.data(), 8 * R.units.size());
    put(info, R.info.data(), 4 * R.info.size());
    put(present, R.present.data(), 4 * R.present.size());
    put(unknown, all.data(), all.size());
    unknown[all.size()] = 0;
    return 0;
}
