// mh_sam.cpp -- SAM text to pileup rows on the host: remap.matchmaker
// (micall/core/remap.py:853-889) with include_singles=True, then the fields
// merge_reads uses (remap.py:86-126).  Plain C++, no device part: it is also
// compiled alone, with the sanitizers, by tests/test_debug_reports_host.py.
#include "mh_sam.h"

#include <cstdarg>
#include <cstring>
#include <string_view>
#include <unordered_map>

#include "mh_text.h"

namespace mh {

void set_error(const char *fmt, ...);

static int fail(std::string &err, int64_t line, const char *what)
{
    err = "SAM line " + std::to_string((long long)line) + ": " + what;
    return -3;
}

int sam_parse(const char *text, int64_t len, SamRows &R, std::string &err)
{
    R = SamRows{};
    struct Row {
        std::string_view qname, cigar, seq, qual;
        int32_t flag, ref, pos;
    };
    std::vector<Row> rows;                                   // kept rows in line order
    std::unordered_map<std::string_view, int32_t> refidx;    // views into text
    std::vector<int64_t> units;                              // row numbers in line order
    std::vector<std::string_view> f;
    const char *p = text, *end = text + (len > 0 ? len : 0);
    int64_t line_no = 0;
    while (p < end) {
        const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end;
        const std::string_view line(p, (size_t)(le - p));
        p = nl ? nl + 1 : end;
        ++line_no;
        f.clear();
        for (size_t a = 0;;) {
            const size_t t = line.find('\t', a);
            if (t == std::string_view::npos) { f.push_back(line.substr(a)); break; }
            f.push_back(line.substr(a, t - a));
            a = t + 1;
        }
        if (!line.empty() && line[0] == '@') {
            if (f[0] != "@SQ") continue;
            for (size_t k = 1; k < f.size(); ++k) {
                const size_t colon = f[k].find(':');
                if (colon == std::string_view::npos) return fail(err, line_no, "@SQ field without ':'");
                if (f[k].substr(0, colon) != "SN") continue;
                const std::string_view name = f[k].substr(colon + 1);
                if (refidx.emplace(name, (int32_t)R.names.size()).second) R.names.emplace_back(name);
            }
            continue;
        }
        if (f.size() < 3) return fail(err, line_no, "fewer than three fields");
        const auto hit = refidx.find(f[2]);
        if (hit == refidx.end()) continue;   // RNAME outside @SQ ('*' too): dropped
        if (f.size() < 11) return fail(err, line_no, "fewer than eleven fields");
        Row r;
        r.qname = f[0];
        r.ref = hit->second;
        if (!py_int32(f[1], r.flag)) return fail(err, line_no, "FLAG is not an integer");
        if (!py_int32(f[3], r.pos)) return fail(err, line_no, "POS is not an integer");
        r.cigar = f[5];
        r.seq = f[9];
        r.qual = f[10];
        rows.push_back(r);
    }
    matchmake((int64_t)rows.size(), [&](int64_t row) { return rows[(size_t)row].qname; },
              [](int64_t) { return true; }, units);
    // rows renumbered in unit order
    R.ends.assign(R.names.size(), 0);
    std::vector<uint32_t> ops;
    for (const int64_t src : units) {
        if (src < 0) { R.units.push_back(-1); continue; }
        const Row &r = rows[(size_t)src];
        R.units.push_back((int64_t)R.flag.size());
        R.flag.push_back(r.flag);
        R.ref.push_back(r.ref);
        R.pos.push_back(r.pos);
        R.cig_off.push_back((int32_t)R.cigar.size());
        int maxm = 0;
        ops.clear();
        if (!(r.flag & 4)) {
            if (!parse_cigar_ops(r.cigar, ops, maxm) || ops.size() > MH_MAXOPS) ops.assign(1, 3u);
            int64_t span = 0;
            for (const uint32_t w : ops)
                if ((w & 15) == MH_OP_M || (w & 15) == MH_OP_D) span += w >> 4;
            const int64_t e = (int64_t)r.pos - 1 + span;
            if (e > R.ends[(size_t)r.ref]) R.ends[(size_t)r.ref] = (int32_t)(e > INT32_MAX ? INT32_MAX : e);
        }
        R.n_cigar.push_back((int32_t)ops.size());
        R.cigar.insert(R.cigar.end(), ops.begin(), ops.end());
        R.off.push_back((int64_t)R.seq.size());
        R.len.push_back((int32_t)r.seq.size());
        R.seq.insert(R.seq.end(), r.seq.begin(), r.seq.end());
        const size_t nq = r.qual.size() < r.seq.size() ? r.qual.size() : r.seq.size();
        R.qual.insert(R.qual.end(), r.qual.begin(), r.qual.begin() + nq);
        R.qual.insert(R.qual.end(), r.seq.size() - nq, (uint8_t)'J');
    }
    return 0;
}

}  // namespace mh

extern "C" int mh_sam_parse(const char *text, int64_t len, mh_sam_sizes *sizes, int32_t *flag,
                            int32_t *ref, int32_t *pos, int32_t *cigar_off, int32_t *n_cigar,
                            uint32_t *cigar, int64_t *seq_off, int32_t *seq_len, uint8_t *seq,
                            uint8_t *qual, int64_t *units, char *names, int32_t *ends)
{
    if ((!text && len > 0) || len < 0 || !sizes) return -3;
    mh::SamRows R;
    std::string err;
    if (int st = mh::sam_parse(text, len, R, err)) {
        mh::set_error("%s", err.c_str());
        return st;
    }
    std::string all;
    for (const std::string &n : R.names) { all += n; all.push_back('\n'); }
    sizes->n_rows = (int64_t)R.flag.size();
    sizes->n_units = (int64_t)R.units.size() / 2;
    sizes->n_cigar = (int64_t)R.cigar.size();
    sizes->n_bases = (int64_t)R.seq.size();
    sizes->n_refs = (int32_t)R.names.size();
    sizes->names_bytes = all.size();
    if (!flag || !ref || !pos || !cigar_off || !n_cigar || !cigar || !seq_off || !seq_len || !seq ||
        !qual || !units || !names || !ends)
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
    put(names, all.data(), all.size());
    names[all.size()] = 0;
    put(ends, R.ends.data(), 4 * R.ends.size());
    return 0;
}
