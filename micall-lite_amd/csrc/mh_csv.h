// mh_csv.h -- the one reader of the csv-module dialect MiCall's files use
// (csv.DictReader over DictWriter's QUOTE_MINIMAL output): header columns,
// one record as views, block cuts at record ends, Python's int(), and
// remap.matchmaker.  prelim.csv, remap.csv and aligned.csv are all read with
// these; plain C++ and HIP translation units both include it.
#pragma once
#include <stdint.h>

#include <cstring>
#include <deque>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "mh_gunzip.h"

namespace mh {

// One CSV record as views into the text.  A quoted field that needs no
// unescaping is a view too; one with "" escapes, or with text after its
// closing quote (appended, as csv does), is built in scratch[k], k its
// field index.  '\r', '\n' and '\r\n' all end a record.  False at the end
// of the text.
inline bool csv_views(const char *&p, const char *end, std::vector<std::string_view> &f,
                      std::deque<std::string> &scratch)
{
    f.clear();
    if (p >= end) return false;
    auto ends_field = [&](const char *q) { return q == end || *q == ',' || *q == '\n' || *q == '\r'; };
    for (;;) {
        const char *close = nullptr;
        if (*p == '"' && p + 1 < end) close = (const char *)std::memchr(p + 1, '"', (size_t)(end - p - 1));
        if (close && ends_field(close + 1)) {
            f.emplace_back(p + 1, (size_t)(close - p - 1));
            p = close + 1;
        } else if (*p == '"') {
            if (scratch.size() <= f.size()) scratch.resize(f.size() + 1);
            std::string &s = scratch[f.size()];
            s.clear();
            ++p;
            while (p < end) {
                if (*p == '"') {
                    if (p + 1 < end && p[1] == '"') { s.push_back('"'); p += 2; continue; }
                    ++p;
                    break;
                }
                s.push_back(*p++);
            }
            while (!ends_field(p)) s.push_back(*p++);
            f.emplace_back(s);
        } else {
            const char *q = p;
            while (!ends_field(p)) ++p;
            f.emplace_back(q, (size_t)(p - q));
        }
        if (p < end && *p == ',') {
            if (++p < end) continue;
            f.emplace_back(p, (size_t)0);   // the text ends after a comma: one more, empty field
            return true;
        }
        if (p < end && *p == '\r') ++p;
        if (p < end && *p == '\n') ++p;
        return true;
    }
}

// One record as owned strings (header rows).
inline bool csv_record(const char *&p, const char *end, std::vector<std::string> &f)
{
    std::vector<std::string_view> v;
    std::deque<std::string> scratch;
    f.clear();
    if (!csv_views(p, end, v, scratch)) return false;
    f.assign(v.begin(), v.end());
    return true;
}

// DictReader's column of each wanted name: the last duplicate wins, -1 when
// the header does not have it (the caller decides what that means).
inline void csv_columns(const std::vector<std::string> &head, const char *const *want, int n, int *col)
{
    for (int k = 0; k < n; ++k) {
        col[k] = -1;
        for (size_t z = 0; z < head.size(); ++z)
            if (head[z] == want[k]) col[k] = (int)z;
    }
}

// nt + 1 record starts that cut [p, end) into nt blocks for host threads:
// each cut follows the first '\n' at or after the even split.  The quotes
// before a cut are counted (par_for, one block per thread); a cut with an
// odd count lies inside a quoted field and moves on to the end of that
// record.  Cuts are monotone and a block may be empty.  (As csv.writer never
// leaves a lone '"' inside an unquoted field, parity decides.)
inline std::vector<const char *> csv_cuts(const char *p, const char *end, int nt)
{
    if (nt < 1) nt = 1;
    std::vector<const char *> cut((size_t)nt + 1, p);
    cut[(size_t)nt] = end;
    const int64_t bytes = end - p;
    for (int t = 1; t < nt; ++t) {
        const char *q = p + bytes * t / nt;
        const char *nl = (const char *)std::memchr(q, '\n', (size_t)(end - q));
        cut[(size_t)t] = nl ? nl + 1 : end;
    }
    std::vector<int64_t> quotes((size_t)nt, 0);
    par_for(nt, [&](int t) {
        int64_t n = 0;
        for (const char *q = cut[(size_t)t]; q < cut[(size_t)t + 1]; ++q) n += *q == '"';
        quotes[(size_t)t] = n;
    });
    int64_t before = 0;   // quotes in [p, the even split's cut t)
    for (int t = 1; t < nt; ++t) {
        before += quotes[(size_t)t - 1];
        const char *q = cut[(size_t)t];
        if (q < cut[(size_t)t - 1]) { cut[(size_t)t] = cut[(size_t)t - 1]; continue; }   // behind a moved cut
        if (!(before & 1)) continue;
        int64_t seen = before;
        while (q < end && !(*q == '\n' && !(seen & 1))) seen += *q++ == '"';
        cut[(size_t)t] = q < end ? q + 1 : end;
    }
    return cut;
}

// Python's int() on a field: the six ASCII blanks stripped at both ends, one
// optional sign, decimal digits only ('1_2' is refused, which int() takes);
// false when it is no integer or does not fit int64.  Callers check ranges.
inline bool py_int(std::string_view v, int64_t &out)
{
    auto blank = [](char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); };
    size_t a = 0, b = v.size();
    while (a < b && blank(v[a])) ++a;
    while (b > a && blank(v[b - 1])) --b;
    bool neg = false;
    if (a < b && (v[a] == '-' || v[a] == '+')) neg = v[a++] == '-';
    if (a == b) return false;
    int64_t x = 0;
    for (; a < b; ++a) {
        if (v[a] < '0' || v[a] > '9') return false;
        const int d = v[a] - '0';
        if (x > (INT64_MAX - d) / 10) return false;
        x = x * 10 + d;
    }
    out = neg ? -x : x;
    return true;
}

inline bool py_int32(std::string_view v, int32_t &out)
{
    int64_t x = 0;
    if (!py_int(v, x) || x < INT32_MIN || x > INT32_MAX) return false;
    out = (int32_t)x;
    return true;
}

// C atoi() on a view, not int(): the prelim.csv reader is lenient on purpose
// (leading blanks and a sign, then digits up to the first other character).
inline int sv_atoi(std::string_view v)
{
    size_t i = 0;
    while (i < v.size() && (v[i] == ' ' || v[i] == '\t')) ++i;
    bool neg = false;
    if (i < v.size() && (v[i] == '-' || v[i] == '+')) neg = v[i++] == '-';
    long long x = 0;
    while (i < v.size() && v[i] >= '0' && v[i] <= '9') x = x * 10 + (v[i++] - '0');
    return (int)(neg ? -x : x);
}

// remap.matchmaker (remap.py:853-889) with include_singles=True over the
// rows keep(row) takes: a row whose qname is waiting pairs with the waiting
// row (appended as it completes), else it waits; the rows still waiting
// follow in their order, each with mate -1.
template <class QnameOf, class Keep>
void matchmake(int64_t n_rows, QnameOf qname_of, Keep keep, std::vector<int64_t> &units)
{
    std::unordered_map<std::string_view, int64_t> pending;   // qname -> slot in order
    std::vector<std::pair<int64_t, bool>> order;             // (row, still single)
    pending.reserve((size_t)n_rows);
    order.reserve((size_t)n_rows);
    for (int64_t row = 0; row < n_rows; ++row) {
        if (!keep(row)) continue;
        const std::string_view qname = qname_of(row);
        const auto hit = pending.find(qname);
        if (hit == pending.end()) {
            pending.emplace(qname, (int64_t)order.size());
            order.push_back({row, true});
        } else {
            order[(size_t)hit->second].second = false;
            units.push_back(order[(size_t)hit->second].first);
            units.push_back(row);
            pending.erase(hit);
        }
    }
    for (const auto &o : order)
        if (o.second) { units.push_back(o.first); units.push_back(-1); }
}

}  // namespace mh
