// mh_text.h -- host-side text helpers shared by the C-ABI translation units:
// CIGAR strings as sam2aln.apply_cigar accepts them and csv.writer's
// QUOTE_MINIMAL fields; the CSV reader is mh_csv.h (included here).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "mh_csv.h"
#include "micall_hip.h"

namespace mh {

inline bool parse_cigar_ops(std::string_view c, std::vector<uint32_t> &ops, int &maxm)
{
    // ^((\d+)([MIDNSHPX=]))*$ ; only M/I/D/S are usable (sam2aln.py:113-142)
    ops.clear();
    maxm = 0;
    size_t i = 0;
    while (i < c.size()) {
        size_t j = i;
        uint64_t n = 0;
        while (j < c.size() && c[j] >= '0' && c[j] <= '9') { n = n * 10 + (c[j] - '0'); ++j; }
        if (j == i || j >= c.size()) return false;
        const char op = c[j];
        uint32_t code;
        switch (op) {
        case 'M': code = MH_OP_M; if ((int)n > maxm) maxm = (int)n; break;
        case 'I': code = MH_OP_I; break;
        case 'D': code = MH_OP_D; break;
        case 'S': code = MH_OP_S; break;
        case 'N': case 'H': case 'P': case 'X': case '=': code = 3; break;  // unsupported
        default: return false;
        }
        ops.push_back(((uint32_t)n << 4) | code);
        i = j + 1;
    }
    return true;
}

// csv.writer QUOTE_MINIMAL: quote a field holding ',', '"', '\n' or '\r'.
inline void csv_field(std::string &out, const char *s, size_t n)
{
    bool quote = false;
    for (size_t i = 0; i < n; ++i)
        if (s[i] == ',' || s[i] == '"' || s[i] == '\n' || s[i] == '\r') { quote = true; break; }
    if (!quote) { out.append(s, n); return; }
    out.push_back('"');
    for (size_t i = 0; i < n; ++i) {
        if (s[i] == '"') out.push_back('"');
        out.push_back(s[i]);
    }
    out.push_back('"');
}

}  // namespace mh
