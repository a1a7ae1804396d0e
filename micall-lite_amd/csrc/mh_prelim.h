// mh_prelim.h -- prelim.csv text (prelim_map.py:142-151) as remap() reads it
// back (remap.py:474-498), parsed on the host into the rows mh_rows_load
// takes.  No device part (mh_prelim.cpp is plain C++).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace mh {

struct PrelimRows {
    // every data row, in file order; ref is the compact reference id
    std::vector<int32_t> flag, ref, pos, cig_off, n_cigar, len;
    std::vector<uint32_t> cigar;
    std::vector<int64_t> off;
    std::vector<uint8_t> seq, qual;      // qual cut or padded with 'J' to seq's length
    std::vector<int64_t> units;          // pairs of row indices, -1: no mate
    // what mh_rows_info hands back
    std::vector<int32_t> info;           // per row: name id, flag, longest M run, compact ref id
    std::vector<int32_t> present;        // compact ref id -> index into refnames
    std::vector<std::string> unknown;    // rnames outside refnames, in first-seen order
};

// 0, or -3 with `err`.  threads: host threads (blocks of the text), 0 for the
// default; the result is the same for any count.
int prelim_parse(const char *text, int64_t len, int n_refs, const char *const *refnames, int threads,
                 PrelimRows &R, std::string &err);

}  // namespace mh
