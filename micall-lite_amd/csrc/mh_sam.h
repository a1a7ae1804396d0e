// mh_sam.h -- SAM text as remap.matchmaker(samfile, include_singles=True)
// reads it (micall/core/remap.py:853-889), parsed on the host into the rows
// mh_rows_load takes.  No device part (mh_sam.cpp is plain C++).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace mh {

struct SamRows {
    // kept rows (RNAME an @SQ name), numbered in unit order
    std::vector<int32_t> flag, ref, pos, cig_off, n_cigar, len;
    std::vector<uint32_t> cigar;
    std::vector<int64_t> off;
    std::vector<uint8_t> seq, qual;
    std::vector<int64_t> units;          // pairs of row indices, -1: no mate
    std::vector<std::string> names;      // @SQ SN values in first-seen order
    std::vector<int32_t> ends;           // per name: largest reference end of a mapped row
};

// 0, or -3 with `err` naming the line (1-based) the reference would raise on
int sam_parse(const char *text, int64_t len, SamRows &R, std::string &err);

}  // namespace mh
