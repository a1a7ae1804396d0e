// csv_readers_main.cpp -- stand-alone check of the CSV reader (mh_csv.h) and
// the prelim.csv parse (mh_prelim.cpp), built by test_csv_readers_host.py
// with mh_prelim.cpp, mh_sam.cpp, mh_gunzip.cpp and mh_pinflate.cpp under
// AddressSanitizer + UBSan and under ThreadSanitizer.
//   csv_readers texts FILE...   csv_cuts for 1 .. 8 blocks: every cut is a
//                               record start of a serial csv_record walk;
//                               prelim_parse with 1 .. 8 threads: one result
//   csv_readers truncate FILE LO HI   prelim_parse with 1 .. 8 threads over
//                               FILE cut at every byte offset in [LO, HI): any
//                               result or error is accepted
//   csv_readers pyint TEXT...   py_int of each argument: "ok <value>" or "no"
// Exits 0 when every check holds, else prints the failed checks and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "mh_prelim.h"
#include "mh_text.h"

namespace mh {
void set_error(const char *, ...) {}   // mh_api.cpp's, not linked here
}

static int failures = 0;
#define CHECK(cond, what)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: failed: %s (%s)\n", __FILE__, __LINE__, #cond, what); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static const char *const REFS[] = {"refA", "refB"};

static std::string slurp(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

static bool same(const mh::PrelimRows &a, const mh::PrelimRows &b)
{
    return a.flag == b.flag && a.ref == b.ref && a.pos == b.pos && a.cig_off == b.cig_off &&
           a.n_cigar == b.n_cigar && a.len == b.len && a.cigar == b.cigar && a.off == b.off &&
           a.seq == b.seq && a.qual == b.qual && a.units == b.units && a.info == b.info &&
           a.present == b.present && a.unknown == b.unknown;
}

static void check_text(const char *path)
{
    const std::string text = slurp(path);
    const char *p = text.data(), *end = p + text.size();
    std::vector<std::string> f;
    std::set<const char *> starts;   // of the body's records, and its end
    if (mh::csv_record(p, end, f)) {
        const char *q = p;
        do starts.insert(q); while (mh::csv_record(q, end, f));
        starts.insert(end);
        for (int nt = 1; nt <= 8; ++nt) {
            const std::vector<const char *> cut = mh::csv_cuts(p, end, nt);
            CHECK(cut.size() == (size_t)nt + 1 && cut.front() == p && cut.back() == end, path);
            for (size_t t = 0; t < cut.size(); ++t) {
                CHECK(starts.count(cut[t]) == 1, path);
                CHECK(t == 0 || cut[t - 1] <= cut[t], path);
            }
        }
    }
    mh::PrelimRows first;
    std::string first_err;
    const int first_st = mh::prelim_parse(text.data(), (int64_t)text.size(), 2, REFS, 1, first, first_err);
    for (int threads = 2; threads <= 8; ++threads) {
        mh::PrelimRows R;
        std::string err;
        const int st = mh::prelim_parse(text.data(), (int64_t)text.size(), 2, REFS, threads, R, err);
        CHECK(st == first_st && err == first_err, path);
        CHECK(st != 0 || same(R, first), path);
    }
}

static void check_truncated(const char *path, size_t lo, size_t hi)
{
    const std::string text = slurp(path);
    const char *const refs[] = {"HIV1B-pol-seed"};
    CHECK(lo < hi && hi <= text.size() + 1, path);
    for (size_t n = lo; n < hi && n <= text.size(); ++n) {
        // an exact-size copy: a read past the cut is a read past the buffer
        std::vector<char> part(text.begin(), text.begin() + (long)n);
        for (int threads = 1; threads <= 8; ++threads) {
            mh::PrelimRows R;
            std::string err;
            const int st = mh::prelim_parse(part.data(), (int64_t)n, 1, refs, threads, R, err);
            CHECK(st == 0 || st == -3, path);
        }
    }
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "pyint") {
        for (int k = 2; k < argc; ++k) {
            int64_t v = 0;
            if (mh::py_int(argv[k], v)) std::printf("ok %lld\n", (long long)v);
            else std::puts("no");
        }
        return 0;
    }
    if (mode != "texts" && mode != "truncate") {
        std::fprintf(stderr, "usage: csv_readers texts|truncate|pyint ...\n");
        return 2;
    }
    if (mode == "truncate" && argc == 5)
        check_truncated(argv[2], (size_t)std::atol(argv[3]), (size_t)std::atol(argv[4]));
    else if (mode == "truncate")
        ++failures;
    else
        for (int k = 2; k < argc; ++k) check_text(argv[k]);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("csv_readers ok");
    return 0;
}
