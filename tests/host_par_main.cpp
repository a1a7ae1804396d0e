// host_par_main.cpp -- stand-alone check of the host helpers of mh_gunzip.h
// (par_for, write_all_at, read_all_at), built by test_host_par.py with
// mh_gunzip.cpp and mh_pinflate.cpp under AddressSanitizer + UBSan and under
// ThreadSanitizer.  Exits 0 when every check holds, else prints the failed
// checks and exits 1.
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <thread>
#include <vector>

#include "mh_gunzip.h"

namespace mh {
void set_error(const char *, ...) {}   // mh_api.cpp's, not linked here
}

using mh::par_for;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void check_par_for()
{
    {   // one thread: index 0, on the caller
        const std::thread::id me = std::this_thread::get_id();
        int calls = 0, index = -1;
        std::thread::id ran;
        par_for(1, [&](int t) { ++calls; index = t; ran = std::this_thread::get_id(); });
        CHECK(calls == 1 && index == 0 && ran == me);
    }
    {   // eight threads: every index exactly once
        std::vector<std::atomic<int>> hits(8);
        for (auto &h : hits) h = 0;
        par_for(8, [&](int t) { ++hits[(size_t)t]; });
        for (auto &h : hits) CHECK(h == 1);
    }
    {   // index 3 throws bad_alloc: rethrown here, after the other seven ended
        std::atomic<int> completed(0);
        bool caught = false;
        int seen = -1;
        try {
            par_for(8, [&](int t) {
                if (t == 3) throw std::bad_alloc();
                // long enough that a rethrow before the join would see fewer
                std::this_thread::sleep_for(std::chrono::milliseconds(20));
                ++completed;
            });
        } catch (const std::bad_alloc &) {
            caught = true;
            seen = completed.load();
        }
        CHECK(caught);
        CHECK(seen == 7);
    }
    {   // two indices throw different types: one of the two arrives
        int kind = 0;
        try {
            par_for(8, [&](int t) {
                if (t == 2) throw std::runtime_error("two");
                if (t == 5) throw std::out_of_range("five");
            });
        } catch (const std::out_of_range &) {
            kind = 5;
        } catch (const std::runtime_error &) {
            kind = 2;
        } catch (...) {
            kind = -1;
        }
        CHECK(kind == 2 || kind == 5);
    }
    {   // nested: every inner index of every outer worker runs
        std::atomic<int> inner(0);
        par_for(4, [&](int) { par_for(4, [&](int) { ++inner; }); });
        CHECK(inner == 16);
    }
}

static void check_io()
{
    char path[] = "/tmp/host_par_XXXXXX";
    const int fd = mkstemp(path);
    CHECK(fd >= 0);
    if (fd < 0) return;
    unlink(path);
    const size_t n = ((size_t)9 << 20) + 1;
    const int64_t off = 4097;
    std::vector<unsigned char> a(n), b(n, 0);
    uint32_t x = 12345;
    for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; a[i] = (unsigned char)(x >> 24); }
    CHECK(mh::write_all_at(fd, a.data(), n, off) == 0);
    CHECK(lseek(fd, 0, SEEK_END) == (off_t)(off + (int64_t)n));
    CHECK(mh::read_all_at(fd, b.data(), n, off) == 0);
    CHECK(a == b);
    CHECK(mh::read_all_at(fd, b.data(), n, off + 1) != 0);   // one byte short: an error
    CHECK(mh::write_all_at(fd, a.data(), 0, off) == 0);
    close(fd);
    CHECK(mh::write_all_at(fd, a.data(), 16, 0) != 0);       // closed descriptor
    CHECK(mh::read_all_at(fd, b.data(), 16, 0) != 0);
}

int main()
{
    check_par_for();
    check_io();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("host_par ok");
    return 0;
}
