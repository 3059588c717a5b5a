// The check of a HOST chain table in front of cvs_chain_joins (joins_host_table_wrong, cvs_joins.h) as a stand-alone program: built by
// tests/test_joins_cpu.py with -fsanitize=address,undefined and run over valid and broken tables that lie on the heap at exactly their
// size, so that a read past a table ends the program.  No HIP, no library.  Prints "joins host table OK" and exits 0.
#define CVS_JOINS_HOST_ONLY
#include "cvs_joins.h"

#include <climits>
#include <cstdio>
#include <vector>

namespace {

struct Entry {
    int32_t start, length, flags, reserved;
};

// the verdict on a table that is copied to a heap block of exactly its size first
bool refused(int n_points, const std::vector<Entry>& t)
{
    std::vector<int32_t> words;
    words.reserve(t.size() * 4);
    for (const Entry& e : t) {
        words.push_back(e.start);
        words.push_back(e.length);
        words.push_back(e.flags);
        words.push_back(e.reserved);
    }
    words.shrink_to_fit();
    return cvs::joins_host_table_wrong(n_points, words.empty() ? nullptr : words.data(), (int)t.size()) != nullptr;
}

int failures = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

}  // namespace

int main()
{
    const std::vector<Entry> good = {{0, 3, 0, 0}, {3, 1, 1, 0}, {4, 5, 0, 7}};   // `reserved` and the flags are not looked at
    expect(!refused(9, good), "a table that is the running sum");
    expect(!refused(0, {}), "no points, no chains");
    expect(refused(5, {}), "points without a chain");
    expect(refused(10, good), "lengths that stop short of n_points");
    expect(refused(8, good), "lengths that pass n_points");
    expect(refused(0, good), "chains without points");
    for (int c = 0; c < 3; ++c) {
        std::vector<Entry> t = good;
        t[(size_t)c].start += 1;
        expect(refused(9, t), "a start one too far");
        t = good;
        t[(size_t)c].start -= 1;
        expect(refused(9, t), "a start one too near");
        t = good;
        t[(size_t)c].length = 0;
        expect(refused(9, t), "an empty chain");
        t = good;
        t[(size_t)c].length = -t[(size_t)c].length;
        expect(refused(9, t), "a negative length");
    }
    // sums that would not fit 32 bits are added as 64-bit values
    expect(refused(INT_MAX, {{0, INT_MAX, 0, 0}, {INT_MAX, INT_MAX, 0, 0}}), "lengths whose sum passes 2^31");
    expect(!refused(INT_MAX, {{0, INT_MAX, 0, 0}}), "one chain of 2^31 - 1 points");
    expect(refused(INT_MAX, {{0, INT_MAX - 1, 0, 0}, {INT_MIN, 1, 0, 0}}), "a start of INT_MIN");
    // a long table
    std::vector<Entry> many;
    for (int c = 0; c < 100000; ++c) many.push_back({2 * c, 2, c & 1, 0});
    expect(!refused(200000, many), "a hundred thousand chains");
    many[99999].length = 3;
    expect(refused(200000, many), "the last chain of a hundred thousand one too long");
    // the hash table of the nodes: a power of two of slots, at least 4 per chain (2 per end), fewer than 8 per chain beyond two chains
    for (int n : {1, 2, 3, 4, 5, 1000, 65536, 65537, cvs::kJoinMaxChains - 1, cvs::kJoinMaxChains}) {
        const size_t s = cvs::join_slots(n);
        expect((s & (s - 1)) == 0 && s >= 8 && s >= 4 * (size_t)n && (s == 8 || s < 8 * (size_t)n), "the slots of the node table");
        expect(cvs::join_scratch_bytes(n) == 112 * (size_t)n + 16 * s && cvs::join_scratch_bytes(n) <= 240 * (size_t)n, "the scratch of a call");
    }
    if (failures) return 1;
    std::printf("joins host table OK\n");
    return 0;
}
