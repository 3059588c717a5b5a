// The rules of a HOST chain table (cvs_chain_table.h) as a stand-alone program: the running-sum rule in front of cvs_chain_turns and
// cvs_chain_joins, the inside-points rule in front of cvs_chain_polylines, cvs_chain_measures and cvs_polyline_segments, and the size of
// the join scratch.  Built by tests/test_joins_cpu.py with -fsanitize=address,undefined and run over valid and broken tables that lie on
// the heap at exactly their size, so that a read past a table ends the program.  No HIP, no library.  Prints "chain table OK" and exits 0.
#include "cvs_chain_table.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Entry {
    int32_t start, length, flags, reserved;
};

typedef const char* (*Rule)(int, const int32_t*, int);

// the verdict of a rule on a table that is copied to a heap block of exactly its size first
const char* verdict(Rule rule, int n_points, const std::vector<Entry>& t)
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
    return rule(n_points, words.empty() ? nullptr : words.data(), (int)t.size());
}
bool refused(int n_points, const std::vector<Entry>& t) { return verdict(cvs::chain_table_not_running_sum, n_points, t) != nullptr; }
bool outside(int n_points, const std::vector<Entry>& t)
{
    const char* what = verdict(cvs::chain_table_outside, n_points, t);
    return what && std::strcmp(what, "a chain does not lie inside points") == 0;
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
    // ---- the running-sum rule ----
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
    expect(std::strcmp(verdict(cvs::chain_table_not_running_sum, 9, {{0, 3, 0, 0}, {3, 0, 0, 0}}), "a chain has no point") == 0 &&
               std::strcmp(verdict(cvs::chain_table_not_running_sum, 9, {{0, 3, 0, 0}, {4, 6, 0, 0}}),
                           "the chain starts are not the running sum of the lengths") == 0 &&
               std::strcmp(verdict(cvs::chain_table_not_running_sum, 9, {{0, 3, 0, 0}, {3, 7, 0, 0}}), "the chains hold more points than n_points") == 0 &&
               std::strcmp(verdict(cvs::chain_table_not_running_sum, 9, {{0, 3, 0, 0}, {3, 5, 0, 0}}), "the chain lengths do not add up to n_points") == 0,
           "the texts of the running-sum rule");

    // ---- the inside-points rule: chains in any order, overlapping or with gaps, each inside 0 .. n_points ----
    const std::vector<Entry> loose = {{4, 5, 0, 7}, {0, 3, 1, 0}, {2, 1, 0, 0}};
    expect(verdict(cvs::chain_table_outside, 9, loose) == nullptr, "chains that lie inside points");
    expect(verdict(cvs::chain_table_outside, 9, good) == nullptr, "the running sum lies inside points");
    expect(verdict(cvs::chain_table_outside, 0, {}) == nullptr && verdict(cvs::chain_table_outside, 5, {}) == nullptr, "no chains");
    expect(outside(8, loose), "a start + length one past n_points");
    expect(outside(0, loose), "chains without points");
    for (int c = 0; c < 3; ++c) {
        std::vector<Entry> t = loose;
        t[(size_t)c].start = -1;
        expect(outside(9, t), "a start of -1");
        t = loose;
        t[(size_t)c].length = 0;
        expect(outside(9, t), "a length of 0");
        t = loose;
        t[(size_t)c].length = -t[(size_t)c].length;
        expect(outside(9, t), "a negative length");
        t = loose;
        t[(size_t)c].length = 9 - t[(size_t)c].start;
        expect(verdict(cvs::chain_table_outside, 9, t) == nullptr, "a chain that ends at n_points");
        t[(size_t)c].length += 1;
        expect(outside(9, t), "a chain that ends one past n_points");
    }
    // start + length is a 64-bit sum
    expect(outside(INT_MAX, {{INT_MAX, INT_MAX, 0, 0}}), "a start + length that passes 2^31");
    expect(outside(INT_MAX, {{1, INT_MAX, 0, 0}}), "a start + length of exactly 2^31");
    expect(verdict(cvs::chain_table_outside, INT_MAX, {{0, INT_MAX, 0, 0}, {INT_MAX - 1, 1, 0, 0}}) == nullptr, "chains up to 2^31 - 1");
    expect(outside(INT_MAX, {{INT_MIN, 1, 0, 0}}), "a start of INT_MIN");
    expect(outside(200000, many), "the last chain of a hundred thousand one too long");
    many[99999].length = 2;
    expect(verdict(cvs::chain_table_outside, 200000, many) == nullptr, "a hundred thousand chains inside points");
    many[99999].start += 1;
    expect(outside(200000, many), "the last chain of a hundred thousand one too far");

    // ---- the hash table of the join nodes: a power of two of slots, at least 4 per chain (2 per end), fewer than 8 per chain beyond two
    // chains ----
    const int kJoinMaxChains = 1 << 26;   // cvs_joins.h
    for (int n : {1, 2, 3, 4, 5, 1000, 65536, 65537, kJoinMaxChains - 1, kJoinMaxChains}) {
        const size_t s = cvs::join_slots(n);
        expect((s & (s - 1)) == 0 && s >= 8 && s >= 4 * (size_t)n && (s == 8 || s < 8 * (size_t)n), "the slots of the node table");
        expect(cvs::join_scratch_bytes(n) == 112 * (size_t)n + 16 * s && cvs::join_scratch_bytes(n) <= 240 * (size_t)n, "the scratch of a call");
    }
    if (failures) return 1;
    std::printf("chain table OK\n");
    return 0;
}
