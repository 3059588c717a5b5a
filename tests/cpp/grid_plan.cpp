// grid_plan.cpp -- every grid that follows the image height (cvsteer_amd/csrc/cvs_grid.h), swept on the CPU: no device, no HIP header.
//
//   grid_plan          checks the functions of cvs_grid.h; exit 0 = every requirement holds
//   grid_plan parent   checks the formulas the launchers had before cvs_grid.h existed (kept below as `parent_*`); they must NOT pass
//
// Requirements, for every function and every shape of three sets (the tall shapes of tests/test_gpu_tall.py, the image shapes of the
// legs tests/golden/timed_instances.json names, and seeded random (rows, cols) with rows * cols <= 2^31 - 2, rows up to 2^31 - 2):
//   y <= 65535 and z <= 65535;  x * 256 < 2^32;
//   every row, tile row, row group or strip is covered exactly once by (launch, block index, iteration) -- the kernels' own loops are
//   re-enacted here: every unit enumerated where there are at most 65536, the first and last eight units where there are more;
//   for the timed shapes the dimensions equal the parent's, so the benchmarked launches are the ones they were.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "cvs_grid.h"

using cvs::GridDims;

namespace {

int g_failed = 0, g_checked = 0;
std::string g_where;
const char* const kFamilies[] = {"generic_grid", "tile_grid", "pyr_down_grid", "nonmax_grid", "strip plan", "timed"};
int g_broken[6] = {0, 0, 0, 0, 0, 0};
bool g_print_all = false;   // the tall shapes report every broken requirement, the sweeps the first few

void fail(const char* what, long long a = 0, long long b = 0)
{
    for (int f = 0; f < 6; ++f)
        if (!g_where.compare(0, std::strlen(kFamilies[f]), kFamilies[f])) ++g_broken[f];
    if (++g_failed <= 40 || g_print_all) std::printf("FAIL %s: %s (%lld, %lld)\n", g_where.c_str(), what, a, b);
}

void bounds(const GridDims& g)
{
    ++g_checked;
    if (g.x < 1 || g.y < 1 || g.z < 1) fail("an empty grid", g.y, g.z);
    if (g.y > 65535u) fail("grid.y > 65535", g.y);
    if (g.z > 65535u) fail("grid.z > 65535", g.z);
    if ((unsigned long long)g.x * 256ull >= (1ull << 32)) fail("grid.x * 256 >= 2^32", g.x);
}

// the loop `for (t = blockIdx.y; t < n; t += gridDim.y)` over a grid of Y rows of workgroups: every t in [0, n) exactly once
void stride_cover(long long n, unsigned Y)
{
    if (Y < 1) return fail("no workgroup row");
    if ((long long)Y > n) fail("workgroup rows without a unit", Y, n);
    if (n <= (1 << 16)) {
        std::vector<unsigned char> seen((size_t)n, 0);
        for (unsigned b = 0; b < Y; ++b)
            for (long long t = b; t < n; t += Y) ++seen[(size_t)t];
        for (long long t = 0; t < n; ++t)
            if (seen[(size_t)t] != 1) return fail("unit not covered exactly once", t, seen[(size_t)t]);
        return;
    }
    // too many units to mark them all: the kernel's own loop is run for the workgroup rows that own the first and the last eight units,
    // and those sixteen units must each be met exactly once; in between, the loop of any row b meets b, b + Y, ... and nothing else
    // (arithmetic, not enumerated: a plain stride cannot do otherwise)
    constexpr long long kWin = 8;
    int seen[2 * kWin] = {0};
    std::vector<unsigned> owners;
    for (long long t = 0; t < kWin; ++t) {
        owners.push_back((unsigned)(t % Y));
        owners.push_back((unsigned)((n - 1 - t) % Y));
    }
    std::sort(owners.begin(), owners.end());
    owners.erase(std::unique(owners.begin(), owners.end()), owners.end());
    for (unsigned blk : owners) {
        long long iters = 0, last = -1;
        for (long long t = blk; t < n; t += Y) {   // for (t = blockIdx.y; t < n; t += gridDim.y)
            if (t < kWin) ++seen[t];
            if (t >= n - kWin) ++seen[kWin + (t - (n - kWin))];
            ++iters;
            last = t;
        }
        if (iters != (n - blk + Y - 1) / Y || last < 0 || last + (long long)Y < n) fail("a workgroup row stops short", blk, iters);
    }
    for (int i = 0; i < 2 * kWin; ++i)
        if (seen[i] != 1) fail("an end unit not covered exactly once", i, seen[i]);
}

// one block per unit and no loop (the parent's launchers, and nonmax): every unit exactly once iff the grid has exactly n rows of workgroups
void direct_cover(long long n, unsigned Y)
{
    if ((long long)Y != n) fail("workgroup rows != units", Y, n);
}

// ---- what the launchers computed before cvs_grid.h: the parent's formulas as they stood in the launchers, but in 64 bits, so that the
// sweep itself stays defined at the largest heights (rows + 31 does not fit an int there) ----
GridDims parent_generic(long long rows, long long cols) { return {(unsigned)((cols + 255) / 256), (unsigned)rows, 1u}; }
GridDims parent_tiles(long long rows, long long cols, int tw, int th, int planes) { return {(unsigned)((cols + tw - 1) / tw), (unsigned)((rows + th - 1) / th), (unsigned)planes}; }
GridDims parent_pyr_down(long long rows, long long cols)
{
    const long long orows = (rows + 1) / 2, ocols = (cols + 1) / 2;
    return {(unsigned)((ocols + 63) / 64), (unsigned)(((orows + 1) / 2 + 3) / 4), 1u};
}
GridDims parent_nonmax(long long rows, long long cols, long long frames, int* strip_out)
{
    const long long tiles = (cols + 62 - 1) / 62;
    long long strip = (long long)rows * tiles * frames / 8192;
    strip = strip < 8 ? 8 : strip > 64 ? 64 : strip;
    *strip_out = (int)strip;
    return {(unsigned)((tiles + 3) / 4), (unsigned)((rows + strip - 1) / strip), (unsigned)frames};
}
unsigned parent_dynamic_blocks(unsigned long long ntiles, int* dyn_static)
{
    const unsigned long long tail = ntiles * 10 / 100 > 8 ? ntiles * 10 / 100 : 8;
    const unsigned long long stat = ntiles > tail ? (ntiles - tail) / 8 * 8 : 0;
    *dyn_static = (int)stat;
    const unsigned long long queued = ntiles - stat;
    return (unsigned)(stat + (queued + queued * 25 / 100 + 7) / 8 * 8);
}
GridDims parent_strip_grid(int order, int gx, int gy, unsigned nz, int* dyn_static)
{
    if (order == cvs::kOrderDynamic) return {parent_dynamic_blocks((unsigned long long)gx * gy * nz, dyn_static), 1u, 1u};
    if (order == cvs::kOrderXcdColumns) return {8u * (unsigned)(((gx + 7) / 8) * gy), 1u, nz};
    return {(unsigned)gx, (unsigned)gy, nz};
}

bool g_parent = false;

// ---- the checks, one per launcher family ----
void check_generic(int rows, int cols)
{
    g_where = "generic_grid " + std::to_string(rows) + "x" + std::to_string(cols);
    const GridDims g = g_parent ? parent_generic(rows, cols) : cvs::generic_grid(rows, cols);
    bounds(g);
    if ((long long)g.x * 256 < cols) fail("columns not covered");
    if (g_parent) direct_cover(rows, g.y);
    else stride_cover(rows, g.y);
}

void check_tiles(const char* name, int rows, int cols, int tw, int th, int planes)
{
    g_where = std::string(name) + " " + std::to_string(rows) + "x" + std::to_string(cols) + " x" + std::to_string(planes);
    const GridDims g = g_parent ? parent_tiles(rows, cols, tw, th, planes) : cvs::tile_grid(rows, cols, tw, th, planes);
    bounds(g);
    const long long n = cvs::tile_row_count(rows, th);
    if (n * th < rows || (n - 1) * th >= rows) fail("tile rows do not tile the image", n);
    if ((long long)g.x * tw < cols || (long long)(g.x - 1) * tw >= cols) fail("tile columns do not tile the image", g.x);
    if ((int)g.z != planes) fail("one z per plane", g.z, planes);
    if (g_parent) direct_cover(n, g.y);
    else stride_cover(n, g.y);
}

void check_pyr_down(int rows, int cols)
{
    g_where = "pyr_down_grid " + std::to_string(rows) + "x" + std::to_string(cols);
    const GridDims g = g_parent ? parent_pyr_down(rows, cols) : cvs::pyr_down_grid(rows, cols);
    bounds(g);
    const long long orows = (rows + 1) / 2, n = cvs::pyr_down_group_count(rows);
    if (n * 8 < orows || (n - 1) * 8 >= orows) fail("groups of eight output rows do not tile the output", n, orows);
    if ((long long)g.x * 64 < (cols + 1) / 2) fail("output columns not covered");
    if (g_parent) direct_cover(n, g.y);
    else stride_cover(n, g.y);
}

void check_nonmax(int rows, int cols, long long frames)
{
    g_where = "nonmax_grid " + std::to_string(rows) + "x" + std::to_string(cols) + " x" + std::to_string(frames);
    int strip = 0;
    const GridDims g = g_parent ? parent_nonmax(rows, cols, frames, &strip) : cvs::nonmax_grid(rows, cols, frames, &strip);
    bounds(g);
    if (strip < 8) fail("strip under 8 rows", strip);
    if ((long long)g.x * 4 * 62 < cols) fail("columns not covered");
    // strip b covers rows [b * strip, min((b + 1) * strip, rows)): no loop in the kernel
    if ((long long)g.y * strip < rows || (long long)(g.y - 1) * strip >= rows) fail("strips do not tile the rows", g.y, strip);
    if (!g_parent) {   // the bound may only raise the strip where 64 rows would not do; ordinary images keep the parent's strip
        int ps = 0;
        const GridDims p = parent_nonmax(rows, cols, frames, &ps);
        if (p.y <= 65535u && (ps != strip || p.y != g.y || p.x != g.x)) fail("the strip of an ordinary image changed", ps, strip);
    }
}

// the strip kernels: for_each_band's walk over [0, rows) with band_rows = strip_band_rows(...), one launch per band, grid from
// strip_grid; a workgroup's tile is decoded as static_tile / pick_tile do.  fit = rows of the 2 GiB window (a huge value: memory never binds).
void check_strips(int rows, int cols, int strip_rows, int order, unsigned nz, unsigned long long fit, int width)
{
    g_where = "strip plan " + std::to_string(rows) + "x" + std::to_string(cols) + " strip " + std::to_string(strip_rows) + " order " +
              std::to_string(order) + " nz " + std::to_string(nz) + " fit " + std::to_string(fit);
    const int gx = cvs::strip_grid_x(cols);
    if ((long long)gx * 256 < cols || (long long)(gx - 1) * 256 >= cols) fail("column blocks do not tile the image", gx);
    const long long cap = g_parent ? (long long)rows : cvs::strip_band_cap(order, gx, strip_rows, nz);
    const int per = cvs::strip_band_rows(rows, fit, width, strip_rows, cap);
    if (per == 0) return;   // the generic path
    if (per < 0) return fail("negative band");
    long long covered = 0, launches = 0;
    for (long long lo = 0; lo < rows; lo += per) {
        const int hi = (int)(lo + per < rows ? lo + per : rows);
        const int strip = strip_rows > per ? per : strip_rows;
        const int gy = cvs::strip_grid_y((int)lo, hi, strip);
        if ((long long)gy * strip < hi - lo || (long long)(gy - 1) * strip >= hi - lo) fail("strips do not tile the band", gy, strip);
        int dyn_static = -1;
        const GridDims g = g_parent ? parent_strip_grid(order, gx, gy, nz, &dyn_static) : cvs::strip_grid(order, gx, gy, nz, &dyn_static);
        bounds(g);
        const unsigned long long tiles = (unsigned long long)gx * gy * nz;
        if (order == 0) {
            if ((int)g.x != gx || (int)g.y != gy || g.z != nz) fail("plain order: one workgroup per tile", g.y, gy);
        } else if (order == cvs::kOrderXcdColumns) {   // static_tile: k = b >> 3, by = k / cpx, bx = xcd * cpx + k % cpx; padding slots leave
            const long long cpx = (gx + 7) / 8;
            if ((long long)g.x != 8 * cpx * gy || g.y != 1 || g.z != nz) fail("xcd columns: eight column ranges per strip row", g.x);
            if (gy <= 64 && gx <= 64) {
                std::vector<int> seen((size_t)gx * gy, 0);
                for (unsigned b = 0; b < g.x; ++b) {
                    const long long k = b >> 3, by = k / cpx, bx = (b & 7) * cpx + (k - by * cpx);
                    if (bx < gx && by < gy) ++seen[(size_t)(by * gx + bx)];
                }
                for (int v : seen)
                    if (v != 1) { fail("xcd columns: a tile not dealt exactly once", v); break; }
            }
        } else {   // dynamic: dyn_static tiles by index, the rest through the queues; enough workgroups for every tile
            if (g.y != 1 || g.z != 1) fail("dynamic order: one row of workgroups");
            if (tiles > 0x7fffffffull) fail("dynamic order: more tiles than pick_tile's int arithmetic holds", (long long)tiles);
            if (dyn_static < 0 || (unsigned long long)dyn_static > tiles || dyn_static % 8) fail("dynamic order: static share", dyn_static);
            if ((unsigned long long)g.x < tiles || g.x % 8) fail("dynamic order: fewer workgroups than tiles", g.x, (long long)tiles);
        }
        covered += hi - lo;
        ++launches;
        if (launches > 1 && lo % strip_rows && per >= strip_rows) fail("a band starts inside a strip", lo);
    }
    if (covered != rows) fail("bands do not add up to the image", covered, rows);
    if (g_parent && launches != 1 && fit >= (unsigned long long)rows) fail("the parent made one launch");
}

// a batch in one launch (never banded): wherever strip_batch_fits says yes, the grid of every order holds the bounds at that strip
// height and at taller ones; the parent launched every batch this way
void check_batch(int rows, int cols, int min_strip, int n)
{
    g_where = "strip plan, batch of " + std::to_string(n) + " " + std::to_string(rows) + "x" + std::to_string(cols) + " strip >= " + std::to_string(min_strip);
    if (!g_parent && !cvs::strip_batch_fits(rows, cols, min_strip, n)) return;
    const int gx = cvs::strip_grid_x(cols);
    for (int strip : {min_strip, min_strip + 9, 46})
        for (int order : {0, cvs::kOrderXcdColumns, cvs::kOrderDynamic})
            for (int ways : {1, 2}) {
                const unsigned nz = (unsigned)((n + ways - 1) / ways * ways);
                int ds = 0;
                const int gy = cvs::strip_grid_y(0, rows, strip);
                bounds(g_parent ? parent_strip_grid(order, gx, gy, nz, &ds) : cvs::strip_grid(order, gx, gy, nz, &ds));
            }
}

// strip_one_launch (the tuner's fit rule for a launch that must stay ONE launch, 8-bit outputs): it says yes exactly where the band walk
// makes one launch, for every order and the strip heights the tuner offers
void check_one_launch(int rows, int cols)
{
    g_where = "strip plan, one launch " + std::to_string(rows) + "x" + std::to_string(cols);
    for (int strip : {7, 10, 19})
        for (int order : {0, cvs::kOrderXcdColumns, cvs::kOrderDynamic}) {
            const long long cap = cvs::strip_band_cap(order, cvs::strip_grid_x(cols), strip, 1u);
            const bool one = cvs::strip_band_rows(rows, ~0ull >> 1, 4, strip, cap) >= rows;
            ++g_checked;
            if (one != cvs::strip_one_launch(order, cols, strip, 1u, rows)) fail("strip_one_launch disagrees with the band walk", strip, order);
        }
}

constexpr int kCcTileW = 128, kCcTileH = 32, kChRows = 32, kHystTileW = 128, kHystTileH = 32;   // (held to the sources by tests/test_grid_plan_cpu.py)
const int kStrips[] = {1, 6, 10, 14, 20, 40, 46};
const int kOrders[] = {0, cvs::kOrderXcdColumns, cvs::kOrderDynamic};

void check_shape(int rows, int cols, bool all_strips)
{
    check_generic(rows, cols);
    check_tiles("tile_grid(k_cc_tiles, k_link_tiles, k_chb_tiles)", rows, cols, kCcTileW, kCcTileH, 1);
    check_tiles("tile_grid(k_link_tiles, 3 planes)", rows, cols, kCcTileW, kCcTileH, 3);
    check_tiles("tile_grid(k_ch_links, k_chb_links)", rows, cols, 256, kChRows, 1);
    check_tiles("tile_grid(k_hyst_propagate)", rows, cols, kHystTileW, kHystTileH, 2);
    check_pyr_down(rows, cols);
    check_nonmax(rows, cols, 1);
    if ((long long)rows * cols * 32 <= (1ll << 31)) check_nonmax(rows, cols, 32);
    // (3 W + 1 rows and W + 1 columns, W = 4 for the G2 bank and 6 for the G4 pair: smaller images never reach the strip kernels)
    if (rows < 13 || cols < 5) return;
    for (int strip : kStrips) {
        if (!all_strips && strip != 1 && strip != 10 && strip != 40) continue;
        for (int order : kOrders) {
            check_strips(rows, cols, strip, order, 1u, ~0ull >> 1, 4);
            if (rows >= 19 && cols >= 7) check_strips(rows, cols, strip, order, 2u, ~0ull >> 1, 6);
        }
    }
    if (!g_parent) check_one_launch(rows, cols);
    for (int n : {1, 32, 65534, 65535, 70000})
        if ((long long)rows * cols * n <= (1ll << 36)) {   // (what a card could hold)
            check_batch(rows, cols, 1, n);
            check_batch(rows, cols, 10, n);
        }
    // a 2 GiB window that binds as well (pitch 64 floats: 2^23 rows; a wide pitch: a few thousand)
    for (unsigned long long fit : {1ull << 23, 5000ull})
        for (int order : kOrders) check_strips(rows, cols, 10, order, 1u, fit, 4);
}

struct Dims { int rows, cols, strip, order; unsigned nz; unsigned x, y, z; };

// The shapes of the legs tests/golden/timed_instances.json names (4096^2, 8192^2 and its pyramid levels, 32 frames of 1920 x 1080), with the
// grids the parent commit launched for them: literals worked out from the parent's formulas (plan_strips: gx = ceil(ceil(cols / 64) / 4),
// gy = ceil(rows / strip); plain (gx, gy, nz); XCD columns (8 ceil(gx / 8) gy, 1, nz); dynamic (stat + ceil8(1.25 queued), 1, 1) with
// tail = max(8, n / 10), stat = floor8(n - tail), queued = n - stat).
const Dims kTimed[] = {
    {4096, 4096, 10, 0, 1, 16, 410, 1},
    {4096, 4096, 10, cvs::kOrderXcdColumns, 1, 6560, 1, 1},
    {4096, 4096, 10, cvs::kOrderDynamic, 1, 6728, 1, 1},     // n = 6560: tail 656, stat 5904, queued 656 -> 5904 + 824
    {4096, 4096, 20, 0, 1, 16, 205, 1},
    {4096, 4096, 40, 0, 2, 16, 103, 2},                      // the G4 pair launch
    {4096, 4096, 40, cvs::kOrderDynamic, 2, 3384, 1, 1},     // n = 3296: tail 329, stat 2960, queued 336 -> 2960 + 424
    {8192, 8192, 10, 0, 1, 32, 820, 1},
    {8192, 8192, 10, cvs::kOrderDynamic, 1, 26896, 1, 1},    // n = 26240: tail 2624, stat 23616, queued 2624 -> 23616 + 3280
    {8192, 8192, 46, 0, 1, 32, 179, 1},                      // cvs_pyr_down as a strip march
    {2048, 2048, 10, 0, 1, 8, 205, 1},
    {1024, 1024, 10, 0, 1, 4, 103, 1},
    {512, 512, 10, 0, 1, 2, 52, 1},
    {1080, 1920, 10, 0, 32, 8, 108, 32},                     // 32 frames on grid.z
    {1080, 1920, 14, cvs::kOrderXcdColumns, 32, 624, 1, 32},
    {1080, 1920, 10, cvs::kOrderDynamic, 32, 28344, 1, 1},   // n = 27648: tail 2764, stat 24880, queued 2768 -> 24880 + 3464
};
const int kTimedShapes[][2] = {{4096, 4096}, {8192, 8192}, {2048, 2048}, {1024, 1024}, {512, 512}, {1080, 1920}};

void check_timed()
{
    for (const Dims& d : kTimed) {
        g_where = "timed " + std::to_string(d.rows) + "x" + std::to_string(d.cols) + " strip " + std::to_string(d.strip) + " order " + std::to_string(d.order);
        const int gx = cvs::strip_grid_x(d.cols);
        const long long cap = cvs::strip_band_cap(d.order, gx, d.strip, d.nz);
        if (cvs::strip_band_rows(d.rows, ~0ull >> 1, 4, d.strip, cap) != d.rows) fail("a timed shape is banded");
        int ds = 0;
        const GridDims g = cvs::strip_grid(d.order, gx, cvs::strip_grid_y(0, d.rows, d.strip), d.nz, &ds);
        ++g_checked;
        if (g.x != d.x || g.y != d.y || g.z != d.z) fail("a timed launch changed its grid", g.x, g.y);
        int ps = 0;
        const GridDims p = parent_strip_grid(d.order, gx, (d.rows + d.strip - 1) / d.strip, d.nz, &ps);
        if (p.x != d.x || p.y != d.y || p.z != d.z || ps != ds) fail("the literal is not the parent's", p.x, p.y);
    }
    // the other launchers at the timed shapes: the parent's grid, dimension for dimension
    for (const auto& s : kTimedShapes) {
        const int rows = s[0], cols = s[1];
        g_where = "timed " + std::to_string(rows) + "x" + std::to_string(cols);
        auto same = [](const GridDims& a, const GridDims& b) { return a.x == b.x && a.y == b.y && a.z == b.z; };
        int s0 = 0, s1 = 0;
        if (!same(cvs::generic_grid(rows, cols), parent_generic(rows, cols))) fail("generic grid changed");
        if (!same(cvs::tile_grid(rows, cols, kCcTileW, kCcTileH, 1), parent_tiles(rows, cols, kCcTileW, kCcTileH, 1))) fail("tile grid changed");
        if (!same(cvs::tile_grid(rows, cols, 256, kChRows, 1), parent_tiles(rows, cols, 256, kChRows, 1))) fail("links grid changed");
        if (!same(cvs::pyr_down_grid(rows, cols), parent_pyr_down(rows, cols))) fail("pyr_down grid changed");
        for (long long frames : {1ll, 32ll})
            if (!same(cvs::nonmax_grid(rows, cols, frames, &s0), parent_nonmax(rows, cols, frames, &s1)) || s0 != s1) fail("nonmax grid changed", s0, s1);
        g_checked += 6;
    }
    {
        g_where = "timed literals";   // two of the rows above, once more by hand
        const GridDims a = cvs::pyr_down_grid(8192, 8192), b = cvs::tile_grid(1080, 1920, kCcTileW, kCcTileH, 1);
        if (a.x != 64 || a.y != 512 || a.z != 1) fail("pyr_down 8192^2 is (64, 512, 1)", a.x, a.y);
        if (b.x != 15 || b.y != 34 || b.z != 1) fail("tiles of 1080p are (15, 34, 1)", b.x, b.y);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    g_parent = argc > 1 && !std::strcmp(argv[1], "parent");
    // 1. the tall shapes of tests/test_gpu_tall.py: one workgroup row past 65535 and 65536 for each launcher
    const int tall[][2] = {{65537, 3}, {65537, 9}, {65537, 5}, {65537, 7}, {655361, 5}, {1048577, 2}, {1048577, 5}, {2097153, 5}, {2097153, 1},
                           {4194305, 1}, {4194305, 5}, {4194241, 1}, {4194241, 2}, {65535, 5}, {65536, 5}, {2097120, 5}, {2097121, 5}};
    g_print_all = true;
    for (const auto& s : tall) check_shape(s[0], s[1], true);
    g_print_all = false;
    if (!g_parent) {   // 500,000 x 8: one launch with the default ten-row strips, not with the tuner's seven-row challenger
        g_where = "strip plan, one launch 500000x8";
        check_shape(500000, 8, true);
        if (!cvs::strip_one_launch(0, 8, 10, 1u, 500000) || cvs::strip_one_launch(0, 8, 7, 1u, 500000)) fail("500,000 rows: ten-row strips fit one plain grid, seven-row strips do not");
        if (!cvs::strip_one_launch(cvs::kOrderDynamic, 8, 7, 1u, 500000)) fail("500,000 rows, seven-row strips: the dynamic order's one row of workgroups holds them");
    }
    // 2. the timed shapes
    for (const auto& s : kTimedShapes) check_shape(s[0], s[1], true);
    if (!g_parent) check_timed();
    // 3. seeded random shapes inside the pixel limit, log-uniform in rows, the extremes included
    std::mt19937_64 rng(20240607);
    const long long kMaxPix = (1ll << 31) - 2;
    check_shape((int)kMaxPix, 1, false);
    check_shape(46340, 46340, false);
    for (int i = 0; i < 300; ++i) {
        const double u = std::uniform_real_distribution<double>(0.0, 31.0)(rng);
        long long rows = (long long)std::exp2(u);
        rows = rows < 1 ? 1 : rows > kMaxPix ? kMaxPix : rows;
        const long long cmax = kMaxPix / rows;
        const double v = std::uniform_real_distribution<double>(0.0, std::log2((double)cmax + 1.0))(rng);
        long long cols = (long long)std::exp2(v);
        cols = cols < 1 ? 1 : cols > cmax ? cmax : cols;
        check_shape((int)rows, (int)cols, false);
    }
    for (int f = 0; f < 6; ++f) std::printf("%s: %d broken\n", kFamilies[f], g_broken[f]);
    std::printf("%s: %d grids checked, %d requirement(s) broken\n", g_parent ? "parent formulas" : "cvs_grid.h", g_checked, g_failed);
    if (!g_failed) std::printf("grid plan holds\n");
    return g_failed ? 1 : 0;
}
