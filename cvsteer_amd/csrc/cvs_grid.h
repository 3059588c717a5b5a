// cvs_grid.h -- the grid arithmetic of every launcher whose grid.y or grid.z follows the image height (or the plane count): plain
// functions of (rows, cols, strip, planes, ...) with no HIP type in them, so that tests/cpp/grid_plan.cpp can sweep them on the CPU.
// The launchers take the three dimensions of their grids from these functions and from nothing else.
//
// One bound for all of them: y and z stay <= 65535 (kGridMaxYZ, the figure the z-chunked launchers have always used).  x is held below
// 2^24 workgroups (x * 256 lanes fits 32 bits) where it follows the row count -- the one-dimensional orders of the strip kernels;
// where x follows the columns alone (generic_grid, tile_grid, ...) nothing is enforced: it stays below 2^24 for every image but a
// single row of more than 2^31 - 128 columns, the wide side these functions do not deal with.
// Rows past the bound are covered in one of two ways:
//   - the kernel strides: for (t = blockIdx.y; t < n; t += gridDim.y), n = the *_count() beside the grid function (constexpr: the
//     kernels call them too);
//   - the strip kernels (k_basis, k_basis_lit, k_basis_pair), whose device code takes one tile per workgroup, get more launches: row
//     bands of at most strip_band_cap() rows (for_each_band).
#pragma once

namespace cvs {

constexpr unsigned kGridMaxYZ = 65535u;
constexpr unsigned kGridMaxX = (1u << 24) - 1u;   // x * 256 < 2^32

constexpr int kOrderXcdColumns = 1000000;  // BasisArgs::block_order: every XCD owns a contiguous range of column blocks
constexpr int kOrderDynamic = 2000000;     // BasisArgs::block_order: the tail of the launch is taken from per-XCD queues (tile_ctr)

struct GridDims {
    unsigned x, y, z;
};

inline unsigned grid_cap_yz(long long n) { return n < 1 ? 1u : n > (long long)kGridMaxYZ ? kGridMaxYZ : (unsigned)n; }
constexpr long long grid_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// ---- one workgroup per 256 columns of ONE row; the kernel strides the rows (k_rowpass_generic, k_colpass_generic) ----
inline GridDims generic_grid(int rows, int cols)
{
    return {(unsigned)grid_ceil_div(cols, 256), grid_cap_yz(rows), 1u};
}

// ---- one workgroup per `per` entries of a LIST (points, chains): x alone, held to kGridMaxX; the kernel strides the list with
// gridDim.x * per (k_turn_summary) or shows that its list never reaches the bound (k_turns, k_turn_nms: 2^30 points / 256) ----
inline GridDims list_grid(long long n, int per)
{
    const long long g = grid_ceil_div(n, per);
    return {g < 1 ? 1u : g > (long long)kGridMaxX ? kGridMaxX : (unsigned)g, 1u, 1u};
}

// ---- one workgroup per tile_w x tile_h tile and plane; the kernel strides the tile rows (k_cc_tiles, k_link_tiles, k_ch_links,
// k_hyst_propagate, k_chb_links, k_chb_tiles) ----
constexpr int tile_row_count(int rows, int tile_h) { return (int)grid_ceil_div(rows, tile_h); }
inline GridDims tile_grid(int rows, int cols, int tile_w, int tile_h, int planes)
{
    return {(unsigned)grid_ceil_div(cols, tile_w), grid_cap_yz(tile_row_count(rows, tile_h)), (unsigned)planes};
}

// ---- k_pyr_down: 64 output columns per workgroup, four waves of two output rows each; the kernel strides these 8-row groups ----
constexpr int pyr_down_group_count(int rows) { return (((rows + 1) / 2 + 1) / 2 + 3) / 4; }
inline GridDims pyr_down_grid(int rows, int cols)
{
    return {(unsigned)grid_ceil_div((cols + 1) / 2, 64), grid_cap_yz(pyr_down_group_count(rows)), 1u};
}

// ---- k_nonmax / k_nms_frames: four 62-column wave tiles per workgroup, one strip of rows per blockIdx.y.  Rows per strip: enough
// waves to keep every CU's memory pipeline busy (~8K waves), at least 8 rows so that the two halo rows of a strip stay a small part of
// its reads, at most 64 -- and more than 64 only where fewer rows per strip would need more than kGridMaxYZ strips (the decisions do
// not depend on the strip: any strip gives the same values) ----
inline GridDims nonmax_grid(int rows, int cols, long long frames, int* strip_out)
{
    const long long tiles = grid_ceil_div(cols, 62);
    long long strip = (long long)rows * tiles * frames / 8192;
    strip = strip < 8 ? 8 : strip > 64 ? 64 : strip;
    const long long need = grid_ceil_div(rows, kGridMaxYZ);
    if (strip < need) strip = need;
    *strip_out = (int)strip;
    return {(unsigned)((tiles + 3) / 4), (unsigned)grid_ceil_div(rows, strip), (unsigned)frames};
}

// ---- the strip kernels: one workgroup of four waves per 256 columns and strip of rows, nz planes of tiles ----
inline int strip_grid_x(int cols) { return ((cols + 63) / 64 + 3) / 4; }
inline int strip_grid_y(int row_lo, int row_hi, int strip_rows) { return (row_hi - row_lo + strip_rows - 1) / strip_rows; }

// dynamic order: the last tenth of the tiles goes through the queues (the rest: tile = workgroup index) with a quarter more
// workgroups than queued tiles (see pick_tile; both figures from the sweep in profiles/r04_order_probe.txt), a multiple of 8 so
// that every XCD gets the same number
inline unsigned dynamic_blocks(unsigned long long ntiles, int* dyn_static)
{
    const unsigned long long pct = 25, tail_pct = 10;
    const unsigned long long tail = ntiles * tail_pct / 100 > 8 ? ntiles * tail_pct / 100 : 8;
    const unsigned long long stat = ntiles > tail ? (ntiles - tail) / 8 * 8 : 0;
    *dyn_static = (int)stat;
    const unsigned long long queued = ntiles - stat;
    return (unsigned)(stat + (queued + queued * pct / 100 + 7) / 8 * 8);
}

// the grid of one strip launch over grid_x x grid_y tiles in nz planes; `order` already normalised (0, kOrderXcdColumns, kOrderDynamic)
inline GridDims strip_grid(int order, int grid_x, int grid_y, unsigned nz, int* dyn_static)
{
    if (order == kOrderDynamic) return {dynamic_blocks((unsigned long long)grid_x * grid_y * nz, dyn_static), 1u, 1u};
    if (order == kOrderXcdColumns) return {8u * (unsigned)(((grid_x + 7) / 8) * grid_y), 1u, nz};
    return {(unsigned)grid_x, (unsigned)grid_y, nz};
}

// Most output rows ONE strip launch may cover so that strip_grid() stays inside the bounds: a multiple of strip_rows, never less than
// one strip.  Plain order: grid.y.  The two one-dimensional orders: grid.x (the dynamic order's grid is at most 1.025 n + 23
// workgroups for n tiles; 4/5 of the bound leaves room for that).
inline long long strip_band_cap(int order, int grid_x, int strip_rows, unsigned nz)
{
    long long gy;
    if (order == kOrderDynamic) gy = (long long)(kGridMaxX / 5u * 4u) / ((long long)grid_x * nz);
    else if (order == kOrderXcdColumns) gy = (long long)kGridMaxX / (8ll * ((grid_x + 7) / 8));
    else gy = kGridMaxYZ;
    if (gy < 1) gy = 1;
    return gy * strip_rows;
}

// Does ONE strip launch in this order and with this strip height cover `rows` rows?  (The tuner asks before it lets a challenger run a
// launch the API layer has already judged to be one fused launch: cvs_tune.cpp, fits.)
inline bool strip_one_launch(int order, int cols, int strip_rows, unsigned nz, int rows)
{
    return strip_band_cap(order, strip_grid_x(cols), strip_rows > 0 ? strip_rows : 1, nz) >= rows;
}

// A batch of n frames in ONE strip launch (frames on grid.z, or all tiles in one row of workgroups) is never banded: does its grid stay
// inside the bounds in every order, with strips of min_strip_rows rows or more?  (z: the frames rounded up to the two parts they are
// dealt from.)  Where not, the batch goes frame by frame through the single-image path, which bands.
inline bool strip_batch_fits(int rows, int cols, int min_strip_rows, int n)
{
    const long long gx = strip_grid_x(cols), gy = grid_ceil_div(rows, min_strip_rows), nz = (long long)n + 1;
    return gy <= (long long)kGridMaxYZ && nz <= (long long)kGridMaxYZ && 8 * ((gx + 7) / 8) * gy <= (long long)kGridMaxX &&
           gx * gy * nz <= (long long)(kGridMaxX / 5u * 4u);
}

// Output rows per launch of a strip kernel over `rows` rows (band_rows in cvs_kernels_basis.hip; for_each_band walks the bands): `fit` =
// the rows whose 32-bit buffer offsets stay below 2 GiB at the launch's widest pitch (band + halo rows, relative to the shifted plane
// base), `cap` = strip_band_cap().  The whole image where both allow it; 0 = not even one strip with its halo fits (generic path).
inline int strip_band_rows(int rows, unsigned long long fit, int width, int strip_rows, long long cap)
{
    if (fit >= (unsigned long long)rows) return cap < rows ? (int)cap : rows;
    if (fit < (unsigned long long)(2 * width + 2)) return 0;
    const int room = (int)fit - 2 * width;
    const int per = room >= strip_rows ? room / strip_rows * strip_rows : room;  // very wide rows: one short strip per band
    return cap < per ? (int)cap : per;
}

}  // namespace cvs
