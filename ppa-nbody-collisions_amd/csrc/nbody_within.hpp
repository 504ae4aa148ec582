// csrc/nbody_within.hpp -- radius queries on the cell list (nbody_get_within, nbody_batch_get_within, include/nbody.h;
// DESIGN.md 4.21): for every row - a current body, or a probe point - the number of sources within a distance h, the nearest
// of them, how many of them overlap the row and, on request, the neighbour list in CSR form.  The first near-field query
// that is O(n) on a grid matched to h: a row looks at the cells of a window around its own cell coordinates only, through
// the cell list of the cell sums (nbody_cells.hpp).  One system (nbody_ctx.hip) and a batch (nbody_batch.hip: system =
// blockIdx.y, per-body arrays `stride` apart, one grid and one set of points for every system) share each kernel.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  The sources are
// the bodies with inside(j) of the cell sums.  A row at (x, y) with radius r (+0 for a point), own index i (none for a point):
//     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)                 the d2 of nbody_get_neighbors
//     near(j)  <=>  inside(j) && j != i && d2_j <= h2
//     count = #near;  nearest = the minimum of (d2_j, j) over the near j, lexicographic;  overlaps = #near with d2_j <= s*s
// Every output is an integer, a minimum under a total order or a sorted list: none depends on the order of the visit, so the
// cells are walked as they lie and the result has the bits of the brute-force definition - PROVIDED the window holds every
// cell that can hold a near source.
//
// The window rule (cells_span, nbody_cells.hpp; tests/within_cases.py restates it, DESIGN.md 4.21 has the derivation).  Per axis, with the
// row's cell coordinate t = (x - x0) * sx as the cell sums compute it and w0 = fl(h * sx), h = fl(sqrt(h2)), both once on the
// host:   w = w0 + (2^-20 + (|t| + w0) * 2^-40);   columns (int)max(t - w, 0) .. (int)min(t + w, nx - 1).
// A window is empty only where t + w < 0 or t - w >= nx holds as a compare; a t that is not finite, or a NaN in t - w or
// t + w (inf - inf), means every column.  A grid of more than 2^400 cells per unit length means every column too (w0 = +inf
// from the host): there the product dx*dx can underflow for bodies many cells apart.
//
// Kernels, on the handle's stream after the four list stages of the cell sums (cells_list_run) and the gather of the list's
// sorted records {x, y, r, j} (cells_gather_run), so that the walk reads contiguous memory and no index per pair.  The view of
// a system's list, the cell coordinates, the window walk and the workgroup prefix are the list's (nbody_cells.hpp: cells_view,
// cells_coords, cells_window_walk, cells_block_prefix); this file has the rows, the pair and the row scan.
//   within_walk<T, kOwn, Count, kList>  one lane per row.  Own rows inside the grid are taken in cell order (lane = slot: the
//                             64 rows of a wave share a few cells, nearly one window, and their loads hit the same lines);
//                             own rows outside the grid follow, one lane per body that leaves unless its cell is -1; points
//                             in the order given.  The grid is row-major, so the members of columns c0 .. c1 of one row of
//                             cells are ONE contiguous range of the sorted records: a lane walks r1 - r0 + 1 ranges, four
//                             records loaded ahead of their pairs (cells_window_walk).  Per pair: 2 subtractions, 2 multiplies, 1 add and the
//                             compare with h2; the count, the minimum, the overlap compare and the list store sit behind the
//                             branch that compare makes.  kList: the second pass, which stores the near j at the row's start.
//   within_block_sums<Count>, within_block_scan<Count>, within_block_starts<Count>   the exclusive 64-bit prefix sum of
//                             the counts in row order into start[0 .. rows], over the whole chip: the sum and the greatest
//                             (count, row) of every block of 1024 rows; one workgroup per system that scans the block sums
//                             and writes the info record (total, largest and the lowest row with it); and, only where the
//                             starts are asked for, start[row] = the block's offset + the prefix inside the block.  One
//                             workgroup scanning all rows took 0.21 ms for 262144 rows, two thirds of a call's kernels:
//                             it reads 24 bytes per row through one compute unit.
//   within_rank<Count>        one lane per list entry: the row by bisection of start, then the entry moves to start[row] +
//                             #{entries of the row with a smaller index} - a counting sort per row, as cells_rank's per cell:
//                             the segment is ascending whatever order the cells were walked in.
// Every index that comes out of memory (an entry of order, a start of a cell or a row, a j of a record) is range-checked
// before it is used as one.  A batch's count goes through batch_checked_count; cells_assign has reported a bad one, every
// kernel here treats that system as empty.  No kernel uses scratch; registers: DESIGN.md 4.21.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_cells.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct WithinOut { double d2; int index, count, overlaps, cell; };         // struct nbody_within as device code writes it
static_assert(sizeof(WithinOut) == 24 && sizeof(nbody_within) == 24, "nbody_within layout");
static_assert(offsetof(nbody_within, d2) == 0 && offsetof(nbody_within, index) == 8 && offsetof(nbody_within, count) == 12 &&
              offsetof(nbody_within, overlaps) == 16 && offsetof(nbody_within, cell) == 20 && offsetof(WithinOut, count) == 12 &&
              offsetof(WithinOut, cell) == 20, "nbody_within and its device mirror");
static_assert(sizeof(nbody_within_info) == 32 && offsetof(nbody_within_info, n) == 8, "nbody_within_info layout");

constexpr int kWithinScanPer = 4;                                // consecutive rows per lane of the row scan
constexpr int kWithinBlockRows = kDiagBlock * kWithinScanPer;    // rows per workgroup of the row scan

struct WithinWin { double h2, wx0, wy0; };                       // the call's values: h2, and h in cells per axis

// One lane per row; grid = (ceil(lanes / kDiagBlock), systems) with lanes = 2 * n_bound for own rows - lane q < n is slot q
// of the cell list, lane n + j is body j and has a row only where cell_of[j] is -1 - and m for points.
// kList = false: the counting pass, which writes the record of every row.  kList = true: the filling pass, which writes
// nothing but the near j of every row, from rstart[row] on, into raw_all ([systems * list_stride]).
template <typename T, bool kOwn, typename Count, bool kList>
__global__ __launch_bounds__(kDiagBlock) void within_walk(const Rec<T>* __restrict__ J_all, const CellRec<T>* __restrict__ sorted_all,
                                                          const Meta* __restrict__ meta_all, int stride, int n_one,
                                                          const nbody_grid g, const WithinWin win,
                                                          const int32_t* __restrict__ cell_of_all,
                                                          const int32_t* __restrict__ start_all,
                                                          const FieldPoint* __restrict__ points, int m,
                                                          WithinOut* __restrict__ out_all,
                                                          const long long* __restrict__ rstart_all,
                                                          int32_t* __restrict__ raw_all, long long list_stride) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    const int n = cl.n, sys = cl.sys;
    const int lanes = kOwn ? 2 * n : m;
    if ((int)(blockIdx.x * kDiagBlock) >= lanes) return;
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const int q = blockIdx.x * kDiagBlock + threadIdx.x;
    const size_t per = kOwn ? (size_t)stride : (size_t)m;        // rows of one system in out and rstart

    // the lane's row: its index in out, its own index among the sources (-1: none), the position and the radius
    int row = -1, self = -1;
    double x = 0.0, y = 0.0, r = 0.0;
    if (kOwn) {
        if (q < cl.inside) {
            const CellRec<T> w = sorted[q];
            if ((unsigned)w.j < (unsigned)n) { row = self = w.j; x = (double)w.x; y = (double)w.y; r = (double)w.r; }
        } else if (q >= n && q < lanes) {
            const int j = q - n;
            if (cell_of_all[cl.at + j] < 0) {
                const Rec<T> b = J_all[cl.at + j];
                row = self = j; x = (double)b.x; y = (double)b.y; r = (double)b.r;
            }
        }
    } else if (q < m) {
        const FieldPoint p = points[q];
        row = q; x = p.x; y = p.y;
    }
    if (row < 0) return;                                         // no barrier follows

    double best = __builtin_inf();
    int index = -1, count = 0, overlaps = 0;
    long long at = 0, end = 0;                                   // kList: where the row's next entry goes, and its segment's end
    int32_t* __restrict__ raw = nullptr;
    if constexpr (kList) {
        const long long* __restrict__ rstart = rstart_all + (size_t)sys * (per + 1);
        at = rstart[row]; end = rstart[row + 1];
        if (at < 0 || end > list_stride || at > end) at = end = 0;
        raw = raw_all + (size_t)sys * (size_t)list_stride;
    }
    const CellCoords t = cells_coords(g, x, y);
    cells_window_walk(cl, sorted, g, t.tx, t.ty, win.wx0, win.wy0, [&](const CellRec<T>& s) {
        const double dx = (double)s.x - x, dy = (double)s.y - y;
        const double d2 = (dx * dx) + (dy * dy);
        if (d2 <= win.h2 && s.j != self) {                       // the rest only for a pair that passes
            if constexpr (kList) {
                if (at < end) raw[at] = s.j;
                ++at;
            } else {
                ++count;
                if (d2 < best || (d2 == best && s.j < index)) { best = d2; index = s.j; }
                const double sum = r + (double)s.r;
                overlaps += d2 <= sum * sum ? 1 : 0;
            }
        }
    });
    if constexpr (!kList)
        out_all[(size_t)sys * per + row] = WithinOut{best, index, count, overlaps, cells_cell(g, x, y)};
}

// The row scan's pieces; the workgroup's exclusive prefix is cells_block_prefix (nbody_cells.hpp).
// (count, row) as one word whose maximum is the greatest count and, among equal counts, the lowest row.
__device__ __forceinline__ unsigned long long within_key(int count, int row) {
    return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)row);
}

// The workgroup's maximum key in lane 0 of wave 0.  wkey: shared, one entry per wave.
__device__ __forceinline__ unsigned long long within_group_max(unsigned long long key, unsigned long long* wkey) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
        const unsigned long long o = __shfl_down(key, sh, kWave);
        key = o > key ? o : key;
    }
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kDiagBlock / kWave; ++w) key = wkey[w] > key ? wkey[w] : key;
    return key;
}

// The counts of the lane's kWithinScanPer consecutive rows of block blockIdx.x; a row past the last, or a negative count: 0.
__device__ __forceinline__ void within_load_counts(const WithinOut* __restrict__ out, int rows, int (&v)[kWithinScanPer]) {
    const int r0 = blockIdx.x * kWithinBlockRows + threadIdx.x * kWithinScanPer;
#pragma unroll
    for (int u = 0; u < kWithinScanPer; ++u) {
        const int c = r0 + u < rows ? out[r0 + u].count : 0;
        v[u] = c < 0 ? 0 : c;
    }
}

// Stage 1 of the row scan: grid = (blocks, systems), a block of kWithinBlockRows rows per workgroup; m < 0: own rows.
// bsum_all, bkey_all: [systems * blocks] - the block's sum of counts and its greatest (count, row).
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void within_block_sums(const Meta* __restrict__ meta_all, int stride, int n_one, int m,
                                                                const WithinOut* __restrict__ out_all,
                                                                long long* __restrict__ bsum_all,
                                                                unsigned long long* __restrict__ bkey_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one);
    const int sys = cl.sys, rows = m < 0 ? cl.n : m;
    if ((long long)blockIdx.x * kWithinBlockRows >= rows) return;               // the whole workgroup
    const size_t per = m < 0 ? (size_t)stride : (size_t)m;
    __shared__ long long wsum[kDiagBlock / kWave];
    __shared__ unsigned long long wkey[kDiagBlock / kWave];
    int v[kWithinScanPer];
    within_load_counts(out_all + (size_t)sys * per, rows, v);
    const int r0 = blockIdx.x * kWithinBlockRows + threadIdx.x * kWithinScanPer;
    long long mine = 0;
    unsigned long long key = 0;
#pragma unroll
    for (int u = 0; u < kWithinScanPer; ++u) {
        mine += v[u];
        const unsigned long long k = r0 + u < rows ? within_key(v[u], r0 + u) : 0ull;
        key = k > key ? k : key;
    }
    const long long total = cells_block_prefix<long long, kDiagBlock>(mine, wsum).total;
    key = within_group_max(key, wkey);
    if (threadIdx.x == 0) {
        const size_t at = (size_t)sys * (size_t)gridDim.x + blockIdx.x;
        bsum_all[at] = total;
        bkey_all[at] = key;
    }
}

// Stage 2: one workgroup per system scans its blocks' sums into boff_all ([systems * blocks], exclusive) and writes the info
// record and, where the starts are asked for, start[rows] = total.  cinfo_all: the cell list's info.
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void within_block_scan(const Meta* __restrict__ meta_all, int stride, int n_one, int m,
                                                                int blocks, const long long* __restrict__ bsum_all,
                                                                const unsigned long long* __restrict__ bkey_all,
                                                                long long* __restrict__ boff_all,
                                                                long long* __restrict__ rstart_all,
                                                                const nbody_cells_info* __restrict__ cinfo_all,
                                                                nbody_within_info* __restrict__ info_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one);
    const int sys = cl.sys, n = cl.n, rows = m < 0 ? n : m;
    const size_t per = m < 0 ? (size_t)stride : (size_t)m;
    int mine_blocks = (int)(((long long)rows + kWithinBlockRows - 1) / kWithinBlockRows);
    mine_blocks = mine_blocks > blocks ? blocks : mine_blocks;
    __shared__ long long wsum[kDiagBlock / kWave];
    __shared__ unsigned long long wkey[kDiagBlock / kWave];
    const size_t at = (size_t)sys * (size_t)blocks;
    long long carry = 0;
    unsigned long long key = 0;
    for (int base = 0; base < mine_blocks; base += kDiagBlock) {
        const int b = base + threadIdx.x;
        const long long x = b < mine_blocks ? bsum_all[at + b] : 0;
        if (b < mine_blocks) key = bkey_all[at + b] > key ? bkey_all[at + b] : key;
        const BlockPrefix<long long> p = cells_block_prefix<long long, kDiagBlock>(x, wsum);
        if (b < mine_blocks) boff_all[at + b] = carry + p.at;
        carry += p.total;
        __syncthreads();                                         // wsum is written again in the next trip
    }
    key = within_group_max(key, wkey);
    if (threadIdx.x == 0) {
        if (rstart_all) rstart_all[(size_t)sys * (per + 1) + rows] = carry;
        const nbody_cells_info ci = cinfo_all[sys];
        const int largest = (int)(key >> 32), largest_row = rows > 0 ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : 0;
        info_all[sys] = nbody_within_info{carry, n, rows, ci.inside, ci.outside, largest, largest_row};
    }
}

// Stage 3, only where the starts are asked for: grid as stage 1; start[row] = the block's offset + the exclusive prefix inside it.
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void within_block_starts(const Meta* __restrict__ meta_all, int stride, int n_one, int m,
                                                                  const WithinOut* __restrict__ out_all,
                                                                  const long long* __restrict__ boff_all,
                                                                  long long* __restrict__ rstart_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one);
    const int sys = cl.sys, rows = m < 0 ? cl.n : m;
    if ((long long)blockIdx.x * kWithinBlockRows >= rows) return;               // the whole workgroup
    const size_t per = m < 0 ? (size_t)stride : (size_t)m;
    __shared__ long long wsum[kDiagBlock / kWave];
    int v[kWithinScanPer];
    within_load_counts(out_all + (size_t)sys * per, rows, v);
    const int r0 = blockIdx.x * kWithinBlockRows + threadIdx.x * kWithinScanPer;
    long long mine = 0;
#pragma unroll
    for (int u = 0; u < kWithinScanPer; ++u) mine += v[u];
    long long at = boff_all[(size_t)sys * (size_t)gridDim.x + blockIdx.x] + cells_block_prefix<long long, kDiagBlock>(mine, wsum).at;
    long long* __restrict__ rstart = rstart_all + (size_t)sys * (per + 1);
#pragma unroll
    for (int u = 0; u < kWithinScanPer; ++u) {
        if (r0 + u < rows) rstart[r0 + u] = at;
        at += v[u];
    }
}

// One lane per list entry; grid = (ceil(list_stride / kDiagBlock), systems).  raw_all, list_all: [systems * list_stride].
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void within_rank(const Meta* __restrict__ meta_all, int stride, int n_one, int m,
                                                          const long long* __restrict__ rstart_all,
                                                          const int32_t* __restrict__ raw_all, int32_t* __restrict__ list_all,
                                                          long long list_stride) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one);
    const int sys = cl.sys, rows = m < 0 ? cl.n : m;
    const size_t per = m < 0 ? (size_t)stride : (size_t)m;
    const long long* __restrict__ rstart = rstart_all + (size_t)sys * (per + 1);
    const long long total = rows > 0 ? rstart[rows] : 0;
    const long long e = (long long)blockIdx.x * kDiagBlock + threadIdx.x;
    if (total > list_stride || e >= total) return;
    int lo = 0, hi = rows;                                       // rstart[lo] <= e < rstart[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (rstart[mid] <= e) lo = mid; else hi = mid;
    }
    const long long a = rstart[lo], b = rstart[lo + 1];
    if (a < 0 || a > e || b <= e || b > total) return;
    const int32_t* __restrict__ raw = raw_all + (size_t)sys * (size_t)list_stride;
    const int idx = raw[e];
    long long rank = 0;
    for (long long k = a; k < b; ++k) rank += raw[k] < idx ? 1 : 0;
    if (a + rank < b) list_all[(size_t)sys * (size_t)list_stride + a + rank] = idx;
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, next to its CellState: nothing before the first call.
// ---------------------------------------------------------------------------------------------------------
struct WithinState {
    RowPoints pts;
    RowsArray<WithinOut> out;               // [systems * per]: device and pinned
    RowsArray<long long> rstart;            // [systems * (per + 1)]
    RowsArray<long long> blocks;            // device [3][systems * blocks]: the row scan's block sums, keys and offsets
    RowsArray<nbody_within_info> info;      // [systems]
    RowsArray<int32_t> raw;                 // device [systems * list_stride]: the lists as the walk leaves them
    RowsArray<int32_t> list;                // [systems * list_stride]
};

inline void within_free(WithinState& w) {
    rows_free(w.pts); rows_free(w.out); rows_free(w.rstart); rows_free(w.blocks); rows_free(w.info); rows_free(w.raw); rows_free(w.list);
}

inline int within_fail_alloc(WithinState& w, hipError_t e, const char* who, const char* what) {
    within_free(w);
    return rows_alloc_failed(e, who, what);
}

// The argument checks an entry point makes before any device call, the values before the handle; `required`: the handle,
// out and info.  result_systems: the systems whose records share the caller's out.
inline int within_check_args(const char* who, std::initializer_list<const void*> required, const nbody_grid* grid, double h2,
                             int m, const int64_t* start, const int32_t* list, int cap, unsigned long long systems) {
    int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    if (rc != NBODY_OK) return rc;
    if (!(h2 >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: h2 = %g (a squared radius: >= 0, +inf allowed)", who, h2);
    if (list && !start) return nbody_fail(NBODY_ERR_INVALID, "%s: list without start", who);
    if (cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    return rows_check_args(who, required, m, systems * sizeof(nbody_within), " of results");
}

// The call's window values: h once, in cells per axis; a grid too fine for the margin's proof looks at every cell.
inline WithinWin within_window(const nbody_grid& grid, double h2) {
    const double h = sqrt(h2);
    const bool fine = cells_fine(grid);
    return WithinWin{h2, fine ? __builtin_inf() : h * grid.sx, fine ? __builtin_inf() : h * grid.sy};
}

// One call, from the reservation to the caller's arrays; the site, Count and read_meta as for rows_run (nbody_rows.hpp).
// points == NULL: own rows, `stride` apart per system in out and stride + 1 in start; otherwise m and m + 1.  Two waits with
// a list: the counts first - they say whether it fits - then the entries.  On NBODY_ERR_CAPACITY out, start and info are
// complete and list is untouched.
template <typename T, typename Count, typename ReadMeta>
int within_run(const char* who, const RowsSite& s, CellState& g, WithinState& ws, const nbody_grid& grid, double h2,
               const nbody_vec2* points, int m, nbody_within* out, int64_t* start, int32_t* list, int cap, nbody_within_info* info,
               ReadMeta read_meta) {
    static_assert(sizeof(long long) == sizeof(int64_t), "start is copied as it stands");
    const bool own = points == nullptr;
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny, bodies = S * (size_t)s.stride;
    const size_t per = own ? (size_t)s.stride : (size_t)m;
    const int n_one = s.n_one<Count>(), m_dev = own ? -1 : m;
    const int lanes = own ? 2 * s.n_bound : m;
    int rc = cells_reserve(g, S, C, bodies, who, sizeof(CellRec<T>));
    if (rc != NBODY_OK) return rc;
    hipError_t e = rows_reserve(ws.pts, own || m == 0 ? 1 : (size_t)m);
    if (e == hipSuccess) e = rows_reserve(ws.out, S * per > 0 ? S * per : 1);
    if (e == hipSuccess) e = rows_reserve(ws.rstart, S * (per + 1));
    if (e == hipSuccess) e = rows_reserve(ws.info, S);
    const size_t rows_bound = own ? (size_t)s.n_bound : (size_t)m;         // rows of a system that can hold a result
    const size_t nblk = rows_bound > 0 ? (rows_bound + kWithinBlockRows - 1) / kWithinBlockRows : 1;
    if (e == hipSuccess) e = rows_reserve_device(ws.blocks, 3 * S * nblk);
    if (e != hipSuccess) return within_fail_alloc(ws, e, who, "row buffers");
    const Rec<T>* J = (const Rec<T>*)s.J;
    const CellRec<T>* sorted = reinterpret_cast<const CellRec<T>*>(g.sorted.d);
    const WithinWin win = within_window(grid, h2);
    if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
    if (!own && m > 0) NBK_ROWS_TRY(rows_upload(ws.pts, points, m, s.stream));
    const auto walk = [&](auto fill, long long list_stride) {
        constexpr bool kList = decltype(fill)::value;
        if (lanes <= 0) return;
        if (own)
            hipLaunchKernelGGL((within_walk<T, true, Count, kList>), s.grid(lanes), dim3(kDiagBlock), 0, s.stream, J,
                               sorted, s.meta, s.stride, n_one, grid, win, (const int32_t*)g.cell_of.d,
                               (const int32_t*)g.start.d, (const FieldPoint*)nullptr, 0, ws.out.d, (const long long*)ws.rstart.d,
                               ws.raw.d, list_stride);
        else
            hipLaunchKernelGGL((within_walk<T, false, Count, kList>), s.grid(lanes), dim3(kDiagBlock), 0, s.stream, J,
                               sorted, s.meta, s.stride, n_one, grid, win, (const int32_t*)g.cell_of.d,
                               (const int32_t*)g.start.d, (const FieldPoint*)ws.pts.d, m, ws.out.d, (const long long*)ws.rstart.d,
                               ws.raw.d, list_stride);
    };
    walk(std::false_type{}, 0);
    NBK_ROWS_TRY(hipGetLastError());
    long long* bsum = ws.blocks.d;
    unsigned long long* bkey = reinterpret_cast<unsigned long long*>(ws.blocks.d + S * nblk);
    long long* boff = ws.blocks.d + 2 * S * nblk;
    const dim3 per_block((unsigned)nblk, (unsigned)S);
    if (rows_bound > 0) {
        hipLaunchKernelGGL((within_block_sums<Count>), per_block, dim3(kDiagBlock), 0, s.stream, s.meta, s.stride, n_one, m_dev,
                           (const WithinOut*)ws.out.d, bsum, bkey);
        NBK_ROWS_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((within_block_scan<Count>), dim3(1, (unsigned)S), dim3(kDiagBlock), 0, s.stream, s.meta, s.stride, n_one,
                       m_dev, (int)nblk, (const long long*)bsum, (const unsigned long long*)bkey, boff,
                       start ? ws.rstart.d : (long long*)nullptr, (const nbody_cells_info*)g.info.d, ws.info.d);
    NBK_ROWS_TRY(hipGetLastError());
    if (start && rows_bound > 0) {
        hipLaunchKernelGGL((within_block_starts<Count>), per_block, dim3(kDiagBlock), 0, s.stream, s.meta, s.stride, n_one, m_dev,
                           (const WithinOut*)ws.out.d, (const long long*)boff, ws.rstart.d);
        NBK_ROWS_TRY(hipGetLastError());
    }
    const size_t out_n = Count::kBatch ? S * per : rows_bound, start_n = Count::kBatch ? S * (per + 1) : rows_bound + 1;
    if (out_n > 0) NBK_ROWS_TRY(hipMemcpyAsync(ws.out.h, ws.out.d, out_n * sizeof(WithinOut), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipMemcpyAsync(ws.info.h, ws.info.d, S * sizeof(nbody_within_info), hipMemcpyDeviceToHost, s.stream));
    if (start) NBK_ROWS_TRY(hipMemcpyAsync(ws.rstart.h, ws.rstart.d, start_n * sizeof(long long), hipMemcpyDeviceToHost, s.stream));
    rc = s.sync<Count>(true, read_meta);
    if (rc != NBODY_OK) return rc;
    memcpy(info, ws.info.h, S * sizeof(nbody_within_info));
    const WithinOut* h_out = reinterpret_cast<const WithinOut*>(ws.out.h);
    const long long* h_start = reinterpret_cast<const long long*>(ws.rstart.h);
    int over = -1;
    long long most = 0;                                          // the longest list of a system
    for (size_t sys = 0; sys < S; ++sys) {                       // a system's rows and rows + 1 starts; the rest stays
        const size_t rows = (size_t)(info[sys].rows < 0 ? 0 : info[sys].rows);
        if (rows > rows_bound) return nbody_fail(NBODY_ERR_STATE, "%s: system %zu has %zu rows, the launch covered %zu", who, sys, rows, rows_bound);
        if (rows > 0) memcpy(out + sys * per, h_out + sys * per, rows * sizeof(WithinOut));
        if (start) memcpy(start + sys * (per + 1), h_start + sys * (per + 1), (rows + 1) * sizeof(long long));
        if (info[sys].total > (int64_t)cap && over < 0) over = (int)sys;
        if (info[sys].total > most) most = info[sys].total;
    }
    if (!list) return NBODY_OK;
    if (over >= 0)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: room for %d list entries, system %d has %lld: call again with that cap", who, cap,
                          over, (long long)info[over].total);
    if (most == 0) return NBODY_OK;
    e = rows_reserve_device(ws.raw, S * (size_t)most);
    if (e == hipSuccess) e = rows_reserve(ws.list, S * (size_t)most);
    if (e != hipSuccess) return within_fail_alloc(ws, e, who, "list buffers");
    walk(std::true_type{}, most);
    NBK_ROWS_TRY(hipGetLastError());
    hipLaunchKernelGGL((within_rank<Count>), dim3((unsigned)((most + kDiagBlock - 1) / kDiagBlock), (unsigned)S), dim3(kDiagBlock), 0,
                       s.stream, s.meta, s.stride, n_one, m_dev, (const long long*)ws.rstart.d, (const int32_t*)ws.raw.d, ws.list.d,
                       most);
    NBK_ROWS_TRY(hipGetLastError());
    size_t used = 0;                                             // entries of the staging up to the last one written
    for (size_t sys = 0; sys < S; ++sys)
        if (info[sys].total > 0) used = sys * (size_t)most + (size_t)info[sys].total;
    NBK_ROWS_TRY(hipMemcpyAsync(ws.list.h, ws.list.d, used * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
    const int32_t* h_list = reinterpret_cast<const int32_t*>(ws.list.h);
    for (size_t sys = 0; sys < S; ++sys)
        if (info[sys].total > 0)
            memcpy(list + sys * (size_t)cap, h_list + sys * (size_t)most, (size_t)info[sys].total * sizeof(int32_t));
    return NBODY_OK;
}

}  // namespace nbk
