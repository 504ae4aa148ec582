// csrc/nbody_pairs_grid.hpp -- pair counts and bound pairs on the cell list (nbody_get_pair_counts_grid,
// nbody_get_binaries_grid and their batch forms, include/nbody.h): the binned pair histogram of
// nbody_get_pair_counts and the binaries of nbody_get_binaries, restricted to the bodies inside a caller-given grid and found
// by walking the cells around every row instead of all n sources per row - O(n) on a grid matched to the top edge or to the
// separation, where the tile walks of nbody_pairs.hpp and nbody_binaries.hpp are O(n^2).  Included after nbody_within.hpp,
// nbody_pairs.hpp and nbody_binaries.hpp by both translation units: one system (nbody_ctx.hip) and a batch (nbody_batch.hip:
// system = blockIdx.y, per-body arrays `stride` apart, one grid, one set of points and edges for every system) share each of
// the two new kernels.
//
// The definitions (include/nbody.h has them in full).  IEEE fp64, every operation rounded on its own, no fma.  The sources
// are the bodies with inside(j) of the cell sums.
//   Pair counts: d2, counts[k], below and the derived rest of nbody_get_pair_counts, bit for bit, over the counted pairs - own
//   form: the unordered pairs of inside bodies, pairs = inside * (inside - 1) / 2, rows = n; points form: every (point, inside
//   body) pair, pairs = m * inside, rows = m, a point may lie anywhere.
//   Binaries: nbody_get_binaries, bit for bit, over the pairs i < j of inside bodies, indices those of the state; coincident
//   counts the pairs of inside bodies at d2 == 0 - two such bodies share a cell and are always seen.
// Counts are integers and the list is sorted by (i, j) on the host: neither depends on the order of the visit, so the cells are
// walked as they lie and the results have the bits of the brute-force definitions - PROVIDED the window holds every cell that
// can hold a counted or near source.  What follows, and is tested:
//   - with outside == 0 the counts, below, rest and pairs, and the list and every count of the binaries, are the bytes of the
//     plain calls, whatever the grid;
//   - with any grid they are what the plain calls give on a context holding exactly the inside bodies (indices mapped back);
//   - with outside == 0 and own rows, 2 * counts[0] at edges2 = {0, nextafter(h2, +inf)} is the sum of nbody_get_within's count
//     at h2;  near + coincident == counts[0] of the pair counts on the same grid at {0, nextafter(sep2, +inf)}.
//
// The window: the fixed-radius rule of the radius queries (nbody_within.hpp; DESIGN.md 4.21 has the proof) with h2 = the top
// edge edges2[bins], or sep2 - the same host computation (within_window), the same cells_fine escape, the same cells_span.
// The window covers d2 <= h2; the pair counts count d2 < top, so a pair exactly at the top edge is walked and not counted; the
// binaries take d2 <= sep2.  A top edge or a sep2 of +inf is legal: the whole grid, correct and slow.
//
// Kernels, on the handle's stream after the four list stages of the cell sums (cells_list_run) and the gather of the sorted
// records {x, y, r, j} (cells_gather_run):
//   pair_counts_grid<T, kOwn, Count>  own form: one lane per slot q < inside of the cell list (lane = slot, as
//                             groups_grid_sweep); points form: one lane per point in the order given.  cells_window_walk over
//                             the lane's window; per candidate 2 subtractions, 2 multiplies, 1 add and the compare with the
//                             top edge - and, own form, s.j < self: a pair is seen from both ends and counted at the higher.
//                             A counted candidate: pair_slot over the edges in LDS (nbody_pairs.hpp), one 64-bit LDS atomicAdd
//                             into the workgroup's histogram; one barrier; the flush of pair_counts.  The passing branch is
//                             NOT rare here: on a matched grid about pi / 9 of the candidates of a 3 x 3 window pass.
//   binaries_grid_walk<T, Count>  one lane per slot.  The hot compare is d2 <= sep2 && s.j < self on the sorted records alone;
//                             a passing pair gathers the mass and the velocity of the source by index from J and V (the
//                             row's own are read once, before the walk) and does exactly the arithmetic of
//                             BinFour::close_pair in the same orientation: the row is the higher index, the record is
//                             {lower, higher}.  The lane's counts are summed over the wave by rows_wave_add.
// THE RULE OF THIS FILE.  within_walk and groups_grid_sweep let a lane without a row return early, because no barrier follows.
// Here one does: pair_counts_grid has a __syncthreads() before its flush and binaries_grid_walk a wave reduction at its end.
// A workgroup may leave as a whole before the first barrier, on a workgroup-uniform condition (no row in it: a system with a
// bad count has inside == 0 and leaves there).  After that NO LANE RETURNS: a lane without a row (q >= inside, a record that
// fails its check) stays, is predicated off the walk and reaches every barrier and every shuffle.  A lane that left between
// the first and the last barrier is how such a kernel hangs a card.
// Every index that comes out of memory (a start of a cell, the j of a record before it indexes J or V) is range-checked
// before it is used as one.  No device-side waiting, no retry loop, plain stores and atomics only.  No scratch; registers and
// LDS: DESIGN.md 4.24.
//
// Cost by counting: the list stages and the gather as for the radius queries; then, on a grid matched to h, 9 cells of about
// 4 bodies each per row - about 36 candidates instead of n, 16 (32) bytes each from L2 - and pi / 9 of them pass.
// Measured (profiles/pairs_grid_probe.txt; one MI355X, fp32, n = 130965, the stock state after 3 steps, the matched grid
// within_grid(field, h); medians of 3 rounds of a kernel trace, the plain kernels in the same run): pair_counts_grid 0.014 and
// 0.022 ms with 32 bins up to 381.8 and 824.8, the list stages and the gather 0.183 and 0.066 ms, against pair_counts 5.37 and
// 5.57 ms; binaries_grid_walk 0.019 ms at sep = 128 and 0.122 ms at sep = 1024 with the counts only, 0.960 ms with the list of
// 652339 records (binaries_walk: 5.38, 5.79 and 9.25 ms), the stages 0.615 ms on 1024 x 1024 cells and 0.052 on 195 x 195.  Whole
// counts-only calls 0.14 - 0.68 ms against 5.3 - 5.7 ms.  On 1 x 1 cells the walks take 13.3 and 12.2 ms and lose; a batch of
// 256 x 1024 wins in kernels (0.06 - 0.07 against 0.12 - 0.16 ms) and, as a whole call,
// loses for the listed binaries, is level for the pair counts and wins for the counts-only binaries.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_cells.hpp"
#include "nbody_within.hpp"
#include "nbody_pairs.hpp"
#include "nbody_binaries.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_pair_grid_info) == 56 && offsetof(nbody_pair_grid_info, rest) == 32 &&
              offsetof(nbody_pair_grid_info, inside) == 40 && offsetof(nbody_pair_grid_info, outside) == 48,
              "nbody_pair_grid_info layout: nbody_pair_info, then inside and outside");
static_assert(sizeof(nbody_binary_grid_info) == 72 && offsetof(nbody_binary_grid_info, sep2) == 48 &&
              offsetof(nbody_binary_grid_info, inside) == 56 && offsetof(nbody_binary_grid_info, outside) == 64,
              "nbody_binary_grid_info layout: nbody_binary_info, then inside and outside");

// grid = (ceil(rows / kDiagBlock), systems) with rows = n_bound for the own form (lane q < inside is slot q) and m for points.
// edges2: bins + 1 squared edges; hist_all: bins + 1 counters per system, cleared by the host - slot 0 is `below`, slot k + 1
// is counts[k] (the layout of pair_counts).
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void pair_counts_grid(const CellRec<T>* __restrict__ sorted_all,
                                                               const Meta* __restrict__ meta_all, int stride, int n_one,
                                                               const nbody_grid g, const WithinWin win,
                                                               const int32_t* __restrict__ start_all,
                                                               const FieldPoint* __restrict__ points, int m,
                                                               const double* __restrict__ edges2, int bins,
                                                               unsigned long long* __restrict__ hist_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    const int rows = kOwn ? cl.inside : m;
    // the whole workgroup, before any barrier: no row in it, or no source in the system (a bad count: inside == 0)
    if ((int)(blockIdx.x * kDiagBlock) >= rows || cl.inside == 0) return;
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const int tid = threadIdx.x, q = blockIdx.x * kDiagBlock + tid;
    __shared__ double se[kPairEdgeSlots];
    __shared__ unsigned long long hist[kPairMaxBins + 1];
    for (int k = tid; k < kPairEdgeSlots; k += kDiagBlock) se[k] = k < bins ? edges2[k] : __builtin_inf();
    for (int k = tid; k <= bins; k += kDiagBlock) hist[k] = 0;
    int first = 1;
    while (2 * first <= bins) first *= 2;                        // 2^(ceil(log2(bins + 1)) - 1): workgroup-uniform
    const double top = edges2[bins];

    // the lane's row; a lane without one stays (the rule of this file) and walks nothing
    bool valid = false;
    int self = -1;
    double x = 0.0, y = 0.0;
    if (q < rows) {
        if (kOwn) {
            const CellRec<T> w = sorted[q];
            if ((unsigned)w.j < (unsigned)cl.n) { valid = true; self = w.j; x = (double)w.x; y = (double)w.y; }
        } else {
            const FieldPoint p = points[q];
            valid = true; x = p.x; y = p.y;
        }
    }
    __syncthreads();                                             // the edges and the zeroed histogram are in LDS
    if (valid) {
        const CellCoords t = cells_coords(g, x, y);
        cells_window_walk(cl, sorted, g, t.tx, t.ty, win.wx0, win.wy0, [&](const CellRec<T>& s) {
            const double dx = (double)s.x - x, dy = (double)s.y - y;
            const double d2 = (dx * dx) + (dy * dy);
            if (d2 < top && (!kOwn || (s.j < self && s.j >= 0)))   // not rare: about pi / 9 of a matched window
                atomicAdd(hist + pair_slot(se, first, d2), 1ull);
        });
    }
    __syncthreads();                                             // every LDS count of the workgroup is in
    unsigned long long* __restrict__ out = hist_all + (size_t)cl.sys * (size_t)(bins + 1);
    for (int k = tid; k <= bins; k += kDiagBlock) {
        const unsigned long long v = hist[k];
        if (v) atomicAdd(out + k, v);
    }
}

// grid = (ceil(n_bound / kDiagBlock), systems), lane q < inside is slot q.  V_all: the velocities, indexed like J_all.
// log_all: cap records per system; cnt_all: one BinCounts per system, cleared by the host.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void binaries_grid_walk(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                                 const CellRec<T>* __restrict__ sorted_all,
                                                                 const Meta* __restrict__ meta_all, int stride, int n_one,
                                                                 const nbody_grid g, const WithinWin win,
                                                                 const int32_t* __restrict__ start_all,
                                                                 BinRaw* __restrict__ log_all, int cap,
                                                                 BinCounts* __restrict__ cnt_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    if ((int)(blockIdx.x * kDiagBlock) >= cl.inside) return;     // the whole workgroup; from here on no lane returns
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const Rec<T>* __restrict__ J = J_all + cl.at;
    const Vec2<T>* __restrict__ V = V_all + cl.at;
    const int q = blockIdx.x * kDiagBlock + threadIdx.x, n = cl.n;
    BinCounts* cnt = cnt_all + cl.sys;
    BinRaw* __restrict__ log = log_all + (size_t)cl.sys * (size_t)cap;
    unsigned n_near = 0u, n_coin = 0u, n_over = 0u, n_appr = 0u, n_bound = 0u;

    bool valid = false;
    int self = -1;
    BinRow w{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (q < cl.inside) {
        const CellRec<T> me = sorted[q];
        if ((unsigned)me.j < (unsigned)n) {
            valid = true; self = me.j;
            const Rec<T> b = J[self];
            const Vec2<T> v = V[self];
            w = BinRow{(double)me.x, (double)me.y, (double)b.m, (double)me.r, (double)v.x, (double)v.y};
        }
    }
    if (valid) {
        const double sep2 = win.h2, g2 = 2.0 * (double)kG;
        const CellCoords t = cells_coords(g, w.x, w.y);
        cells_window_walk(cl, sorted, g, t.tx, t.ty, win.wx0, win.wy0, [&](const CellRec<T>& s) {
            const double dx = (double)s.x - w.x, dy = (double)s.y - w.y;
            const double d2 = (dx * dx) + (dy * dy);
            if (d2 <= sep2 && s.j < self && s.j >= 0) {          // the rest only for a pair that passes: BinFour::close_pair's
                const bool coincident = d2 == 0.0;
                n_coin += coincident ? 1u : 0u;
                n_near += coincident ? 0u : 1u;
                if (!coincident) {
                    const Rec<T> sb = J[s.j];
                    const Vec2<T> sv = V[s.j];
                    const double dvx = (double)sv.x - w.vx, dvy = (double)sv.y - w.vy;
                    const double v2 = (dvx * dvx) + (dvy * dvy);
                    const double mu = g2 * (w.m + (double)sb.m);
                    const double ww = (v2 * v2) * d2;
                    const double k = mu * mu;
                    if (0.0 < mu && k < __builtin_inf() && ww < k) {
                        const double hz = (dx * dvy) - (dy * dvx);
                        const double b = (dx * dvx) + (dy * dvy);
                        const double sum = w.r + (double)s.r;
                        const unsigned flags = (d2 <= sum * sum ? (unsigned)NBODY_BINARY_OVERLAP : 0u) |
                                               (b < 0.0 ? (unsigned)NBODY_BINARY_APPROACHING : 0u);
                        if (cap > 0) {                           // uniform over the launch
                            const unsigned long long slot = atomicAdd(&cnt->pairs, 1ull);
                            if (slot < (unsigned long long)cap) log[slot] = BinRaw{s.j, self, flags, 0u, d2, v2, mu, hz};
                        } else {
                            n_bound += 1u;                       // the counts only: no slot to ask for
                        }
                        n_over += flags & NBODY_BINARY_OVERLAP ? 1u : 0u;
                        n_appr += flags & NBODY_BINARY_APPROACHING ? 1u : 0u;
                    }
                }
            }
        });
    }
    // one atomic per wave and count: every lane of the workgroup is here, none has returned since the first line
    rows_wave_add<5>({&cnt->near, &cnt->coincident, &cnt->overlapping, &cnt->approaching, &cnt->pairs},
                     {n_near, n_coin, n_over, n_appr, n_bound});
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  No buffers of its own: the cell list and its sorted records of CellState, the edges, histograms and points of
// PairsState, the log and the counters of BinState - each allocated by whichever query of the handle asks first.
// ---------------------------------------------------------------------------------------------------------

// The argument checks before any device call, the values before the handle: the grid as the cell sums check it, then what
// the plain calls check.
inline int pairs_grid_check_args(const char* who, std::initializer_list<const void*> required, const nbody_grid* grid, int m,
                                 const double* edges2, int bins, unsigned long long systems) {
    const int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    return rc != NBODY_OK ? rc : pairs_check_args(who, required, m, edges2, bins);
}

inline int binaries_grid_check_args(const char* who, const void* handle, const nbody_grid* grid, double sep2, const nbody_binary* out,
                                    int cap, const nbody_binary_grid_info* info, unsigned long long systems) {
    const int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    if (rc != NBODY_OK) return rc;
    return pair_log_check_args(who, handle, BinQuery{sep2}, out, cap, reinterpret_cast<const nbody_binary_info*>(info), systems);
}

// The inside bodies of system sys as the host counts them: the cell list's, held to [0, n].
inline int64_t pairs_grid_inside(const CellState& g, int sys, int64_t n) {
    const int64_t inside = n ? reinterpret_cast<const nbody_cells_info*>(g.info.h)[sys].inside : 0;
    return inside < 0 ? 0 : inside > n ? n : inside;
}

// One call, from the reservation to the caller's counts; the site, Count and read_meta as for rows_run (nbody_rows.hpp).  The
// list stages run wherever a system can hold a body - info.inside comes from them - the walk only where there is a row.
template <typename T, typename Count, typename ReadMeta>
int pairs_grid_run(const char* who, const RowsSite& s, CellState& g, PairsState& ps, const nbody_grid& grid, const nbody_vec2* points,
                   int m, const double* edges2, int bins, uint64_t* counts, nbody_pair_grid_info* info, ReadMeta read_meta) {
    const bool own = points == nullptr;
    const int rows = own ? s.n_bound : m;                                  // what the grid of lanes covers
    const size_t S = (size_t)s.systems, slots = (size_t)bins + 1, C = (size_t)grid.nx * (size_t)grid.ny;
    const bool listed = s.n_bound > 0, launched = listed && rows > 0;
    if (listed) {
        int rc = cells_reserve(g, S, C, S * (size_t)s.stride, who, sizeof(CellRec<T>));
        if (rc != NBODY_OK || (rc = pairs_reserve(ps, S, own ? 0 : (size_t)m, who)) != NBODY_OK) return rc;
        if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    }
    if (launched) {
        const CellRec<T>* sorted = reinterpret_cast<const CellRec<T>*>(g.sorted.d);
        const WithinWin win = within_window(grid, edges2[bins]);
        const int n_one = s.n_one<Count>();
        memcpy(ps.h, edges2, slots * sizeof(double));
        NBK_ROWS_TRY(hipMemcpyAsync(ps.edges, ps.h, slots * sizeof(double), hipMemcpyHostToDevice, s.stream));
        NBK_ROWS_TRY(hipMemsetAsync(ps.hist, 0, S * slots * sizeof(unsigned long long), s.stream));
        if (own) {
            hipLaunchKernelGGL((pair_counts_grid<T, true, Count>), s.grid(rows), dim3(kDiagBlock), 0, s.stream, sorted, s.meta, s.stride,
                               n_one, grid, win, (const int32_t*)g.start.d, (const FieldPoint*)nullptr, 0, (const double*)ps.edges,
                               bins, ps.hist);
        } else {
            NBK_ROWS_TRY(rows_upload(ps.pts, points, m, s.stream));
            hipLaunchKernelGGL((pair_counts_grid<T, false, Count>), s.grid(rows), dim3(kDiagBlock), 0, s.stream, sorted, s.meta, s.stride,
                               n_one, grid, win, (const int32_t*)g.start.d, (const FieldPoint*)ps.pts.d, m, (const double*)ps.edges,
                               bins, ps.hist);
        }
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(ps.h + (kPairMaxBins + 1) * sizeof(double), ps.hist, S * slots * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(listed, read_meta);
    if (rc != NBODY_OK) return rc;
    const unsigned long long* h =
        launched ? reinterpret_cast<const unsigned long long*>(ps.h + (kPairMaxBins + 1) * sizeof(double)) : nullptr;
    for (int sys = 0; sys < s.systems; ++sys) {
        const int64_t n = s.count(sys);
        const int64_t in = listed ? pairs_grid_inside(g, sys, n) : 0;
        const int64_t r = own ? n : (int64_t)m;
        const int64_t pairs = own ? in * (in - 1) / 2 : r * in;
        uint64_t* out = counts + (size_t)sys * (size_t)bins;
        uint64_t below = 0, binned = 0;
        for (int k = 0; k < bins; ++k) out[k] = 0;
        if (h && pairs > 0) {
            const unsigned long long* hs = h + (size_t)sys * slots;
            below = hs[0];
            for (int k = 0; k < bins; ++k) {
                out[k] = hs[k + 1];
                binned += hs[k + 1];
            }
        }
        info[sys] = nbody_pair_grid_info{n, r, pairs, (int64_t)below, pairs - (int64_t)below - (int64_t)binned, in, n - in};
    }
    return NBODY_OK;
}

// The pair-log driver's sibling for the walk over the cells (pair_log_run, nbody_rows.hpp: the encounters and the plain
// binaries keep their launches, waits and bytes).  The list stages and the gather before the launch, the cell list's info with
// the counters; everything after the first wait - the counters, the cap rule, the second wait, the host half - is the
// driver's own tail, pair_log_tail, with an info writer that adds inside and outside.
template <typename T, typename Count, typename ReadMeta>
int binaries_grid_run(const char* who, const RowsSite& s, const void* V, CellState& g, BinState& bs, const nbody_grid& grid, double sep2,
                      nbody_binary* out, int cap, nbody_binary_grid_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny;
    const bool launched = s.n_bound > 0;
    const BinQuery q{sep2};
    if (launched) {
        int rc = cells_reserve(g, S, C, S * (size_t)s.stride, who, sizeof(CellRec<T>));
        if (rc != NBODY_OK || (rc = pair_log_reserve(bs, S, (size_t)cap, who)) != NBODY_OK) return rc;
        if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemsetAsync(bs.cnt.d, 0, S * sizeof(BinCounts), s.stream));
        hipLaunchKernelGGL((binaries_grid_walk<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Rec<T>*)s.J,
                           (const Vec2<T>*)V, reinterpret_cast<const CellRec<T>*>(g.sorted.d), s.meta, s.stride, s.n_one<Count>(), grid,
                           within_window(grid, sep2), (const int32_t*)g.start.d, bs.log.d, cap, bs.cnt.d);
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(bs.cnt.h, bs.cnt.d, S * sizeof(BinCounts), hipMemcpyDeviceToHost, s.stream));
        NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    return pair_log_tail(who, s, bs, q, launched, out, cap, [&](int sys, int64_t n, const BinCounts& c) {
        const int64_t in = launched ? pairs_grid_inside(g, sys, n) : 0;
        const nbody_binary_info bi = q.info(n, c);
        info[sys] = nbody_binary_grid_info{bi.n_bodies, bi.pairs, bi.near, bi.coincident, bi.overlapping, bi.approaching, bi.sep2, in, n - in};
    });
}

}  // namespace nbk
