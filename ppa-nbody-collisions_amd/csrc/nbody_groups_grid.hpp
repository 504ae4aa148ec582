// csrc/nbody_groups_grid.hpp -- group finding on the cell list (nbody_get_groups_grid, nbody_batch_get_groups_grid,
// include/nbody.h): the friends-of-friends labels of nbody_get_groups, restricted to the bodies inside a
// caller-given grid, found by walking the cells around every body instead of all n sources per row - O(n) per sweep on a
// grid matched to the reach of a typical body, where the triangular walk of nbody_groups.hpp is O(n^2).  Included after
// nbody_groups.hpp and nbody_within.hpp by both translation units: one system (nbody_ctx.hip) and a batch (nbody_batch.hip:
// system = blockIdx.y, per-body arrays `stride` apart, one grid for every system) share the one new kernel.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  linked(i, j) is
// the predicate of nbody_get_groups, bit for bit, between two bodies that are both inside(.) of the cell sums:
//     dx = X_j - X_i;  dy = Y_j - Y_i;  d2 = (dx*dx) + (dy*dy);  s = (radius_scale * (R_i + R_j)) + link;  d2 <= s*s
// A body outside the grid is linked to nobody.  label[i] = the lowest index of i's component: an integer function of the SET
// of links, so the cells are walked as they lie and the labels have the bits of the brute-force definition - PROVIDED every
// link is seen from at least one of its two ends.
//
// The window: the larger end finds the pair (DESIGN.md 4.22 has the derivation; tests/groups_grid_cases.py restates it).  Row
// i, with a = |R_i|, looks for the sources whose |radius| is at most its own:
//     S_i = (radius_scale * (a + a)) + link;   h2_i = S_i * S_i            the roundings of s
// For |R_j| <= a: |fl(R_i + R_j)| <= 2a, so |s_ij| <= S_i (rounding is monotone, radius_scale and link are >= 0), so
// fl(s_ij * s_ij) <= h2_i: a linked j has d2 <= h2_i.  Of the two ends of a link one has the other's |radius| <= its own.
// The cells of row i are cells_span's with w0 = fl(S_i * sx) and fl(S_i * sy), per lane; a grid of more than 2^400 cells per
// unit length means every cell (`fine`, from the host: cells_fine); S_i = +inf means every cell through cells_span as it
// stands; a NaN S_i (a NaN radius, or radius_scale = 0 with an infinite one) links nothing in the definition either - every
// s_ij of that row is NaN - and the lane leaves.
// One body ten times the typical size widens its own window only: the price is that one lane walks it.
//
// Kernels, on the handle's stream: the four list stages of the cell sums (cells_list_run), the gather of the list's sorted
// {x, y, r, j} records (cells_gather_run; the buffer the radius queries walk), groups_init, then groups_grid_sweep until a
// sweep changes nothing, then groups_flatten - groups_init, groups_find, groups_hook, groups_flatten and GroupsState as
// nbody_groups.hpp has them.  Bodies outside the grid get no lane: groups_init leaves them their own root.
//   groups_grid_sweep<T, Count>  one lane per slot q < inside of the cell list (lane = slot: the 64 rows of a wave share a few
//                             cells).  The row-of-cells ranges of the lane's window are walked by cells_window_walk
//                             (nbody_cells.hpp), the walk of within_walk: four records loaded ahead of their pairs.
//                             Per pair: 2 subtractions, 2 multiplies, 1 add and the compare with the lane's h2_i (and
//                             j != self); behind that branch the exact predicate - s from both radii, d2 <= s*s, which
//                             may still fail, or hold for a j of larger radius: a true link is a true link - and
//                             groups_hook.  No j < i: the end that sees a pair may be either.
// The `changed` words are groups_sweep's: set where unequal roots are SEEN; a batch's words of the last sweep are read at the
// prologue and a system that had converged leaves there as a whole workgroup; the host reads 4 bytes per system after each
// sweep and gives up after n_bound + 1.  The proofs of nbody_groups.hpp - a find ends, a sweep that sets no word has seen
// every linked pair under one root, each other sweep removes a root - never use the order of the walk, nor that a pair is
// visited once: they hold for any walk that visits every link at least once per sweep, which the window rule provides.
// No device-side waiting, no retry loop, plain stores and atomicMin only.  Every index that comes out of memory (a start of a
// cell, a j of a record) is range-checked before it is used as one.  A batch's count goes through batch_checked_count;
// cells_assign has reported a bad one, every kernel here treats that system as empty.  No scratch; registers: DESIGN.md 4.22.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_cells.hpp"
#include "nbody_within.hpp"
#include "nbody_groups.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_groups_grid_info) == 24 && offsetof(nbody_groups_grid_info, inside) == 16, "nbody_groups_grid_info layout");

// One lane per slot; grid = (ceil(n_bound / kDiagBlock), systems).  prev / cur: the systems' `changed` words of the last
// sweep and of this one.  fine: every cell (cells_fine).
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void groups_grid_sweep(const CellRec<T>* __restrict__ sorted_all,
                                                                const Meta* __restrict__ meta_all, int stride, int n_one,
                                                                const nbody_grid g, double link, double scale, int fine,
                                                                const int32_t* __restrict__ start_all, int32_t* parent_all,
                                                                const int* __restrict__ prev, int* __restrict__ cur) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    if (prev[cl.sys] == 0) return;                               // converged in an earlier sweep: the whole workgroup
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const int q = blockIdx.x * kDiagBlock + threadIdx.x, n = cl.n;
    if (q >= cl.inside) return;                                  // no barrier follows
    const CellRec<T> me = sorted[q];
    const int self = me.j;
    if ((unsigned)self >= (unsigned)n) return;
    const double x = (double)me.x, y = (double)me.y, r = (double)me.r;
    const double a = fabs(r);
    const double S = (scale * (a + a)) + link;                   // >= every |s| of this row with a source of no larger |radius|
    if (S != S) return;                                          // every s of this row is NaN: it links nothing
    const double h2 = S * S;
    const double inf = __builtin_inf();
    const CellCoords t = cells_coords(g, x, y);
    int32_t* parent = parent_all + cl.at;
    int* changed = cur + cl.sys;
    cells_window_walk(cl, sorted, g, t.tx, t.ty, fine ? inf : S * g.sx, fine ? inf : S * g.sy, [&](const CellRec<T>& s) {
        const double dx = (double)s.x - x, dy = (double)s.y - y;
        const double d2 = (dx * dx) + (dy * dy);
        if (d2 <= h2 && s.j != self) {                           // the rest only for a pair that passes
            const double sum = (scale * (r + (double)s.r)) + link;
            if (d2 <= sum * sum && (unsigned)s.j < (unsigned)n) groups_hook(parent, changed, self, s.j);
        }
    });
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  No buffers of its own: the cell list and its sorted records of CellState, the parents and labels of GroupsState -
// each allocated by whichever query of the handle asks first.
// ---------------------------------------------------------------------------------------------------------

// The argument checks an entry point makes before any device call, the values before the handle: the grid as the cell sums
// check it, then the link, the scale and the pointers as nbody_get_groups does.
inline int groups_grid_check_args(const char* who, std::initializer_list<const void*> required, const nbody_grid* grid, double link,
                                  double radius_scale, unsigned long long systems) {
    const int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    return rc != NBODY_OK ? rc : groups_check_args(who, link, radius_scale, required);
}

// One call, from the reservation to the caller's labels; the site, Count and read_meta as for rows_run (nbody_rows.hpp).  One
// wait per sweep and one at the end.  The host loop is groups_run's (nbody_groups.hpp) with another sweep; it is written
// out here as well, because a shared driver would name groups_sweep before groups_init and move both in the code object.
template <typename T, typename Count, typename ReadMeta>
int groups_grid_run(const char* who, const RowsSite& s, CellState& g, GroupsState& gs, const nbody_grid& grid, double link,
                    double radius_scale, int32_t* label, nbody_groups_grid_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny, total = S * (size_t)s.stride;
    int sweeps = 0;
    if (s.n_bound > 0) {
        int rc = cells_reserve(g, S, C, total, who, sizeof(CellRec<T>));
        if (rc != NBODY_OK || (rc = groups_reserve(gs, total, S, who)) != NBODY_OK) return rc;
        const dim3 per_body = s.grid(s.n_bound), block(kDiagBlock);
        const int n_one = s.n_one<Count>(), fine = cells_fine(grid);
        int* h_changed = reinterpret_cast<int*>(gs.h + total * sizeof(int32_t));
        if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
        hipLaunchKernelGGL((groups_init<Count>), per_body, block, 0, s.stream, gs.parent, s.stride, s.n_bound);
        NBK_ROWS_TRY(hipGetLastError());
        int* prev = gs.changed;
        int* cur = gs.changed + S;
        NBK_ROWS_TRY(hipMemsetAsync(prev, 1, S * sizeof(int), s.stream));          // every system takes part in sweep 1
        bool again = true;
        while (again) {
            if (sweeps > s.n_bound)
                return nbody_fail(NBODY_ERR_HIP, "%s: did not converge in %d sweeps over at most %d bodies", who, sweeps, s.n_bound);
            NBK_ROWS_TRY(hipMemsetAsync(cur, 0, S * sizeof(int), s.stream));
            hipLaunchKernelGGL((groups_grid_sweep<T, Count>), per_body, block, 0, s.stream, reinterpret_cast<const CellRec<T>*>(g.sorted.d),
                               s.meta, s.stride, n_one, grid, link, radius_scale, fine, (const int32_t*)g.start.d, gs.parent,
                               (const int*)prev, cur);
            NBK_ROWS_TRY(hipGetLastError());
            ++sweeps;
            NBK_ROWS_TRY(hipMemcpyAsync(h_changed, cur, S * sizeof(int), hipMemcpyDeviceToHost, s.stream));
            NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
            again = false;
            for (size_t k = 0; k < S; ++k) again = again || h_changed[k] != 0;
            int* t = prev; prev = cur; cur = t;
        }
        hipLaunchKernelGGL((groups_flatten<T, Count>), per_body, block, 0, s.stream, (const Rec<T>*)s.J, s.meta, s.counters, s.stride,
                           n_one, (const int32_t*)gs.parent, gs.label);
        NBK_ROWS_TRY(hipGetLastError());
        const size_t copied = Count::kBatch ? total : (size_t)s.n_bound;
        NBK_ROWS_TRY(hipMemcpyAsync(gs.h, gs.label, copied * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
        NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(s.n_bound > 0, read_meta);
    if (rc != NBODY_OK) return rc;
    std::vector<int32_t> size;
    for (int sys = 0; sys < s.systems; ++sys) {
        const int n = s.count(sys);
        const int32_t* h = n ? reinterpret_cast<const int32_t*>(gs.h) + (size_t)sys * (size_t)s.stride : nullptr;   // no staging yet
        if (n) memcpy(label + (size_t)sys * (size_t)s.stride, h, (size_t)n * sizeof(int32_t));
        nbody_groups_info gi;
        groups_summarise(h, n, sweeps, size, &gi);
        int inside = n ? reinterpret_cast<const nbody_cells_info*>(g.info.h)[sys].inside : 0;    // the cell list's
        inside = inside < 0 ? 0 : inside > n ? n : inside;
        info[sys] = nbody_groups_grid_info{gi.n_bodies, gi.n_groups, gi.largest, gi.sweeps, inside, n - inside};
    }
    return NBODY_OK;
}

}  // namespace nbk
