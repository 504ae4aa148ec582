// csrc/nbody_encounters_grid.hpp -- encounters on the cell list (nbody_get_encounters_grid, nbody_batch_get_encounters_grid,
// include/nbody.h): the swept contacts of nbody_get_encounters, restricted to the bodies inside a caller-given
// grid and found by walking the cells around every row instead of all n sources per row - O(n) on a grid matched to the reach
// of a typical body, where the triangular walk of nbody_encounters.hpp is O(n^2).  Included after nbody_within.hpp and
// nbody_encounters.hpp by both translation units: one system (nbody_ctx.hip) and a batch (nbody_batch.hip: system =
// blockIdx.y, per-body arrays `stride` apart, one grid and one horizon for every system) share the one new kernel.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  swept, the flags
// and the raw values c, b, disc are those of nbody_get_encounters, bit for bit, over the pairs i < j of bodies that are both
// inside(.) of the cell sums; the indices are those of the state.  The raw record does not depend on which end evaluates the
// pair: c, b and disc are built from d2, s and products of two differences, ex and ey change sign as a whole, R_i + R_j
// commutes - so {lower, higher, flags, c, b, disc} has the same bits from either end (nbody_encounters.hpp evaluates at the
// higher index; here the reporting row may be the lower).  Counts are integers and the list is sorted by (t, i, j) on the
// host: neither depends on the order of the visit, so the cells are walked as they lie and the results have the bits of the
// brute-force definition - PROVIDED every swept pair is evaluated by exactly one of its two ends.
//
// The window: the end with the larger REACH finds the pair (DESIGN.md 4.25 has the proof; tests/encounters_grid_cases.py
// restates the rule).  With h the horizon, per body, on the exactly widened record:
//     rho = |R| + (h * (|VX| + |VY|))                    the L1 norm: no square root
//     rho = +inf where that is NaN (a NaN velocity or radius, 0 * inf), and, in an fp64 context, where any of X, Y, VX, VY, R
//           is not finite, or non-zero with a magnitude outside [2^-100, 2^200] (there a product of the definition could
//           underflow or overflow, and the proof's relative errors would not hold)
//     H = (rho + rho) * (1 + 2^-40);   H2 = H * H
// Row i OWNS the pair (i, j) iff rho_i > rho_j, or rho_i == rho_j and i > j: a total order on [0, +inf] x index, so every
// pair has exactly one owner, and both ends compute rho by the same expression from the same values.  A pair that is swept
// as the definition computes it has d2 <= H2 of its owner: the cell of the other end lies in the owner's window
// cells_span(t, fl(H * sx), nx) x cells_span(t, fl(H * sy), ny) by the proof of the radius queries with h = H (DESIGN.md
// 4.21), per lane as groups_grid_sweep passes its S; a grid of more than 2^400 cells per unit length means every cell
// (cells_fine); H = +inf means every cell through cells_span as it stands: correct, and slow.
// The rule uses |v|, not the speed relative to the neighbours: a common bulk velocity widens every window.
//
// The kernel, on the handle's stream after the four list stages of the cell sums (cells_list_run) and the gather of the sorted
// records {x, y, r, j} (cells_gather_run):
//   encounters_grid_walk<T, Count>  one lane per slot q < inside of the cell list (lane = slot, as binaries_grid_walk).  The
//                             lane reads its own record and velocity once: rho, H, H2.  cells_window_walk over its window;
//                             the hot compare is d2 <= H2 && s.j != self && s.j >= 0 on the sorted record alone - 2
//                             subtractions, 2 multiplies, 1 add and the compare.  Behind that branch: the velocity of the
//                             source by range-checked index from V, its rho, the ownership, and for an owned pair exactly
//                             the arithmetic of EncFour::four for one pair and EncFour::append's append, the record as
//                             {lower, higher}.  cap == 0: the pairs are counted in the lane, no slot is asked for.  The
//                             lane's counts are summed over the wave by rows_wave_add.
// The rule of nbody_pairs_grid.hpp holds: the workgroup may leave as a whole before the first collective, on a
// workgroup-uniform condition; after that NO LANE RETURNS - a lane without a row is predicated off the walk and reaches the
// wave reduction.  Every index that comes out of memory (a start of a cell, the j of a record before it indexes V) is
// range-checked before it is used as one.  No device-side waiting, no retry loop, plain stores and atomics only.  No
// scratch; registers and LDS: DESIGN.md 4.25.
//
// Cost by counting: the list stages and the gather as for the radius queries; then, on a grid matched to the typical reach
// (Python: encounters_grid), 9 cells per typical row instead of n sources, 16 (32) bytes per candidate from L2, and the 27
// arithmetic instructions of the definition only for the candidates that pass the compare and are owned.
// Measured (profiles/encounters_grid_probe.txt; one MI355X, fp32, n = 130965, the stock state after 3 steps, the matched grid
// encounters_grid(field, h, median radius, median |vx| + |vy|); medians of 3 rounds of a kernel trace, encounters_walk in the
// same run): encounters_grid_walk 0.076 / 0.080 / 0.095 ms with the counts only and 0.101 / 0.133 / 0.280 ms with the list at
// h = 0 / 0.2 / 2.0, the list stages and the gather 0.39 / 0.33 / 0.12 ms, against encounters_walk's 18.4 - 18.9 ms; whole
// counts-only calls 0.26 - 0.51 ms against 18.8 - 19.0 ms.  On 1 x 1 cells the walk takes 12.96 ms (the call 14.7 against 18.4
// ms); a batch of 256 x 1024 wins in kernels (0.065 against 0.309 ms) and as a whole call.  h = +inf was not timed.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_cells.hpp"
#include "nbody_within.hpp"
#include "nbody_encounters.hpp"
#include "nbody_pairs_grid.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_encounter_grid_info) == 64 && offsetof(nbody_encounter_grid_info, horizon) == 40 &&
              offsetof(nbody_encounter_grid_info, inside) == 48 && offsetof(nbody_encounter_grid_info, outside) == 56,
              "nbody_encounter_grid_info layout: nbody_encounter_info, then inside and outside");

// A component the fp64 proof covers: zero, or a magnitude in [2^-100, 2^200]; a NaN or an infinity is none.
__device__ __forceinline__ bool enc_grid_in_range(double v) {
    const double a = fabs(v);
    return a == 0.0 || (a >= 0x1p-100 && a <= 0x1p200);
}

// The reach of a body: both ends of a pair call this with the same values, so the owner does not depend on the lane.
template <typename T>
__device__ __forceinline__ double enc_grid_reach(double x, double y, double r, double vx, double vy, double h) {
    double rho = fabs(r) + (h * (fabs(vx) + fabs(vy)));
    if (rho != rho) rho = __builtin_inf();
    if constexpr (std::is_same<T, double>::value) {
        if (!(enc_grid_in_range(x) && enc_grid_in_range(y) && enc_grid_in_range(vx) && enc_grid_in_range(vy) && enc_grid_in_range(r)))
            rho = __builtin_inf();
    }
    return rho;
}

// grid = (ceil(n_bound / kDiagBlock), systems), lane q < inside is slot q.  V_all: the velocities, indexed like the bodies.
// fine: every cell (cells_fine).  log_all: cap records per system; cnt_all: one EncCounts per system, cleared by the host.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void encounters_grid_walk(const Vec2<T>* __restrict__ V_all,
                                                                   const CellRec<T>* __restrict__ sorted_all,
                                                                   const Meta* __restrict__ meta_all, int stride, int n_one,
                                                                   const nbody_grid g, double h, int fine,
                                                                   const int32_t* __restrict__ start_all,
                                                                   EncRaw* __restrict__ log_all, int cap,
                                                                   EncCounts* __restrict__ cnt_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    if ((int)(blockIdx.x * kDiagBlock) >= cl.inside) return;     // the whole workgroup; from here on no lane returns
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const Vec2<T>* __restrict__ V = V_all + cl.at;
    const int q = blockIdx.x * kDiagBlock + threadIdx.x, n = cl.n;
    EncCounts* cnt = cnt_all + cl.sys;
    EncRaw* __restrict__ log = log_all + (size_t)cl.sys * (size_t)cap;
    unsigned n_pairs = 0u, n_now = 0u, n_end = 0u, n_missed = 0u;

    bool valid = false;
    int self = -1;
    EncRow w{0.0, 0.0, 0.0, 0.0, 0.0};
    if (q < cl.inside) {
        const CellRec<T> me = sorted[q];
        if ((unsigned)me.j < (unsigned)n) {
            valid = true; self = me.j;
            const Vec2<T> v = V[self];
            w = EncRow{(double)me.x, (double)me.y, (double)me.r, (double)v.x, (double)v.y};
        }
    }
    if (valid) {
        const double inf = __builtin_inf();
        const double rho = enc_grid_reach<T>(w.x, w.y, w.r, w.vx, w.vy, h);
        const double H = (rho + rho) * (1.0 + 0x1p-40);
        const double H2 = H * H;
        const CellCoords t = cells_coords(g, w.x, w.y);
        cells_window_walk(cl, sorted, g, t.tx, t.ty, fine ? inf : H * g.sx, fine ? inf : H * g.sy, [&](const CellRec<T>& s) {
            const double dx = (double)s.x - w.x, dy = (double)s.y - w.y;
            const double d2 = (dx * dx) + (dy * dy);
            if (d2 <= H2 && s.j != self && s.j >= 0) {           // the rest only for a candidate that passes
                if (s.j < n) {
                    const Vec2<T> sv = V[s.j];
                    const double svx = (double)sv.x, svy = (double)sv.y;
                    const double rho_j = enc_grid_reach<T>((double)s.x, (double)s.y, (double)s.r, svx, svy, h);
                    if (rho > rho_j || (rho == rho_j && self > s.j)) {       // this row owns the pair: EncFour::four's
                        const double dvx = svx - w.vx, dvy = svy - w.vy;
                        const double sum = w.r + (double)s.r;
                        const double s2 = sum * sum;
                        const double c = d2 - s2;
                        const double b = (dx * dvx) + (dy * dvy);
                        const double a = (dvx * dvx) + (dvy * dvy);
                        const double disc = (b * b) - (a * c);
                        const double ex = dx + (dvx * h), ey = dy + (dvy * h);
                        const double e2 = (ex * ex) + (ey * ey);
                        const bool now = d2 <= s2, end = e2 <= s2;
                        const bool mid = b < 0.0 && (-b) < (a * h) && disc >= 0.0;
                        if (now || end || mid) {
                            const unsigned flags = (now ? (unsigned)NBODY_ENCOUNTER_NOW : 0u) | (end ? (unsigned)NBODY_ENCOUNTER_END : 0u);
                            if (cap > 0) {                       // uniform over the launch
                                const unsigned long long slot = atomicAdd(&cnt->pairs, 1ull);
                                if (slot < (unsigned long long)cap) {
                                    const int lower = s.j < self ? s.j : self, higher = s.j < self ? self : s.j;
                                    log[slot] = EncRaw{lower, higher, flags, 0u, c, b, disc};
                                }
                            } else {
                                n_pairs += 1u;                   // the counts only: no slot to ask for
                            }
                            n_now += now ? 1u : 0u;
                            n_end += end ? 1u : 0u;
                            n_missed += flags == 0u ? 1u : 0u;
                        }
                    }
                }
            }
        });
    }
    // one atomic per wave and count: every lane of the workgroup is here, none has returned since the first line
    rows_wave_add<4>({&cnt->pairs, &cnt->now, &cnt->end, &cnt->missed}, {n_pairs, n_now, n_end, n_missed});
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  No buffers of its own: the cell list and its sorted records of CellState, the log and the counters of EncState -
// each allocated by whichever query of the handle asks first.
// ---------------------------------------------------------------------------------------------------------

// The argument checks before any device call, the values before the handle: the grid as the cell sums check it, then what
// nbody_get_encounters checks.
inline int encounters_grid_check_args(const char* who, const void* handle, const nbody_grid* grid, double horizon,
                                      const nbody_encounter* out, int cap, const nbody_encounter_grid_info* info,
                                      unsigned long long systems) {
    const int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    if (rc != NBODY_OK) return rc;
    return pair_log_check_args(who, handle, EncQuery{horizon}, out, cap, reinterpret_cast<const nbody_encounter_info*>(info), systems);
}

// The sibling of binaries_grid_run (nbody_pairs_grid.hpp): the list stages and the gather before the launch, the cell list's
// info with the counters; everything after the first wait is the pair-log driver's tail with an info writer that adds inside
// and outside.  The plain encounters keep their launch, waits and bytes.
template <typename T, typename Count, typename ReadMeta>
int encounters_grid_run(const char* who, const RowsSite& s, const void* V, CellState& g, EncState& es, const nbody_grid& grid,
                        double horizon, nbody_encounter* out, int cap, nbody_encounter_grid_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny;
    const bool launched = s.n_bound > 0;
    const EncQuery q{horizon};
    if (launched) {
        int rc = cells_reserve(g, S, C, S * (size_t)s.stride, who, sizeof(CellRec<T>));
        if (rc != NBODY_OK || (rc = pair_log_reserve(es, S, (size_t)cap, who)) != NBODY_OK) return rc;
        if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemsetAsync(es.cnt.d, 0, S * sizeof(EncCounts), s.stream));
        hipLaunchKernelGGL((encounters_grid_walk<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Vec2<T>*)V,
                           reinterpret_cast<const CellRec<T>*>(g.sorted.d), s.meta, s.stride, s.n_one<Count>(), grid, horizon,
                           cells_fine(grid) ? 1 : 0, (const int32_t*)g.start.d, es.log.d, cap, es.cnt.d);
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(es.cnt.h, es.cnt.d, S * sizeof(EncCounts), hipMemcpyDeviceToHost, s.stream));
        NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    return pair_log_tail(who, s, es, q, launched, out, cap, [&](int sys, int64_t n, const EncCounts& c) {
        const int64_t in = launched ? pairs_grid_inside(g, sys, n) : 0;
        const nbody_encounter_info ei = q.info(n, c);
        info[sys] = nbody_encounter_grid_info{ei.n_bodies, ei.pairs, ei.now, ei.end, ei.missed, ei.horizon, in, n - in};
    });
}

}  // namespace nbk
