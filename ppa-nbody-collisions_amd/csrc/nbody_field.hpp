// csrc/nbody_field.hpp -- field evaluation of the resident state (nbody_get_field, nbody_batch_get_field, include/nbody.h;
// DESIGN.md 4.8): acceleration and potential at the bodies' own positions or at arbitrary probe points, in fp64 over the
// n current bodies (fp32 states are widened exactly),
//     phi(x) = -G sum_j m_j / r_j          a(x) = -G sum_j m_j (x - x_j) / r_j^3          r_j = |x - x_j| > 0,
// a source at distance exactly 0 left out of all three sums and counted.  The launch geometry, the count and the early
// exits are those of every row query (nbody_rows.hpp); this file has the pair, the walk's use and the result record.
//
// Order contract.  ax, ay and phi of a point are each ONE running sum over j = 0, 1, ..., n-1 in
// ascending order: the bits depend on the state and the point only.  The walk is diag_walk_sums and the pair is diag_pair
// (nbody_diag.hpp), called, not restated: phi is the fma chain of diag_potential, so with the bodies' own positions
// out[i].phi has the bits nbody_get_diagnostics puts in phi[i].  Per pair, on top of the potential's d2 and diag_rinv (y):
//     y2 = y*y;  w = mj * (y2*y);  ax = fma(w, dx, ax);  ay = fma(w, dy, ay)          (5)          dx = xj - x
// so the sums are those of +m_j (x_j - x) / r_j^3 and the results are G * ax, G * ay and -G * s.
// A sum whose chain accumulator is not finite (a source at distance 0, d2 outside the chain's range, y^3 or a product out of
// range, a non-finite input) is redone by the general code, again ascending walks over j, both of them the one exact walk
// (diag_general_walk, nbody_diag.hpp: the pairs it skips and its d are not restated here): diag_row_general for the
// potential and the count, field_acc_general with
//     q = (mj / d) / d;  ax = fma(q, dx / d, ax)
// (IEEE sqrt and divide, hypot outside the normal range of d2): q is m_j / r_j^2 itself, |dx / d| <= 1, so a term overflows
// only where m_j / r_j^2 does.  Each of the three sums is replaced on its own and only when it is not finite: a finite chain
// sum is never replaced (that is what keeps the phi bits the diagnostics').  The count of coincident sources comes from the
// general walk, which every point with one takes (d2 = 0 makes all three chains NaN).
// Range of the chain for the acceleration: y^3 and m_j y^3 must stay normal, d2 within [2^-680, 2^680] for masses of
// moderate size - every pair of an fp32 state, whose d2 lies within [2^-298, 2^257].  Above that range a term's weight
// underflows gradually instead of being flagged (below it, it overflows and the sum is redone).
//
// field_at: kOwn leaves the self term out by index through diag_walk_sums' checked self tile.  Its row is loaded here, not
// by rows_row, whose x = NaN for a lane without a row compiles to other code than this +0.  The result record carries the
// point's coincident count; the host adds them up.  What follows the walk is field_finish, which the tracers' advance
// (tracers_advance, nbody_tracers.hpp) calls after the same walk: a tracer's field has the bits of a probe point's.
#pragma once
#include <float.h>
#include <stddef.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct FieldOut { double ax, ay, phi; long long coincident; };   // device result of one point
static_assert(sizeof(FieldOut) == 32, "FieldOut layout");
static_assert(sizeof(nbody_field) == 24 && offsetof(nbody_field, ax) == 0 && offsetof(nbody_field, ay) == 8 &&
              offsetof(nbody_field, phi) == 16, "nbody_field layout");

struct FieldSums {
    static constexpr bool kMore = true;
    double s = 0.0, ax = 0.0, ay = 0.0;
    // after the walk has added mj * rinv to s: the same pair's acceleration terms
    __device__ __forceinline__ void more(double mj, double dx, double dy, double rinv) {
        const double y2 = rinv * rinv;
        const double w = mj * (y2 * rinv);
        ax = __builtin_fma(w, dx, ax);
        ay = __builtin_fma(w, dy, ay);
    }
};

// The general code of a flagged point's acceleration: the exact walk (diag_general_walk, nbody_diag.hpp) with
//     q = (mj / d) / d;  ax = fma(q, dx / d, ax).
// i < 0: a point that is no body, nothing is left out by index.
struct FieldAcc { double ax, ay; };
template <typename T>
__device__ __forceinline__ FieldAcc field_acc_general(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi) {
    double ax = 0.0, ay = 0.0;
    diag_general_walk<T>(J, n, i, xi, yi, DiagKeepAll{}, [&](int, double mj, double dx, double dy, double d) {
        const double q = (mj / d) / d;
        ax = __builtin_fma(q, dx / d, ax);
        ay = __builtin_fma(q, dy / d, ay);
    });
    return FieldAcc{ax, ay};
}

// What follows the walk for a point that has a row, field_at's and tracers_advance's (nbody_tracers.hpp): the finite tests,
// the general code for the sums that failed them, and the products with G.  n > 0.  The sums are repaired in place, through
// the reference: handed over by value, field_at's replacement compiled to other code than it had.
template <typename T>
__device__ __forceinline__ FieldOut field_finish(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi, FieldSums& a,
                                                 double G) {
    long long coin = 0;
    if (!(__builtin_isfinite(a.s) && __builtin_isfinite(a.ax) && __builtin_isfinite(a.ay))) {
        const DiagRow g = diag_row_general<T>(J, n, i, xi, yi);                  // the potential's, and the count
        const FieldAcc ga = field_acc_general<T>(J, n, i, xi, yi);
        coin = g.coincident;
        if (!__builtin_isfinite(a.s)) a.s = g.s;
        if (!__builtin_isfinite(a.ax)) a.ax = ga.ax;
        if (!__builtin_isfinite(a.ay)) a.ay = ga.ay;
    }
    return FieldOut{G * a.ax, G * a.ay, -G * a.s, coin};
}

// grid and early exits: rows_prologue (nbody_rows.hpp).  An empty system gives +0 in every field.
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void field_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                       Counters* __restrict__ ctr_all, int stride, int n_one,
                                                       const FieldPoint* __restrict__ points, int m, double G,
                                                       FieldOut* __restrict__ out_all) {
    RowsLane<T, FieldOut> L;
    if (rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, out_all, FieldOut{0.0, 0.0, 0.0, 0})) return;
    const Rec<T>* __restrict__ J = L.J;
    const int n = L.n, p = L.p;
    double xi = 0.0, yi = 0.0;                                   // not rows_row: see the head of the file
    if (L.valid) {
        if (kOwn) {
            const Rec<T> r = J[p];
            xi = (double)r.x; yi = (double)r.y;
        } else {
            const FieldPoint q = points[p];
            xi = q.x; yi = q.y;
        }
    }
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
    FieldSums a;
    diag_walk_sums<false, kOwn, T>(J, n, kOwn ? p : -1, xi, yi, L.self_tile, L.wave_works, a, sx, sy, sm);
    if (!L.valid) return;
    L.out[p] = field_finish<T>(J, n, kOwn ? p : -1, xi, yi, a, G);
}

// The query's traits for rows_run (nbody_rows.hpp): the caller gets 24-byte records and, per system, the sum of their
// coincident sources.
using FieldState = PointBuffers<FieldOut>;

struct FieldQuery {
    using Device = FieldOut;
    using Result = nbody_field;
    double G;
    int64_t* coincident;            // [systems]
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, FieldOut* out, Common... common) const {
        hipLaunchKernelGGL((field_at<T, kOwn, Count>), grid, dim3(kDiagBlock), 0, stream, common..., G, out);
    }
    size_t width() const { return 1; }
    void empty(int sys) const { coincident[sys] = 0; }
    void unpack(int sys, const FieldOut* h, size_t cnt, nbody_field* out, size_t row0) const {
        long long coin = 0;
        out += row0;
        for (size_t p = 0; p < cnt; ++p) {
            out[p].ax = h[p].ax; out[p].ay = h[p].ay; out[p].phi = h[p].phi;
            coin += h[p].coincident;
        }
        coincident[sys] = (int64_t)coin;
    }
};

}  // namespace nbk
