// csrc/nbody_shell_moments.hpp -- shell moments on the resident state (nbody_get_shell_moments, nbody_batch_get_shell_moments,
// include/nbody.h): for every row - a current body with its own velocity, or a probe point with a velocity of
// its own - nine fp64 running sums and a count over the sources in each bin of squared distance, 1 <= bins <=
// NBODY_SHELL_MOMENTS_MAX.  It is nbody_get_shells (nbody_shells.hpp) with the velocity terms: the launch geometry, the count
// and the early exits are those of every row query (nbody_rows.hpp), the pair, the edges and the four-pair functor (ShellFour,
// hot path and all) are the shell sums'.  This file has the terms, the accumulator with its rare path, the kernel and the
// host side.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma, no divide, no
// square root.  A row at (x, y) with velocity (vx, vy) and a source j with (X_j, Y_j, VX_j, VY_j, M_j) widened exactly:
//     dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)                         the d2 of nbody_get_shells, same bits
//     in(k, j)  <=>  e2[k] <= d2 && d2 < e2[k+1]                                   the rule of nbody_get_shells
//     ux = VX_j - vx;  uy = VY_j - vy;  w2 = (ux*ux) + (uy*uy)
//     s = (dx*ux) + (dy*uy);  c = (dx*uy) - (dy*ux)
//     mass += M_j;  px += M_j*ux;  py += M_j*uy;  ke += M_j*w2;  mr2 += M_j*d2;  rad += M_j*s;  ang += M_j*c;
//     rad2 += M_j*(s*s);  ang2 += M_j*(c*c);  count += 1                           for j ascending, where in(k, j)
// every accumulator starting at +0.0.  Own form: j != i by index.  The order of every sum is part of the contract.
//
// shell_moments_at<T, kOwn, Count, B>: shells_at's shape - one lane per row, rows_walk's full walk over {x, y} planes, 4 KiB of
// LDS - with ShellMomentSums<T, B> for ShellSums<B> as ShellFour's accumulator: nine doubles and a count per bin in registers, 18 VGPRs per bin for the
// doubles, so the tiers are B = 4 and 8 and there is none of 16 (288 VGPRs of accumulators would not fit without scratch).
//   * Hot path, per pair: shells_at's, through the same pair_d2 - 2 subtractions, 2 multiplies, 1 add and ONE compare,
//     d2 < e2[bins]; four pairs share one wave-level branch around the rare path.  No velocity is read here: the LDS planes
//     hold {x, y} only.
//   * Rare path (some lane's pair is below the top edge): the four sources in ascending j; a source that no lane of the wave
//     has hit is skipped; for the others M_j and V_j are read from the system's arrays (J, V) at the wave-uniform index
//     clamped to n - 1 - and only here - dx and dy are formed again from the LDS entry (the same operands, the same bits as
//     inside pair_d2), the nine terms are built ONCE per source, and ShellMomentSums::hit runs the fully unrolled select-add
//     over the B bins: per edge one compare, per bin in = ge[k] && !ge[k+1] and  acc[k] = acc[k] + (in ? term : +0.0)  for each
//     of the nine sums, count[k] += in.
//     The select-add is exact although seven of the terms are signed: an accumulator that started at +0.0 is never -0.0 -
//     a sum is -0.0 only where both terms are, and x + (-x) is +0.0 under round-to-nearest - so adding +0.0 returns its bits,
//     NaN included; and where the term is -0.0 and the accumulator +0.0, the definition's own addition gives +0.0 as well.  A
//     lane's accumulators see exactly the additions of the definition, in its order.
//   * A point at rest (point_vel == NULL) carries (+0.0, +0.0): V - (+0.0) is V bit for bit, -0.0 and NaN included, so the
//     one subtraction serves both forms.
//   * No register array is indexed by a runtime value; the edges are a kernel argument by value (ShellEdges<B>).
//   * The result: `bins` records of 80 bytes (nbody_shell_moment) per row, a row's records next to each other, so rows_run
//     sends them on as they stand (width() = bins).  An empty system's explicit points get zeroed records from the workgroup's
//     early exit, here.
//
// Registers, cost and the ISA comparison with shells_at: DESIGN.md 4.19.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_pairs.hpp"
#include "nbody_shells.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_shell_moment) == 80 && offsetof(nbody_shell_moment, count) == 72, "nbody_shell_moment layout");

// The nine terms of one source, built once (the head of the file has the chain).
struct ShellMomentTerms { double mass, px, py, ke, mr2, rad, ang, rad2, ang2; };

__device__ __forceinline__ ShellMomentTerms shell_moment_terms(double mj, double dx, double dy, double d2, double ux, double uy) {
    const double w2 = (ux * ux) + (uy * uy);
    const double s = (dx * ux) + (dy * uy);
    const double c = (dx * uy) - (dy * ux);
    return ShellMomentTerms{mj, mj * ux, mj * uy, mj * w2, mj * d2, mj * s, mj * c, mj * (s * s), mj * (c * c)};
}

// What a row carries along the j stream, and ShellFour's accumulator (nbody_shells.hpp): the sums, and what the rare path
// needs beyond the positions - the system's velocities V, indexed like J, and the row's own velocity.
template <typename T, int B>
struct ShellMomentSums {
    const Vec2<T>* V;
    double vx, vy;
    double mass[B], px[B], py[B], ke[B], mr2[B], rad[B], ang[B], rad2[B], ang2[B];
    int count[B];
    // Source ju at squared distance d2 below the top edge (hence no NaN), dx and dy the differences d2 was made of: M_j and
    // V_j are read here and only here, the terms are built once, and the one bin that holds d2 takes them and one count; every
    // other bin adds +0.0 and 0 (exact: see the head of the file).
    __device__ __forceinline__ void hit(const ShellEdges<B>& e, double d2, const Rec<T>* __restrict__ J, int ju, double dx, double dy) {
        const Rec<T> r = J[ju];
        const Vec2<T> v = V[ju];
        const ShellMomentTerms t = shell_moment_terms((double)r.m, dx, dy, d2, (double)v.x - vx, (double)v.y - vy);
        bool ge = e.e[0] <= d2;                                  // of edge k
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const bool next = e.e[k + 1] <= d2;                  // of edge k + 1
            const bool in = ge && !next;
            mass[k] = mass[k] + (in ? t.mass : 0.0);
            px[k] = px[k] + (in ? t.px : 0.0);
            py[k] = py[k] + (in ? t.py : 0.0);
            ke[k] = ke[k] + (in ? t.ke : 0.0);
            mr2[k] = mr2[k] + (in ? t.mr2 : 0.0);
            rad[k] = rad[k] + (in ? t.rad : 0.0);
            ang[k] = ang[k] + (in ? t.ang : 0.0);
            rad2[k] = rad2[k] + (in ? t.rad2 : 0.0);
            ang2[k] = ang2[k] + (in ? t.ang2 : 0.0);
            count[k] += in ? 1 : 0;
            ge = next;
        }
    }
};

// grid and early exits: rows_prologue; the full walk: rows_walk (nbody_rows.hpp).  V_all: the velocities, indexed like J_all.
// point_vel (explicit points): the points' velocities, or NULL for points at rest.  out_all: `bins` records per row, system
// sys's rows from sys * (kOwn ? stride : m) on, as rows_run lays out every query's records.  top = edges.e[bins].
template <typename T, bool kOwn, typename Count, int B>
__global__ __launch_bounds__(kDiagBlock) void shell_moments_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                               Counters* __restrict__ ctr_all, int stride, int n_one,
                                                               const FieldPoint* __restrict__ points, int m,
                                                               const Vec2<T>* __restrict__ V_all,
                                                               const FieldPoint* __restrict__ point_vel, int bins, double top,
                                                               const ShellEdges<B> edges, nbody_shell_moment* __restrict__ out_all) {
    RowsLane<T, RowsNoOut> L;
    const bool leave = rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, (RowsNoOut*)nullptr, RowsNoOut{});
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int p = blockIdx.x * kDiagBlock + threadIdx.x;
    nbody_shell_moment* __restrict__ out = out_all + ((size_t)sys * (size_t)(kOwn ? stride : m) + (size_t)p) * (size_t)bins;
    if (leave) {                                                 // no row in this workgroup, or an empty system: its explicit
        if (p < L.rows)                                          // points get `bins` zeroed records each (it has no own rows)
            for (int k = 0; k < bins; ++k) out[k] = nbody_shell_moment{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
        return;
    }
    const Vec2<T>* __restrict__ V = V_all + (size_t)sys * (size_t)stride;
    double vx = 0.0, vy = 0.0;                                   // a point at rest; a lane without a row
    if (L.valid) {
        if (kOwn) {
            const Vec2<T> v = V[L.p];
            vx = (double)v.x; vy = (double)v.y;
        } else if (point_vel) {
            const FieldPoint v = point_vel[L.p];
            vx = v.x; vy = v.y;
        }
    }
    __shared__ double sx[2][kTile], sy[2][kTile];
    ShellFour<T, B, ShellMomentSums<T, B>> f{&sx, &sy, L.p, rows_row<T, kOwn>(L, points), L.J, L.n - 1, top, edges, {V, vx, vy}};
#pragma unroll
    for (int k = 0; k < B; ++k) {
        f.a.mass[k] = 0.0; f.a.px[k] = 0.0; f.a.py[k] = 0.0; f.a.ke[k] = 0.0; f.a.mr2[k] = 0.0;
        f.a.rad[k] = 0.0; f.a.ang[k] = 0.0; f.a.rad2[k] = 0.0; f.a.ang2[k] = 0.0; f.a.count[k] = 0;
    }
    rows_walk<kOwn, false>(L, RowsStage<false, T>{L.J, &sx, &sy, nullptr}, f);
    if (L.valid) {
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < bins)
                out[k] = nbody_shell_moment{f.a.mass[k], f.a.px[k], f.a.py[k], f.a.ke[k], f.a.mr2[k], f.a.rad[k], f.a.ang[k],
                                            f.a.rad2[k], f.a.ang2[k], f.a.count[k], 0};
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, allocated on the first call: the points and the records (rows_run's),
// and the explicit points' velocities.
// ---------------------------------------------------------------------------------------------------------
struct ShellMomentState {
    PointBuffers<nbody_shell_moment> buf;
    RowPoints vel;
};

inline void shell_moments_free(ShellMomentState& f) { rows_free(f.buf); rows_free(f.vel); }

// The query's traits for rows_run (nbody_rows.hpp): `bins` records per row, the caller's own record.
struct ShellMomentQuery {
    using Device = nbody_shell_moment;
    using Result = nbody_shell_moment;
    const double* edges2;           // the caller's, bins + 1
    int bins;
    const void* V;                  // device Vec2<T>, indexed like the site's J
    const FieldPoint* point_vel;    // device, [m], or NULL
    template <int B, typename T, bool kOwn, typename Count, typename... Common>
    void tier(dim3 grid, hipStream_t stream, nbody_shell_moment* out, Common... common) const {
        hipLaunchKernelGGL((shell_moments_at<T, kOwn, Count, B>), grid, dim3(kDiagBlock), 0, stream, common..., (const Vec2<T>*)V,
                           point_vel, bins, edges2[bins], shell_edges<B>(edges2, bins), out);
    }
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, nbody_shell_moment* out, Common... common) const {
        if (bins <= 4) tier<4, T, kOwn, Count>(grid, stream, out, common...);          // the smaller tier that holds `bins`
        else tier<8, T, kOwn, Count>(grid, stream, out, common...);
    }
    size_t width() const { return (size_t)bins; }
    void empty(int) const {}
    void unpack(int, const nbody_shell_moment* h, size_t cnt, nbody_shell_moment* out, size_t row0) const {
        memcpy(out + row0 * (size_t)bins, h, cnt * (size_t)bins * sizeof(nbody_shell_moment));
    }
};

// The argument checks an entry point makes before any device call, the values before the handle so that each can be seen
// without one: bins; point_vel without points; m and the size of the caller's results (80 bytes per record, bins records per
// row, every system's); the edges, by pairs_check_args with its messages; then `required`, every other pointer that must not
// be NULL.
inline int shell_moments_check_args(const char* who, std::initializer_list<const void*> required, const nbody_vec2* points,
                                    const nbody_vec2* point_vel, int m, const double* edges2, int bins, unsigned long long systems) {
    static_assert(NBODY_SHELL_MOMENTS_MAX == 8, "the larger tier of ShellMomentQuery::launch");
    static_assert(NBODY_SHELL_MOMENTS_MAX <= kPairMaxBins, "pairs_check_args passes every bin count of this query");
    if (bins < 1 || bins > NBODY_SHELL_MOMENTS_MAX)
        return nbody_fail(NBODY_ERR_INVALID, "%s: bins = %d (1 .. %d)", who, bins, NBODY_SHELL_MOMENTS_MAX);
    if (point_vel && !points) return nbody_fail(NBODY_ERR_INVALID, "%s: point_vel without points", who);
    int rc = rows_check_args(who, {edges2}, m, systems * (unsigned long long)bins * sizeof(nbody_shell_moment), " of results");
    if (rc != NBODY_OK || (rc = pairs_check_args(who, {}, 0, edges2, bins)) != NBODY_OK) return rc;
    return rows_check_args(who, required, 0, 0, "");
}

// One call; the site, Count and read_meta as for rows_run.  V: the velocities, indexed like the site's J.
template <typename T, typename Count, typename ReadMeta>
int shell_moments_run(const char* who, const RowsSite& s, ShellMomentState& st, const void* V, const nbody_vec2* points,
                      const nbody_vec2* point_vel, int m, const double* edges2, int bins, nbody_shell_moment* out,
                      ReadMeta read_meta) {
    const FieldPoint* pv;
    const int rc = rows_point_vel(who, st.vel, point_vel, m, s.stream, &pv);
    if (rc != NBODY_OK) return rc;
    return rows_run<T, Count>(who, s, st.buf, ShellMomentQuery{edges2, bins, V, pv}, points, m, out, read_meta);
}

}  // namespace nbk
