// csrc/nbody_tides.hpp -- field derivatives of the resident state (nbody_get_tides, nbody_batch_get_tides, include/nbody.h;
// DESIGN.md 4.17): the tidal tensor T = da/dx and the jerk da/dt along the motion, at the bodies' own positions or at
// arbitrary probe points, in fp64 over the n current bodies (fp32 states are widened exactly).  With d = x_j - x, r = |d| > 0
// and dv = v_j - v,
//     T_ab(x)    = G sum_j m_j (3 d_a d_b / r^5 - delta_ab / r^3)                    -> txx, txy, tyy
//     adot_a(x,v) = G sum_j m_j (dv_a / r^3 - 3 (d . dv) d_a / r^5)                   -> jx, jy
// a source at distance exactly 0 left out of every sum and counted.  The force law is the 3-D one in a plane: txx + tyy =
// G sum m_j / r_j^3, not 0.  The launch geometry, the count and the early exits are those of every row query (nbody_rows.hpp:
// rows_prologue, rows_row); this file has the pair, the jerk's planes for the ordered walk, the general code and the host side.
//
// Order contract.  Six running sums per row, each over j = 0, 1, ..., n-1 in ascending order:
//     sw = sum w          sxx, sxy, syy = sum 3 w u_a u_b          jx, jy = sum (w dv_a - 3 w (u . dv) u_a)
// and the results are G (sxx - sw), G sxy, G (syy - sw), G jx, G jy: the bits depend on the state, the point and (jerk) its
// velocity only - not on rank, world, transport, m, the point's place in `points`, or whether the launch also sums the jerk.
//
// Per-pair chain, written once: TideSums::more.  It continues the field's pair - dx, dy, d2 and y = diag_rinv(d2) are
// diag_pair's (nbody_diag.hpp), called, not restated:
//     y2 = y*y;  w = mj * (y2*y);  w3 = 3*w;  ux = dx*y;  uy = dy*y;  px = w3*ux;  py = w3*uy                 (8)
//     sw = sw + w;  sxx = fma(px, ux, sxx);  sxy = fma(px, uy, sxy);  syy = fma(py, uy, syy)                  (4)
// and for the jerk, with dvx = vxj - vx, dvy = vyj - vy                                                        (2)
//     ru = fma(ux, dvx, uy*dvy);  k = w3*ru                                                                   (3)
//     jx = fma(w, dvx, jx);  jx = fma(-k, ux, jx);  jy = fma(w, dvy, jy);  jy = fma(-k, uy, jy)               (4)
// This is NOT the association m y^5 d_a d_b: the factors r^-2 are taken into the unit vector u = d y, so the narrowest
// intermediate is w = m_j y^3, the field's own.  Range of the chain: y^3 and m_j y^3 must stay normal - d2 within
// [2^-680, 2^680] for masses of moderate size.  Every pair of an fp32 state lies inside it: d2 within [2^-298, 2^257] gives y^3
// within [2^-386, 2^447]; a mass within [2^-149, 2^57] (1e17 < 2^57) puts w and w3 within [2^-535, 2^506]; |u| <= 1 + 4 u, and
// |dv| <= 2^129 keeps w dv and k below 2^637.  Below the range y^3 or w overflows and the sums are flagged; above it the
// weight underflows gradually instead (the term is then below 2^-1000 of any unit, as for the field).  The suggested m y^5
// association would leave [2^-408, 2^408] and, unlike this one, lose a term silently at 2^600.
//
// Flagged sums (the policy of nbody_field.hpp).  A sum whose chain accumulator is not finite - a source at distance 0, d2
// outside the range, an overflowing product, a non-finite input - is redone by the general code, tides_general: one more
// ascending walk over j, the exact walk of every flagged row (diag_general_walk, nbody_diag.hpp: IEEE sqrt and divide, hypot
// outside the normal range of d2), with
//     q = ((mj / d) / d) / d;  q3 = 3*q;  ux = dx / d;  uy = dy / d
// in place of w, w3 and u in the very same sums: q is m_j / r_j^3 itself and |u| <= 1, so a term overflows only where
// m_j / r_j^3 does.  Each of the six sums is replaced on its own and only when it is not finite; a finite chain sum is never
// replaced.  The count of coincident sources comes from diag_row_general, which every point with one takes (d2 = 0 makes
// every chain NaN).
//
// The walk.  Both launches ride diag_walk_sums (nbody_diag.hpp) with TideSums as the kMore object, as field_at
// does with FieldSums: the checked self tile comes with it, and the potential's fma into `s`, which nothing reads, is dead
// code.  kJerk = true needs {vx, vy} of the j tile in LDS - five double-buffered planes, 10 KiB: it hands the walk TideVel, which
// stages the two planes more and sets dv in the sums before each pair.  One loop adds the pairs through the one
// TideSums::more, in one order: the tensor of a kJerk = true launch has the bits of a kJerk = false launch.  rows_walk is the
// NaN-padded family's.  Plain C++ loads and stores only, no device-side waiting.
#pragma once
#include <float.h>
#include <stddef.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct TideOut { double txx, txy, tyy, jx, jy; long long coincident; };   // device result of one row
static_assert(sizeof(TideOut) == 48, "TideOut layout");
static_assert(sizeof(nbody_tide) == 24 && offsetof(nbody_tide, txx) == 0 && offsetof(nbody_tide, txy) == 8 &&
              offsetof(nbody_tide, tyy) == 16, "nbody_tide layout");

// The running sums of one row and the pair's chain (the head of the file has it).  `s` is what diag_pair adds the
// potential's term to: never read here.  dvx, dvy (kJerk): v_j - v of the pair about to be added, set by TideVel::look.
template <bool kJerk>
struct TideSums {
    static constexpr bool kMore = true;
    double s = 0.0;
    double sw = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, jx = 0.0, jy = 0.0;
    double dvx = 0.0, dvy = 0.0;
    // w: the weight m_j / r^3 (chain: mj * y^3; general code: ((mj / d) / d) / d); ux, uy: the unit vector d / r.
    __device__ __forceinline__ void add(double w, double ux, double uy) {
        const double w3 = 3.0 * w;
        const double px = w3 * ux, py = w3 * uy;
        sw = sw + w;
        sxx = __builtin_fma(px, ux, sxx);
        sxy = __builtin_fma(px, uy, sxy);
        syy = __builtin_fma(py, uy, syy);
        if constexpr (kJerk) {
            const double ru = __builtin_fma(ux, dvx, uy * dvy);
            const double k = w3 * ru;
            jx = __builtin_fma(w, dvx, jx);
            jx = __builtin_fma(-k, ux, jx);
            jy = __builtin_fma(w, dvy, jy);
            jy = __builtin_fma(-k, uy, jy);
        }
    }
    // after the walk's pair (diag_pair) has formed dx, dy and rinv = diag_rinv(d2)
    __device__ __forceinline__ void more(double mj, double dx, double dy, double rinv) {
        const double y2 = rinv * rinv;
        add(mj * (y2 * rinv), dx * rinv, dy * rinv);
    }
    __device__ __forceinline__ bool finite() const {
        bool ok = __builtin_isfinite(sw) && __builtin_isfinite(sxx) && __builtin_isfinite(sxy) && __builtin_isfinite(syy);
        if constexpr (kJerk) ok = ok && __builtin_isfinite(jx) && __builtin_isfinite(jy);
        return ok;
    }
};

// What the jerk adds to the ordered walk (diag_walk_sums' `planes`): {vx, vy} of the j tile in two more LDS planes, and
// dv = v_j - v of the row's velocity (vxi, vyi) put into the sums before each pair.  V: the velocities, indexed like J.
template <typename T>
struct TideVel {
    const Vec2<T>* __restrict__ V;
    double vxi, vyi;
    DiagPlanes *svx, *svy;
    __device__ __forceinline__ void stage(int b, int e, int j) const {
        const Vec2<T> v = V[j];
        (*svx)[b][e] = (double)v.x; (*svy)[b][e] = (double)v.y;
    }
    __device__ __forceinline__ void look(TideSums<true>& a, int b, int q) const {
        a.dvx = (*svx)[b][q] - vxi; a.dvy = (*svy)[b][q] - vyi;
    }
};

// The general code of a flagged row: the exact walk (diag_general_walk, nbody_diag.hpp) into the same sums.
// i < 0: a point that is no body, nothing is left out by index.  V is read only for kJerk.
template <typename T, bool kJerk>
__device__ __forceinline__ TideSums<kJerk> tides_general(const Rec<T>* __restrict__ J, const Vec2<T>* __restrict__ V, int n, int i,
                                                        double xi, double yi, double vxi, double vyi) {
    TideSums<kJerk> g;
    diag_general_walk<T>(J, n, i, xi, yi, DiagKeepAll{}, [&](int j,double mj, double dx, double dy, double d) {
        if constexpr (kJerk) {
            const Vec2<T> v = V[j];
            g.dvx = (double)v.x - vxi; g.dvy = (double)v.y - vyi;
        }
        g.add(((mj / d) / d) / d, dx / d, dy / d);
    });
    return g;
}

// grid and early exits: rows_prologue (nbody_rows.hpp).  An empty system gives +0 in every field.  V_all (kJerk): the
// velocities, indexed like J_all.  point_vel (kJerk, explicit points): the points' velocities, or NULL for points at rest.
template <typename T, bool kOwn, bool kJerk, typename Count>
__global__ __launch_bounds__(kDiagBlock) void tides_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                       Counters* __restrict__ ctr_all, int stride, int n_one,
                                                       const FieldPoint* __restrict__ points, int m,
                                                       const Vec2<T>* __restrict__ V_all, const FieldPoint* __restrict__ point_vel,
                                                       double G, TideOut* __restrict__ out_all) {
    RowsLane<T, TideOut> L;
    if (rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, out_all, TideOut{0.0, 0.0, 0.0, 0.0, 0.0, 0})) return;
    const Rec<T>* __restrict__ J = L.J;
    const int n = L.n, p = L.p, i = kOwn ? L.p : -1;
    const RowsRow w = rows_row<T, kOwn>(L, points);
    const Vec2<T>* __restrict__ V = nullptr;
    double vxi = 0.0, vyi = 0.0;
    TideSums<kJerk> a;
    if constexpr (kJerk) {
        V = V_all + (size_t)(Count::kBatch ? (int)blockIdx.y : 0) * (size_t)stride;
        if (L.valid) {
            if (kOwn) {
                const Vec2<T> v = V[p];
                vxi = (double)v.x; vyi = (double)v.y;
            } else if (point_vel) {
                const FieldPoint v = point_vel[p];
                vxi = v.x; vyi = v.y;
            }
        }
        __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile], svx[2][kTile], svy[2][kTile];
        diag_walk_sums<false, kOwn, T>(J, n, i, w.x, w.y, L.self_tile, L.wave_works, a, sx, sy, sm, TideVel<T>{V, vxi, vyi, &svx, &svy});
    } else {
        __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
        diag_walk_sums<false, kOwn, T>(J, n, i, w.x, w.y, L.self_tile, L.wave_works, a, sx, sy, sm);
    }
    if (!L.valid) return;
    long long coin = 0;
    if (!a.finite()) {
        coin = diag_row_general<T>(J, n, i, w.x, w.y).coincident;
        const TideSums<kJerk> g = tides_general<T, kJerk>(J, V, n, i, w.x, w.y, vxi, vyi);
        if (!__builtin_isfinite(a.sw)) a.sw = g.sw;
        if (!__builtin_isfinite(a.sxx)) a.sxx = g.sxx;
        if (!__builtin_isfinite(a.sxy)) a.sxy = g.sxy;
        if (!__builtin_isfinite(a.syy)) a.syy = g.syy;
        if constexpr (kJerk) {
            if (!__builtin_isfinite(a.jx)) a.jx = g.jx;
            if (!__builtin_isfinite(a.jy)) a.jy = g.jy;
        }
    }
    L.out[p] = TideOut{G * (a.sxx - a.sw), G * a.sxy, G * (a.syy - a.sw), G * a.jx, G * a.jy, coin};
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, allocated on the first call: the points and the results (rows_run's),
// and the explicit points' velocities.
// ---------------------------------------------------------------------------------------------------------
struct TidesState {
    PointBuffers<TideOut> buf;
    RowPoints vel;
};

inline void tides_free(TidesState& f) { rows_free(f.buf); rows_free(f.vel); }

struct TideResult { nbody_tide* tide; nbody_vec2* jerk; };       // the caller's; jerk may be NULL

// The query's traits for rows_run (nbody_rows.hpp): the caller gets 24-byte tensors, 16-byte jerks where asked and, per
// system, the sum of the rows' coincident sources.
struct TidesQuery {
    using Device = TideOut;
    using Result = TideResult;
    double G;
    const void* V;                  // device Vec2<T>, indexed like the site's J; read only with `jerk`
    const FieldPoint* point_vel;    // device, [m], or NULL
    bool jerk;
    int64_t* coincident;            // [systems]
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, TideOut* out, Common... common) const {
        if (jerk)
            hipLaunchKernelGGL((tides_at<T, kOwn, true, Count>), grid, dim3(kDiagBlock), 0, stream, common..., (const Vec2<T>*)V,
                               point_vel, G, out);
        else
            hipLaunchKernelGGL((tides_at<T, kOwn, false, Count>), grid, dim3(kDiagBlock), 0, stream, common...,
                               (const Vec2<T>*)nullptr, (const FieldPoint*)nullptr, G, out);
    }
    size_t width() const { return 1; }
    void empty(int sys) const { coincident[sys] = 0; }
    void unpack(int sys, const TideOut* h, size_t cnt, TideResult* out, size_t row0) const {
        long long coin = 0;
        nbody_tide* tide = out->tide + row0;
        for (size_t p = 0; p < cnt; ++p) {
            tide[p].txx = h[p].txx; tide[p].txy = h[p].txy; tide[p].tyy = h[p].tyy;
            coin += h[p].coincident;
        }
        if (jerk) {
            nbody_vec2* j = out->jerk + row0;
            for (size_t p = 0; p < cnt; ++p) { j[p].X = h[p].jx; j[p].Y = h[p].jy; }
        }
        coincident[sys] = (int64_t)coin;
    }
};

// The argument checks an entry point makes before any device call.  `required`: the handle and the result pointers that
// must not be NULL; `systems`: whose results a point has.  The values are looked at before the pointers, so that each message
// names what is wrong with the call whatever else is.
inline int tides_check_args(const char* who, std::initializer_list<const void*> required, const nbody_vec2* points,
                            const nbody_vec2* point_vel, const nbody_vec2* jerk, int m, unsigned long long systems) {
    if (point_vel && !points) return nbody_fail(NBODY_ERR_INVALID, "%s: point_vel without points", who);
    if (point_vel && !jerk) return nbody_fail(NBODY_ERR_INVALID, "%s: point_vel without jerk", who);
    int rc = rows_check_args(who, {}, m, systems * sizeof(nbody_tide), " of results");
    if (rc == NBODY_OK) rc = rows_check_args(who, required, 0, 0, "");
    return rc;
}

// One call; the site, Count and read_meta as for rows_run.  V: the velocities, indexed like the site's J (read only when
// jerk != NULL).
template <typename T, typename Count, typename ReadMeta>
int tides_run(const char* who, const RowsSite& s, TidesState& st, double G, const void* V, const nbody_vec2* points,
              const nbody_vec2* point_vel, int m, nbody_tide* tide, nbody_vec2* jerk, int64_t* coincident, ReadMeta read_meta) {
    const FieldPoint* pv;
    const int rc = rows_point_vel(who, st.vel, point_vel, m, s.stream, &pv);
    if (rc != NBODY_OK) return rc;
    TideResult out{tide, jerk};
    return rows_run<T, Count>(who, s, st.buf, TidesQuery{G, V, pv, jerk != nullptr, coincident}, points, m, &out, read_meta);
}

}  // namespace nbk
