// csrc/nbody_field.hpp -- field evaluation of the resident state (nbody_get_field, nbody_batch_get_field, include/nbody.h;
// DESIGN.md 4.8): acceleration and potential at the bodies' own positions or at arbitrary probe points, in fp64 over the
// n current bodies (fp32 states are widened exactly),
//     phi(x) = -G sum_j m_j / r_j          a(x) = -G sum_j m_j (x - x_j) / r_j^3          r_j = |x - x_j| > 0,
// a source at distance exactly 0 left out of all three sums and counted.  Included after nbody_diag.hpp by both
// translation units; one system (nbody_ctx.hip) and a batch (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride`
// apart, one set of points for every system) share the one kernel.
//
// Order contract.  ax, ay and phi of a point are each ONE running sum over j = 0, 1, ..., n-1 in
// ascending order: the bits depend on the state and the point only.  The walk is diag_walk_sums and the pair is diag_pair
// (nbody_diag.hpp), called, not restated: phi is the fma chain of diag_potential, so with the bodies' own positions
// out[i].phi has the bits nbody_get_diagnostics puts in phi[i].  Per pair, on top of the potential's d2 and diag_rinv (y):
//     y2 = y*y;  w = mj * (y2*y);  ax = fma(w, dx, ax);  ay = fma(w, dy, ay)          (5)          dx = xj - x
// so the sums are those of +m_j (x_j - x) / r_j^3 and the results are G * ax, G * ay and -G * s.
// A sum whose chain accumulator is not finite (a source at distance 0, d2 outside the chain's range, y^3 or a product out of
// range, a non-finite input) is redone by the general code, again ascending walks over j: diag_row_general for the potential
// and the count, field_acc_general over the same pairs with
//     q = (mj / d) / d;  ax = fma(q, dx / d, ax)
// (IEEE sqrt and divide, hypot outside the normal range of d2): q is m_j / r_j^2 itself, |dx / d| <= 1, so a term overflows
// only where m_j / r_j^2 does.  Each of the three sums is replaced on its own and only when it is not finite: a finite chain
// sum is never replaced (that is what keeps the phi bits the diagnostics').  The count of coincident sources comes from the
// general walk, which every point with one takes (d2 = 0 makes all three chains NaN).
// Range of the chain for the acceleration: y^3 and m_j y^3 must stay normal, d2 within [2^-680, 2^680] for masses of
// moderate size - every pair of an fp32 state, whose d2 lies within [2^-298, 2^257].  Above that range a term's weight
// underflows gradually instead of being flagged (below it, it overflows and the sum is redone).
//
// field_at: one lane per point, kDiagBlock lanes per workgroup.  kOwn: the points are the bodies themselves (read from J on
// the device), the self term is left out by index through diag_walk's checked self tile; otherwise there is no checked
// loop at all.  Workgroups past the last point leave before the first barrier; a wave past the last point only loads
// tiles.  An empty system gives +0 in every field.  The result record carries the point's coincident count; the host adds
// them up.
#pragma once
#include <float.h>
#include <stddef.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_diag.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct FieldOut { double ax, ay, phi; long long coincident; };   // device result of one point
static_assert(sizeof(FieldOut) == 32, "FieldOut layout");
static_assert(sizeof(nbody_field) == 24 && offsetof(nbody_field, ax) == 0 && offsetof(nbody_field, ay) == 8 &&
              offsetof(nbody_field, phi) == 16, "nbody_field layout");
struct FieldPoint { double x, y; };                               // nbody_vec2
static_assert(sizeof(FieldPoint) == sizeof(nbody_vec2), "nbody_vec2 layout");

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

// The general code of a flagged point's acceleration: diag_row_general's walk (the same pairs skipped, the same d), with
//     q = (mj / d) / d;  ax = fma(q, dx / d, ax).
// i < 0: a point that is no body, nothing is left out by index.
struct FieldAcc { double ax, ay; };
template <typename T>
__device__ __forceinline__ FieldAcc field_acc_general(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi) {
    double ax = 0.0, ay = 0.0;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const Rec<T> r = J[j];
        const double dx = (double)r.x - xi, dy = (double)r.y - yi;
        if (dx == 0.0 && dy == 0.0) continue;
        const double d2 = __builtin_fma(dx, dx, dy * dy);
        const double d = (d2 >= DBL_MIN && d2 <= DBL_MAX) ? __builtin_sqrt(d2) : hypot(dx, dy);
        const double q = ((double)r.m / d) / d;
        ax = __builtin_fma(q, dx / d, ax);
        ay = __builtin_fma(q, dy / d, ay);
    }
    return FieldAcc{ax, ay};
}

// Where the count comes from.  One system: the exact count is an argument (the host has just read Meta) and blockIdx.y is 0.
// A batch (FieldBatchCount, nbody_batch.hip): from the system's Meta through batch_checked_count.
struct FieldOneCount {
    static constexpr bool kBatch = false;
    static __device__ __forceinline__ int checked(const Meta*, int, int, int n_one) { return n_one; }
};

// grid = (ceil(points / kDiagBlock), systems).  Count::checked < 0: a count outside [0, stride], treated as 0 and reported
// once as kIndexError.  A batch's J and - for kOwn - out are `stride` apart per system; explicit points: out[sys * m + p].
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void field_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                       Counters* __restrict__ ctr_all, int stride, int n_one,
                                                       const FieldPoint* __restrict__ points, int m, double G,
                                                       FieldOut* __restrict__ out_all) {
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x;
    const int chk = Count::checked(meta_all, sys, stride, n_one);
    const int n = chk < 0 ? 0 : chk;
    if (chk < 0 && blockIdx.x == 0 && tid == 0) atomicAdd(&ctr_all[sys].errors, kIndexError);
    const int rows = kOwn ? n : m;
    const int row0 = blockIdx.x * kDiagBlock;                    // first point of the workgroup
    if (row0 >= rows) return;                                    // the whole workgroup, before any barrier
    const int p = row0 + tid;                                    // point of this lane
    const bool valid = p < rows;
    const Rec<T>* __restrict__ J = J_all + (size_t)sys * (size_t)stride;
    FieldOut* __restrict__ out = out_all + (size_t)sys * (size_t)(kOwn ? stride : m);
    if (n == 0) {                                                // explicit points over an empty system: +0 everywhere
        if (valid) out[p] = FieldOut{0.0, 0.0, 0.0, 0};
        return;
    }
    double xi = 0.0, yi = 0.0;
    if (valid) {
        if (kOwn) {
            const Rec<T> r = J[p];
            xi = (double)r.x; yi = (double)r.y;
        } else {
            const FieldPoint q = points[p];
            xi = q.x; yi = q.y;
        }
    }
    const int wave0 = row0 + (tid & ~(kWave - 1));               // first point of this wave
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
    FieldSums a;
    diag_walk_sums<false, kOwn, T>(J, n, kOwn ? p : -1, xi, yi, kOwn ? wave0 / kTile : -1, wave0 < rows, a, sx, sy, sm);
    if (!valid) return;
    long long coin = 0;
    if (!(__builtin_isfinite(a.s) && __builtin_isfinite(a.ax) && __builtin_isfinite(a.ay))) {
        const DiagRow g = diag_row_general<T>(J, n, kOwn ? p : -1, xi, yi);      // the potential's, and the count
        const FieldAcc ga = field_acc_general<T>(J, n, kOwn ? p : -1, xi, yi);
        coin = g.coincident;
        if (!__builtin_isfinite(a.s)) a.s = g.s;
        if (!__builtin_isfinite(a.ax)) a.ax = ga.ax;
        if (!__builtin_isfinite(a.ay)) a.ay = ga.ay;
    }
    out[p] = FieldOut{G * a.ax, G * a.ay, -G * a.s, coin};
}

// ---------------------------------------------------------------------------------------------------------
// Host side shared by the two steppers: the buffers of one context or batch, allocated on the first call and grown to the
// largest request seen - the device points, the device results, and one pinned staging area for both directions.  A
// template over the device result record: FieldOut here, NeighborOut for the neighbour queries (nbody_neighbors.hpp).
// ---------------------------------------------------------------------------------------------------------
constexpr unsigned long long kFieldMaxBytes = 1ull << 31;   // of the caller's `out`

template <typename Out>
struct PointBuffers {
    FieldPoint* pts = nullptr;      // [cap_pts]
    Out* out = nullptr;             // [cap_out]
    unsigned char* h = nullptr;     // pinned: max(cap_pts * sizeof(FieldPoint), cap_out * sizeof(Out)) bytes
    size_t cap_pts = 0, cap_out = 0, h_bytes = 0;
};
using FieldState = PointBuffers<FieldOut>;

template <typename Out>
inline void field_free(PointBuffers<Out>& f) {
    (void)hipFree(f.pts); (void)hipFree(f.out);
    if (f.h) (void)hipHostFree(f.h);
    f = PointBuffers<Out>{};
}

template <typename Out>
inline int field_reserve(PointBuffers<Out>& f, size_t n_pts, size_t n_out, const char* who) {
    hipError_t e = hipSuccess;
    if (n_pts > f.cap_pts) {
        (void)hipFree(f.pts);
        f.pts = nullptr; f.cap_pts = 0;
        e = hipMalloc((void**)&f.pts, n_pts * sizeof(FieldPoint));
        if (e == hipSuccess) f.cap_pts = n_pts; else f.pts = nullptr;
    }
    if (e == hipSuccess && n_out > f.cap_out) {
        (void)hipFree(f.out);
        f.out = nullptr; f.cap_out = 0;
        e = hipMalloc((void**)&f.out, n_out * sizeof(Out));
        if (e == hipSuccess) f.cap_out = n_out; else f.out = nullptr;
    }
    const size_t hb = f.cap_pts * sizeof(FieldPoint) > f.cap_out * sizeof(Out) ? f.cap_pts * sizeof(FieldPoint)
                                                                               : f.cap_out * sizeof(Out);
    if (e == hipSuccess && hb > f.h_bytes) {
        if (f.h) (void)hipHostFree(f.h);
        f.h = nullptr; f.h_bytes = 0;
        e = hipHostMalloc((void**)&f.h, hb, hipHostMallocDefault);
        if (e == hipSuccess) f.h_bytes = hb; else f.h = nullptr;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, point and result buffers: %s", who,
                          hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks the entry points make before any device call.  `more`: a further output that must not be NULL (the
// field's coincident count), or `out` again; `record`: the size of one of the caller's result records.
inline int field_check_args(const char* who, const void* handle, int m, const void* out, const void* n_out_or_handle,
                            const void* more, unsigned long long systems, size_t record = sizeof(nbody_field)) {
    if (!handle || !out || !n_out_or_handle || !more) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (m < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: m = %d", who, m);
    if ((unsigned long long)m * systems * record > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d points are more than 2^31 bytes of results", who, m);
    return NBODY_OK;
}

// Stages the explicit points and enqueues their copy to the device.
template <typename Out>
inline hipError_t field_stage_points(PointBuffers<Out>& f, hipStream_t stream, const nbody_vec2* points, int m) {
    memcpy(f.h, points, (size_t)m * sizeof(FieldPoint));
    return hipMemcpyAsync(f.pts, f.h, (size_t)m * sizeof(FieldPoint), hipMemcpyHostToDevice, stream);
}

// Unpacks `cnt` staged device records into the caller's 24-byte records; returns their coincident sources.
inline long long field_unpack(const FieldOut* h, size_t cnt, nbody_field* out) {
    long long coin = 0;
    for (size_t p = 0; p < cnt; ++p) {
        out[p].ax = h[p].ax; out[p].ay = h[p].ay; out[p].phi = h[p].phi;
        coin += h[p].coincident;
    }
    return coin;
}

}  // namespace nbk
