// csrc/nbody_diag.hpp -- physical diagnostics of the resident state (nbody_get_diagnostics, include/nbody.h): the
// per-body potential phi_i = -G sum_{j != i, r_ij > 0} m_j / r_ij and the O(N) moments, all in fp64 (fp32 inputs are
// widened exactly).  Included after nbody_kernels.hpp.  What every kernel that sums over j in ascending order and every
// finish of the totals must agree on bit for bit lives here once:
//   * diag_walk_sums, the ordered walk: the one ascending tile loop of diag_potential, batch_diag_potential, track_potential
//     (through diag_walk), field_at, tracers_advance and tides_at, the jerk's two more planes included;
//   * diag_general_walk, the exact walk of a flagged row: the one loop under diag_row_general, field_acc_general,
//     tides_general and group_row_general;
//   * diag_add / diag_finish (host and device: diag_collect in nbody_ctx.hip, batch_diag_reduce).
//
// Order contract.  phi_i is ONE running sum over j = 0, 1, ..., n-1 in ascending order, whatever the
// launch: it depends on (i, n) only, never on the rank, the world, the own count or the CU count.  The totals are
// reduced per aligned 128-body tile (nbody_partition's unit) in ascending order inside the tile, and the host then adds
// the tiles in ascending global order: a call gives the same bits for every partition of the same state.
//
// diag_potential: one lane per row i of the own range, 256-lane workgroups.  diag_walk: the j stream is wave-uniform:
// every workgroup walks the replica tile by tile; a tile's {x, y, m} are widened to fp64 ONCE, into LDS (double-buffered,
// one barrier per tile), and read back as broadcasts.  Per pair:
//     dx = xj - xi;  dy = yj - yi;  d2 = fma(dx, dx, dy*dy)                               (4)
//     y = v_rsq_f64(d2);  t = y*y;  e = fma(-d2, t, 1);  r = fma(y*e, fma(e, 3/8, 1/2), y)  (1 trans + 5)
//     acc = fma(mj, r, acc)                                                                (1)
// One third-order step takes v_rsq_f64's estimate to 1/sqrt(d2) within about 1 u (u = 2^-53): with d2 within 4 u of
// dx^2 + dy^2 of the exact differences, each term m_j / r_ij is within 3 u (3 ulps) of its exact value while d2 stays
// in [2^-1000, 2^1000] (any pair of an fp32 state).
// Self term and coincident pairs cost nothing per pair in the common case:
//   * j == i can only occur in the tile of i's own rows; a wave takes a checked loop in the tiles that hold a self term
//     of one of its lanes (self term -> m = 0, d2 = 1: adds an exact +0; the other pairs as in the unchecked loop, so
//     which loop a wave took does not show in the bits) and the unchecked loop elsewhere.  Contiguous rows: that is ONE
//     tile, known wave-uniformly.  Gathered rows (track_potential): the lanes vote per tile.
//   * d2 == 0 for j != i gives e = fma(-0, inf, 1) = NaN, and so do the degenerate d2 the fast chain cannot take
//     (t = y*y overflowing or 0): the row's accumulator is then not finite.  After the walk, exactly those rows are
//     redone with the general code (IEEE sqrt and divide, hypot outside the normal range, coincident pairs counted and
//     left out) - again one ascending walk over j, so the row's value still depends on (i, n) only.
// Each workgroup also writes, per row tile, the partial sum of m_i phi_i and the coincident count (rows ascending).
//
// diag_moments: one lane per own tile, a sequential walk over the tile's rows: mass, momentum, sum m x, angular momentum
// about the origin, sum m v^2.
#pragma once
#include <float.h>
#include <stddef.h>

#include "nbody.h"

#pragma clang fp contract(off)

namespace nbk {

struct DiagTile {             // per aligned 128-body tile of the own range (sums over its rows, ascending)
    double mass, px, py, mx, my, L, K2, pot;   // K2 = sum m v^2, pot = sum m_i phi_i
    long long coincident;                      // ordered pairs (i, j), i in the tile, j != i, at distance 0
};
static_assert(sizeof(DiagTile) == 72, "DiagTile layout");

// The finished record: struct nbody_diag (include/nbody.h) as device code writes it.
struct DiagOut {
    long long step, n_bodies, coincident_pairs;
    double mass, momentum[2], center_of_mass[2], angular_momentum, kinetic, potential;
};
static_assert(sizeof(DiagOut) == 88 && sizeof(nbody_diag) == sizeof(DiagOut), "nbody_diag layout");
static_assert(offsetof(DiagOut, step) == 0 && offsetof(DiagOut, n_bodies) == 8 && offsetof(DiagOut, coincident_pairs) == 16 &&
              offsetof(DiagOut, mass) == 24 && offsetof(DiagOut, momentum) == 32 && offsetof(DiagOut, center_of_mass) == 48 &&
              offsetof(DiagOut, angular_momentum) == 64 && offsetof(DiagOut, kinetic) == 72 &&
              offsetof(DiagOut, potential) == 80, "nbody_diag layout");
static_assert(offsetof(nbody_diag, step) == offsetof(DiagOut, step) && offsetof(nbody_diag, n_bodies) == offsetof(DiagOut, n_bodies) &&
              offsetof(nbody_diag, coincident_pairs) == offsetof(DiagOut, coincident_pairs) &&
              offsetof(nbody_diag, mass) == offsetof(DiagOut, mass) && offsetof(nbody_diag, momentum) == offsetof(DiagOut, momentum) &&
              offsetof(nbody_diag, center_of_mass) == offsetof(DiagOut, center_of_mass) &&
              offsetof(nbody_diag, angular_momentum) == offsetof(DiagOut, angular_momentum) &&
              offsetof(nbody_diag, kinetic) == offsetof(DiagOut, kinetic) &&
              offsetof(nbody_diag, potential) == offsetof(DiagOut, potential), "nbody_diag and its device mirror");

// The end of the diagnostics, the same operations on the host (one context, a group) and on the device (a batch): the
// tiles are added into a zero-initialised DiagTile in ascending global order, then the record is finished.
__host__ __device__ inline void diag_add(DiagTile& total, const DiagTile& d) {
    total.mass = total.mass + d.mass; total.px = total.px + d.px; total.py = total.py + d.py;
    total.mx = total.mx + d.mx; total.my = total.my + d.my;
    total.L = total.L + d.L; total.K2 = total.K2 + d.K2; total.pot = total.pot + d.pot;
    total.coincident += d.coincident;
}
__host__ __device__ inline DiagOut diag_finish(const DiagTile& total, long long step, long long n) {
    DiagOut o;
    o.step = step;
    o.n_bodies = n;
    o.coincident_pairs = total.coincident;
    o.mass = total.mass;
    o.momentum[0] = total.px;
    o.momentum[1] = total.py;
    o.center_of_mass[0] = total.mass == 0.0 ? __builtin_nan("") : total.mx / total.mass;   // an empty system has none
    o.center_of_mass[1] = total.mass == 0.0 ? __builtin_nan("") : total.my / total.mass;
    o.angular_momentum = total.L;
    o.kinetic = 0.5 * total.K2;
    o.potential = 0.5 * total.pot;
    return o;
}

constexpr int kDiagBlock = 256;               // four waves, two row tiles

// v_rsq_f64 is good to about 2^-25 only (one Newton step left 10 u on the MI355X): a third-order step,
// y (1 + e/2 + 3e^2/8) with e = 1 - d2 y^2, leaves O(e^3) ~ 2^-75 plus the roundings of t and of the last fma, about 1 u.
__device__ __forceinline__ double diag_rinv(double d2) {
    const double y = __builtin_amdgcn_rsq(d2);
    const double t = y * y;
    const double e = __builtin_fma(-d2, t, 1.0);
    const double p = __builtin_fma(e, 0.375, 0.5);
    return __builtin_fma(y * e, p, y);
}

// What a row carries along the j stream: the potential's running sum `s`, and for kMore whatever else is summed over
// the same pairs (FieldSums, nbody_field.hpp: the two acceleration components; TideSums, nbody_tides.hpp: the tensor's and
// the jerk's).  The per-pair expressions - dx, dy, d2, diag_rinv and the fma into s - are written here and in
// diag_walk_sums' checked loop, nowhere else: every kernel that sums over j calls the one walk.
struct DiagPhiSum {
    static constexpr bool kMore = false;
    double s = 0.0;
    __device__ __forceinline__ void more(double, double, double, double) {}
};

// One pair of the fast chain: source j at (xj, yj) with mass mj - references into the LDS tile, read where the expressions
// use them - and the row at (xi, yi).
template <typename Sums>
__device__ __forceinline__ void diag_pair(Sums& a, const double& xj, const double& yj, const double& mj, double xi, double yi) {
    const double dx = xj - xi, dy = yj - yi;
    const double d2 = __builtin_fma(dx, dx, dy * dy);
    a.s = __builtin_fma(mj, diag_rinv(d2), a.s);
    if constexpr (Sums::kMore) a.more(mj, dx, dy, diag_rinv(d2));   // the same d2, mj and diag_rinv: evaluated once
}

// The exact walk of a flagged row, the only one: j = 0 .. n-1 ascending, the self term j == i left out (i < 0: a point
// that is no body), then every j that keep(j) refuses (a membership test; DiagKeepAll: none), then every source at distance
// exactly 0, which is counted.  What remains goes to f(j, mj, dx, dy, d) with d = |(dx, dy)| by IEEE sqrt, by hypot where
// d2 leaves the normal range.  -> the count.  Every general code below and in the query headers is a functor on top of
// this: the same pairs skipped, the same d.
struct DiagKeepAll { __device__ __forceinline__ bool operator()(int) const { return true; } };
template <typename T, typename Keep, typename F>
__device__ __forceinline__ long long diag_general_walk(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi,
                                                       const Keep keep, F f) {
    long long c = 0;
    for (int j = 0; j < n; ++j) {
        if (j == i || !keep(j)) continue;
        const Rec<T> r = J[j];
        const double dx = (double)r.x - xi, dy = (double)r.y - yi;
        if (dx == 0.0 && dy == 0.0) { ++c; continue; }
        const double d2 = __builtin_fma(dx, dx, dy * dy);
        const double d = (d2 >= DBL_MIN && d2 <= DBL_MAX) ? __builtin_sqrt(d2) : hypot(dx, dy);
        f(j, (double)r.m, dx, dy, d);
    }
    return c;
}

// The general code of a flagged row's potential: s = s + mj / d over the kept pairs (group_potential keeps the members of
// the row's group, nbody_group_energy.hpp), and the count.
struct DiagRow { double s; long long coincident; };
template <typename T, typename Keep = DiagKeepAll>
__device__ __forceinline__ DiagRow diag_row_general(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi,
                                                    const Keep keep = Keep{}) {
    double s = 0.0;
    const long long c = diag_general_walk<T>(J, n, i, xi, yi, keep, [&s](int, double mj, double, double, double d) { s = s + mj / d; });
    return DiagRow{s, c};
}

// The ordered walk, the only ascending tile loop: the sum over j of row i at (xi, yi), j = 0 .. n-1 - every potential
// kernel's inner walk, field_at's, tracers_advance's and tides_at's.  Called by all kDiagBlock lanes of the workgroup (it has
// the barriers), lanes without a row included.
// self_tile: the j tile that holds the lane's self term j == i.
// kGatheredRows = false: the rows of a wave are contiguous and within one tile; self_tile is that tile, wave-uniform
//                        (lanes past the last row carry it too: they compute and are not stored).
// kGatheredRows = true : any row per lane, -1 for a lane without one; the wave votes per tile.
// kSelfTerms = false   : no row is a body (probe points): there is no checked loop at all.
// wave_works (wave-uniform): a wave without any row only loads tiles.
// sx, sy, sm: the caller's LDS planes - diag_walk's for the potential kernels, so that their LDS layout stays what it was.
// planes: what a caller stages besides {x, y, m} and looks at before each pair.  planes.stage(b, e, j): lane e fills entry e
//         of buffer b of its own planes from source j; planes.look(a, b, q): just before the pair of entry q goes into a
//         (TideVel, nbody_tides.hpp: the jerk's {vx, vy} planes, and dvx, dvy set in the sums).  DiagNoPlanes: nothing, and
//         no code.
typedef double DiagPlanes[2][kTile];          // one component of the double-buffered j tile, in LDS
struct DiagNoPlanes {
    __device__ __forceinline__ void stage(int, int, int) const {}
    template <typename Sums>
    __device__ __forceinline__ void look(Sums&, int, int) const {}
};
template <bool kGatheredRows, bool kSelfTerms, typename T, typename Sums, typename Planes = DiagNoPlanes>
__device__ __forceinline__ void diag_walk_sums(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi,
                                               int self_tile, bool wave_works, Sums& a, DiagPlanes& sx, DiagPlanes& sy,
                                               DiagPlanes& sm, const Planes planes = Planes{}) {
    const int tid = threadIdx.x;
    const int jtiles = (n + kTile - 1) / kTile;
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < jn) {
            const Rec<T> r = J[j0 + tid];
            sx[b][tid] = (double)r.x; sy[b][tid] = (double)r.y; sm[b][tid] = (double)r.m;
            planes.stage(b, tid, j0 + tid);
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!wave_works) continue;
        if (!kSelfTerms || (kGatheredRows ? !__any(self_tile == t) : t != self_tile)) {
            int q = 0;
            for (; q + 4 <= jn; q += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    planes.look(a, b, q + u);
                    diag_pair(a, sx[b][q + u], sy[b][q + u], sm[b][q + u], xi, yi);
                }
            }
            for (; q < jn; ++q) {
                planes.look(a, b, q);
                diag_pair(a, sx[b][q], sy[b][q], sm[b][q], xi, yi);
            }
        } else {
            // diag_pair with the self term masked (m = 0 at d2 = 1: an exact +0).  Written out: a function boundary around
            // the conditional LDS read changes the code of every kernel that has this loop.
            for (int q = 0; q < jn; ++q) {
                const bool self = j0 + q == i;
                const double dx = sx[b][q] - xi, dy = sy[b][q] - yi;
                const double d2 = self ? 1.0 : __builtin_fma(dx, dx, dy * dy);
                planes.look(a, b, q);
                a.s = __builtin_fma(self ? 0.0 : sm[b][q], diag_rinv(d2), a.s);
                if constexpr (Sums::kMore) a.more(self ? 0.0 : sm[b][q], dx, dy, diag_rinv(d2));
            }
        }
    }
}
template <bool kGatheredRows, typename T>
__device__ __forceinline__ double diag_walk(const Rec<T>* __restrict__ J, int n, int i, double xi, double yi,
                                            int self_tile) {
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
    DiagPhiSum a;
    diag_walk_sums<kGatheredRows, true, T>(J, n, i, xi, yi, self_tile, !kGatheredRows || __any(self_tile >= 0), a, sx, sy, sm);
    return a.s;
}

template <typename T>
__global__ __launch_bounds__(kDiagBlock) void diag_potential(const Rec<T>* __restrict__ J, int n, int lo, int cnt,
                                                             double G, double* __restrict__ phi,
                                                             DiagTile* __restrict__ tiles) {
    __shared__ double wpot[kDiagBlock];
    __shared__ long long wcoin[kDiagBlock];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kDiagBlock;                    // first own row of the workgroup
    const int k = row0 + tid;                                    // own row of this lane
    const bool valid = k < cnt;
    const int i = lo + k;
    double xi = 0.0, yi = 0.0, mi = 0.0;
    if (valid) {
        const Rec<T> r = J[i];
        xi = (double)r.x; yi = (double)r.y; mi = (double)r.m;
    }
    // global tile of this wave's rows (lo is tile-aligned): the one j tile that holds their self terms
    double acc = diag_walk<false>(J, n, i, xi, yi, (lo + row0 + (tid & ~(kWave - 1))) / kTile);
    long long coin = 0;
    if (valid && !__builtin_isfinite(acc)) {
        const DiagRow g = diag_row_general<T>(J, n, i, xi, yi);
        acc = g.s;
        coin = g.coincident;
    }
    const double p = -G * acc;
    if (valid) phi[k] = p;
    wpot[tid] = mi * p;
    wcoin[tid] = coin;
    __syncthreads();
    if ((tid & (kTile - 1)) == 0) {                             // one lane per row tile: its rows in ascending order
        const int r0 = row0 + tid;
        if (r0 < cnt) {
            const int rn = cnt - r0 < kTile ? cnt - r0 : kTile;
            double s = 0.0;
            long long c = 0;
            for (int q = 0; q < rn; ++q) { s = s + wpot[tid + q]; c += wcoin[tid + q]; }
            tiles[r0 / kTile].pot = s;
            tiles[r0 / kTile].coincident = c;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kWave) void diag_moments(const Rec<T>* __restrict__ J, const Vec2<T>* __restrict__ Vown,
                                                      int lo, int cnt, DiagTile* __restrict__ tiles) {
    const int t = blockIdx.x * kWave + threadIdx.x;
    const int r0 = t * kTile;
    if (r0 >= cnt) return;
    const int rn = cnt - r0 < kTile ? cnt - r0 : kTile;
    double mass = 0.0, px = 0.0, py = 0.0, mx = 0.0, my = 0.0, L = 0.0, K2 = 0.0;
    for (int q = 0; q < rn; ++q) {
        const Rec<T> r = J[lo + r0 + q];
        const Vec2<T> v = Vown[r0 + q];
        const double x = r.x, y = r.y, m = r.m, vx = v.x, vy = v.y;
        mass = mass + m;
        px = px + m * vx;
        py = py + m * vy;
        mx = mx + m * x;
        my = my + m * y;
        L = L + m * (x * vy - y * vx);
        K2 = K2 + m * (vx * vx + vy * vy);
    }
    DiagTile& d = tiles[t];
    d.mass = mass; d.px = px; d.py = py; d.mx = mx; d.my = my; d.L = L; d.K2 = K2;
}

}  // namespace nbk
