// csrc/nbody_neighbors.hpp -- neighbour queries on the resident state (nbody_get_neighbors, nbody_batch_get_neighbors,
// include/nbody.h): for every row - a current body, or an arbitrary probe point - the nearest source, its
// squared distance, and the number of sources that satisfy the reference's collision predicate with the row.  The launch
// geometry, the count and the early exits are those of every row query (nbody_rows.hpp); this file has the pair, the tile
// loop and the result record.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A row at (x, y)
// with radius r (+0 for a probe point; the body's own, widened exactly, for a body) and a source j at (X_j, Y_j) with
// radius R_j (fp32 records widened exactly):
//     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)
//     nearest : best = +inf, index = -1;  for j ascending:  if (d2_j < best) { best = d2_j; index = j; }
//     overlaps: the number of j with  d2_j <= s*s,  s = r + R_j
// A NaN d2 fails both comparisons, a +inf d2 fails the first: such a source is never the nearest and a NaN one never an
// overlap.  The result is a function of the set of sources only; this kernel happens to walk j ascending with one lane per
// row, so `d2 < best` IS the tie rule (the lowest j among equal distances).
//
// neighbors_at: every workgroup walks the replica in kTile-body tiles; a tile's {x, y, r} are widened to fp64 ONCE into
// double-buffered LDS planes (6 KiB, one barrier per tile) and read back as wave-uniform broadcasts, the way
// diag_walk_sums reads {x, y, m}.
//   * The ragged last tile is padded with x = NaN (y = r = +0): a padding entry has d2 = NaN and can be neither nearest nor
//     overlap, so the pair loop carries no bound test and no remainder loop - it runs in fours up to the tile's count
//     rounded up to 4.  (Not to kTile: a 64-body system of a batch would pay 128 pairs per row for 64.)
//   * kOwn: only the wave's self tile (nbody_rows.hpp) runs the loop with the index test.
// Per pair: 2 subtractions, 2 multiplies, 1 add, 1 compare and the selects of best (2 halves) and index; for the count
// 1 add, 1 multiply, 1 compare and the add of the compare's bit.  No transcendental, no divide.
// The device record is the caller's nbody_neighbor: the host copies it out of the pinned staging as it stands.
#pragma once
#include <stddef.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct NeighborOut { double d2; int index; int overlaps; };      // struct nbody_neighbor as device code writes it
static_assert(sizeof(NeighborOut) == 16 && sizeof(nbody_neighbor) == 16, "nbody_neighbor layout");
static_assert(offsetof(nbody_neighbor, d2) == 0 && offsetof(nbody_neighbor, index) == 8 && offsetof(nbody_neighbor, overlaps) == 12 &&
              offsetof(NeighborOut, d2) == 0 && offsetof(NeighborOut, index) == 8 && offsetof(NeighborOut, overlaps) == 12,
              "nbody_neighbor and its device mirror");

// What a row carries along the j stream.
struct NeighborBest {
    double best = __builtin_inf();
    int index = -1, overlaps = 0;
};

// One pair: source j at (xj, yj) with radius rj - references into the LDS tile - and the row at (xi, yi) with radius ri.
// kChecked: the tile holds the row's self term, which takes part in neither result.
// kPoint: the row is a probe point, r = +0: s = +0 + R_j differs from R_j only where R_j is -0, and s*s not even there.
template <bool kChecked, bool kPoint>
__device__ __forceinline__ void neighbor_pair(NeighborBest& a, const double& xj, const double& yj, const double& rj, int j,
                                              int i, double xi, double yi, double ri) {
    const double dx = xj - xi, dy = yj - yi;
    const double d2 = (dx * dx) + (dy * dy);
    const double s = kPoint ? rj : ri + rj;
    const bool other = !kChecked || j != i;
    if (other && d2 < a.best) { a.best = d2; a.index = j; }
    a.overlaps += (other && d2 <= s * s) ? 1 : 0;
    // Emits nothing; keeps the counts of a trip's four pairs apart.  Each is then one v_addc_co_u32 with the compare's mask as
    // its carry; left to itself the compiler packs the four bits into a mask and counts that, in 12 instructions for 4.
    asm("" : "+v"(a.overlaps));
}

// grid and early exits: rows_prologue (nbody_rows.hpp).  An empty system gives {+inf, -1, 0}.
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void neighbors_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                           Counters* __restrict__ ctr_all, int stride, int n_one,
                                                           const FieldPoint* __restrict__ points, int m,
                                                           NeighborOut* __restrict__ out_all) {
    RowsLane<T, NeighborOut> L;
    if (rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, out_all, NeighborOut{__builtin_inf(), -1, 0}))
        return;
    const Rec<T>* __restrict__ J = L.J;
    const int n = L.n, p = L.p, tid = threadIdx.x;
    double xi = 0.0, yi = 0.0, ri = 0.0;
    if (L.valid) {
        if (kOwn) {
            const Rec<T> r = J[p];
            xi = (double)r.x; yi = (double)r.y; ri = (double)r.r;
        } else {
            const FieldPoint q = points[p];
            xi = q.x; yi = q.y;
        }
    }
    __shared__ double sx[2][kTile], sy[2][kTile], sr[2][kTile];
    NeighborBest a;
    const int jtiles = (n + kTile - 1) / kTile;
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) {
            double x = __builtin_nan(""), y = 0.0, r = 0.0;      // padding: d2 = NaN, neither nearest nor overlap
            if (tid < jn) {
                const Rec<T> s = J[j0 + tid];
                x = (double)s.x; y = (double)s.y; r = (double)s.r;
            }
            sx[b][tid] = x; sy[b][tid] = y; sr[b][tid] = r;
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!L.wave_works) continue;
        const int jn4 = (jn + 3) & ~3;                           // <= kTile: the padding is there
        if (!kOwn || t != L.self_tile) {
            for (int q = 0; q < jn4; q += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    neighbor_pair<false, !kOwn>(a, sx[b][q + u], sy[b][q + u], sr[b][q + u], j0 + q + u, p, xi, yi, ri);
            }
        } else {
            for (int q = 0; q < jn4; q += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    neighbor_pair<true, false>(a, sx[b][q + u], sy[b][q + u], sr[b][q + u], j0 + q + u, p, xi, yi, ri);
            }
        }
    }
    if (L.valid) L.out[p] = NeighborOut{a.best, a.index, a.overlaps};
}

// The query's traits for rows_run (nbody_rows.hpp): the device record is the caller's, copied as it stands.
using NeighborState = PointBuffers<NeighborOut>;

struct NeighborQuery {
    using Device = NeighborOut;
    using Result = nbody_neighbor;
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, NeighborOut* out, Common... common) const {
        hipLaunchKernelGGL((neighbors_at<T, kOwn, Count>), grid, dim3(kDiagBlock), 0, stream, common..., out);
    }
    void empty(int) const {}
    void unpack(int, const NeighborOut* h, size_t cnt, nbody_neighbor* out) const { memcpy(out, h, cnt * sizeof(NeighborOut)); }
};

}  // namespace nbk
