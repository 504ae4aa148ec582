// csrc/nbody_binaries.hpp -- bound-pair queries on the resident state (nbody_get_binaries, nbody_batch_get_binaries,
// include/nbody.h): which pairs of bodies within a separation are gravitationally bound to each other as a
// two-body system, the one read-out that sets masses and velocities against positions.  The launch geometry, the count and the
// early exits are those of every row query, the tile loop is rows_walk's and the host side is the pair-log driver's
// (nbody_rows.hpp); this file has the pair, the stage of its six LDS planes, the append and the driver's traits.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A pair i < j with
// records (X, Y, M, R) and velocities (VX, VY) widened exactly, G2 = 2 * (double)kG, sep2 the squared largest separation:
//     dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
//     d2 = (dx*dx) + (dy*dy);   coincident = d2 == 0;   near = 0 < d2 && d2 <= sep2
//     v2 = (dvx*dvx) + (dvy*dvy);   mu = G2 * (M_i + M_j);   w = (v2*v2) * d2;   k = mu * mu
//     bound = near && 0 < mu && k < +inf && w < k
//     hz = (dx*dvy) - (dy*dvx);   b = (dx*dvx) + (dy*dvy);   s = R_i + R_j
//     flags: OVERLAP where d2 <= s*s; APPROACHING where b < 0
// symmetric bit for bit - the four differences only change sign, every product has two of them - so row i walks the sources
// j < i (the triangular walk) and reports the pair as (j, i).
//
// Division of labour.  The device does the O(n^2) part, which has subtractions, multiplies, additions and compares only: no
// divide, no square root.  Per bound pair it appends a raw record {i, j, flags, d2, v2, mu, hz} to the system's capped log; the
// host does the O(bound) part in plain C (nbody_binary_finish, nbody_binaries.c): the orbit from d2, v2, mu and hz with the C
// library's sqrt and /, then the sort.
//
// binaries_walk: one lane per body i.  The hot loop is pair_counts' (nbody_pairs.hpp): per pair 2 LDS reads, 2 subtractions,
// 3 operations for d2 and ONE compare, d2 <= sep2, which a NaN fails and a coincident pair passes (sep2 >= 0).  Four pairs
// share one branch around the rest.
//   * A pair at d2 <= sep2: d2 == 0 is counted as coincident and left; otherwise it is near, and reads the four other planes:
//     2 subtractions, 3 operations for v2, 2 for mu, 2 for w, 1 for k and three compares decide `bound`.
//   * A bound pair: 3 operations for hz, 3 for b, 2 for s*s and two compares give the flags; one atomicAdd on the system's
//     64-bit `pairs` counter gives the slot; the record is stored if slot < cap, otherwise only counted.  With cap == 0 (the
//     counts only) there is no slot to ask for and the lane counts the pair itself: where most pairs are bound - sep2 = +inf
//     on a cold state - the slot atomics, all on one address, are what the kernel waits for (DESIGN.md 4.15 has the figures).
//   * End: the lane's near / coincident / overlapping / approaching (and, with cap == 0, bound) counts are summed over the
//     wave and added to the system's counters with one atomic each per wave.
// No device-side waiting, no retry loop; plain C++ stores and atomics only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct BinRaw { int32_t i, j; uint32_t flags, reserved; double d2, v2, mu, hz; };              // nbody_binary_raw
struct BinCounts { unsigned long long pairs, near, coincident, overlapping, approaching; };     // of one system, cleared before the launch
static_assert(sizeof(BinRaw) == 48 && sizeof(nbody_binary_raw) == 48 && offsetof(nbody_binary_raw, d2) == 16,
              "nbody_binary_raw layout");
static_assert(sizeof(nbody_binary) == 48 && offsetof(nbody_binary, i) == 32, "nbody_binary layout");
static_assert(sizeof(nbody_binary_info) == 56, "nbody_binary_info layout");

// The row: body i with its mass and velocity.
struct BinRow { double x, y, m, r, vx, vy; };

// The four pairs of one trip of the walk: sources j .. j + 3 at entries q .. q + 3 of buffer b.  kChecked: the tile holds the
// wave's own rows, only a source below the row i counts.
struct BinFour {
    const DiagPlanes *sx, *sy, *sm, *sr, *svx, *svy;
    int i; BinRow w;                    // the row
    double sep2, g2;                    // the squared separation; 2 G
    BinRaw* log; int cap;               // the system's
    BinCounts* cnt;
    unsigned n_near, n_coin, n_over, n_appr;   // this lane's: a row has fewer than 2^31 pairs
    unsigned n_bound;                          // cap == 0 only: the bound pairs, which no slot atomic counts then

    // a pair at d2 <= sep2: source j at entry q of buffer bf
    __device__ __forceinline__ void close_pair(int bf, int q, int j, double d2) {
        const bool coincident = d2 == 0.0;                       // no orbit: counted, never listed
        n_coin += coincident ? 1u : 0u;                          // two adds: a choice between the counters becomes a choice
        n_near += coincident ? 0u : 1u;                          // between their addresses, and the lane's counts go to scratch
        if (coincident) return;
        const double dvx = (*svx)[bf][q] - w.vx, dvy = (*svy)[bf][q] - w.vy;
        const double v2 = (dvx * dvx) + (dvy * dvy);
        const double mu = g2 * (w.m + (*sm)[bf][q]);             // M_i + M_j: the sum commutes
        const double ww = (v2 * v2) * d2;
        const double k = mu * mu;
        if (!(0.0 < mu && k < __builtin_inf() && ww < k)) return;
        const double dx = (*sx)[bf][q] - w.x, dy = (*sy)[bf][q] - w.y;   // the bits d2 was made of
        const double hz = (dx * dvy) - (dy * dvx);
        const double b = (dx * dvx) + (dy * dvy);
        const double s = w.r + (*sr)[bf][q];
        const unsigned flags = (d2 <= s * s ? (unsigned)NBODY_BINARY_OVERLAP : 0u) | (b < 0.0 ? (unsigned)NBODY_BINARY_APPROACHING : 0u);
        if (cap > 0) {                                           // uniform over the launch
            const unsigned long long slot = atomicAdd(&cnt->pairs, 1ull);
            if (slot < (unsigned long long)cap) log[slot] = BinRaw{j, i, flags, 0u, d2, v2, mu, hz};   // j < i: the pair as (lower, higher)
        } else {
            n_bound += 1u;                                       // the counts only: no slot to ask for
        }
        n_over += flags & NBODY_BINARY_OVERLAP ? 1u : 0u;
        n_appr += flags & NBODY_BINARY_APPROACHING ? 1u : 0u;
    }

    template <bool kChecked>
    __device__ __forceinline__ void four(int bf, int q, int j) {
        bool hit[4];
        double d2[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = (*sx)[bf][q + u] - w.x, dy = (*sy)[bf][q + u] - w.y;
            d2[u] = (dx * dx) + (dy * dy);
            hit[u] = (!kChecked || j + u < i) && d2[u] <= sep2;
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare where sep2 is small against the system
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (hit[u]) close_pair(bf, q + u, j + u, d2[u]);
        }
    }
};

// grid and early exits: rows_prologue (own rows, no per-row record).  The walk is rows_walk's triangular shape (nbody_rows.hpp)
// over six planes: the stage adds the masses and the velocities to {x, y, r} and pads with x = NaN (everything else +0), so d2
// is NaN and fails the one compare.  V_all: the velocities, indexed like J_all.  log_all: cap records per system; cnt_all: one
// BinCounts per system.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void binaries_walk(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                            const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                            int stride, int n_one, double sep2, BinRaw* __restrict__ log_all, int cap,
                                                            BinCounts* __restrict__ cnt_all) {
    RowsLane<T, RowsNoOut> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, (RowsNoOut*)nullptr, RowsNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const Rec<T>* __restrict__ J = L.J;
    const Vec2<T>* __restrict__ V = V_all + (size_t)sys * (size_t)stride;
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile], sr[2][kTile], svx[2][kTile], svy[2][kTile];
    BinRow row{__builtin_nan(""), 0.0, 0.0, 0.0, 0.0, 0.0};     // a lane without a row: every d2 it forms is NaN
    if (L.valid) {
        const Rec<T> r = J[L.p];
        const Vec2<T> v = V[L.p];
        row = BinRow{(double)r.x, (double)r.y, (double)r.m, (double)r.r, (double)v.x, (double)v.y};
    }
    BinCounts* g = cnt_all + sys;
    BinFour f{&sx, &sy, &sm, &sr, &svx, &svy, L.p, row, sep2, 2.0 * (double)kG, log_all + (size_t)sys * (size_t)cap, cap, g,
              0u, 0u, 0u, 0u, 0u};
    rows_walk<true, true>(L, [J, V](int b, int e, bool live, int j) {
        double x = __builtin_nan(""), y = 0.0, m = 0.0, r = 0.0, vx = 0.0, vy = 0.0;   // padding: d2 = NaN
        if (live) {
            const Rec<T> s = J[j];
            const Vec2<T> v = V[j];
            x = (double)s.x; y = (double)s.y; m = (double)s.m; r = (double)s.r; vx = (double)v.x; vy = (double)v.y;
        }
        sx[b][e] = x; sy[b][e] = y; sm[b][e] = m; sr[b][e] = r; svx[b][e] = vx; svy[b][e] = vy;
    }, f);
    // one atomic per wave and count (every lane of the workgroup is here: none has returned since the prologue)
    rows_wave_add<5>({&g->near, &g->coincident, &g->overlapping, &g->approaching, &g->pairs},
                     {f.n_near, f.n_coin, f.n_over, f.n_appr, f.n_bound});
}

// ---------------------------------------------------------------------------------------------------------
// Host side: the query's traits for the pair-log driver (nbody_rows.hpp), which has the buffers, the argument checks and the
// call from the reservation to the caller's list.
// ---------------------------------------------------------------------------------------------------------
struct BinQuery {
    using Raw = BinRaw;
    using Counts = BinCounts;
    using Info = nbody_binary_info;
    using Record = nbody_binary;
    static constexpr const char* kNoun = "binaries";
    double sep2;
    int check_value(const char* who) const {
        if (!(sep2 >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: sep2 = %g (a squared length: >= 0, +inf allowed)", who, sep2);
        return NBODY_OK;
    }
    template <typename T, typename Count>
    void launch(dim3 grid, hipStream_t stream, const Rec<T>* J, const Vec2<T>* V, const Meta* meta, Counters* counters, int stride,
                int n_one, BinRaw* log, int cap, BinCounts* cnt) const {
        hipLaunchKernelGGL((binaries_walk<T, Count>), grid, dim3(kDiagBlock), 0, stream, J, V, meta, counters, stride, n_one, sep2, log,
                           cap, cnt);
    }
    nbody_binary_info info(int64_t n, const BinCounts& c) const {
        return nbody_binary_info{n, (int64_t)c.pairs, (int64_t)c.near, (int64_t)c.coincident, (int64_t)c.overlapping,
                                 (int64_t)c.approaching, sep2};
    }
    int finish(const BinRaw* raw, int pairs, nbody_binary* out) const {
        return nbody_binary_finish(reinterpret_cast<const nbody_binary_raw*>(raw), pairs, out);
    }
};
using BinState = PairLogState<BinQuery>;

}  // namespace nbk
