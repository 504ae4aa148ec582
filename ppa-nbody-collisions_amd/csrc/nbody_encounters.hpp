// csrc/nbody_encounters.hpp -- encounter queries on the resident state (nbody_get_encounters, nbody_batch_get_encounters,
// include/nbody.h): which pairs of bodies touch within the next h seconds if every body keeps its velocity,
// the one read-out that sets the velocities against the positions.  The launch geometry, the count and the early exits are
// those of every row query, the tile loop is rows_walk's and the host side is the pair-log driver's (nbody_rows.hpp; DESIGN.md
// 4.8a); this file has the pair, the stage of its five LDS planes, the append and the driver's traits.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A pair i < j with
// records (X, Y, R) and velocities (VX, VY) widened exactly:
//     dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
//     d2 = (dx*dx) + (dy*dy);   s = R_i + R_j;   s2 = s*s;   c = d2 - s2
//     b  = (dx*dvx) + (dy*dvy); a = (dvx*dvx) + (dvy*dvy);   disc = (b*b) - (a*c)
//     ex = dx + (dvx*h);        ey = dy + (dvy*h);            e2 = (ex*ex) + (ey*ey)
//     now = d2 <= s2;  end = e2 <= s2;  mid = b < 0 && (-b) < (a*h) && disc >= 0;  swept = now || end || mid
// symmetric bit for bit - the four differences only change sign, every product has two of them - so row i walks the sources
// j < i (the triangular walk) and reports the pair as (j, i).
//
// Division of labour.  The device does the O(n^2) part, which has subtractions, multiplies, additions and compares only: no
// divide, no square root.  Per swept pair it appends a raw record {i, j, flags, c, b, disc} to the system's capped log; the
// host does the O(hits) part in plain C (nbody_encounter_finish, nbody_encounters.c): t from c, b, disc and h with the C
// library's sqrt and /, then the sort.
//
// encounters_walk: one lane per body i.  Per pair 5 LDS reads, 27 fp64 arithmetic instructions (4 subtractions; 3 for d2, 2
// for s2, 1 for c, 3 for b, 3 for a, 3 for disc, 7 for e2, 1 for a*h) and 5 compares.  Every pair
// evaluates everything: `end` cannot be skipped where b >= 0, because e2 >= d2 holds for the exact values only, not for
// the rounded ones, and the contract is in bits.  Four pairs share one branch around the rare path.
//   * Rare path (a swept pair): one atomicAdd on the system's 64-bit `pairs` counter gives the slot; the record is stored
//     if slot < cap, otherwise only counted.  The lane adds the pair to its own now / end / missed counts.
//   * End: the three counts are summed over the wave and added to the system's counters with one atomic each per wave.
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

struct EncRaw { int32_t i, j; uint32_t flags, reserved; double c, b, disc; };      // nbody_encounter_raw
struct EncCounts { unsigned long long pairs, now, end, missed; };                  // of one system, cleared before the launch
static_assert(sizeof(EncRaw) == 40 && sizeof(nbody_encounter_raw) == 40 && offsetof(nbody_encounter_raw, c) == 16,
              "nbody_encounter_raw layout");
static_assert(sizeof(nbody_encounter) == 24, "nbody_encounter layout");
static_assert(sizeof(nbody_encounter_info) == 48, "nbody_encounter_info layout");

// The row: body i with its velocity.
struct EncRow { double x, y, r, vx, vy; };

// The four pairs of one trip of the walk: sources j .. j + 3 at entries q .. q + 3 of buffer b.  kChecked: the tile holds the
// wave's own rows, only a source below the row i counts.
struct EncFour {
    const DiagPlanes *sx, *sy, *sr, *svx, *svy;
    int i; EncRow w;                    // the row
    double h;                           // the horizon
    EncRaw* log; int cap;               // the system's
    EncCounts* cnt;
    unsigned n_now, n_end, n_missed;    // this lane's: a row has fewer than 2^31 pairs

    __device__ __forceinline__ void append(int j, unsigned flags, double c, double b, double disc) {
        const unsigned long long slot = atomicAdd(&cnt->pairs, 1ull);
        if (slot < (unsigned long long)cap) log[slot] = EncRaw{j, i, flags, 0u, c, b, disc};   // j < i: the pair as (lower, higher)
        n_now += flags & NBODY_ENCOUNTER_NOW ? 1u : 0u;
        n_end += flags & NBODY_ENCOUNTER_END ? 1u : 0u;
        n_missed += flags == 0u ? 1u : 0u;
    }

    template <bool kChecked>
    __device__ __forceinline__ void four(int bf, int q, int j) {
        bool hit[4];
        unsigned flags[4];
        double c[4], b[4], disc[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = (*sx)[bf][q + u] - w.x, dy = (*sy)[bf][q + u] - w.y;
            const double dvx = (*svx)[bf][q + u] - w.vx, dvy = (*svy)[bf][q + u] - w.vy;
            const double d2 = (dx * dx) + (dy * dy);
            const double s = w.r + (*sr)[bf][q + u];
            const double s2 = s * s;
            c[u] = d2 - s2;
            b[u] = (dx * dvx) + (dy * dvy);
            const double a = (dvx * dvx) + (dvy * dvy);
            disc[u] = (b[u] * b[u]) - (a * c[u]);
            const double ex = dx + (dvx * h), ey = dy + (dvy * h);
            const double e2 = (ex * ex) + (ey * ey);
            const bool now = d2 <= s2, end = e2 <= s2;
            const bool mid = b[u] < 0.0 && (-b[u]) < (a * h) && disc[u] >= 0.0;
            flags[u] = (now ? (unsigned)NBODY_ENCOUNTER_NOW : 0u) | (end ? (unsigned)NBODY_ENCOUNTER_END : 0u);
            hit[u] = (!kChecked || j + u < i) && (now || end || mid);
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare where the horizon is short against the crossing time
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (hit[u]) append(j + u, flags[u], c[u], b[u], disc[u]);
        }
    }
};

// grid and early exits: rows_prologue (own rows, no per-row record).  The walk is rows_walk's triangular shape (nbody_rows.hpp)
// over five planes: the stage adds the velocities to {x, y, r} and pads with x = NaN (everything else +0), so every comparison
// of such a pair fails.  V_all: the velocities, indexed like J_all.  log_all: cap records per system; cnt_all: one EncCounts
// per system.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void encounters_walk(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                              const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                              int stride, int n_one, double h, EncRaw* __restrict__ log_all, int cap,
                                                              EncCounts* __restrict__ cnt_all) {
    RowsLane<T, RowsNoOut> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, (RowsNoOut*)nullptr, RowsNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const Rec<T>* __restrict__ J = L.J;
    const Vec2<T>* __restrict__ V = V_all + (size_t)sys * (size_t)stride;
    __shared__ double sx[2][kTile], sy[2][kTile], sr[2][kTile], svx[2][kTile], svy[2][kTile];
    const RowsRow w = rows_row<T, true>(L, nullptr);
    EncRow row{w.x, w.y, w.r, 0.0, 0.0};
    if (L.valid) {
        const Vec2<T> v = V[L.p];
        row.vx = (double)v.x; row.vy = (double)v.y;
    }
    EncCounts* g = cnt_all + sys;
    EncFour f{&sx, &sy, &sr, &svx, &svy, L.p, row, h, log_all + (size_t)sys * (size_t)cap, cap, g, 0u, 0u, 0u};
    rows_walk<true, true>(L, [J, V](int b, int e, bool live, int j) {
        double x = __builtin_nan(""), y = 0.0, r = 0.0, vx = 0.0, vy = 0.0;   // padding: d2 = e2 = b = NaN
        if (live) {
            const Rec<T> s = J[j];
            const Vec2<T> v = V[j];
            x = (double)s.x; y = (double)s.y; r = (double)s.r; vx = (double)v.x; vy = (double)v.y;
        }
        sx[b][e] = x; sy[b][e] = y; sr[b][e] = r; svx[b][e] = vx; svy[b][e] = vy;
    }, f);
    // one atomic per wave and count (every lane of the workgroup is here: none has returned since the prologue)
    rows_wave_add<3>({&g->now, &g->end, &g->missed}, {f.n_now, f.n_end, f.n_missed});
}

// ---------------------------------------------------------------------------------------------------------
// Host side: the query's traits for the pair-log driver (nbody_rows.hpp), which has the buffers, the argument checks and the
// call from the reservation to the caller's list.
// ---------------------------------------------------------------------------------------------------------
struct EncQuery {
    using Raw = EncRaw;
    using Counts = EncCounts;
    using Info = nbody_encounter_info;
    using Record = nbody_encounter;
    static constexpr const char* kNoun = "encounters";
    double horizon;
    int check_value(const char* who) const {
        if (!(horizon >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: horizon = %g (seconds: >= 0, +inf allowed)", who, horizon);
        return NBODY_OK;
    }
    template <typename T, typename Count>
    void launch(dim3 grid, hipStream_t stream, const Rec<T>* J, const Vec2<T>* V, const Meta* meta, Counters* counters, int stride,
                int n_one, EncRaw* log, int cap, EncCounts* cnt) const {
        hipLaunchKernelGGL((encounters_walk<T, Count>), grid, dim3(kDiagBlock), 0, stream, J, V, meta, counters, stride, n_one, horizon,
                           log, cap, cnt);
    }
    nbody_encounter_info info(int64_t n, const EncCounts& c) const {
        return nbody_encounter_info{n, (int64_t)c.pairs, (int64_t)c.now, (int64_t)c.end, (int64_t)c.missed, horizon};
    }
    int finish(const EncRaw* raw, int pairs, nbody_encounter* out) const {
        return nbody_encounter_finish(reinterpret_cast<const nbody_encounter_raw*>(raw), pairs, horizon, out);
    }
};
using EncState = PairLogState<EncQuery>;

}  // namespace nbk
