// csrc/nbody_encounters.hpp -- encounter queries on the resident state (nbody_get_encounters, nbody_batch_get_encounters,
// include/nbody.h): which pairs of bodies touch within the next h seconds if every body keeps its velocity,
// the one read-out that sets the velocities against the positions.  The launch geometry, the count and the early exits are
// those of every row query (nbody_rows.hpp: rows_prologue, rows_row); this file has the pair, its own tile walk (five LDS
// planes: rows_walk stages three and is left as it is, so no existing kernel is compiled differently), the append and the
// host side.
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
// with two more planes: only the tiles up to the one that holds the workgroup's last row are staged (a workgroup-uniform
// bound: the barriers need it); a wave computes on the tiles below its own rows unchecked, on its own tile checked and only
// up to its last row, on none above.  The ragged tile is padded with x = NaN (everything else +0): every comparison of such
// a pair fails.  V_all: the velocities, indexed like J_all.  log_all: cap records per system; cnt_all: one EncCounts per system.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void encounters_walk(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                              const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                              int stride, int n_one, double h, EncRaw* __restrict__ log_all, int cap,
                                                              EncCounts* __restrict__ cnt_all) {
    RowsLane<T, RowsNoOut> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, (RowsNoOut*)nullptr, RowsNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x, n = L.n;
    const Rec<T>* __restrict__ J = L.J;
    const Vec2<T>* __restrict__ V = V_all + (size_t)sys * (size_t)stride;
    __shared__ double sx[2][kTile], sy[2][kTile], sr[2][kTile], svx[2][kTile], svy[2][kTile];
    const RowsRow w = rows_row<T, true>(L, nullptr);
    EncRow row{w.x, w.y, w.r, 0.0, 0.0};
    if (L.valid) {
        const Vec2<T> v = V[L.p];
        row.vx = (double)v.x; row.vy = (double)v.y;
    }
    EncFour f{&sx, &sy, &sr, &svx, &svy, L.p, row, h, log_all + (size_t)sys * (size_t)cap, cap, cnt_all + sys, 0u, 0u, 0u};
    const int row0 = blockIdx.x * kDiagBlock;
    const int last = (row0 + kDiagBlock < n ? row0 + kDiagBlock : n) - 1;   // the workgroup's last row
    const int jtiles = last / kTile + 1;                                    // workgroup-uniform
    const int wave_end = row0 + (tid & ~(kWave - 1)) + kWave;               // one past the wave's last row
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) {
            double x = __builtin_nan(""), y = 0.0, r = 0.0, vx = 0.0, vy = 0.0;   // padding: d2 = e2 = b = NaN
            if (tid < jn) {
                const Rec<T> s = J[j0 + tid];
                const Vec2<T> v = V[j0 + tid];
                x = (double)s.x; y = (double)s.y; r = (double)s.r; vx = (double)v.x; vy = (double)v.y;
            }
            sx[b][tid] = x; sy[b][tid] = y; sr[b][tid] = r; svx[b][tid] = vx; svy[b][tid] = vy;
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!L.wave_works || t > L.self_tile) continue;
        if (t != L.self_tile) {
            const int jn4 = (jn + 3) & ~3;                       // <= kTile: the padding is there
            for (int q = 0; q < jn4; q += 4) f.template four<false>(b, q, j0 + q);
        } else {
            const int je = wave_end - j0 < jn ? wave_end - j0 : jn;   // no row of this wave is above wave_end - 1
            const int jn4 = (je + 3) & ~3;
            for (int q = 0; q < jn4; q += 4) f.template four<true>(b, q, j0 + q);
        }
    }
    // one atomic per wave and count (every lane of the workgroup is here: none has returned since the prologue)
    unsigned long long c_now = f.n_now, c_end = f.n_end, c_missed = f.n_missed;
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
        c_now += __shfl_down(c_now, sh, kWave);
        c_end += __shfl_down(c_end, sh, kWave);
        c_missed += __shfl_down(c_missed, sh, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        EncCounts* g = cnt_all + sys;
        if (c_now) atomicAdd(&g->now, c_now);
        if (c_end) atomicAdd(&g->end, c_end);
        if (c_missed) atomicAdd(&g->missed, c_missed);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch: the counters on the first call, the log (cap records per system) and its
// pinned staging grown to the largest cap seen.
// ---------------------------------------------------------------------------------------------------------
struct EncState {
    EncCounts* cnt = nullptr;       // [systems]
    EncCounts* h_cnt = nullptr;     // pinned [systems]
    RowsArray<EncRaw> log;          // [systems * cap]: device and pinned
};

inline void encounters_free(EncState& g) {
    (void)hipFree(g.cnt);
    if (g.h_cnt) (void)hipHostFree(g.h_cnt);
    rows_free(g.log);
    g = EncState{};
}

inline int encounters_reserve(EncState& g, size_t systems, size_t cap, const char* who) {
    hipError_t e = hipSuccess;
    if (!g.h_cnt) {
        e = hipMalloc((void**)&g.cnt, systems * sizeof(EncCounts));
        if (e == hipSuccess) e = hipHostMalloc((void**)&g.h_cnt, systems * sizeof(EncCounts), hipHostMallocDefault);
        if (e != hipSuccess) g.h_cnt = nullptr;
    }
    if (e == hipSuccess) e = rows_reserve(g.log, systems * (cap > 0 ? cap : 1));     // never a NULL log
    if (e != hipSuccess) {
        (void)hipGetLastError();
        encounters_free(g);
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, counters and log: %s", who,
                          hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call.
inline int encounters_check_args(const char* who, const void* handle, double horizon, const nbody_encounter* out, int cap,
                                 const nbody_encounter_info* info, unsigned long long systems) {
    if (!handle || !info) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (!(horizon >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: horizon = %g (seconds: >= 0, +inf allowed)", who, horizon);
    if (cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    if (!out && cap > 0) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL out with cap = %d", who, cap);
    if (systems * (unsigned long long)cap * sizeof(nbody_encounter) > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d encounters in each of %llu system(s) are more than 2^31 bytes", who, cap, systems);
    return NBODY_OK;
}

// One call, from the reservation to the caller's list; the site, Count and read_meta as for rows_run (nbody_rows.hpp).  V: the
// velocities, indexed like the site's J.  Two waits: the counters first - they say whether the log is complete and how much
// of it to read - then the records.
template <typename T, typename Count, typename ReadMeta>
int encounters_run(const char* who, const RowsSite& s, const void* V, EncState& g, double horizon, nbody_encounter* out, int cap,
                   nbody_encounter_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems;
    const bool launched = s.n_bound > 0;
    if (launched) {
        const int rc = encounters_reserve(g, S, (size_t)cap, who);
        if (rc != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemsetAsync(g.cnt, 0, S * sizeof(EncCounts), s.stream));
        hipLaunchKernelGGL((encounters_walk<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Rec<T>*)s.J,
                           (const Vec2<T>*)V, s.meta, s.counters, s.stride, s.n_one<Count>(), horizon, g.log.d, cap, g.cnt);
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(g.h_cnt, g.cnt, S * sizeof(EncCounts), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    int over = -1;
    size_t used = 0;                                             // records of the log up to the last one written
    for (int sys = 0; sys < s.systems; ++sys) {
        const int64_t n = s.count(sys);
        const EncCounts c = launched && n > 0 ? g.h_cnt[sys] : EncCounts{0, 0, 0, 0};
        info[sys] = nbody_encounter_info{n, (int64_t)c.pairs, (int64_t)c.now, (int64_t)c.end, (int64_t)c.missed, horizon};
        if (c.pairs > (unsigned long long)cap && over < 0) over = sys;
        if (c.pairs) used = (size_t)sys * (size_t)cap + (size_t)c.pairs;
    }
    if (!out) return NBODY_OK;                                   // cap == 0: the counts only
    if (over >= 0)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: room for %d encounters, system %d has %lld: call again with that cap", who, cap,
                          over, (long long)info[over].pairs);
    if (used == 0) return NBODY_OK;
    NBK_ROWS_TRY(hipMemcpyAsync(g.log.h, g.log.d, used * sizeof(EncRaw), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
    const nbody_encounter_raw* raw = reinterpret_cast<const nbody_encounter_raw*>(g.log.h);
    for (int sys = 0; sys < s.systems; ++sys) {
        const int fin = nbody_encounter_finish(raw + (size_t)sys * (size_t)cap, (int)info[sys].pairs, horizon,
                                               out + (size_t)sys * (size_t)cap);
        if (fin != NBODY_OK) return fin;
    }
    return NBODY_OK;
}

}  // namespace nbk
