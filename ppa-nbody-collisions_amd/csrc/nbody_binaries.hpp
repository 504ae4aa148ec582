// csrc/nbody_binaries.hpp -- bound-pair queries on the resident state (nbody_get_binaries, nbody_batch_get_binaries,
// include/nbody.h): which pairs of bodies within a separation are gravitationally bound to each other as a
// two-body system, the one read-out that sets masses and velocities against positions.  The launch geometry, the count and the
// early exits are those of every row query (nbody_rows.hpp: rows_prologue, rows_row); this file has the pair, its own tile walk
// (six LDS planes: rows_walk stages three and is left as it is, so no existing kernel is compiled differently), the append and
// the host side.
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
// with three more planes: only the tiles up to the one that holds the workgroup's last row are staged (a workgroup-uniform
// bound: the barriers need it); a wave computes on the tiles below its own rows unchecked, on its own tile checked and only
// up to its last row, on none above.  The ragged tile is padded with x = NaN (everything else +0): d2 is NaN and fails the one
// compare.  V_all: the velocities, indexed like J_all.  log_all: cap records per system; cnt_all: one BinCounts per system.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void binaries_walk(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                            const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                            int stride, int n_one, double sep2, BinRaw* __restrict__ log_all, int cap,
                                                            BinCounts* __restrict__ cnt_all) {
    RowsLane<T, RowsNoOut> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, (RowsNoOut*)nullptr, RowsNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x, n = L.n;
    const Rec<T>* __restrict__ J = L.J;
    const Vec2<T>* __restrict__ V = V_all + (size_t)sys * (size_t)stride;
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile], sr[2][kTile], svx[2][kTile], svy[2][kTile];
    BinRow row{__builtin_nan(""), 0.0, 0.0, 0.0, 0.0, 0.0};     // a lane without a row: every d2 it forms is NaN
    if (L.valid) {
        const Rec<T> r = J[L.p];
        const Vec2<T> v = V[L.p];
        row = BinRow{(double)r.x, (double)r.y, (double)r.m, (double)r.r, (double)v.x, (double)v.y};
    }
    BinFour f{&sx, &sy, &sm, &sr, &svx, &svy, L.p, row, sep2, 2.0 * (double)kG, log_all + (size_t)sys * (size_t)cap, cap,
              cnt_all + sys, 0u, 0u, 0u, 0u, 0u};
    const int row0 = blockIdx.x * kDiagBlock;
    const int last = (row0 + kDiagBlock < n ? row0 + kDiagBlock : n) - 1;   // the workgroup's last row
    const int jtiles = last / kTile + 1;                                    // workgroup-uniform
    const int wave_end = row0 + (tid & ~(kWave - 1)) + kWave;               // one past the wave's last row
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) {
            double x = __builtin_nan(""), y = 0.0, m = 0.0, r = 0.0, vx = 0.0, vy = 0.0;   // padding: d2 = NaN
            if (tid < jn) {
                const Rec<T> s = J[j0 + tid];
                const Vec2<T> v = V[j0 + tid];
                x = (double)s.x; y = (double)s.y; m = (double)s.m; r = (double)s.r; vx = (double)v.x; vy = (double)v.y;
            }
            sx[b][tid] = x; sy[b][tid] = y; sm[b][tid] = m; sr[b][tid] = r; svx[b][tid] = vx; svy[b][tid] = vy;
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
    unsigned long long c_near = f.n_near, c_coin = f.n_coin, c_over = f.n_over, c_appr = f.n_appr, c_bound = f.n_bound;
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
        c_near += __shfl_down(c_near, sh, kWave);
        c_coin += __shfl_down(c_coin, sh, kWave);
        c_over += __shfl_down(c_over, sh, kWave);
        c_appr += __shfl_down(c_appr, sh, kWave);
        c_bound += __shfl_down(c_bound, sh, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        BinCounts* g = cnt_all + sys;
        if (c_near) atomicAdd(&g->near, c_near);
        if (c_coin) atomicAdd(&g->coincident, c_coin);
        if (c_over) atomicAdd(&g->overlapping, c_over);
        if (c_appr) atomicAdd(&g->approaching, c_appr);
        if (c_bound) atomicAdd(&g->pairs, c_bound);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch: the counters on the first call, the log (cap records per system) and its
// pinned staging grown to the largest cap seen.
// ---------------------------------------------------------------------------------------------------------
struct BinState {
    BinCounts* cnt = nullptr;       // [systems]
    BinCounts* h_cnt = nullptr;     // pinned [systems]
    RowsArray<BinRaw> log;          // [systems * cap]: device and pinned
};

inline void binaries_free(BinState& g) {
    (void)hipFree(g.cnt);
    if (g.h_cnt) (void)hipHostFree(g.h_cnt);
    rows_free(g.log);
    g = BinState{};
}

inline int binaries_reserve(BinState& g, size_t systems, size_t cap, const char* who) {
    hipError_t e = hipSuccess;
    if (!g.h_cnt) {
        e = hipMalloc((void**)&g.cnt, systems * sizeof(BinCounts));
        if (e == hipSuccess) e = hipHostMalloc((void**)&g.h_cnt, systems * sizeof(BinCounts), hipHostMallocDefault);
        if (e != hipSuccess) g.h_cnt = nullptr;
    }
    if (e == hipSuccess) e = rows_reserve(g.log, systems * (cap > 0 ? cap : 1));     // never a NULL log
    if (e != hipSuccess) {
        (void)hipGetLastError();
        binaries_free(g);
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, counters and log: %s", who,
                          hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call.
inline int binaries_check_args(const char* who, const void* handle, double sep2, const nbody_binary* out, int cap,
                               const nbody_binary_info* info, unsigned long long systems) {
    if (!handle || !info) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (!(sep2 >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: sep2 = %g (a squared length: >= 0, +inf allowed)", who, sep2);
    if (cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    if (!out && cap > 0) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL out with cap = %d", who, cap);
    if (systems * (unsigned long long)cap * sizeof(nbody_binary) > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d binaries in each of %llu system(s) are more than 2^31 bytes", who, cap, systems);
    return NBODY_OK;
}

// One call, from the reservation to the caller's list; the site, Count and read_meta as for rows_run (nbody_rows.hpp).  V: the
// velocities, indexed like the site's J.  Two waits: the counters first - they say whether the log is complete and how much
// of it to read - then the records.
template <typename T, typename Count, typename ReadMeta>
int binaries_run(const char* who, const RowsSite& s, const void* V, BinState& g, double sep2, nbody_binary* out, int cap,
                 nbody_binary_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems;
    const bool launched = s.n_bound > 0;
    if (launched) {
        const int rc = binaries_reserve(g, S, (size_t)cap, who);
        if (rc != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemsetAsync(g.cnt, 0, S * sizeof(BinCounts), s.stream));
        hipLaunchKernelGGL((binaries_walk<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Rec<T>*)s.J,
                           (const Vec2<T>*)V, s.meta, s.counters, s.stride, s.n_one<Count>(), sep2, g.log.d, cap, g.cnt);
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(g.h_cnt, g.cnt, S * sizeof(BinCounts), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    int over = -1;
    size_t used = 0;                                             // records of the log up to the last one written
    for (int sys = 0; sys < s.systems; ++sys) {
        const int64_t n = s.count(sys);
        const BinCounts c = launched && n > 0 ? g.h_cnt[sys] : BinCounts{0, 0, 0, 0, 0};
        info[sys] = nbody_binary_info{n, (int64_t)c.pairs, (int64_t)c.near, (int64_t)c.coincident, (int64_t)c.overlapping,
                                      (int64_t)c.approaching, sep2};
        if (c.pairs > (unsigned long long)cap && over < 0) over = sys;
        if (c.pairs) used = (size_t)sys * (size_t)cap + (size_t)c.pairs;
    }
    if (!out) return NBODY_OK;                                   // cap == 0: the counts only
    if (over >= 0)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: room for %d binaries, system %d has %lld: call again with that cap", who, cap,
                          over, (long long)info[over].pairs);
    if (used == 0) return NBODY_OK;
    NBK_ROWS_TRY(hipMemcpyAsync(g.log.h, g.log.d, used * sizeof(BinRaw), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
    const nbody_binary_raw* raw = reinterpret_cast<const nbody_binary_raw*>(g.log.h);
    for (int sys = 0; sys < s.systems; ++sys) {
        const int fin = nbody_binary_finish(raw + (size_t)sys * (size_t)cap, (int)info[sys].pairs, out + (size_t)sys * (size_t)cap);
        if (fin != NBODY_OK) return fin;
    }
    return NBODY_OK;
}

}  // namespace nbk
