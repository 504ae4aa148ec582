// csrc/nbody_knn_grid.hpp -- the k nearest neighbours on the cell list (nbody_get_knn_grid, nbody_batch_get_knn_grid,
// include/nbody.h): nbody_get_knn's result for every row - a current body, or a probe point - found through
// the cell list of the cell sums (nbody_cells.hpp) instead of a walk over all n sources: about 9 k candidates per row on a
// grid whose cells hold about k bodies, O(n) for the call.  An optional cut h2_max keeps the k nearest within a radius.  One
// system (nbody_ctx.hip) and a batch (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride` apart, one grid and one
// set of points for every system) share the kernel.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  The sources are
// the bodies with inside(j) of the cell sums.  A row at (x, y), own index i (none for a point):
//     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)                 the d2 of nbody_get_knn, same bits
//     eligible(j)  <=>  inside(j) && j != i && d2_j < +inf && d2_j <= h2_max
// and the row's result is the first k eligible sources under (d2, j) ascending, then {+inf, -1}.  The first k of a set under
// a total order: the cells are walked as they lie and the result has the bits of the brute-force definition - PROVIDED a row
// stops widening only when no unseen source can come before its k-th entry.
//
// The widening rule (include/nbody.h states it, tests/knn_grid_cases.py restates it, DESIGN.md 4.23 has the proof).  Round
// t = 0, 1, ... of a row: h_t = h0 * 2^t and H2_t = fl(h0*h0) * 4^t, both +inf from t = 48; where H2_t >= h2_max the round
// takes h = fl(sqrt(h2_max)) (once, on the host) and H2 = h2_max and is final.  The window is cells_span(tx, fl(h*sx), nx) x
// cells_span(ty, fl(h*sy), ny), per axis never narrower than the round before; a cells_fine grid looks at every cell in round
// 0; a round whose spans are both the whole axis is final.  The row is done after a final round, or when its list holds k
// entries and the k-th d2 <= H2_t: section 4.21's window proof puts every inside source with d2 <= H2_t into the window, so
// every unseen one has d2 > H2_t >= d2_k and can neither enter the list nor tie with its last entry.
//
// knn_grid_walk<T, kOwn, Count, K>: one lane per row, after the four list stages (cells_list_run) and the gather of the
// sorted records (cells_gather_run) on the handle's stream; one launch for a whole batch.
//   * Rows as within_walk's: own rows inside the grid in cell order (lane = slot), n more lanes for the bodies whose cell is
//     -1, points in the order given.  Every index read from memory is range-checked before it is used as one.
//   * The list is KnnList<K> of nbody_knn.hpp in registers, tiers 4 / 8 / 16 / 32, the smallest >= k.
//   * The insertion compares (d2, j) lexicographically - knn_grid_insert: an entry moves down where d2 > v or (d2 == v and
//     index > j) - because cells do not hand j over in ascending order, as the tile walk of knn_at does.
//   * Hot path, per record: 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 <= bound, bound = min(the list's k-th d2,
//     h2_max).  The tie with the k-th entry, +inf (no entry is above it: nothing moves) and the row's own record are
//     resolved behind the branch that compare makes.  A NaN d2 passes no compare.
//   * Widening: round 0 walks the window, every later round only the frame - the cells of the new spans that the spans of
//     the round before did not hold (cells_frame_walk, nbody_cells.hpp) - so no source is seen twice and the list is never
//     cleared.  Lanes of a wave finish after different numbers of rounds; the loop runs until the wave has none left.  No
//     barrier, no LDS.
//   * info.rounds and info.widened: one max and one ballot per wave, then at most two integer atomics by its first lane -
//     the max only where it is above what the word already holds.
// Measured (profiles/knn_grid_probe.txt; one MI355X, fp32, own rows, N = 262144, the stock seeded state, knn_at in the same
// run): k = 8 on 181 x 181 cells the walk 0.100 ms and all six kernels 0.164 ms against knn_at 20.19 ms; k = 32 on 90 x 90
// the walk 1.473 ms, all kernels 1.525 ms against 39.96 ms.  Every body in one cell of 8 x 8, k = 8: the walk 43.7 ms (and
// cells_rank 5.0) against knn_at 20.3 ms: one lane per row reads all n records from memory.  Whole calls: DESIGN.md 4.23.
// Registers (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; 256-thread workgroups; fp32 and fp64
// records of a context, fp32 of a batch: 24 instantiations; own rows and points alike; VGPRs f32 / f64 records, SGPRs a
// context / a batch; "to lanes": scalar registers the compiler keeps in lanes of a vector register - the insertion's
// compare masks, two SGPRs per entry - not in memory):
//     tier K   VGPRs       SGPRs       to lanes    scratch   LDS bytes   waves per SIMD
//        4     71 / 80     91 / 95        0           0          0           7 / 6
//        8     97 / 103   105 / 106     0 / 4         0          0             4
//       16    146 / 152   106 / 106    32 / 36        0          0             3
//       32    222 / 228   106 / 106    99 / 103       0          0             2
// No instantiation uses scratch.  Every kernel that was there before keeps its text, registers and occupancy.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_cells.hpp"
#include "nbody_knn.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_knn_grid_info) == 24 && offsetof(nbody_knn_grid_info, widened) == 16, "nbody_knn_grid_info layout");

constexpr int kKnnGridRounds = 48;                               // from this round on the radius is +inf

// The call's values, once on the host: the first radius and its square, the cut and its root, and the grid's guard.
struct KnnGridWin { double h0, h02, h2_max, h_max; int fine; };

// Source j at squared distance v goes before every entry that is above it under (d2, index); the last entry drops out.
// Nothing changes where no entry is above (v, j): v = +inf meets only {+inf, -1}, whose index is below every j.  The list
// is sorted under that order, so an entry whose predecessor is above (v, j) is above it too.
template <int K>
__device__ __forceinline__ void knn_grid_insert(KnnList<K>& a, double v, int j) {
    bool above = a.d2[K - 1] > v || (a.d2[K - 1] == v && a.index[K - 1] > j);      // of entry c
#pragma unroll
    for (int c = K - 1; c > 0; --c) {
        const bool prev = a.d2[c - 1] > v || (a.d2[c - 1] == v && a.index[c - 1] > j);
        const double d = prev ? a.d2[c - 1] : v;
        const int x = prev ? a.index[c - 1] : j;
        a.d2[c] = above ? d : a.d2[c];
        a.index[c] = above ? x : a.index[c];
        above = prev;
    }
    a.d2[0] = above ? v : a.d2[0];
    a.index[0] = above ? j : a.index[0];
}

// A span that is never narrower than the one of the round before.
__device__ __forceinline__ CellSpan knn_grid_join(CellSpan now, CellSpan before) {
    if (before.lo > before.hi) return now;
    if (now.lo > now.hi) return before;
    return CellSpan{now.lo < before.lo ? now.lo : before.lo, now.hi > before.hi ? now.hi : before.hi};
}

// One lane per row; grid = (ceil(lanes / kDiagBlock), systems) with lanes = 2 * n_bound for own rows and m for points, as
// within_walk.  out_all: k entries per row, system sys's rows from sys * (kOwn ? stride : m) on.  words_all: [systems][2],
// zero at the launch - the greatest number of rounds of a row, and the rows that took more than one.
template <typename T, bool kOwn, typename Count, int K>
__global__ __launch_bounds__(kDiagBlock) void knn_grid_walk(const Rec<T>* __restrict__ J_all, const CellRec<T>* __restrict__ sorted_all,
                                                            const Meta* __restrict__ meta_all, int stride, int n_one,
                                                            const nbody_grid g, const KnnGridWin win,
                                                            const int32_t* __restrict__ cell_of_all,
                                                            const int32_t* __restrict__ start_all,
                                                            const FieldPoint* __restrict__ points, int m, int k,
                                                            KnnEntry* __restrict__ out_all, unsigned* __restrict__ words_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, g.nx * g.ny, start_all);
    const int n = cl.n, sys = cl.sys;
    const int lanes = kOwn ? 2 * n : m;
    if ((int)(blockIdx.x * kDiagBlock) >= lanes) return;         // the whole workgroup
    const CellRec<T>* __restrict__ sorted = sorted_all + cl.at;
    const int q = blockIdx.x * kDiagBlock + threadIdx.x;
    const size_t per = kOwn ? (size_t)stride : (size_t)m;        // rows of one system in out

    // the lane's row: its index in out, its own index among the sources (-1: none) and the position
    int row = -1, self = -1;
    double x = 0.0, y = 0.0;
    if (kOwn) {
        if (q < cl.inside) {
            const CellRec<T> w = sorted[q];
            if ((unsigned)w.j < (unsigned)n) { row = self = w.j; x = (double)w.x; y = (double)w.y; }
        } else if (q >= n && q < lanes) {
            const int j = q - n;
            if (cell_of_all[cl.at + j] < 0) {
                const Rec<T> b = J_all[cl.at + j];
                row = self = j; x = (double)b.x; y = (double)b.y;
            }
        }
    } else if (q < m) {
        const FieldPoint p = points[q];
        row = q; x = p.x; y = p.y;
    }

    const double inf = __builtin_inf();
    KnnList<K> a;
#pragma unroll
    for (int c = 0; c < K; ++c) { a.d2[c] = inf; a.index[c] = -1; }
    double kth = inf, bound = win.h2_max;                        // the list's k-th d2, and min(kth, h2_max)
    const auto pair = [&](const CellRec<T>& s) {
        const double dx = (double)s.x - x, dy = (double)s.y - y;
        const double d2 = (dx * dx) + (dy * dy);
        if (d2 <= bound && s.j != self) {                        // rare once the list holds k: the tie is settled here
            knn_grid_insert(a, d2, s.j);
#pragma unroll
            for (int c = 0; c < K; ++c) kth = c == k - 1 ? a.d2[c] : kth;
            bound = kth < win.h2_max ? kth : win.h2_max;
        }
    };

    const CellCoords t = cells_coords(g, x, y);
    double h = win.h0, H2 = win.h02;
    CellSpan px{0, -1}, py{0, -1};                               // the spans of the round before: none
    int rounds = 0;
    bool done = row < 0;                                         // a lane without a row waits for its wave
    while (!done) {
        if (rounds >= kKnnGridRounds) h = H2 = inf;
        double hr = h, H2r = H2;
        bool last = false;
        if (H2 >= win.h2_max) { hr = win.h_max; H2r = win.h2_max; last = true; }
        const bool every = win.fine != 0 && rounds == 0;
        const CellSpan cx = knn_grid_join(cells_span(t.tx, every ? inf : hr * g.sx, g.nx), px);
        const CellSpan cy = knn_grid_join(cells_span(t.ty, every ? inf : hr * g.sy, g.ny), py);
        last = last || (cx.lo == 0 && cx.hi == g.nx - 1 && cy.lo == 0 && cy.hi == g.ny - 1);
        cells_frame_walk(cl, sorted, g, cx, cy, px, py, pair);
        px = cx; py = cy;
        ++rounds;
        done = last || (kth < inf && kth <= H2r);
        h = h * 2.0; H2 = H2 * 4.0;                              // exact; an overflow to +inf ends the row in the next round
    }
    if (row >= 0) {
        KnnEntry* __restrict__ out = out_all + ((size_t)sys * per + (size_t)row) * (size_t)k;
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (c < k) out[c] = KnnEntry{a.d2[c], a.index[c]};
    }
    // every lane of the wave is here: the wave's greatest number of rounds, and its rows that took more than one
    int most = rounds;
#pragma unroll
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
        const int o = __shfl_xor(most, sh, kWave);
        most = o > most ? o : most;
    }
    const unsigned long long wide = __ballot(rounds > 1);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        unsigned* __restrict__ words = words_all + 2 * (size_t)sys;
        if ((unsigned)most > __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(words, (unsigned)most);
        if (wide) atomicAdd(words + 1, (unsigned)__popcll(wide));
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, next to its CellState: nothing before the first call.
// ---------------------------------------------------------------------------------------------------------
struct KnnGridState {
    RowPoints pts;
    RowsArray<KnnEntry> out;                // [systems * per * k]: device and pinned
    RowsArray<unsigned> words;              // [systems][2]: rounds, widened
};

inline void knn_grid_free(KnnGridState& w) { rows_free(w.pts); rows_free(w.out); rows_free(w.words); }

// The argument checks an entry point makes before any device call, the values before the handle; `required`: the handle,
// d2, index and info.
inline int knn_grid_check_args(const char* who, std::initializer_list<const void*> required, const nbody_grid* grid, int m, int k,
                               double h0, double h2_max, unsigned long long systems) {
    int rc = cells_check_args(who, {}, grid, 0, nullptr, nullptr, nullptr, 0, systems);
    if (rc != NBODY_OK) return rc;
    if (k < 1 || k > NBODY_KNN_MAX) return nbody_fail(NBODY_ERR_INVALID, "%s: k = %d (1 .. %d)", who, k, NBODY_KNN_MAX);
    if (!(h2_max >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: h2_max = %g (a squared radius: >= 0, +inf for none)", who, h2_max);
    if (!(h0 >= 0x1p-500 && h0 < __builtin_inf()))
        return nbody_fail(NBODY_ERR_INVALID, "%s: h0 = %g (the first radius: finite and >= 2^-500)", who, h0);
    return rows_check_args(who, required, m, systems * (unsigned long long)k * sizeof(KnnEntry), " of results");
}

// One call, from the reservation to the caller's arrays; the site, Count and read_meta as for rows_run (nbody_rows.hpp).
// points == NULL: own rows, `stride` apart per system in d2 and index; otherwise m.  One wait.
template <typename T, typename Count, typename ReadMeta>
int knn_grid_run(const char* who, const RowsSite& s, CellState& g, KnnGridState& ks, const nbody_grid& grid,
                 const nbody_vec2* points, int m, int k, double h0, double h2_max, double* d2, int32_t* index,
                 nbody_knn_grid_info* info, ReadMeta read_meta) {
    const bool own = points == nullptr;
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny, bodies = S * (size_t)s.stride;
    const size_t per = own ? (size_t)s.stride : (size_t)m, width = (size_t)k;
    const int n_one = s.n_one<Count>();
    const int lanes = own ? 2 * s.n_bound : m;
    const size_t rows_bound = own ? (size_t)s.n_bound : (size_t)m;         // rows of a system that can hold a result
    const size_t out_n = (Count::kBatch ? S * per : rows_bound) * width;
    int rc = cells_reserve(g, S, C, bodies, who, sizeof(CellRec<T>));
    if (rc != NBODY_OK) return rc;
    hipError_t e = rows_reserve(ks.pts, own || m == 0 ? 1 : (size_t)m);
    if (e == hipSuccess) e = rows_reserve(ks.out, out_n > 0 ? out_n : 1);
    if (e == hipSuccess) e = rows_reserve(ks.words, 2 * S);
    if (e != hipSuccess) {
        knn_grid_free(ks);
        return rows_alloc_failed(e, who, "row buffers");
    }
    const KnnGridWin win{h0, h0 * h0, h2_max, sqrt(h2_max), cells_fine(grid) ? 1 : 0};
    if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK || (rc = cells_gather_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
    if (!own && m > 0) NBK_ROWS_TRY(rows_upload(ks.pts, points, m, s.stream));
    NBK_ROWS_TRY(hipMemsetAsync(ks.words.d, 0, 2 * S * sizeof(unsigned), s.stream));
    if (lanes > 0) {
        const Rec<T>* J = (const Rec<T>*)s.J;
        const CellRec<T>* sorted = reinterpret_cast<const CellRec<T>*>(g.sorted.d);
        const auto walk = [&](auto own_rows, auto tier) {
            constexpr bool kOwn = decltype(own_rows)::value;
            constexpr int K = decltype(tier)::value;
            hipLaunchKernelGGL((knn_grid_walk<T, kOwn, Count, K>), s.grid(lanes), dim3(kDiagBlock), 0, s.stream, J, sorted, s.meta,
                               s.stride, n_one, grid, win, (const int32_t*)g.cell_of.d, (const int32_t*)g.start.d,
                               kOwn ? (const FieldPoint*)nullptr : (const FieldPoint*)ks.pts.d, kOwn ? 0 : m, k, ks.out.d, ks.words.d);
        };
        const auto tiers = [&](auto own_rows) {                  // the smallest tier >= k
            if (k <= 4) walk(own_rows, std::integral_constant<int, 4>{});
            else if (k <= 8) walk(own_rows, std::integral_constant<int, 8>{});
            else if (k <= 16) walk(own_rows, std::integral_constant<int, 16>{});
            else walk(own_rows, std::integral_constant<int, 32>{});
        };
        if (own) tiers(std::true_type{}); else tiers(std::false_type{});
        NBK_ROWS_TRY(hipGetLastError());
        if (out_n > 0) NBK_ROWS_TRY(hipMemcpyAsync(ks.out.h, ks.out.d, out_n * sizeof(KnnEntry), hipMemcpyDeviceToHost, s.stream));
    }
    NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipMemcpyAsync(ks.words.h, ks.words.d, 2 * S * sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    rc = s.sync<Count>(true, read_meta);
    if (rc != NBODY_OK) return rc;
    const nbody_cells_info* ci = reinterpret_cast<const nbody_cells_info*>(g.info.h);
    const unsigned* words = reinterpret_cast<const unsigned*>(ks.words.h);
    const KnnEntry* h_out = reinterpret_cast<const KnnEntry*>(ks.out.h);
    for (size_t sys = 0; sys < S; ++sys) {                       // a system's rows; the rest of its slice stays
        const size_t rows = own ? (size_t)(ci[sys].n < 0 ? 0 : ci[sys].n) : (size_t)m;
        if (rows > rows_bound) return nbody_fail(NBODY_ERR_STATE, "%s: system %zu has %zu rows, the launch covered %zu", who, sys, rows, rows_bound);
        info[sys] = nbody_knn_grid_info{ci[sys].n, (int32_t)rows, ci[sys].inside, ci[sys].outside, (int32_t)words[2 * sys + 1],
                                        (int32_t)words[2 * sys]};
        const size_t at = sys * per * width;
        for (size_t e2 = 0; e2 < rows * width; ++e2) { d2[at + e2] = h_out[at + e2].d2; index[at + e2] = h_out[at + e2].index; }
    }
    return NBODY_OK;
}

}  // namespace nbk
