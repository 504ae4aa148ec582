// csrc/nbody_shells.hpp -- shell sums on the resident state (nbody_get_shells, nbody_batch_get_shells, include/nbody.h;
// DESIGN.md 4.18): for every row - a current body, or an arbitrary probe point - the mass and the number of the sources in
// each bin of squared distance, 1 <= bins <= NBODY_SHELLS_MAX.  The launch geometry, the count and the early exits are those
// of every row query (nbody_rows.hpp); this file has the pair, the accumulators, the result entry and the traits for rows_run.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A row at (x, y)
// and a source j with the record (X_j, Y_j, M_j) widened exactly:
//     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)                       the d2 of nbody_get_neighbors, same bits
//     in(k, j)  <=>  e2[k] <= d2_j && d2_j < e2[k+1]                               the rule of nbody_get_pair_counts
//     count[row][k] = the number of sources with in(k, j)
//     mass [row][k] = acc after:  acc = +0.0;  for j ascending:  if in(k, j)  acc = acc + M_j
// Own form: j != i by index.  The order of the mass sum is part of the contract.
//
// shells_at<T, kOwn, Count, B>: one lane per row, rows_walk's full shape over {x, y} planes (4 KiB of LDS, no radius plane),
// for the own form as well: a row needs every j != i, not the triangle.  Along one lane that walk visits j in ascending order.
//   * The accumulators are ShellSums<B>: B masses and B counts in registers.  B is the tier, a compile-time capacity of 4, 8,
//     16 or 32 bins; the host takes the smallest tier >= bins and gives the surplus bins +inf edges, which no source below the
//     top edge reaches.  No register array is ever indexed by a runtime value; bins only decides how many entries are stored
//     at the end (a wave-uniform test per entry).
//   * The edges are a kernel argument by value (ShellEdges<B>, B + 1 doubles): wave-uniform, read where the rare path needs
//     them.  No device buffer, no copy, no LDS for them.
//   * Hot path, per pair: pair_counts': 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 < e2[bins].  Four pairs share
//     one wave-level branch around the rare path.  Padding entries and lanes without a row carry x = NaN (nbody_rows.hpp): d2 =
//     NaN passes no compare; so does d2 = +inf under a +inf top edge.  kOwn: only the wave's self tile applies j != i.
//   * Rare path (some lane's pair is below the top edge): the four sources in ascending j; per source M_j is read from the
//     replica (the index is wave-uniform and clamped to n - 1, so a padding entry reads a body, which no lane adds), then
//     for the lanes that hit it - a source that no lane of the wave has hit is skipped - ShellSums::hit, fully unrolled: per edge
//     one compare ge[k] = e2[k] <= d2, per bin in = ge[k] && !ge[k+1] (for a d2 that is no NaN - it is below the top edge -
//     !(e <= d2) is d2 < e) and one select-add,  mass[k] += in ? M_j : +0.0;  count[k] += in.
//     The select-add is exact: an accumulator that started at +0.0 is never -0.0 (a sum is -0.0 only where both terms are),
//     so adding +0.0 to it returns its bits, NaN included.  A lane's accumulator therefore sees exactly the additions of the
//     definition, in its order.
//   * The result: B entries of 12 bytes {mass, count} per row, a row's entries next to each other ([row][k], the caller's
//     order), so rows_run sends them on as they stand.  An empty system's explicit points get their {+0.0, 0} entries from the
//     workgroup's early exit, here, not from rows_prologue: a row has `bins` records, not one.
//
// Cost by counting: the hot path is pair_counts' points kernel, instruction for instruction (in the four-pair loop: 4
// ds_read2_b64, 20 fp64 operations, 4 compares, 4 adds of the compare's bit).  A rare trip runs, for each of its four sources
// that some lane has hit - on sparse edges one of them - B + 1 compares and per bin a mask operation, the select of M_j's two
// halves, one fp64 add and one add-with-carry: about 6 B instructions and one read of M_j, against about 40 for a hot trip.
// At most 256 times the share of the pairs below the top edge is the share of the trips that take it (64 lanes, 4 pairs).
// Measured (profiles/shells_probe.txt; one MI355X, fp32, n = 130965, medians of 3 rounds of a kernel trace, spreads <= 0.1 ms):
// on 65536 points against pair_counts' points kernel on the same points and 32 edges, 5.200 against 5.203 ms where 6.8e-6 of the
// pairs are in range and 5.767 against 5.363 ms (1.075) where 4.9e-5 are - at most 1.25 % of the trips, each about 5 hot trips'
// worth of instructions: at most +6.3 % by the count, the rest is the read's latency, which was not measured apart.  Own rows:
// 5.76 / 5.90 ms for 8 / 32 bins on the sparser edges, 6.27 / 6.94 ms on the other: 1.11 to 1.25 times the TRIANGULAR
// pair_counts call (5.20 / 5.54 ms), not twice - the full walk is even over the workgroups, the triangle is not; neighbors_at
// 9.53 ms in the same run.  One bin [0, +inf), every pair added: 26.45 ms.  Batch 256 x 1024, 8 bins: 0.133 ms.
//
// Registers (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; 256-thread workgroups; fp32 and fp64
// records, a context and a batch: 24 instantiations, the SGPRs as ranges over them):
//     tier B   VGPRs own / points   SGPRs own / points   scratch   LDS bytes   waves per SIMD
//        4          50 / 46           61-62 / 58-60         0        4096            8
//        8          62 / 62           69-70 / 66-68         0        4096            8
//       16          94 / 94           85-86 / 82-84         0        4096            5
//       32         158 / 158            106 / 106           0        4096            3
// No instantiation uses scratch.  The B + 1 edges live in 2 B + 2 scalar registers; at the 32-bin tier that is 66 of them and
// the compiler keeps 8 to 12 scalars in lanes of a vector register instead (v_writelane / v_readlane, no memory).  The
// accumulators of that tier are 96 vector registers, as knn_at's 32-entry list: the same VGPRs and occupancy tier for tier.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_pairs.hpp"

#pragma clang fp contract(off)

namespace nbk {

// One bin of a row as device code writes it and the pinned staging holds it.
struct __attribute__((packed, aligned(4))) ShellEntry { double mass; int32_t count; };
static_assert(sizeof(ShellEntry) == 12, "an entry is the caller's 8 + 4 bytes");

// The squared edges of a tier, a kernel argument: e[0 .. bins] the caller's, +inf from there on.
template <int B>
struct ShellEdges { double e[B + 1]; };

// The squared edges of a tier as the host fills them: the caller's bins + 1, +inf from there on.
template <int B>
inline ShellEdges<B> shell_edges(const double* edges2, int bins) {
    ShellEdges<B> e;
    for (int k = 0; k <= B; ++k) e.e[k] = k <= bins ? edges2[k] : __builtin_inf();
    return e;
}

// What a row carries along the j stream, and ShellFour's accumulator: hit() is the rare path's one source.
template <int B>
struct ShellSums {
    double mass[B];
    int count[B];
    // Source ju at squared distance d2 below the top edge (hence no NaN): the one bin that holds d2 takes M_j and one count,
    // every other bin adds +0.0 and 0.
    template <typename T>
    __device__ __forceinline__ void hit(const ShellEdges<B>& e, double d2, const Rec<T>* __restrict__ J, int ju, double, double) {
        const double mj = (double)J[ju].m;
        bool ge = e.e[0] <= d2;                                  // of edge k
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const bool next = e.e[k + 1] <= d2;                  // of edge k + 1
            const bool in = ge && !next;
            mass[k] = mass[k] + (in ? mj : 0.0);
            count[k] += in ? 1 : 0;
            ge = next;
        }
    }
};

// The four pairs of one trip of rows_walk, for shells_at and shell_moments_at (nbody_shell_moments.hpp): sources j .. j + 3 at
// entries q .. q + 3 of buffer b.  kChecked: the tile holds the wave's own rows, the self term j == i is no source.  Acc: the
// sums of the query, called as a.hit(e, d2, J, ju, dx, dy) for a source that the lane has hit - dx and dy from the LDS
// operands d2 was made of, the same bits as inside pair_d2; an accumulator that does not use them costs nothing.
template <typename T, int B, typename Acc>
struct ShellFour {
    const DiagPlanes *sx, *sy;
    int i; RowsRow w;               // the row
    const Rec<T>* J; int last;      // the system's sources and n - 1: where the rare path reads source j
    double top;                     // e2[bins]
    ShellEdges<B> e;
    Acc a;
    template <bool kChecked>
    __device__ __forceinline__ void four(int b, int q, int j) {
        bool hit[4];
        double d2[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            d2[u] = pair_d2((*sx)[b][q + u], (*sy)[b][q + u], w.x, w.y);
            hit[u] = (!kChecked || j + u != i) && d2[u] < top;
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare where the top edge is small against the system
#pragma unroll
            for (int u = 0; u < 4; ++u) {                        // in j order
                const int ju = j + u < last ? j + u : last;      // a padding entry: no lane has hit it
                if (hit[u])                                      // skipped where no lane of the wave has hit source u
                    a.hit(e, d2[u], J, ju, (*sx)[b][q + u] - w.x, (*sy)[b][q + u] - w.y);
            }
        }
    }
};

// grid and early exits: rows_prologue; the full walk: rows_walk (nbody_rows.hpp).  out_all: `bins` entries per row, system
// sys's rows from sys * (kOwn ? stride : m) on, as rows_run lays out every query's records.  top = edges.e[bins].
template <typename T, bool kOwn, typename Count, int B>
__global__ __launch_bounds__(kDiagBlock) void shells_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                        Counters* __restrict__ ctr_all, int stride, int n_one,
                                                        const FieldPoint* __restrict__ points, int m, int bins, double top,
                                                        const ShellEdges<B> edges, ShellEntry* __restrict__ out_all) {
    RowsLane<T, RowsNoOut> L;
    const bool leave = rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, (RowsNoOut*)nullptr, RowsNoOut{});
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int p = blockIdx.x * kDiagBlock + threadIdx.x;
    ShellEntry* __restrict__ out = out_all + ((size_t)sys * (size_t)(kOwn ? stride : m) + (size_t)p) * (size_t)bins;
    if (leave) {                                                 // no row in this workgroup, or an empty system: its explicit
        if (p < L.rows)                                          // points get `bins` empty entries each (it has no own rows)
            for (int k = 0; k < bins; ++k) out[k] = ShellEntry{0.0, 0};
        return;
    }
    __shared__ double sx[2][kTile], sy[2][kTile];
    ShellFour<T, B, ShellSums<B>> f{&sx, &sy, L.p, rows_row<T, kOwn>(L, points), L.J, L.n - 1, top, edges, {}};
#pragma unroll
    for (int k = 0; k < B; ++k) { f.a.mass[k] = 0.0; f.a.count[k] = 0; }
    rows_walk<kOwn, false>(L, RowsStage<false, T>{L.J, &sx, &sy, nullptr}, f);
    if (L.valid) {
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (k < bins) out[k] = ShellEntry{f.a.mass[k], f.a.count[k]};
    }
}

// The query's traits for rows_run (nbody_rows.hpp): `bins` entries per row, taken apart into the caller's two arrays.
using ShellState = PointBuffers<ShellEntry>;

struct ShellResult { double* mass; int32_t* count; };            // the caller's, [rows * bins] each

struct ShellQuery {
    using Device = ShellEntry;
    using Result = ShellResult;
    const double* edges2;           // the caller's, bins + 1
    int bins;
    template <int B, typename T, bool kOwn, typename Count, typename... Common>
    void tier(dim3 grid, hipStream_t stream, ShellEntry* out, Common... common) const {
        hipLaunchKernelGGL((shells_at<T, kOwn, Count, B>), grid, dim3(kDiagBlock), 0, stream, common..., bins, edges2[bins],
                           shell_edges<B>(edges2, bins), out);
    }
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, ShellEntry* out, Common... common) const {
        if (bins <= 4) tier<4, T, kOwn, Count>(grid, stream, out, common...);          // the smallest tier >= bins
        else if (bins <= 8) tier<8, T, kOwn, Count>(grid, stream, out, common...);
        else if (bins <= 16) tier<16, T, kOwn, Count>(grid, stream, out, common...);
        else tier<32, T, kOwn, Count>(grid, stream, out, common...);
    }
    size_t width() const { return (size_t)bins; }
    void empty(int) const {}
    void unpack(int, const ShellEntry* h, size_t cnt, ShellResult* out, size_t row0) const {
        double* mass = out->mass + row0 * (size_t)bins;
        int32_t* count = out->count + row0 * (size_t)bins;
        for (size_t e = 0; e < cnt * (size_t)bins; ++e) { mass[e] = h[e].mass; count[e] = h[e].count; }
    }
};

// The argument checks an entry point makes before any device call, the values before the handle so that each can be seen
// without one: bins; m and the size of the caller's results (12 bytes per entry, bins entries per row, every system's); the
// edges, by pairs_check_args with its messages; then `required`, every other pointer that must not be NULL.
inline int shells_check_args(const char* who, std::initializer_list<const void*> required, int m, const double* edges2, int bins,
                             unsigned long long systems) {
    static_assert(NBODY_SHELLS_MAX == 32, "the largest tier of ShellQuery::launch");
    static_assert(NBODY_SHELLS_MAX <= kPairMaxBins, "pairs_check_args passes every bin count of this query");
    if (bins < 1 || bins > NBODY_SHELLS_MAX) return nbody_fail(NBODY_ERR_INVALID, "%s: bins = %d (1 .. %d)", who, bins, NBODY_SHELLS_MAX);
    int rc = rows_check_args(who, {edges2}, m, systems * (unsigned long long)bins * sizeof(ShellEntry), " of results");
    if (rc != NBODY_OK || (rc = pairs_check_args(who, {}, 0, edges2, bins)) != NBODY_OK) return rc;
    return rows_check_args(who, required, 0, 0, "");
}

}  // namespace nbk
