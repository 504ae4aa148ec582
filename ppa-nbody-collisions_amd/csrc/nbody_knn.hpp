// csrc/nbody_knn.hpp -- k-nearest-neighbour queries on the resident state (nbody_get_knn, nbody_batch_get_knn,
// include/nbody.h): for every row - a current body, or an arbitrary probe point - the k nearest sources and
// their squared distances, 1 <= k <= NBODY_KNN_MAX.  The launch geometry, the count and the early exits are those of every
// row query (nbody_rows.hpp); this file has the pair, the sorted list, the result entry and the traits for rows_run.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A row at (x, y)
// and a source j with the record (X_j, Y_j) widened exactly:
//     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)                       the d2 of nbody_get_neighbors, same bits
// A source is eligible iff d2_j < +inf (own form: and j != i, by index).  The row's result is the first k eligible sources
// under the total order (d2, j) ascending, then {+inf, -1} up to k.  A function of the set of sources only.
//
// knn_at<T, kOwn, Count, K>: one lane per row, rows_walk's full shape over {x, y} planes (4 KiB of LDS, no radius plane).
//   * The list is KnnList<K>: K squared distances and K indices in registers, sorted, +inf / -1 where empty.  K is the tier,
//     a compile-time capacity of 4, 8, 16 or 32; the host takes the smallest tier >= k.  A lane keeps the K nearest whatever k
//     is - the first k of the K nearest are the k nearest - so no register array is ever indexed by a runtime value; k only
//     decides how many entries are stored at the end (a wave-uniform test per entry).
//   * Hot path, per pair: 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 < worst, worst being the list's last entry
//     (+inf until K sources have been listed, which also keeps a +inf or NaN d2 out).  Four pairs share one branch around the
//     rare path, as in pair_counts: it is taken when some lane of the wave passed a compare.
//   * Rare path: knn_insert, a fully unrolled compare-and-shift - per entry one compare with the new d2 and the selects of the
//     entry's two d2 halves and index between itself, its predecessor and the new pair.  The new pair goes behind every entry
//     whose d2 is <= its own; j ascends along the walk, so that IS the (d2, j) order, with no compare of indices.  A lane
//     whose compare was made against a `worst` that an earlier pair of the same four has lowered since inserts nothing: no
//     entry is above its d2.
//   * Padding entries and lanes without a row carry x = NaN (nbody_rows.hpp): d2 = NaN passes no compare.  kOwn: only the
//     wave's self tile applies j != i.
//   * The result: K entries of 12 bytes per row, a row's entries next to each other ([row][c], the caller's order), so
//     rows_run sends them on as they stand.  An empty system's explicit points get their k empty entries from the workgroup's
//     early exit, here, not from rows_prologue: a row has k records, not one.
//
// How often the rare path runs, by counting: a row inserts about K ln(n / K) times over its walk (the chance that source j
// is among the K nearest of the first j is K / j), so some lane of a wave of 64 rows inserts on about 64 K (1 + ln(n / (64 K)))
// of its n sources: nearly all of the first 64 K, then ever fewer.  At n = 130965, the state of the probe, that is 1.4 %
// (K = 4), 2.6 % (8), 4.6 % (16) and 8.1 % (32) of the pairs, each such pair costing one insertion of about 7 K instructions
// against about 9 per pair on the hot path: 1.04 / 1.16 / 1.57 / 3.0 times the walk without insertions.
// Measured (profiles/knn_probe.txt; one MI355X, fp32, own form, n = 130965, neighbors_at in the same run 9.49 ms): 5.94 /
// 6.49 / 8.63 / 15.76 ms for K = 4 / 8 / 16 / 32, k = 1 on the 4-entry tier 6.00 ms.  With the 4-entry tier as the base, the
// count predicts 6.6 / 8.9 / 17.1 ms for the three larger tiers: the measurement follows it and stays 2 to 8 per cent below,
// the more the larger the tier.  Why it stays below was not measured (no counters were read); the 7 K and the 9 are counts
// of instructions in the listing, not of cycles.  k = 1 is 0.63 of neighbors_at's time per pair: no
// overlap count (an add, a multiply, a compare, an add-with-carry) and no selects on the hot path.
//
// Registers (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; 256-thread workgroups; the same for fp32
// and fp64 records, a context and a batch: 24 instantiations):
//     tier K   VGPRs own / points   SGPRs own / points   scratch   LDS bytes   waves per SIMD
//        4          50 / 46              45 / 42            0        4096            8
//        8          62 / 62              45 / 42            0        4096            8
//       16          94 / 94              45 / 42            0        4096            5
//       32         158 / 158             45 / 42            0        4096            3
// No instantiation uses scratch.  The 32-entry list is 96 registers; a 256-thread workgroup is one wave per SIMD and could use
// 512, so that tier keeps its list in registers like the others: neither LDS nor a smaller workgroup was needed.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

// One entry of a row's list as device code writes it and the pinned staging holds it.
struct __attribute__((packed, aligned(4))) KnnEntry { double d2; int32_t index; };
static_assert(sizeof(KnnEntry) == 12, "an entry is the caller's 8 + 4 bytes");

// What a row carries along the j stream: the K nearest so far under (d2, j), ascending; {+inf, -1} where there is none yet.
template <int K>
struct KnnList {
    double d2[K];
    int index[K];
};

// Source j at squared distance v goes behind every entry whose d2 is <= v; the last entry drops out.  Nothing changes where
// no entry is above v (v at or above the worst, v = NaN).  d2 is sorted, so an entry whose predecessor is above v is above v
// too: it takes its predecessor's place; the one entry above v whose predecessor is not takes the new pair.
template <int K>
__device__ __forceinline__ void knn_insert(KnnList<K>& a, double v, int j) {
    bool above = a.d2[K - 1] > v;                                // of entry c
#pragma unroll
    for (int c = K - 1; c > 0; --c) {
        const bool prev = a.d2[c - 1] > v;                       // of entry c - 1
        const double d = prev ? a.d2[c - 1] : v;
        const int x = prev ? a.index[c - 1] : j;
        a.d2[c] = above ? d : a.d2[c];
        a.index[c] = above ? x : a.index[c];
        above = prev;
    }
    a.d2[0] = above ? v : a.d2[0];
    a.index[0] = above ? j : a.index[0];
}

// The four pairs of one trip of rows_walk: sources j .. j + 3 at entries q .. q + 3 of buffer b.  kChecked: the tile holds
// the wave's own rows, the self term j == i is no source.
template <int K>
struct KnnFour {
    const DiagPlanes *sx, *sy;
    int i; RowsRow w;               // the row
    KnnList<K> a;
    template <bool kChecked>
    __device__ __forceinline__ void four(int b, int q, int j) {
        bool hit[4];
        double d2[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = (*sx)[b][q + u] - w.x, dy = (*sy)[b][q + u] - w.y;
            d2[u] = (dx * dx) + (dy * dy);
            hit[u] = (!kChecked || j + u != i) && d2[u] < a.d2[K - 1];
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare once the list is full: see the head of the file
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (hit[u]) knn_insert(a, d2[u], j + u);         // in j order
        }
    }
};

// grid and early exits: rows_prologue; the full walk: rows_walk (nbody_rows.hpp).  out_all: k entries per row, system sys's
// rows from sys * (kOwn ? stride : m) on, as rows_run lays out every query's records.
template <typename T, bool kOwn, typename Count, int K>
__global__ __launch_bounds__(kDiagBlock) void knn_at(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                     Counters* __restrict__ ctr_all, int stride, int n_one,
                                                     const FieldPoint* __restrict__ points, int m, int k,
                                                     KnnEntry* __restrict__ out_all) {
    RowsLane<T, RowsNoOut> L;
    const bool leave = rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, (RowsNoOut*)nullptr, RowsNoOut{});
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int p = blockIdx.x * kDiagBlock + threadIdx.x;
    KnnEntry* __restrict__ out = out_all + ((size_t)sys * (size_t)(kOwn ? stride : m) + (size_t)p) * (size_t)k;
    if (leave) {                                                 // no row in this workgroup, or an empty system: its explicit
        if (p < L.rows)                                          // points get k empty entries each (it has no own rows)
            for (int c = 0; c < k; ++c) out[c] = KnnEntry{__builtin_inf(), -1};
        return;
    }
    __shared__ double sx[2][kTile], sy[2][kTile];
    KnnFour<K> f{&sx, &sy, L.p, rows_row<T, kOwn>(L, points), {}};
#pragma unroll
    for (int c = 0; c < K; ++c) { f.a.d2[c] = __builtin_inf(); f.a.index[c] = -1; }
    rows_walk<kOwn, false>(L, RowsStage<false, T>{L.J, &sx, &sy, nullptr}, f);
    if (L.valid) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (c < k) out[c] = KnnEntry{f.a.d2[c], f.a.index[c]};
    }
}

// The query's traits for rows_run (nbody_rows.hpp): k entries per row, taken apart into the caller's two arrays.
using KnnState = PointBuffers<KnnEntry>;

struct KnnResult { double* d2; int32_t* index; };                // the caller's, [rows * k] each

struct KnnQuery {
    using Device = KnnEntry;
    using Result = KnnResult;
    int k;
    template <typename T, bool kOwn, typename Count, typename... Common>
    void launch(dim3 grid, hipStream_t stream, KnnEntry* out, Common... common) const {
        const dim3 block(kDiagBlock);                            // the smallest tier >= k
        if (k <= 4) hipLaunchKernelGGL((knn_at<T, kOwn, Count, 4>), grid, block, 0, stream, common..., k, out);
        else if (k <= 8) hipLaunchKernelGGL((knn_at<T, kOwn, Count, 8>), grid, block, 0, stream, common..., k, out);
        else if (k <= 16) hipLaunchKernelGGL((knn_at<T, kOwn, Count, 16>), grid, block, 0, stream, common..., k, out);
        else hipLaunchKernelGGL((knn_at<T, kOwn, Count, 32>), grid, block, 0, stream, common..., k, out);
    }
    size_t width() const { return (size_t)k; }
    void empty(int) const {}
    void unpack(int, const KnnEntry* h, size_t cnt, KnnResult* out, size_t row0) const {
        double* d2 = out->d2 + row0 * (size_t)k;
        int32_t* index = out->index + row0 * (size_t)k;
        for (size_t e = 0; e < cnt * (size_t)k; ++e) { d2[e] = h[e].d2; index[e] = h[e].index; }
    }
};

// The argument checks an entry point makes before any device call: k, then the pointers, m and the size of the caller's
// results (12 bytes per entry, k entries per row, every system's).
inline int knn_check_args(const char* who, std::initializer_list<const void*> required, int m, int k, unsigned long long systems) {
    static_assert(NBODY_KNN_MAX == 32, "the largest tier of KnnQuery::launch");
    if (k < 1 || k > NBODY_KNN_MAX) return nbody_fail(NBODY_ERR_INVALID, "%s: k = %d (1 .. %d)", who, k, NBODY_KNN_MAX);
    return rows_check_args(who, required, m, systems * (unsigned long long)k * sizeof(KnnEntry), " of results");
}

}  // namespace nbk
