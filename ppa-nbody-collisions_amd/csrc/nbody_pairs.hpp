// csrc/nbody_pairs.hpp -- pair-separation counts on the resident state (nbody_get_pair_counts, nbody_batch_get_pair_counts,
// include/nbody.h): how many pairs fall into each bin of squared separation - the DD (bodies with bodies)
// and DR (probe points with bodies) counts a correlation function is made of.  The launch geometry, the count and the early
// exits are those of every row query (nbody_rows.hpp); this file has the pair, the two tile walks, the histogram and the host
// side.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  A row at (x, y)
// and a source j with the record (X_j, Y_j) widened exactly:
//     dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)                       the d2 of nbody_get_neighbors
//     counts[k] = the number of counted pairs with  e2[k] <= d2 && d2 < e2[k+1]   k = 0 .. B-1
//     below     = the number with  d2 < e2[0]
// over B + 1 strictly increasing squared edges.  Own form: the unordered pairs of bodies, each once - d2_ij and d2_ji have the
// same bits (dx only changes sign), so row i counts the sources j < i and nothing else.  Points form: every (point, body)
// pair.  Counts are integers: the result does not depend on the order the device adds them in.
//
// pair_counts: one lane per row, rows_walk over {x, y} planes (no radius plane): triangular for kOwn, with the test j < i on
// the wave's own tile; full with no checked loop for points.  A NaN d2 (padding, a lane without a row) fails every `<`.
//   * Hot path, per pair: 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 < e2[B].  Four pairs share one branch
//     around the rare path.
//   * Rare path (a pair below the top edge): a branchless binary search over the edges in LDS - they are copied there once,
//     before the first barrier, followed by +inf up to the next power of two, so the search needs no bound test and its trip
//     count ceil(log2(B + 1)) is workgroup-uniform.  It gives slot = the number of edges <= d2: slot 0 is `below`, slots
//     1 .. B are the bins; then one atomicAdd on the workgroup's 64-bit LDS counter hist[slot].
//   * Flush: one barrier after the walk, then the lanes k <= B whose counter is not zero add it to the system's histogram in
//     device memory with one 64-bit atomicAdd each.  The host clears that histogram before the launch and derives `rest`.
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

static_assert(sizeof(nbody_pair_info) == 40, "nbody_pair_info layout");

constexpr int kPairMaxBins = 256;
constexpr int kPairEdgeSlots = 512;            // the edges in LDS: e2[0 .. B-1], then +inf; a power of two above every probe

// The number of edges <= d2, for a d2 below the top edge: e[k] is e2[k] for k < B and +inf from there on, `first` is
// 2^(trips - 1) with trips = ceil(log2(B + 1)), so lo + step - 1 <= 2^trips - 2 < kPairEdgeSlots.
__device__ __forceinline__ int pair_slot(const double* e, int first, double d2) {
    int lo = 0;
    for (int step = first; step > 0; step >>= 1) lo += e[lo + step - 1] <= d2 ? step : 0;
    return lo;
}

// One pair: source j at (xj, yj) - references into the LDS tile - and the row at (xi, yi).
__device__ __forceinline__ double pair_d2(const double& xj, const double& yj, double xi, double yi) {
    const double dx = xj - xi, dy = yj - yi;
    return (dx * dx) + (dy * dy);
}

// The four pairs of one trip of rows_walk: sources j .. j + 3 at entries q .. q + 3 of buffer b.  kChecked: the tile holds
// the wave's own rows, only a source below the row i counts.
struct PairFour {
    const DiagPlanes *sx, *sy;
    int i; RowsRow w;               // the row
    double top;                     // e2[B]
    const double* se; int first;    // pair_slot's
    unsigned long long* hist;
    template <bool kChecked>
    __device__ __forceinline__ void four(int b, int q, int j) {
        bool hit[4];
        double d2[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            d2[u] = pair_d2((*sx)[b][q + u], (*sy)[b][q + u], w.x, w.y);
            hit[u] = (!kChecked || j + u < i) && d2[u] < top;
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare where the top edge is small against the system
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (hit[u]) atomicAdd(hist + pair_slot(se, first, d2[u]), 1ull);
        }
    }
};

// grid and early exits: rows_prologue; the walk: rows_walk (nbody_rows.hpp), triangular for kOwn, full for points.  edges2:
// bins + 1 squared edges; hist_all: bins + 1 counters per system, cleared by the host - slot 0 is `below`, slot k + 1 is
// counts[k].
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void pair_counts(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                          Counters* __restrict__ ctr_all, int stride, int n_one,
                                                          const FieldPoint* __restrict__ points, int m,
                                                          const double* __restrict__ edges2, int bins,
                                                          unsigned long long* __restrict__ hist_all) {
    RowsLane<T, RowsNoOut> L;
    if (rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, (RowsNoOut*)nullptr, RowsNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x;
    __shared__ double se[kPairEdgeSlots];
    __shared__ unsigned long long hist[kPairMaxBins + 1];
    __shared__ double sx[2][kTile], sy[2][kTile];
    for (int k = tid; k < kPairEdgeSlots; k += kDiagBlock) se[k] = k < bins ? edges2[k] : __builtin_inf();
    for (int k = tid; k <= bins; k += kDiagBlock) hist[k] = 0;   // both before the first barrier
    int first = 1;
    while (2 * first <= bins) first *= 2;                        // 2^(ceil(log2(bins + 1)) - 1): workgroup-uniform
    PairFour f{&sx, &sy, L.p, rows_row<T, kOwn>(L, points), edges2[bins], se, first, hist};
    rows_walk<kOwn, kOwn>(L, RowsStage<false, T>{L.J, &sx, &sy, nullptr}, f);
    __syncthreads();                                             // every LDS count of the workgroup is in
    unsigned long long* __restrict__ g = hist_all + (size_t)sys * (size_t)(bins + 1);
    for (int k = tid; k <= bins; k += kDiagBlock) {
        const unsigned long long v = hist[k];
        if (v) atomicAdd(g + k, v);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, allocated on the first call: the edges and the histograms are sized for
// kPairMaxBins whatever the call asks for, the points (RowPoints, nbody_rows.hpp) grow to the largest m seen.
// ---------------------------------------------------------------------------------------------------------
struct PairsState {
    double* edges = nullptr;                // [kPairMaxBins + 1]
    unsigned long long* hist = nullptr;     // [systems * (kPairMaxBins + 1)], a call uses systems * (bins + 1)
    unsigned char* h = nullptr;             // pinned: the edges, then the histograms
    RowPoints pts;
};

inline void pairs_free(PairsState& g) {
    (void)hipFree(g.edges); (void)hipFree(g.hist);
    if (g.h) (void)hipHostFree(g.h);
    rows_free(g.pts);
    g = PairsState{};
}

inline int pairs_reserve(PairsState& g, size_t systems, size_t n_pts, const char* who) {
    constexpr size_t kSlots = kPairMaxBins + 1;
    hipError_t e = hipSuccess;
    if (!g.h) {
        e = hipMalloc((void**)&g.edges, kSlots * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&g.hist, systems * kSlots * sizeof(unsigned long long));
        if (e == hipSuccess)
            e = hipHostMalloc((void**)&g.h, kSlots * sizeof(double) + systems * kSlots * sizeof(unsigned long long),
                              hipHostMallocDefault);
        if (e != hipSuccess) g.h = nullptr;
    }
    if (e == hipSuccess) e = rows_reserve(g.pts, n_pts);
    if (e != hipSuccess) {
        pairs_free(g);
        return rows_alloc_failed(e, who, "edge, histogram and point buffers");
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call: the pointers and m, then the query's values.
inline int pairs_check_args(const char* who, std::initializer_list<const void*> required, int m, const double* edges2, int bins) {
    const int rc = rows_check_args(who, required, m, sizeof(nbody_vec2), "");
    if (rc != NBODY_OK) return rc;
    if (bins < 1 || bins > kPairMaxBins) return nbody_fail(NBODY_ERR_INVALID, "%s: bins = %d (1 .. %d)", who, bins, kPairMaxBins);
    if (!(edges2[0] >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: edges2[0] = %g (a squared length: >= 0)", who, edges2[0]);
    for (int k = 1; k <= bins; ++k)
        if (!(edges2[k] > edges2[k - 1]))
            return nbody_fail(NBODY_ERR_INVALID, "%s: edges2[%d] = %g is not above edges2[%d] = %g", who, k, edges2[k], k - 1,
                              edges2[k - 1]);
    return NBODY_OK;
}

// One call, from the reservation to the caller's counts; the site, Count and read_meta as for rows_run (nbody_rows.hpp).
// `rest` is derived here, on the host.
template <typename T, typename Count, typename ReadMeta>
int pairs_run(const char* who, const RowsSite& s, PairsState& g, const nbody_vec2* points, int m, const double* edges2, int bins,
              uint64_t* counts, nbody_pair_info* info, ReadMeta read_meta) {
    const bool own = points == nullptr;
    const int rows = own ? s.n_bound : m;                                  // what the grid covers
    const size_t S = (size_t)s.systems, slots = (size_t)bins + 1;
    const bool launched = rows > 0 && s.n_bound > 0;
    if (launched) {
        int rc = pairs_reserve(g, S, own ? 0 : (size_t)m, who);
        if (rc != NBODY_OK) return rc;
        const dim3 grid = s.grid(rows), block(kDiagBlock);
        const Rec<T>* J = (const Rec<T>*)s.J;
        memcpy(g.h, edges2, slots * sizeof(double));
        NBK_ROWS_TRY(hipMemcpyAsync(g.edges, g.h, slots * sizeof(double), hipMemcpyHostToDevice, s.stream));
        NBK_ROWS_TRY(hipMemsetAsync(g.hist, 0, S * slots * sizeof(unsigned long long), s.stream));
        if (own) {
            hipLaunchKernelGGL((pair_counts<T, true, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride,
                               s.n_one<Count>(), (const FieldPoint*)nullptr, 0, (const double*)g.edges, bins, g.hist);
        } else {
            NBK_ROWS_TRY(rows_upload(g.pts, points, m, s.stream));
            hipLaunchKernelGGL((pair_counts<T, false, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride,
                               s.n_one<Count>(), (const FieldPoint*)g.pts.d, m, (const double*)g.edges, bins, g.hist);
        }
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(g.h + (kPairMaxBins + 1) * sizeof(double), g.hist, S * slots * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    const unsigned long long* h =
        launched ? reinterpret_cast<const unsigned long long*>(g.h + (kPairMaxBins + 1) * sizeof(double)) : nullptr;   // no staging yet
    for (int sys = 0; sys < s.systems; ++sys) {
        const int64_t n = s.count(sys);
        const int64_t r = own ? n : (int64_t)m;
        const int64_t pairs = own ? n * (n - 1) / 2 : r * n;
        uint64_t* out = counts + (size_t)sys * (size_t)bins;
        uint64_t below = 0, inside = 0;
        for (int k = 0; k < bins; ++k) out[k] = 0;
        if (h && pairs > 0) {
            const unsigned long long* hs = h + (size_t)sys * slots;
            below = hs[0];
            for (int k = 0; k < bins; ++k) {
                out[k] = hs[k + 1];
                inside += hs[k + 1];
            }
        }
        info[sys] = nbody_pair_info{n, r, pairs, (int64_t)below, pairs - (int64_t)below - (int64_t)inside};
    }
    return NBODY_OK;
}

}  // namespace nbk
