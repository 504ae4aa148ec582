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
// pair_counts: one lane per row, kDiagBlock lanes per workgroup.  A tile's {x, y} are widened to fp64 once into
// double-buffered LDS planes, as groups_sweep does, the ragged tile padded with x = NaN; a lane without a row carries
// x = NaN.  A NaN d2 fails every `<`, so the pair loop carries no bound test.
//   * kOwn: the triangular walk of groups_sweep - tiles up to the one that holds the workgroup's last row are staged, a wave
//     computes on the tiles below its own rows without an index test, on its own tile with the test j < i and only up to its
//     last row, and on none above.  Points: the full walk with no checked loop, as neighbors_at<T, false>.
//   * Hot path, per pair: 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 < e2[B].  Four pairs share one branch
//     around the rare path, as the hit[4] / any of groups_sweep.
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

// A row query with no per-row result: rows_prologue's write of the empty record is this assignment, which writes nothing.
struct PairNoOut {
    PairNoOut() = default;
    PairNoOut(const PairNoOut&) = default;
    __host__ __device__ PairNoOut& operator=(const PairNoOut&) { return *this; }
};

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

// The four pairs of one trip of the tile loop: sources j .. j + 3 at entries q .. q + 3 of the planes (sx, sy).  kChecked:
// the tile holds the wave's own rows, only a source below the row i counts.
template <bool kChecked>
__device__ __forceinline__ void pair_four(const double* sx, const double* sy, int q, int j, int i, double xi, double yi,
                                          double top, const double* se, int first, unsigned long long* hist) {
    bool hit[4];
    double d2[4];
    int any = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        d2[u] = pair_d2(sx[q + u], sy[q + u], xi, yi);
        hit[u] = (!kChecked || j + u < i) && d2[u] < top;
        any += hit[u] ? 1 : 0;
        asm("" : "+v"(any));                                     // as groups_sweep: one add-with-carry per compare mask
    }
    if (any) {                                                   // rare where the top edge is small against the system
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (hit[u]) atomicAdd(hist + pair_slot(se, first, d2[u]), 1ull);
    }
}

// grid and early exits: rows_prologue (nbody_rows.hpp).  edges2: bins + 1 squared edges; hist_all: bins + 1 counters per
// system, cleared by the host - slot 0 is `below`, slot k + 1 is counts[k].
template <typename T, bool kOwn, typename Count>
__global__ __launch_bounds__(kDiagBlock) void pair_counts(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                          Counters* __restrict__ ctr_all, int stride, int n_one,
                                                          const FieldPoint* __restrict__ points, int m,
                                                          const double* __restrict__ edges2, int bins,
                                                          unsigned long long* __restrict__ hist_all) {
    RowsLane<T, PairNoOut> L;
    if (rows_prologue<T, kOwn, Count>(L, J_all, meta_all, ctr_all, stride, n_one, m, (PairNoOut*)nullptr, PairNoOut{})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const Rec<T>* __restrict__ J = L.J;
    const int n = L.n, p = L.p, tid = threadIdx.x;
    __shared__ double se[kPairEdgeSlots];
    __shared__ unsigned long long hist[kPairMaxBins + 1];
    __shared__ double sx[2][kTile], sy[2][kTile];
    for (int k = tid; k < kPairEdgeSlots; k += kDiagBlock) se[k] = k < bins ? edges2[k] : __builtin_inf();
    for (int k = tid; k <= bins; k += kDiagBlock) hist[k] = 0;   // both before the first barrier
    const double top = edges2[bins];
    int first = 1;
    while (2 * first <= bins) first *= 2;                        // 2^(ceil(log2(bins + 1)) - 1): workgroup-uniform
    double xi = __builtin_nan(""), yi = 0.0;                     // a lane without a row counts nothing
    if (L.valid) {
        if (kOwn) {
            const Rec<T> r = J[p];
            xi = (double)r.x; yi = (double)r.y;
        } else {
            const FieldPoint q = points[p];
            xi = q.x; yi = q.y;
        }
    }
    const int row0 = blockIdx.x * kDiagBlock;
    const int last = (row0 + kDiagBlock < n ? row0 + kDiagBlock : n) - 1;   // kOwn: the workgroup's last row
    const int jtiles = kOwn ? last / kTile + 1 : (n + kTile - 1) / kTile;   // workgroup-uniform
    const int wave_end = row0 + (tid & ~(kWave - 1)) + kWave;    // one past the wave's last row
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) {
            double x = __builtin_nan(""), y = 0.0;               // padding: d2 = NaN
            if (tid < jn) {
                const Rec<T> s = J[j0 + tid];
                x = (double)s.x; y = (double)s.y;
            }
            sx[b][tid] = x; sy[b][tid] = y;
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!L.wave_works || (kOwn && t > L.self_tile)) continue;
        if (!kOwn || t != L.self_tile) {
            const int jn4 = (jn + 3) & ~3;                       // <= kTile: the padding is there
            for (int q = 0; q < jn4; q += 4) pair_four<false>(sx[b], sy[b], q, j0 + q, p, xi, yi, top, se, first, hist);
        } else {
            const int je = wave_end - j0 < jn ? wave_end - j0 : jn;   // no row of this wave is above wave_end - 1
            const int jn4 = (je + 3) & ~3;
            for (int q = 0; q < jn4; q += 4) pair_four<true>(sx[b], sy[b], q, j0 + q, p, xi, yi, top, se, first, hist);
        }
    }
    __syncthreads();                                             // every LDS count of the workgroup is in
    unsigned long long* __restrict__ g = hist_all + (size_t)sys * (size_t)(bins + 1);
    for (int k = tid; k <= bins; k += kDiagBlock) {
        const unsigned long long v = hist[k];
        if (v) atomicAdd(g + k, v);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, allocated on the first call: the edges and the histograms are sized for
// kPairMaxBins whatever the call asks for, the points grow to the largest m seen.
// ---------------------------------------------------------------------------------------------------------
struct PairsState {
    double* edges = nullptr;                // [kPairMaxBins + 1]
    unsigned long long* hist = nullptr;     // [systems * (kPairMaxBins + 1)], a call uses systems * (bins + 1)
    FieldPoint* pts = nullptr;              // [cap_pts]
    unsigned char* h = nullptr;             // pinned: the edges, then the histograms
    unsigned char* h_pts = nullptr;         // pinned: cap_pts points
    size_t cap_pts = 0;
};

inline void pairs_free(PairsState& g) {
    (void)hipFree(g.edges); (void)hipFree(g.hist); (void)hipFree(g.pts);
    if (g.h) (void)hipHostFree(g.h);
    if (g.h_pts) (void)hipHostFree(g.h_pts);
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
    if (e == hipSuccess && n_pts > g.cap_pts) {
        (void)hipFree(g.pts);
        if (g.h_pts) (void)hipHostFree(g.h_pts);
        g.pts = nullptr; g.h_pts = nullptr; g.cap_pts = 0;
        e = hipMalloc((void**)&g.pts, n_pts * sizeof(FieldPoint));
        if (e == hipSuccess) e = hipHostMalloc((void**)&g.h_pts, n_pts * sizeof(FieldPoint), hipHostMallocDefault);
        if (e == hipSuccess) g.cap_pts = n_pts; else g.h_pts = nullptr;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pairs_free(g);
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, edge, histogram and point buffers: %s",
                          who, hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call.
inline int pairs_check_args(const char* who, std::initializer_list<const void*> required, int m, const double* edges2, int bins) {
    for (const void* p : required)
        if (!p) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (m < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: m = %d", who, m);
    if ((unsigned long long)m * sizeof(nbody_vec2) > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d points are more than 2^31 bytes", who, m);
    if (bins < 1 || bins > kPairMaxBins) return nbody_fail(NBODY_ERR_INVALID, "%s: bins = %d (1 .. %d)", who, bins, kPairMaxBins);
    if (!(edges2[0] >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: edges2[0] = %g (a squared length: >= 0)", who, edges2[0]);
    for (int k = 1; k <= bins; ++k)
        if (!(edges2[k] > edges2[k - 1]))
            return nbody_fail(NBODY_ERR_INVALID, "%s: edges2[%d] = %g is not above edges2[%d] = %g", who, k, edges2[k], k - 1,
                              edges2[k - 1]);
    return NBODY_OK;
}

// One call, from the reservation to the caller's counts.  Count says whose, as for rows_run: a context hands over the exact
// count it has just read (s.n_bound), a batch an upper bound, and the kernel takes each count from Meta.  read_meta
// synchronises the stream and reports a device-side failure; `rest` is derived here, on the host.
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
        const dim3 grid((rows + kDiagBlock - 1) / kDiagBlock, s.systems), block(kDiagBlock);
        const Rec<T>* J = (const Rec<T>*)s.J;
        const int n_one = Count::kBatch ? 0 : s.n_bound;
        memcpy(g.h, edges2, slots * sizeof(double));
        NBK_ROWS_TRY(hipMemcpyAsync(g.edges, g.h, slots * sizeof(double), hipMemcpyHostToDevice, s.stream));
        NBK_ROWS_TRY(hipMemsetAsync(g.hist, 0, S * slots * sizeof(unsigned long long), s.stream));
        if (own) {
            hipLaunchKernelGGL((pair_counts<T, true, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride, n_one,
                               (const FieldPoint*)nullptr, 0, (const double*)g.edges, bins, g.hist);
        } else {
            memcpy(g.h_pts, points, (size_t)m * sizeof(FieldPoint));
            NBK_ROWS_TRY(hipMemcpyAsync(g.pts, g.h_pts, (size_t)m * sizeof(FieldPoint), hipMemcpyHostToDevice, s.stream));
            hipLaunchKernelGGL((pair_counts<T, false, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride, n_one,
                               (const FieldPoint*)g.pts, m, (const double*)g.edges, bins, g.hist);
        }
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(g.h + (kPairMaxBins + 1) * sizeof(double), g.hist, S * slots * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, s.stream));
    }
    if (Count::kBatch || launched) {
        const int rc = read_meta();                            // synchronises; a system whose count failed its check ends here
        if (rc != NBODY_OK) return rc;
    }
    const unsigned long long* h =
        launched ? reinterpret_cast<const unsigned long long*>(g.h + (kPairMaxBins + 1) * sizeof(double)) : nullptr;   // no staging yet
    for (int sys = 0; sys < s.systems; ++sys) {
        const int c = s.h_meta[sys].n;
        const int64_t n = c < 0 || c > s.stride || c > s.n_bound ? 0 : c;
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
