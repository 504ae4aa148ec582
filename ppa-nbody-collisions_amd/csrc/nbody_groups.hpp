// csrc/nbody_groups.hpp -- group finding on the resident state (nbody_get_groups, nbody_batch_get_groups, include/nbody.h;
// DESIGN.md 4.10): friends-of-friends, the connected components of the graph of linked pairs, label[i] = the lowest index
// of body i's component.  The launch geometry, the count and the early exits are those of every row query
// (nbody_rows.hpp); this file has the pair, the triangular tile walk, the parent array and the host loop.
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  Bodies i != j
// with records (X, Y, R) widened exactly:
//     dx = X_j - X_i;  dy = Y_j - Y_i;  d2 = (dx*dx) + (dy*dy)
//     s  = (radius_scale * (R_i + R_j)) + link
//     linked(i, j)  <=>  d2 <= s*s
// symmetric bit for bit, so only the pairs j < i are walked.
//
// Hook and repeat.  parent[i] = i (groups_init); then groups_sweep until a sweep changes nothing; then groups_flatten.
//   * parent[x] <= x always: it starts as x and is only ever lowered (atomicMin) to an index of x's own component.  So
//     groups_find, which follows parent until parent[x] == x, strictly descends and ends whatever mixture of old and new
//     values it reads, and what it returns is some ancestor of x in x's component.
//   * A sweep walks every pair j < i; on a linked pair whose two finds differ it sets the system's `changed` word and lowers
//     the parent of the larger root to the smaller.  It does not retry and it waits for nobody: no device-side spin, no loop
//     whose end depends on another workgroup.
//   * A sweep that sets no `changed` word has written nothing, so every read it made was of memory as the launch found it
//     (kernel boundaries are coherent), and in that memory every linked pair shares a root: every component has one root,
//     and since parent[m] <= m stays inside the component its lowest index m is that root.  groups_flatten then reads
//     label[i] = find(i) = m.
//   * The bound.  A sweep that sees unequal roots somewhere removes at least one true root: if nothing was written during
//     the sweep, the lane that looked saw the truth and its atomicMin lowers a root; otherwise some write lowered one.  A
//     system has at most n roots, and the last sweep only confirms: sweeps <= n + 1.  The host gives up there.
//   * find reads with relaxed device-scope atomic loads - not needed for any of the above, which holds for arbitrarily
//     stale reads, but a fresher view hooks more in one sweep, and the read is on the rare path only.
//
// groups_sweep: one lane per body i, kDiagBlock lanes per workgroup.  A tile's {x, y, r} are widened to fp64 once into
// double-buffered LDS planes, as neighbors_at does, the ragged tile padded with x = NaN (d2 = NaN links nothing; a lane
// without a row carries x = NaN for the same reason).  The walk is triangular: a workgroup stages only the tiles up to the
// one that holds its last row (a workgroup-uniform bound: the barriers need it); a wave computes on the tiles below its own
// rows without an index test, on its own tile (nbody_rows.hpp: self_tile) with the test j < i and only up to its last row,
// and on none above.
// Per pair: 2 subtractions, 2 multiplies, 1 add for d2; 1 add, 1 multiply, 1 add for s; 1 multiply, 1 compare.
// A batch: the system's `changed` word of the previous sweep is read at the prologue and a system that had converged
// leaves there (nothing writes its parents any more); the words of this sweep are another array, cleared by the host before
// the launch, so the exit races with nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_groups_info) == 16, "nbody_groups_info layout");

// The root of x as this lane sees it: strictly descending, see above.
__device__ __forceinline__ int groups_find(const int32_t* parent, int x) {
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// A linked pair (rare): one hook, no retry.
__device__ __forceinline__ void groups_hook(int32_t* parent, int* changed, int i, int j) {
    const int ri = groups_find(parent, i), rj = groups_find(parent, j);
    if (ri == rj) return;
    *changed = 1;
    atomicMin(parent + (ri > rj ? ri : rj), ri > rj ? rj : ri);
}

// One pair: source j at (xj, yj) with radius rj - references into the LDS tile - and body i.  kChecked: the tile holds the
// wave's own rows, only j < i counts.
template <bool kChecked>
__device__ __forceinline__ bool groups_linked(const double& xj, const double& yj, const double& rj, int j, int i, double xi,
                                              double yi, double ri, double link, double scale) {
    const double dx = xj - xi, dy = yj - yi;
    const double d2 = (dx * dx) + (dy * dy);
    const double s = (scale * (ri + rj)) + link;
    return (!kChecked || j < i) && d2 <= s * s;
}

// grid = (ceil(n_bound / kDiagBlock), systems): covers every parent a sweep can read, whatever the counts are.  (A template
// like the other two: one definition per translation unit that asks for it.)
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void groups_init(int32_t* __restrict__ parent_all, int stride, int n_bound) {
    const int i = blockIdx.x * kDiagBlock + threadIdx.x;
    if (i < n_bound && i < stride) parent_all[(size_t)blockIdx.y * (size_t)stride + i] = i;
}

// grid and early exits: rows_prologue (nbody_rows.hpp).  prev / cur: the systems' `changed` words of the last sweep and of
// this one.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void groups_sweep(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                           Counters* __restrict__ ctr_all, int stride, int n_one, double link,
                                                           double scale, int32_t* parent_all, const int* __restrict__ prev,
                                                           int* __restrict__ cur) {
    RowsLane<T, int32_t> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, parent_all, (int32_t)0)) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    if (prev[sys] == 0) return;                                  // converged in an earlier sweep: the whole workgroup
    const Rec<T>* __restrict__ J = L.J;
    int32_t* parent = L.out;
    int* changed = cur + sys;
    const int n = L.n, p = L.p, tid = threadIdx.x;
    double xi = __builtin_nan(""), yi = 0.0, ri = 0.0;           // a lane without a row links nothing
    if (L.valid) {
        const Rec<T> r = J[p];
        xi = (double)r.x; yi = (double)r.y; ri = (double)r.r;
    }
    __shared__ double sx[2][kTile], sy[2][kTile], sr[2][kTile];
    const int row0 = blockIdx.x * kDiagBlock;
    const int last = (row0 + kDiagBlock < n ? row0 + kDiagBlock : n) - 1;   // the workgroup's last row
    const int jtiles = last / kTile + 1;                         // workgroup-uniform
    const int wave_end = row0 + (tid & ~(kWave - 1)) + kWave;    // one past the wave's last row
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) {
            double x = __builtin_nan(""), y = 0.0, r = 0.0;      // padding: d2 = NaN
            if (tid < jn) {
                const Rec<T> s = J[j0 + tid];
                x = (double)s.x; y = (double)s.y; r = (double)s.r;
            }
            sx[b][tid] = x; sy[b][tid] = y; sr[b][tid] = r;
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!L.wave_works || t > L.self_tile) continue;
        if (t != L.self_tile) {
            const int jn4 = (jn + 3) & ~3;                       // <= kTile: the padding is there
            for (int q = 0; q < jn4; q += 4) {
                bool hit[4];
                int any = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hit[u] = groups_linked<false>(sx[b][q + u], sy[b][q + u], sr[b][q + u], j0 + q + u, p, xi, yi, ri, link, scale);
                    any += hit[u] ? 1 : 0;
                    asm("" : "+v"(any));                         // as neighbor_pair: one add-with-carry per compare mask
                }
                if (any) {                                       // rare
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit[u]) groups_hook(parent, changed, p, j0 + q + u);
                }
            }
        } else {
            const int je = wave_end - j0 < jn ? wave_end - j0 : jn;   // no row of this wave is above wave_end - 1
            const int jn4 = (je + 3) & ~3;
            for (int q = 0; q < jn4; q += 4) {
                bool hit[4];
                int any = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hit[u] = groups_linked<true>(sx[b][q + u], sy[b][q + u], sr[b][q + u], j0 + q + u, p, xi, yi, ri, link, scale);
                    any += hit[u] ? 1 : 0;
                    asm("" : "+v"(any));                         // as neighbor_pair: one add-with-carry per compare mask
                }
                if (any) {                                       // rare
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit[u]) groups_hook(parent, changed, p, j0 + q + u);
                }
            }
        }
    }
}

// label[i] = find(i), after the sweep that changed nothing: the lowest index of i's component.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void groups_flatten(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                             Counters* __restrict__ ctr_all, int stride, int n_one,
                                                             const int32_t* parent_all, int32_t* __restrict__ label_all) {
    RowsLane<T, int32_t> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, label_all, (int32_t)0)) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    if (L.valid) L.out[L.p] = groups_find(parent_all + (size_t)sys * (size_t)stride, L.p);
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch, allocated on the first call: they depend on systems * stride only.
// ---------------------------------------------------------------------------------------------------------
struct GroupsState {
    int32_t* parent = nullptr;      // [systems * stride]
    int32_t* label = nullptr;       // [systems * stride]
    int* changed = nullptr;         // [2][systems]: the words of the last sweep and of this one, in turns
    unsigned char* h = nullptr;     // pinned: systems * stride labels, then `systems` changed words
};

inline void groups_free(GroupsState& g) {
    (void)hipFree(g.parent); (void)hipFree(g.label); (void)hipFree(g.changed);
    if (g.h) (void)hipHostFree(g.h);
    g = GroupsState{};
}

inline int groups_reserve(GroupsState& g, size_t total, size_t systems, const char* who) {
    if (g.h) return NBODY_OK;
    hipError_t e = hipMalloc((void**)&g.parent, total * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g.label, total * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g.changed, 2 * systems * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void**)&g.h, total * sizeof(int32_t) + systems * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g.h = nullptr;
        groups_free(g);
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, parent and label buffers: %s", who,
                          hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call.
inline int groups_check_args(const char* who, double link, double radius_scale, std::initializer_list<const void*> required) {
    if (!(link >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: link = %g (a length: >= 0, +inf allowed)", who, link);
    if (!(radius_scale >= 0.0) || radius_scale == __builtin_inf())
        return nbody_fail(NBODY_ERR_INVALID, "%s: radius_scale = %g (finite and >= 0)", who, radius_scale);
    for (const void* p : required)
        if (!p) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    return NBODY_OK;
}

// n_groups and largest of one system's n labels.
inline void groups_summarise(const int32_t* label, int n, int sweeps, std::vector<int32_t>& size, nbody_groups_info* info) {
    size.assign((size_t)n, 0);
    int32_t groups = 0, largest = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t l = label[i];
        groups += l == i;
        if (l >= 0 && l < n && ++size[(size_t)l] > largest) largest = size[(size_t)l];
    }
    *info = nbody_groups_info{n, groups, largest, sweeps};
}

// One call, from the reservation to the caller's labels.  Count says whose, as for rows_run: a context hands over the exact
// count it has just read (s.n_bound), a batch an upper bound, and the kernels take each count from Meta.  read_meta
// synchronises the stream and reports a device-side failure.
template <typename T, typename Count, typename ReadMeta>
int groups_run(const char* who, const RowsSite& s, GroupsState& g, double link, double radius_scale, int32_t* label,
               nbody_groups_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, total = S * (size_t)s.stride;
    int sweeps = 0;
    if (s.n_bound > 0) {
        int rc = groups_reserve(g, total, S, who);
        if (rc != NBODY_OK) return rc;
        const dim3 grid((s.n_bound + kDiagBlock - 1) / kDiagBlock, s.systems), block(kDiagBlock);
        const Rec<T>* J = (const Rec<T>*)s.J;
        const int n_one = Count::kBatch ? 0 : s.n_bound;
        int* h_changed = reinterpret_cast<int*>(g.h + total * sizeof(int32_t));
        hipLaunchKernelGGL((groups_init<Count>), grid, block, 0, s.stream, g.parent, s.stride, s.n_bound);
        NBK_ROWS_TRY(hipGetLastError());
        int* prev = g.changed;
        int* cur = g.changed + S;
        NBK_ROWS_TRY(hipMemsetAsync(prev, 1, S * sizeof(int), s.stream));          // every system takes part in sweep 1
        bool again = true;
        while (again) {
            if (sweeps > s.n_bound)
                return nbody_fail(NBODY_ERR_HIP, "%s: did not converge in %d sweeps over at most %d bodies", who, sweeps, s.n_bound);
            NBK_ROWS_TRY(hipMemsetAsync(cur, 0, S * sizeof(int), s.stream));
            hipLaunchKernelGGL((groups_sweep<T, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride, n_one, link,
                               radius_scale, g.parent, (const int*)prev, cur);
            NBK_ROWS_TRY(hipGetLastError());
            ++sweeps;
            NBK_ROWS_TRY(hipMemcpyAsync(h_changed, cur, S * sizeof(int), hipMemcpyDeviceToHost, s.stream));
            NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
            again = false;
            for (size_t k = 0; k < S; ++k) again = again || h_changed[k] != 0;
            int* t = prev; prev = cur; cur = t;
        }
        hipLaunchKernelGGL((groups_flatten<T, Count>), grid, block, 0, s.stream, J, s.meta, s.counters, s.stride, n_one,
                           (const int32_t*)g.parent, g.label);
        NBK_ROWS_TRY(hipGetLastError());
        const size_t copied = Count::kBatch ? total : (size_t)s.n_bound;
        NBK_ROWS_TRY(hipMemcpyAsync(g.h, g.label, copied * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    }
    if (Count::kBatch || s.n_bound > 0) {
        const int rc = read_meta();                            // synchronises; a system whose count failed its check ends here
        if (rc != NBODY_OK) return rc;
    }
    std::vector<int32_t> size;
    for (int sys = 0; sys < s.systems; ++sys) {
        const int m = s.h_meta[sys].n;
        const int n = m < 0 || m > s.stride || m > s.n_bound ? 0 : m;
        const int32_t* h = n ? reinterpret_cast<const int32_t*>(g.h) + (size_t)sys * (size_t)s.stride : nullptr;   // no staging yet
        if (n) memcpy(label + (size_t)sys * (size_t)s.stride, h, (size_t)n * sizeof(int32_t));
        groups_summarise(h, n, sweeps, size, info + sys);
    }
    return NBODY_OK;
}

}  // namespace nbk
