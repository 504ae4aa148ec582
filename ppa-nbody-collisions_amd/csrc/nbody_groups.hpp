// csrc/nbody_groups.hpp -- group finding on the resident state (nbody_get_groups, nbody_batch_get_groups, include/nbody.h;
// DESIGN.md 4.10): friends-of-friends, the connected components of the graph of linked pairs, label[i] = the lowest index
// of body i's component.  The launch geometry, the count and the early exits are those of every row query
// (nbody_rows.hpp), and so is the tile walk (rows_walk, triangular shape); this file has the pair, the parent array and the
// host loop.
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
// groups_sweep: one lane per body i, rows_walk's triangular shape over {x, y, r} planes: a padding entry or a lane without a
// row has d2 = NaN and links nothing; on the wave's own tile the test is j < i.
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

// The four pairs of one trip of rows_walk: the hooks wait behind one branch, which is rarely taken.
struct GroupsFour {
    const DiagPlanes *sx, *sy, *sr;
    int i; RowsRow w;               // the row
    double link, scale;
    int32_t* parent; int* changed;  // the system's
    template <bool kChecked>
    __device__ __forceinline__ void four(int b, int q, int j) {
        bool hit[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hit[u] = groups_linked<kChecked>((*sx)[b][q + u], (*sy)[b][q + u], (*sr)[b][q + u], j + u, i, w.x, w.y, w.r, link, scale);
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as neighbor_pair: one add-with-carry per compare mask
        }
        if (any) {                                               // rare
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (hit[u]) groups_hook(parent, changed, i, j + u);
        }
    }
};

// grid and early exits: rows_prologue; the triangular walk: rows_walk (nbody_rows.hpp).  prev / cur: the systems' `changed`
// words of the last sweep and of this one.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void groups_sweep(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                           Counters* __restrict__ ctr_all, int stride, int n_one, double link,
                                                           double scale, int32_t* parent_all, const int* __restrict__ prev,
                                                           int* __restrict__ cur) {
    RowsLane<T, int32_t> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, parent_all, (int32_t)0)) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    if (prev[sys] == 0) return;                                  // converged in an earlier sweep: the whole workgroup
    __shared__ double sx[2][kTile], sy[2][kTile], sr[2][kTile];
    GroupsFour f{&sx, &sy, &sr, L.p, rows_row<T, true>(L, nullptr), link, scale, L.out, cur + sys};
    rows_walk<true, true>(L, RowsStage<true, T>{L.J, &sx, &sy, &sr}, f);
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
        g.h = nullptr;
        groups_free(g);
        return rows_alloc_failed(e, who, "parent and label buffers");
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call: the query's values, then the pointers.
inline int groups_check_args(const char* who, double link, double radius_scale, std::initializer_list<const void*> required) {
    if (!(link >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "%s: link = %g (a length: >= 0, +inf allowed)", who, link);
    if (!(radius_scale >= 0.0) || radius_scale == __builtin_inf())
        return nbody_fail(NBODY_ERR_INVALID, "%s: radius_scale = %g (finite and >= 0)", who, radius_scale);
    return rows_check_args(who, required, 0, 0, "");
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

// One call, from the reservation to the caller's labels; the site, Count and read_meta as for rows_run (nbody_rows.hpp).
template <typename T, typename Count, typename ReadMeta>
int groups_run(const char* who, const RowsSite& s, GroupsState& g, double link, double radius_scale, int32_t* label,
               nbody_groups_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, total = S * (size_t)s.stride;
    int sweeps = 0;
    if (s.n_bound > 0) {
        int rc = groups_reserve(g, total, S, who);
        if (rc != NBODY_OK) return rc;
        const dim3 grid = s.grid(s.n_bound), block(kDiagBlock);
        const Rec<T>* J = (const Rec<T>*)s.J;
        const int n_one = s.n_one<Count>();
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
    const int rc = s.sync<Count>(s.n_bound > 0, read_meta);
    if (rc != NBODY_OK) return rc;
    std::vector<int32_t> size;
    for (int sys = 0; sys < s.systems; ++sys) {
        const int n = s.count(sys);
        const int32_t* h = n ? reinterpret_cast<const int32_t*>(g.h) + (size_t)sys * (size_t)s.stride : nullptr;   // no staging yet
        if (n) memcpy(label + (size_t)sys * (size_t)s.stride, h, (size_t)n * sizeof(int32_t));
        groups_summarise(h, n, sweeps, size, info + sys);
    }
    return NBODY_OK;
}

}  // namespace nbk
