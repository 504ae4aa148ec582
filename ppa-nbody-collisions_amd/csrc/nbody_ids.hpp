// csrc/nbody_ids.hpp -- gfx950 device code of body identities (NBODY_FLAG_TRACK_IDS, include/nbody.h):
// an index -> identity map that follows the per-step compaction, and the collision log translated through it while the
// map of the step is still valid.  Shared by the one-system stepper (nbody_ctx.hip: one system, blockIdx.y = 0) and the
// batched stepper (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride` apart, like every other batch kernel).
//
// The identity of a body is its index in the last upload.  ids_cur[i] is the identity of the body at index i of step t;
// both kernels run after the force kernel of step t and BEFORE the commit, so Meta is still that of step t, S_J holds
// the staged masses of step t and the event log holds every event of step t in the index space of step t.
//   ids_translate : lineage[k] = {ids_cur[ev[k].i], ids_cur[ev[k].j]} for the events [done, min(events, ev_cap)) -
//                   the ones logged since the last translation.  Reads `done`, never writes it.
//   ids_scatter   : ids_next[offset of q among the survivors] = ids_cur[q].  The keep test and the offset are the
//                   commit's own (compact_keep, compact_offset, nbody_kernels.hpp), so the map follows the bodies; one
//                   thread advances `done`.  Never reads `done`.
// The host swaps ids_cur and ids_next after the pair.  Every kernel here is a template: both translation units include
// this file (NBK_TEMPLATES_ONLY in nbody_batch.hip).
#pragma once
#include <vector>

#include "nbody.h"
#include "nbody_kernels.hpp"
#include "nbody_rows.hpp"

namespace nbk {

struct IdPair { int32_t id_i, id_j; };                     // one lineage record next to event k: who i and j were

constexpr int kIdsBlock = 256;                             // threads of ids_fill / ids_translate workgroups

// batch_checked_count (nbody_kernels.hpp) for the kernels that leave the report to others: the system is treated as empty.
__device__ __forceinline__ int ids_checked_count(int n, int stride) {
    const int chk = batch_checked_count(n, stride);
    return chk < 0 ? 0 : chk;
}

// Events of a log that are stored: the counter runs on past the capacity (overflow is counted, not stored).
__host__ __device__ inline unsigned long long log_stored(unsigned long long logged, int ev_cap) {
    return logged < (unsigned long long)ev_cap ? logged : (unsigned long long)ev_cap;
}

// Upload: identity = index.  grid = (ceil(stride / B), S); the whole slice is written, so no later read sees memory
// nobody wrote.
template <int B>
__global__ __launch_bounds__(B) void ids_fill(int32_t* __restrict__ ids_all, int stride) {
    const int q = blockIdx.x * B + threadIdx.x;
    if (q < stride) ids_all[(size_t)blockIdx.y * (size_t)stride + q] = q;
}

// grid = (any fixed number of workgroups, S): a grid-stride loop over the system's untranslated events.  An event index
// outside [0, n_t) is not used as an address: the record gets -1 and the system's Counters::errors gets kIndexError.
template <int B>
__global__ __launch_bounds__(B) void ids_translate(const Event* __restrict__ ev_all, int ev_cap,
                                                   Counters* __restrict__ ctr_all,
                                                   const unsigned long long* __restrict__ done_all,
                                                   const Meta* __restrict__ meta_all,
                                                   const int32_t* __restrict__ ids_cur_all, int stride,
                                                   IdPair* __restrict__ lineage_all) {
    const int sys = blockIdx.y;
    const int n = ids_checked_count(meta_all[sys].n, stride);
    const unsigned long long end = log_stored(ctr_all[sys].events, ev_cap);
    const Event* __restrict__ ev = ev_all + (size_t)sys * (size_t)ev_cap;
    IdPair* __restrict__ lineage = lineage_all + (size_t)sys * (size_t)ev_cap;
    const int32_t* __restrict__ ids = ids_cur_all + (size_t)sys * (size_t)stride;
    unsigned bad = 0;
    for (unsigned long long k = done_all[sys] + blockIdx.x * B + threadIdx.x; k < end; k += (unsigned long long)gridDim.x * B) {
        const Event e = ev[k];
        const bool ok_i = (unsigned)e.i < (unsigned)n, ok_j = (unsigned)e.j < (unsigned)n;
        lineage[k] = IdPair{ok_i ? ids[e.i] : -1, ok_j ? ids[e.j] : -1};
        bad += (ok_i ? 0u : 1u) + (ok_j ? 0u : 1u);
    }
    if (bad) atomicAdd(&ctr_all[sys].errors, kIndexError * bad);
}

// grid = (nblk, S), B threads: workgroup x of system s covers bodies [x * B, (x + 1) * B) of that system.  blk_counts
// holds the survivors of every workgroup of the same geometry (compact_count / batch_count, [s * nblk + x]); it is read
// only for workgroups above the first, so a system that fits one workgroup counts by itself.  done_all == NULL: the
// context keeps no event log.
template <typename T, int B>
__global__ __launch_bounds__(B) void ids_scatter(const Rec<T>* __restrict__ S_J_all, const Meta* __restrict__ meta_all,
                                                 const int* __restrict__ blk_counts,
                                                 const int32_t* __restrict__ ids_cur_all,
                                                 int32_t* __restrict__ ids_next_all, int stride,
                                                 const Counters* __restrict__ ctr_all,
                                                 unsigned long long* __restrict__ done_all, int ev_cap) {
    const int sys = blockIdx.y;
    const int cnt = ids_checked_count(meta_all[sys].n, stride);
    const size_t base = (size_t)sys * (size_t)stride;
    const int q = blockIdx.x * B + threadIdx.x;
    int32_t id = 0;
    bool keep = false;
    if (q < cnt) {
        id = ids_cur_all[base + q];
        keep = compact_keep(S_J_all[base + q].m);
    }
    const CompactOffset o = compact_offset<B>(keep, blk_counts + (size_t)sys * gridDim.x);
    if (keep) ids_next_all[base + o.off] = id;             // off < survivors <= cnt <= stride
    if (q == 0 && done_all != nullptr)                     // everything logged so far is translated (ids_translate, before)
        done_all[sys] = log_stored(ctr_all[sys].events, ev_cap);
}

// ---------------------------------------------------------------------------------------------------------
// Host side shared by the two steppers: the device state of one context or batch, and the launches.
// Both translation units name these templates in functions at the END of the file (declared further up): the compiler
// emits kernels in the order the host code first names them, so the kernels of this file come after every kernel that
// existed before and those keep their place, and their label numbers, in the assembly of `make asm`.
// ---------------------------------------------------------------------------------------------------------
struct IdsState {
    int32_t* map[2] = {nullptr, nullptr};   // [systems * stride] each; map[cur][s * stride + i] = identity of system s's body i
    int cur = 0;                            // swapped by the host after every step's ids_scatter
    IdPair* lineage = nullptr;              // [systems * ev_cap], next to the event buffer (with NBODY_FLAG_RECORD_EVENTS)
    unsigned long long* done = nullptr;     // [systems] events translated so far
    bool on() const { return map[0] != nullptr; }
    const int32_t* current() const { return map[cur]; }
};

// Create with NBODY_FLAG_TRACK_IDS: the two maps, and for a handle that logs `events` (> 0) events per system the lineage
// and the cleared counters.  A failure leaves what was made to ids_free.
inline hipError_t ids_alloc(IdsState& st, hipStream_t stream, size_t systems, size_t stride, size_t events) {
    hipError_t e = hipMalloc((void**)&st.map[0], systems * stride * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&st.map[1], systems * stride * sizeof(int32_t));
    if (e != hipSuccess || events == 0) return e;
    e = hipMalloc((void**)&st.lineage, systems * events * sizeof(IdPair));
    if (e == hipSuccess) e = hipMalloc((void**)&st.done, systems * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(st.done, 0, systems * sizeof(unsigned long long), stream);
    return e;
}

inline void ids_free(IdsState& st) {
    (void)hipFree(st.map[0]); (void)hipFree(st.map[1]); (void)hipFree(st.lineage); (void)hipFree(st.done);
    st = IdsState{};
}

// The lineage starts empty with the event log: an upload, nbody_clear_events.
inline hipError_t ids_clear_done(IdsState& st, hipStream_t stream, size_t systems) {
    return st.done ? hipMemsetAsync(st.done, 0, systems * sizeof(unsigned long long), stream) : hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------
// Reading back (nbody_get_events / _ids / _lineage and their batch twins), from where the handle knows its count: a context
// has read its one Meta and Counters, a batch those of every system.  The pointers are one system's slices.
// ---------------------------------------------------------------------------------------------------------
// The first min(total, ev_cap, cap) records of a log: what was stored and fits the caller's buffer.
static_assert(sizeof(nbody_event) == sizeof(Event), "event layouts must match");
inline unsigned long long log_prefix(unsigned long long total, int ev_cap, int cap) {
    const unsigned long long stored = log_stored(total, ev_cap);
    return stored < (unsigned long long)cap ? stored : (unsigned long long)cap;
}

inline int events_read(const Event* ev_dev, unsigned long long logged, int ev_cap, nbody_event* out, int cap, int64_t* total) {
    *total = (int64_t)logged;
    const unsigned long long ncopy = log_prefix(logged, ev_cap, cap);
    if (ncopy) NBK_ROWS_TRY(hipMemcpy(out, ev_dev, ncopy * sizeof(Event), hipMemcpyDeviceToHost));
    return NBODY_OK;
}

// n: the system's count as Meta has it; it is checked against the stride before it sizes the copy.
inline int ids_read(const char* who, const int32_t* map_dev, int n, int stride, int32_t* ids, int cap, int* n_out) {
    if (n < 0 || n > stride) return nbody_fail(NBODY_ERR_STATE, "%s: %d bodies, capacity %d", who, n, stride);
    const int k = n < cap ? n : cap;
    if (k > 0) NBK_ROWS_TRY(hipMemcpy(ids, map_dev, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost));
    *n_out = n;
    return NBODY_OK;
}

// An event past `done` belongs to no committed step and has not been translated: it reads -1.
inline int lineage_read(const Event* ev_dev, const IdPair* who_dev, const unsigned long long* done_dev, unsigned long long logged,
                        int ev_cap, nbody_lineage* out, int cap, int64_t* total) {
    *total = (int64_t)logged;
    const unsigned long long ncopy = log_prefix(logged, ev_cap, cap);
    if (ncopy == 0) return NBODY_OK;
    unsigned long long done = 0;
    std::vector<Event> ev((size_t)ncopy);
    std::vector<IdPair> who((size_t)ncopy);
    NBK_ROWS_TRY(hipMemcpy(&done, done_dev, sizeof(done), hipMemcpyDeviceToHost));
    NBK_ROWS_TRY(hipMemcpy(ev.data(), ev_dev, ncopy * sizeof(Event), hipMemcpyDeviceToHost));
    NBK_ROWS_TRY(hipMemcpy(who.data(), who_dev, ncopy * sizeof(IdPair), hipMemcpyDeviceToHost));
    for (unsigned long long k = 0; k < ncopy; ++k) {
        const bool have = k < done;
        out[k] = nbody_lineage{ev[k].step, have ? who[k].id_i : -1, have ? who[k].id_j : -1, ev[k].kind};
    }
    return NBODY_OK;
}

// Upload: identity = index, for every system; the caller empties `done` with the event counters.
template <int B>
void ids_enqueue_fill(IdsState& st, hipStream_t stream, int systems, int stride) {
    st.cur = 0;
    hipLaunchKernelGGL((ids_fill<B>), dim3((stride + B - 1) / B, systems), dim3(B), 0, stream, st.map[0], stride);
}

// One step: after the force kernel (and the per-workgroup count, where there is more than one workgroup per system) and
// before the commit.  nblk workgroups of B threads per system, the geometry of the count that filled blk_counts.
template <typename T, int B>
void ids_enqueue_step(IdsState& st, hipStream_t stream, int nblk, int systems, int translate_grid, const Rec<T>* S_J,
                      const Meta* meta, const int* blk_counts, int stride, Counters* ctr, const Event* ev, int ev_cap) {
    if (st.lineage)
        hipLaunchKernelGGL((ids_translate<kIdsBlock>), dim3(translate_grid, systems), dim3(kIdsBlock), 0, stream, ev, ev_cap,
                           ctr, (const unsigned long long*)st.done, meta, (const int32_t*)st.map[st.cur], stride, st.lineage);
    hipLaunchKernelGGL((ids_scatter<T, B>), dim3(nblk, systems), dim3(B), 0, stream, S_J, meta, blk_counts,
                       (const int32_t*)st.map[st.cur], st.map[st.cur ^ 1], stride, (const Counters*)ctr,
                       st.lineage ? st.done : nullptr, ev_cap);
    st.cur ^= 1;
}

}  // namespace nbk
