// csrc/nbody_batch_kernels.hpp -- gfx950 device code of the batched stepper (nbody_batch_*, include/nbody.h):
// S independent systems per launch, DESIGN.md 4.5.
//
// Layout.  Every per-system object of the one-system stepper exists S times, `stride` (= the batch's capacity) bodies
// apart: the records J, the velocities V, the staged step results S_J / S_V, and one Meta, one Counters, one
// StepParams and one slice of the event buffer per system.  A system is a rank that owns everything (lo = 0, cnt = n,
// world = 1), so there is no slot, no header and no gather: the commit compacts S_J / S_V straight into J / V.
//
// The system index is blockIdx.y of every kernel: at most 65535 systems per batch (nbody_batch_create refuses more).
#pragma once
#define NBK_TEMPLATES_ONLY          // the kernels of nbody_kernels.hpp that are not templates live in nbody_ctx.hip
#include "nbody_kernels.hpp"

#pragma clang fp contract(off)

namespace nbk {

constexpr int kBatchMaxSystems = 65535;                    // gridDim.y

// ---------------------------------------------------------------------------------------------------------
// Force + collision + drift: nbody_forces_v3.inc once more, in its 256-thread form (two 128-lane groups of ONE
// system per workgroup, four waves, see forces_v3w_f32), K lanes per body.  What differs from forces_v3w_f32 is only
// where things are: the system's Meta, parameters, records, velocities, staging, event slice and counters are found
// from blockIdx.y.  interact(), finish_body() and the text of the .inc are those of the one-system kernels, so system s
// computes what forces_v3w_f32 computes on the same bodies: literal quirks, N < 128 and the frozen tail follow from
// that system's own N.  Workgroups past a system's live count leave at once (the .inc's range test), an empty system
// (n = 0) costs exactly those.
// Registers: sized for 4 waves per SIMD (128 VGPRs) at K = 1, 2 like forces_v3w_f32<K, kLog, 4>; K = 4, 8 sit at 126 to
// 128 VGPRs already in forces_v3_f32 and spill with the per-system addressing on top, so they are sized for 3 waves
// (no scratch in any of the eight instantiations; K >= 4 is chosen when the bodies do not fill the chip anyway).
// ---------------------------------------------------------------------------------------------------------
#define NB_V3_REAL float
#define NB_V3_SIGNATURE                                                                                      \
    template <int K, bool kLog>                                                                              \
    __global__ __launch_bounds__(2 * kTile, K >= 4 ? 3 : 4) void forces_batch_f32(                           \
        const Rec<float>* __restrict__ J_all, const Vec2<float>* __restrict__ V_all,                         \
        Rec<float>* __restrict__ S_J_all, Vec2<float>* __restrict__ S_V_all, const Meta* __restrict__ meta_all, \
        const StepParams<float>* __restrict__ params, Event* ev_all, int ev_cap, Counters* ctr_all, int stride)
#define NB_V3_LDS                                                                                            \
    __shared__ Rec<T> tile_all[2][2][2 * kTile];                                                             \
    __shared__ int tile_bad_all[2][2][kTile / kWave];                                                        \
    __shared__ int tile_rnz_all[2][2][kTile / kWave];                                                        \
    Rec<T>(&tile)[2][2 * kTile] = tile_all[threadIdx.x / kTile];                                             \
    int(&tile_bad)[2][kTile / kWave] = tile_bad_all[threadIdx.x / kTile];                                    \
    int(&tile_rnz)[2][kTile / kWave] = tile_rnz_all[threadIdx.x / kTile];
#define NB_V3_LANE const int lane = threadIdx.x % kTile;
#define NB_V3_WG const int wg = blockIdx.x * 2 + threadIdx.x / kTile;
#define NB_V3_BATCH 8
#define NB_V3_CONSTANTS
#define NB_V3_RANGE                                                                                          \
    const int sys = blockIdx.y;                                                                              \
    const size_t base = (size_t)sys * (size_t)stride;                                                        \
    const int N = meta_all[sys].n, lo = 0, cnt = N, step = meta_all[sys].step;                               \
    const StepParams<float> p = params[sys];                                                                 \
    const Rec<float>* __restrict__ J = J_all + base;                                                         \
    const Vec2<float>* __restrict__ Vown = V_all + base;                                                     \
    Rec<float>* __restrict__ S_J = S_J_all + base;                                                           \
    Vec2<float>* __restrict__ S_V = S_V_all + base;                                                          \
    Event* const ev = ev_all + (size_t)sys * (size_t)ev_cap;                                                 \
    Counters* const ctr = ctr_all + sys;
#define NB_V3_REC(j) J[j]
#define NB_V3_VEL(i) Vown[i - lo]
#define NB_V3_PUT(q, i, out, vout) S_J[q] = out; S_V[q] = vout;
#define NB_V3_KEEP(q, i, a, v) S_J[q] = Rec<T>{a.xi, a.yi, a.mi, a.ri}; S_V[q] = v;
#define NB_V3_COUNT(pairs)                                                                                   \
    for (int sh = kWave / 2; sh > 0; sh >>= 1) pairs += __shfl_down(pairs, sh, kWave);                      \
    if ((lane & (kWave - 1)) == 0 && pairs) atomicAdd(&ctr->pairs, pairs);
#include "nbody_forces_v3.inc"
#undef NB_V3_REAL
#undef NB_V3_SIGNATURE
#undef NB_V3_LDS
#undef NB_V3_LANE
#undef NB_V3_WG
#undef NB_V3_BATCH
#undef NB_V3_CONSTANTS
#undef NB_V3_RANGE
#undef NB_V3_REC
#undef NB_V3_VEL
#undef NB_V3_PUT
#undef NB_V3_KEEP
#undef NB_V3_COUNT

// ---------------------------------------------------------------------------------------------------------
// Commit: stable compaction of every system on `mass != 0` (src/nbody.cu:488-510) from the staging buffers into the
// state, and the system's new Meta.  The keep test, the per-workgroup count and the offsets are those of the one-system
// compaction (compact_keep, compact_block_count, compact_offset, nbody_kernels.hpp).  grid = (nblk, S), B threads; nblk
// covers the largest uploaded count.
//   nblk == 1 : batch_commit alone counts, scatters and writes Meta (one workgroup sees the whole system).
//   nblk  > 1 : batch_count leaves the survivors per block and saves the old count in Meta::n_prev; batch_commit adds up
//               the blocks below its own, scatters, and its LAST block writes Meta.  No block of batch_commit reads
//               Meta::n or Meta::step then (the count comes from n_prev), so the in-place update is race-free.
// Meta::summary is not kept (0): the one-lane kernel builds its screens from the tiles it stages and never reads it.
// A count outside [0, stride] cannot come from these kernels; if one is found the system is emptied instead of
// indexed with, and Counters::errors of that system says so (kIndexError, as the ring kernel's index checks do).
// The check is batch_checked_count (nbody_kernels.hpp).
// ---------------------------------------------------------------------------------------------------------

template <int B>
__global__ __launch_bounds__(B) void batch_count(const Rec<float>* __restrict__ S_J_all, Meta* __restrict__ meta_all,
                                                 int* __restrict__ blk_counts, int stride) {
    const int sys = blockIdx.y;
    const int n_old = meta_all[sys].n;
    const int chk = batch_checked_count(n_old, stride);
    const int cnt = chk < 0 ? 0 : chk;
    const Rec<float>* __restrict__ S_J = S_J_all + (size_t)sys * (size_t)stride;
    const int q = blockIdx.x * B + threadIdx.x;
    const int s = compact_block_count<B>(q < cnt && compact_keep(S_J[q].m));
    if (threadIdx.x == 0) {
        blk_counts[(size_t)sys * gridDim.x + blockIdx.x] = s;
        if (blockIdx.x == 0) meta_all[sys].n_prev = n_old;   // nothing in this kernel reads n_prev
    }
}

template <int B>
__global__ __launch_bounds__(B) void batch_commit(const Rec<float>* __restrict__ S_J_all,
                                                  const Vec2<float>* __restrict__ S_V_all,
                                                  Rec<float>* __restrict__ J_all, Vec2<float>* __restrict__ V_all,
                                                  Meta* __restrict__ meta_all, const int* __restrict__ blk_counts,
                                                  Counters* __restrict__ ctr_all, int stride) {
    const int sys = blockIdx.y;
    const int nblk = gridDim.x;
    const bool single = nblk == 1;
    const int n_old = single ? meta_all[sys].n : meta_all[sys].n_prev;
    const int chk = batch_checked_count(n_old, stride);
    const int cnt = chk < 0 ? 0 : chk;
    const size_t base = (size_t)sys * (size_t)stride;
    const int q = blockIdx.x * B + threadIdx.x;
    Rec<float> rec{};
    Vec2<float> vel{};
    bool keep = false;
    if (q < cnt) {
        rec = S_J_all[base + q];
        vel = S_V_all[base + q];
        keep = compact_keep(rec.m);
    }
    // a single workgroup has none below it and reads no count
    const CompactOffset o = compact_offset<B>(keep, blk_counts + (size_t)sys * nblk);
    // The last block knows the total: the system's new Meta.  single: every thread of this (only) block has read Meta::n
    // by now (compact_offset's barriers).  nblk > 1: the other blocks read n_prev alone, which is not written here.
    if (threadIdx.x == 0 && (int)blockIdx.x == nblk - 1) {
        const int tot = o.below + o.here;
        Meta* m = meta_all + sys;
        if (single) m->n_prev = n_old;                     // nblk > 1: batch_count did, and other blocks are reading it
        m->n = tot;
        m->lo = 0;
        m->cnt = tot;
        m->step = m->step + 1;
        m->summary = 0;
        if (chk < 0) atomicAdd(&ctr_all[sys].errors, kIndexError);
    }
    if (keep) {
        J_all[base + o.off] = rec;
        V_all[base + o.off] = vel;
    }
}

}  // namespace nbk
