// csrc/nbody_tracers.hpp -- tracer particles (nbody_tracers_*, nbody_batch_tracers_*, include/nbody.h):
// massless probes {x, y, vx, vy}, always fp64, advanced once inside every step from the field of the state the step starts
// from.  A tracer is attracted by the bodies, attracts nothing, collides with nothing and is never deleted or compacted.
// Included after nbody_field.hpp by both translation units: one system (nbody_ctx.hip) and a batch (nbody_batch.hip: system
// = blockIdx.y, the same m per system) share the one kernel.
//
// The advance of one tracer (the whole contract is in include/nbody.h):
//     (ax, ay, phi, coincident) = the field at (x, y) over the n bodies of J_t: the ordered walk (diag_walk_sums,
//                                 nbody_diag.hpp) with FieldSums, then field_finish (nbody_field.hpp) with the exact walk
//                                 for a flagged tracer - called, not restated: the bits of nbody_get_field
//     dvx = dt * ax;  [walls: tx = x + (ax * dt); if (tx > hi_x || tx < lo_x) vx = vx * -1.0]
//     vx = vx + dvx;  x = x + (dt * vx)                              (y likewise; finish_body's rule with r = 0)
// every operation IEEE fp64 and rounded on its own.  The launch sits between the step's compute and its commit: J still
// holds step t (the commit overwrites it), on the same stream, enqueue-only.
//   * The count comes from the system's Meta on the device (the host does not know n_t inside nbody_step(ctx, 50)); one
//     outside [0, stride] never becomes an index - the system is treated as empty and reported as kIndexError, as
//     rows_prologue does.
//   * The prologue is the kernel's own, not rows_prologue: that one writes an "empty" record and leaves when n == 0, and a
//     tracer over an empty system must still drift (field +0, +0, +0).
//   * Workgroups past m leave before the first barrier; n is workgroup-uniform, so the walk's barriers are too.
#pragma once
#include <stddef.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_field.hpp"

#pragma clang fp contract(off)

namespace nbk {

struct alignas(16) Tracer { double x, y, vx, vy; };             // nbody_tracer
struct TracerLast { double ax, ay, phi; };                      // nbody_field: the field of the most recent advance
static_assert(sizeof(Tracer) == 32 && sizeof(nbody_tracer) == 32 && offsetof(nbody_tracer, x) == 0 &&
              offsetof(nbody_tracer, y) == 8 && offsetof(nbody_tracer, vx) == 16 && offsetof(nbody_tracer, vy) == 24,
              "nbody_tracer layout");
static_assert(sizeof(TracerLast) == sizeof(nbody_field), "nbody_field layout");
static_assert(sizeof(nbody_tracer_info) == 24, "nbody_tracer_info layout");

// StepParams<T>'s time step and walls widened to double: what the update uses.
struct TracerParams { double dt, hi_x, lo_x, hi_y, lo_y; };
template <typename T>
__host__ __device__ inline TracerParams tracer_params(const StepParams<T>& p) {
    return TracerParams{(double)p.dt, (double)p.wall_hi_x, (double)p.wall_lo_x, (double)p.wall_hi_y, (double)p.wall_lo_y};
}

// Whose tracers: a context (one system, parameters by value) or a batch (system = blockIdx.y, each system's parameters
// from the batch's device array).  Either way the count is read from Meta (RowsBatchCount).
struct TracersOne { static constexpr bool kBatch = false; };
struct TracersBatch { static constexpr bool kBatch = true; };

// grid = (ceil(m / kDiagBlock), systems), one lane per tracer.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void tracers_advance(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                              Counters* __restrict__ ctr_all, int stride, TracerParams p_one,
                                                              const StepParams<T>* __restrict__ p_all, double G, unsigned flags,
                                                              Tracer* __restrict__ tr_all, TracerLast* __restrict__ last_all,
                                                              unsigned long long* __restrict__ coin_all, int m) {
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kDiagBlock;                    // first tracer of the workgroup
    if (row0 >= m) return;
    const int chk = RowsBatchCount::checked(meta_all, sys, stride, 0);
    const int n = chk < 0 ? 0 : chk;
    if (chk < 0 && blockIdx.x == 0 && tid == 0) atomicAdd(&ctr_all[sys].errors, kIndexError);
    const int p = row0 + tid;
    const bool valid = p < m;
    const Rec<T>* __restrict__ J = J_all + (size_t)sys * (size_t)stride;
    Tracer* __restrict__ tr = tr_all + (size_t)sys * (size_t)m;
    TracerLast* __restrict__ last = last_all + (size_t)sys * (size_t)m;
    Tracer t{0.0, 0.0, 0.0, 0.0};
    if (valid) t = tr[p];
    FieldOut f{0.0, 0.0, 0.0, 0};                                // an empty system: +0 in every field
    if (n > 0) {
        __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
        FieldSums a;
        diag_walk_sums<false, false, T>(J, n, -1, t.x, t.y, -1, row0 + (tid & ~(kWave - 1)) < m, a, sx, sy, sm);
        if (valid) f = field_finish<T>(J, n, -1, t.x, t.y, a, G);
    }
    if (valid) {
        const TracerParams q = Count::kBatch ? tracer_params<T>(p_all[sys]) : p_one;
        const double dvx = q.dt * f.ax, dvy = q.dt * f.ay;
        double vx = t.vx, vy = t.vy;
        if (flags & NBODY_TRACER_WALLS) {                        // finish_body's test: ax * dt, not v
            const double tx = t.x + (f.ax * q.dt), ty = t.y + (f.ay * q.dt);
            if (tx > q.hi_x || tx < q.lo_x) vx = vx * -1.0;
            if (ty > q.hi_y || ty < q.lo_y) vy = vy * -1.0;
        }
        vx = vx + dvx;
        vy = vy + dvy;
        tr[p] = Tracer{t.x + (q.dt * vx), t.y + (q.dt * vy), vx, vy};
        last[p] = TracerLast{f.ax, f.ay, f.phi};
    }
    // one atomic per wave for the coincident count (every lane of the workgroup is here: none has returned)
    unsigned long long coin = (unsigned long long)f.coincident;
    for (int sh = kWave / 2; sh > 0; sh >>= 1) coin += __shfl_down(coin, sh, kWave);
    if ((tid & (kWave - 1)) == 0 && coin) atomicAdd(&coin_all[sys], coin);
}

// ---------------------------------------------------------------------------------------------------------
// Host side: the tracers of one context or batch.  Nothing is allocated before the first set.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kTracerFlags = NBODY_TRACER_WALLS;

struct TracerState {
    Tracer* d = nullptr;                 // [systems * m]
    TracerLast* last = nullptr;          // [systems * m]
    unsigned long long* coin = nullptr;  // [systems]: coincident sources summed over the advances since the set
    unsigned char* h = nullptr;          // pinned staging: tracers | last | coin
    int m = 0;                           // per system; 0: none set
    uint32_t flags = 0;
    int64_t steps = 0;                   // advances enqueued since the set (every system of a batch advances together)
    bool on() const { return m > 0; }
};

inline void tracers_free(TracerState& s) {
    (void)hipFree(s.d); (void)hipFree(s.last); (void)hipFree(s.coin);
    if (s.h) (void)hipHostFree(s.h);
    s = TracerState{};
}

// The argument checks of a set, before any device call.  bytes: of the caller's array, all systems.
inline int tracers_check_set(const char* who, const void* handle, const nbody_tracer* t, int m, uint32_t flags, int systems) {
    if (!handle) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL handle", who);
    if (m < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: m = %d", who, m);
    if (m > 0 && !t) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL tracers with m = %d", who, m);
    if (flags & ~kTracerFlags) return nbody_fail(NBODY_ERR_INVALID, "%s: flags 0x%x (only NBODY_TRACER_WALLS)", who, flags);
    if ((unsigned long long)m * (unsigned long long)systems * sizeof(nbody_tracer) > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d tracers in each of %d system(s) are more than 2^31 bytes", who, m, systems);
    return NBODY_OK;
}

// Replaces the tracers (m == 0: removes and frees).  Waits for the stream first: enqueued steps still use the old ones.
inline int tracers_set(const char* who, TracerState& s, hipStream_t stream, int systems, const nbody_tracer* t, int m,
                       uint32_t flags) {
    NBK_ROWS_TRY(hipStreamSynchronize(stream));
    tracers_free(s);
    if (m == 0) return NBODY_OK;
    const size_t total = (size_t)systems * (size_t)m;
    const size_t coin_bytes = (size_t)systems * sizeof(unsigned long long);
    hipError_t e = hipMalloc((void**)&s.d, total * sizeof(Tracer));
    if (e == hipSuccess) e = hipMalloc((void**)&s.last, total * sizeof(TracerLast));
    if (e == hipSuccess) e = hipMalloc((void**)&s.coin, coin_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&s.h, total * (sizeof(Tracer) + sizeof(TracerLast)) + coin_bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        s.h = nullptr;
        tracers_free(s);
        return rows_alloc_failed(e, who, "tracer buffers");
    }
    memcpy(s.h, t, total * sizeof(Tracer));
    NBK_ROWS_TRY(hipMemcpyAsync(s.d, s.h, total * sizeof(Tracer), hipMemcpyHostToDevice, stream));
    NBK_ROWS_TRY(hipMemsetAsync(s.last, 0, total * sizeof(TracerLast), stream));
    NBK_ROWS_TRY(hipMemsetAsync(s.coin, 0, coin_bytes, stream));
    NBK_ROWS_TRY(hipStreamSynchronize(stream));
    s.m = m; s.flags = flags; s.steps = 0;
    return NBODY_OK;
}

// One advance of every tracer of every system, enqueued on the owner's stream.
template <typename T, typename Count>
inline int tracers_enqueue(TracerState& s, hipStream_t stream, int systems, const Rec<T>* J, const Meta* meta, Counters* counters,
                           int stride, const TracerParams& p_one, const StepParams<T>* p_all) {
    hipLaunchKernelGGL((tracers_advance<T, Count>), dim3((s.m + kDiagBlock - 1) / kDiagBlock, systems), dim3(kDiagBlock), 0,
                       stream, J, meta, counters, stride, p_one, p_all, (double)kG, (unsigned)s.flags, s.d, s.last, s.coin, s.m);
    NBK_ROWS_TRY(hipGetLastError());
    s.steps += 1;
    return NBODY_OK;
}

// Reads the first `take` <= m tracers of every system back (out and last are `take` apart per system; last may be NULL) and
// fills info[systems].  sync: synchronises the stream and reports a device-side failure.
template <typename Sync>
inline int tracers_get(const TracerState& s, hipStream_t stream, int systems, nbody_tracer* out, nbody_field* last, int take,
                       nbody_tracer_info* info, Sync sync) {
    const size_t total = (size_t)systems * (size_t)s.m;
    unsigned char* h_tr = s.h;
    unsigned char* h_last = s.h + total * sizeof(Tracer);
    unsigned char* h_coin = h_last + total * sizeof(TracerLast);
    if (s.on()) {
        if (take > 0) {
            NBK_ROWS_TRY(hipMemcpyAsync(h_tr, s.d, total * sizeof(Tracer), hipMemcpyDeviceToHost, stream));
            if (last) NBK_ROWS_TRY(hipMemcpyAsync(h_last, s.last, total * sizeof(TracerLast), hipMemcpyDeviceToHost, stream));
        }
        NBK_ROWS_TRY(hipMemcpyAsync(h_coin, s.coin, (size_t)systems * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    }
    const int rc = sync();
    if (rc != NBODY_OK) return rc;
    for (int sys = 0; sys < systems; ++sys) {
        unsigned long long coin = 0;
        if (s.on()) {
            memcpy(&coin, h_coin + (size_t)sys * sizeof(coin), sizeof(coin));
            if (take > 0) {
                memcpy(out + (size_t)sys * take, h_tr + (size_t)sys * s.m * sizeof(Tracer), (size_t)take * sizeof(Tracer));
                if (last) memcpy(last + (size_t)sys * take, h_last + (size_t)sys * s.m * sizeof(TracerLast), (size_t)take * sizeof(TracerLast));
            }
        }
        info[sys] = nbody_tracer_info{s.on() ? s.steps : 0, (int64_t)coin, s.m, s.flags};
    }
    return NBODY_OK;
}

}  // namespace nbk
