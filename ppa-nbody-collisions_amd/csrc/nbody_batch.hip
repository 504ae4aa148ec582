// csrc/nbody_batch.hip -- host side of the batched stepper (nbody_batch_*, include/nbody.h).
//
// S independent systems share every launch: per ensemble step one force launch and one commit launch (two when a
// system does not fit one commit workgroup), whatever S is, and nothing else - no device-to-host copy, no host wait.
// Grids are sized from the uploaded counts.  A system's body count only shrinks (bodies are deleted, never made), so
// the grid of the upload covers every later step; each kernel takes the exact count from the system's device-side Meta
// and workgroups past it exit at once (the argument of launch_compute in nbody_ctx.hip, without its refresh of the
// bound: a batch is small systems, the idle workgroups cost less than a host wait would).
// Diagnostics of every system (nbody_batch_diagnostics) and the recorded series (nbody_batch_diag_*) are two launches per
// call or record on the same stream, sized the same way; a record is enqueue-only like a step (nbody_batch_diag.hpp).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_batch_kernels.hpp"
#include "nbody_batch_diag.hpp"
#include "nbody_queries.hpp"

using namespace nbk;

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return nbody_fail(NBODY_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),      \
                              __FILE__, __LINE__);                                                        \
    } while (0)

struct nbody_batch {
    nbody_batch_desc desc{};
    int S = 0;                  // systems
    int cap = 0;                // bodies per system = distance between two systems in every per-body array
    int ev_cap = 0;             // events per system (0: not recorded)
    int K = 1;                  // lanes per body of the force kernel
    int num_cus = 256;
    hipStream_t stream = nullptr;
    RowsOwned own;              // every device and pinned block made at create
    // device memory
    Rec<float>* J = nullptr;            // [S * cap]
    Vec2<float>* V = nullptr;           // [S * cap]
    Rec<float>* S_J = nullptr;          // [S * cap] staged step results, step-t index space
    Vec2<float>* S_V = nullptr;
    Meta* meta = nullptr;               // [S]
    Counters* counters = nullptr;       // [S]
    StepParams<float>* params = nullptr;   // [S]
    Event* events = nullptr;            // [S * ev_cap]
    int* blk_counts = nullptr;          // [S * ceil(cap / 1024)]
    // host
    Meta* h_meta = nullptr;             // pinned [S]
    Counters* h_counters = nullptr;     // pinned [S]
    unsigned char* h_stage = nullptr;   // upload: records then velocities of all systems; download: one system
    size_t h_stage_bytes = 0;
    int n_upper = 0;                    // largest uploaded count: sizes every grid until the next upload
    bool uploaded = false;
    int64_t steps = 0;
    // diagnostics (nbody_batch_diagnostics, nbody_batch_diag_*): nothing is allocated until one of them is called
    RowsArray<DiagTile> dg_tiles;       // device [S * ceil(cap / 128)] tile partials, first diagnostics call of any kind
    RowsArray<DiagOut> dg_out;          // [S] records of one nbody_batch_diagnostics call: device and pinned
    RowsArray<double> dg_phi;           // [S * cap], first call that asks for phi: device and pinned
    RowsArray<DiagOut> dg_log;          // device [log_cap * S] recorded series (nbody_batch_diag_reserve)
    int log_cap = 0;                    // samples reserved
    int log_rows = 0;                   // samples recorded since the reservation or the last upload: the next row
    // identities (NBODY_FLAG_TRACK_IDS, nbody_ids.hpp): nothing is allocated without the flag
    IdsState ids;                       // the map [S * cap] twice, the lineage [S * ev_cap], [S] translated-up-to counters
    // track log (nbody_batch_track_*, nbody_tracks.hpp): nothing is allocated without a reservation
    TrackState trk;
    // the queries (nbody_queries.hpp): nothing is allocated before the first call of each
    QueryStates q;
};

namespace {

constexpr int kCommitSmall = 256, kCommitLarge = 1024;     // threads of a commit workgroup
// Identities (NBODY_FLAG_TRACK_IDS), defined at the end of this file (see nbody_ids.hpp for why there).
void ids_step(nbody_batch* b, int nblk, int threads);   // before the commit; the commit's geometry
int ids_restart(nbody_batch* b);                        // nbody_batch_upload

void free_all(nbody_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->desc.device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    b->own.release();
    ids_free(b->ids);
    track_free(b->trk);
    queries_free(b->q);
    rows_free(b->dg_tiles); rows_free(b->dg_out); rows_free(b->dg_phi); rows_free(b->dg_log);
    free(b->h_stage);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    (void)hipGetLastError();
    delete b;
}

// Lanes per body when the caller leaves it to the library, from the most the batch can hold (S x capacity bodies): K
// doubles until S x capacity x K reaches 512 lanes per CU (two waves per SIMD) or K = 4.  Measured on an MI355X (256
// CUs: 131072 lanes), S systems of N = 1024, stock configuration, us per ensemble step for K = 1 / 2 / 4 / 8
// (csrc/tune/batch_probe.py --variants, profiles/batch_probe.txt):
//     S =  16 ( 16384 bodies):  48.5 /  40.5 /  39.3 /  54.7   -> 4
//     S =  64 ( 65536 bodies):  63.0 /  60.9 / 102.6 / 224.8   -> 2
//     S = 128 (131072 bodies):  76.6 /  93.7 / 218.1 / 432.2   -> 1
//     S = 256 (262144 bodies): 127.2 / 220.6 / 444.1 / 847.3   -> 1
// K = 8 won nowhere and is left to kernel_variant; batches of fewer than 16384 bodies have not been measured.
int automatic_lanes(long long bodies, int num_cus) {
    const long long fill = (long long)num_cus * 512;
    int K = 1;
    while (K < 4 && bodies * K < fill) K *= 2;
    return K;
}

template <int K>
void launch_forces_k(nbody_batch* b, int nblocks, bool log) {
    const dim3 grid((nblocks * K + 1) / 2, b->S);          // two 128-lane groups of one system per workgroup
#define NB_BATCH_ARGS b->J, b->V, b->S_J, b->S_V, (const Meta*)b->meta, (const StepParams<float>*)b->params, \
                      b->events, b->ev_cap, b->counters, b->cap
    if (log) hipLaunchKernelGGL((forces_batch_f32<K, true>), grid, dim3(2 * kTile), 0, b->stream, NB_BATCH_ARGS);
    else hipLaunchKernelGGL((forces_batch_f32<K, false>), grid, dim3(2 * kTile), 0, b->stream, NB_BATCH_ARGS);
#undef NB_BATCH_ARGS
}

template <int B>
void launch_commit_b(nbody_batch* b, int nblk) {
    const dim3 grid(nblk, b->S);
    if (nblk > 1)
        hipLaunchKernelGGL((batch_count<B>), grid, dim3(B), 0, b->stream, (const Rec<float>*)b->S_J, b->meta,
                           b->blk_counts, b->cap);
    // identities: before the commit, where Meta::n and the map are still those of step t and S_J is staged; the events of
    // this step go through the map of this step, then the map follows the compaction (batch_count's partials above one
    // workgroup per system, its own count otherwise)
    if (b->ids.on()) ids_step(b, nblk, B);
    hipLaunchKernelGGL((batch_commit<B>), grid, dim3(B), 0, b->stream, (const Rec<float>*)b->S_J,
                       (const Vec2<float>*)b->S_V, b->J, b->V, b->meta, (const int*)b->blk_counts, b->counters, b->cap);
}

// One ensemble step: 2 launches when the largest uploaded system fits one commit workgroup (1024 bodies), 3 otherwise.
int enqueue_step(nbody_batch* b) {
    const int n = b->n_upper;
    const int nblocks = (n + kTile - 1) / kTile > 0 ? (n + kTile - 1) / kTile : 1;   // reference blocks, frozen tail included
    const bool log = b->ev_cap > 0;
    switch (b->K) {
        case 1: launch_forces_k<1>(b, nblocks, log); break;
        case 2: launch_forces_k<2>(b, nblocks, log); break;
        case 4: launch_forces_k<4>(b, nblocks, log); break;
        default: launch_forces_k<8>(b, nblocks, log); break;
    }
    if (b->q.trc.on()) {                                   // tracers: J still holds step t until the commit
        const int rc = tracers_enqueue<float, TracersBatch>(b->q.trc, b->stream, b->S, (const Rec<float>*)b->J, (const Meta*)b->meta,
                                                            b->counters, b->cap, TracerParams{}, (const StepParams<float>*)b->params);
        if (rc != NBODY_OK) return rc;
    }
    if (n <= kCommitSmall) launch_commit_b<kCommitSmall>(b, 1);
    else launch_commit_b<kCommitLarge>(b, (n + kCommitLarge - 1) / kCommitLarge);
    HIP_TRY(hipGetLastError());
    return NBODY_OK;
}

// Synchronises and refreshes the host copies of every system's Meta and Counters; a device-side failure of any system
// is reported here, with the system's number.
int read_meta(nbody_batch* b) {
    HIP_TRY(hipMemcpyAsync(b->h_meta, b->meta, sizeof(Meta) * (size_t)b->S, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(b->h_counters, b->counters, sizeof(Counters) * (size_t)b->S, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int s = 0; s < b->S; ++s)
        if (b->h_counters[s].errors != 0)
            return nbody_fail(NBODY_ERR_HIP, "system %d of the batch: device reported %llu failed index check(s) (the system "
                                             "was emptied instead of indexed with a bad count): upload again",
                              s, b->h_counters[s].errors / kIndexError);
    return NBODY_OK;
}

int check_system(const nbody_batch* b, int system, const char* who) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL batch", who);
    if (system < 0 || system >= b->S)
        return nbody_fail(NBODY_ERR_INVALID, "%s: system %d out of range (the batch has %d)", who, system, b->S);
    return NBODY_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Diagnostics (kernels in nbody_batch_diag.hpp)
// ---------------------------------------------------------------------------------------------------------
// The tile partials: S * ceil(cap / 128) records, cleared once so that no later read sees memory nobody wrote.
int diag_alloc_tiles(nbody_batch* b) {
    if (b->dg_tiles.d) return NBODY_OK;
    const size_t tiles = (size_t)b->S * (size_t)batch_diag_tiles(b->cap);
    const hipError_t e = rows_reserve_device(b->dg_tiles, tiles);
    if (e != hipSuccess) return rows_alloc_failed(e, "batch diagnostics", "tile partials");
    HIP_TRY(hipMemsetAsync(b->dg_tiles.d, 0, tiles * sizeof(DiagTile), b->stream));
    return NBODY_OK;
}

// The two launches of one sample of every system: rows of `out` are S records; phi may be NULL.
int enqueue_diagnostics(nbody_batch* b, DiagOut* out, double* phi) {
    const double G = (double)kG;
    if (b->n_upper > 0) {
        const dim3 grid((b->n_upper + kDiagBlock - 1) / kDiagBlock, b->S);
        if (phi)
            hipLaunchKernelGGL((batch_diag_potential<true>), grid, dim3(kDiagBlock), 0, b->stream, (const Rec<float>*)b->J,
                               (const Vec2<float>*)b->V, (const Meta*)b->meta, b->cap, G, phi, b->dg_tiles.d);
        else
            hipLaunchKernelGGL((batch_diag_potential<false>), grid, dim3(kDiagBlock), 0, b->stream, (const Rec<float>*)b->J,
                               (const Vec2<float>*)b->V, (const Meta*)b->meta, b->cap, G, (double*)nullptr, b->dg_tiles.d);
    }
    hipLaunchKernelGGL((batch_diag_reduce<kWave>), dim3((b->S + kWave - 1) / kWave), dim3(kWave), 0, b->stream,
                       (const DiagTile*)b->dg_tiles.d, (const Meta*)b->meta, b->counters, b->S, b->cap, out);
    HIP_TRY(hipGetLastError());
    return NBODY_OK;
}

}  // namespace

extern "C" {

int nbody_batch_create(nbody_batch** out, const nbody_batch_desc* d, const nbody_batch_params* params) {
    if (!out || !d) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: NULL argument");
    *out = nullptr;
    if (!params) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: NULL params (one nbody_batch_params per system)");
    if (d->systems < 1 || d->systems > kBatchMaxSystems)
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: %d systems (1..%d: the system index is gridDim.y)",
                          d->systems, kBatchMaxSystems);
    if (d->capacity < 1) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: capacity %d per system", d->capacity);
    if ((long long)d->systems * d->capacity > (1ll << 28))
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: %d systems x %d bodies is more than 2^28 bodies",
                          d->systems, d->capacity);
    if (d->precision == NBODY_F64)
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: fp64 batches are not implemented (NBODY_F32 only); "
                                             "step fp64 systems with one nbody_ctx each");
    if (d->precision != NBODY_F32) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: bad precision");
    if (d->semantics != NBODY_LITERAL && d->semantics != NBODY_CLEAN)
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: bad semantics");
    if (d->flags & ~(uint32_t)(NBODY_FLAG_RECORD_EVENTS | NBODY_FLAG_TRACK_IDS))
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: flags 0x%x (only NBODY_FLAG_RECORD_EVENTS and "
                                             "NBODY_FLAG_TRACK_IDS: a batch has no exchange)", d->flags);
    if (d->event_capacity < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: negative event_capacity");
    if (d->kernel_variant != 0 && d->kernel_variant != 1 && d->kernel_variant != 2 && d->kernel_variant != 4 &&
        d->kernel_variant != 8)
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_create: kernel_variant %d (0 automatic, or 1, 2, 4, 8 lanes "
                                             "per body)", d->kernel_variant);
    const bool log = (d->flags & NBODY_FLAG_RECORD_EVENTS) != 0;
    // default event slice: 2^24 events over the whole batch, at least 1024 and at most 2^20 per system
    int ev_cap = 0;
    if (log) {
        ev_cap = d->event_capacity;
        if (ev_cap == 0) {
            ev_cap = (1 << 24) / d->systems;
            if (ev_cap < 1024) ev_cap = 1024;
            if (ev_cap > (1 << 20)) ev_cap = 1 << 20;
        }
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return nbody_fail(NBODY_ERR_NO_DEVICE, "no HIP device visible (%s); this library has no CPU path",
                          e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (d->device < 0 || d->device >= ndev)
        return nbody_fail(NBODY_ERR_INVALID, "device ordinal %d out of range (0..%d)", d->device, ndev - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, d->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return nbody_fail(NBODY_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 only", d->device,
                          prop.gcnArchName);
    HIP_TRY(hipSetDevice(d->device));

    nbody_batch* b = new (std::nothrow) nbody_batch();
    if (!b) return nbody_fail(NBODY_ERR_NOMEM, "nbody_batch_create: out of host memory");
    b->desc = *d;
    b->S = d->systems;
    b->cap = d->capacity;
    b->ev_cap = ev_cap;
    b->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    b->K = d->kernel_variant ? d->kernel_variant : automatic_lanes((long long)b->S * b->cap, b->num_cus);
    const size_t bodies = (size_t)b->S * (size_t)b->cap;

#define BATCH_TRY(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) {                                                                          \
            int rc__ = rows_alloc_failed(e__, "nbody_batch_create", #expr);                               \
            free_all(b);                                                                                  \
            return rc__;                                                                                  \
        }                                                                                                 \
    } while (0)
    BATCH_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    BATCH_TRY(b->own.device(&b->J, bodies * sizeof(Rec<float>)));
    BATCH_TRY(b->own.device(&b->V, bodies * sizeof(Vec2<float>)));
    BATCH_TRY(b->own.device(&b->S_J, bodies * sizeof(Rec<float>)));
    BATCH_TRY(b->own.device(&b->S_V, bodies * sizeof(Vec2<float>)));
    BATCH_TRY(b->own.device(&b->meta, sizeof(Meta) * (size_t)b->S));
    BATCH_TRY(b->own.device(&b->counters, sizeof(Counters) * (size_t)b->S));
    BATCH_TRY(b->own.device(&b->params, sizeof(StepParams<float>) * (size_t)b->S));
    BATCH_TRY(b->own.device(&b->blk_counts, sizeof(int) * (size_t)b->S * (size_t)(b->cap / kCommitLarge + 1)));
    if (log) BATCH_TRY(b->own.device(&b->events, sizeof(Event) * (size_t)b->S * (size_t)ev_cap));
    if (d->flags & NBODY_FLAG_TRACK_IDS) BATCH_TRY(ids_alloc(b->ids, b->stream, (size_t)b->S, (size_t)b->cap, (size_t)ev_cap));
    BATCH_TRY(b->own.host(&b->h_meta, sizeof(Meta) * (size_t)b->S));
    BATCH_TRY(b->own.host(&b->h_counters, sizeof(Counters) * (size_t)b->S));
    memset(b->h_meta, 0, sizeof(Meta) * (size_t)b->S);
    memset(b->h_counters, 0, sizeof(Counters) * (size_t)b->S);
    b->h_stage_bytes = bodies * (sizeof(Rec<float>) + sizeof(Vec2<float>));
    if (b->h_stage_bytes < sizeof(StepParams<float>) * (size_t)b->S) b->h_stage_bytes = sizeof(StepParams<float>) * (size_t)b->S;
    b->h_stage = (unsigned char*)malloc(b->h_stage_bytes);
    if (!b->h_stage) {
        const size_t wanted = b->h_stage_bytes;
        free_all(b);
        return nbody_fail(NBODY_ERR_NOMEM, "nbody_batch_create: out of host memory (%zu bytes of staging)", wanted);
    }
    {   // once per system; the hand-off limit is the ring kernel's and a batch has none
        StepParams<float>* hp = reinterpret_cast<StepParams<float>*>(b->h_stage);
        for (int s = 0; s < b->S; ++s)
            hp[s] = make_params<float>(params[s].timestep, params[s].growthRate, params[s].fieldWidth, params[s].fieldHeight,
                                       d->semantics, 0);
        BATCH_TRY(hipMemcpyAsync(b->params, hp, sizeof(StepParams<float>) * (size_t)b->S, hipMemcpyHostToDevice, b->stream));
    }
    BATCH_TRY(hipMemsetAsync(b->meta, 0, sizeof(Meta) * (size_t)b->S, b->stream));
    BATCH_TRY(hipMemsetAsync(b->counters, 0, sizeof(Counters) * (size_t)b->S, b->stream));
    BATCH_TRY(hipStreamSynchronize(b->stream));
#undef BATCH_TRY
    *out = b;
    return NBODY_OK;
}

int nbody_batch_destroy(nbody_batch* b) {
    free_all(b);
    return NBODY_OK;
}

int nbody_batch_upload(nbody_batch* b, const void* const* blocks, const int* counts) {
    if (!b || !blocks || !counts) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_upload: NULL argument");
    for (int s = 0; s < b->S; ++s) {
        if (counts[s] < 0 || counts[s] > b->cap)
            return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_upload: system %d has %d bodies (0..capacity %d)", s,
                              counts[s], b->cap);
        if (!blocks[s]) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_upload: system %d has no block", s);
    }
    HIP_TRY(hipSetDevice(b->desc.device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    // pack every [P|V|M|R] block (src/nbody.cu:66-77) into {x,y,m,r} records and velocities, `cap` apart
    const size_t bodies = (size_t)b->S * (size_t)b->cap;
    Rec<float>* st = reinterpret_cast<Rec<float>*>(b->h_stage);
    Vec2<float>* sv = reinterpret_cast<Vec2<float>*>(b->h_stage + bodies * sizeof(Rec<float>));
    int n_upper = 0;
    for (int s = 0; s < b->S; ++s) {
        const int n = counts[s];
        Rec<float>* r = st + (size_t)s * b->cap;
        Vec2<float>* v = sv + (size_t)s * b->cap;
        nbody_block_pack(blocks[s], n, NBODY_F32, r, v, nullptr, 0);   // no batch kernel looks at a summary: it stays 0
        if (n < b->cap) {                                  // never read; defined all the same
            memset(r + n, 0, (size_t)(b->cap - n) * sizeof(Rec<float>));
            memset(v + n, 0, (size_t)(b->cap - n) * sizeof(Vec2<float>));
        }
        b->h_meta[s] = meta_at_upload(n, 0, n, 0);
        if (n > n_upper) n_upper = n;
    }
    HIP_TRY(hipMemcpyAsync(b->J, st, bodies * sizeof(Rec<float>), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->V, sv, bodies * sizeof(Vec2<float>), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->meta, b->h_meta, sizeof(Meta) * (size_t)b->S, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(b->counters, 0, sizeof(Counters) * (size_t)b->S, b->stream));   // pairs, events, errors
    if (b->ids.on()) {                                     // identity = index of this upload; both logs start empty
        int ri = ids_restart(b);
        if (ri != NBODY_OK) return ri;
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    memset(b->h_counters, 0, sizeof(Counters) * (size_t)b->S);
    b->n_upper = n_upper;
    b->uploaded = true;
    b->steps = 0;
    b->log_rows = 0;                                       // the recorded series restarts, the reservation stays
    b->trk.recorded = 0;                                   // and so does the track log
    return NBODY_OK;
}

int nbody_batch_step(nbody_batch* b, int nsteps) {
    if (!b || nsteps < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_step: bad argument");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_step before nbody_batch_upload");
    HIP_TRY(hipSetDevice(b->desc.device));
    for (int s = 0; s < nsteps; ++s) {
        int rc = enqueue_step(b);
        if (rc != NBODY_OK) return rc;
        b->steps += 1;
    }
    return NBODY_OK;
}

int nbody_batch_sync(nbody_batch* b) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_sync: NULL batch");
    HIP_TRY(hipSetDevice(b->desc.device));
    HIP_TRY(hipGetLastError());
    return read_meta(b);
}

int nbody_batch_counts(nbody_batch* b, int* counts) {
    if (!b || !counts) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_counts: NULL argument");
    HIP_TRY(hipSetDevice(b->desc.device));
    int rc = read_meta(b);
    if (rc != NBODY_OK) return rc;
    for (int s = 0; s < b->S; ++s) counts[s] = b->h_meta[s].n;
    return NBODY_OK;
}

int nbody_batch_download(nbody_batch* b, int system, void* block, int* n_out) {
    int rc = check_system(b, system, "nbody_batch_download");
    if (rc != NBODY_OK) return rc;
    if (!block || !n_out) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_download: NULL argument");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_download before nbody_batch_upload");
    HIP_TRY(hipSetDevice(b->desc.device));
    rc = read_meta(b);
    if (rc != NBODY_OK) return rc;
    const int n = b->h_meta[system].n;
    if (n < 0 || n > b->cap) return nbody_fail(NBODY_ERR_STATE, "system %d reports %d bodies, capacity %d", system, n, b->cap);
    Rec<float>* st = reinterpret_cast<Rec<float>*>(b->h_stage);
    Vec2<float>* sv = reinterpret_cast<Vec2<float>*>(b->h_stage + (size_t)b->cap * sizeof(Rec<float>));
    const size_t base = (size_t)system * (size_t)b->cap;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(st, b->J + base, (size_t)n * sizeof(Rec<float>), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(sv, b->V + base, (size_t)n * sizeof(Vec2<float>), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    nbody_block_unpack(block, n, NBODY_F32, st, sv);       // the survivors' re-carved block, src/nbody.cu:496-510
    *n_out = n;
    return NBODY_OK;
}

int nbody_batch_get_events(nbody_batch* b, int system, nbody_event* out, int cap, int64_t* total) {
    int rc = check_system(b, system, "nbody_batch_get_events");
    if (rc != NBODY_OK) return rc;
    if (!total || cap < 0 || (cap > 0 && !out)) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_get_events: bad argument");
    HIP_TRY(hipSetDevice(b->desc.device));
    rc = read_meta(b);
    if (rc != NBODY_OK) return rc;
    return events_read(b->events + (size_t)system * (size_t)b->ev_cap, b->h_counters[system].events, b->ev_cap, out, cap, total);
}

int nbody_batch_get_ids(nbody_batch* b, int system, int32_t* ids, int cap, int* n_out) {
    int rc = check_system(b, system, "nbody_batch_get_ids");
    if (rc != NBODY_OK) return rc;
    if (!n_out || cap < 0 || (cap > 0 && !ids)) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_get_ids: bad argument");
    if (!b->ids.on()) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_get_ids: the batch was created without NBODY_FLAG_TRACK_IDS");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_get_ids before nbody_batch_upload");
    HIP_TRY(hipSetDevice(b->desc.device));
    rc = read_meta(b);
    if (rc != NBODY_OK) return rc;
    return ids_read("nbody_batch_get_ids", b->ids.current() + (size_t)system * (size_t)b->cap, b->h_meta[system].n, b->cap, ids, cap,
                    n_out);
}

int nbody_batch_get_lineage(nbody_batch* b, int system, nbody_lineage* out, int cap, int64_t* total) {
    int rc = check_system(b, system, "nbody_batch_get_lineage");
    if (rc != NBODY_OK) return rc;
    if (!total || cap < 0 || (cap > 0 && !out)) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_get_lineage: bad argument");
    if (!b->ids.on()) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_get_lineage: the batch was created without NBODY_FLAG_TRACK_IDS");
    if (!b->ids.lineage) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_get_lineage: the batch was created without NBODY_FLAG_RECORD_EVENTS");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_get_lineage before nbody_batch_upload");
    HIP_TRY(hipSetDevice(b->desc.device));
    rc = read_meta(b);                                     // synchronises; a failed index check of a translation ends here
    if (rc != NBODY_OK) return rc;
    const size_t first = (size_t)system * (size_t)b->ev_cap;
    return lineage_read(b->events + first, b->ids.lineage + first, b->ids.done + system, b->h_counters[system].events, b->ev_cap, out,
                        cap, total);
}

int nbody_batch_get_stats(nbody_batch* b, int system, nbody_stats* out) {
    int rc = check_system(b, system, "nbody_batch_get_stats");
    if (rc != NBODY_OK) return rc;
    if (!out) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_get_stats: NULL");
    HIP_TRY(hipSetDevice(b->desc.device));
    rc = read_meta(b);
    if (rc != NBODY_OK) return rc;
    memset(out, 0, sizeof(*out));
    out->steps = b->steps;
    out->pairs = (int64_t)b->h_counters[system].pairs;
    out->n_bodies = b->h_meta[system].n;
    return NBODY_OK;
}

int nbody_batch_diagnostics(nbody_batch* b, nbody_diag* out, double* phi) {
    if (!b || !out) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diagnostics: NULL argument");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_diagnostics before nbody_batch_upload");
    HIP_TRY(hipSetDevice(b->desc.device));
    int rc = diag_alloc_tiles(b);
    if (rc != NBODY_OK) return rc;
    const size_t bodies = (size_t)b->S * (size_t)b->cap;
    hipError_t e = rows_reserve(b->dg_out, (size_t)b->S);
    if (e != hipSuccess) return rows_alloc_failed(e, "batch diagnostics", "output records");
    if (phi && (e = rows_reserve(b->dg_phi, bodies)) != hipSuccess) return rows_alloc_failed(e, "batch diagnostics", "potential buffer");
    rc = enqueue_diagnostics(b, b->dg_out.d, phi ? b->dg_phi.d : nullptr);
    if (rc != NBODY_OK) return rc;
    HIP_TRY(hipMemcpyAsync(b->dg_out.h, b->dg_out.d, sizeof(DiagOut) * (size_t)b->S, hipMemcpyDeviceToHost, b->stream));
    if (phi) HIP_TRY(hipMemcpyAsync(b->dg_phi.h, b->dg_phi.d, bodies * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    rc = read_meta(b);                                     // synchronises; a system whose count failed its check ends here
    if (rc != NBODY_OK) return rc;
    const DiagOut* h_out = reinterpret_cast<const DiagOut*>(b->dg_out.h);
    const double* h_phi = reinterpret_cast<const double*>(b->dg_phi.h);
    memcpy(out, h_out, sizeof(DiagOut) * (size_t)b->S);
    if (phi)
        for (int s = 0; s < b->S; ++s) {
            const long long n = h_out[s].n_bodies;         // what the kernels used: 0..cap
            if (n > 0) memcpy(phi + (size_t)s * b->cap, h_phi + (size_t)s * b->cap, (size_t)n * sizeof(double));
        }
    return NBODY_OK;
}

int nbody_batch_diag_reserve(nbody_batch* b, int samples) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_reserve: NULL batch");
    if (samples < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_reserve: %d samples", samples);
    const unsigned long long bytes = (unsigned long long)samples * (unsigned long long)b->S * sizeof(DiagOut);
    if (bytes > (1ull << 31))
        return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_reserve: %d samples of %d systems are %llu bytes (at most 2^31)",
                          samples, b->S, bytes);
    HIP_TRY(hipSetDevice(b->desc.device));
    HIP_TRY(hipStreamSynchronize(b->stream));              // records in flight write the log that is about to go
    rows_free(b->dg_log);
    b->log_cap = 0;
    b->log_rows = 0;
    if (samples == 0) return NBODY_OK;
    int rc = diag_alloc_tiles(b);                          // here, so that a record allocates nothing
    if (rc != NBODY_OK) return rc;
    const hipError_t e = rows_reserve_device(b->dg_log, (size_t)samples * (size_t)b->S);
    if (e != hipSuccess) return rows_alloc_failed(e, "batch diagnostics", "recorded series");
    HIP_TRY(hipMemsetAsync(b->dg_log.d, 0, (size_t)bytes, b->stream));
    b->log_cap = samples;
    return NBODY_OK;
}

int nbody_batch_diag_record(nbody_batch* b) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_record: NULL batch");
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_diag_record before nbody_batch_upload");
    if (!b->dg_log.d) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_diag_record without a reservation (nbody_batch_diag_reserve)");
    if (b->log_rows >= b->log_cap)
        return nbody_fail(NBODY_ERR_CAPACITY, "nbody_batch_diag_record: the log holds its %d samples already", b->log_cap);
    HIP_TRY(hipSetDevice(b->desc.device));
    int rc = enqueue_diagnostics(b, b->dg_log.d + (size_t)b->log_rows * (size_t)b->S, nullptr);
    if (rc != NBODY_OK) return rc;
    b->log_rows += 1;
    return NBODY_OK;
}

int nbody_batch_diag_read(nbody_batch* b, nbody_diag* out, int cap_samples, int* n_samples) {
    if (!b || !out || !n_samples) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_read: NULL argument");
    if (cap_samples < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_diag_read: cap_samples %d", cap_samples);
    HIP_TRY(hipSetDevice(b->desc.device));
    int rc = read_meta(b);                                 // synchronises: every enqueued record has been written
    if (rc != NBODY_OK) return rc;
    const int rows = b->log_rows < cap_samples ? b->log_rows : cap_samples;
    if (rows > 0)
        HIP_TRY(hipMemcpy(out, b->dg_log.d, (size_t)rows * (size_t)b->S * sizeof(DiagOut), hipMemcpyDeviceToHost));
    *n_samples = b->log_rows;
    return NBODY_OK;
}

const char* nbody_batch_kernel_name(nbody_batch* b) {
    if (!b) return "";
    switch (b->K) {
        case 1: return "forces_batch_f32 (1 lane per body)";
        case 2: return "forces_batch_f32 (2 lanes per body)";
        case 4: return "forces_batch_f32 (4 lanes per body)";
        default: return "forces_batch_f32 (8 lanes per body)";
    }
}

}  // extern "C"

namespace {

constexpr int kIdsTranslateGrid = 2;                       // workgroups of ids_translate per system (a grid-stride loop)

template <int B>
void ids_step_b(nbody_batch* b, int nblk) {
    ids_enqueue_step<float, B>(b->ids, b->stream, nblk, b->S, kIdsTranslateGrid, (const Rec<float>*)b->S_J,
                               (const Meta*)b->meta, (const int*)b->blk_counts, b->cap, b->counters,
                               (const Event*)b->events, b->ev_cap);
}

void ids_step(nbody_batch* b, int nblk, int threads) {
    if (threads == kCommitSmall) ids_step_b<kCommitSmall>(b, nblk);
    else ids_step_b<kCommitLarge>(b, nblk);
}

int ids_restart(nbody_batch* b) {
    ids_enqueue_fill<kIdsBlock>(b->ids, b->stream, b->S, b->cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ids_clear_done(b->ids, b->stream, (size_t)b->S));
    return NBODY_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Track log (nbody_batch_track_*; kernels and the shared host code in nbody_tracks.hpp): one selection for every system,
// system = blockIdx.y.  At the end of the file for the reason the identities are.
// ---------------------------------------------------------------------------------------------------------
extern "C" {

int nbody_batch_track_reserve(nbody_batch* b, int samples, const int32_t* ids, int k, uint32_t fields) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_track_reserve: NULL batch");
    return track_reserve(b->trk, b->stream, b->desc.device, "nbody_batch_track_reserve", b->ids.on(), b->S, b->cap,
                         sizeof(TrackRec<float>), samples, ids, k, fields);
}

int nbody_batch_track_record(nbody_batch* b) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_track_record: NULL batch");
    if (!b->ids.on()) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_track_record: the batch was created without NBODY_FLAG_TRACK_IDS");
    return track_record<float>(b->trk, b->stream, b->desc.device, "nbody_batch_track_record", b->uploaded,
                               (const Rec<float>*)b->J, (const Vec2<float>*)b->V, (const Meta*)b->meta, b->counters,
                               b->ids.current(), b->cap);
}

int nbody_batch_track_read(nbody_batch* b, nbody_track_row* rows, void* rec, int32_t* index, double* phi, int cap_samples,
                           int* n_samples, int* columns) {
    if (!b) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_track_read: NULL batch");
    if (cap_samples < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_track_read: cap_samples %d", cap_samples);
    if (!b->ids.on()) return nbody_fail(NBODY_ERR_STATE, "nbody_batch_track_read: the batch was created without NBODY_FLAG_TRACK_IDS");
    HIP_TRY(hipSetDevice(b->desc.device));
    int rc = read_meta(b);                                 // synchronises: every enqueued record has been written
    if (rc != NBODY_OK) return rc;
    return track_read(b->trk, "nbody_batch_track_read", rows, rec, index, phi, cap_samples, n_samples, columns);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Row queries (nbody_batch_get_field, nbody_batch_get_neighbors, nbody_batch_get_knn, nbody_batch_get_shells, nbody_batch_get_groups,
// nbody_batch_get_pair_counts, nbody_batch_get_encounters, nbody_batch_get_binaries, nbody_batch_get_tides, nbody_batch_get_shell_moments; nbody_rows.hpp and the ten query headers): one launch (groups: per sweep) for every system, system = blockIdx.y, one set
// of points and edges for all of them.  At the end of the file for the reason the identities are.
// ---------------------------------------------------------------------------------------------------------
namespace {

// The systems as an entry point's argument checks count them: those come before the check of the handle itself.
unsigned long long batch_systems(const nbody_batch* b) { return b ? (unsigned long long)b->S : 1; }

// What every row query of a batch begins with.  It makes no read before the launch: the grid covers the largest uploaded
// count (site.n_bound), each system's count comes from Meta on the device.
int batch_rows_site(nbody_batch* b, const char* who, RowsSite& site) {
    if (!b->uploaded) return nbody_fail(NBODY_ERR_STATE, "%s before nbody_batch_upload", who);
    HIP_TRY(hipSetDevice(b->desc.device));
    site = RowsSite{b->stream, b->J, (const Meta*)b->meta, b->counters, b->h_meta, b->cap, b->S, b->n_upper};
    return NBODY_OK;
}

// run(T(), read_meta): run is the query's host driver <T, RowsBatchCount>; a batch is fp32.
template <typename Run>
int batch_rows_run(nbody_batch* b, Run run) { return run(float(), [b] { return read_meta(b); }); }

// A query with a record per row (rows_run).
template <typename Q>
int batch_rows(nbody_batch* b, const char* who, PointBuffers<typename Q::Device>& buf, const Q& q, const nbody_vec2* points,
               int m, typename Q::Result* out) {
    RowsSite site;
    const int rc = batch_rows_site(b, who, site);
    if (rc != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return rows_run<decltype(t), RowsBatchCount>(who, site, buf, q, points, m, out, sync);
    });
}

}  // namespace

extern "C" {

int nbody_batch_get_field(nbody_batch* b, const nbody_vec2* points, int m, nbody_field* out, int64_t* coincident) {
    const int rc = rows_check_args("nbody_batch_get_field", {b, out, coincident}, m,
                                   batch_systems(b) * sizeof(nbody_field), " of results");
    if (rc != NBODY_OK) return rc;
    return batch_rows(b, "nbody_batch_get_field", b->q.fld, FieldQuery{(double)kG, coincident}, points, m, out);
}

int nbody_batch_get_neighbors(nbody_batch* b, const nbody_vec2* points, int m, nbody_neighbor* out) {
    const int rc = rows_check_args("nbody_batch_get_neighbors", {b, out}, m,
                                   batch_systems(b) * sizeof(nbody_neighbor), " of results");
    if (rc != NBODY_OK) return rc;
    return batch_rows(b, "nbody_batch_get_neighbors", b->q.nbr, NeighborQuery{}, points, m, out);
}

int nbody_batch_get_knn(nbody_batch* b, const nbody_vec2* points, int m, int k, double* d2, int32_t* index) {
    const int rc = knn_check_args("nbody_batch_get_knn", {b, d2, index}, m, k, batch_systems(b));
    if (rc != NBODY_OK) return rc;
    KnnResult out{d2, index};
    return batch_rows(b, "nbody_batch_get_knn", b->q.knn, KnnQuery{k}, points, m, &out);
}

int nbody_batch_get_shells(nbody_batch* b, const nbody_vec2* points, int m, const double* edges2, int bins, double* mass,
                           int32_t* count) {
    const int rc = shells_check_args("nbody_batch_get_shells", {b, edges2, mass, count}, m, edges2, bins,
                                     batch_systems(b));
    if (rc != NBODY_OK) return rc;
    ShellResult out{mass, count};
    return batch_rows(b, "nbody_batch_get_shells", b->q.shl, ShellQuery{edges2, bins}, points, m, &out);
}

// Shell moments (nbody_shell_moments.hpp): one set of points, point velocities and edges for every system, one launch.
int nbody_batch_get_shell_moments(nbody_batch* b, const nbody_vec2* points, const nbody_vec2* point_vel, int m,
                                  const double* edges2, int bins, nbody_shell_moment* out) {
    const char* who = "nbody_batch_get_shell_moments";
    RowsSite site;
    int rc = shell_moments_check_args(who, {b, out}, points, point_vel, m, edges2, bins, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return shell_moments_run<decltype(t), RowsBatchCount>(who, site, b->q.shm, b->V, points, point_vel, m, edges2, bins, out,
                                                              sync);
    });
}

int nbody_batch_get_groups(nbody_batch* b, double link, double radius_scale, int32_t* label, nbody_groups_info* info) {
    const char* who = "nbody_batch_get_groups";
    RowsSite site;
    int rc = groups_check_args(who, link, radius_scale, {b, label, info});
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return groups_run<decltype(t), RowsBatchCount>(who, site, b->q.grp, link, radius_scale, label, info, sync);
    });
}

int nbody_batch_get_pair_counts(nbody_batch* b, const nbody_vec2* points, int m, const double* edges2, int bins, uint64_t* counts,
                                nbody_pair_info* info) {
    const char* who = "nbody_batch_get_pair_counts";
    RowsSite site;
    int rc = pairs_check_args(who, {b, edges2, counts, info}, m, edges2, bins);
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return pairs_run<decltype(t), RowsBatchCount>(who, site, b->q.prs, points, m, edges2, bins, counts, info, sync);
    });
}

// Encounters (nbody_encounters.hpp): one horizon and one cap for every system, one launch.
int nbody_batch_get_encounters(nbody_batch* b, double horizon, nbody_encounter* out, int cap, nbody_encounter_info* info) {
    const char* who = "nbody_batch_get_encounters";
    RowsSite site;
    int rc = pair_log_check_args(who, b, EncQuery{horizon}, out, cap, info, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return pair_log_run<decltype(t), RowsBatchCount>(who, site, b->V, b->q.enc, EncQuery{horizon}, out, cap, info, sync);
    });
}

// Bound pairs (nbody_binaries.hpp): one sep2 and one cap for every system, one launch.
int nbody_batch_get_binaries(nbody_batch* b, double sep2, nbody_binary* out, int cap, nbody_binary_info* info) {
    const char* who = "nbody_batch_get_binaries";
    RowsSite site;
    int rc = pair_log_check_args(who, b, BinQuery{sep2}, out, cap, info, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return pair_log_run<decltype(t), RowsBatchCount>(who, site, b->V, b->q.bin, BinQuery{sep2}, out, cap, info, sync);
    });
}

// Tidal tensor and jerk (nbody_tides.hpp): one set of points and point velocities for every system, one launch.
int nbody_batch_get_tides(nbody_batch* b, const nbody_vec2* points, const nbody_vec2* point_vel, int m, nbody_tide* tide,
                          nbody_vec2* jerk, int64_t* coincident) {
    const char* who = "nbody_batch_get_tides";
    RowsSite site;
    int rc = tides_check_args(who, {b, tide, coincident}, points, point_vel, jerk, m, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return tides_run<decltype(t), RowsBatchCount>(who, site, b->q.tid, (double)kG, b->V, points, point_vel, m, tide, jerk,
                                                      coincident, sync);
    });
}

// Tracers (nbody_tracers.hpp): the same m for every system, one launch per ensemble step.
int nbody_batch_tracers_set(nbody_batch* b, const nbody_tracer* t, int m, uint32_t flags) {
    const char* who = "nbody_batch_tracers_set";
    const int rc = tracers_check_set(who, b, t, m, flags, (int)batch_systems(b));
    if (rc != NBODY_OK) return rc;
    HIP_TRY(hipSetDevice(b->desc.device));
    return tracers_set(who, b->q.trc, b->stream, b->S, t, m, flags);
}

int nbody_batch_tracers_get(nbody_batch* b, nbody_tracer* out, nbody_field* last, nbody_tracer_info* info) {
    if (!b || !info) return nbody_fail(NBODY_ERR_INVALID, "nbody_batch_tracers_get: NULL argument");
    HIP_TRY(hipSetDevice(b->desc.device));
    return tracers_get(b->q.trc, b->stream, b->S, out, last, out ? b->q.trc.m : 0, info, [b] { return read_meta(b); });
}

// Group energies (nbody_group_energy.hpp): every sweep and the potential ONE launch each for the whole batch.
int nbody_batch_get_group_potential(nbody_batch* b, double link, double radius_scale, int32_t* label, double* phi_in,
                                    nbody_group_energy_info* info) {
    const char* who = "nbody_batch_get_group_potential";
    RowsSite site;
    int rc = groups_check_args(who, link, radius_scale, {b, label, phi_in, info});
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return group_energy_run<decltype(t), RowsBatchCount>(who, site, b->q.grp, b->q.gen, (double)kG, link, radius_scale, label, phi_in,
                                                             info, sync);
    });
}

}  // extern "C"

// Cell sums (nbody_cells.hpp): one grid for every system, each stage ONE launch for the whole batch.  After everything else,
// for the group energies' reason.
extern "C" {

int nbody_batch_get_cells(nbody_batch* b, const nbody_grid* grid, uint32_t flags, nbody_cell* cells, int32_t* cell_of,
                          int32_t* start, int32_t* order, nbody_cells_info* info) {
    const char* who = "nbody_batch_get_cells";
    RowsSite site;
    int rc = cells_check_args(who, {b, cells, info}, grid, flags, cell_of, start, order, 0, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return cells_run<decltype(t), RowsBatchCount>(who, site, b->q.cel, b->V, *grid, flags, cells, cell_of, start, order, info, sync);
    });
}

}  // extern "C"

// Radius queries (nbody_within.hpp): one grid, one h2, one set of points and one cap for every system, each stage ONE launch
// for the whole batch.
extern "C" {

int nbody_batch_get_within(nbody_batch* b, const nbody_grid* grid, double h2, const nbody_vec2* points, int m, nbody_within* out,
                           int64_t* start, int32_t* list, int cap, nbody_within_info* info) {
    const char* who = "nbody_batch_get_within";
    RowsSite site;
    int rc = within_check_args(who, {b, out, info}, grid, h2, m, start, list, cap, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return within_run<decltype(t), RowsBatchCount>(who, site, b->q.cel, b->q.wth, *grid, h2, points, m, out, start, list, cap, info,
                                                       sync);
    });
}

}  // extern "C"

// Groups on the cell list (nbody_groups_grid.hpp): one grid, one link and one scale for every system, the list stages and
// every sweep ONE launch each for the whole batch.
extern "C" {

int nbody_batch_get_groups_grid(nbody_batch* b, const nbody_grid* grid, double link, double radius_scale, int32_t* label,
                                nbody_groups_grid_info* info) {
    const char* who = "nbody_batch_get_groups_grid";
    RowsSite site;
    int rc = groups_grid_check_args(who, {b, label, info}, grid, link, radius_scale, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return groups_grid_run<decltype(t), RowsBatchCount>(who, site, b->q.cel, b->q.grp, *grid, link, radius_scale, label,
                                                            info, sync);
    });
}

}  // extern "C"

// The k nearest on the cell list (nbody_knn_grid.hpp): one grid, one set of points, one k, one h0 and one h2_max for every
// system, the list stages and the walk ONE launch each for the whole batch.
extern "C" {

int nbody_batch_get_knn_grid(nbody_batch* b, const nbody_grid* grid, const nbody_vec2* points, int m, int k, double h0,
                             double h2_max, double* d2, int32_t* index, nbody_knn_grid_info* info) {
    const char* who = "nbody_batch_get_knn_grid";
    RowsSite site;
    int rc = knn_grid_check_args(who, {b, d2, index, info}, grid, m, k, h0, h2_max, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return knn_grid_run<decltype(t), RowsBatchCount>(who, site, b->q.cel, b->q.kng, *grid, points, m, k, h0, h2_max, d2, index,
                                                         info, sync);
    });
}

}  // extern "C"

// Pair counts and bound pairs on the cell list (nbody_pairs_grid.hpp): one grid, one set of points and edges or one sep2 and
// one cap for every system, the list stages and the walk ONE launch each for the whole batch.
extern "C" {

int nbody_batch_get_pair_counts_grid(nbody_batch* b, const nbody_grid* grid, const nbody_vec2* points, int m, const double* edges2,
                                     int bins, uint64_t* counts, nbody_pair_grid_info* info) {
    const char* who = "nbody_batch_get_pair_counts_grid";
    RowsSite site;
    int rc = pairs_grid_check_args(who, {b, edges2, counts, info}, grid, m, edges2, bins, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return pairs_grid_run<decltype(t), RowsBatchCount>(who, site, b->q.cel, b->q.prs, *grid, points, m, edges2, bins, counts, info,
                                                           sync);
    });
}

int nbody_batch_get_binaries_grid(nbody_batch* b, const nbody_grid* grid, double sep2, nbody_binary* out, int cap,
                                  nbody_binary_grid_info* info) {
    const char* who = "nbody_batch_get_binaries_grid";
    RowsSite site;
    int rc = binaries_grid_check_args(who, b, grid, sep2, out, cap, info, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return binaries_grid_run<decltype(t), RowsBatchCount>(who, site, b->V, b->q.cel, b->q.bin, *grid, sep2, out, cap, info, sync);
    });
}

}  // extern "C"

// Encounters on the cell list (nbody_encounters_grid.hpp): one grid, one horizon and one cap for every system, the list
// stages and the walk ONE launch each for the whole batch.
extern "C" {

int nbody_batch_get_encounters_grid(nbody_batch* b, const nbody_grid* grid, double horizon, nbody_encounter* out, int cap,
                                    nbody_encounter_grid_info* info) {
    const char* who = "nbody_batch_get_encounters_grid";
    RowsSite site;
    int rc = encounters_grid_check_args(who, b, grid, horizon, out, cap, info, batch_systems(b));
    if (rc != NBODY_OK || (rc = batch_rows_site(b, who, site)) != NBODY_OK) return rc;
    return batch_rows_run(b, [&](auto t, auto sync) {
        return encounters_grid_run<decltype(t), RowsBatchCount>(who, site, b->V, b->q.cel, b->q.enc, *grid, horizon, out, cap, info,
                                                                sync);
    });
}

}  // extern "C"
