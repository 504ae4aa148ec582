// csrc/nbody_tracks.hpp -- gfx950 device code and shared host code of the track log (nbody_track_*, nbody_batch_track_*,
// include/nbody.h): a device-side table of samples x columns, column c standing for body IDENTITY sel[c]
// (NBODY_FLAG_TRACK_IDS, nbody_ids.hpp).  A record enqueues one row - where was identity k, how heavy was it, is it still
// there - with no device-to-host copy and no host wait; the table is read back once.  Shared by the one-system stepper
// (nbody_ctx.hip: blockIdx.y = 0) and the batched stepper (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride`
// apart, one selection for every system), like nbody_ids.hpp.
//
// Both kernels run between steps, on the committed state: Meta, J, V and the map ids_cur are those of the same moment.
//   track_gather    : one lane per column.  The map is strictly increasing in i (the compaction is stable), so sel[c] is
//                     found by binary search over [0, n); and ids[i] >= i, so the search never looks past index sel[c].
//                     Present: index = i and the record is {x, y, vx, vy, m, r} of body i, moved, never computed with
//                     (the bits of nbody_download).  Absent: index = -1 and a record of all-zero bytes.  Every column is
//                     written exactly once per record: no memset of the row, no atomics on it.  Lane 0 of a system writes
//                     the row header from Meta.
//   track_potential : one lane per column, working for the columns track_gather found present (it reads `index`, written
//                     by the launch before it on the same stream).  The sum over j is diag_walk (nbody_diag.hpp) in its
//                     form for gathered rows - the tile that holds a lane's self term is not wave-uniform, so the lanes
//                     of a wave vote per tile - and diag_row_general for a flagged row: phi has the bits diag_potential
//                     gives that row.  Workgroups without a present column leave before the first tile; absent columns
//                     get +0.
// A count outside [0, stride] never becomes an index or a search bound (ids_checked_count's rule): the row is all absent,
// n_bodies = 0, and the system's Counters::errors gets kIndexError.
//
// Every kernel here is a template: both translation units include this file, and both name the templates at the END of
// the file, so every kernel that existed before keeps its place and its code (see nbody_ids.hpp).
#pragma once
#include <stdint.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_diag.hpp"
#include "nbody_rows.hpp"
#include "nbody_ids.hpp"

#pragma clang fp contract(off)

namespace nbk {

template <typename T> struct TrackRec { T x, y, vx, vy, m, r; };   // nbody_track_f32 / nbody_track_f64
struct TrackRow { long long step, n_bodies; };                      // nbody_track_row
static_assert(sizeof(TrackRec<float>) == sizeof(nbody_track_f32) && sizeof(TrackRec<float>) == 24, "nbody_track_f32 layout");
static_assert(sizeof(TrackRec<double>) == sizeof(nbody_track_f64) && sizeof(TrackRec<double>) == 48, "nbody_track_f64 layout");
static_assert(sizeof(TrackRow) == sizeof(nbody_track_row) && sizeof(TrackRow) == 16, "nbody_track_row layout");

constexpr int kTrackBlock = 256;                            // lanes of a track_gather workgroup; track_potential: kDiagBlock

// grid = (ceil(columns / B), S).  rows / rec / index point at the sample's row: [S], [S * columns], [S * columns].
// sel == NULL: column c is identity c.
template <typename T, int B>
__global__ __launch_bounds__(B) void track_gather(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                  const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                  const int32_t* __restrict__ ids_all, int stride,
                                                  const int32_t* __restrict__ sel, int columns,
                                                  TrackRow* __restrict__ rows, TrackRec<T>* __restrict__ rec,
                                                  int32_t* __restrict__ index) {
    const int sys = blockIdx.y;
    const Meta m = meta_all[sys];
    const bool bad = m.n < 0 || m.n > stride;
    const int n = bad ? 0 : m.n;
    const int c = blockIdx.x * B + threadIdx.x;
    if (c == 0) {
        rows[sys] = TrackRow{(long long)m.step, (long long)n};
        if (bad) atomicAdd(&ctr_all[sys].errors, kIndexError);
    }
    if (c >= columns) return;
    const size_t base = (size_t)sys * (size_t)stride;
    const int32_t* __restrict__ ids = ids_all + base;
    const int32_t key = sel ? sel[c] : c;
    // first i in [0, n) with ids[i] >= key; ids[i] >= i, so it is at most key
    int lo = 0, hi = key < n ? key + 1 : n;                 // key >= 0 (checked by the reservation); hi <= n <= stride
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const bool present = lo < n && ids[lo] == key;
    TrackRec<T> o{(T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    if (present) {
        const Rec<T> r = J_all[base + lo];
        const Vec2<T> v = V_all[base + lo];
        o = TrackRec<T>{r.x, r.y, v.x, v.y, r.m, r.r};
    }
    const size_t out = (size_t)sys * (size_t)columns + c;
    rec[out] = o;
    index[out] = present ? lo : -1;
}

// grid = (ceil(columns / kDiagBlock), S).  index / phi point at the sample's row, [S * columns] each.
template <typename T>
__global__ __launch_bounds__(kDiagBlock) void track_potential(const Rec<T>* __restrict__ J_all,
                                                              const Meta* __restrict__ meta_all, int stride, double G,
                                                              const int32_t* __restrict__ index, int columns,
                                                              double* __restrict__ phi) {
    const int sys = blockIdx.y;
    const int n = ids_checked_count(meta_all[sys].n, stride);
    const int tid = threadIdx.x;
    const int c = blockIdx.x * kDiagBlock + tid;
    const size_t out = (size_t)sys * (size_t)columns + (c < columns ? c : 0);
    const int i = c < columns ? index[out] : -1;             // the row of this lane: a body index, not a column
    const bool valid = i >= 0 && i < n;
    if (c < columns && !valid) phi[out] = 0.0;
    if (!__syncthreads_or(valid)) return;                    // the whole workgroup: no present column
    const Rec<T>* __restrict__ J = J_all + (size_t)sys * (size_t)stride;
    double xi = 0.0, yi = 0.0;
    if (valid) {
        const Rec<T> r = J[i];
        xi = (double)r.x; yi = (double)r.y;
    }
    double acc = diag_walk<true>(J, n, i, xi, yi, valid ? i / kTile : -1);   // the self tile differs from lane to lane
    if (!valid) return;
    if (!__builtin_isfinite(acc)) acc = diag_row_general<T>(J, n, i, xi, yi).s;
    phi[out] = -G * acc;
}

// ---------------------------------------------------------------------------------------------------------
// Host side shared by the two steppers: the log of one context or batch, the argument checks and the launches.
// ---------------------------------------------------------------------------------------------------------
struct TrackState {
    unsigned char* buf = nullptr;   // ONE allocation: rows [samples * S] | phi | rec | index, [samples * S * columns] each
    TrackRow* rows = nullptr;
    double* phi = nullptr;          // with NBODY_TRACK_PHI
    unsigned char* rec = nullptr;   // TrackRec<T>
    int32_t* index = nullptr;
    int32_t* sel = nullptr;         // [columns] selected identities, ascending; NULL: column c is identity c
    int samples = 0, columns = 0, systems = 1;
    int recorded = 0;               // rows enqueued since the reservation or the last upload: the next row
    size_t rec_bytes = 0;           // sizeof(TrackRec<T>)
    uint32_t fields = 0;
    bool on() const { return buf != nullptr; }
};

#define NBK_TRACK_TRY(expr)                                                                               \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return nbody_fail(rows_status(e__), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),   \
                              __FILE__, __LINE__);                                                        \
    } while (0)

// The handle's free_all, after its stream synchronise.
inline void track_free(TrackState& st) {
    (void)hipFree(st.buf); (void)hipFree(st.sel);
    st = TrackState{};
}

inline int track_release(TrackState& st, hipStream_t stream) {
    NBK_TRACK_TRY(hipStreamSynchronize(stream));            // records in flight write the log that is about to go
    unsigned char* buf = st.buf;
    int32_t* sel = st.sel;
    st = TrackState{};
    if (buf) NBK_TRACK_TRY(hipFree(buf));
    if (sel) NBK_TRACK_TRY(hipFree(sel));
    return NBODY_OK;
}

// Everything a reservation can refuse is refused here, before any device call.  tracked: NBODY_FLAG_TRACK_IDS was given.
inline int track_reserve(TrackState& st, hipStream_t stream, int device, const char* who, bool tracked, int systems,
                         int capacity, size_t rec_bytes, int samples, const int32_t* ids, int k, uint32_t fields) {
    if (samples < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: %d samples", who, samples);
    if (fields & ~(uint32_t)NBODY_TRACK_PHI) return nbody_fail(NBODY_ERR_INVALID, "%s: unknown fields 0x%x", who, fields);
    if (ids) {
        if (k <= 0) return nbody_fail(NBODY_ERR_INVALID, "%s: %d identities", who, k);
        for (int c = 0; c < k; ++c)
            if (ids[c] < 0 || ids[c] >= capacity || (c > 0 && ids[c] <= ids[c - 1]))
                return nbody_fail(NBODY_ERR_INVALID, "%s: ids[%d] = %d (strictly increasing within [0, capacity %d))", who,
                                  c, ids[c], capacity);
    }
    const int columns = ids ? k : capacity;
    const unsigned long long cells = (unsigned long long)samples * (unsigned long long)systems;
    const unsigned long long per_cell = sizeof(TrackRow) + (unsigned long long)columns *
                                        (rec_bytes + sizeof(int32_t) + ((fields & NBODY_TRACK_PHI) ? sizeof(double) : 0));
    const unsigned long long limit = 1ull << 31;            // the recorded diagnostics' rule; each factor first: no overflow
    const unsigned long long bytes = (cells > limit || per_cell > limit) ? limit + 1 : cells * per_cell;
    if (bytes > limit)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d samples of %d systems x %d columns are more than 2^31 bytes", who, samples,
                          systems, columns);
    if (!tracked) return nbody_fail(NBODY_ERR_STATE, "%s: created without NBODY_FLAG_TRACK_IDS", who);
    NBK_TRACK_TRY(hipSetDevice(device));
    int rc = track_release(st, stream);
    if (rc != NBODY_OK || samples == 0) return rc;
    unsigned char* buf = nullptr;
    int32_t* sel = nullptr;
    hipError_t e = hipMalloc((void**)&buf, (size_t)bytes);
    if (e == hipSuccess && ids) e = hipMalloc((void**)&sel, sizeof(int32_t) * (size_t)k);
    if (e == hipSuccess) e = hipMemsetAsync(buf, 0, (size_t)bytes, stream);   // no later read sees memory nobody wrote
    if (e == hipSuccess && ids) e = hipMemcpyAsync(sel, ids, sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // `ids` is the caller's
    if (e != hipSuccess) {
        (void)hipFree(buf); (void)hipFree(sel);
        return rows_alloc_failed(e, who, "track log");
    }
    const size_t plane = (size_t)cells * (size_t)columns;
    st.buf = buf;
    st.sel = sel;
    st.rows = reinterpret_cast<TrackRow*>(buf);
    unsigned char* p = buf + (size_t)cells * sizeof(TrackRow);
    if (fields & NBODY_TRACK_PHI) { st.phi = reinterpret_cast<double*>(p); p += plane * sizeof(double); }
    st.rec = p;
    st.index = reinterpret_cast<int32_t*>(p + plane * rec_bytes);
    st.samples = samples; st.columns = columns; st.systems = systems; st.recorded = 0;
    st.rec_bytes = rec_bytes; st.fields = fields;
    return NBODY_OK;
}

// One record: one launch, two with NBODY_TRACK_PHI.  The host checks come first: a refused record enqueues nothing.
template <typename T>
int track_record(TrackState& st, hipStream_t stream, int device, const char* who, bool uploaded, const Rec<T>* J,
                 const Vec2<T>* V, const Meta* meta, Counters* ctr, const int32_t* ids_cur, int stride) {
    if (!uploaded) return nbody_fail(NBODY_ERR_STATE, "%s before an upload", who);
    if (!st.on()) return nbody_fail(NBODY_ERR_STATE, "%s without a reservation", who);
    if (st.recorded >= st.samples)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: the log holds its %d samples already", who, st.samples);
    NBK_TRACK_TRY(hipSetDevice(device));
    const size_t row = (size_t)st.recorded * (size_t)st.systems;
    const size_t cell = row * (size_t)st.columns;
    int32_t* index = st.index + cell;
    hipLaunchKernelGGL((track_gather<T, kTrackBlock>), dim3((st.columns + kTrackBlock - 1) / kTrackBlock, st.systems),
                       dim3(kTrackBlock), 0, stream, J, V, meta, ctr, ids_cur, stride, (const int32_t*)st.sel, st.columns,
                       st.rows + row, reinterpret_cast<TrackRec<T>*>(st.rec) + cell, index);
    if (st.phi) {
        hipLaunchKernelGGL((track_potential<T>), dim3((st.columns + kDiagBlock - 1) / kDiagBlock, st.systems),
                           dim3(kDiagBlock), 0, stream, J, meta, stride, (double)kG, (const int32_t*)index, st.columns, st.phi + cell);
    }
    NBK_TRACK_TRY(hipGetLastError());
    st.recorded += 1;
    return NBODY_OK;
}

// After the caller has synchronised: min(recorded, cap_samples) rows of every plane that was asked for.
inline int track_read(const TrackState& st, const char* who, nbody_track_row* rows, void* rec, int32_t* index, double* phi,
                      int cap_samples, int* n_samples, int* columns) {
    if (phi && !st.phi) return nbody_fail(NBODY_ERR_STATE, "%s: the log was reserved without NBODY_TRACK_PHI", who);
    const int take = st.recorded < cap_samples ? st.recorded : cap_samples;
    const size_t cells = (size_t)take * (size_t)st.systems, plane = cells * (size_t)st.columns;
    if (cells) {
        if (rows) NBK_TRACK_TRY(hipMemcpy(rows, st.rows, cells * sizeof(TrackRow), hipMemcpyDeviceToHost));
        if (rec) NBK_TRACK_TRY(hipMemcpy(rec, st.rec, plane * st.rec_bytes, hipMemcpyDeviceToHost));
        if (index) NBK_TRACK_TRY(hipMemcpy(index, st.index, plane * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (phi) NBK_TRACK_TRY(hipMemcpy(phi, st.phi, plane * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (n_samples) *n_samples = st.recorded;
    if (columns) *columns = st.columns;
    return NBODY_OK;
}

#undef NBK_TRACK_TRY

}  // namespace nbk
