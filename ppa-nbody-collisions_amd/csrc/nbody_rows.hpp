// csrc/nbody_rows.hpp -- a row per lane over the resident state: what the row queries (field evaluation, nbody_field.hpp;
// neighbour queries, nbody_neighbors.hpp) have in common, on the device and on the host.  Included
// after nbody_diag.hpp and before the query headers by both translation units: one system (nbody_ctx.hip) and a batch
// (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride` apart, one set of points for every system) share each
// query's one kernel.
//
// A row is a current body (kOwn: read from J on the device, results `stride` apart per system) or an explicit point
// (results m apart per system).  One lane per row, kDiagBlock lanes per workgroup, grid = (ceil(rows / kDiagBlock),
// systems); every workgroup walks all n sources of its system in kTile-body tiles.
//   * The count.  One system: the exact count is an argument (the host has just read Meta).  A batch: from the system's
//     Meta; a count outside [0, stride] never becomes an index - the system is treated as empty and reported once (block 0,
//     lane 0) as kIndexError in its Counters::errors, which fails the host's next read_meta.
//   * Workgroups past the last row leave before the first barrier; a wave past the last row only loads tiles.
//   * An empty system: every row gets the query's empty record and the workgroup leaves, again as a whole.
//   * kOwn: the self term j == i can only occur in the tile that holds the wave's own rows (64 contiguous rows, inside one
//     128-body tile: wave-uniform), so only that tile runs a checked loop.  Points have no checked loop at all.
//
// Adding a row query takes a kernel `<T, kOwn, Count>` that opens with rows_prologue and walks with its own pair functor,
// and a traits struct (FieldQuery, NeighborQuery) that names the records, launches that kernel and unpacks a system's
// results; rows_run and the per-handle wrappers in the two .hip files do the rest.
#pragma once
#include <stddef.h>
#include <string.h>
#include <initializer_list>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_diag.hpp"

namespace nbk {

struct FieldPoint { double x, y; };                               // nbody_vec2
static_assert(sizeof(FieldPoint) == sizeof(nbody_vec2), "nbody_vec2 layout");

// Where the count comes from; < 0: outside [0, stride] (batch_checked_count, nbody_kernels.hpp).
struct RowsOneCount {
    static constexpr bool kBatch = false;
    static __device__ __forceinline__ int checked(const Meta*, int, int, int n_one) { return n_one; }
};
struct RowsBatchCount {
    static constexpr bool kBatch = true;
    static __device__ __forceinline__ int checked(const Meta* meta_all, int sys, int stride, int) {
        return batch_checked_count(meta_all[sys].n, stride);
    }
};

// What the prologue leaves a lane with.
template <typename T, typename Out>
struct RowsLane {
    const Rec<T>* J;            // the system's sources, [n]
    Out* out;                   // the system's results, [rows]
    int n, rows, p;             // sources, rows, this lane's row
    int self_tile;              // kOwn: the one j tile that holds this wave's self terms; otherwise -1
    bool valid, wave_works;     // the lane has a row; its wave has one
};

// true: the whole workgroup returns now (it has no row, or the system is empty and its rows have `empty` already).  The
// kernel takes that exit before any barrier.
template <typename T, bool kOwn, typename Count, typename Out>
__device__ __forceinline__ bool rows_prologue(RowsLane<T, Out>& L, const Rec<T>* __restrict__ J_all,
                                              const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all, int stride,
                                              int n_one, int m, Out* __restrict__ out_all, Out empty) {
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int tid = threadIdx.x;
    const int chk = Count::checked(meta_all, sys, stride, n_one);
    L.n = chk < 0 ? 0 : chk;
    if (chk < 0 && blockIdx.x == 0 && tid == 0) atomicAdd(&ctr_all[sys].errors, kIndexError);
    L.rows = kOwn ? L.n : m;
    const int row0 = blockIdx.x * kDiagBlock;                    // first row of the workgroup
    if (row0 >= L.rows) return true;
    L.p = row0 + tid;
    L.valid = L.p < L.rows;
    L.J = J_all + (size_t)sys * (size_t)stride;
    L.out = out_all + (size_t)sys * (size_t)(kOwn ? stride : m);
    if (L.n == 0) {                                              // explicit points over an empty system
        if (L.valid) L.out[L.p] = empty;
        return true;
    }
    const int wave0 = row0 + (tid & ~(kWave - 1));               // first row of this wave
    L.wave_works = wave0 < L.rows;
    L.self_tile = kOwn ? wave0 / kTile : -1;
    return false;
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one query of one context or batch, allocated on the first call and grown to the largest
// request seen - the device points, the device results, and one pinned staging area for both directions.
// ---------------------------------------------------------------------------------------------------------
constexpr unsigned long long kFieldMaxBytes = 1ull << 31;   // of the caller's `out`

template <typename Out>
struct PointBuffers {
    FieldPoint* pts = nullptr;      // [cap_pts]
    Out* out = nullptr;             // [cap_out]
    unsigned char* h = nullptr;     // pinned: max(cap_pts * sizeof(FieldPoint), cap_out * sizeof(Out)) bytes
    size_t cap_pts = 0, cap_out = 0, h_bytes = 0;
};

template <typename Out>
inline void rows_free(PointBuffers<Out>& f) {
    (void)hipFree(f.pts); (void)hipFree(f.out);
    if (f.h) (void)hipHostFree(f.h);
    f = PointBuffers<Out>{};
}

template <typename Out>
inline int rows_reserve(PointBuffers<Out>& f, size_t n_pts, size_t n_out, const char* who) {
    hipError_t e = hipSuccess;
    if (n_pts > f.cap_pts) {
        (void)hipFree(f.pts);
        f.pts = nullptr; f.cap_pts = 0;
        e = hipMalloc((void**)&f.pts, n_pts * sizeof(FieldPoint));
        if (e == hipSuccess) f.cap_pts = n_pts; else f.pts = nullptr;
    }
    if (e == hipSuccess && n_out > f.cap_out) {
        (void)hipFree(f.out);
        f.out = nullptr; f.cap_out = 0;
        e = hipMalloc((void**)&f.out, n_out * sizeof(Out));
        if (e == hipSuccess) f.cap_out = n_out; else f.out = nullptr;
    }
    const size_t hb = f.cap_pts * sizeof(FieldPoint) > f.cap_out * sizeof(Out) ? f.cap_pts * sizeof(FieldPoint)
                                                                               : f.cap_out * sizeof(Out);
    if (e == hipSuccess && hb > f.h_bytes) {
        if (f.h) (void)hipHostFree(f.h);
        f.h = nullptr; f.h_bytes = 0;
        e = hipHostMalloc((void**)&f.h, hb, hipHostMallocDefault);
        if (e == hipSuccess) f.h_bytes = hb; else f.h = nullptr;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return nbody_fail(e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP, "%s, point and result buffers: %s", who,
                          hipGetErrorString(e));
    }
    return NBODY_OK;
}

// The argument checks an entry point makes before any device call.  `required`: every pointer that must not be NULL;
// `record`: the size of one of the caller's result records, of which there are m per system.
inline int rows_check_args(const char* who, std::initializer_list<const void*> required, int m, unsigned long long systems,
                           size_t record) {
    for (const void* p : required)
        if (!p) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (m < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: m = %d", who, m);
    if ((unsigned long long)m * systems * record > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d points are more than 2^31 bytes of results", who, m);
    return NBODY_OK;
}

#define NBK_ROWS_TRY(expr)                                                                                \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return nbody_fail(NBODY_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),      \
                              __FILE__, __LINE__);                                                        \
    } while (0)

// What a context or a batch lends rows_run.
struct RowsSite {
    hipStream_t stream;
    const void* J;              // device Rec<T> [systems * stride]
    const Meta* meta;           // device [systems]
    Counters* counters;         // device [systems]
    const Meta* h_meta;         // the host's copy [systems], current once read_meta has returned
    int stride, systems;
    int n_bound;                // own rows the grid covers: a context's exact count, a batch's upper bound
};

// One query, from the reservation to the caller's records.  Count says whose: a context (RowsOneCount: the exact count,
// read by the caller just before, goes to the kernel; nothing to do for no rows) or a batch (RowsBatchCount: the grid
// covers n_bound rows of every system, the kernel takes each count from Meta, and read_meta is called even for no rows).
// Q: the query's traits - Device and Result records, launch<T, kOwn, Count>(grid, stream, out, common kernel arguments...),
// empty(s) and unpack(s, staged records, how many, the caller's) for system s.  read_meta synchronises the stream and
// reports a device-side failure.
template <typename T, typename Count, typename Q, typename ReadMeta>
int rows_run(const char* who, const RowsSite& s, PointBuffers<typename Q::Device>& buf, const Q& q, const nbody_vec2* points,
             int m, typename Q::Result* out, ReadMeta read_meta) {
    using Device = typename Q::Device;
    const bool own = points == nullptr;
    const int rows = own ? s.n_bound : m;                                  // what the grid covers
    const size_t per_sys = own ? (size_t)s.stride : (size_t)m;             // results of one system on the device
    const size_t total = Count::kBatch ? per_sys * (size_t)s.systems : (size_t)rows;
    for (int sys = 0; sys < s.systems; ++sys) q.empty(sys);
    if (rows == 0) return Count::kBatch ? read_meta() : NBODY_OK;
    int rc = rows_reserve(buf, own ? 0 : (size_t)m, total, who);
    if (rc != NBODY_OK) return rc;
    const dim3 grid((rows + kDiagBlock - 1) / kDiagBlock, s.systems);
    const Rec<T>* J = (const Rec<T>*)s.J;
    const int n_one = Count::kBatch ? 0 : s.n_bound;
    if (own) {
        q.template launch<T, true, Count>(grid, s.stream, buf.out, J, s.meta, s.counters, s.stride, n_one,
                                          (const FieldPoint*)nullptr, 0);
    } else {
        memcpy(buf.h, points, (size_t)m * sizeof(FieldPoint));
        NBK_ROWS_TRY(hipMemcpyAsync(buf.pts, buf.h, (size_t)m * sizeof(FieldPoint), hipMemcpyHostToDevice, s.stream));
        q.template launch<T, false, Count>(grid, s.stream, buf.out, J, s.meta, s.counters, s.stride, n_one,
                                           (const FieldPoint*)buf.pts, m);
    }
    NBK_ROWS_TRY(hipGetLastError());
    NBK_ROWS_TRY(hipMemcpyAsync(buf.h, buf.out, total * sizeof(Device), hipMemcpyDeviceToHost, s.stream));
    rc = read_meta();                                      // synchronises; a system whose count failed its check ends here
    if (rc != NBODY_OK) return rc;
    const Device* h = reinterpret_cast<const Device*>(buf.h);
    for (int sys = 0; sys < s.systems; ++sys) {
        const int n = s.h_meta[sys].n;
        const size_t cnt = own ? (size_t)(n < 0 || n > s.stride ? 0 : n) : (size_t)m;
        q.unpack(sys, h + (size_t)sys * per_sys, cnt, out + (size_t)sys * per_sys);
    }
    return NBODY_OK;
}

}  // namespace nbk
