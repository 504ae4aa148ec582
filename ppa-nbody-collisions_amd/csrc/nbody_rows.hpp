// csrc/nbody_rows.hpp -- a row per lane over the resident state: what the row queries (field evaluation, nbody_field.hpp;
// neighbour queries, nbody_neighbors.hpp; group finding, nbody_groups.hpp; pair counts, nbody_pairs.hpp; the k nearest,
// nbody_knn.hpp; encounters, nbody_encounters.hpp; bound pairs, nbody_binaries.hpp; group energies, nbody_group_energy.hpp;
// shell sums and moments, nbody_shells.hpp and nbody_shell_moments.hpp)
// have in common, on the device and on the host.  Included after nbody_diag.hpp and before the query headers by both translation units: one system
// (nbody_ctx.hip) and a batch (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride` apart, one set of points for
// every system) share each query's one kernel.
//
// A row is a current body (kOwn: read from J on the device, results `stride` apart per system) or an explicit point
// (results m apart per system).  One lane per row, kDiagBlock lanes per workgroup, grid = (ceil(rows / kDiagBlock),
// systems); every workgroup walks the sources of its system in kTile-body tiles.
//   * The count.  One system: the exact count is an argument (the host has just read Meta).  A batch: from the system's
//     Meta; a count outside [0, stride] never becomes an index - the system is treated as empty and reported once (block 0,
//     lane 0) as kIndexError in its Counters::errors, which fails the host's next read_meta.
//   * Workgroups past the last row leave before the first barrier; a wave past the last row only loads tiles.
//   * An empty system: every row gets the query's empty record and the workgroup leaves, again as a whole.
//   * kOwn: the self term j == i can only occur in the tile that holds the wave's own rows (64 contiguous rows, inside one
//     128-body tile: wave-uniform), so only that tile runs a checked loop.  Points have no checked loop at all.
//
// Adding a row query takes a kernel `<T, kOwn, Count>` that opens with rows_prologue, loads its row with rows_row and hands
// rows_walk (the one tile loop, below) a stage and a functor with the query's four pairs of one trip.  The
// stage says which LDS planes a tile's entry goes into and what a padding entry holds: RowsStage for {x, y[, r]}, a lambda
// in the kernel for a query that needs more (velocities, masses, labels).  A kernel whose lanes count ends with rows_wave_add.
// The host side is built from rows_run (a fixed number of result records per row: a traits struct such as FieldQuery,
// NeighborQuery or KnnQuery is all it takes), from the pair-log driver at the end of this file (a capped list of found
// pairs per system and counters: a traits struct such as EncQuery or BinQuery) or, for another shape of result, from the
// pieces of rows_run - RowsSite's grid, count and sync, RowPoints, rows_check_args.  The per-handle preamble and the
// precision dispatch are in the two .hip files.  Only the ordered family stays out of rows_walk (see there): field_at and
// tides_at (nbody_tides.hpp) walk with diag_walk_sums (nbody_diag.hpp), the ascending
// family's one tile loop; the jerk hands it the velocities' two planes.
#pragma once
#include <stddef.h>
#include <string.h>
#include <initializer_list>
#include <vector>

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

// For a kernel that writes no record of type Out per row (pair_counts has no per-row result, knn_at writes k entries itself):
// rows_prologue's write of the empty record is this assignment, which writes nothing.
struct RowsNoOut {
    RowsNoOut() = default;
    RowsNoOut(const RowsNoOut&) = default;
    __host__ __device__ RowsNoOut& operator=(const RowsNoOut&) { return *this; }
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

// The lane's own row widened to fp64: the body {x, y, r} or the point (r = +0).  A lane without a row carries x = NaN: every
// d2 it forms is NaN, which passes no comparison of any query.
struct RowsRow { double x, y, r; };
template <typename T, bool kOwn, typename Out>
__device__ __forceinline__ RowsRow rows_row(const RowsLane<T, Out>& L, const FieldPoint* __restrict__ points) {
    RowsRow w{__builtin_nan(""), 0.0, 0.0};
    if (L.valid) {
        if (kOwn) {
            const Rec<T> r = L.J[L.p];
            w = RowsRow{(double)r.x, (double)r.y, (double)r.r};
        } else {
            const FieldPoint q = points[L.p];
            w = RowsRow{q.x, q.y, 0.0};
        }
    }
    return w;
}

// The tile walk of every row query whose pairs need no order - the only tile loop of the NaN-padded family: all kDiagBlock
// lanes call it after rows_prologue.  A tile's entries are widened to fp64 ONCE into the query's own double-buffered LDS
// planes (one barrier per tile) and read back by the functor as wave-uniform broadcasts.  Which planes, the walk does not
// know: lane e < kTile calls stage(b, e, live, j), which fills entry e of buffer b from source j where `live` and with the
// query's padding otherwise.  The padding of the ragged tile passes no comparison of the query (RowsStage: x = NaN, so
// d2 = NaN), so the pair loop carries no bound test and no remainder loop - it runs in fours up to the tile's count rounded
// up to 4 (not to kTile: a 64-body system of a batch would pay 128 pairs per row).  The functor is called as
// f.template four<kChecked>(b, q, j): the sources j .. j + 3 are entries q .. q + 3 of buffer b; kChecked: the tile holds
// the wave's own rows, the functor applies its index test.  It is walked in a copy and handed back at the end: what it
// carries from pair to pair (NeighborFour's best), carried through the reference, is promoted from memory twice and every
// pair pays two more selects.
//   * kTri = false, the full walk: every tile; kOwn runs the whole self tile checked, points have no checked loop.
//   * kTri = true (kOwn only), the triangular walk for symmetric pairs, each counted at the higher row: only the tiles up
//     to the one that holds the workgroup's last row are staged (a workgroup-uniform bound: the barriers need it); a wave
//     computes on the tiles below its own rows unchecked, on its own tile checked and only up to its last row, on none above.
// Two tile loops, not one: diag_walk_sums (nbody_diag.hpp), which the potential kernels, field_at, tracers_advance and tides_at
// call, is the ordered family's.  It sums in ascending order under the order contract: a padding entry would
// have to add an exact +0 to every sum instead of failing a comparison, so it keeps a remainder loop; it votes per tile for
// gathered rows; and its self term is masked inside the pair, not tested by the functor.
template <bool kOwn, bool kTri, typename T, typename Out, typename Stage, typename Four>
__device__ __forceinline__ void rows_walk(const RowsLane<T, Out>& L, const Stage stage, Four& carried) {
    static_assert(kOwn || !kTri, "the triangular walk is over own rows");
    Four f = carried;                                            // see above: a local of the function that has the loops
    const int n = L.n, tid = threadIdx.x;
    const int row0 = blockIdx.x * kDiagBlock;
    const int last = (row0 + kDiagBlock < n ? row0 + kDiagBlock : n) - 1;   // kTri: the workgroup's last row
    const int jtiles = kTri ? last / kTile + 1 : (n + kTile - 1) / kTile;   // workgroup-uniform
    const int wave_end = row0 + (tid & ~(kWave - 1)) + kWave;    // one past the wave's last row
    for (int t = 0; t < jtiles; ++t) {
        const int b = t & 1;
        const int j0 = t * kTile;
        const int jn = n - j0 < kTile ? n - j0 : kTile;
        if (tid < kTile) stage(b, tid, tid < jn, j0 + tid);
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        if (!L.wave_works || (kTri && t > L.self_tile)) continue;
        if (!kOwn || t != L.self_tile) {
            const int jn4 = (jn + 3) & ~3;                       // <= kTile: the padding is there
            for (int q = 0; q < jn4; q += 4) f.template four<false>(b, q, j0 + q);
        } else {
            const int je = kTri && wave_end - j0 < jn ? wave_end - j0 : jn;   // no row of this wave is above wave_end - 1
            const int jn4 = (je + 3) & ~3;
            for (int q = 0; q < jn4; q += 4) f.template four<true>(b, q, j0 + q);
        }
    }
    carried = f;
}

// The stage of the queries that need positions only: {x, y[, r]} of the system's records J, the padding x = NaN (y = r = +0).
// sr is staged only for kRadius and may be NULL otherwise.
template <bool kRadius, typename T>
struct RowsStage {
    const Rec<T>* __restrict__ J;
    DiagPlanes *sx, *sy, *sr;
    __device__ __forceinline__ void operator()(int b, int e, bool live, int j) const {
        double x = __builtin_nan(""), y = 0.0, r = 0.0;          // padding: d2 = NaN
        if (live) {
            const Rec<T> s = J[j];
            x = (double)s.x; y = (double)s.y; r = (double)s.r;
        }
        (*sx)[b][e] = x; (*sy)[b][e] = y;
        if constexpr (kRadius) (*sr)[b][e] = r;
    }
};

// The tail of a kernel whose lanes count: each of the N lane counts is summed over the wave and added to its 64-bit counter
// with one atomic from the wave's first lane; a sum of zero adds nothing.  Every lane of the wave calls it.  The N sums go
// through the shuffles together, ahead of the one branch to the first lane.
template <int N>
__device__ __forceinline__ void rows_wave_add(unsigned long long* const (&counter)[N], const unsigned (&lane_count)[N]) {
    unsigned long long c[N];
#pragma unroll
    for (int k = 0; k < N; ++k) c[k] = lane_count[k];
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) c[k] += __shfl_down(c[k], sh, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (c[k]) atomicAdd(counter[k], c[k]);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side.
// ---------------------------------------------------------------------------------------------------------
constexpr unsigned long long kFieldMaxBytes = 1ull << 31;   // of the caller's `out`

#define NBK_ROWS_TRY(expr)                                                                                \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return nbody_fail(NBODY_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),      \
                              __FILE__, __LINE__);                                                        \
    } while (0)

// The one place a HIP error becomes a status, and the epilogue of every failed allocation: the error is cleared, the
// message says who was allocating what.  The caller frees what it holds first or after; nothing here touches it.
inline int rows_status(hipError_t e) { return e == hipErrorOutOfMemory ? NBODY_ERR_NOMEM : NBODY_ERR_HIP; }
inline int rows_alloc_failed(hipError_t e, const char* who, const char* what) {
    (void)hipGetLastError();
    return nbody_fail(rows_status(e), "%s, %s: %s", who, what, hipGetErrorString(e));
}

// What a handle allocates when it is created: every block is recorded here where it is made, and release() is all the
// handle's free_all knows of them - whatever was made before a create failed half way, and each block once.
struct RowsOwned {
    std::vector<void*> dev, pinned;
    template <typename P>
    hipError_t device(P** p, size_t bytes) {
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) dev.push_back(*p);
        return e;
    }
    template <typename P>
    hipError_t host(P** p, size_t bytes) {
        const hipError_t e = hipHostMalloc((void**)p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) pinned.push_back(*p);
        return e;
    }
    void release() {
        for (void* p : dev) (void)hipFree(p);
        for (void* p : pinned) (void)hipHostFree(p);
        dev.clear(); pinned.clear();
    }
};

// A device array and the pinned memory it is sent from or read back into, allocated on the first use and grown to the
// largest request seen.  RowPoints: the explicit points of one query of one context or batch.
template <typename E>
struct RowsArray {
    E* d = nullptr;                 // [cap]
    unsigned char* h = nullptr;     // pinned: cap elements
    size_t cap = 0;
};
using RowPoints = RowsArray<FieldPoint>;

template <typename E>
inline void rows_free(RowsArray<E>& f) {
    (void)hipFree(f.d);
    if (f.h) (void)hipHostFree(f.h);
    f = RowsArray<E>{};
}

template <typename E>
inline hipError_t rows_reserve(RowsArray<E>& f, size_t n) {
    if (n <= f.cap) return hipSuccess;
    rows_free(f);
    hipError_t e = hipMalloc((void**)&f.d, n * sizeof(E));
    if (e == hipSuccess) e = hipHostMalloc((void**)&f.h, n * sizeof(E), hipHostMallocDefault);
    if (e == hipSuccess) f.cap = n; else f.h = nullptr;
    return e;
}

// Device only: scratch nothing reads back, or an array read back into the caller's memory.  h stays NULL.
template <typename E>
inline hipError_t rows_reserve_device(RowsArray<E>& f, size_t n) {
    if (n <= f.cap) return hipSuccess;
    rows_free(f);
    const hipError_t e = hipMalloc((void**)&f.d, n * sizeof(E));
    if (e == hipSuccess) f.cap = n;
    return e;
}

// Enqueues the copy of the caller's m points (reserved before) to the device.
inline hipError_t rows_upload(RowPoints& f, const nbody_vec2* points, int m, hipStream_t stream) {
    memcpy(f.h, points, (size_t)m * sizeof(FieldPoint));
    return hipMemcpyAsync(f.d, f.h, (size_t)m * sizeof(FieldPoint), hipMemcpyHostToDevice, stream);
}

// The explicit points' velocities of a query that takes them (tides, shell moments), reserved and uploaded like the points.
// *pv: the device array, or NULL for points at rest.
inline int rows_point_vel(const char* who, RowPoints& vel, const nbody_vec2* point_vel, int m, hipStream_t stream,
                          const FieldPoint** pv) {
    *pv = nullptr;
    if (!point_vel || m <= 0) return NBODY_OK;
    const hipError_t e = rows_reserve(vel, (size_t)m);
    if (e != hipSuccess) return rows_alloc_failed(e, who, "point velocities");
    NBK_ROWS_TRY(rows_upload(vel, point_vel, m, stream));
    *pv = vel.d;
    return NBODY_OK;
}

// The buffers of one query with a record per row: the points and the results.
template <typename Out>
struct PointBuffers {
    RowPoints pts;
    RowsArray<Out> out;
};

template <typename Out>
inline void rows_free(PointBuffers<Out>& f) { rows_free(f.pts); rows_free(f.out); }

template <typename Out>
inline int rows_reserve(PointBuffers<Out>& f, size_t n_pts, size_t n_out, const char* who) {
    hipError_t e = rows_reserve(f.pts, n_pts);
    if (e == hipSuccess) e = rows_reserve(f.out, n_out);
    return e == hipSuccess ? NBODY_OK : rows_alloc_failed(e, who, "point and result buffers");
}

// The argument checks every entry point makes before any device call; a query's own value checks stay next to the query.
// `required`: every pointer that must not be NULL; `bytes_per_point`: the caller's result records of all systems per point
// (`of` = " of results") or the point itself (`of` = ""); a query without points passes m = 0.
inline int rows_check_args(const char* who, std::initializer_list<const void*> required, int m, unsigned long long bytes_per_point,
                           const char* of) {
    for (const void* p : required)
        if (!p) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (m < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: m = %d", who, m);
    if ((unsigned long long)m * bytes_per_point > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d points are more than 2^31 bytes%s", who, m, of);
    return NBODY_OK;
}

// What a context or a batch lends a row query, and what every host driver derives from it.  Count says whose: a context
// (RowsOneCount: the exact count, read by the caller just before, goes to the kernel) or a batch (RowsBatchCount: the grid
// covers n_bound rows of every system and the kernel takes each count from Meta).
struct RowsSite {
    hipStream_t stream;
    const void* J;              // device Rec<T> [systems * stride]
    const Meta* meta;           // device [systems]
    Counters* counters;         // device [systems]
    const Meta* h_meta;         // the host's copy [systems], current once read_meta has returned
    int stride, systems;
    int n_bound;                // own rows the grid covers: a context's exact count, a batch's upper bound

    dim3 grid(int rows) const { return dim3((rows + kDiagBlock - 1) / kDiagBlock, systems); }
    template <typename Count>
    int n_one() const { return Count::kBatch ? 0 : n_bound; }
    // The bodies of system sys as the host counts them after read_meta: 0 for a count that failed its check.  A count
    // above n_bound cannot occur - bodies only merge - and its rows past n_bound were never covered by the grid.
    int count(int sys) const {
        const int c = h_meta[sys].n;
        return c < 0 || c > stride || c > n_bound ? 0 : c;
    }
    // read_meta synchronises the stream and reports a device-side failure (a count that failed its check ends there).  A
    // batch calls it even when nothing was launched; a context has read Meta just before.
    template <typename Count, typename ReadMeta>
    int sync(bool launched, ReadMeta read_meta) const { return Count::kBatch || launched ? read_meta() : NBODY_OK; }
};

// One query with q.width() records per row (1: field, neighbours; k: the k nearest), a row's records next to each other on
// the device, from the reservation to the caller's results.
// Q: the query's traits - Device records and the caller's Result, launch<T, kOwn, Count>(grid, stream, out, common kernel
// arguments...), empty(s) and unpack(s, system s's staged records, how many rows, the caller's, system s's first row there).
template <typename T, typename Count, typename Q, typename ReadMeta>
int rows_run(const char* who, const RowsSite& s, PointBuffers<typename Q::Device>& buf, const Q& q, const nbody_vec2* points,
             int m, typename Q::Result* out, ReadMeta read_meta) {
    using Device = typename Q::Device;
    const bool own = points == nullptr;
    const int rows = own ? s.n_bound : m;                                  // what the grid covers
    const size_t width = q.width();
    const size_t per_sys = own ? (size_t)s.stride : (size_t)m;             // rows of one system on the device
    const size_t total = (Count::kBatch ? per_sys * (size_t)s.systems : (size_t)rows) * width;
    for (int sys = 0; sys < s.systems; ++sys) q.empty(sys);
    if (rows > 0) {
        const int rc = rows_reserve(buf, own ? 0 : (size_t)m, total, who);
        if (rc != NBODY_OK) return rc;
        const Rec<T>* J = (const Rec<T>*)s.J;
        if (own) {
            q.template launch<T, true, Count>(s.grid(rows), s.stream, buf.out.d, J, s.meta, s.counters, s.stride,
                                              s.n_one<Count>(), (const FieldPoint*)nullptr, 0);
        } else {
            NBK_ROWS_TRY(rows_upload(buf.pts, points, m, s.stream));
            q.template launch<T, false, Count>(s.grid(rows), s.stream, buf.out.d, J, s.meta, s.counters, s.stride,
                                               s.n_one<Count>(), (const FieldPoint*)buf.pts.d, m);
        }
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(buf.out.h, buf.out.d, total * sizeof(Device), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(rows > 0, read_meta);
    if (rc != NBODY_OK || rows == 0) return rc;
    const Device* h = reinterpret_cast<const Device*>(buf.out.h);
    for (int sys = 0; sys < s.systems; ++sys)
        q.unpack(sys, h + (size_t)sys * per_sys * width, own ? (size_t)s.count(sys) : (size_t)m, out, (size_t)sys * per_sys);
    return NBODY_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The pair-log driver: the host side of a query whose kernel appends one raw record per found pair to a capped log per
// system and counts into one Counts per system (encounters, nbody_encounters.hpp; bound pairs, nbody_binaries.hpp).
// Q: the query's traits, an object that holds the call's value (the horizon, sep2) -
//     Raw, Counts (first member `pairs`), Info (a member `pairs`) and Record, the caller's;  kNoun, for the messages;
//     check_value(who);  launch<T, Count>(grid, stream, J, V, meta, counters, stride, n_one, log, cap, cnt);
//     info(n, counts) -> Info;  finish(raw, pairs, out): the host's O(pairs) part for one system.
// The buffers of one context or batch: the counters on the first call, the log (cap records per system) and its pinned
// staging grown to the largest cap seen.
// ---------------------------------------------------------------------------------------------------------
template <typename Q>
struct PairLogState {
    RowsArray<typename Q::Counts> cnt;      // [systems]: device and pinned
    RowsArray<typename Q::Raw> log;         // [systems * cap]: device and pinned
};

template <typename Q>
inline void pair_log_free(PairLogState<Q>& g) { rows_free(g.cnt); rows_free(g.log); }

template <typename Q>
inline int pair_log_reserve(PairLogState<Q>& g, size_t systems, size_t cap, const char* who) {
    hipError_t e = rows_reserve(g.cnt, systems);
    if (e == hipSuccess) e = rows_reserve(g.log, systems * (cap > 0 ? cap : 1));     // never a NULL log
    if (e == hipSuccess) return NBODY_OK;
    pair_log_free(g);
    return rows_alloc_failed(e, who, "counters and log");
}

// The argument checks an entry point makes before any device call; the value's own check is the query's.
template <typename Q>
inline int pair_log_check_args(const char* who, const void* handle, const Q& q, const typename Q::Record* out, int cap,
                               const typename Q::Info* info, unsigned long long systems) {
    if (!handle || !info) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    const int rc = q.check_value(who);
    if (rc != NBODY_OK) return rc;
    if (cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    if (!out && cap > 0) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL out with cap = %d", who, cap);
    if (systems * (unsigned long long)cap * sizeof(typename Q::Record) > kFieldMaxBytes)
        return nbody_fail(NBODY_ERR_INVALID, "%s: %d %s in each of %llu system(s) are more than 2^31 bytes", who, cap, Q::kNoun, systems);
    return NBODY_OK;
}

// Everything after the first wait of a pair-log call: the counters say whether the log is complete and how much of it to
// read, then the second wait and the host's O(pairs) part.  write_info(sys, n, counts) writes system sys's info record - the
// query's own (pair_log_run) or one with more in it (the binaries on the cell list, nbody_pairs_grid.hpp).  On
// NBODY_ERR_CAPACITY every info is written and out untouched.
template <typename Q, typename WriteInfo>
int pair_log_tail(const char* who, const RowsSite& s, PairLogState<Q>& g, const Q& q, bool launched, typename Q::Record* out, int cap,
                  WriteInfo write_info) {
    using Raw = typename Q::Raw;
    using Counts = typename Q::Counts;
    const Counts* h_cnt = reinterpret_cast<const Counts*>(g.cnt.h);
    int over = -1;
    unsigned long long most = 0;                                 // the pairs of the first system that does not fit
    size_t used = 0;                                             // records of the log up to the last one written
    for (int sys = 0; sys < s.systems; ++sys) {
        const int64_t n = s.count(sys);
        const Counts c = launched && n > 0 ? h_cnt[sys] : Counts{};
        write_info(sys, n, c);
        if (c.pairs > (unsigned long long)cap && over < 0) { over = sys; most = c.pairs; }
        if (c.pairs) used = (size_t)sys * (size_t)cap + (size_t)c.pairs;
    }
    if (!out) return NBODY_OK;                                   // cap == 0: the counts only
    if (over >= 0)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: room for %d %s, system %d has %lld: call again with that cap", who, cap, Q::kNoun,
                          over, (long long)most);
    if (used == 0) return NBODY_OK;
    NBK_ROWS_TRY(hipMemcpyAsync(g.log.h, g.log.d, used * sizeof(Raw), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipStreamSynchronize(s.stream));
    const Raw* raw = reinterpret_cast<const Raw*>(g.log.h);
    for (int sys = 0; sys < s.systems; ++sys) {
        const Counts c = launched && s.count(sys) > 0 ? h_cnt[sys] : Counts{};
        const int fin = q.finish(raw + (size_t)sys * (size_t)cap, (int)c.pairs, out + (size_t)sys * (size_t)cap);
        if (fin != NBODY_OK) return fin;
    }
    return NBODY_OK;
}

// One call, from the reservation to the caller's list; the site, Count and read_meta as for rows_run.  V: the velocities,
// indexed like the site's J.  Two waits: the counters first - they say whether the log is complete and how much of it to
// read - then the records (pair_log_tail).  On NBODY_ERR_CAPACITY info is complete and out untouched.
template <typename T, typename Count, typename Q, typename ReadMeta>
int pair_log_run(const char* who, const RowsSite& s, const void* V, PairLogState<Q>& g, const Q& q, typename Q::Record* out, int cap,
                 typename Q::Info* info, ReadMeta read_meta) {
    using Counts = typename Q::Counts;
    const size_t S = (size_t)s.systems;
    const bool launched = s.n_bound > 0;
    if (launched) {
        const int rc = pair_log_reserve(g, S, (size_t)cap, who);
        if (rc != NBODY_OK) return rc;
        NBK_ROWS_TRY(hipMemsetAsync(g.cnt.d, 0, S * sizeof(Counts), s.stream));
        q.template launch<T, Count>(s.grid(s.n_bound), s.stream, (const Rec<T>*)s.J, (const Vec2<T>*)V, s.meta, s.counters, s.stride,
                                    s.n_one<Count>(), g.log.d, cap, g.cnt.d);
        NBK_ROWS_TRY(hipGetLastError());
        NBK_ROWS_TRY(hipMemcpyAsync(g.cnt.h, g.cnt.d, S * sizeof(Counts), hipMemcpyDeviceToHost, s.stream));
    }
    const int rc = s.sync<Count>(launched, read_meta);
    if (rc != NBODY_OK) return rc;
    return pair_log_tail(who, s, g, q, launched, out, cap, [&](int sys, int64_t n, const Counts& c) { info[sys] = q.info(n, c); });
}

}  // namespace nbk
