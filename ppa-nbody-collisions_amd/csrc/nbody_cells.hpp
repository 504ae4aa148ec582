// csrc/nbody_cells.hpp -- cell sums on the resident state (nbody_get_cells, nbody_batch_get_cells, include/nbody.h;
// DESIGN.md 4.20): for every cell of a caller-given uniform grid the count, the mass, the momentum and twice the kinetic
// energy of the bodies in it, and on request the cell of every body and the CSR cell list (cell offsets, bodies in cell
// order).  The first query about a place instead of a body or a point, and the project's only spatial index: O(n) where every
// row query is O(n^2).  One system (nbody_ctx.hip) and a batch (nbody_batch.hip: system = blockIdx.y, per-body arrays `stride`
// apart, per-cell arrays nx*ny apart, one grid for every system) share each kernel; the count comes from the row queries'
// RowsOneCount / RowsBatchCount (nbody_rows.hpp).
//
// The definition (include/nbody.h has it in full).  IEEE fp64, every operation rounded on its own, no fma.  Body j with the
// record (X, Y, M) and the velocity (VX, VY), widened exactly:
//     tx = (X - x0) * sx;  ty = (Y - y0) * sy
//     inside(j)  <=>  0 <= tx && tx < nx && 0 <= ty && ty < ny          on the doubles; a NaN is outside
//     cell(j) = (int)ty * nx + (int)tx  if inside(j), else -1            converted only after the compares
// and per cell, over its members in ASCENDING j, every accumulator from +0.0:
//     mass = mass + M;  px = px + (M*VX);  py = py + (M*VY);  k2 = k2 + (M*((VX*VX) + (VY*VY)))
// The order is the contract, so no float atomic takes part: the sums run over a cell list that is built on the device with
// integer atomics only and then made independent of the order the waves arrived in.
//
// Five kernels on the handle's stream, no host wait between them, one sync at the end:
//   cells_assign<T, Count>   one lane per body: the cell, cell_of[j], and count[cell] by integer atomicAdd.  Aggregated per
//                            wave: a lane whose predecessor has another cell heads a run, its length is the distance to the
//                            next head (one ballot, one ffs), and only heads issue the atomic, with the run's length.  Bodies
//                            are stored in no spatial order, so on a spread state most runs are one lane; a clump in one
//                            cell gives one atomic per wave: 4096 for 262144 bodies, where one word takes about 88
//                            returning atomics per us.
//   cells_scan<Count>        one workgroup of 1024 lanes per system: the exclusive prefix sum of the counts into start[0 ..
//                            cells], in chunks of 4096 cells (4 consecutive cells per lane, a wave scan by shuffles, the 16
//                            wave totals through LDS, a carry from chunk to chunk; the next chunk's counts are loaded before
//                            the current one is scanned).  Also the info record: n, inside = start[cells], outside, occupied,
//                            largest and the lowest cell that has it (per lane in ascending cells, then one reduction).
//   cells_place<Count>       one lane per body: slot[start[c] + cursor++] = j with the runs of cells_assign - a run's base
//                            from one returning atomic of its head, a lane's offset its distance from the head.  The order
//                            inside a segment is whatever the waves' arrival made it.
//   cells_rank<Count>        one lane per slot e: the entry moves to order[start[c] + #{members of its segment with a
//                            smaller index}]: a counting sort per segment, the same result whatever cells_place left.  The
//                            segments a workgroup's 256 slots belong to are one contiguous range of slots; it is walked
//                            through double-buffered LDS tiles of 1024 indices (one barrier per tile), each lane comparing
//                            against the part of the tile inside its own segment, four indices per ds_read_b128 where the
//                            part is aligned.  Sum of s^2 integer compares over the segment sizes s: at most the n^2 pair
//                            tests of any row query, a few per body on a grid matched to the state.
//   cells_sum<T, Count, kMoments>  one lane per cell.  A cell of fewer than 64 members: the lane walks its segment, four
//                            members' indices and records gathered ahead of their adds (the indices do not depend on the
//                            chain).  A cell of 64 or more: the wave takes its heavy cells one after the other (a ballot);
//                            for each, 64 lanes gather 64 members and form the four terms in parallel into the wave's own
//                            2 KiB of LDS, chain-major, and lane k adds chain k's terms in ascending order: one fp64 add
//                            instruction per member for all four chains, each lane's add waiting for its own previous
//                            one only; the 64 terms of a full gather are read ahead of their adds.  Without kMoments the
//                            velocities are never read and px, py, k2 stay +0.0.
// What every query on the grid shares lives here as well (nbody_within.hpp and nbody_groups_grid.hpp walk the list):
//   CellView, cells_view<Count>   one system's list as a kernel sees it - sys, n, cells, inside (held to [0, n]), the offset of
//                            its per-body arrays and its start: the preamble of every kernel of the family.
//   cells_coords             the cell coordinates (tx, ty): cells_cell sorts by them, the window walk places its window by them.
//   CellRec<T>, cells_gather<T, Count>, cells_gather_run   the list's records {x, y, r, j} in cell order (CellState::sorted),
//                            one lane per slot of `order`, launched after cells_list_run by the queries that walk the list.
//   cells_span, cells_window_walk   the window along one axis, and the one walk over the row-of-cells ranges of a window:
//                            pair(rec) per record, four records loaded ahead.
//   cells_frame_walk         the same walk over integer spans less an inner rectangle already covered (nbody_knn_grid.hpp).
//   cells_block_prefix<V, kBlock>   a workgroup's exclusive prefix (cells_scan here, the row scan of nbody_within.hpp).
//   cells_fine               the host's guard for a grid too fine for the window's proof.
// Every index that comes out of memory (a cell of cell_of, an entry of slot or order, a start) is range-checked before it is
// used as one; by construction none fails.  A batch's count goes through batch_checked_count; cells_assign reports a bad
// one once as kIndexError (rows_prologue), every kernel treats the system as empty.
//
// Cost by counting, n bodies, C cells: assign and place read 16 (32) + 4 bytes and write 4 per body; the scan reads and
// writes 4 C bytes; the rank reads 4 s bytes per member of a segment of s; the sum gathers 16 (32) + 8 (16) bytes per member
// and writes 40 C.  Memset: 8 C bytes.  Results to the host: 40 C bytes, with lists 8 n + 4 C more.
// Measured (profiles/cells_probe.txt; one MI355X, fp32, n = 262144, the stock seeded state, moments and lists, medians of 3
// rounds of a kernel trace): the five kernels 0.084 ms on 256 x 256 cells (assign 0.013, scan 0.040, place 0.014, rank 0.007,
// sum 0.009) and 0.632 ms on 1024 x 1024, of which the one-workgroup scan is 0.578; render_discs 0.009 ms and neighbors_at
// 30.541 ms in the same run.  Every body in one cell of 8 x 8: 8.937 ms (rank 4.796, sum 4.024) against neighbors_at 30.732 ms
// on that state; whole calls 9.52 against 31.42 ms.  With lane 0 alone adding the four chains the sum took 13.525 ms.  A batch
// of 256 x 1024 on 32 x 32 cells: 0.044 ms of kernels, 1.21 ms for StepperBatch.cells() with its lists.
//
// Registers (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; fp32 and fp64 records of a context, fp32
// of a batch: 19 instantiations; VGPRs f32 / f64 for the kernels that read records, SGPRs a context / a batch):
//     kernel                       lanes   VGPRs   SGPRs   scratch   LDS bytes   waves per SIMD
//     cells_assign  f32 / f64       256    10 / 12    26 / 28      0           0           8
//     cells_scan                   1024      59       72 / 74      0         256           8
//     cells_place                   256      12       18 / 26      0           0           8
//     cells_rank                    256      38       37 / 40      0        8192           8
//     cells_sum     no moments      256    36 / 36    33 / 35      0        2112           8
//     cells_sum     moments         256    46 / 48    35 / 37      0        8448           8
//     cells_gather  f32 / f64       256    10 / 14    20 / 20      0           0           8
// No instantiation uses scratch.  (profiles/grid_walk_refactor.txt has every instantiation next to its form before the pieces
// above were shared.)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_grid) == 40, "nbody_grid layout");
static_assert(sizeof(nbody_cell) == 40, "nbody_cell layout");
static_assert(sizeof(nbody_cells_info) == 24, "nbody_cells_info layout");

constexpr int kCellHeavy = kWave;                                // members from which a cell gets the whole wave
constexpr int kCellScanBlock = 1024, kCellScanPer = 4;           // lanes of cells_scan, consecutive cells per lane
constexpr int kCellScanChunk = kCellScanBlock * kCellScanPer;    // cells per trip of the scan
constexpr int kCellTile = 1024;                                  // indices per LDS tile of cells_rank
constexpr unsigned long long kCellsBatchMax = 1ull << 22;        // systems * cells of one batch call

// The body count of system sys as every kernel but cells_assign takes it: a count that fails its check is an empty system.
template <typename Count>
__device__ __forceinline__ int cells_n(const Meta* __restrict__ meta_all, int sys, int stride, int n_one) {
    const int chk = Count::checked(meta_all, sys, stride, n_one);
    return chk < 0 ? 0 : chk;
}

// One system's cell list as a kernel sees it: what every kernel of the grid family starts from.  at: where the system's
// entries begin in a per-body array (cell_of, slot, order, the sorted records, J), so `x_all + cl.at` is the system's x.
// inside: the last start, held to [0, n] - every index a kernel takes from the list is checked against it.
struct CellView {
    int sys, n, cells, inside;
    size_t at;
    const int32_t* __restrict__ start;                           // [cells + 1]
};
// Without a list (cells_scan, which writes it, and the row scan of nbody_within.hpp): sys, n and at only; inside is 0.
template <typename Count>
__device__ __forceinline__ CellView cells_view(const Meta* __restrict__ meta_all, int stride, int n_one, int cells = 0,
                                               const int32_t* __restrict__ start_all = nullptr) {
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int n = cells_n<Count>(meta_all, sys, stride, n_one);
    const int32_t* __restrict__ start = start_all ? start_all + (size_t)sys * (size_t)(cells + 1) : nullptr;
    const int last = start && n > 0 ? start[cells] : 0;
    return CellView{sys, n, cells, last < 0 ? 0 : last > n ? n : last, (size_t)sys * (size_t)stride, start};
}

// The cell coordinates of the definition.  cells_cell sorts a body by them and cells_window_walk places a row's window by
// them: one function, so a body lies in the window around the cell it was sorted into.
struct CellCoords { double tx, ty; };
__device__ __forceinline__ CellCoords cells_coords(const nbody_grid& g, double x, double y) {
    return CellCoords{(x - g.x0) * g.sx, (y - g.y0) * g.sy};
}

// cell(j) of the definition.  The compares are on the doubles; what is converted has passed them (or is +0.0), so no
// value outside [0, nx) or [0, ny) ever reaches a float-to-int conversion.
__device__ __forceinline__ int cells_cell(const nbody_grid& g, double x, double y) {
    const CellCoords t = cells_coords(g, x, y);
    const bool inside = 0.0 <= t.tx && t.tx < (double)g.nx && 0.0 <= t.ty && t.ty < (double)g.ny;
    const int ix = (int)(inside ? t.tx : 0.0), iy = (int)(inside ? t.ty : 0.0);
    return inside ? iy * g.nx + ix : -1;
}

// A workgroup's exclusive prefix over its lanes' values: the lane's offset, and the workgroup's total in every lane.  A
// wave scan by shuffles, the wave totals through wsum (shared, kBlock / kWave entries).  Every lane of the workgroup
// calls it; a caller that calls it again puts a barrier in between, since wsum is written again.
template <typename V> struct BlockPrefix { V at, total; };
template <typename V, int kBlock>
__device__ __forceinline__ BlockPrefix<V> cells_block_prefix(V mine, V* wsum) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    V x = mine;                                                  // inclusive over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const V y = __shfl_up(x, d, kWave);
        if (lane >= d) x += y;
    }
    if (lane == kWave - 1) wsum[wave] = x;
    __syncthreads();
    V before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
        const V t = wsum[w];
        before += w < wave ? t : 0;
        total += t;
    }
    return BlockPrefix<V>{before + x - mine, total};
}

// The runs of equal cells along a wave's lanes: a lane heads a run where its predecessor holds another cell (lane 0 always
// does).  head_lane: the head of this lane's run; len: for a head, the lanes of its run.  Every lane of the wave calls it.
struct CellRun { int head_lane, len; bool head; };
__device__ __forceinline__ CellRun cells_wave_runs(int c) {
    const int lane = threadIdx.x & (kWave - 1);
    const int prev = __shfl_up(c, 1, kWave);
    const bool head = lane == 0 || prev != c;
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & (~0ull >> (kWave - 1 - lane));       // bit 0 is set: lane 0 is a head
    const int head_lane = kWave - 1 - __clzll((long long)upto);
    const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const int next = above ? lane + __ffsll((unsigned long long)above) : kWave;  // ffs is 1-based
    return CellRun{head_lane, next - lane, head};
}

// grid and early exits: rows_prologue (own rows).  count_all: [systems * cells], zero at the launch.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void cells_assign(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                           Counters* __restrict__ ctr_all, int stride, int n_one,
                                                           const nbody_grid g, int32_t* __restrict__ cell_of_all,
                                                           unsigned* __restrict__ count_all) {
    RowsLane<T, int32_t> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, cell_of_all, (int32_t)-1)) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    int c = -1;                                                  // a lane without a row: a run of its own kind, no atomic
    if (L.valid) {
        const Rec<T> r = L.J[L.p];
        c = cells_cell(g, (double)r.x, (double)r.y);
        L.out[L.p] = c;
    }
    const CellRun run = cells_wave_runs(c);
    if (run.head && c >= 0) atomicAdd(count_all + (size_t)sys * (size_t)(g.nx * g.ny) + (size_t)c, (unsigned)run.len);
}

// One workgroup per system.  start_all: [systems * (cells + 1)].
template <typename Count>
__global__ __launch_bounds__(kCellScanBlock) void cells_scan(const Meta* __restrict__ meta_all, int stride, int n_one, int cells,
                                                             const unsigned* __restrict__ count_all,
                                                             int32_t* __restrict__ start_all,
                                                             nbody_cells_info* __restrict__ info_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one);
    const int sys = cl.sys, n = cl.n;
    const unsigned* __restrict__ count = count_all + (size_t)sys * (size_t)cells;
    int32_t* __restrict__ start = start_all + (size_t)sys * (size_t)(cells + 1);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kCellScanBlock / kWave;
    __shared__ int wsum[kWaves];
    __shared__ int r_occ[kWaves], r_best[kWaves], r_cell[kWaves];
    int carry = 0, occupied = 0, best = -1, best_cell = 0;
    int v[kCellScanPer], nv[kCellScanPer];
#pragma unroll
    for (int u = 0; u < kCellScanPer; ++u) {
        const int c = tid * kCellScanPer + u;
        nv[u] = c < cells ? (int)count[c] : 0;
    }
    for (int base = 0; base < cells; base += kCellScanChunk) {
        const int c0 = base + tid * kCellScanPer;
        int mine = 0;
#pragma unroll
        for (int u = 0; u < kCellScanPer; ++u) { v[u] = nv[u]; mine += v[u]; }
#pragma unroll
        for (int u = 0; u < kCellScanPer; ++u) {                 // the next chunk's, ahead of this chunk's scan
            const long long c = (long long)c0 + kCellScanChunk + u;
            nv[u] = c < cells ? (int)count[c] : 0;
        }
        const BlockPrefix<int> p = cells_block_prefix<int, kCellScanBlock>(mine, wsum);
        int at = carry + p.at;
#pragma unroll
        for (int u = 0; u < kCellScanPer; ++u) {
            if (c0 + u < cells) {
                start[c0 + u] = at;
                occupied += v[u] > 0 ? 1 : 0;
                if (v[u] > best) { best = v[u]; best_cell = c0 + u; }            // ascending cells: the lowest stays
                at += v[u];
            }
        }
        carry += p.total;
        __syncthreads();                                         // wsum is written again in the next trip
    }
    if (tid == 0) start[cells] = carry;
    // occupied: a sum; (best, best_cell): the larger count, then the lower cell
#pragma unroll
    for (int sh = kWave / 2; sh > 0; sh >>= 1) {
        occupied += __shfl_down(occupied, sh, kWave);
        const int ob = __shfl_down(best, sh, kWave), oc = __shfl_down(best_cell, sh, kWave);
        if (ob > best || (ob == best && oc < best_cell)) { best = ob; best_cell = oc; }
    }
    if (lane == 0) { r_occ[wave] = occupied; r_best[wave] = best; r_cell[wave] = best_cell; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w) {
            occupied += r_occ[w];
            if (r_best[w] > best || (r_best[w] == best && r_cell[w] < best_cell)) { best = r_best[w]; best_cell = r_cell[w]; }
        }
        info_all[sys] = nbody_cells_info{n, carry, n - carry, occupied, best < 0 ? 0 : best, best_cell};
    }
}

// One lane per body.  cursor_all: [systems * cells], zero at the launch; slot_all: [systems * stride].
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void cells_place(const Meta* __restrict__ meta_all, int stride, int n_one, int cells,
                                                          const int32_t* __restrict__ cell_of_all,
                                                          const int32_t* __restrict__ start_all, unsigned* __restrict__ cursor_all,
                                                          int32_t* __restrict__ slot_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, cells, start_all);
    if ((int)(blockIdx.x * kDiagBlock) >= cl.n) return;          // the whole workgroup
    const int j = blockIdx.x * kDiagBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int c = j < cl.n ? cell_of_all[cl.at + j] : -1;
    if ((unsigned)c >= (unsigned)cells) c = -1;
    const CellRun run = cells_wave_runs(c);
    unsigned base = 0;
    if (run.head && c >= 0) base = atomicAdd(cursor_all + (size_t)cl.sys * (size_t)cells + (size_t)c, (unsigned)run.len);
    base = __shfl(base, run.head_lane, kWave);
    if (c >= 0) {
        const long long pos = (long long)cl.start[c] + base + (lane - run.head_lane);
        if (pos >= 0 && pos < cl.n) slot_all[cl.at + pos] = j;
    }
}

// One lane per slot.  order_all: [systems * stride].
template <typename Count>
__global__ __launch_bounds__(kDiagBlock) void cells_rank(const Meta* __restrict__ meta_all, int stride, int n_one, int cells,
                                                         const int32_t* __restrict__ cell_of_all,
                                                         const int32_t* __restrict__ start_all,
                                                         const int32_t* __restrict__ slot_all, int32_t* __restrict__ order_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, cells, start_all);
    const int32_t* __restrict__ cell_of = cell_of_all + cl.at;
    const int32_t* __restrict__ slot = slot_all + cl.at;
    const int inside = cl.inside;
    const int e0 = blockIdx.x * kDiagBlock, tid = threadIdx.x;
    if (e0 >= inside) return;                                    // the whole workgroup, before any barrier
    // a slot's index, cell and segment; nothing that fails its check becomes an index
    const auto segment = [&](int e, int& idx, int& s0, int& s1) {
        idx = slot[e];
        s0 = s1 = 0;
        if ((unsigned)idx >= (unsigned)cl.n) return false;
        const int c = cell_of[idx];
        if ((unsigned)c >= (unsigned)cells) return false;
        s0 = cl.start[c]; s1 = cl.start[c + 1];
        if (s0 < 0 || s1 > inside || s0 > s1) { s0 = s1 = 0; return false; }
        return true;
    };
    // the slots this workgroup's segments span: from the first slot's segment to the last one's (workgroup-uniform)
    const int e_last = e0 + kDiagBlock - 1 < inside - 1 ? e0 + kDiagBlock - 1 : inside - 1;
    int idx, lo, hi, s0, s1;
    segment(e0, idx, lo, s1);
    segment(e_last, idx, s0, hi);
    const int e = e0 + tid;
    const bool valid = e < inside && segment(e, idx, s0, s1);
    if (!valid) { idx = 0; s0 = s1 = 0; }
    __shared__ __attribute__((aligned(16))) int32_t tile[2][kCellTile];
    int rank = 0;
    const int tiles = hi > lo ? (hi - lo + kCellTile - 1) / kCellTile : 0;
    for (int t = 0; t < tiles; ++t) {
        const int b = t & 1;
        const int g0 = lo + t * kCellTile;
        const int cnt = hi - g0 < kCellTile ? hi - g0 : kCellTile;
#pragma unroll
        for (int u = 0; u < kCellTile / kDiagBlock; ++u) {
            const int k = tid + u * kDiagBlock;
            if (k < cnt) tile[b][k] = slot[g0 + k];
        }
        // buffer b was last read in tile t-2: every lane has passed tile t-1's barrier since
        __syncthreads();
        int k = (s0 > g0 ? s0 : g0) - g0;                        // the part of the tile inside the lane's segment
        const int end = (s1 < g0 + cnt ? s1 : g0 + cnt) - g0;
        for (; k < end && (k & 3); ++k) rank += tile[b][k] < idx ? 1 : 0;
        for (; k + 4 <= end; k += 4) {
            const int4 q = *reinterpret_cast<const int4*>(&tile[b][k]);
            rank += (q.x < idx ? 1 : 0) + (q.y < idx ? 1 : 0) + (q.z < idx ? 1 : 0) + (q.w < idx ? 1 : 0);
        }
        for (; k < end; ++k) rank += tile[b][k] < idx ? 1 : 0;
    }
    if (valid && s0 + rank < s1) order_all[cl.at + s0 + rank] = idx;
}

// A source in cell order: what a walk over the list reads instead of an index and a record per pair.
template <typename T> struct CellRec;
template <> struct alignas(16) CellRec<float> { float x, y, r; int j; };
template <> struct alignas(32) CellRec<double> { double x, y, r; int j; };
static_assert(sizeof(CellRec<float>) == 16 && sizeof(CellRec<double>) == 32, "a record is one 16 or 32 byte load");

// One lane per slot of `order`: the record {x, y, r, j} into sorted_all ([systems * stride]), in cell order.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void cells_gather(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                           int stride, int n_one, int cells,
                                                           const int32_t* __restrict__ start_all,
                                                           const int32_t* __restrict__ order_all,
                                                           CellRec<T>* __restrict__ sorted_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, cells, start_all);
    const int e = blockIdx.x * kDiagBlock + threadIdx.x;
    if (e >= cl.inside) return;
    const int idx = order_all[cl.at + e];
    CellRec<T> w{(T)__builtin_nan(""), (T)0, (T)0, 0};            // an entry that fails its check: d2 = NaN, never near
    if ((unsigned)idx < (unsigned)cl.n) {
        const Rec<T> r = J_all[cl.at + idx];
        w = CellRec<T>{r.x, r.y, r.r, idx};
    }
    sorted_all[cl.at + e] = w;
}

// The window along one axis around the cell coordinate t, w0 cells to either side and a margin (DESIGN.md 4.21 has the
// rule and its proof): cells lo .. hi, hi < lo for none.
struct CellSpan { int lo, hi; };
__device__ __forceinline__ CellSpan cells_span(double t, double w0, int cells) {
    const double w = w0 + (0x1p-20 + (fabs(t) + w0) * 0x1p-40);
    const double lo = t - w, hi = t + w;
    if (!(fabs(t) < __builtin_inf()) || lo != lo || hi != hi) return CellSpan{0, cells - 1};
    if (hi < 0.0 || lo >= (double)cells) return CellSpan{0, -1};
    // lo < cells and hi >= 0: what is converted lies in [0, cells)
    return CellSpan{lo > 0.0 ? (int)lo : 0, hi < (double)(cells - 1) ? (int)hi : cells - 1};
}

// The one walk over the cells around a place: pair(rec) for every sorted record of the window around the cell coordinates
// (tx, ty) of cells_coords, wx0 and wy0 cells wide to either side.  The grid is row-major, so the members of columns lo .. hi
// of one row of cells are ONE contiguous range of the sorted records, start[yy * nx + lo] .. start[yy * nx + hi + 1]; a range
// that fails its check is skipped; four records are loaded ahead of their pairs.
template <typename T, typename Pair>
__device__ __forceinline__ void cells_window_walk(const CellView& cl, const CellRec<T>* __restrict__ sorted, const nbody_grid& g,
                                                  double tx, double ty, double wx0, double wy0, Pair pair) {
    const CellSpan cx = cells_span(tx, wx0, g.nx), cy = cells_span(ty, wy0, g.ny);
    if (cx.lo > cx.hi) return;
    for (int yy = cy.lo; yy <= cy.hi; ++yy) {
        const int a = cl.start[yy * g.nx + cx.lo], b = cl.start[yy * g.nx + cx.hi + 1];
        if (a < 0 || b > cl.inside || a >= b) continue;
        for (int k = a; k < b; k += 4) {                         // four loads ahead of their pairs
            CellRec<T> s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = sorted[k + u < b ? k + u : b - 1];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k + u < b) pair(s[u]);
        }
    }
}

// The walk over a window given by its integer spans, less an inner rectangle that an earlier walk has covered: pair(rec) for
// every sorted record of the cells of cx x cy that do not lie in ix x iy.  The inner spans lie inside the outer ones, or one
// of them is empty (hi < lo) and nothing is left out.  Per row of cells that is one contiguous range of the sorted records
// where the inner rectangle does not reach the row, and at most two where it does: columns cx.lo .. ix.lo - 1 and
// ix.hi + 1 .. cx.hi.  Ranges and records are checked and loaded as in cells_window_walk.  The k nearest on the list
// (nbody_knn_grid.hpp) widen a row's window with it: no record is handed over twice.
template <typename T, typename Pair>
__device__ __forceinline__ void cells_frame_walk(const CellView& cl, const CellRec<T>* __restrict__ sorted, const nbody_grid& g,
                                                 CellSpan cx, CellSpan cy, CellSpan ix, CellSpan iy, Pair pair) {
    if (cx.lo > cx.hi) return;
    const bool hole = ix.lo <= ix.hi && iy.lo <= iy.hi;
    for (int yy = cy.lo; yy <= cy.hi; ++yy) {
        const bool cut = hole && iy.lo <= yy && yy <= iy.hi;
        for (int part = 0; part < (cut ? 2 : 1); ++part) {
            const int c0 = part == 0 ? cx.lo : ix.hi + 1, c1 = cut && part == 0 ? ix.lo - 1 : cx.hi;
            if (c0 > c1) continue;
            const int a = cl.start[yy * g.nx + c0], b = cl.start[yy * g.nx + c1 + 1];
            if (a < 0 || b > cl.inside || a >= b) continue;
            for (int k = a; k < b; k += 4) {                     // four loads ahead of their pairs
                CellRec<T> s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = sorted[k + u < b ? k + u : b - 1];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < b) pair(s[u]);
            }
        }
    }
}

// One member's terms, widened exactly; kMoments: with the velocity.
struct CellTerms { double m, px, py, k2; };
template <typename T, bool kMoments>
__device__ __forceinline__ CellTerms cells_terms(const Rec<T>* __restrict__ J, const Vec2<T>* __restrict__ V, int idx) {
    CellTerms t{(double)J[idx].m, 0.0, 0.0, 0.0};
    if constexpr (kMoments) {
        const Vec2<T> v = V[idx];
        const double vx = (double)v.x, vy = (double)v.y;
        t.px = t.m * vx;
        t.py = t.m * vy;
        t.k2 = t.m * ((vx * vx) + (vy * vy));
    }
    return t;
}

// One lane per cell; V_all is not read without kMoments.  cells_all: [systems * cells].
template <typename T, typename Count, bool kMoments>
__global__ __launch_bounds__(kDiagBlock) void cells_sum(const Rec<T>* __restrict__ J_all, const Vec2<T>* __restrict__ V_all,
                                                        const Meta* __restrict__ meta_all, int stride, int n_one, int cells,
                                                        const int32_t* __restrict__ start_all,
                                                        const int32_t* __restrict__ order_all, nbody_cell* __restrict__ cells_all) {
    const CellView cl = cells_view<Count>(meta_all, stride, n_one, cells, start_all);
    const int n = cl.n;
    const Rec<T>* __restrict__ J = J_all + cl.at;
    const Vec2<T>* __restrict__ V = kMoments ? V_all + cl.at : nullptr;
    const int32_t* __restrict__ order = order_all + cl.at;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int c = blockIdx.x * kDiagBlock + tid;
    const bool live = c < cells;
    int s0 = 0, cnt = 0;
    if (live && n > 0) {
        s0 = cl.start[c];
        cnt = cl.start[c + 1] - s0;
        if (s0 < 0 || cnt < 0 || s0 > n || cnt > n - s0) { s0 = 0; cnt = 0; }
    }
    // an entry of the list as an index into J and V
    const auto member = [&](int k) {
        const int idx = order[k];
        return (unsigned)idx < (unsigned)n ? idx : 0;
    };
    double mass = 0.0, px = 0.0, py = 0.0, k2 = 0.0;
    const int first = cnt > 0 ? member(s0) : -1;
    if (cnt < kCellHeavy) {
        for (int k = 0; k < cnt; k += 4) {                       // four gathers ahead of their adds
            CellTerms t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = cells_terms<T, kMoments>(J, V, member(s0 + (k + u < cnt ? k + u : cnt - 1)));
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
                    mass = mass + t[u].m;
                    if constexpr (kMoments) { px = px + t[u].px; py = py + t[u].py; k2 = k2 + t[u].k2; }
                }
            }
        }
    }
    // the wave's heavy cells, one after the other: 64 lanes gather and multiply into the wave's own LDS, chain-major (a row
    // of 66 doubles per chain: the rows of lanes 0 .. 3 start 4 banks apart); lane k adds chain k's 64 terms in ascending
    // order - one instruction per member for the four chains, each lane's add waiting only for its own previous one
    constexpr int kChains = kMoments ? 4 : 1;
    __shared__ __attribute__((aligned(16))) double terms[kDiagBlock / kWave][kChains][kWave + 2];
    unsigned long long heavy = __ballot(cnt >= kCellHeavy);
    while (heavy) {
        const int src = __ffsll(heavy) - 1;
        heavy &= heavy - 1;
        const int h0 = __shfl(s0, src, kWave), hn = __shfl(cnt, src, kWave);
        double acc = 0.0;                                        // lane k < kChains: chain k of the cell
        const double* __restrict__ mine = terms[wave][lane < kChains ? lane : 0];
        for (int base = 0; base < hn; base += kWave) {
            const int m = hn - base < kWave ? hn - base : kWave;
            if (lane < m) {
                const CellTerms t = cells_terms<T, kMoments>(J, V, member(h0 + base + lane));
                terms[wave][0][lane] = t.m;
                if constexpr (kMoments) { terms[wave][1][lane] = t.px; terms[wave][2][lane] = t.py; terms[wave][3][lane] = t.k2; }
            }
            // the wave's own LDS: its DS operations complete in order, the fence keeps the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane < kChains) {
                if (m == kWave) {                                // the terms read ahead of the adds
#pragma unroll
                    for (int q = 0; q < kWave; ++q) acc = acc + mine[q];
                } else {
                    for (int q = 0; q < m; ++q) acc = acc + mine[q];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const double a0 = __shfl(acc, 0, kWave);
        double a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if constexpr (kMoments) { a1 = __shfl(acc, 1, kWave); a2 = __shfl(acc, 2, kWave); a3 = __shfl(acc, 3, kWave); }
        if (lane == src) { mass = a0; px = a1; py = a2; k2 = a3; }
    }
    if (live) cells_all[(size_t)cl.sys * (size_t)cells + c] = nbody_cell{mass, px, py, k2, cnt, first};
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The buffers of one context or batch: nothing before the first call, grown to the largest grid seen; the
// per-body arrays depend on systems * stride only.
// ---------------------------------------------------------------------------------------------------------
struct CellState {
    RowsArray<nbody_cell> cells;        // [systems * cells]: device and pinned
    RowsArray<int32_t> start;           // [systems * (cells + 1)]
    RowsArray<int32_t> cell_of, order;  // [systems * stride]
    RowsArray<nbody_cells_info> info;   // [systems]
    RowsArray<unsigned> words;          // device [2][systems * cells]: the counts, then the cursors of cells_place
    RowsArray<int32_t> slot;            // device [systems * stride]: the list as cells_place leaves it
    RowsArray<unsigned char> sorted;    // device [systems * stride] CellRec<T>: the list's records, for the queries that walk it
};

inline void cells_free(CellState& g) {
    rows_free(g.cells); rows_free(g.start); rows_free(g.cell_of); rows_free(g.order); rows_free(g.info); rows_free(g.words);
    rows_free(g.slot); rows_free(g.sorted);
}

// rec_bytes: 0 for the cell sums, which need the cell records; sizeof(CellRec<T>) for a query that walks the list
// (nbody_within.hpp, nbody_groups_grid.hpp), which needs the sorted records instead.
inline int cells_reserve(CellState& g, size_t systems, size_t cells, size_t bodies, const char* who, size_t rec_bytes = 0) {
    hipError_t e = rec_bytes ? rows_reserve_device(g.sorted, (bodies > 0 ? bodies : 1) * rec_bytes) : rows_reserve(g.cells, systems * cells);
    if (e == hipSuccess) e = rows_reserve(g.start, systems * (cells + 1));
    if (e == hipSuccess) e = rows_reserve(g.cell_of, bodies > 0 ? bodies : 1);
    if (e == hipSuccess) e = rows_reserve(g.order, bodies > 0 ? bodies : 1);
    if (e == hipSuccess) e = rows_reserve(g.info, systems);
    if (e == hipSuccess) e = rows_reserve_device(g.words, 2 * systems * cells);
    if (e == hipSuccess) e = rows_reserve_device(g.slot, bodies > 0 ? bodies : 1);
    if (e == hipSuccess) return NBODY_OK;
    cells_free(g);
    return rows_alloc_failed(e, who, "cell buffers");
}

// The argument checks an entry point makes before any device call, the values before the handle so that each can be seen
// without one; `required`: the handle and every other pointer that must not be NULL.  cap is the room of the lists, looked
// at only where one is asked for; whether it holds the bodies is for the caller, who knows their count.
inline int cells_check_args(const char* who, std::initializer_list<const void*> required, const nbody_grid* grid, uint32_t flags,
                            const int32_t* cell_of, const int32_t* start, const int32_t* order, int cap,
                            unsigned long long systems) {
    static_assert((unsigned long long)NBODY_CELLS_MAX <= kCellsBatchMax, "a single system's grid passes the batch bound");
    if (!grid) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL grid", who);
    if (grid->nx < 1 || grid->ny < 1 || (long long)grid->nx * (long long)grid->ny > (long long)NBODY_CELLS_MAX)
        return nbody_fail(NBODY_ERR_INVALID, "%s: a grid of %d x %d cells (each >= 1, at most %d in all)", who, grid->nx, grid->ny,
                          NBODY_CELLS_MAX);
    const unsigned long long cells = (unsigned long long)grid->nx * (unsigned long long)grid->ny;
    if (systems * cells > kCellsBatchMax)
        return nbody_fail(NBODY_ERR_CAPACITY, "%s: %llu systems of %llu cells are more than %llu cells in all", who, systems, cells,
                          kCellsBatchMax);
    const double inf = __builtin_inf();
    if (!(grid->x0 > -inf && grid->x0 < inf && grid->y0 > -inf && grid->y0 < inf))
        return nbody_fail(NBODY_ERR_INVALID, "%s: origin (%g, %g) is not finite", who, grid->x0, grid->y0);
    if (!(grid->sx > 0.0 && grid->sx < inf && grid->sy > 0.0 && grid->sy < inf))
        return nbody_fail(NBODY_ERR_INVALID, "%s: (%g, %g) cells per unit length (finite and > 0)", who, grid->sx, grid->sy);
    if (flags & ~(uint32_t)NBODY_CELLS_MOMENTS) return nbody_fail(NBODY_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
    if (order && !start) return nbody_fail(NBODY_ERR_INVALID, "%s: order without start", who);
    if ((cell_of || order) && cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    return rows_check_args(who, required, 0, 0, "");
}

// The list stages on the site's stream, no wait: the memset of the counts and cursors, cells_assign, cells_scan, cells_place
// and cells_rank.  Leaves g.cell_of, g.start, g.order and g.info on the device; g is reserved by the caller.  What the cell
// sums, the radius queries (nbody_within.hpp) and the groups on the grid (nbody_groups_grid.hpp) run first.
template <typename T, typename Count>
int cells_list_run(const RowsSite& s, CellState& g, const nbody_grid& grid) {
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny;
    const int cells = (int)C;
    const Rec<T>* J = (const Rec<T>*)s.J;
    const int n_one = s.n_one<Count>();
    unsigned* count = g.words.d;
    unsigned* cursor = g.words.d + S * C;
    const dim3 per_body = s.grid(s.n_bound);
    NBK_ROWS_TRY(hipMemsetAsync(g.words.d, 0, 2 * S * C * sizeof(unsigned), s.stream));
    if (s.n_bound > 0) {
        hipLaunchKernelGGL((cells_assign<T, Count>), per_body, dim3(kDiagBlock), 0, s.stream, J, s.meta, s.counters, s.stride,
                           n_one, grid, g.cell_of.d, count);
        NBK_ROWS_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((cells_scan<Count>), dim3(1, (unsigned)S), dim3(kCellScanBlock), 0, s.stream, s.meta, s.stride, n_one,
                       cells, (const unsigned*)count, g.start.d, g.info.d);
    NBK_ROWS_TRY(hipGetLastError());
    if (s.n_bound > 0) {
        hipLaunchKernelGGL((cells_place<Count>), per_body, dim3(kDiagBlock), 0, s.stream, s.meta, s.stride, n_one, cells,
                           (const int32_t*)g.cell_of.d, (const int32_t*)g.start.d, cursor, g.slot.d);
        NBK_ROWS_TRY(hipGetLastError());
        hipLaunchKernelGGL((cells_rank<Count>), per_body, dim3(kDiagBlock), 0, s.stream, s.meta, s.stride, n_one, cells,
                           (const int32_t*)g.cell_of.d, (const int32_t*)g.start.d, (const int32_t*)g.slot.d, g.order.d);
        NBK_ROWS_TRY(hipGetLastError());
    }
    return NBODY_OK;
}

// After cells_list_run, on the same stream, no wait: cells_gather into g.sorted.  A function of its own: the cell sums do not
// read the records, and their entry point must not name the kernel.
template <typename T, typename Count>
int cells_gather_run(const RowsSite& s, CellState& g, const nbody_grid& grid) {
    if (s.n_bound <= 0) return NBODY_OK;
    hipLaunchKernelGGL((cells_gather<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Rec<T>*)s.J, s.meta,
                       s.stride, s.n_one<Count>(), grid.nx * grid.ny, (const int32_t*)g.start.d, (const int32_t*)g.order.d,
                       reinterpret_cast<CellRec<T>*>(g.sorted.d));
    NBK_ROWS_TRY(hipGetLastError());
    return NBODY_OK;
}

// A grid too fine for the proof of the window's margin (more than 2^400 cells per unit length: dx*dx can underflow for
// bodies many cells apart): a walk over it looks at every cell.
inline bool cells_fine(const nbody_grid& grid) { return !(grid.sx <= 0x1p400 && grid.sy <= 0x1p400); }

// One call, from the reservation to the caller's arrays; the site, Count and read_meta as for rows_run (nbody_rows.hpp).
// V: the velocities, indexed like the site's J, read only with NBODY_CELLS_MOMENTS.  A list the caller did not ask for is
// built all the same - the sums run over it - and not copied.
template <typename T, typename Count, typename ReadMeta>
int cells_run(const char* who, const RowsSite& s, CellState& g, const void* V, const nbody_grid& grid, uint32_t flags,
              nbody_cell* cells_out, int32_t* cell_of, int32_t* start, int32_t* order, nbody_cells_info* info, ReadMeta read_meta) {
    const size_t S = (size_t)s.systems, C = (size_t)grid.nx * (size_t)grid.ny, bodies = S * (size_t)s.stride;
    const int cells = (int)C;
    int rc = cells_reserve(g, S, C, bodies, who);
    if (rc != NBODY_OK) return rc;
    const Rec<T>* J = (const Rec<T>*)s.J;
    const int n_one = s.n_one<Count>();
    const dim3 per_cell((unsigned)((C + kDiagBlock - 1) / kDiagBlock), (unsigned)S);
    if ((rc = cells_list_run<T, Count>(s, g, grid)) != NBODY_OK) return rc;
    if (flags & NBODY_CELLS_MOMENTS)
        hipLaunchKernelGGL((cells_sum<T, Count, true>), per_cell, dim3(kDiagBlock), 0, s.stream, J, (const Vec2<T>*)V, s.meta,
                           s.stride, n_one, cells, (const int32_t*)g.start.d, (const int32_t*)g.order.d, g.cells.d);
    else
        hipLaunchKernelGGL((cells_sum<T, Count, false>), per_cell, dim3(kDiagBlock), 0, s.stream, J, (const Vec2<T>*)nullptr,
                           s.meta, s.stride, n_one, cells, (const int32_t*)g.start.d, (const int32_t*)g.order.d, g.cells.d);
    NBK_ROWS_TRY(hipGetLastError());
    // to the pinned staging: the records and the info always, a list where the caller asked for it and a system can hold a body
    const size_t listed = Count::kBatch ? bodies : (size_t)s.n_bound;
    NBK_ROWS_TRY(hipMemcpyAsync(g.cells.h, g.cells.d, S * C * sizeof(nbody_cell), hipMemcpyDeviceToHost, s.stream));
    NBK_ROWS_TRY(hipMemcpyAsync(g.info.h, g.info.d, S * sizeof(nbody_cells_info), hipMemcpyDeviceToHost, s.stream));
    if (start) NBK_ROWS_TRY(hipMemcpyAsync(g.start.h, g.start.d, S * (C + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    if (cell_of && s.n_bound > 0)
        NBK_ROWS_TRY(hipMemcpyAsync(g.cell_of.h, g.cell_of.d, listed * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    if (order && s.n_bound > 0)
        NBK_ROWS_TRY(hipMemcpyAsync(g.order.h, g.order.d, listed * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    rc = s.sync<Count>(true, read_meta);
    if (rc != NBODY_OK) return rc;
    memcpy(cells_out, g.cells.h, S * C * sizeof(nbody_cell));
    memcpy(info, g.info.h, S * sizeof(nbody_cells_info));
    if (start) memcpy(start, g.start.h, S * (C + 1) * sizeof(int32_t));
    const int32_t* h_cell_of = reinterpret_cast<const int32_t*>(g.cell_of.h);
    const int32_t* h_order = reinterpret_cast<const int32_t*>(g.order.h);
    for (size_t sys = 0; sys < S; ++sys) {                       // a system's n cells and `inside` entries; the rest stays
        const size_t at = sys * (size_t)s.stride;
        const int n = info[sys].n, inside = info[sys].inside;
        if (cell_of && n > 0 && n <= s.n_bound) memcpy(cell_of + at, h_cell_of + at, (size_t)n * sizeof(int32_t));
        if (order && inside > 0 && inside <= n && n <= s.n_bound) memcpy(order + at, h_order + at, (size_t)inside * sizeof(int32_t));
    }
    return NBODY_OK;
}

}  // namespace nbk
