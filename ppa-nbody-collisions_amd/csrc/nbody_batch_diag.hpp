// csrc/nbody_batch_diag.hpp -- per-system diagnostics of a batch (nbody_batch_diagnostics, nbody_batch_diag_record,
// include/nbody.h; DESIGN.md 4.5 "Diagnostics"): what nbody_get_diagnostics returns for an nbody_ctx holding system s,
// bit for bit, for every system of the batch in two launches, whatever S is.  Included by nbody_batch.hip after
// nbody_batch_kernels.hpp.
//
// The order contract is the one of nbody_diag.hpp, and its code is called, not restated: phi_i is
// diag_walk's running fma chain over j = 0, 1, ..., n-1 (diag_row_general for a flagged row); the totals are summed per
// aligned 128-body tile with rows ascending, then over the tiles ascending by diag_add, and finished by diag_finish (mx /
// mass, 0.5 * K2, 0.5 * pot), the two functions nbody_get_diagnostics runs on the host.  A system is a rank that owns
// everything (lo = 0, cnt = n).
//
// The system index is blockIdx.y.  Grids are sized from the largest uploaded count; each kernel takes the exact count
// from the system's Meta through batch_checked_count, workgroups past it leave at once (as whole workgroups, before the
// first barrier), a count outside [0, stride] is treated as 0 and batch_diag_reduce adds kIndexError to the system's
// Counters::errors.
//
// batch_diag_potential: diag_potential on the system's slice of J.  What differs: the phi store is optional (kPhi:
// a record and a call without `phi` keep no per-body values), and the per-tile epilogue also sums the moments of
// diag_moments - every lane forms the seven products of its own row (the very expressions of diag_moments, velocities
// from the batch's V) and leaves them in LDS, and nine lanes per row tile each add one quantity over the tile's rows in
// ascending order.  The sums are the same chains as diag_moments' sequential walk (each starts from +0 and adds the
// rounded products one by one), so the bits are the same, and the separate moments launch is gone.
//
// batch_diag_reduce: one lane per system adds the system's tiles in ascending order and writes the finished 88-byte
// record straight into the output row (the caller's device buffer, or a row of the recorded series).
#pragma once
#include <stddef.h>

#include "nbody_batch_kernels.hpp"
#include "nbody_diag.hpp"

#pragma clang fp contract(off)

namespace nbk {

constexpr int kDiagSums = 8;                  // the doubles of a DiagTile, in its order: mass px py mx my L K2 pot
static_assert(offsetof(DiagTile, pot) == 7 * sizeof(double) && offsetof(DiagTile, coincident) == 8 * sizeof(double),
              "the epilogue stores a DiagTile's sums by index");

__host__ __device__ constexpr int batch_diag_tiles(int stride) { return (stride + kTile - 1) / kTile; }

template <bool kPhi>
__global__ __launch_bounds__(kDiagBlock) void batch_diag_potential(const Rec<float>* __restrict__ J_all,
                                                                   const Vec2<float>* __restrict__ V_all,
                                                                   const Meta* __restrict__ meta_all, int stride, double G,
                                                                   double* __restrict__ phi_all,
                                                                   DiagTile* __restrict__ tiles_all) {
    __shared__ double wsum[kDiagSums][kDiagBlock];
    __shared__ long long wcoin[kDiagBlock];
    const int sys = blockIdx.y;
    const int chk = batch_checked_count(meta_all[sys].n, stride);
    const int n = chk < 0 ? 0 : chk;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * kDiagBlock;                    // first row of the workgroup
    if (row0 >= n) return;                                       // the whole workgroup, before any barrier
    const size_t base = (size_t)sys * (size_t)stride;
    const Rec<float>* __restrict__ J = J_all + base;
    const int i = row0 + tid;                                    // row of this lane
    const bool valid = i < n;
    double xi = 0.0, yi = 0.0, mi = 0.0, vx = 0.0, vy = 0.0;
    if (valid) {
        const Rec<float> r = J[i];
        const Vec2<float> v = V_all[base + i];
        xi = (double)r.x; yi = (double)r.y; mi = (double)r.m;
        vx = (double)v.x; vy = (double)v.y;
    }
    // tile of this wave's rows: the one j tile that holds their self terms
    double acc = diag_walk<false>(J, n, i, xi, yi, (row0 + (tid & ~(kWave - 1))) / kTile);
    long long coin = 0;
    if (valid && !__builtin_isfinite(acc)) {
        const DiagRow g = diag_row_general<float>(J, n, i, xi, yi);
        acc = g.s;
        coin = g.coincident;
    }
    const double p = -G * acc;
    if (kPhi && valid) phi_all[base + i] = p;
    // the products of diag_moments, one row per lane
    wsum[0][tid] = mi;
    wsum[1][tid] = mi * vx;
    wsum[2][tid] = mi * vy;
    wsum[3][tid] = mi * xi;
    wsum[4][tid] = mi * yi;
    wsum[5][tid] = mi * (xi * vy - yi * vx);
    wsum[6][tid] = mi * (vx * vx + vy * vy);
    wsum[7][tid] = mi * p;
    wcoin[tid] = coin;
    __syncthreads();
    const int qty = tid & (kTile - 1);                           // nine lanes per row tile: one quantity each
    const int r0 = row0 + (tid & ~(kTile - 1));
    if (qty <= kDiagSums && r0 < n) {
        const int rn = n - r0 < kTile ? n - r0 : kTile;
        const int w0 = tid & ~(kTile - 1);
        DiagTile* const d = tiles_all + (size_t)sys * batch_diag_tiles(stride) + r0 / kTile;
        if (qty < kDiagSums) {
            double s = 0.0;
            for (int q = 0; q < rn; ++q) s = s + wsum[qty][w0 + q];     // rows ascending
            reinterpret_cast<double*>(d)[qty] = s;
        } else {
            long long c = 0;
            for (int q = 0; q < rn; ++q) c += wcoin[w0 + q];
            d->coincident = c;
        }
    }
}

// One lane per system: diag_add over the system's tiles ascending, then diag_finish.  B lanes per workgroup (a template
// so that it is emitted after the stepping kernels, whose code then stays byte for byte the same).
template <int B>
__global__ __launch_bounds__(B) void batch_diag_reduce(const DiagTile* __restrict__ tiles_all,
                                                       const Meta* __restrict__ meta_all, Counters* __restrict__ ctr_all,
                                                       int systems, int stride, DiagOut* __restrict__ out) {
    const int sys = blockIdx.x * B + threadIdx.x;
    if (sys >= systems) return;
    const Meta m = meta_all[sys];
    const int chk = batch_checked_count(m.n, stride);
    const int n = chk < 0 ? 0 : chk;
    if (chk < 0) atomicAdd(&ctr_all[sys].errors, kIndexError);
    const DiagTile* __restrict__ tiles = tiles_all + (size_t)sys * batch_diag_tiles(stride);
    const int nt = (n + kTile - 1) / kTile;
    DiagTile total{};
    for (int t = 0; t < nt; ++t) diag_add(total, tiles[t]);
    out[sys] = diag_finish(total, m.step, n);
}

}  // namespace nbk
