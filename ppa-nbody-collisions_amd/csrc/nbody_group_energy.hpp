// csrc/nbody_group_energy.hpp -- group energies on the resident state (nbody_get_group_potential,
// nbody_batch_get_group_potential, include/nbody.h): the potential of every current body due to the other
// members of its own friends-of-friends group,
//     phi_in[i] = -G sum_{ j != i, label[j] == label[i], r_ij > 0 } m_j / r_ij,
// label[] being the labels of nbody_get_groups for the same (link, radius_scale).  Included after nbody_groups.hpp by both
// translation units.  The launch geometry, the count, the early exits and the tile loop (rows_walk, full shape) are those of
// every row query (nbody_rows.hpp); this file has the masked pair, the stage of its {x, y, m} and label
// planes, the general row and the host driver.  The O(N) catalogue is plain C on the host
// (nbody_group_energy.c).
//
// The sub-state rule, which is the contract in bits.  Let a group's members be i_0 < i_1 < ... < i_k.  phi_in[i_a] has the
// bits nbody_get_diagnostics puts in phi[a] for a context that holds exactly those k + 1 bodies in that order: ONE running
// sum over j = 0 .. n-1 ascending, in fp64 on exactly widened records, a term being diag_pair's own (called, not restated),
// and a non-member LEFT OUT - its pair never reaches the accumulator, not even as a NaN.
//   * A member pair: t = a; diag_pair(t, ...); a.s = t.s - the fast chain's fma into the running sum.
//   * A pair that is no member: a.s stays what it was.  The pair may have been evaluated (the lanes of a wave that have a
//     member among the same four sources run the chain together); its value, NaN included, is dropped by the select.
//   * The self term, which only the checked tile can hold: a.s + 0.0, the bits of the diagnostics' fma(+0, diag_rinv(1), s).
// Because leaving a pair out is exact, a wave may skip four sources none of its rows has a member among: per four sources
// the row's label is compared with the four staged labels, and one branch, which the whole wave takes or not (shaped like
// GroupsFour's rare path, nbody_groups.hpp), goes around the fp64 chain.  Where most groups are small the hot loop is four
// integer compares per four pairs; where one group holds everything it is the potential walk plus the compares.
// The padding of a ragged tile carries label -1 (x = y = m = +0), a lane without a row label -2 and x = y = 0: real labels lie
// in [0, n), so neither ever matches and the loop runs in fours without a bound test.  Labels are only compared, never used
// as an index.
// A row whose accumulator is not finite after the walk (a member at distance 0, a member's d2 outside the chain's range,
// non-finite input) is redone by group_row_general: diag_row_general itself (nbody_diag.hpp), handed the label test as the
// exact walk's membership test - members at distance exactly 0 left out and counted.  The walk is full, not triangular: a row needs its members on both sides in order, and there are no float
// atomics.  Every row writes its own record: plain loads and stores only.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "nbody.h"
#include "nbody_error.h"
#include "nbody_rows.hpp"
#include "nbody_groups.hpp"

#pragma clang fp contract(off)

namespace nbk {

static_assert(sizeof(nbody_group_energy_info) == 24 && offsetof(nbody_group_energy_info, n_bodies) == 0 &&
              offsetof(nbody_group_energy_info, n_groups) == 4 && offsetof(nbody_group_energy_info, largest) == 8 &&
              offsetof(nbody_group_energy_info, sweeps) == 12 && offsetof(nbody_group_energy_info, coincident) == 16,
              "nbody_group_energy_info layout");

struct GroupPhiOut { double phi; long long coincident; };   // device result of one row
static_assert(sizeof(GroupPhiOut) == 16, "GroupPhiOut layout");

typedef int32_t GroupLabels[2][kTile];        // the labels of the double-buffered j tile, in LDS

// The general code of a flagged row: diag_row_general (nbody_diag.hpp) keeping the members of the row's group only.
template <typename T>
__device__ __forceinline__ DiagRow group_row_general(const Rec<T>* __restrict__ J, const int32_t* __restrict__ label, int n, int i,
                                                     int32_t li, double xi, double yi) {
    return diag_row_general<T>(J, n, i, xi, yi, [label, li](int j) { return label[j] == li; });
}

// The four pairs of one trip of rows_walk: four integer compares, and the fp64 chain behind one branch.
struct GroupFour {
    const DiagPlanes *sx, *sy, *sm;
    const GroupLabels* sl;
    int i; int32_t li;              // the row and its label
    double xi, yi;
    DiagPhiSum a;
    template <bool kChecked>
    __device__ __forceinline__ void four(int b, int q, int j) {
        bool hit[4];
        int any = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hit[u] = (*sl)[b][q + u] == li;
            any += hit[u] ? 1 : 0;
            asm("" : "+v"(any));                                 // as GroupsFour: one add-with-carry per compare mask
        }
        if (any) {                                               // no lane of the wave has a member here: the wave skips
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                DiagPhiSum t = a;
                diag_pair(t, (*sx)[b][q + u], (*sy)[b][q + u], (*sm)[b][q + u], xi, yi);
                const double with = hit[u] ? t.s : a.s;          // no member: left out, whatever t.s is
                a.s = kChecked && j + u == i ? a.s + 0.0 : with; // the self term: the diagnostics' exact +0
            }
        }
    }
};

// grid and early exits: rows_prologue; the full walk, j = 0 .. n-1 ascending along a lane: rows_walk (nbody_rows.hpp) over the
// {x, y, m} planes of diag_walk_sums and a label plane; the padding and the lanes without a row as the head of the file says.
// label_all: the labels groups_flatten left, `stride` apart per system.
template <typename T, typename Count>
__global__ __launch_bounds__(kDiagBlock) void group_potential(const Rec<T>* __restrict__ J_all, const Meta* __restrict__ meta_all,
                                                              Counters* __restrict__ ctr_all, int stride, int n_one,
                                                              const int32_t* __restrict__ label_all, double G,
                                                              GroupPhiOut* __restrict__ out_all) {
    RowsLane<T, GroupPhiOut> L;
    if (rows_prologue<T, true, Count>(L, J_all, meta_all, ctr_all, stride, n_one, 0, out_all, GroupPhiOut{0.0, 0})) return;
    const int sys = Count::kBatch ? (int)blockIdx.y : 0;
    const int32_t* __restrict__ label = label_all + (size_t)sys * (size_t)stride;
    double xi = 0.0, yi = 0.0;
    int32_t li = -2;                                             // a lane without a row: no source's label
    if (L.valid) {
        const Rec<T> r = L.J[L.p];
        xi = (double)r.x; yi = (double)r.y;
        li = label[L.p];
    }
    __shared__ double sx[2][kTile], sy[2][kTile], sm[2][kTile];
    __shared__ int32_t sl[2][kTile];
    GroupFour f{&sx, &sy, &sm, &sl, L.p, li, xi, yi, DiagPhiSum{}};
    const Rec<T>* __restrict__ J = L.J;
    rows_walk<true, false>(L, [J, label](int b, int e, bool live, int j) {
        double x = 0.0, y = 0.0, m = 0.0;
        int32_t l = -1;                                          // padding: no row's label
        if (live) {
            const Rec<T> s = J[j];
            x = (double)s.x; y = (double)s.y; m = (double)s.m;
            l = label[j];
        }
        sx[b][e] = x; sy[b][e] = y; sm[b][e] = m; sl[b][e] = l;
    }, f);
    if (!L.valid) return;
    double acc = f.a.s;
    long long coin = 0;
    if (!__builtin_isfinite(acc)) {
        const DiagRow g = group_row_general<T>(L.J, label, L.n, L.p, li, xi, yi);
        acc = g.s;
        coin = g.coincident;
    }
    L.out[L.p] = GroupPhiOut{-G * acc, coin};
}

// ---------------------------------------------------------------------------------------------------------
// Host side.  The rows' records and their pinned staging, allocated on the first call and sized like groups_reserve's
// buffers: systems * stride.
// ---------------------------------------------------------------------------------------------------------
using GroupEnergyState = RowsArray<GroupPhiOut>;

// One call: the group finding exactly as nbody_get_groups makes it (groups_run: the caller's labels and the four counts; the
// labels stay resident in g.label), then one launch of group_potential over those labels on the same stream, whatever the
// number of systems is.  The site, Count and read_meta as for rows_run (nbody_rows.hpp).
template <typename T, typename Count, typename ReadMeta>
int group_energy_run(const char* who, const RowsSite& s, GroupsState& g, GroupEnergyState& buf, double G, double link,
                     double radius_scale, int32_t* label, double* phi_in, nbody_group_energy_info* info, ReadMeta read_meta) {
    std::vector<nbody_groups_info> gi((size_t)s.systems);
    int rc = groups_run<T, Count>(who, s, g, link, radius_scale, label, gi.data(), read_meta);
    if (rc != NBODY_OK) return rc;
    if (s.n_bound > 0) {
        const size_t total = (size_t)s.systems * (size_t)s.stride;
        const hipError_t e = rows_reserve(buf, total);
        if (e != hipSuccess) return rows_alloc_failed(e, who, "result buffers");
        hipLaunchKernelGGL((group_potential<T, Count>), s.grid(s.n_bound), dim3(kDiagBlock), 0, s.stream, (const Rec<T>*)s.J, s.meta,
                           s.counters, s.stride, s.n_one<Count>(), (const int32_t*)g.label, G, buf.d);
        NBK_ROWS_TRY(hipGetLastError());
        const size_t copied = Count::kBatch ? total : (size_t)s.n_bound;
        NBK_ROWS_TRY(hipMemcpyAsync(buf.h, buf.d, copied * sizeof(GroupPhiOut), hipMemcpyDeviceToHost, s.stream));
        if ((rc = s.sync<Count>(true, read_meta)) != NBODY_OK) return rc;
    }
    for (int sys = 0; sys < s.systems; ++sys) {
        const int n = gi[(size_t)sys].n_bodies;                  // what groups_run counted: nothing has run in between
        const GroupPhiOut* h = n ? reinterpret_cast<const GroupPhiOut*>(buf.h) + (size_t)sys * (size_t)s.stride : nullptr;
        double* out = phi_in + (size_t)sys * (size_t)s.stride;
        long long coin = 0;
        for (int p = 0; p < n; ++p) { out[p] = h[p].phi; coin += h[p].coincident; }
        info[sys] = nbody_group_energy_info{n, gi[(size_t)sys].n_groups, gi[(size_t)sys].largest, gi[(size_t)sys].sweeps, (int64_t)coin};
    }
    return NBODY_OK;
}

}  // namespace nbk
