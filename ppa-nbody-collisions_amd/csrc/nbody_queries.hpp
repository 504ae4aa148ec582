// csrc/nbody_queries.hpp -- every query header, and the state a context or a batch keeps for the queries.  Both translation
// units include this file where they used to list the headers, in that order: the order decides where each kernel lands in
// the code object, so a new header goes at the end.
//
// What a new query adds to the handles: its header here, one member of QueryStates, one line of queries_free, and its two
// entry points (nbody_get_* in nbody_ctx.hip, nbody_batch_get_* in nbody_batch.hip).  Nothing is allocated before a query's
// first call (tracers: the first set); each state grows to the largest request seen and is released by queries_free.
// A query that is another walk over what the states already hold adds no member: the groups on the cell list
// (nbody_groups_grid.hpp) use `cel` and `grp`, the pair counts and binaries on it (nbody_pairs_grid.hpp) `cel`, `prs` and `bin`,
// the encounters on it (nbody_encounters_grid.hpp) `cel` and `enc`.
// IdsState and TrackState are not queries - they are set up at create and by a reservation - and stay members of the
// handles, with ids_free and track_free next to them.
#pragma once
#include "nbody_rows.hpp"
#include "nbody_field.hpp"
#include "nbody_tracers.hpp"
#include "nbody_ids.hpp"
#include "nbody_tracks.hpp"
#include "nbody_neighbors.hpp"
#include "nbody_groups.hpp"
#include "nbody_group_energy.hpp"
#include "nbody_pairs.hpp"
#include "nbody_knn.hpp"
#include "nbody_shells.hpp"
#include "nbody_shell_moments.hpp"
#include "nbody_cells.hpp"
#include "nbody_within.hpp"
#include "nbody_encounters.hpp"
#include "nbody_binaries.hpp"
#include "nbody_tides.hpp"
#include "nbody_groups_grid.hpp"
#include "nbody_knn_grid.hpp"
#include "nbody_pairs_grid.hpp"
#include "nbody_encounters_grid.hpp"

namespace nbk {

struct QueryStates {
    FieldState fld;             // field evaluation (nbody_field.hpp)
    NeighborState nbr;          // neighbour queries (nbody_neighbors.hpp)
    GroupsState grp;            // group finding (nbody_groups.hpp)
    GroupEnergyState gen;       // group energies (nbody_group_energy.hpp): the labels of `grp` and these
    PairsState prs;             // pair-separation counts (nbody_pairs.hpp)
    KnnState knn;               // k nearest neighbours (nbody_knn.hpp)
    ShellState shl;             // shell sums (nbody_shells.hpp)
    ShellMomentState shm;       // shell moments (nbody_shell_moments.hpp)
    CellState cel;              // cell sums (nbody_cells.hpp): the cell list and its sorted records, for every query on the grid
    WithinState wth;            // radius queries (nbody_within.hpp): the cell list of `cel` and these
    EncState enc;               // encounter queries (nbody_encounters.hpp)
    BinState bin;               // bound-pair queries (nbody_binaries.hpp)
    TidesState tid;             // tidal tensor and jerk (nbody_tides.hpp)
    TracerState trc;            // tracer particles (nbody_tracers.hpp)
    KnnGridState kng;           // the k nearest on the cell list (nbody_knn_grid.hpp): the cell list of `cel` and these
};

// After the handle has synchronised its stream.
inline void queries_free(QueryStates& q) {
    rows_free(q.fld);
    rows_free(q.nbr);
    groups_free(q.grp);
    rows_free(q.gen);
    pairs_free(q.prs);
    rows_free(q.knn);
    rows_free(q.shl);
    shell_moments_free(q.shm);
    cells_free(q.cel);
    within_free(q.wth);
    pair_log_free(q.enc);
    pair_log_free(q.bin);
    tides_free(q.tid);
    tracers_free(q.trc);
    knn_grid_free(q.kng);
}

}  // namespace nbk
