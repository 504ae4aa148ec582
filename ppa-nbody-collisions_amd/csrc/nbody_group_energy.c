/* csrc/nbody_group_energy.c -- the host half of the group energies (nbody_group_catalog, include/nbody.h):
 * one record per friends-of-friends group from the bodies, the labels and the in-group potential phi_in that
 * nbody_get_group_potential returns.  Plain C, no device.  Every sum is s = s + term over the group's members in ascending
 * index, starting from +0, every operation rounded on its own (-ffp-contract=off), so a scalar loop in any language restates
 * it bit for bit:
 *     pass 1:  mass, sum m x, sum m y, sum m vx, sum m vy;  then each sum / mass (mass == 0: NaN, as diag_finish)
 *     pass 2:  dvx = vx_i - vx;  dvy = vy_i - vy;  w = (dvx*dvx) + (dvy*dvy);  K2 += m_i * w;  P += m_i * phi_in_i;
 *              a bound member: ((0.5*w) + phi_in_i) < 0
 *     kinetic = 0.5*K2;  potential = 0.5*P;  energy = kinetic + potential
 * O(n) in time and memory and no sort: label[i] == i marks a group's lowest member, so one ascending pass numbers the groups
 * in the order of their labels (slot[label] = record), and the two passes over the bodies, ascending, add each member into
 * its group's record - which is each group's members in ascending index.  The records themselves hold the running sums. */
#include <math.h>
#include <stdlib.h>

#include "nbody.h"
#include "nbody_error.h"

int nbody_group_catalog(int n, const double* x, const double* y, const double* vx, const double* vy, const double* m,
                        const int32_t* label, const double* phi_in, nbody_group_record* out, int cap, int32_t* n_groups) {
    const char* who = "nbody_group_catalog";
    if (n < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: n = %d", who, n);
    if (cap < 0) return nbody_fail(NBODY_ERR_INVALID, "%s: cap = %d", who, cap);
    if (!n_groups || (!out && cap > 0)) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    if (n > 0 && (!x || !y || !vx || !vy || !m || !label || !phi_in)) return nbody_fail(NBODY_ERR_INVALID, "%s: NULL argument", who);
    /* the labels, before anything is indexed by one */
    for (int i = 0; i < n; ++i) {
        const int32_t l = label[i];
        if (l < 0 || l >= n) return nbody_fail(NBODY_ERR_INVALID, "%s: label[%d] = %d outside [0, %d)", who, i, (int)l, n);
    }
    for (int i = 0; i < n; ++i) {
        const int32_t l = label[i];
        if (l > i || label[l] != l)
            return nbody_fail(NBODY_ERR_INVALID, "%s: label[%d] = %d is not the lowest index of its group", who, i, (int)l);
    }
    int32_t groups = 0;
    for (int i = 0; i < n; ++i) groups += label[i] == i;
    *n_groups = groups;
    const int stored = groups < cap ? groups : cap;
    if (stored == 0) return NBODY_OK;
    int32_t* slot = (int32_t*)malloc((size_t)n * sizeof(int32_t));   /* slot[label]: the group's record, by ascending label */
    if (!slot) return nbody_fail(NBODY_ERR_NOMEM, "%s: %d slots", who, n);
    int32_t k = 0;
    for (int i = 0; i < n; ++i) {
        if (label[i] != i) continue;
        slot[i] = k;
        if (k < stored) {
            nbody_group_record* g = out + k;
            g->mass = 0.0; g->cx = 0.0; g->cy = 0.0; g->vx = 0.0; g->vy = 0.0;
            g->kinetic = 0.0; g->potential = 0.0; g->energy = 0.0;
            g->label = i; g->count = 0; g->bound_members = 0; g->flags = 0;
        }
        ++k;
    }
    for (int i = 0; i < n; ++i) {                                     /* pass 1: the moments */
        const int32_t s = slot[label[i]];
        if (s >= stored) continue;
        nbody_group_record* g = out + s;
        g->mass = g->mass + m[i];
        g->cx = g->cx + (m[i] * x[i]);
        g->cy = g->cy + (m[i] * y[i]);
        g->vx = g->vx + (m[i] * vx[i]);
        g->vy = g->vy + (m[i] * vy[i]);
        g->count += 1;
    }
    for (int32_t s = 0; s < stored; ++s) {
        nbody_group_record* g = out + s;
        const int none = g->mass == 0.0;                              /* no centre, as diag_finish */
        g->cx = none ? NAN : g->cx / g->mass;
        g->cy = none ? NAN : g->cy / g->mass;
        g->vx = none ? NAN : g->vx / g->mass;
        g->vy = none ? NAN : g->vy / g->mass;
    }
    for (int i = 0; i < n; ++i) {                                     /* pass 2: in the centre-of-mass frame */
        const int32_t s = slot[label[i]];
        if (s >= stored) continue;
        nbody_group_record* g = out + s;
        const double dvx = vx[i] - g->vx, dvy = vy[i] - g->vy;
        const double w = (dvx * dvx) + (dvy * dvy);
        g->kinetic = g->kinetic + (m[i] * w);
        g->potential = g->potential + (m[i] * phi_in[i]);
        g->bound_members += ((0.5 * w) + phi_in[i]) < 0.0;
    }
    for (int32_t s = 0; s < stored; ++s) {
        nbody_group_record* g = out + s;
        g->kinetic = 0.5 * g->kinetic;
        g->potential = 0.5 * g->potential;
        g->energy = g->kinetic + g->potential;
        g->flags = g->energy < 0.0 ? (int32_t)NBODY_GROUP_BOUND : 0;
    }
    free(slot);
    return NBODY_OK;
}
