/* csrc/nbody_encounters.c -- the host half of the encounter query (nbody_encounter_finish, include/nbody.h; DESIGN.md
 * 4.14): the time of contact from the raw record of a swept pair, and the order of the list.  Plain C, no device: the
 * division and the square root of the contract are the C library's, which are correctly rounded, not the device's
 * expansions (nbody_kernels.hpp, ieee_rcp: one known significand where a refined reciprocal is one ulp low).
 *     t = now ? +0 : (b < 0 && disc >= 0) ? min(c / (sqrt(disc) - b), h) : h          min(x, h) = x < h ? x : h
 * Every operation is rounded on its own (-ffp-contract=off; there is nothing to contract here anyway). */
#include <math.h>
#include <stdlib.h>

#include "nbody.h"
#include "nbody_error.h"

static double encounter_time(const nbody_encounter_raw* r, double h) {
    if (r->flags & NBODY_ENCOUNTER_NOW) return 0.0;
    if (r->b < 0.0 && r->disc >= 0.0) {
        const double x = r->c / (sqrt(r->disc) - r->b);
        return x < h ? x : h;
    }
    return h;
}

/* (t, i, j) ascending; t is never NaN (h is not, and a NaN quotient gives h). */
static int encounter_order(const void* pa, const void* pb) {
    const nbody_encounter* a = (const nbody_encounter*)pa;
    const nbody_encounter* b = (const nbody_encounter*)pb;
    if (a->t != b->t) return a->t < b->t ? -1 : 1;
    if (a->i != b->i) return a->i < b->i ? -1 : 1;
    if (a->j != b->j) return a->j < b->j ? -1 : 1;
    return 0;
}

int nbody_encounter_finish(const nbody_encounter_raw* raw, int count, double horizon, nbody_encounter* out) {
    if (count < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_encounter_finish: count = %d", count);
    if (count > 0 && (!raw || !out)) return nbody_fail(NBODY_ERR_INVALID, "nbody_encounter_finish: NULL argument");
    if (!(horizon >= 0.0)) return nbody_fail(NBODY_ERR_INVALID, "nbody_encounter_finish: horizon = %g", horizon);
    for (int k = 0; k < count; ++k) {
        const nbody_encounter_raw* r = raw + k;
        nbody_encounter e;
        e.t = encounter_time(r, horizon);
        e.i = r->i < r->j ? r->i : r->j;
        e.j = r->i < r->j ? r->j : r->i;
        e.flags = r->flags & (NBODY_ENCOUNTER_NOW | NBODY_ENCOUNTER_END);
        e.reserved = 0;
        out[k] = e;
    }
    if (count > 1) qsort(out, (size_t)count, sizeof(nbody_encounter), encounter_order);
    return NBODY_OK;
}
