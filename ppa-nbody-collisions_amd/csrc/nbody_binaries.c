/* csrc/nbody_binaries.c -- the host half of the bound-pair query (nbody_binary_finish, include/nbody.h):
 * the two-body orbit from the raw record of a bound pair, and the order of the list.  Plain C, no device: the divisions and
 * the square roots of the contract are the C library's, which are correctly rounded, not the device's expansions
 * (nbody_kernels.hpp, ieee_rcp: one known significand where a refined reciprocal is one ulp low).
 *     r = sqrt(d2);  gm = 0.5*mu;  eps = (0.5*v2) - (gm/r)
 *     a      = eps < 0 ? gm / (-(eps+eps)) : +inf
 *     e2     = 1.0 + (((eps+eps) * (hz*hz)) / (gm*gm));   ecc = e2 > 0 ? sqrt(e2) : +0.0
 *     period = a < +inf ? 6.283185307179586 * sqrt(((a*a)*a) / gm) : +inf
 *     sep    = r
 * The device's predicate is the squared one, (v2*v2)*d2 < mu*mu; within a few ulps of a parabolic or a circular orbit the
 * rounded eps and e2 may fall on the other side, which the two guards turn into a defined outcome instead of a NaN.
 * Every operation is rounded on its own (-ffp-contract=off). */
#include <math.h>
#include <stdlib.h>

#include "nbody.h"
#include "nbody_error.h"

static void binary_orbit(const nbody_binary_raw* q, nbody_binary* o) {
    const double r = sqrt(q->d2);
    const double gm = 0.5 * q->mu;
    const double eps = (0.5 * q->v2) - (gm / r);
    const double a = eps < 0.0 ? gm / (-(eps + eps)) : INFINITY;
    const double e2 = 1.0 + (((eps + eps) * (q->hz * q->hz)) / (gm * gm));
    o->a = a;
    o->ecc = e2 > 0.0 ? sqrt(e2) : 0.0;
    o->period = a < INFINITY ? 6.283185307179586 * sqrt(((a * a) * a) / gm) : INFINITY;
    o->sep = r;
}

/* (i, j) ascending: exact and total whatever the values are. */
static int binary_order(const void* pa, const void* pb) {
    const nbody_binary* a = (const nbody_binary*)pa;
    const nbody_binary* b = (const nbody_binary*)pb;
    if (a->i != b->i) return a->i < b->i ? -1 : 1;
    if (a->j != b->j) return a->j < b->j ? -1 : 1;
    return 0;
}

int nbody_binary_finish(const nbody_binary_raw* raw, int count, nbody_binary* out) {
    if (count < 0) return nbody_fail(NBODY_ERR_INVALID, "nbody_binary_finish: count = %d", count);
    if (count > 0 && (!raw || !out)) return nbody_fail(NBODY_ERR_INVALID, "nbody_binary_finish: NULL argument");
    for (int k = 0; k < count; ++k) {
        const nbody_binary_raw* q = raw + k;
        nbody_binary o;
        binary_orbit(q, &o);
        o.i = q->i < q->j ? q->i : q->j;
        o.j = q->i < q->j ? q->j : q->i;
        o.flags = q->flags & (NBODY_BINARY_OVERLAP | NBODY_BINARY_APPROACHING);
        o.reserved = 0;
        out[k] = o;
    }
    if (count > 1) qsort(out, (size_t)count, sizeof(nbody_binary), binary_order);
    return NBODY_OK;
}
