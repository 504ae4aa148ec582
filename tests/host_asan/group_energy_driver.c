/* tests/host_asan/group_energy_driver.c -- nbody_group_catalog (csrc/nbody_group_energy.c) under AddressSanitizer + UBSan:
 * every array of exactly n entries and `cap` records on the heap, so a read or write past either end is caught, for every n
 * from 0 to 300 with cap 0, cap 1 and a full cap; the records are checked against sums made here.  Host code only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nbody.h"

static unsigned long long lcg(unsigned long long* s) { return *s = *s * 6364136223846793005ull + 1442695040888963407ull; }
static double unit(unsigned long long* s) { return (double)(lcg(s) >> 11) / 9007199254740992.0; }

static double* reals(int n) { return (double*)malloc((size_t)(n ? n : 1) * sizeof(double)); }

static int run(int n, unsigned long long seed) {
    double *x = reals(n), *y = reals(n), *vx = reals(n), *vy = reals(n), *m = reals(n), *phi = reals(n);
    int32_t* label = (int32_t*)malloc((size_t)(n ? n : 1) * sizeof(int32_t));
    if (!x || !y || !vx || !vy || !m || !phi || !label) return 2;
    int32_t groups = 0;
    for (int i = 0; i < n; ++i) {
        /* a new group, or the group of an earlier body: label[label[i]] == label[i] <= i by construction */
        label[i] = (i == 0 || lcg(&seed) % 3u == 0) ? i : label[(int)(lcg(&seed) % (unsigned)i)];
        groups += label[i] == i;
        x[i] = 100.0 * unit(&seed); y[i] = 100.0 * unit(&seed);
        vx[i] = 2.0 * unit(&seed) - 1.0; vy[i] = 2.0 * unit(&seed) - 1.0;
        m[i] = i % 17 == 0 ? 0.0 : 1.0 + unit(&seed);
        phi[i] = i % 13 == 0 ? NAN : -unit(&seed);
    }
    const int caps[3] = {0, 1, groups};
    for (int c = 0; c < 3; ++c) {
        const int cap = caps[c];
        nbody_group_record* out = cap ? (nbody_group_record*)malloc((size_t)cap * sizeof(*out)) : NULL;
        if (cap && !out) return 2;
        int32_t count = -1;
        const int rc = nbody_group_catalog(n, n ? x : NULL, n ? y : NULL, n ? vx : NULL, n ? vy : NULL, n ? m : NULL, n ? label : NULL,
                                           n ? phi : NULL, out, cap, &count);
        if (rc != NBODY_OK || count != groups) { printf("n %d cap %d: rc %d, %d groups, %d expected\n", n, cap, rc, (int)count, (int)groups); return 1; }
        const int stored = cap < groups ? cap : groups;
        long members = 0;
        for (int k = 0; k < stored; ++k) {
            const nbody_group_record* g = out + k;
            double mass = 0.0;
            int32_t cnt = 0;
            if (g->label < 0 || g->label >= n || label[g->label] != g->label || (k && out[k - 1].label >= g->label)) { printf("n %d record %d: label\n", n, k); return 1; }
            for (int i = 0; i < n; ++i)
                if (label[i] == g->label) { mass = mass + m[i]; ++cnt; }
            if (g->count != cnt || g->mass != mass || g->bound_members < 0 || g->bound_members > cnt || (g->flags & ~1)) { printf("n %d record %d: sums\n", n, k); return 1; }
            if (((g->flags & 1) != 0) != (g->energy < 0.0)) { printf("n %d record %d: flag\n", n, k); return 1; }
            members += cnt;
        }
        if (cap == groups && members != n) { printf("n %d: %ld members\n", n, members); return 1; }
        free(out);
    }
    free(x); free(y); free(vx); free(vy); free(m); free(phi); free(label);
    return 0;
}

int main(void) {
    for (int n = 0; n <= 300; ++n)
        if (run(n, 31u + 7u * (unsigned)n)) return 1;
    /* refused before anything is read */
    int32_t count = -1;
    const int32_t up[2] = {1, 1}, out_of_range[2] = {0, 2};
    const double v[2] = {1.0, 2.0};
    nbody_group_record rec[2];
    if (nbody_group_catalog(2, v, v, v, v, v, up, v, rec, 2, &count) != NBODY_ERR_INVALID) return 1;
    if (nbody_group_catalog(2, v, v, v, v, v, out_of_range, v, rec, 2, &count) != NBODY_ERR_INVALID) return 1;
    if (nbody_group_catalog(-1, v, v, v, v, v, up, v, rec, 2, &count) != NBODY_ERR_INVALID) return 1;
    if (nbody_group_catalog(2, v, v, v, v, v, up, v, NULL, 2, &count) != NBODY_ERR_INVALID) return 1;
    if (nbody_group_catalog(2, v, v, v, v, v, up, v, rec, 2, NULL) != NBODY_ERR_INVALID || count != -1) return 1;
    printf("group energy ok\n");
    return 0;
}
