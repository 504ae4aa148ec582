/* tests/host_asan/encounters_driver.c -- nbody_encounter_finish (csrc/nbody_encounters.c) under AddressSanitizer + UBSan:
 * buffers of exactly `count` records on the heap, so a read or write past either end is caught; the order and the values
 * are checked too.  Host code only. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nbody.h"

static unsigned long long lcg(unsigned long long* s) { return *s = *s * 6364136223846793005ull + 1442695040888963407ull; }
static double unit(unsigned long long* s) { return (double)(lcg(s) >> 11) / 9007199254740992.0; }

static int run(int count, double h, unsigned long long seed) {
    nbody_encounter_raw* raw = (nbody_encounter_raw*)malloc((size_t)(count ? count : 1) * sizeof(*raw));
    nbody_encounter* out = (nbody_encounter*)malloc((size_t)(count ? count : 1) * sizeof(*out));
    if (!raw || !out) return 2;
    for (int k = 0; k < count; ++k) {
        raw[k].i = (int32_t)(lcg(&seed) % 1000u);
        raw[k].j = raw[k].i + 1 + (int32_t)(lcg(&seed) % 1000u);
        if (lcg(&seed) & 1) { int32_t t = raw[k].i; raw[k].i = raw[k].j; raw[k].j = t; }
        raw[k].flags = (uint32_t)(lcg(&seed) % 4u) | 0x100u;
        raw[k].reserved = 0;
        raw[k].c = 100.0 * unit(&seed);
        raw[k].b = 20.0 * unit(&seed) - 15.0;
        raw[k].disc = k % 7 == 0 ? NAN : 50.0 * unit(&seed) - 5.0;
    }
    int rc = nbody_encounter_finish(count ? raw : NULL, count, h, count ? out : NULL);
    if (rc != NBODY_OK) { printf("finish rc=%d\n", rc); return 1; }
    for (int k = 0; k < count; ++k) {
        const nbody_encounter* e = out + k;
        if (!(e->i < e->j) || e->reserved != 0 || (e->flags & ~3u) || !(e->t >= 0.0) || !(e->t <= h)) { printf("record %d\n", k); return 1; }
        if ((e->flags & NBODY_ENCOUNTER_NOW) && e->t != 0.0) { printf("now %d\n", k); return 1; }
        if (k && (out[k - 1].t > e->t || (out[k - 1].t == e->t && (out[k - 1].i > e->i || (out[k - 1].i == e->i && out[k - 1].j > e->j))))) {
            printf("order %d\n", k);
            return 1;
        }
    }
    free(raw);
    free(out);
    return 0;
}

int main(void) {
    const int counts[] = {0, 1, 2, 3, 64, 1000, 4097};
    const double hs[] = {0.0, 0.5, 20.0, INFINITY};
    for (size_t a = 0; a < sizeof(counts) / sizeof(counts[0]); ++a)
        for (size_t b = 0; b < sizeof(hs) / sizeof(hs[0]); ++b)
            if (run(counts[a], hs[b], 17u + a * 31u + b)) return 1;
    if (nbody_encounter_finish(NULL, 3, 1.0, NULL) != NBODY_ERR_INVALID || nbody_encounter_finish(NULL, -1, 1.0, NULL) != NBODY_ERR_INVALID ||
        nbody_encounter_finish(NULL, 0, -1.0, NULL) != NBODY_ERR_INVALID || nbody_encounter_finish(NULL, 0, NAN, NULL) != NBODY_ERR_INVALID)
        return 1;
    printf("encounters ok\n");
    return 0;
}
