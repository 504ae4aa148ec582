/* csrc/nbody_screen.h -- the per-body rule behind Meta::summary and tile_rmax, shared by the C host code (the block
 * packing of csrc/nbody_bodies.c, which nbody_upload goes through) and the device code (unpack_slots rebuilds both every
 * step, ref_layout_pack_f32 for the reference-shaped launch; csrc/nbody_kernels.hpp).
 *
 * The fp32 ring kernel skips its per-pair screens on the strength of these bits: a wrong one is silent wrong physics.
 * What each bound buys is told where the kernels use it (nbody_kernels.hpp, "fast chain"); here is only the rule.
 *
 * Meta::summary, OR-ed over every body of the replica:
 *   bit 0  some coordinate is not below the coordinate bound in magnitude (NaN included)
 *   bit 1  some radius is not +0 (-0.0 is not +0)
 *   bit 2  fp32 contexts only: some coordinate is below the coordinate floor in magnitude (zero and NaN included)
 *   bit 3  fp32 contexts only: some mass is not below the mass bound in magnitude (NaN included)
 * tile_rmax[k]: the largest radius bits (below) of the aligned NBODY_BLOCK-body tile k. */
#ifndef NBODY_SCREEN_H
#define NBODY_SCREEN_H

#include <stdint.h>

#include "nbody_partition.h"   /* NBODY_HOST_DEVICE, NBODY_BLOCK */

enum { NBODY_SUMMARY_UNBOUNDED = 1, NBODY_SUMMARY_RADIUS = 2, NBODY_SUMMARY_SMALL = 4, NBODY_SUMMARY_MASS = 8 };

#define NBODY_COORD_BOUND_F32 0x1p38f    /* |x|,|y| < 2^38 for both bodies of a pair  =>  d2 <= 2^79 */
#define NBODY_COORD_FLOOR_F32 0x1p-16f   /* |x|,|y| >= 2^-16 for both  =>  d2 is exactly 0 or at least 2^-78 */
#define NBODY_MASS_BOUND_F32 0x1p90f     /* every |m| < 2^90: a term does not overflow at ordinary distances */
#define NBODY_COORD_BOUND_F64 0x1p249    /* the fp64 kernels' coordinate bound */

/* One body of an fp32 context: all four bits. */
NBODY_HOST_DEVICE static inline int nbody_screen_bits_f32(float x, float y, float m, float r) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    uint32_t rb;
    __builtin_memcpy(&rb, &r, 4);
    return ((ax < NBODY_COORD_BOUND_F32 && ay < NBODY_COORD_BOUND_F32) ? 0 : NBODY_SUMMARY_UNBOUNDED) |
           (rb != 0u ? NBODY_SUMMARY_RADIUS : 0) |
           ((ax >= NBODY_COORD_FLOOR_F32 && ay >= NBODY_COORD_FLOOR_F32) ? 0 : NBODY_SUMMARY_SMALL) |
           (__builtin_fabsf(m) < NBODY_MASS_BOUND_F32 ? 0 : NBODY_SUMMARY_MASS);
}

/* One body of an fp64 context: bits 0 and 1 only (no kernel of those contexts looks at the others). */
NBODY_HOST_DEVICE static inline int nbody_screen_bits_f64(double x, double y, double r) {
    uint64_t rb;
    __builtin_memcpy(&rb, &r, 8);
    return ((__builtin_fabs(x) < NBODY_COORD_BOUND_F64 && __builtin_fabs(y) < NBODY_COORD_BOUND_F64) ? 0 : NBODY_SUMMARY_UNBOUNDED) |
           (rb != 0u ? NBODY_SUMMARY_RADIUS : 0);
}

/* The radius bits: |r| rounded to float, as unsigned bits - non-negative floats order like unsigned integers, inf on
 * top -, 0 for a NaN: a NaN radius never collides (the predicate is false), so it bounds nothing. */
NBODY_HOST_DEVICE static inline uint32_t nbody_radius_bits_f32(float r) {
    const float ar = __builtin_fabsf(r);
    uint32_t b;
    __builtin_memcpy(&b, &ar, 4);
    return ar == ar ? b : 0u;
}
NBODY_HOST_DEVICE static inline uint32_t nbody_radius_bits_f64(double r) { return nbody_radius_bits_f32((float)__builtin_fabs(r)); }

/* A block [P|V|M|R] (src/nbody.cu:66-77) of n bodies to and from what the contexts keep: n records {x,y,m,r} and n
 * velocities, all of the block's precision (csrc/nbody_bodies.c; internal to the library, not exported).
 *   pack    returns the summary of the n bodies under the rule above.  tile_bits (or NULL): n_tiles entries, n_tiles >
 *           (n - 1) / NBODY_BLOCK, cleared and set to the tiles' radius bits in the same pass.  vel (or NULL: the caller
 *           copies a range straight out of the block, nbody_block_velocity) receives every velocity.
 *   unpack  the reverse; vel NULL leaves the block's velocities to the caller. */
#ifdef __cplusplus
extern "C" {
#endif
#define NBODY_INTERNAL __attribute__((visibility("hidden")))
NBODY_INTERNAL int nbody_block_pack(const void* block, int n, int precision, void* rec, void* vel, uint32_t* tile_bits,
                                    int n_tiles);
NBODY_INTERNAL void nbody_block_unpack(void* block, int n, int precision, const void* rec, const void* vel);
NBODY_INTERNAL void* nbody_block_velocity(const void* block, int n, int precision, int i);   /* where body i's lies */
#ifdef __cplusplus
}
#endif

#endif /* NBODY_SCREEN_H */
