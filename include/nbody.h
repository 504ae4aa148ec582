/* include/nbody.h -- C ABI of the MI355X-native direct N-body gravity + collision stepper.
 *
 * Drop-in boundary for the hot path of Aidan900/ppa-nbody-collisions.  The reference has no plugin / FFI
 * layer: main() (src/nbody.cu:373-551) calls its kernels directly.  Each entry point below names the
 * reference code it replaces (paths are relative to the reference tree).  Plain C types only; no
 * exceptions, no exit(): every function returns an nbody_status (0 = OK, negative = error) and
 * nbody_last_error_string() describes the last failure on the calling thread.
 *
 * Library: ppa-nbody-collisions_amd/libnbody_mi355x.so (built by __graft_entry__.build() / csrc/Makefile).
 * All compute entry points need a gfx950 device and FAIL (NBODY_ERR_NO_DEVICE / NBODY_ERR_HIP) without one:
 * there is no CPU fallback anywhere in the library.
 */
#ifndef NBODY_MI355X_H
#define NBODY_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_ABI_VERSION 2

/* ---------------------------------------------------------------------------------------------------
 * Status codes
 * ------------------------------------------------------------------------------------------------- */
typedef enum nbody_status {
    NBODY_OK = 0,
    NBODY_ERR_INVALID = -1,      /* bad argument                                                       */
    NBODY_ERR_IO = -2,           /* config file cannot be opened  (include/nbodyConfig.h:25-28)        */
    NBODY_ERR_PARSE = -3,        /* "<key> invalid value"          (include/nbodyConfig.h:41-45 etc.)  */
    NBODY_ERR_NOMEM = -4,        /* host or device allocation failed (src/nbody.cu:68-72)              */
    NBODY_ERR_NO_DEVICE = -5,    /* no gfx950 device visible                                           */
    NBODY_ERR_HIP = -6,          /* a HIP runtime call failed (replaces CUDA_SYNC_CHECK, :20-33)       */
    NBODY_ERR_CAPACITY = -7,     /* more bodies / events than the context was created for             */
    NBODY_ERR_COMM = -8,         /* RCCL failure or collective library unavailable                     */
    NBODY_ERR_STATE = -9         /* call sequence error (e.g. step before upload)                      */
} nbody_status;

const char* nbody_last_error_string(void);
const char* nbody_status_string(int status);
int nbody_abi_version(void);

/* ---------------------------------------------------------------------------------------------------
 * Body layout -- include/vec2f.h:13-20 (Vec2f: 8 bytes, align 4) and include/vec2.h:6-17 (Vec2<double>).
 * A host "block" is ONE allocation [Positions vec2[N] | Velocities vec2[N] | Masses real[N] | Radii real[N]]
 * exactly as BodiesData::alloc carves it (src/nbody.cu:63-79): 24*N bytes (fp32) or 48*N bytes (fp64).
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_vec2f { float X, Y; } nbody_vec2f;
typedef struct nbody_vec2 { double X, Y; } nbody_vec2;

typedef enum nbody_precision { NBODY_F32 = 0, NBODY_F64 = 1 } nbody_precision;

size_t nbody_block_bytes(int n, int precision);
/* BodiesData::alloc (src/nbody.cu:63-79) / freeData (:81-86), host part. */
void* nbody_block_alloc(int n, int precision);
void nbody_block_free(void* block);
/* Pointer carving of src/nbody.cu:74-77 (and :147-150, :283-286). Any output pointer may be NULL. */
int nbody_block_carve_f32(void* block, int n, nbody_vec2f** P, nbody_vec2f** V, float** M, float** R);
int nbody_block_carve_f64(void* block, int n, nbody_vec2** P, nbody_vec2** V, double** M, double** R);
/* Stable compaction on `mass != 0` with re-carving for the new count (src/nbody.cu:488-510). Host side
 * utility for callers that step through the reference-shaped launches below. Returns the new count or <0. */
int nbody_block_compact(void* block, int n, int precision);

/* ---------------------------------------------------------------------------------------------------
 * nbodyConfig.txt -- include/nbodyConfig.h:4-19 (struct ConfigData) and :22-227 (parseConfigFile)
 * ------------------------------------------------------------------------------------------------- */
#define NBODY_IMAGE_PATH_MAX 1024

enum { /* bit k of nbody_config.present is set when key k was accepted */
    NBODY_KEY_particleCount = 0, NBODY_KEY_totalIterations, NBODY_KEY_save_Image_Every_Xth_Iteration,
    NBODY_KEY_timestep, NBODY_KEY_minRandBodyMass, NBODY_KEY_maxRandBodyMass, NBODY_KEY_minRadius,
    NBODY_KEY_maxRadius, NBODY_KEY_radiusGrowthRate, NBODY_KEY_imgWidth, NBODY_KEY_imgHeight,
    NBODY_KEY_fieldWidth, NBODY_KEY_fieldHeight, NBODY_KEY_imagePath, NBODY_KEY_COUNT
};

typedef struct nbody_config {
    int particleCount;
    int totalIterations;
    int save_Image_Every_Xth_Iteration;
    float timestep;
    float minRandBodyMass;
    float maxRandBodyMass;
    float minRadius;
    float maxRadius;
    float growthRate;               /* file key "radiusGrowthRate" (include/nbodyConfig.h:13,208-220) */
    int imgWidth;
    int imgHeight;
    int fieldWidth;
    int fieldHeight;
    char imagePath[NBODY_IMAGE_PATH_MAX];
    uint32_t present;               /* deviation: the reference leaves missing keys uninitialised;  */
                                    /* we zero them and record which keys were seen                 */
} nbody_config;

/* parseConfigFile (include/nbodyConfig.h:22-227): same grammar (`key=value` per line, std::stoi/std::stof
 * number syntax so `0.2f`, `1e4f`, `50.f` parse), same echo text on stdout including the reference's
 * `minRandBodymass=` / `growthRate=` spellings and `Invalid variable: <name>` for unknown lines.  Instead of
 * exit(1) it returns NBODY_ERR_IO / NBODY_ERR_PARSE after printing the reference's message. */
int nbody_config_parse(const char* path, nbody_config* out);
/* Same, echo written to file descriptor echo_fd (-1: no echo). */
int nbody_config_parse_fd(const char* path, nbody_config* out, int echo_fd);
/* The stock nbodyConfig.txt values (nbodyConfig.txt:1-14). */
void nbody_config_stock(nbody_config* out);

/* ---------------------------------------------------------------------------------------------------
 * Initial conditions -- src/nbody.cu:401-416 with jbutil::randgen (include/jbutil.h:514-562)
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_rng { uint64_t u, v, w; } nbody_rng;
void nbody_rng_seed(nbody_rng* g, uint64_t s);            /* randgen::seed   jbutil.h:525-534 */
uint64_t nbody_rng_ival64(nbody_rng* g);                  /* randgen::ival64 jbutil.h:545-552 */
double nbody_rng_fval(nbody_rng* g);                      /* randgen::fval() jbutil.h:553-556 */
double nbody_rng_fval_range(nbody_rng* g, double a, double b); /* fval(a,b)  jbutil.h:557-560 */

/* Fills a block of cfg->particleCount bodies: seed 1024, draws x,y,m,r per body in that order, v = 0.
 * fp32 rounds each draw to float exactly where the reference does; fp64 keeps the double draws. */
int nbody_init_bodies(const nbody_config* cfg, void* block, int precision);
/* nbody_init_bodies with the seed as an argument (the reference fixes 1024, src/nbody.cu:401-416): other realisations
 * of the same configuration, e.g. the members of an ensemble.  nbody_init_bodies is the seed-1024 call of it. */
int nbody_init_bodies_seeded(const nbody_config* cfg, void* block, int precision, uint64_t seed);

/* ---------------------------------------------------------------------------------------------------
 * Stepper context -- replaces the per-iteration host loop src/nbody.cu:460-545 (cudaMalloc scratch,
 * H2D, ComputeForces, MoveBodies, D2H, host compaction) with device-resident state.
 * ------------------------------------------------------------------------------------------------- */
typedef enum nbody_semantics {
    NBODY_LITERAL = 0,  /* exactly what src/nbody.cu computes, index quirks included */
    NBODY_CLEAN = 1     /* every body active, true all-pairs, j ascending                                */
} nbody_semantics;

enum { /* nbody_ctx_desc.flags */
    NBODY_FLAG_RECORD_EVENTS = 1u << 0,   /* keep the collision event log (E_t, D_t of SURVEY.md A.2)   */
    NBODY_FLAG_GROUP_EXCHANGE = 1u << 1,  /* world>1, every rank is a context of this process: the       */
                                          /* exchange is done by nbody_group_step with peer copies        */
    NBODY_FLAG_FORCE_COMM = 1u << 2,      /* create the RCCL communicator and run the slot all-gather    */
                                          /* even when world == 1 (exercises the multi-rank path on one  */
                                          /* GPU)                                                         */
    NBODY_FLAG_TRACK_IDS = 1u << 3        /* keep the index -> identity map on the device (nbody_get_ids, */
                                          /* nbody_get_lineage); world == 1 without an exchange flag only */
};

typedef struct nbody_ctx nbody_ctx;

typedef struct nbody_ctx_desc {
    int precision;          /* nbody_precision                                                          */
    int semantics;          /* nbody_semantics                                                          */
    int capacity;           /* max bodies (>= first upload's n)                                         */
    int device;             /* HIP device ordinal                                                       */
    int rank, world;        /* range partition of bodies over ranks; world = 1 for a single GPU         */
    uint32_t flags;
    int event_capacity;     /* max logged events (0: default)                                           */
    double timestep;        /* cfg.timestep  (kernel arg `timestep`,  src/nbody.cu:482)                 */
    double growthRate;      /* cfg.growthRate (kernel arg `growthRate`, :482)                           */
    int fieldWidth;         /* kernel args :482                                                         */
    int fieldHeight;
    const void* comm_id;    /* world>1 with RCCL: 128-byte id from nbody_comm_unique_id on rank 0       */
    int kernel_variant;     /* 0 = automatic (by own-range size); tuning / A-B testing only: 1 general kernel,  */
                            /* 11/12/14/18 one-lane..eight-lanes-per-body kernel, 31/32 its 256-thread form,    */
                            /* 50/52/54 ring-of-waves kernel with 2x8 / 4x4 / 1x8 (rings x waves) workgroups    */
                            /* (53, 55, 56, 58, 59: its tuning forms).  fp64: 1 selects the general kernel, anything   */
                            /* else the fp64 production kernel                                                  */
} nbody_ctx_desc;

void nbody_ctx_desc_from_config(nbody_ctx_desc* d, const nbody_config* cfg, int precision);

int nbody_ctx_create(nbody_ctx** out, const nbody_ctx_desc* desc);
int nbody_ctx_destroy(nbody_ctx* ctx);

/* BodiesData::uploadToDevice (src/nbody.cu:88-96): copies a host block of n bodies (the FULL set on every
 * rank) to the device; the context keeps it resident between steps. */
int nbody_upload(nbody_ctx* ctx, const void* block, int n);
/* nsteps iterations of the loop body src/nbody.cu:463-510 (forces+collisions, drift+commit, stable
 * compaction), asynchronous: returns after enqueueing. */
int nbody_step(nbody_ctx* ctx, int nsteps);
/* cudaMemcpyAsync D2H of the state (src/nbody.cu:486) + the survivors' re-carved block (:496-510):
 * writes 24*n (48*n) bytes laid out for the CURRENT count n and stores n. block must hold `capacity`.
 * On an RCCL context (world > 1) this is a COLLECTIVE: velocities live only on their owner, every rank must
 * call it (the same holds for nbody_state_save, which downloads). */
int nbody_download(nbody_ctx* ctx, void* block, int* n);
int nbody_body_count(nbody_ctx* ctx, int* n);   /* synchronises */
int nbody_sync(nbody_ctx* ctx);                 /* CUDA_SYNC_CHECK (src/nbody.cu:20-33,546)           */
/* Context introspection used by the state files. */
int nbody_ctx_info(nbody_ctx* ctx, nbody_ctx_desc* desc_out, int64_t* steps);
int nbody_ctx_set_steps(nbody_ctx* ctx, int64_t steps);

typedef struct nbody_event {  /* one collision event, in the index space of the step it happened in    */
    int32_t step;             /* step counter since upload (0-based)                                   */
    int32_t i;                /* the body whose thread saw the collision                               */
    int32_t j;                /* the other body; j < 0 is never produced                               */
    int32_t kind;             /* 0: i absorbs j (E_t)   1: i deleted because of j (D_t witness)        */
} nbody_event;
/* Copies up to cap logged events (unordered within a step) and the total number logged since the last
 * clear; total > cap means the caller's buffer was too small, total > event_capacity means the log
 * overflowed (extra events were counted, not stored).  nbody_upload (and so nbody_state_load) clears the log and
 * restarts the total: events carry step numbers of the current upload only. */
int nbody_get_events(nbody_ctx* ctx, nbody_event* out, int cap, int64_t* total);
int nbody_clear_events(nbody_ctx* ctx);

/* Body identities (NBODY_FLAG_TRACK_IDS).  Every step ends with a stable compaction on `mass != 0`, so index
 * i names a different body afterwards.  With the flag the context keeps, on the device, the identity of every current body:
 * its index in the last nbody_upload, 0 .. n-1 (nbody_state_load uploads, so it restarts identities).  The map follows the
 * compaction itself, not the log: a body uploaded with mass 0 disappears at the first step without any event, a NaN mass
 * stays.  The compaction is stable, so the identities of the survivors are strictly increasing in i.  Two more launches per
 * step (one without NBODY_FLAG_RECORD_EVENTS), no device-to-host copy, no host wait; a context without the flag allocates and
 * launches nothing.  The flag needs world == 1 and neither NBODY_FLAG_GROUP_EXCHANGE nor NBODY_FLAG_FORCE_COMM (the other
 * ranks' keep flags are not in the slot): anything else is NBODY_ERR_INVALID from nbody_ctx_create, found before any device
 * call.  Both calls below: NBODY_ERR_STATE without the flag or before an upload, NBODY_ERR_INVALID for a NULL pointer or
 * cap < 0; both synchronise.
 * nbody_get_ids: ids[i] = identity of current body i; *n = current count, min(cap, n) entries are written. */
int nbody_get_ids(nbody_ctx* ctx, int32_t* ids, int cap, int* n);
typedef struct nbody_lineage {  /* an nbody_event in identity space                                    */
    int32_t step;               /* as nbody_event                                                      */
    int32_t id_i;               /* identity of the body that had index i in that step                  */
    int32_t id_j;               /* identity of the body that had index j in that step                  */
    int32_t kind;               /* as nbody_event: 0 id_i absorbs id_j, 1 id_i deleted because of id_j */
} nbody_lineage;
/* The event log translated through the map of the step each event happened in (needs NBODY_FLAG_RECORD_EVENTS as well:
 * NBODY_ERR_STATE without).  Record k is event k of nbody_get_events: same position, same step and kind; total, cap and the
 * overflow rules are those of nbody_get_events, and nbody_clear_events / nbody_upload empty both.  Only events of committed
 * steps are covered: what nbody_debug_force_only logs after the last step reads -1 / -1, and the tuning records of
 * kernel_variant 58 / 59 are outside the contract.  An event index outside [0, n) of its step is never used as an address: the
 * record gets -1 and the context fails its next synchronising call like after any failed index check. */
int nbody_get_lineage(nbody_ctx* ctx, nbody_lineage* out, int cap, int64_t* total);

/* Track log (NBODY_FLAG_TRACK_IDS): where was body k at each sample, how heavy was it, when did it vanish.
 * A device-side table of `samples` rows x `columns` identities.  nbody_track_record enqueues one row - one launch, two with
 * NBODY_TRACK_PHI - with no device-to-host copy and no host wait; the table is read back once, instead of nbody_download +
 * nbody_get_ids (two synchronising calls and a copy of the whole state) after every sample.
 * Row contract.  Column c stands for identity sel[c].  If a current body i has that identity: index[c] = i, rec[c] =
 * {x, y, vx, vy, m, r} of body i in the context's precision - the bits nbody_download followed by nbody_get_ids would give at
 * that moment - and, with NBODY_TRACK_PHI, phi[c] = the bits nbody_get_diagnostics puts in phi[i] (the order contract above:
 * one running sum over j ascending).  Otherwise index[c] = -1, every byte of rec[c] is 0 and phi[c] = +0.  Presence is read
 * from index, never from a field: a NaN mass is a present body, and a body uploaded with mass 0 is present in a row recorded
 * before the first step.  step and n_bodies of the row header come from the device-side state, like the recorded
 * diagnostics' rows.  A count outside [0, capacity] never becomes an index: the row is all absent with n_bodies = 0 and the
 * context fails its next synchronising call, like after any failed index check.
 * nbody_track_reserve allocates (or re-allocates) the log and empties it; samples = 0 frees it; it may be called before the
 * first upload.  ids == NULL: columns = capacity and column c is identity c; otherwise k columns, ids strictly increasing
 * within [0, capacity) (an identity at or above the uploaded count is simply always absent).  NBODY_ERR_INVALID, found before
 * any device call: k <= 0 with ids, an unsorted, repeated or out-of-range id, samples < 0, unknown `fields` bits, a log above
 * 2^31 bytes in all.  NBODY_ERR_STATE: a context created without NBODY_FLAG_TRACK_IDS.
 * nbody_track_record is enqueue-only on the context's stream, like nbody_step.  A full log is NBODY_ERR_CAPACITY, found on the
 * host: nothing is enqueued and the earlier rows stay.  No reservation, or no upload yet: NBODY_ERR_STATE.  nbody_upload (and
 * so nbody_state_load) restarts the log at row 0 and keeps the reservation.
 * nbody_track_read synchronises, copies min(recorded, cap_samples) rows and stores the number recorded and the columns.  Any of
 * rows, rec, index, phi may be NULL; rows[s], and rec / index / phi [s * columns + c]; rec is nbody_track_f32 or
 * nbody_track_f64 by the context's precision.  A non-NULL phi on a log reserved without NBODY_TRACK_PHI: NBODY_ERR_STATE.
 * A context that never reserves allocates nothing and launches nothing more, and the kernels it runs keep their code.
 * Cost (one MI355X, fp32, stock radii, ms per sample over plain stepping, median of 3 rounds (spread), the one read at the end
 * included; profiles/track_probe.txt), against nbody_download + nbody_get_ids after every step: N = 262144 with 64 columns
 * 0.064 (0.089) against 0.974 (0.167); a batch of 256 x 1024 with all columns 2.32 (0.05) against 27.74 (0.15); N = 262144 with
 * all columns 2.18 (0.38) against 2.21 (0.51), and 2.29 against 1.90 in an earlier run - there the log moves capacity columns
 * per sample where a download moves the current count, and what it buys is a loop without host waits.  On the device a record
 * is one launch of 6 to 9 us.  A potential row is a serial chain over j by contract, so NBODY_TRACK_PHI on k columns costs about
 * one wave's walk over the n bodies, not k/n of nbody_get_diagnostics: 64 columns at n = 102089 4.11 ms (spread 0.05) against
 * 6.89 ms for the full call. */
enum { NBODY_TRACK_PHI = 1u << 0 };   /* nbody_track_reserve fields */
typedef struct nbody_track_f32 { float  x, y, vx, vy, m, r; } nbody_track_f32;   /* 24 bytes */
typedef struct nbody_track_f64 { double x, y, vx, vy, m, r; } nbody_track_f64;   /* 48 bytes */
typedef struct nbody_track_row { int64_t step, n_bodies; } nbody_track_row;
int nbody_track_reserve(nbody_ctx* ctx, int samples, const int32_t* ids, int k, uint32_t fields);
int nbody_track_record(nbody_ctx* ctx);
int nbody_track_read(nbody_ctx* ctx, nbody_track_row* rows, void* rec, int32_t* index, double* phi,
                     int cap_samples, int* n_samples, int* columns);

typedef struct nbody_stats {
    int64_t steps;            /* steps enqueued since upload                                           */
    int64_t pairs;            /* ordered (i,j) pairs evaluated by THIS rank since upload (device count) */
    double force_kernel_ms;   /* sum of force-kernel durations measured with HIP events (0 if off)      */
    int64_t force_kernel_launches;
    int n_bodies;             /* current global body count                                             */
    int n_own;                /* bodies owned by this rank                                             */
    double exchange_ms;       /* sum of the per-step slot all-gather durations, HIP events (0 if off or no exchange) */
    int64_t exchange_launches;
    int64_t exchange_bytes;   /* bytes this rank received through all-gathers since upload              */
    int64_t slot_bytes_now;   /* bytes ONE rank contributes to the next step's all-gather (0: no exchange): follows */
                              /* the live body count, not the capacity                                   */
} nbody_stats;
int nbody_get_stats(nbody_ctx* ctx, nbody_stats* out);  /* synchronises */
/* Bracket every force-kernel launch with HIP events on the context's stream (bench / profiling). */
int nbody_set_kernel_timing(nbody_ctx* ctx, int enable);
/* Which force kernel the next step of this context launches (static string; reporting only). */
const char* nbody_force_kernel_name(nbody_ctx* ctx);

/* Image output.  nbody_render_image = cudaMemsetAsync(254) + generateImage + D2H
 * (src/nbody.cu:531-537, kernel :294-348): bodies drawn as filled discs of value 0 into img[width*height]; the
 * kernel's missing `i < numBodies` guard is present.  On a multi-rank context every rank can render (the
 * replica holds all positions and radii).  nbody_write_pgm = saveImageToDisk (:350-371): prints
 * "Saving (WxH) to disk", writes "P5\nW H\n255\n" + bytes; where the reference prints its error and exit(1)s
 * it prints the same text to stderr and returns NBODY_ERR_IO. */
int nbody_render_image(nbody_ctx* ctx, unsigned char* img, int width, int height);
int nbody_write_pgm(const char* path, const unsigned char* img, int width, int height);

/* State dump / restore (the reference has none): a 64-byte header {magic "NBODYST1", precision,
 * body count, steps since upload, timestep, growthRate, field} followed by the [P|V|M|R] block of the current
 * survivors, i.e. exactly what nbody_download returns.  nbody_state_load uploads the block into ctx (which must
 * have the same precision and enough capacity) and restores the step counter; parameters in the file are
 * informational, the context keeps its own.  A rank of a NBODY_FLAG_GROUP_EXCHANGE group holds its own velocities only:
 * nbody_state_save on it is NBODY_ERR_STATE and no file is opened.  nbody_group_state_save writes the block of
 * nbody_group_download under the header of rank 0 (the same file a plain context in that state writes); every rank of a
 * group loads such a file with nbody_state_load. */
int nbody_state_save(nbody_ctx* ctx, const char* path);
int nbody_group_state_save(nbody_ctx** ctxs, int world, const char* path);
int nbody_state_load(nbody_ctx* ctx, const char* path);
/* Reads only the header of a state file. Any output pointer may be NULL. */
int nbody_state_peek(const char* path, int* precision, int* n, int64_t* steps);

/* Multi-rank plumbing (world > 1).  One process per GPU; the host language moves the 128-byte id. */
#define NBODY_COMM_ID_BYTES 128
int nbody_comm_unique_id(void* out128);   /* ncclGetUniqueId via dlopen("librccl.so.1") */

/* Single-process form of the same partition: ctxs[g] is rank g of `world`, all created in this process
 * with NBODY_FLAG_GROUP_EXCHANGE (one per device, or several on one device).  The per-step all-gather is
 * done with stream-ordered device-to-device copies; no RCCL, no host synchronisation inside the loop. */
int nbody_group_step(nbody_ctx** ctxs, int world, int nsteps);
int nbody_group_download(nbody_ctx** ctxs, int world, void* block, int* n);
/* Global index range [lo, lo+cnt) currently owned by this rank (synchronises). */
int nbody_own_range(nbody_ctx* ctx, int* lo, int* cnt);
/* The partition rule itself (pure host function, no device needed): whole reference blocks of 128 bodies
 * (THREADS_PER_BLOCK, src/nbody.cu:36), as evenly as the block count allows, in rank order.  nbody_upload draws it
 * for the uploaded count and the device re-draws it from the survivor count after every step, so ranks stay level
 * as bodies are deleted (the reference's compaction is global, src/nbody.cu:488-510). */
int nbody_partition(int n, int rank, int world, int* lo, int* cnt);
void* nbody_ctx_stream(nbody_ctx* ctx);   /* hipStream_t of the context */

/* ---------------------------------------------------------------------------------------------------
 * Physical diagnostics of the resident state (the reference has none).  Everything in IEEE fp64 (fp32 states are widened
 * exactly), over the n current bodies, independent of the semantics (a literal context's frozen tail counts like any
 * other body); G = (double)6.67408e-11f as in the force kernels.
 *     mass = sum m_i                       momentum = sum m_i v_i             center_of_mass = sum m_i x_i / mass
 *     angular_momentum = sum m_i (x_i v_iy - y_i v_ix), about the origin      kinetic = 1/2 sum m_i |v_i|^2
 *     phi_i = -G sum_{j != i, r_ij > 0} m_j / r_ij                            potential = 1/2 sum m_i phi_i
 * center_of_mass is NaN when mass == 0.  Ordered pairs i != j at distance exactly 0 are left out of phi and counted in
 * coincident_pairs.  Each term m_j / r_ij is within 4 ulps of its exact value; phi_i is one sum over j ascending, and the
 * totals are reduced per aligned 128-body tile and then over the tiles in ascending order: the result bits depend on the
 * state only, not on the rank, the world, the transport or the force kernel.  A call never changes what later steps
 * compute.  Non-finite inputs may give non-finite outputs.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_diag {
    int64_t step;              /* steps since upload                                                      */
    int64_t n_bodies;          /* current global body count                                               */
    int64_t coincident_pairs;  /* ordered pairs i != j at distance 0, left out of phi and potential       */
    double mass, momentum[2], center_of_mass[2], angular_momentum, kinetic, potential;
} nbody_diag;
/* Synchronises. phi: NULL, or room for `capacity` doubles; receives phi_i in global index order.
 * On an RCCL context (world > 1) this is a COLLECTIVE, like nbody_download: every rank calls it, every rank
 * gets the same bits.  A rank of a NBODY_FLAG_GROUP_EXCHANGE group on its own: NBODY_ERR_STATE (use the group form). */
int nbody_get_diagnostics(nbody_ctx* ctx, nbody_diag* out, double* phi);
/* The same for a single-process group (ctxs as in nbody_group_step); refuses ranks that were not uploaded and stepped
 * together. */
int nbody_group_diagnostics(nbody_ctx** ctxs, int world, nbody_diag* out, double* phi);

/* ---------------------------------------------------------------------------------------------------
 * Field evaluation (the reference has none): acceleration and potential at the bodies' own positions or at
 * arbitrary probe points.  Over the n current bodies, in IEEE fp64 (fp32 states are widened exactly), G = (double)6.67408e-11f,
 * independent of the semantics like the diagnostics (a literal context's frozen tail is a source like any other body).  With
 * x_j a source position, m_j its mass and r_j = |x - x_j|:
 *     phi(x) = -G sum_j m_j / r_j                    a(x) = -G sum_j m_j (x - x_j) / r_j^3
 * over the sources with r_j > 0; a source at distance exactly 0 is left out of all three sums and counted in *coincident.
 * Explicit points (points != NULL): m probe points, always nbody_vec2 (double) whatever the context's precision; out[p] is the
 * field at points[p]; *n_out = m; m == 0 is legal and launches nothing.
 * Own positions (points == NULL): the probe points are the current bodies' own positions, taken on the device with no
 * download; body i's self term is excluded by index and not counted, so *coincident equals nbody_diag.coincident_pairs; m is
 * the room in out, *n_out the current count n; m < n is NBODY_ERR_CAPACITY with nothing written.
 * Order contract (the one of the diagnostics).  ax, ay and phi of a point are each one running sum over j = 0 .. n-1 ascending:
 * the bits depend on the state and the point only, not on rank, world, transport, force kernel, m or the point's position in
 * points.  With points == NULL, out[i].phi has the bits nbody_get_diagnostics puts in phi[i], for every state.  A sum whose fast
 * chain is not finite is redone by general code (IEEE sqrt and divide, hypot outside the normal range, distance-0 sources
 * skipped and counted) in which a term overflows only where m_j / r_j^2 itself does; a finite sum is never replaced.  Each
 * term of a component is within 13 ulps of its exact value (m_j / r_j within 3): |error| <= (n + 14) 2^-53 sum_j |term|.
 * Non-finite inputs may give non-finite outputs.
 * nbody_get_field synchronises, reads the replica only and never changes what later steps compute.  It is NOT collective:
 * every rank's replica holds every position and mass (as nbody_render_image relies on), so any context may call it on its own
 * - world > 1, a rank of a NBODY_FLAG_GROUP_EXCHANGE group, a NBODY_FLAG_FORCE_COMM context - and each gives the same bits.
 * The device points, the device results and their pinned staging are allocated on the first call and grown to the largest m
 * seen; a context that never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: NULL ctx, out, n_out or coincident; m < 0; m x 24 bytes above 2^31.
 * NBODY_ERR_STATE: before an upload.  A device-side failure is reported as by every synchronising call.
 * Cost (one MI355X, fp32; profiles/field_probe.txt): a whole call at N = 262144 with points == NULL 42.5 ms (the kernel 40.8 ms:
 * 1.35 times the time per pair of the diagnostics' potential kernel, 1.38 expected from the 15 + 1 against 10 + 1 fp64
 * instructions per pair), against 29.4 ms for nbody_get_diagnostics with phi and 28.7 ms for a step; 65536 explicit points on
 * that state 13.9 ms (1.79 times: 256 workgroups are one wave per SIMD); a batch of 256 x 1024 with points == NULL 1.42 ms per
 * call, 0.18 ms of it the kernel.
 * nbody_batch_get_field: the same evaluation for every system of a batch in ONE launch, whatever S is, with the one set of
 * points for all of them.  Explicit points: system s's results at out[s * m + p] (systems x m x 24 bytes at most 2^31).
 * points == NULL: system s's results go to out + s * capacity, one entry per current body, the rest of the slice is left
 * unchanged (the layout of nbody_batch_diagnostics' phi).  coincident: one int64_t per system.  System s gives the bits an
 * nbody_ctx holding that system's state gives; an empty system gives +0 in every field of every point and 0 coincident.  A
 * count outside [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_diagnostics.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_field { double ax, ay, phi; } nbody_field;   /* 24 bytes */
int nbody_get_field(nbody_ctx* ctx, const nbody_vec2* points, int m, nbody_field* out, int* n_out, int64_t* coincident);
struct nbody_batch;   /* the batched stepper, below */
int nbody_batch_get_field(struct nbody_batch* b, const nbody_vec2* points, int m, nbody_field* out, int64_t* coincident);

/* ---------------------------------------------------------------------------------------------------
 * Tidal tensor and jerk (the reference has none): how the field of nbody_get_field changes in space and, along
 * the motion, in time.  The conventions are nbody_get_field's: over the n current bodies, IEEE fp64 (fp32 states widened
 * exactly), G = (double)6.67408e-11f, independent of the semantics.  With d = x_j - x, r = |d| > 0 and dv = v_j - v:
 *     T_ab(x)     = da_a/dx_b = G sum_j m_j (3 d_a d_b / r^5 - delta_ab / r^3)             -> tide[p].txx, txy, tyy
 *     adot_a(x,v) = da_a/dt   = G sum_j m_j (dv_a / r^3 - 3 (d . dv) d_a / r^5)            -> jerk[p].X, Y
 * (the tensor is the gradient of the Newtonian acceleration, the tidal approximation of e.g. Binney & Tremaine, Galactic
 * Dynamics, 2nd ed., ch. 8; the jerk is the Hermite scheme's, Makino & Aarseth 1992, PASJ 44, 141, eq. 2, and feeds the step
 * check eta sqrt(|a| / |adot|)).  A source at distance exactly 0 is left out of every sum and counted in *coincident.  The
 * force law is the 3-D one in a plane: txx + tyy = G sum_j m_j / r_j^3 > 0, the tensor is not traceless and the missing tzz is
 * the negative of that sum.  With every source at rest adot = T v.  A body's tidal (Hill) radius is (G m / lambda_max)^(1/3),
 * lambda_max the larger eigenvalue of T.
 * Rows.  points != NULL: m probe points, *n_out = m, m == 0 is legal and launches nothing; v is point_vel[p], or 0 with
 * point_vel == NULL (a point at rest).  points == NULL: the current bodies' own positions and velocities; body i's self term
 * is excluded by index and not counted, so *coincident equals nbody_get_field's; m is the room in tide (and jerk), *n_out the
 * current count n; m < n is NBODY_ERR_CAPACITY with nothing written.
 * jerk == NULL: the tensor alone, read from the replica only.  This form is NOT collective: any context may call it on its own -
 * world > 1, a rank of a NBODY_FLAG_GROUP_EXCHANGE group, a NBODY_FLAG_FORCE_COMM context - and gets the bits of a plain context.
 * jerk != NULL: the velocities are read, which a rank holds for its own range only: NBODY_ERR_STATE on a context with
 * world > 1, NBODY_FLAG_GROUP_EXCHANGE or NBODY_FLAG_FORCE_COMM (the rule of nbody_get_encounters and the tracers).
 * Order contract.  Every reported number is built from running sums over j = 0 .. n-1 ascending (sum m/r^3, the three sums
 * 3 m u_a u_b / r^3 with u = d / r, and the two jerk sums): the bits depend on the state, the point and its velocity only, not on
 * rank, world, transport, force kernel, m, the point's place in points, or whether the call also asks for the jerk - tide[] of a
 * call with jerk has the bits of a call without.  A sum whose fast chain is not finite is redone by general code (IEEE sqrt and
 * divide, hypot outside the normal range, distance-0 sources skipped and counted) in which a term overflows only where
 * m_j / r_j^3 itself does; a finite sum is never replaced.  Error bounds, u = 2^-53 (derived in DESIGN.md 4.17):
 *     |error of T_ab|  <= (n + 26) u G sum_j m_j (3 |d_a d_b| / r^2 + delta_ab) / r^3
 *     |error of adot_a| <= (2 n + 28) u G sum_j m_j (|dv_a| + 3 (|dx dvx| + |dy dvy|) |d_a| / r^2) / r^3
 * Non-finite inputs may give non-finite outputs.
 * Both calls synchronise and read only: stepping after any number of calls is bit-identical to stepping without them.  The
 * device points, point velocities, results and their pinned staging are allocated on the first call and grown to the largest m
 * seen; a context that never calls allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: a NULL handle, tide, n_out or coincident; m < 0; point_vel without points;
 * point_vel with jerk == NULL; m x 24 bytes (a batch: systems x m x 24) above 2^31.  NBODY_ERR_STATE: before an upload.  A
 * device-side failure is reported as by every synchronising call.
 * Cost (one MI355X, fp32; profiles/tides_probe.txt): a whole call at N = 262144 with points == NULL 53.7 ms for the tensor (the
 * kernel 51.4 ms: 1.28 times the time per pair of nbody_get_field's kernel, 1.34 expected from the 21 + 1 against 15 + 1 fp64
 * instructions per pair) and 74.0 ms with the jerk (the kernel 71.1 ms: 1.76 times, 1.83 expected from 30 + 1), against 41.9 ms
 * for nbody_get_field and 28.1 ms for a step; 65536 explicit points on that state 16.2 ms and, moving, with the jerk 21.1 ms
 * (1.25 and 1.62 times nbody_get_field's kernel at the same points); a batch of 256 x 1024 with points == NULL 1.82 and 2.34 ms
 * per call, 0.22 and 0.29 ms of it the kernel.
 * nbody_batch_get_tides: the same for every system of a batch in ONE launch, with the one set of points and point velocities
 * for all of them.  The layout of tide and jerk, the per-system coincident, the treatment of an empty system and of a count
 * outside [0, capacity] are nbody_batch_get_field's.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_tide { double txx, txy, tyy; } nbody_tide;   /* 24 bytes */
int nbody_get_tides(nbody_ctx* ctx, const nbody_vec2* points, const nbody_vec2* point_vel, int m, nbody_tide* tide,
                    nbody_vec2* jerk /* may be NULL */, int* n_out, int64_t* coincident);
int nbody_batch_get_tides(struct nbody_batch* b, const nbody_vec2* points, const nbody_vec2* point_vel, int m, nbody_tide* tide,
                          nbody_vec2* jerk /* may be NULL */, int64_t* coincident /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Neighbour queries (the reference has none): for every row - a current body, or an arbitrary probe point -
 * the nearest of the n current bodies, its squared distance, and how many of them satisfy the reference's collision
 * predicate d^2 <= (r_i + r_j)^2 (src/nbody.cu:126-134) with the row right now.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  A row has
 * a position (x, y) and a radius r: for an explicit point r = +0; for a body x, y and r are the body's record widened
 * exactly.  A source j has the record (X_j, Y_j, R_j), widened exactly from fp32 or taken as it is from fp64.  Then
 *     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy);              three roundings after the two subtractions
 *     nearest:  best = +inf, index = -1;  for j ascending:  if (d2_j < best) { best = d2_j; index = j; }
 *     overlaps: the number of j with  d2_j <= s*s,  s = r + R_j            the reference's predicate read in fp64
 * and out.d2 = best, out.index = index, out.overlaps = that number.  What follows from it:
 *   - ties go to the lowest j;
 *   - a source whose d2 is NaN or +inf is never the nearest; a source whose d2 is NaN is never an overlap (one whose d2 is
 *     +inf is an overlap exactly where s*s is +inf too);
 *   - a row with no eligible source gives {+inf, -1, 0};
 *   - the result is a function of the set of sources only, so an implementation may walk j in any order and with any number
 *     of lanes per row, as long as it returns exactly this;
 *   - it is independent of the semantics, like the diagnostics: a literal context's frozen tail is a source like any other
 *     body; the masses play no part;
 *   - with the bodies' own positions d2_ij and d2_ji have the same bits (dx only changes sign, s is the same sum), so
 *     overlaps are symmetric: j counts for i exactly where i counts for j;
 *   - accuracy: the inputs are exact, dx is within 1 u of the exact difference, its square within 3 u, the sum within 4 u
 *     (first order, u = 2^-53): d2 is within 4 u of the exact squared distance as long as no square underflows.
 * Explicit points (points != NULL): m probe points, always nbody_vec2 (double) whatever the context's precision; out[p]
 * belongs to points[p]; *n_out = m; m == 0 is legal and launches nothing.
 * Own positions (points == NULL): the rows are the current bodies, taken on the device with no download; body i's self term
 * is excluded by index (a second body at the same place is a source at d2 = +0); m is the room in out, *n_out the current
 * count n; m < n is NBODY_ERR_CAPACITY with nothing written.
 * nbody_get_neighbors synchronises, reads the replica only and never changes what later steps compute.  It is NOT
 * collective: every rank's replica holds every {x, y, m, r}, so any context may call it on its own - world > 1, a rank of a
 * NBODY_FLAG_GROUP_EXCHANGE group, a NBODY_FLAG_FORCE_COMM context - and each gives the same bits.  The device points, the
 * device results and their pinned staging are allocated on the first call and grown to the largest m seen; a context that
 * never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: NULL ctx, out or n_out; m < 0; m x 16 bytes above 2^31.
 * NBODY_ERR_STATE: before an upload.  A device-side failure is reported as by every synchronising call.
 * Cost (one MI355X, fp32, stock radii; profiles/neighbor_probe.txt): a whole call at N = 262144 with points == NULL 31.6 ms (the
 * kernel 29.5 ms: 2.33e12 ordered pairs per second, 0.95 times the time per pair of the diagnostics' potential kernel and 0.71
 * times field_at's, measured in the same run); 65536 explicit points on that state 13.0 ms (1.60 times the potential's time
 * per pair: 256 workgroups are one wave per SIMD); a batch of 256 x 1024 with points == NULL 0.13 ms of kernel, 1.9 ms for
 * StepperBatch.neighbors() with its 4 MiB of results.  The route without the call, nbody_download plus the numpy model on the
 * host, took 1.28 s at N = 16384 against 0.93 ms for the call.
 * nbody_batch_get_neighbors: the same query for every system of a batch in ONE launch, whatever S is, with the one set of
 * points for all of them.  Explicit points: system s's results at out[s * m + p] (systems x m x 16 bytes at most 2^31).
 * points == NULL: system s's results go to out + s * capacity, one entry per current body, the rest of the slice is left
 * unchanged (the layout of nbody_batch_get_field).  System s gives the bits an nbody_ctx holding that system's state gives;
 * an empty system gives {+inf, -1, 0} for every explicit point and writes nothing in the own form.  A count outside
 * [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_get_field.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_neighbor { double d2; int32_t index; int32_t overlaps; } nbody_neighbor;   /* 16 bytes */
int nbody_get_neighbors(nbody_ctx* ctx, const nbody_vec2* points, int m, nbody_neighbor* out, int* n_out);
int nbody_batch_get_neighbors(struct nbody_batch* b, const nbody_vec2* points, int m, nbody_neighbor* out);

/* ---------------------------------------------------------------------------------------------------
 * k nearest neighbours (the reference has none): for every row - a current body, or an arbitrary probe
 * point - the k nearest of the n current bodies and their squared distances, 1 <= k <= NBODY_KNN_MAX: what a local density
 * from the distance to the k-th neighbour, a kNN graph or an isolation measure is made of.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, on the
 * records of nbody_get_neighbors: (X_j, Y_j) of the n current bodies, widened exactly from fp32 or taken as they are from
 * fp64.  Radii and masses play no part.  For a row at (x, y) and a source j:
 *     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)               the d2 of nbody_get_neighbors, same bits
 *   - a source is eligible iff d2_j < +inf: a NaN or +inf d2 is never listed;
 *   - in the own form the self term is excluded by index: a second body at the same place is eligible at d2 = +0;
 *   - the row's result is the first k eligible sources under the total order (d2, j) ascending: ties in d2 go to the lower j;
 *   - entry c of the row is d2[row * k + c], index[row * k + c];
 *   - with fewer than k eligible sources the remaining entries are {+inf, -1}.
 * What follows from it:
 *   - for every k, entry 0 has the bits of nbody_get_neighbors' {d2, index} for that row;
 *   - the lists of k and k' < k agree on the first k' entries;
 *   - d2 is non-decreasing along a row; every index of a row is distinct and is not the row's own;
 *   - the result is a function of the set of sources only, so an implementation may walk j in any order, with any number of
 *     lanes per row, and keep the list anywhere, as long as it returns exactly this;
 *   - it is independent of the semantics: a literal context's frozen tail is a source like any other body;
 *   - a row with no eligible source, or an empty system, is all {+inf, -1}.
 * nbody_get_knn follows nbody_get_neighbors in every respect not named here.  Explicit points (points != NULL): m probe
 * points, always nbody_vec2; *n_out = m; m == 0 is legal and launches nothing.  Own positions (points == NULL): the rows are
 * the current bodies, taken on the device; m is the room in rows, *n_out the current count n; m < n is NBODY_ERR_CAPACITY
 * with nothing written.  It synchronises, reads the replica only and never changes what later steps compute.  It is NOT
 * collective: any rank of any world or transport gives the same bits.  The device points, the device entries (12 bytes each)
 * and their pinned staging are allocated on the first call and grown; a context that never calls it allocates nothing and
 * launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: NULL ctx, d2, index or n_out; k outside [1, NBODY_KNN_MAX]; m < 0;
 * m x k x 12 bytes above 2^31 (in the own form too, where m is the room).  NBODY_ERR_STATE: before an upload.
 * Cost (one MI355X, fp32, stock radii, the N = 262144 state after 3 steps, n = 130965, points == NULL; profiles/knn_probe.txt,
 * a kernel trace with nbody_get_neighbors' kernel timed in the same run at 9.49 ms): the kernel 6.00 / 5.94 / 6.49 / 8.63 /
 * 15.76 ms for k = 1 / 4 / 8 / 16 / 32, that is 0.63 / 0.63 / 0.68 / 0.91 / 1.66 times the nearest-neighbour kernel: per pair
 * it does less (no overlap count, no selects), and pays for an insertion only when some row of a wave lists the source.  The
 * list has a capacity tier of 4, 8, 16 or 32 entries, the smallest that holds k, so k = 1 costs what k = 4 costs.  Whole
 * Stepper.knn() calls, with the copy of n x k x 12 bytes and their split into two arrays: 6.1 / 6.6 / 8.2 / 17.0 / 32.4 ms,
 * next to 9.7 ms for Stepper.neighbors().  65536 explicit points at k = 8 on that state: 5.74 ms of kernel, 6.3 ms the call.  A
 * batch of 256 x 1024 with points == NULL at k = 8: 0.37 ms of kernel, 3.9 ms for StepperBatch.knn() with its 25 MB of
 * results.  Not measured: any other precision, state or k; the cost between the tiers' boundaries is the upper tier's.
 * nbody_batch_get_knn: the same query for every system of a batch in ONE launch, whatever S is, with the one set of points
 * and the one k for all of them (systems x m x k x 12 bytes at most 2^31).  Explicit points: system s's entries at
 * [(s * m + p) * k + c].  points == NULL: at [(s * capacity + i) * k + c], one row per current body, the rest of the slice
 * is left unchanged.  System s gives exactly what an nbody_ctx holding that system's state gives; an empty system gives
 * {+inf, -1} in every entry of every explicit point and writes nothing in the own form.  A count outside [0, capacity] is
 * treated as 0 and reported for that system, as by nbody_batch_get_neighbors.
 * ------------------------------------------------------------------------------------------------- */
#define NBODY_KNN_MAX 32
int nbody_get_knn(nbody_ctx* ctx, const nbody_vec2* points, int m, int k, double* d2, int32_t* index, int* n_out);
int nbody_batch_get_knn(struct nbody_batch* b, const nbody_vec2* points, int m, int k, double* d2, int32_t* index);

/* ---------------------------------------------------------------------------------------------------
 * Shell sums (the reference has none): for every row - a current body, or an arbitrary probe point - the
 * mass and the number of the current bodies in each shell of distance around it, 1 <= bins <= NBODY_SHELLS_MAX: what a
 * local surface density, the enclosed mass M(<r), a half-mass radius or the density profile of a clump is made of; the
 * per-row, mass-weighted counterpart of nbody_get_pair_counts.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  The
 * records are (X_j, Y_j, M_j) of the n current bodies, widened exactly from fp32 or taken as they are from fp64.  Radii and
 * velocities play no part.  For a row at (x, y) and a source j:
 *     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)               the d2 of nbody_get_neighbors, same bits
 *     in(k, j)  <=>  edges2[k] <= d2_j && d2_j < edges2[k+1]                k = 0 .. bins-1, the rule of nbody_get_pair_counts
 *     count[row*bins + k] = the number of sources j with in(k, j)
 *     mass [row*bins + k] = acc after:  acc = +0.0;  for j = 0 .. n-1 ascending:  if in(k, j)  acc = acc + M_j
 * The order of the mass sum is part of the contract, as it is for the field and the diagnostics: the masses span thirteen
 * decades.  edges2 follows the rules of nbody_get_pair_counts: bins + 1 squared edges, strictly increasing, no NaN,
 * edges2[0] >= 0, the last edge may be +inf; the one difference is 1 <= bins <= NBODY_SHELLS_MAX.
 * What is left out: a source below the first edge, a source at or above the last edge and a NaN d2 are not counted anywhere;
 * a +inf d2 is not counted even under a +inf top edge.  There is no `below` and no `rest`: a caller who wants everything
 * sends edges2[0] = 0.
 * Own form (points == NULL): the rows are the current bodies, taken on the device; the self term is excluded by index, so a
 * second body at the same place is a source at d2 = +0 and lands in bin 0 where edges2[0] == 0; m is the room in rows,
 * *n_out the current count n; m < n is NBODY_ERR_CAPACITY with nothing written.  Points form: m probe points, always
 * nbody_vec2, no self exclusion; *n_out = m; m == 0 is legal and launches nothing.
 * What follows from the definition:
 *   - count is exact whatever order the device counts in;
 *   - mass is a function of the state, the row and the edges only: it does not depend on rank, world, transport, force
 *     kernel, m, the row's place in `points`, or the capacity tier the kernel runs at;
 *   - the mass of bin k under edges [.., a, b, ..] equals the mass of the one bin of a call with edges [a, b]: bins are
 *     independent of each other;
 *   - it is independent of the semantics: a literal context's frozen tail is a source like any other body;
 *   - a body of mass 0 counts and adds +0; a NaN mass makes its bin's mass NaN and still counts;
 *   - summed over the own rows, count[:, k] is exactly twice nbody_get_pair_counts' counts[k] for the same edges; summed
 *     over explicit points it is exactly its DR counts[k];
 *   - where every mass is 1.0, mass == count exactly.
 * nbody_get_shells follows nbody_get_knn in every respect not named here.  It synchronises, reads the replica only and never
 * changes what later steps compute: stepping after any number of calls is bit-identical to stepping without them.  It is NOT
 * collective: any rank of any world, a rank of a NBODY_FLAG_GROUP_EXCHANGE group and a NBODY_FLAG_FORCE_COMM context each
 * give the same bits.  The device points, the device entries (12 bytes each) and their pinned staging are allocated on the
 * first call and grown; the edges travel as a kernel argument.  A context that never calls it allocates nothing, launches
 * nothing more, and the kernels it runs keep their code.
 * NBODY_ERR_INVALID, found before any device call: NULL ctx, edges2, mass, count or n_out; bins outside
 * [1, NBODY_SHELLS_MAX]; a bad edge (as nbody_get_pair_counts reports it); m < 0; m x bins x 12 bytes above 2^31 (in the own
 * form too, where m is the room).  NBODY_ERR_STATE: before an upload.
 * Cost (one MI355X, fp32, the N = 262144 state after 3 steps, n = 130965; profiles/shells_probe.txt, a kernel trace with
 * nbody_get_pair_counts' kernel timed in the same run, medians of 3 rounds, spreads <= 0.1 ms).  The accumulators have a
 * capacity tier of 4, 8, 16 or 32 bins, the smallest that holds `bins`.  Per pair the kernel does what the points form of
 * nbody_get_pair_counts does, and pays for its sums only where some row of a wave has a source below the top edge.  On 65536
 * explicit points and the same 32 edges: 5.200 ms against 5.203 ms for nbody_get_pair_counts where 6.8e-6 of the pairs are in
 * range (top edge 381.8 as a length), 5.767 against 5.363 ms (1.075) where 4.9e-5 are (824.8).  points == NULL: 5.76 / 5.90 ms
 * for 8 / 32 bins under the first top edge, 6.27 / 6.94 ms under the second - every ordered pair is walked, yet that is 1.11 to
 * 1.25 times the triangular nbody_get_pair_counts call (5.20 / 5.54 ms), not twice: the full walk is even over the workgroups.
 * One bin [0, +inf), every pair added: 26.45 ms.  Whole Stepper.shells() calls add the copy of rows x bins x 12 bytes and its
 * split into two arrays: 7.2 ms at 8 bins, 17.0 / 17.4 ms at 32 bins (50 MB).  A batch of 256 x 1024 with points == NULL and 8
 * bins: 0.133 ms of kernel, 3.1 ms for StepperBatch.shells() with its 25 MB of results.  Not measured: fp64 records, other
 * states, bins between the tiers (the cost is the upper tier's by construction).
 * nbody_batch_get_shells: the same query for every system of a batch in ONE launch, whatever S is, with the one set of
 * points and edges for all of them (systems x m x bins x 12 bytes at most 2^31).  Explicit points: system s's entries at
 * [(s * m + p) * bins + k].  points == NULL: at [(s * capacity + i) * bins + k], one row per current body, the rest of the
 * slice is left unchanged.  System s gives exactly the bits an nbody_ctx holding that system's state gives; an empty system
 * gives {+0.0, 0} in every bin of every explicit point and writes nothing in the own form.  A count outside [0, capacity] is
 * treated as 0 and reported for that system, as by nbody_batch_get_knn.
 * ------------------------------------------------------------------------------------------------- */
#define NBODY_SHELLS_MAX 32
int nbody_get_shells(nbody_ctx* ctx, const nbody_vec2* points, int m, const double* edges2, int bins,
                     double* mass /* [rows * bins] */, int32_t* count /* [rows * bins] */, int* n_out);
int nbody_batch_get_shells(struct nbody_batch* b, const nbody_vec2* points, int m, const double* edges2, int bins,
                           double* mass, int32_t* count);

/* ---------------------------------------------------------------------------------------------------
 * Shell moments (the reference has none): nbody_get_shells with the velocities.  For every row - a current
 * body with its own velocity, or a probe point with a velocity of its own - and every bin of squared distance, nine fp64
 * running sums and a count over the sources in the bin, 1 <= bins <= NBODY_SHELL_MOMENTS_MAX: what a velocity dispersion
 * profile, the mean radial and tangential motion of a clump (is it contracting? rotating?), the angular momentum around an
 * accreting body or an anisotropy is made of.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, no divide,
 * no square root.  The records are (X_j, Y_j, VX_j, VY_j, M_j) of the n current bodies, widened exactly from fp32 or taken
 * as they are from fp64.  Radii play no part.  For a row at (x, y) with velocity (vx, vy) and a source j:
 *     dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)               the d2 of nbody_get_shells, same bits
 *     in(k, j)  <=>  edges2[k] <= d2 && d2 < edges2[k+1]                  the rule of nbody_get_shells
 *     ux = VX_j - vx;  uy = VY_j - vy
 *     w2 = (ux*ux) + (uy*uy)
 *     s  = (dx*ux) + (dy*uy)                                              d . u  = r v_r
 *     c  = (dx*uy) - (dy*ux)                                              d x u  = r v_t
 * and per (row, k) each sum is  acc = +0.0;  for j = 0 .. n-1 ascending:  if in(k, j)  acc = acc + term  with the terms
 *     mass  M_j            the bits of nbody_get_shells
 *     px    M_j*ux         momentum relative to the row
 *     py    M_j*uy
 *     ke    M_j*w2         twice the kinetic energy relative to the row
 *     mr2   M_j*d2         moment of inertia about the row
 *     rad   M_j*s          half of d(mr2)/dt: its sign tells infall from outflow
 *     ang   M_j*c          angular momentum about the row
 *     rad2  M_j*(s*s)      r^2-weighted radial second moment
 *     ang2  M_j*(c*c)      r^2-weighted tangential second moment
 * count is the number of sources with in(k, j); pad is 0.  The result is [rows * bins] records of 80 bytes, a row's bins next
 * to each other: out[row*bins + k].  The order of every sum is part of the contract.
 * Bins: 1 <= bins <= NBODY_SHELL_MOMENTS_MAX = 8.  The accumulators are registers, nine doubles per bin, and a tier of 16
 * bins would not fit without scratch memory; a caller with more bins makes several calls over adjoining edges, which give the
 * same bits bin for bin (below).  edges2 follows the rules of nbody_get_shells: bins + 1 squared edges, strictly increasing,
 * no NaN, edges2[0] >= 0, the last edge may be +inf.
 * What is left out: a source below the first edge, a source at or above the last edge and a NaN or +inf d2 are counted
 * nowhere, as in nbody_get_shells.
 * Own form (points == NULL): the rows are the current bodies with their own velocities, taken on the device; the self term is
 * excluded by index; m is the room in rows, *n_out the current count n; m < n is NBODY_ERR_CAPACITY with nothing written.
 * Points form: m probe points with the velocities point_vel[p], or at rest with point_vel == NULL - V - (+0.0) is V bit for
 * bit, so a point at rest and a point_vel of zeros give the same bits; no self exclusion; *n_out = m; m == 0 is legal and
 * launches nothing.  point_vel without points is NBODY_ERR_INVALID.
 * What follows from the definition:
 *   - mass and count have the bits of nbody_get_shells for the same edges and rows;
 *   - every sum is a function of the state, the row, its velocity and the two edges of its bin only: bins are independent of
 *     each other, of the capacity tier the kernel runs at (4 or 8), of m and of the row's place in `points`;
 *   - with every source at rest and the row at rest every velocity sum (px, py, ke, rad, ang, rad2, ang2) is +0.0;
 *   - where every mass is 1.0, mass == count exactly;
 *   - a NaN velocity of source j makes the velocity sums of its bin NaN and it still counts; mass and mr2 stay as they were.
 *     A NaN is a NaN: IEEE 754 leaves the sign and the payload of a NaN result open, and they are no part of the contract
 *     (the device subtracts by adding the negated operand, which flips the sign of a NaN operand);
 *   - it is independent of the semantics: a literal context's frozen tail is a source like any other body.
 * It synchronises and never changes what later steps compute.  The velocities of other ranks' bodies are not on a rank, so
 * the query needs a single-rank context: NBODY_ERR_STATE on a context with world > 1, NBODY_FLAG_GROUP_EXCHANGE or
 * NBODY_FLAG_FORCE_COMM, as for nbody_get_encounters and the jerk of nbody_get_tides.  The device points, their velocities,
 * the device records and their pinned staging are allocated on the first call and grown; the edges travel as a kernel
 * argument.  A context that never calls it allocates nothing and the kernels it runs keep their code.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: bins outside [1, NBODY_SHELL_MOMENTS_MAX];
 * point_vel without points; NULL edges2; m < 0; m x bins x 80 bytes above 2^31 (in the own form too, where m is the room); a
 * bad edge (as nbody_get_pair_counts reports it); NULL ctx, out or n_out.  NBODY_ERR_STATE: before an upload; more than one
 * rank.
 * Cost: DESIGN.md 4.19 has the counts and what was measured.  Per pair the kernel does what nbody_get_shells does and pays
 * for its sums only where some row of a wave has a source below the top edge.
 * nbody_batch_get_shell_moments: the same query for every system of a batch in ONE launch, with the one set of points, point
 * velocities and edges for all of them (systems x m x bins x 80 bytes at most 2^31), in nbody_batch_get_shells' layouts.
 * Explicit points: system s's records at [(s * m + p) * bins + k].  points == NULL: at [(s * capacity + i) * bins + k], one
 * row per current body, the rest of the slice is left unchanged.  System s gives exactly the bits an nbody_ctx holding that
 * system's state gives; an empty system gives zeroed records for every explicit point and writes nothing in the own form.
 * ------------------------------------------------------------------------------------------------- */
#define NBODY_SHELL_MOMENTS_MAX 8
typedef struct nbody_shell_moment {
    double mass, px, py, ke, mr2, rad, ang, rad2, ang2;
    int32_t count;
    int32_t pad;                     /* 0 */
} nbody_shell_moment;                /* 80 bytes */
int nbody_get_shell_moments(nbody_ctx* ctx, const nbody_vec2* points, const nbody_vec2* point_vel, int m, const double* edges2,
                            int bins, nbody_shell_moment* out /* [rows * bins] */, int* n_out);
int nbody_batch_get_shell_moments(struct nbody_batch* b, const nbody_vec2* points, const nbody_vec2* point_vel, int m,
                                  const double* edges2, int bins, nbody_shell_moment* out);

/* ---------------------------------------------------------------------------------------------------
 * Group finding (the reference has none): friends-of-friends.  Which of the n current bodies hang together,
 * and how many clumps there are: the connected components of the graph of linked pairs.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, on the
 * records of nbody_get_neighbors: (X, Y, R) of every current body, widened exactly from fp32 or taken as it is from fp64.
 * For two bodies i != j
 *     dx = X_j - X_i;  dy = Y_j - Y_i;  d2 = (dx*dx) + (dy*dy)
 *     s  = (radius_scale * (R_i + R_j)) + link
 *     linked(i, j)  <=>  d2 <= s*s
 * link is a length: link >= 0, +inf allowed; radius_scale is finite and >= 0.  A group is a connected component of the
 * undirected graph of links, and label[i] is the LOWEST INDEX in body i's group.  What follows from it:
 *   - linked is symmetric bit for bit (dx only changes sign, R_i + R_j is commutative);
 *   - a NaN d2 or a NaN s*s links nothing: a body with a NaN coordinate is a group of its own;
 *   - with radius_scale = 1 and link = 0 the predicate is exactly the overlap predicate of nbody_get_neighbors (1*x and
 *     x + 0 are exact where it matters: s*s has the same bits), so body i's number of links equals its `overlaps`;
 *   - with radius_scale = 0 it is classical friends-of-friends on the centres with linking length `link`;
 *   - label[label[i]] == label[i] and label[i] <= i; n_groups is the number of i with label[i] == i;
 *   - the result is a function of the state and the two parameters only: an implementation may find it any way it likes as
 *     long as it returns exactly this;
 *   - it is independent of the semantics: a literal context's frozen tail is a body like any other; the masses play no part.
 * info: n_bodies = n; n_groups; largest = the size of the biggest group (0 for no bodies); sweeps = the pair-walk launches
 * the call made, informational (for a batch the one number of the whole call, repeated in every record).
 * nbody_get_groups follows nbody_get_neighbors with points == NULL in every respect: it synchronises, reads the replica only
 * and never changes what later steps compute; it is NOT collective - any rank of any world or transport may call it on its
 * own and each gives the same labels; cap is the room in label, cap < n is NBODY_ERR_CAPACITY with nothing written; n == 0
 * launches nothing and gives {0, 0, 0, 0}.  The device arrays and their pinned staging are allocated on the first call; a
 * context that never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: a NaN or negative link; a NaN, negative or infinite radius_scale; NULL
 * ctx, label or info; cap < 0.  NBODY_ERR_STATE: before an upload.  A device-side failure is reported as by every
 * synchronising call.
 * How (csrc/nbody_groups.hpp): hook and repeat over a parent array in device memory - a triangular pair walk (j < i) that on
 * a linked pair with different roots lowers the larger root's parent to the smaller with one atomicMin, repeated until a
 * walk changes nothing (at most n + 1 walks; 4 bytes per system come back after each), then label[i] = root of i.  No
 * device-side waiting, no retry loop.
 * Cost (one MI355X, fp32; profiles/groups_probe.txt): the stock state of N = 262144, n = 130965 bodies after 3 steps.  A whole
 * call with (link, radius_scale) = (0, 1) 14.7 ms, with a centre-only link that gives many small groups (381.8: 77493 groups,
 * the largest 21) 14.8 ms, with one that percolates (824.8: 21 groups, the largest 130937) 16.9 ms, each 2 sweeps, against 9.6
 * ms for nbody_get_neighbors with points == NULL on that state.  A sweep's kernel 7.1 / 7.2 / 8.3 ms: 0.76 / 0.79 / 0.92 of
 * neighbors_at's own-form kernel timed in the same run (9.1 - 9.4 ms), not the 0.5 its pair count suggests - the workgroup
 * with the last rows walks the whole replica, and with every workgroup resident at once the busiest CU has 1.5 times the mean
 * work; the percolating link adds two finds per linked pair.  A batch of 256 x 1024: 0.91 ms per call with (0, 1) (2 sweeps of
 * 0.124 ms against neighbors_at's 0.136 ms) and 1.17 ms on a many-small-groups link (3 sweeps of 0.19 / 0.16 / 0.13 ms: the
 * hooks of a system's four workgroups sit on the critical path, so a sweep can cost more than neighbors_at), against 1.94 ms
 * for nbody_batch_get_neighbors.
 * nbody_batch_get_groups: the same for every system of a batch, every sweep ONE launch for the whole batch, whatever S is;
 * the batch sweeps until no system changed, systems that have converged leave at once.  System s's labels go to
 * label + s * capacity, one per current body, the rest of the slice is left unchanged (the layout of
 * nbody_batch_get_neighbors); info: one record per system.  System s gives exactly what an nbody_ctx holding that system's
 * state gives; an empty system gives {0, 0, 0, sweeps}.  A count outside [0, capacity] is treated as 0 and reported for that
 * system, as by nbody_batch_get_neighbors.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_groups_info { int32_t n_bodies, n_groups, largest, sweeps; } nbody_groups_info;   /* 16 bytes */
int nbody_get_groups(nbody_ctx* ctx, double link, double radius_scale, int32_t* label, int cap, nbody_groups_info* info);
int nbody_batch_get_groups(struct nbody_batch* b, double link, double radius_scale, int32_t* label, nbody_groups_info* info);

/* ---------------------------------------------------------------------------------------------------
 * Group energies (the reference has none): is a group held together by its own gravity?  The O(N^2) part on
 * the device, the O(N) catalogue in plain C on the host.
 * nbody_get_group_potential: with label[] the labels of nbody_get_groups for the same (link, radius_scale), for every
 * current body i
 *     phi_in[i] = -G * sum_{ j != i, label[j] == label[i], r_ij > 0 }  m_j / r_ij
 * ONE running sum over j = 0 .. n-1 ascending, in fp64 on exactly widened records, a term being that of
 * nbody_get_diagnostics (d2 = fma(dx, dx, dy*dy), the refined reciprocal square root, s = fma(m_j, y, s)).
 * The contract in bits, the sub-state rule: let a group's members be i_0 < i_1 < ... < i_k; phi_in[i_a] has the bits that
 * nbody_get_diagnostics puts in phi[a] for a context holding exactly those k + 1 bodies in that order.  A body that is no
 * member is left out: its pair never reaches the sum, not even as a NaN.  Members at distance exactly 0 are left out and
 * counted, as by the diagnostics; a row whose fast sum is not finite is redone with IEEE sqrt and divide over its members.
 * label: bit for bit what nbody_get_groups returns for the same arguments; info: its four counts with the same values, and
 * coincident = the ordered pairs (i, j) of one group at distance 0.  Arguments, errors and the cap rule (room in label AND in
 * phi_in) are those of nbody_get_groups, with phi_in one more pointer that must not be NULL.  The call synchronises and reads
 * positions, masses and radii of the replica only; it never changes what later steps compute and it is NOT collective.  No
 * bodies: a zero record.  One body: phi_in[0] = -0.0 (-G * +0, as the diagnostics).
 * nbody_batch_get_group_potential: the same for every system of a batch, every sweep and the potential ONE launch each
 * whatever S is; system s's labels and potentials go to label + s * capacity and phi_in + s * capacity, the rest of each
 * slice is left unchanged; info: one record per system (an empty system: {0, 0, 0, sweeps, 0}, as nbody_batch_get_groups).
 * How (csrc/nbody_group_energy.hpp): the group finding as it is, then one lane per body over a full tile walk with the
 * labels staged next to {x, y, m}; per four sources four integer compares, and a wave none of whose rows has a member among
 * them skips the fp64 chain - exact, because a non-member is left out of the sum anyway.
 *
 * nbody_group_catalog (csrc/nbody_group_energy.c, no device): one record per group from the bodies, the labels and phi_in,
 * sorted by label ascending.  Every sum is a plain s = s + term over the group's members in ascending index, every
 * operation rounded on its own, no fma:
 *     pass 1:  mass, sum m x, sum m y, sum m vx, sum m vy;   cx = (sum m x) / mass and likewise cy, vx, vy (mass == 0: NaN)
 *     pass 2:  dvx = vx_i - vx;  dvy = vy_i - vy;  w = (dvx*dvx) + (dvy*dvy);  K2 += m_i * w;  P += m_i * phi_in_i;
 *              bound member  <=>  ((0.5*w) + phi_in_i) < 0
 *     kinetic = 0.5*K2;  potential = 0.5*P;  energy = kinetic + potential;  flags bit 0: energy < 0
 * Groups past cap are counted in *n_groups and not stored; out == NULL with cap == 0 returns the count.  O(n) in time and
 * memory.  NBODY_ERR_INVALID: n < 0; cap < 0; NULL n_groups; NULL out with cap > 0; with n > 0 a NULL array; a label outside
 * [0, n) or one that is not the lowest index of its class (label[label[i]] != label[i], or label[i] > i) - found before
 * anything is indexed by it.  NBODY_ERR_NOMEM: the one work array (n slots).
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_group_energy_info {
    int32_t n_bodies, n_groups, largest, sweeps;   /* nbody_groups_info's, same values */
    int64_t coincident;                            /* ordered pairs (i, j) of one group at distance 0, left out */
} nbody_group_energy_info;                         /* 24 bytes */
int nbody_get_group_potential(nbody_ctx* ctx, double link, double radius_scale, int32_t* label, double* phi_in, int cap,
                              nbody_group_energy_info* info);
int nbody_batch_get_group_potential(struct nbody_batch* b, double link, double radius_scale, int32_t* label /* [systems * capacity] */,
                                    double* phi_in /* [systems * capacity] */, nbody_group_energy_info* info /* [systems] */);

#define NBODY_GROUP_BOUND 1u                       /* nbody_group_record.flags bit 0: energy < 0 */
typedef struct nbody_group_record {
    double mass, cx, cy, vx, vy;     /* total mass, centre of mass, its velocity            */
    double kinetic, potential;       /* T in the centre-of-mass frame; W = 0.5 sum m_i phi_in */
    double energy;                   /* T + W                                               */
    int32_t label, count;            /* lowest member index; members                        */
    int32_t bound_members, flags;    /* members with 0.5|v_i - V|^2 + phi_in_i < 0; bit 0: energy < 0 */
} nbody_group_record;                /* 80 bytes */
int nbody_group_catalog(int n, const double* x, const double* y, const double* vx, const double* vy, const double* m,
                        const int32_t* label, const double* phi_in, nbody_group_record* out, int cap, int32_t* n_groups);

/* ---------------------------------------------------------------------------------------------------
 * Pair-separation counts (the reference has none): how many pairs lie in each bin of separation - the DD
 * (bodies with bodies) and DR (probe points with bodies) counts from which a two-point correlation function, a radial
 * distribution function g(r) or a Landy-Szalay estimate is made.  The one read-out that says how the bodies lie relative to
 * each other; it has no per-body result.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, on the
 * records (X, Y) of the n current bodies, widened exactly from fp32 or taken as they are from fp64; radii and masses play
 * no part.  For a row at (x, y) and a source j
 *     dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)                  the d2 of nbody_get_neighbors
 * edges2[0 .. bins] are bins + 1 SQUARED edges, 1 <= bins <= 256: strictly increasing, no NaN, edges2[0] >= 0, and
 * edges2[bins] may be +inf.  Then
 *     counts[k] = the number of counted pairs with  edges2[k] <= d2 && d2 < edges2[k+1]      k = 0 .. bins-1
 *     below     = the number with  d2 < edges2[0]
 *     rest      = pairs - below - (the sum of counts)
 * rest is DERIVED, on the host, not counted: it holds every counted pair whose d2 is >= edges2[bins] or NaN (a +inf d2 - a
 * coordinate near 1e200 - is in rest even where edges2[bins] is +inf, since +inf < +inf fails).
 * Own form (points == NULL): the counted pairs are the unordered pairs i < j of the n current bodies, each once:
 * pairs = n (n - 1) / 2, rows = n; m is not used beyond its check.  d2_ij and d2_ji have the same bits (dx and dy only change sign), so one orientation
 * suffices and the result does not depend on which.  Two distinct bodies at the same place are a pair at d2 = +0: in
 * counts[0] where edges2[0] == 0, else in below.
 * Points form (points != NULL): m probe points, always nbody_vec2 (double); the counted pairs are ALL (point, body) pairs:
 * pairs = m n, rows = m, no self exclusion (a point on a body is a pair at d2 = +0).  m == 0 is legal and launches nothing.
 * info: n_bodies = n, rows, pairs, below, rest as above.  What follows from the definition:
 *   - the counts are integers, so they are exact whatever order an implementation adds them in;
 *   - they are a function of the state and the edges only;
 *   - they are independent of the semantics: a literal context's frozen tail counts like any other body.
 * nbody_get_pair_counts follows nbody_get_groups: it synchronises, reads the replica only and never changes what later
 * steps compute; it is NOT collective - any rank of any world or transport may call it on its own and each gives the same
 * numbers.  The device edges, histogram and points and their pinned staging are allocated on the first call; a context that
 * never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: NULL ctx, edges2, counts or info; bins outside [1, 256]; an edge that is
 * NaN, negative or not above its predecessor; m < 0; m x 16 bytes above 2^31 (the limit nbody_get_neighbors sets on its
 * points).  NBODY_ERR_STATE: before an upload.  A device-side failure is reported as by every synchronising call.
 * How (csrc/nbody_pairs.hpp): one lane per row over the tile walk of the row queries - triangular (j < i) in the own form,
 * full in the points form.  A pair costs 2 subtractions, 2 multiplies, 1 add and ONE compare, d2 < edges2[bins]; only a pair
 * below the top edge goes on to a binary search over the edges in LDS and one 64-bit LDS atomic add; a workgroup adds its
 * non-zero counters to the system's histogram in device memory once, at its end.  Cheap where the top edge is small against
 * the system (the clustering use), correct but slower where the edges cover every separation.
 * Cost (one MI355X, fp32; profiles/pairs_probe.txt): the stock state of N = 262144, n = 130965 bodies after 3 steps (8.58e9
 * pairs), points == NULL, 32 logarithmic bins.  Top edge at the sparse centre link of the group probe (381.8; 6.8e-6 of the
 * pairs below it): the kernel 5.49 ms, the whole call 5.47 ms under the host clock; top edge at the percolating link (824.8;
 * 4.9e-5 of the pairs): 5.72 and 5.73 ms.  groups_sweep at (0, 1), which walks the same triangle, took 7.27 ms in the same run:
 * 0.755 and 0.787 of it (2 LDS reads per pair against 3, 6 fp64 instructions against 10), and a call is one walk where
 * nbody_get_groups makes two (14.6 ms).  With a last bin up to +inf every pair takes the search and the LDS atomic: 81.1 ms,
 * 11.1 times a sweep - correct, not the use this shape is for.  A batch of 256 x 1024: 0.12 ms of kernel and 0.48 ms per
 * call on the sparse edges of its density (1.4e-3 of the pairs in range), 1.08 ms and 1.45 ms with a last bin up to +inf.
 * nbody_batch_get_pair_counts: the same for every system of a batch in ONE launch, whatever S is, with the one set of
 * points and edges for all of them: system s's counts at counts[s * bins + k], its record at info[s].  System s gives
 * exactly what an nbody_ctx holding that system's state gives; an empty system gives all zeros (rows = m in the points
 * form).  A count outside [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_get_neighbors.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_pair_info { int64_t n_bodies, rows, pairs, below, rest; } nbody_pair_info;   /* 40 bytes */
int nbody_get_pair_counts(nbody_ctx* ctx, const nbody_vec2* points, int m, const double* edges2, int bins, uint64_t* counts,
                          nbody_pair_info* info);
int nbody_batch_get_pair_counts(struct nbody_batch* b, const nbody_vec2* points, int m, const double* edges2, int bins,
                                uint64_t* counts /* [systems * bins] */, nbody_pair_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Encounter queries (the reference has none): swept contacts within a horizon, by pair.  The stepper finds a
 * collision only where two bodies overlap at the start of a step (d2 <= (r_i + r_j)^2 on the positions of that instant); a
 * pair that closes faster than (r_i + r_j) / dt can pass straight through.  This read-out says which pairs touch within the
 * next h seconds if every body keeps its velocity, when, and which of them a step test at 0 and at h sees at neither end.
 * PHYSICS: this is the UNIFORM-MOTION estimate, not the stepper's own trajectory.  It leaves out the acceleration within the
 * horizon and the wall rule; it predicts the stepper exactly only where one step moves a body by fl(x + dt v).
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, on the
 * records (X, Y, R) and velocities (VX, VY) of the n current bodies, widened exactly from fp32 or taken as they are from
 * fp64; masses play no part.  h is the horizon in seconds: h >= 0, +inf allowed.  For an unordered pair i < j
 *     dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
 *     d2 = (dx*dx) + (dy*dy);   s = R_i + R_j;   s2 = s*s;   c = d2 - s2
 *     b  = (dx*dvx) + (dy*dvy); a = (dvx*dvx) + (dvy*dvy);   disc = (b*b) - (a*c)
 *     ex = dx + (dvx*h);        ey = dy + (dvy*h);            e2 = (ex*ex) + (ey*ey)
 *     now = d2 <= s2                                  the overlap predicate of nbody_get_neighbors, same bits
 *     end = e2 <= s2                                  overlap at time h under uniform motion
 *     mid = b < 0 && (-b) < (a*h) && disc >= 0        closest approach before h, and close enough
 *     swept = now || end || mid
 *     t = now ? +0 : (b < 0 && disc >= 0) ? min(c / (sqrt(disc) - b), h) : h         min(x, h) = x < h ? x : h
 * A swept pair is reported as {t, i, j, flags} with i < j; flags has NBODY_ENCOUNTER_NOW where now holds and
 * NBODY_ENCOUNTER_END where end holds (both may be set).  A swept pair with neither bit is MISSED: it touches strictly inside
 * (0, h) and overlaps at neither end, so with h = dt the stepper's test sees it at neither step.  The list is sorted by
 * (t, i, j) ascending.  info: n_bodies = n; pairs = the swept pairs; now / end = those with the bit; missed = those with
 * neither; horizon = h.  What follows from the definition:
 *   - symmetry: the predicate and t are symmetric bit for bit - the four differences only change sign and every product
 *     holds two of them - so one orientation suffices;
 *   - NaN: a NaN coordinate or radius makes d2, e2, b or s2 NaN, every comparison fails and the pair is not swept.  A NaN
 *     velocity does the same to end and mid; `now` does not read the velocities, so a pair that overlaps is still reported,
 *     with t = +0;
 *   - infinite horizon: with h = +inf, end holds only where s2 is +inf, and a*h is +inf or NaN, so for finite radii
 *     swept = now || (b < 0 && a > 0 && disc >= 0): every pair on a collision course;
 *   - zero horizon: with h = 0, ex = dx + (dvx*0) squares to what dx squares to wherever the velocities are finite, so end
 *     equals now, and a*0 is not above -b, so mid never holds: swept = now, and info.now is half the sum of `overlaps` of
 *     nbody_get_neighbors with points == NULL;
 *   - it is independent of the semantics, like the other read-outs: a literal context's frozen tail counts with its stored
 *     velocity;
 *   - the result is a function of the state and h only: the device appends in any order, the sort fixes the list.
 * Division of labour: the device decides swept and the flags for all n (n - 1) / 2 pairs, with subtractions, multiplies,
 * additions and compares only, counts pairs / now / end / missed in 64-bit integers, and appends a raw record per swept pair
 * - nbody_encounter_raw: i, j, flags, c, b, disc - to a log of cap records per system; records past cap are counted, not
 * stored.  nbody_encounter_finish, a pure host function in plain C that needs no GPU, computes t from c, b, disc and h with
 * the C library's sqrt and /, orders (i, j), and sorts `count` records into out; it reads only the NOW and END bits of flags.
 * A bit-exact contract does not rest on the device's divide and square root (nbody_selftest_rcp_ones_f64 is why).
 * nbody_get_encounters synchronises, reads only, and never changes what later steps compute: state, pair counter, events,
 * tracers.  out has room for cap records; info is always filled once the walk has run.  pairs > cap: NBODY_ERR_CAPACITY, out
 * untouched, info complete - the caller repeats with cap >= info.pairs, so the list is never a nondeterministic subset.  out
 * may be NULL with cap == 0: the counts only, NBODY_OK whatever pairs is.  An empty or one-body system gives zeros.  The
 * device log, the counters and their pinned staging are allocated on the first call and grown to the largest cap seen; a
 * context that never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: a NULL handle or info; a NaN or negative horizon; cap < 0; NULL out with
 * cap > 0; cap x 24 bytes (a batch: systems x cap x 24) above 2^31.  NBODY_ERR_STATE: before an upload; on a context with
 * world > 1, NBODY_FLAG_GROUP_EXCHANGE or NBODY_FLAG_FORCE_COMM: a rank holds only its own bodies' velocities, and a query
 * across ranks has not been built (the tracers' restriction).  A device-side failure is reported as by every synchronising
 * call.
 * How (csrc/nbody_encounters.hpp): one lane per body over the triangular tile walk of nbody_get_groups (j < i, each pair once
 * at the higher row) with two more LDS planes for the velocities (10 KiB double-buffered); 5 LDS reads, 27 fp64 arithmetic
 * instructions and 5 compares per pair against groups_sweep's 3, 10 and 1, so about three times a sweep is what counting gives;
 * one 64-bit atomic per swept pair for its slot in the log, one per wave for each of the three class counts.  No device-side
 * waiting, no retry loop.  Every pair evaluates every term: skipping e2 where b >= 0 would be right for exact values only.
 * Cost (one MI355X, fp32; profiles/encounter_probe.txt): the stock state of N = 262144, n = 130965 bodies after 3 steps
 * (8.58e9 pairs, max |v| 325), every figure measured in that file.  The kernel 18.69 / 18.91 / 18.97 ms for h = 0 / the time step 0.2 / ten time steps
 * (5052 / 9201 / 35603 swept pairs, of them 0 / 0 / 433 missed): 2.61 / 2.64 / 2.65 times groups_sweep at (0, 1), which walks the
 * same triangle (7.17 ms in the same run), and 2.0 times neighbors_at's own-form kernel (9.43 ms); the number of swept pairs
 * hardly shows.  Whole Stepper.encounters() calls with room for the list: 19.2 / 19.7 / 22.2 ms (the copy, the finish and the
 * wrapper's repacking of 35603 records are the 3.3 ms); a call that has to be repeated with a larger cap walks twice (38.6
 * ms).  A batch of 256 x 1024 with h = the time step: 0.333 ms of kernel, 1.02 ms per call.  Not measured: fp64, h = +inf on
 * that state, any other state.
 * nbody_batch_get_encounters: the same for every system of a batch in ONE launch, whatever S is, with the one horizon and
 * the one cap for all of them: system s's list at out + s * cap (pairs records, the rest of the slice is left unchanged), its
 * record at info[s].  If any system has pairs > cap the call is NBODY_ERR_CAPACITY, out untouched, every info complete.
 * System s gives exactly what an nbody_ctx holding that system's state gives.  A count outside [0, capacity] is treated as
 * 0 and reported for that system, as by nbody_batch_get_neighbors.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_encounter { double t; int32_t i, j; uint32_t flags, reserved; } nbody_encounter;   /* 24 bytes */
typedef struct nbody_encounter_info { int64_t n_bodies, pairs, now, end, missed; double horizon; } nbody_encounter_info;
typedef struct nbody_encounter_raw { int32_t i, j; uint32_t flags, reserved; double c, b, disc; } nbody_encounter_raw;   /* 40 bytes */
enum { NBODY_ENCOUNTER_NOW = 1u << 0, NBODY_ENCOUNTER_END = 1u << 1 };
int nbody_get_encounters(nbody_ctx* ctx, double horizon, nbody_encounter* out, int cap, nbody_encounter_info* info);
int nbody_batch_get_encounters(struct nbody_batch* b, double horizon, nbody_encounter* out /* [systems * cap] */, int cap,
                               nbody_encounter_info* info /* [systems] */);
int nbody_encounter_finish(const nbody_encounter_raw* raw, int count, double horizon, nbody_encounter* out /* [count] */);

/* ---------------------------------------------------------------------------------------------------
 * Bound-pair queries (the reference has none): two-body binaries within a separation.  Which pairs of bodies
 * are gravitationally bound to each other, and on what orbit: the precursor of nearly every merger of this stepper, and the
 * binary census that goes with the pair counts and the groups.  The one read-out that sets masses and velocities against
 * positions.  PHYSICS: this is the ISOLATED TWO-BODY estimate on the state of this instant: the energy of the relative orbit
 * of i and j alone, every other body left out, point masses, no walls.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma, on the
 * records (X, Y, M, R) and velocities (VX, VY) of the n current bodies, widened exactly from fp32 or taken as they are from
 * fp64.  G2 = 2.0 * (double)6.67408e-11f, an exact doubling of the library's G.  sep2 is the SQUARED largest separation
 * looked at: sep2 >= 0, +inf allowed; squared like edges2 of the pair counts.  For an unordered pair i < j
 *     dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
 *     d2 = (dx*dx) + (dy*dy)                          the d2 of nbody_get_neighbors, same bits
 *     coincident = d2 == 0                            counted, never listed (no orbit)
 *     near  = 0 < d2 && d2 <= sep2
 *     v2 = (dvx*dvx) + (dvy*dvy);   mu = G2 * (M_i + M_j)
 *     w  = (v2*v2) * d2;            k  = mu * mu
 *     bound = near && 0 < mu && k < +inf && w < k     v2*r < 2G(m_i+m_j), i.e. two-body energy < 0, squared
 *     hz = (dx*dvy) - (dy*dvx);     b = (dx*dvx) + (dy*dvy);    s = R_i + R_j
 *     flags: NBODY_BINARY_OVERLAP where d2 <= s*s (the overlap predicate of nbody_get_neighbors, same bits);
 *            NBODY_BINARY_APPROACHING where b < 0
 * A bound pair is reported as {a, ecc, period, sep, i, j, flags} with i < j; the list is sorted by (i, j) ascending, a key
 * that is exact and total whatever the values are (order by `a` in the caller if wanted).  Per bound pair, from its raw
 * record {d2, v2, mu, hz}, nbody_binary_finish computes with the C library's sqrt and /
 *     r = sqrt(d2);  gm = 0.5*mu;  eps = (0.5*v2) - (gm/r)
 *     a      = eps < 0 ? gm / (-(eps+eps)) : +inf                                     semi-major axis
 *     e2     = 1.0 + (((eps+eps) * (hz*hz)) / (gm*gm));   ecc = e2 > 0 ? sqrt(e2) : +0.0
 *     period = a < +inf ? 6.283185307179586 * sqrt(((a*a)*a) / gm) : +inf
 *     sep    = r
 * The guards eps < 0 and e2 > 0: the device's squared predicate and the host's rounded eps may disagree within a few ulps of
 * a parabolic orbit, and e2 may round to 0 or below within a few ulps of a circular one; the guards make the outcome defined
 * (a = period = +inf; ecc = +0), not NaN.
 * info: n_bodies = n; pairs = the bound pairs, the ones listed; near = all pairs with 0 < d2 <= sep2, bound or not (the
 * denominator of a binary fraction); coincident = the pairs i < j at d2 == 0, whatever sep2 is; overlapping / approaching =
 * the listed pairs with that bit; sep2 = the argument.  What follows from the definition:
 *   - symmetry: the predicate, hz and the flags are symmetric bit for bit - all four differences change sign together and
 *     every product holds two of them, M_i + M_j and R_i + R_j commute - so one orientation suffices and the result does not
 *     depend on which;
 *   - NaN: a NaN coordinate, velocity or mass makes every comparison it reaches fail: the pair is neither bound nor listed.
 *     A NaN position makes d2 NaN, so the pair does not count in near (or coincident) either; a NaN velocity or mass leaves
 *     the pair in near;
 *   - sep2 = +inf: every pair at finite non-zero d2 is near (a pair at d2 = +inf is too, and is never bound: w is +inf or NaN);
 *   - 2 * coincident == nbody_diag.coincident_pairs on the same state;
 *   - near + coincident == counts[0] of nbody_get_pair_counts with edges2 = {0, nextafter(sep2, +inf)} on the same state,
 *     for finite sep2;
 *   - it is independent of the semantics, like the other read-outs: a literal context's frozen tail counts with its stored
 *     velocity;
 *   - the result is a function of the state and sep2 only: the device appends in any order, the sort fixes the list.
 * Division of labour: the device decides near, bound and the flags for all n (n - 1) / 2 pairs, with subtractions,
 * multiplies, additions and compares only - boundness needs no divide and no square root - counts pairs / near / coincident
 * / overlapping / approaching in 64-bit integers, and appends a raw record per bound pair - nbody_binary_raw: i, j, flags,
 * d2, v2, mu, hz - to a log of cap records per system; records past cap are counted, not stored.  nbody_binary_finish, a
 * pure host function in plain C that needs no GPU, computes the orbit as above, orders (i, j), and sorts `count` records
 * into out; it reads only the two flag bits.
 * nbody_get_binaries synchronises, reads only, and never changes what later steps compute: state, pair counter, events,
 * tracers.  out has room for cap records; info is always filled once the walk has run.  pairs > cap: NBODY_ERR_CAPACITY, out
 * untouched, info complete - the caller repeats with cap >= info.pairs, so the list is never a nondeterministic subset.  out
 * may be NULL with cap == 0: the counts only, NBODY_OK whatever pairs is.  An empty or one-body system gives zeros.  The
 * device log, the counters and their pinned staging are allocated on the first call and grown to the largest cap seen; a
 * context or batch that never calls it allocates nothing and launches nothing more.
 * NBODY_ERR_INVALID, found before any device call: a NULL handle or info; a NaN or negative sep2; cap < 0; NULL out with
 * cap > 0; cap x 48 bytes (a batch: systems x cap x 48) above 2^31; nbody_binary_finish: count < 0, NULL raw or out with
 * count > 0.  NBODY_ERR_STATE: before an upload; on a context with world > 1, NBODY_FLAG_GROUP_EXCHANGE or
 * NBODY_FLAG_FORCE_COMM: a rank holds only its own bodies' velocities, and a query across ranks has not been built (the
 * encounters' restriction).  A device-side failure is reported as by every synchronising call.
 * How (csrc/nbody_binaries.hpp): one lane per body over the triangular tile walk of nbody_get_encounters (j < i, each pair
 * once at the higher row) with six LDS planes, x, y, m, r, vx, vy (12 KiB double-buffered).  Per pair the hot loop is that of
 * nbody_get_pair_counts: 2 LDS reads, 2 subtractions, 3 operations for d2 and one compare, d2 <= sep2, four pairs under one
 * wave-level branch.  Only a pair that passes reads the four other planes: coincident pairs are set aside, a near pair pays
 * 10 more fp64 operations and three compares for `bound`, a bound pair 8 more and two compares for hz and the flags, and
 * one 64-bit atomic for its slot in the log.  near and coincident are counted per lane in 32 bits and added per wave with
 * one 64-bit atomic each, as are the two flag counts.  A call for the counts only (cap == 0) takes no slot: its lanes count
 * the bound pairs the same way.  No device-side waiting, no retry loop.
 * Cost (one MI355X, fp32; profiles/binaries_probe.txt): the stock state of N = 262144, n = 130965 bodies after 3 steps
 * (8.58e9 pairs, max |v| 325), every figure measured in that file, in one run with nbody_get_pair_counts' kernel at the one
 * bin [0, sep2) (5.49 ms) and nbody_get_encounters' at h = the time step (18.73 ms).  At sep = 1024 (7.8e-5 of the pairs
 * near: 666502, of them 652339 bound - the stock bodies start at rest) the kernel takes 5.84 ms for the counts only, 1.07
 * times the pair counts, and 9.26 ms (1.69 times) with the list: the 652339 slot atomics, all on one address, and their
 * records are the 3.4 ms.  At sep = 128 (289 near pairs) 5.36 ms, 0.98 times the pair counts: the hot loop is that kernel's.
 * At sep2 = +inf, the counts only (every pair near, 524411846 bound): 35.2 ms, 1.88 times the encounter kernel - every pair
 * then takes the branches of the rare path one after the other.  Whole calls: the counts only 5.7 ms at sep = 1024 and 35.4
 * ms at +inf; Stepper.binaries() with room for the 652339 records 94.6 ms (the 31 MB copy, the finish's sort and the
 * wrapper's repacking are the 85 ms), 100.4 ms when it has to ask for the counts first.  A batch of 256 x 1024 at sep = 1024
 * (10247 bound pairs): 0.094 ms of kernel, 1.32 ms per call.  A list at sep2 = +inf on such a cold state pays the slot
 * atomic 5e8 times (1392 ms measured with slots taken for the counts too, before cap == 0 skipped them) and overflows any cap
 * the 2^31-byte rule admits: ask for the counts.  Not measured: fp64 contexts, any other state.
 * nbody_batch_get_binaries: the same for every system of a batch in ONE launch, whatever S is, with the one sep2 and the one
 * cap for all of them: system s's list at out + s * cap (pairs records, the rest of the slice is left unchanged), its record
 * at info[s].  If any system has pairs > cap the call is NBODY_ERR_CAPACITY, out untouched, every info complete.  System s
 * gives exactly what an nbody_ctx holding that system's state gives.  A count outside [0, capacity] is treated as 0 and
 * reported for that system, as by nbody_batch_get_neighbors.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_binary { double a, ecc, period, sep; int32_t i, j; uint32_t flags, reserved; } nbody_binary;   /* 48 bytes */
typedef struct nbody_binary_raw { int32_t i, j; uint32_t flags, reserved; double d2, v2, mu, hz; } nbody_binary_raw;   /* 48 bytes */
typedef struct nbody_binary_info { int64_t n_bodies, pairs, near, coincident, overlapping, approaching; double sep2; } nbody_binary_info;   /* 56 bytes */
enum { NBODY_BINARY_OVERLAP = 1u << 0, NBODY_BINARY_APPROACHING = 1u << 1 };
int nbody_get_binaries(nbody_ctx* ctx, double sep2, nbody_binary* out, int cap, nbody_binary_info* info);
int nbody_batch_get_binaries(struct nbody_batch* b, double sep2, nbody_binary* out /* [systems * cap] */, int cap,
                             nbody_binary_info* info /* [systems] */);
int nbody_binary_finish(const nbody_binary_raw* raw, int count, nbody_binary* out /* [count] */);

/* ---------------------------------------------------------------------------------------------------
 * Tracer particles (the reference has none): massless probes advected with every step.
 * A tracer has a position and a velocity {x, y, vx, vy}, always fp64 whatever the context's precision.  It behaves like a
 * body of mass 0 and radius 0 that nothing collides with: it is attracted by the bodies; it attracts nothing and is never a
 * source; it is never deleted and never compacted - tracer k stays tracer k.
 * A body step t turns state J_t (n_t bodies) into J_{t+1}.  That step advances every tracer once, from the field of J_t:
 *     (ax, ay, phi, coincident) = what nbody_get_field returns for the one point (x, y) on the state J_t (same bits: the
 *                                 running sums over j ascending, the same general-code replacement of a non-finite sum, a
 *                                 source at distance exactly 0 left out and counted; n_t == 0 gives +0, +0, +0, 0)
 *     dt  = the context's time step widened to double: (double)(float)desc.timestep for fp32, desc.timestep for fp64; per
 *           system for a batch
 *     dvx = dt * ax;  dvy = dt * ay
 *     with NBODY_TRACER_WALLS only (a body's wall rule with r = 0, its quirk included: the test uses ax * dt, not v):
 *           tx = x + (ax * dt);  if (tx > hi_x || tx < lo_x) vx = vx * -1.0       hi_x = fieldWidth, lo_x = -fieldWidth
 *           ty likewise with fieldHeight
 *     vx = vx + dvx;  vy = vy + dvy
 *     x  = x + (dt * vx);  y = y + (dt * vy)
 * Every operation is IEEE fp64 and rounded on its own; there is no fma outside the field sums.  The result for tracer k
 * depends on J_t, the tracer and the parameters only: not on m, on k, on the semantics or on the force kernel.  Non-finite
 * inputs may give non-finite outputs; they never disturb another tracer.  Next to the state the library keeps, per tracer,
 * the {ax, ay, phi} of the most recent advance ("last", +0 until the first) and, per system, the number of advances since
 * the tracers were set and the sum of `coincident` over those advances.
 * Stepping: nbody_step and nbody_batch_step advance the tracers inside every step they enqueue, at the cost of one more
 * launch per step (a batch: one launch for all systems, the same m per system), on the same stream, before the step's
 * commit overwrites J_t; enqueue-only, no copy and no host wait.  The body count comes from the device; a count outside
 * [0, capacity] never becomes an index: the system is treated as empty and the failure reported as by every synchronising
 * call.  nbody_debug_force_only does not advance tracers.  A context or batch that never sets tracers allocates nothing
 * and launches nothing more.
 * nbody_tracers_set replaces the tracers by t[0 .. m-1] and zeroes the counters and "last"; m == 0 removes them and frees
 * their memory.  It may be called before the first upload (stepping still needs one); it waits for the steps enqueued so
 * far.  nbody_upload and nbody_state_load leave the tracers and their counters as they are.
 * nbody_tracers_get synchronises, writes min(cap, m) records to out (and to last, unless NULL) and fills *info: steps,
 * coincident, count = m, flags; out may be NULL with cap == 0.  With no tracers set it gives count = 0 and writes nothing else.
 * nbody_batch_tracers_set: t holds systems x m records, system s's at t[s * m]; nbody_batch_tracers_get writes system s's m
 * records at out[s * m] (out NULL: only info, e.g. to learn m) and info[s].  System s has the bits an nbody_ctx with the
 * same state, parameters and tracers gives; the tracers of an empty system drift only.
 * NBODY_ERR_INVALID, found before any device call: a NULL handle (or info); NULL t with m > 0; m < 0; unknown flag bits;
 * m x 32 bytes (a batch: systems x m x 32) above 2^31; cap < 0; NULL out with cap > 0.
 * NBODY_ERR_STATE: nbody_tracers_set on a context with world > 1, NBODY_FLAG_GROUP_EXCHANGE or NBODY_FLAG_FORCE_COMM: a
 * rank's replica is a step behind for the other ranks' bodies until the exchange, and an advance against it has not been
 * built.
 * Cost (one MI355X, fp32, ms per step under the host clock, every round from a fresh upload; profiles/tracer_probe.txt): the
 * advance is the walk of nbody_get_field over explicit points and costs what that costs.  N = 262144 with 65536 tracers: the
 * first step 30.3 -> 43.2, +12.8 (one field call for those points on that state: 13.2; 0.42 of the step, 0.48 expected from
 * 13.9 against 28.7 above); over 4 steps, while the stock state merges to half its bodies, 16.1 -> 24.0, +7.9.  1048576
 * tracers: the first step +150.8 (the field call 162.0), over 4 steps +96.6.  A batch of 256 x 1024 with 1024 tracers per
 * system: 0.234 -> 0.390, +0.157 over 20 steps.  The route this replaces - per step nbody_get_field, an update on the host,
 * nbody_step(1) - adds 13.9 / 7.2 (M = 65536, first step / 4 steps), 168.9 / 108.9 (M = 1048576) and, with one set of
 * points for all systems, 1.48 for the batch: its wait per step is what a batch step costs several times over, it is a
 * tenth of a million tracers' walk, and at M = 65536 it is repaid because the wait tells the host the current body count
 * for the next step's grids.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_tracer { double x, y, vx, vy; } nbody_tracer;                 /* 32 bytes */
typedef struct nbody_tracer_info { int64_t steps, coincident; int32_t count; uint32_t flags; } nbody_tracer_info;
enum { NBODY_TRACER_WALLS = 1u << 0 };
int nbody_tracers_set(nbody_ctx* ctx, const nbody_tracer* t, int m, uint32_t flags);   /* m == 0 removes and frees */
int nbody_tracers_get(nbody_ctx* ctx, nbody_tracer* out, nbody_field* last /* may be NULL */, int cap, nbody_tracer_info* info);
int nbody_batch_tracers_set(struct nbody_batch* b, const nbody_tracer* t /* [systems * m] */, int m, uint32_t flags);
int nbody_batch_tracers_get(struct nbody_batch* b, nbody_tracer* out /* [systems * m] */, nbody_field* last,
                            nbody_tracer_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Cell sums (the reference has none): for every cell of a caller-given uniform grid the number, the mass, the
 * momentum and twice the kinetic energy of the current bodies in it - what a surface density map, a mean velocity or a
 * dispersion map and a counts-in-cells statistic are made of - and on request the cell of every body and the cell list in
 * CSR form: cell offsets plus the bodies in cell order.  The one query about a place rather than a body or a point, the one
 * query whose cost is O(n), and the project's only spatial index.
 * The grid: nx x ny cells from (x0, y0), sx and sy cells per unit length.  The caller computes sx and sy once (Python's
 * make_grid: sx = nx / (x1 - x0) in fp64) and the definition uses those doubles as they are.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  Body j
 * with the record (X, Y, M) and the velocity (VX, VY), widened exactly from fp32 or taken as they are from fp64:
 *     tx = (X - x0) * sx;   ty = (Y - y0) * sy
 *     inside(j)  <=>  0 <= tx && tx < nx && 0 <= ty && ty < ny      decided on the doubles; a NaN is outside
 *     cell(j) = (int)ty * nx + (int)tx   if inside(j), else -1      converted only after the compares
 * so a coordinate of 1e30 never reaches a float-to-int conversion, a body on a cell boundary belongs to the cell above and
 * to the right, a body at the grid's upper bound is outside and -0.0 at x0 = 0 is in column 0.  Per cell c, with its members
 * - the bodies with cell(j) == c - taken in ASCENDING j and every accumulator starting at +0.0:
 *     count = the number of members;   first = the lowest member index, -1 for an empty cell
 *     mass = mass + M
 *     px = px + (M*VX);   py = py + (M*VY);   k2 = k2 + (M*((VX*VX) + (VY*VY)))
 * The order of the sums is part of the contract, as for every fp64 sum of this library: the masses span thirteen decades.
 * Without NBODY_CELLS_MOMENTS the velocities are not read and px, py and k2 are +0.0; mass, count and first are the same
 * bits either way.  Radii play no part.  The optional lists, each NULL or given:
 *     cell_of[j] = cell(j)                                           j = 0 .. n-1
 *     start[c]   = the exclusive prefix sum of the counts            c = 0 .. nx*ny;  start[nx*ny] = inside
 *     order[start[c] .. start[c+1])  = the members of c in ascending index;  `inside` entries in all
 * order needs start; cap is the room of cell_of and of order in entries and is looked at only where one of them is given:
 * cap < n is NBODY_ERR_CAPACITY with nothing written, as for nbody_get_groups.  info: n, the bodies inside and outside
 * (inside + outside == n), the occupied cells, the largest count and the lowest cell that has it (0 and cell 0 where no body
 * is inside).
 * What follows from the definition: the result is a function of the state and the grid only - not of rank, world,
 * transport, force kernel, the flags (for mass, count, first and the lists) or the order the device's waves ran in; a 1 x 1
 * grid that holds every body has in `mass` the bits of nbody_get_shells' one bin [0, +inf) at a far probe point; it is
 * independent of the semantics: a literal context's frozen tail is binned like any other body; a NaN mass makes its cell's
 * mass NaN and still counts.
 * nbody_get_cells synchronises, reads the replica (and with NBODY_CELLS_MOMENTS the velocities) and never changes what later
 * steps compute.  Without NBODY_CELLS_MOMENTS it is NOT collective: any rank of any world may call it on its own and each
 * gives the same bits.  With it the velocities are read, which a rank holds for its own range only: NBODY_ERR_STATE on a
 * context with world > 1, NBODY_FLAG_GROUP_EXCHANGE or NBODY_FLAG_FORCE_COMM, as for nbody_get_shell_moments.  The device
 * scratch and the pinned staging are allocated on the first call and grown with the grid; a context that never calls it
 * allocates nothing, launches nothing more, and the kernels it runs keep their code.  An empty system: every cell
 * {+0.0, +0.0, +0.0, +0.0, 0, -1}, start all 0.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: a NULL grid; nx or ny below 1 or nx * ny
 * above NBODY_CELLS_MAX; x0 or y0 not finite; sx or sy not finite or not above 0; unknown flag bits; order without start;
 * cap < 0 with a list; a NULL handle, cells or info.  NBODY_ERR_CAPACITY, found there too: a batch with systems * nx * ny
 * above 1 << 22.  NBODY_ERR_STATE: before an upload; moments on more than one rank.
 * How (csrc/nbody_cells.hpp): five kernels on the handle's stream and one wait - the cell of every body and the counts by
 * integer atomics (their sum does not depend on arrival), a prefix sum, the scatter through per-cell cursors, a counting
 * sort inside every cell that makes the list independent of the order of arrival, and the four ordered chains per cell over
 * the sorted list, a whole wave to a cell of 64 members or more.  No float atomic takes part.  Cost: DESIGN.md 4.20 has the
 * counts and what was measured (profiles/cells_probe.txt).
 * nbody_batch_get_cells: the same query for every system of a batch, each stage ONE launch whatever S is, with the one grid
 * for all of them.  System s's cells at [s * nx*ny + c], its start at [s * (nx*ny + 1) + c], its cell_of and order at
 * [s * capacity + .], n and `inside` entries of them, the rest of the slice left unchanged; info[s].  The lists' room is the
 * batch's capacity.  System s gives exactly the bits an nbody_ctx holding that system's state gives.  A count outside
 * [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_get_knn.
 * ------------------------------------------------------------------------------------------------- */
#define NBODY_CELLS_MAX (1 << 20)            /* nx * ny of one call */
#define NBODY_CELLS_MOMENTS 1u               /* read the velocities: px, py, k2 */
typedef struct nbody_grid { double x0, y0, sx, sy; int32_t nx, ny; } nbody_grid;            /* 40 bytes */
typedef struct nbody_cell { double mass, px, py, k2; int32_t count, first; } nbody_cell;    /* 40 bytes */
typedef struct nbody_cells_info { int32_t n, inside, outside, occupied, largest, largest_cell; } nbody_cells_info;
int nbody_get_cells(nbody_ctx* ctx, const nbody_grid* grid, uint32_t flags, nbody_cell* cells /* [nx*ny] */,
                    int32_t* cell_of /* [cap] or NULL */, int32_t* start /* [nx*ny+1] or NULL */,
                    int32_t* order /* [cap] or NULL */, int cap, nbody_cells_info* info);
int nbody_batch_get_cells(struct nbody_batch* b, const nbody_grid* grid, uint32_t flags,
                          nbody_cell* cells /* [systems*nx*ny] */, int32_t* cell_of /* [systems*capacity] or NULL */,
                          int32_t* start /* [systems*(nx*ny+1)] or NULL */, int32_t* order /* [systems*capacity] or NULL */,
                          nbody_cells_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Radius queries on the cell list (the reference has none): for every current body, or for every one of m
 * probe points, the number of bodies within a distance h, the nearest of them, how many of them overlap the row and, on
 * request, the neighbour list in CSR form - what a contact model, an SPH-style density, a local crowding measure or a
 * per-step collision monitor is built from.  The first near-field query that walks the cell list of nbody_get_cells instead
 * of all n sources per row: O(n) on a grid whose cells are about h wide.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  The grid
 * is an nbody_grid as for nbody_get_cells; inside(j) and cell(j) are exactly the cell sums' definitions.
 *   Sources: the current bodies with inside(j).  A body outside the grid is no source and is counted in info.outside.
 *   Rows (points == NULL): every current body, inside the grid or not, with its own radius r and its own term left out by
 *   index.  Rows (points != NULL): the m points with r = +0.  For a row at (x, y), (X_j, Y_j, R_j) widened exactly:
 *     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)               the d2 of nbody_get_neighbors, same bits
 *     near(j)  <=>  inside(j) && j != i && d2_j <= h2
 *     count    = the number of near j
 *     nearest  : d2 = +inf, index = -1; over the near j in ANY order:
 *                if (d2_j < d2 || (d2_j == d2 && j < index)) { d2 = d2_j; index = j; }
 *     overlaps = the number of near j with d2_j <= s*s,  s = r + R_j
 *     cell     = the row's own cell under the grid, -1 outside
 * A d2 of +inf never becomes the nearest (it is counted where h2 is +inf); a NaN d2 is never near.
 * The optional lists: start[rows + 1] (int64) is the exclusive prefix sum of count in row order, start[rows] = info.total;
 * list[start[k] .. start[k+1]) holds the near sources of row k in ASCENDING j.  list needs start; cap is the room of list
 * in entries, at most 2^31 - 1.  info.total > cap with a list is NBODY_ERR_CAPACITY: list is untouched, out, start and info
 * are complete, and the caller repeats with that cap (the rule of nbody_get_binaries).  Without list, cap is only checked
 * for its sign.
 * h2 is the squared radius: >= 0 and not NaN, +inf allowed.  With points == NULL, m is the room of out in rows (and of start
 * in rows + 1): m < n is NBODY_ERR_CAPACITY with nothing written, as for nbody_get_neighbors.
 * info: total = the sum of count (the length of the list); n; rows; inside and outside (inside + outside == n); largest =
 * the greatest count and largest_row = the lowest row that has it (0 and row 0 where there is no row).
 * What follows from the definition:
 *   - every output is an integer, a minimum under a total order or a sorted list, so none depends on the order in which the
 *     sources are visited: apart from `cell`, the result is a function of the state, the set of inside bodies and h2 only.
 *     Two grids that both hold every body give the same bytes in d2, index, count, overlaps, start and list;
 *   - with outside == 0 and h2 = +inf, {d2, index, overlaps} has the bits of nbody_get_neighbors for the same rows;
 *   - with outside == 0, finite h2 and own rows, the sum of count equals 2 * counts[0] of nbody_get_pair_counts with
 *     edges2 = {0, nextafter(h2, +inf)};
 *   - with outside == 0, count summed over points equals the point-body count of nbody_get_pair_counts with those edges;
 *   - it is not a function of rank, world, transport, force kernel or the order the device's waves ran in.
 * The window rule, by which the walk over cells finds exactly the near sources (csrc/nbody_within.hpp; DESIGN.md 4.21 has
 * the proof): a row looks at the columns (int)max(tx - wx, 0) .. (int)min(tx + wx, nx - 1) with tx = (x - x0) * sx,
 * wx = wx0 + (2^-20 + (|tx| + wx0) * 2^-40), wx0 = fl(fl(sqrt(h2)) * sx), and at the rows of cells by the same rule; a
 * window is skipped only where a compare proves it empty, and a tx that is not finite, a NaN in this arithmetic or a grid
 * of more than 2^400 cells per unit length means the whole grid.  The rule costs time, never a result: with a grid much
 * finer than h, or all bodies in a few cells, the call approaches the n^2 pair tests of nbody_get_neighbors, read from
 * memory instead of LDS.  Use a grid matched to h (Python: within_grid).
 * nbody_get_within synchronises (twice with a list), reads positions and radii of the replica only and never changes what
 * later steps compute.  It is NOT collective: any rank of any world may call it on its own and each gives the same bits.
 * Device scratch and pinned staging are allocated on the first call; a handle that never calls it allocates nothing and
 * launches nothing more, and the kernels it runs keep their code.  An empty system: every point's row {+inf, -1, 0, 0, cell}.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: everything nbody_get_cells rejects about
 * the grid; a NaN or negative h2; list without start; cap < 0; m < 0 or m x 24 bytes (x systems) above 2^31; a NULL handle,
 * out or info.  NBODY_ERR_CAPACITY: above, and a batch with systems * nx * ny above 1 << 22.  NBODY_ERR_STATE: before an
 * upload.  Not built: ordered fp64 sums over the neighbourhood (mass within h), see DESIGN.md 9.
 * nbody_batch_get_within: the same query for every system of a batch, each stage ONE launch whatever S is, with one grid,
 * one h2, one set of points and one cap for all of them.  System s's rows at out[s * per + k] and its starts at
 * start[s * (per + 1) + k] with per = the batch's capacity for own rows and m for points, its list at list[s * cap + .],
 * info[s]; the rest of every slice is left unchanged.  System s gives exactly the bits an nbody_ctx holding that system's
 * state gives.  A count outside [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_get_cells.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_within { double d2; int32_t index, count, overlaps, cell; } nbody_within;                  /* 24 bytes */
typedef struct nbody_within_info { int64_t total; int32_t n, rows, inside, outside, largest, largest_row; } nbody_within_info;
int nbody_get_within(nbody_ctx* ctx, const nbody_grid* grid, double h2, const nbody_vec2* points /* NULL: the bodies */, int m,
                     nbody_within* out, int64_t* start /* [rows+1] or NULL */, int32_t* list /* [cap] or NULL */, int cap,
                     nbody_within_info* info);
int nbody_batch_get_within(struct nbody_batch* b, const nbody_grid* grid, double h2, const nbody_vec2* points, int m,
                           nbody_within* out /* [systems*per] */, int64_t* start /* [systems*(per+1)] or NULL */,
                           int32_t* list /* [systems*cap] or NULL */, int cap, nbody_within_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Groups on the cell list (the reference has none): the friends-of-friends labels of nbody_get_groups,
 * found through the cell list of nbody_get_cells instead of a walk over all pairs: O(n) per sweep on a grid whose cells are
 * about as wide as the reach of a TYPICAL body, where nbody_get_groups is O(n^2) per sweep.
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  The grid
 * is an nbody_grid as for nbody_get_cells; inside(j) is exactly the cell sums' definition.  For two bodies i != j
 *     linked_grid(i, j)  <=>  inside(i) && inside(j) && linked(i, j)
 * with linked(i, j) the predicate of nbody_get_groups, bit for bit: dx = X_j - X_i; dy = Y_j - Y_i; d2 = (dx*dx) + (dy*dy);
 * s = (radius_scale * (R_i + R_j)) + link; d2 <= s*s.  link >= 0, +inf allowed; radius_scale finite and >= 0.  A group is a
 * connected component of the graph of these links and label[i] is the LOWEST INDEX in body i's group.  A body outside the
 * grid is linked to nobody: it is a group of its own, label[i] = i, and is counted in info.outside.
 * info: n_bodies = n; n_groups and largest over ALL n bodies, the outside ones included; sweeps = the walks over the cells
 * the call made, informational (for a batch the one number of the whole call); inside + outside == n.
 * What follows from the definition:
 *   - with outside == 0 the labels, n_groups and largest are exactly nbody_get_groups' for the same link and radius_scale;
 *   - the result is a function of the state, the two parameters and the SET of inside bodies only - an integer function of
 *     the set of links, so neither the order in which the cells are visited nor the cells themselves show: two grids that
 *     both hold every body give the same bytes in label, n_groups and largest;
 *   - with (link, radius_scale) = (0, 1) and outside == 0, body i is alone in its group - label[i] == i and no other body
 *     carries i as its label - exactly where nbody_get_within's `overlaps` (h2 = +inf) is 0 for row i;
 *   - label[label[i]] == label[i] and label[i] <= i; a NaN coordinate is outside every grid; a NaN radius links nothing;
 *   - it is not a function of rank, world, transport, force kernel or the order the device's waves ran in.
 * The window rule, by which the walk over cells sees every link (csrc/nbody_groups_grid.hpp; DESIGN.md 4.22 has the proof):
 * a link has to be seen from ONE of its two ends, and the end with the larger |radius| finds it.  Row i looks, with
 * a = |R_i|, S_i = (radius_scale * (a + a)) + link and h2_i = S_i * S_i, at the cells of nbody_get_within's window rule with
 * h = S_i - per row, not per call - and tests the exact predicate on every source there with d2 <= h2_i.  A source of no
 * larger |radius| that is linked to i has d2 <= h2_i; of two linked bodies one has no larger |radius| than the other.  One
 * large body widens its own window only.  The rule costs time, never a result: a grid much finer than the typical reach, a
 * link that percolates, or every body in a few cells brings the call towards the n^2 pair tests of nbody_get_groups, read
 * from memory instead of LDS and with one lane walking each long window.  Use a grid matched to the reach of a typical
 * body, not of the largest (Python: groups_grid).
 * nbody_get_groups_grid follows nbody_get_groups in every other respect: it synchronises (once per sweep), reads positions
 * and radii of the replica only and never changes what later steps compute; it is NOT collective - any rank of any world
 * may call it on its own and each gives the same labels; cap is the room in label, cap < n is NBODY_ERR_CAPACITY with
 * nothing written; n == 0 launches nothing and gives {0, 0, 0, 0, 0, 0}.  It allocates nothing of its own: the cell list of
 * nbody_get_cells, the sorted records of nbody_get_within and the parents and labels of nbody_get_groups, each on the first
 * call of whichever query needs it; a handle that never calls it allocates nothing and launches nothing more, and the
 * kernels it runs keep their code.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: everything nbody_get_cells rejects about
 * the grid; a NaN or negative link; a NaN, negative or infinite radius_scale; a NULL handle, label or info; cap < 0.
 * NBODY_ERR_CAPACITY: above, and a batch with systems * nx * ny above 1 << 22.  NBODY_ERR_STATE: before an upload.
 * How: the list stages of the cell sums, the gather of the radius queries, then hook and repeat as nbody_get_groups - one
 * lane per inside body in cell order walks its window and, on a linked pair with different roots, lowers the larger root's
 * parent to the smaller with one atomicMin; repeated until a walk changes nothing (at most n + 1 walks; 4 bytes per system
 * come back after each), then label[i] = root of i.  No device-side waiting, no retry loop.
 * Cost (one MI355X, fp32; profiles/groups_grid_probe.txt; nbody_get_groups timed in the same runs): the stock state of
 * N = 262144, n = 130965 bodies after 3 steps, radii median 124.5, largest 363.3, on the grid of groups_grid with the median
 * radius.  A whole call with (link, radius_scale) = (0, 1) 0.67 ms (804 x 804 cells, 3 sweeps of 0.011 ms, 0.39 ms of list
 * stages - the one-workgroup scan over the cells) against 14.6 ms; with the many-small-groups link 381.8 0.49 ms (3 sweeps of
 * 0.017 ms) against 14.7 - 22.0 ms; with the percolating link 824.8 1.18 ms (the first sweep 0.86 ms: two finds and an atomic
 * per linked pair, seen from both ends; the confirming one 0.08 ms) against 16.9 ms.  Where it LOSES: on 1 x 1 cells every row
 * walks all n records from L2, 11.7 - 13.3 ms a sweep and 26 - 27 ms a call, 1.2 - 1.8 times nbody_get_groups; and a batch of
 * 256 x 1024, whose kernels win (sweeps 0.014 against 0.234 ms) but whose whole call is 1.23 - 1.30 ms against 0.99 - 1.23 ms:
 * at 1024 bodies per system the triangular sweep is 0.12 ms and the call is bound by its fixed work.  A grid matched to the
 * LARGEST radius (2.9 times the median here) was not slower on this state: 0.36 ms with (0, 1), its scan has 8.5 times fewer
 * cells.  The widest window was 49 cells (mean 10.2); the share of a sweep spent by its slowest workgroup is not measured.
 * nbody_batch_get_groups_grid: the same for every system of a batch, with one grid, one link and one radius_scale for all
 * of them, every stage and every sweep ONE launch whatever S is; the batch sweeps until no system changed, systems that have
 * converged leave at once.  System s's labels go to label + s * capacity, one per current body, the rest of the slice is
 * left unchanged; info: one record per system.  System s gives exactly what an nbody_ctx holding that system's state gives;
 * an empty system gives {0, 0, 0, sweeps, 0, 0}.  A count outside [0, capacity] is treated as 0 and reported for that
 * system, as by nbody_batch_get_cells.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_groups_grid_info { int32_t n_bodies, n_groups, largest, sweeps, inside, outside; } nbody_groups_grid_info;   /* 24 bytes */
int nbody_get_groups_grid(nbody_ctx* ctx, const nbody_grid* grid, double link, double radius_scale, int32_t* label, int cap,
                          nbody_groups_grid_info* info);
int nbody_batch_get_groups_grid(struct nbody_batch* b, const nbody_grid* grid, double link, double radius_scale,
                                int32_t* label /* [systems*capacity] */, nbody_groups_grid_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * k nearest neighbours on the cell list (the reference has none): nbody_get_knn's result for every current
 * body, or for every one of m probe points, found through the cell list of nbody_get_cells instead of a walk over all n
 * sources per row, with an optional cut: the k nearest within a radius.  O(n) on a grid whose cells hold about k bodies
 * (Python: knn_grid), where nbody_get_knn is O(n^2).
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  The grid
 * is an nbody_grid as for nbody_get_cells; inside(j) is exactly the cell sums' definition.
 *   Sources: the current bodies with inside(j).  A body outside the grid is no source and is counted in info.outside.
 *   Rows (points == NULL): every current body, inside the grid or not, with its own term left out by index.  Rows
 *   (points != NULL): the m points.  For a row at (x, y), own index i, and (X_j, Y_j) widened exactly:
 *     dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)               the d2 of nbody_get_neighbors and nbody_get_knn
 *     eligible(j)  <=>  inside(j) && j != i && d2_j < +inf && d2_j <= h2_max
 *   Result: the first k eligible sources under the total order (d2, j) ascending, then {+inf, -1} up to k; entry c of a row
 *   is d2[row * k + c], index[row * k + c], rows by body index or in the order given, as nbody_get_knn.
 * k: 1 .. NBODY_KNN_MAX.  h2_max: the squared cut, >= 0, +inf for none.  h0: the radius of the first round below, finite and
 * >= 2^-500 (below that h0*h0 can round up among the subnormals, which the guarantee below does not survive).  With
 * points == NULL, m is the room of d2 and index in rows: m < n is NBODY_ERR_CAPACITY with nothing written.
 * What follows from the definition:
 *   - with outside == 0 and h2_max = +inf the bytes of d2 and index are nbody_get_knn's, whatever the grid and h0;
 *   - entry 0 has the bits of nbody_get_within's {d2, index} for h2 = h2_max;
 *   - the number of non-empty entries of a row is min(k, count) of nbody_get_within for h2 = h2_max, except that a source
 *     at d2 = +inf is counted there (h2 = +inf) and never listed here;
 *   - the non-empty indices are the first k of that row's list of nbody_get_within, re-sorted by (d2, j);
 *   - the result is a function of the state, the SET of inside bodies, k and h2_max only: two grids that both hold every
 *     body, and any two h0, give the same bytes in d2 and index;
 *   - it is not a function of rank, world, transport, force kernel or the order the device's waves ran in.
 * The widening rule, by which the walk over cells finds exactly these entries; it is part of the contract, since info
 * reports it (csrc/nbody_knn_grid.hpp; DESIGN.md 4.23 has the proof).  Round t = 0, 1, ... of a row:
 *   - h_t = h0 * 2^t and H2_t = fl(h0*h0) * 4^t, both scalings exact, an overflow to +inf allowed; from t = 48 both are +inf;
 *   - where H2_t >= h2_max the round takes h = fl(sqrt(h2_max)), computed once on the host, and H2 = h2_max, and is final;
 *   - the window is cells_span(tx, fl(h*sx), nx) x cells_span(ty, fl(h*sy), ny), the span of nbody_get_within's window rule,
 *     per axis never narrower than in the round before; a grid of more than 2^400 cells per unit length looks at every
 *     cell in round 0; a round whose spans are both the whole axis is final;
 *   - after a round the row is done if the round was final, or if its list holds k entries and the k-th d2 <= H2_t.
 * A round after the first looks only at the cells its spans add, so no source is looked at twice.  Every inside source with
 * d2 <= H2_t lies in the window of round t (the window rule's proof, with room to spare for sqrt(H2_t) <= h_t (1 + 2^-52)),
 * so an unseen source has d2 > H2_t >= d2_k, strictly: it can neither enter the list nor tie with its last entry.
 * info: n; rows; inside and outside (inside + outside == n); rounds = the greatest number of rounds a row took (0 where
 * there is no row); widened = the number of rows that took more than one.  Both are functions of the state, the grid, k,
 * h0 and h2_max; they tell a caller whether the grid and h0 match k: on a matched grid widened is a small part of rows.
 * The rule costs time, never a result: with every body in a few cells, or a grid much finer than the distance to the k-th
 * neighbour, the call approaches the n^2 pair tests of nbody_get_knn, read from memory instead of LDS by one lane per row.
 * nbody_get_knn_grid synchronises once, reads positions of the replica only and never changes what later steps compute.  It
 * is NOT collective: any rank of any world may call it on its own and each gives the same bits.  Device scratch and pinned
 * staging are allocated on the first call; a handle that never calls it allocates nothing and launches nothing more, and
 * the kernels it runs keep their code.  An empty system: every point's entries {+inf, -1}.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: everything nbody_get_cells rejects about
 * the grid; k outside [1, NBODY_KNN_MAX]; a NaN or negative h2_max; an h0 that is NaN, infinite or below 2^-500; m < 0 or
 * m x k x 12 bytes (x systems) above 2^31; a NULL handle, d2, index or info.  NBODY_ERR_CAPACITY: above, and a batch with
 * systems * nx * ny above 1 << 22.  NBODY_ERR_STATE: before an upload.
 * Cost (one MI355X, fp32, points == NULL, the stock seeded state of N = 262144; profiles/knn_grid_probe.txt, nbody_get_knn
 * timed in the same runs): k = 8 on the 181 x 181 cells of knn_grid the six kernels 0.164 ms (the walk 0.100) against
 * knn_at's 20.19 ms, 46 of the rows widened; k = 32 on 90 x 90 cells 1.525 ms (the walk 1.473) against 39.96 ms, 9 rows
 * widened.  Whole Stepper.knn() calls, which also copy n x k x 12 bytes and split them into two arrays: 6.1 against 25.9 ms
 * (4.2 times faster) and 28.3 against 67.9 ms (2.4 times) - the copy and the split are now nearly all of the call.  Where
 * it LOSES: every body in one cell of 8 x 8, k = 8, the walk 43.7 ms and the call 54.8 against 25.8 ms; and a batch of
 * 256 x 1024 on 32 x 32 cells - one body per cell, 258379 of 262144 rows widen - whose walk is 0.206 ms against 0.378 ms
 * but whose whole call is 4.25 against 3.71 ms.  Not measured: fp64, explicit points, other states.
 * nbody_batch_get_knn_grid: the same query for every system of a batch, the list stages and the walk ONE launch each
 * whatever S is, with one grid, one set of points, one k, one h0 and one h2_max for all of them.  System s's entries at
 * [(s * per + row) * k + c] with per = the batch's capacity for own rows and m for points, info[s]; the rest of every slice
 * is left unchanged.  System s gives exactly the bits an nbody_ctx holding that system's state gives.  A count outside
 * [0, capacity] is treated as 0 and reported for that system, as by nbody_batch_get_cells.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_knn_grid_info { int32_t n, rows, inside, outside, widened, rounds; } nbody_knn_grid_info;  /* 24 bytes */
int nbody_get_knn_grid(nbody_ctx* ctx, const nbody_grid* grid, const nbody_vec2* points /* NULL: the bodies */, int m, int k,
                       double h0, double h2_max, double* d2, int32_t* index /* [rows*k] each */, nbody_knn_grid_info* info);
int nbody_batch_get_knn_grid(struct nbody_batch* b, const nbody_grid* grid, const nbody_vec2* points, int m, int k, double h0,
                             double h2_max, double* d2, int32_t* index /* [systems*per*k] each */,
                             nbody_knn_grid_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Pair counts and bound pairs on the cell list (the reference has none): the histogram of
 * nbody_get_pair_counts and the list of nbody_get_binaries among the bodies inside a caller-given grid, found through the cell
 * list of nbody_get_cells instead of a walk over all n sources per row: O(n) on a grid whose cells are about as wide as the
 * top edge, or the separation (Python: within_grid(field, top_edge_or_max_sep)), where the plain calls are O(n^2).
 * The definition, which is the whole contract.  Only IEEE fp64 operations, every one rounded on its own, no fma.  The grid
 * is an nbody_grid as for nbody_get_cells; inside(j) is exactly the cell sums' definition.  The sources are the current
 * bodies with inside(j); a body outside the grid takes part in no pair and is counted in info.outside; inside + outside == n.
 * nbody_get_pair_counts_grid.  d2, counts[k], below and the derived rest are those of nbody_get_pair_counts, bit for bit -
 *     dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy);  counts[k]: edges2[k] <= d2 && d2 < edges2[k+1];  below: d2 < edges2[0]
 * - over the counted pairs.  points == NULL, the own form: the unordered pairs of inside bodies, each once;
 * info.pairs = inside * (inside - 1) / 2 and info.rows = n.  points != NULL: every (point, inside body) pair;
 * info.pairs = m * inside and info.rows = m; a point may lie anywhere - outside the grid, at 1e200, at NaN (it counts nothing).
 * rest = pairs - below - sum(counts), derived on the host.  edges2 and bins follow nbody_get_pair_counts' rules; a top edge
 * of +inf is legal and means the whole grid: correct, and slow.
 * nbody_get_binaries_grid.  The definition of nbody_get_binaries, bit for bit, over the pairs i < j of inside bodies; the
 * indices of a record are those of the state.  coincident counts the pairs of inside bodies at d2 == 0 (two such bodies share
 * a cell).  The host half (nbody_binary_finish, the sort by (i, j)), the cap rule - NBODY_ERR_CAPACITY leaves out untouched
 * with info complete, cap == 0 gives the counts only - and the single-rank restriction are nbody_get_binaries'.
 * What follows from the definition:
 *   - with outside == 0: counts, below, rest and pairs are the bytes of nbody_get_pair_counts, and the list and every count
 *     the bytes of nbody_get_binaries, whatever the grid;
 *   - with any grid they are what the plain calls give on a context that holds exactly the inside bodies, in their order,
 *     the binaries' indices mapped back;
 *   - with outside == 0 and own rows, 2 * counts[0] at edges2 = {0, nextafter(h2, +inf)} equals the sum of `count` of
 *     nbody_get_within at h2 on the same grid;
 *   - near + coincident of the binaries == counts[0] of the pair counts on the same grid at {0, nextafter(sep2, +inf)};
 *   - the results are functions of the state, the values and the SET of inside bodies only: neither the cells nor the order
 *     of the visit show, nor rank, world, transport, force kernel or the order the device's waves ran in.
 * The window (csrc/nbody_pairs_grid.hpp): nbody_get_within's fixed-radius rule with h2 = edges2[bins], or sep2 - the same
 * host values, the same escape for a grid of more than 2^400 cells per unit length, the same span per axis.  It covers
 * d2 <= h2; the pair counts count d2 < edges2[bins], so a pair exactly at the top edge is visited and not counted, the
 * binaries take d2 <= sep2.  The rule costs time, never a result: a grid much finer than h, an h of the order of the
 * system, or every body in a few cells brings the calls towards the n^2 pair tests of the plain ones, read from memory
 * instead of LDS by one lane per row.
 * Both synchronise, read only and never change what later steps compute.  nbody_get_pair_counts_grid reads positions of the
 * replica only and is NOT collective: any rank of any world may call it on its own and each gives the same bytes.
 * nbody_get_binaries_grid reads the velocities: NBODY_ERR_STATE on a context of more than one rank or with an exchange.
 * They allocate nothing of their own - the cell list of nbody_get_cells, the sorted records of nbody_get_within, the edges,
 * histograms and points of nbody_get_pair_counts, the log and counters of nbody_get_binaries, each on the first call of
 * whichever query needs it; a handle that never calls them allocates nothing and launches nothing more, and every other
 * kernel keeps its code.  n == 0 launches nothing.
 * NBODY_ERR_INVALID, found before any device call, the values before the handle: everything nbody_get_cells rejects about
 * the grid; then what nbody_get_pair_counts rejects (bins outside [1, 256]; a NaN, negative or unordered edge; m < 0 or m
 * points above 2^31 bytes; a NULL handle, edges2, counts or info) or what nbody_get_binaries rejects (a NaN or negative sep2;
 * cap < 0; a NULL out with cap > 0; cap records x systems above 2^31 bytes; a NULL handle or info).  NBODY_ERR_CAPACITY: the
 * cap rule, and a batch with systems * nx * ny above 1 << 22.  NBODY_ERR_STATE: before an upload, and above.
 * Cost (one MI355X, fp32; profiles/pairs_grid_probe.txt, the plain calls timed in the same runs; the stock state of N = 262144,
 * n = 130965 after 3 steps, on within_grid(field, top edge or sep)): pair counts with 32 bins up to 381.8 / 824.8, the kernels of
 * a call 0.197 / 0.088 ms (the walk 0.014 / 0.022) against pair_counts' 5.37 / 5.57 ms, whole calls 0.26 / 0.15 against 5.40 / 5.66 ms.
 * Binaries, the counts only, at sep 128 / 1024: kernels 0.634 / 0.173 ms (the walk 0.019 / 0.122; at sep 128 the grid is
 * 1024 x 1024 cells and their one-workgroup scan is 0.6 ms) against 5.38 / 5.79 ms, calls 0.68 / 0.22 against 5.51 / 5.71 ms.  With
 * the list at sep 1024 (652339 records) the kernels are 1.01 against 9.25 ms and the call about 100 ms either way, inside the spread
 * of its three rounds: the copy and the sort are the call.  Where it LOSES: on 1 x 1 cells every row walks all n records from
 * memory - 15.0 against 5.2 ms (pair counts), 13.9 against 5.3 ms (binaries); and a batch of 256 x 1024, whose kernels win
 * (0.056 - 0.072 against 0.120 - 0.159 ms) but whose whole call loses for the binaries with the list (13.5 against 10.8 ms), is level
 * for the pair counts (0.49 against 0.49 ms) and wins for the counts-only binaries (0.111 against 0.156 ms).
 * nbody_batch_get_pair_counts_grid, nbody_batch_get_binaries_grid: the same for every system of a batch, with one grid, one
 * set of points and edges or one sep2 and one cap for all of them, every stage ONE launch whatever S is.  System s's counts
 * at counts + s * bins, its list at out + s * cap, info[s]; the tail of every slice is left unchanged.  System s gives
 * exactly what an nbody_ctx holding that system's state gives.  A count outside [0, capacity] is treated as 0 and reported
 * for that system, as by nbody_batch_get_cells.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_pair_grid_info { int64_t n_bodies, rows, pairs, below, rest, inside, outside; } nbody_pair_grid_info;   /* 56 bytes */
typedef struct nbody_binary_grid_info {
    int64_t n_bodies, pairs, near, coincident, overlapping, approaching; double sep2; int64_t inside, outside;
} nbody_binary_grid_info;   /* 72 bytes */
int nbody_get_pair_counts_grid(nbody_ctx* ctx, const nbody_grid* grid, const nbody_vec2* points /* NULL: the bodies */, int m,
                               const double* edges2 /* [bins + 1] */, int bins, uint64_t* counts /* [bins] */,
                               nbody_pair_grid_info* info);
int nbody_batch_get_pair_counts_grid(struct nbody_batch* b, const nbody_grid* grid, const nbody_vec2* points, int m,
                                     const double* edges2, int bins, uint64_t* counts /* [systems * bins] */,
                                     nbody_pair_grid_info* info /* [systems] */);
int nbody_get_binaries_grid(nbody_ctx* ctx, const nbody_grid* grid, double sep2, nbody_binary* out, int cap,
                            nbody_binary_grid_info* info);
int nbody_batch_get_binaries_grid(struct nbody_batch* b, const nbody_grid* grid, double sep2, nbody_binary* out /* [systems * cap] */,
                                  int cap, nbody_binary_grid_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Encounters on the cell list (the reference has none): the swept contacts of nbody_get_encounters among the
 * bodies inside a caller-given grid, found through the cell list of nbody_get_cells instead of a walk over all n sources per
 * row: O(n) on a grid whose cells are about as wide as the reach of a typical body within the horizon (Python:
 * encounters_grid(field, horizon, r_typical, v_typical)), where the plain call is O(n^2).  The natural use is a per-step
 * monitor with h = the time step.
 * The definition, which is the whole contract.  The result is exactly what nbody_get_encounters defines - swept, flags, t,
 * the sort by (t, i, j), the counts - over the pairs i < j of bodies that are both inside(.) of the cell sums; the indices of
 * a record are those of the state.  inside and outside are as in nbody_binary_grid_info: a body outside the grid takes part
 * in no pair; inside + outside == n.  What follows:
 *   - with outside == 0 the list and every count are the bytes of nbody_get_encounters, whatever the grid;
 *   - with any grid they are what nbody_get_encounters gives on a context that holds exactly the inside bodies, in their
 *     order, the indices mapped back;
 *   - the raw record does not depend on which end of a pair evaluates it.  nbody_get_encounters evaluates a pair at the
 *     higher index; here the reporting row may be the lower.  c, b and disc are built from d2, s and products of two
 *     differences; ex and ey change sign as a whole; R_i + R_j commutes: {lower, higher, flags, c, b, disc} has the same bits
 *     either way;
 *   - the result is a function of the state, h and the SET of inside bodies only: neither the cells nor the order of the
 *     visit show.
 * Carried over unchanged from nbody_get_encounters: the cap rule (pairs > cap: NBODY_ERR_CAPACITY, out untouched, info
 * complete; NULL out with cap == 0: the counts only), the host half (nbody_encounter_finish), the single-rank restriction
 * (NBODY_ERR_STATE on world > 1, NBODY_FLAG_GROUP_EXCHANGE or NBODY_FLAG_FORCE_COMM, and before an upload), "synchronises,
 * reads only, never changes what later steps compute".  NBODY_ERR_INVALID, found before any device call, the values before
 * the handle: everything nbody_get_cells rejects about the grid, then what nbody_get_encounters rejects (a NaN or negative
 * horizon; cap < 0; a NULL out with cap > 0; cap records x systems above 2^31 bytes; a NULL handle or info).
 * NBODY_ERR_CAPACITY also for a batch with systems * nx * ny above 1 << 22.
 * The window (csrc/nbody_encounters_grid.hpp; DESIGN.md 4.25 has the proof).  All fp64, each operation rounded on its own, no
 * fma, on the exactly widened record, with h the horizon:
 *     rho_i = |R_i| + (h * (|VX_i| + |VY_i|))          the reach: radius plus the L1 norm of the displacement within h
 *     rho_i = +inf where that is NaN (a NaN velocity or radius, 0 * inf)
 *     rho_i = +inf where the context is fp64 and any of X, Y, VX, VY, R of body i is not finite, or non-zero with a
 *             magnitude outside [2^-100, 2^200]
 *     H_i = (rho_i + rho_i) * (1 + 2^-40);   H2_i = H_i * H_i
 * Row i owns the pair (i, j) iff rho_i > rho_j, or rho_i == rho_j and i > j - a total order, so every pair has exactly one
 * owner, and both ends compute rho by the same expression from the same record.  A pair that is swept as the definition
 * computes it has d2 <= H2 of its owner, so the other end's cell lies in the owner's window of nbody_get_within's span per
 * axis with h = H_i (per row, as nbody_get_groups_grid passes its S_i; the same escape for a grid of more than 2^400 cells per
 * unit length).  H_i = +inf (h = +inf; a NaN velocity; the fp64 guard) means every cell for that row: correct, and slow.  The
 * rule costs time, never a result.  It uses |v|, not the speed relative to the neighbours: a common bulk velocity widens
 * every window.
 * It allocates nothing of its own - the cell list of nbody_get_cells, the sorted records of nbody_get_within, the log and
 * counters of nbody_get_encounters, each on the first call of whichever query needs it; a handle that never calls it
 * allocates nothing and launches nothing more, and every other kernel keeps its code.  n == 0 launches nothing.
 * Cost (one MI355X, fp32; profiles/encounters_grid_probe.txt, nbody_get_encounters timed in the same runs; the stock state of
 * N = 262144, n = 130965 after 3 steps, on encounters_grid(field, h, median radius 124.5, median |vx| + |vy| 65.8): 804 x 804,
 * 727 x 727 and 390 x 390 cells at h = 0 / 0.2 / 2.0, a median window of 9 cells, the widest 49 / 49 / 64, 2.5 / 2.9 / 9.4
 * candidates per row of which 0.10 / 0.13 / 0.31 pass the compare).  The walk 0.076 / 0.080 / 0.095 ms with the counts only and
 * 0.101 / 0.133 / 0.280 ms with the list of 5052 / 9201 / 35603 records, the kernels of a call 0.47 / 0.41 / 0.21 ms (0.39 / 0.33 /
 * 0.12 of it the list stages) against encounters_walk's 18.4 - 18.9 ms; whole calls 0.51 / 0.46 / 0.26 ms for the counts against
 * 18.8 - 19.0 ms and 0.91 / 1.28 / 3.71 ms with the list against 19.2 / 19.7 / 22.1 ms.  On 1 x 1 cells every row walks all n
 * records from memory: 14.7 against 18.4 ms - ahead of the plain call, 30 times behind the matched grid.  A batch of 256 x 1024
 * at h = 0.2 on 128 x 128 cells: kernels 0.065 against 0.309 ms, whole calls 0.119 against 0.346 ms (counts) and 0.865 against
 * 1.036 ms (the list).  Not measured: h = +inf (every cell for every row), fp64, a state with a bulk velocity.
 * nbody_batch_get_encounters_grid: the same for every system of a batch, with one grid, one horizon and one cap for all of
 * them, every stage ONE launch whatever S is.  System s's list at out + s * cap, info[s]; the tail of every slice is left
 * unchanged.  System s gives exactly what an nbody_ctx holding that system's state gives.  A count outside [0, capacity] is
 * treated as 0 and reported for that system, as by nbody_batch_get_cells.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_encounter_grid_info {
    int64_t n_bodies, pairs, now, end, missed; double horizon; int64_t inside, outside;
} nbody_encounter_grid_info;   /* 64 bytes */
int nbody_get_encounters_grid(nbody_ctx* ctx, const nbody_grid* grid, double horizon, nbody_encounter* out, int cap,
                              nbody_encounter_grid_info* info);
int nbody_batch_get_encounters_grid(struct nbody_batch* b, const nbody_grid* grid, double horizon,
                                    nbody_encounter* out /* [systems * cap] */, int cap,
                                    nbody_encounter_grid_info* info /* [systems] */);

/* ---------------------------------------------------------------------------------------------------
 * Batched stepper: S independent systems in one context, stepped together -- S copies of the loop body
 * src/nbody.cu:463-510 per call, for ensembles of SMALL systems (seeds, radii, growth rates, time steps).  One system of
 * N = 1024 is eight workgroups and a fixed per-step tail on a 256-CU part; S of them as S nbody_ctx cost S launches and
 * S host waits per ensemble step.  A batch costs two launches per ensemble step (three when a system has more than 1024
 * bodies), whatever S is, no device-to-host copy and no host wait.
 *
 * System s of a batch is, bit for bit, what an nbody_ctx with the same precision, semantics and parameters gives after
 * the same upload and the same number of steps: state, survivor count and order, pair counter, and (with
 * NBODY_FLAG_RECORD_EVENTS) the event set of every step.  Systems never see each other: each has its own count, step
 * counter, counters and event slice; the literal index quirks follow from each system's own live count.
 *
 * Where it stops paying (one MI355X, us per ensemble step, S nbody_ctx with a stream each against one batch, stock radii /
 * radii 0; profiles/batch_probe.txt): 1024 x 256 bodies 18878 / 19093 against 108 / 118; 256 x 1024 5135 / 5704 against
 * 214 / 216; 64 x 4096 1345 / 1768 against 350 / 590 (3.8x / 3.0x); 16 x 16384 831 / 2096 against 1108 / 2037 (0.75x /
 * 1.03x).  So from about 16384 bodies per system one nbody_ctx per system - the ring-of-waves kernel, which then fills the
 * chip on its own - is level or faster, and a batch (the one-lane-per-body kernel) is the tool below that.
 *
 * Argument errors (NBODY_ERR_INVALID) are found before any device call.  systems <= 65535: the system index is gridDim.y.
 * ------------------------------------------------------------------------------------------------- */
typedef struct nbody_batch nbody_batch;
typedef struct nbody_batch_params {   /* per system: the kernel arguments of src/nbody.cu:482 */
    double timestep, growthRate;
    int fieldWidth, fieldHeight;
} nbody_batch_params;
typedef struct nbody_batch_desc {
    int precision;       /* NBODY_F32 only in this version; NBODY_F64 -> NBODY_ERR_INVALID                        */
    int semantics;       /* nbody_semantics, one for the whole batch                                              */
    int systems;         /* S, 1..65535                                                                           */
    int capacity;        /* max bodies PER SYSTEM; systems * capacity <= 2^28                                     */
    int device;          /* HIP device ordinal                                                                    */
    uint32_t flags;      /* NBODY_FLAG_RECORD_EVENTS and / or NBODY_FLAG_TRACK_IDS; anything else -> NBODY_ERR_INVALID */
    int event_capacity;  /* max logged events per system (0: default, 2^24 / systems clamped to 1024..2^20)       */
    int kernel_variant;  /* 0 automatic (from systems * capacity); otherwise lanes per body, 1, 2, 4 or 8 (A/B)   */
} nbody_batch_desc;

/* params: one entry per system.  NBODY_ERR_NO_DEVICE without a gfx950 device. */
int nbody_batch_create(nbody_batch** out, const nbody_batch_desc* d, const nbody_batch_params* params);
int nbody_batch_destroy(nbody_batch* b);
/* S times BodiesData::uploadToDevice (src/nbody.cu:88-96): blocks[s] is a host block of counts[s] bodies in the
 * reference layout.  counts[s] == 0 is legal (the system stays empty; blocks[s] must still be a pointer); counts[s] < 0
 * or > capacity and a NULL blocks[s] are NBODY_ERR_INVALID.  Clears every system's event log and counters and restarts
 * the step numbers, as nbody_upload does. */
int nbody_batch_upload(nbody_batch* b, const void* const* blocks, const int* counts);
/* nsteps ensemble steps (src/nbody.cu:463-510 for every system), asynchronous: enqueue only. */
int nbody_batch_step(nbody_batch* b, int nsteps);
/* CUDA_SYNC_CHECK (src/nbody.cu:20-33,546).  A device-side failure of any system (a count that failed its index
 * check) is reported by this and every other synchronising call as NBODY_ERR_HIP, with the system's number. */
int nbody_batch_sync(nbody_batch* b);
int nbody_batch_counts(nbody_batch* b, int* counts);          /* current body count of every system; synchronises */
/* As nbody_download, for one system: the survivors' re-carved block (src/nbody.cu:486,496-510); block must hold
 * `capacity` bodies.  Synchronises. */
int nbody_batch_download(nbody_batch* b, int system, void* block, int* n);
/* As nbody_get_events, for one system's slice of the log; step numbers count from the last upload. */
int nbody_batch_get_events(nbody_batch* b, int system, nbody_event* out, int cap, int64_t* total);
/* As nbody_get_ids and nbody_get_lineage, for one system (NBODY_FLAG_TRACK_IDS in nbody_batch_desc.flags): identities are
 * the indices 0 .. counts[s]-1 of the last nbody_batch_upload, per system; system s gives what an nbody_ctx with the flag
 * gives for the same upload and steps (the lineage as a set per step, like the events).  At most two more launches per
 * ensemble step, whatever S is.  Same errors; a bad system number is NBODY_ERR_INVALID. */
int nbody_batch_get_ids(nbody_batch* b, int system, int32_t* ids, int cap, int* n);
int nbody_batch_get_lineage(nbody_batch* b, int system, nbody_lineage* out, int cap, int64_t* total);
/* steps, pairs and n_bodies of one system; every other field 0.  Synchronises. */
int nbody_batch_get_stats(nbody_batch* b, int system, nbody_stats* out);
/* Which force kernel the batch launches (static string; reporting only). */
const char* nbody_batch_kernel_name(nbody_batch* b);

/* Per-system diagnostics of a batch.  out[s] is exactly what nbody_get_diagnostics returns for an nbody_ctx holding system
 * s's state - the same bits in every field, phi included: step (steps since the batch's upload), n_bodies, coincident_pairs,
 * the centre of mass and every sum, by the order contract above (phi_i one running sum over j ascending, totals per aligned
 * 128-body tile and then over the tiles).  Two launches per call, whatever S is.  An empty system gives n_bodies = 0, every
 * sum +0, no coincident pairs and center_of_mass NaN (the rule for mass == 0).
 * out: room for `systems` records.  phi: NULL, or room for systems * capacity doubles; system s's phi goes to
 * phi + s * capacity, one value per current body, the rest of that slice is left unchanged.  Synchronises.  The device
 * buffers are allocated on the first call (the phi buffer, systems * capacity doubles, on the first call that asks for phi):
 * a batch that never asks keeps its footprint.
 * Against the route without this call (per system: nbody_batch_download, nbody_upload into one reused nbody_ctx,
 * nbody_get_diagnostics; one MI355X, ms per call, stock radii; profiles/batch_diag_probe.txt): 1024 x 256 bodies 190.4 against
 * 0.64, 256 x 1024 56.0 against 0.39, 64 x 4096 22.9 against 0.63, 16 x 16384 14.1 against 2.11 - unlike the stepping, no
 * shape of these favours one nbody_ctx per system.  A record costs 0.66 (256 x 1024) to 0.74 (64 x 4096) of an ensemble step. */
int nbody_batch_diagnostics(nbody_batch* b, nbody_diag* out, double* phi);
/* A recorded series: samples are enqueued between steps into a device-side log and read back once at the end.
 * nbody_batch_diag_reserve allocates (or re-allocates) a log of samples x systems records and empties it; samples = 0
 * frees it; samples < 0 or a log above 2^31 bytes: NBODY_ERR_INVALID, found before any device call.
 * nbody_batch_diag_record is enqueue-only, like nbody_batch_step: it launches the kernels that write the current sample of
 * every system into the next row (no phi is kept), with no device-to-host copy and no synchronisation.  A full log is
 * NBODY_ERR_CAPACITY, found on the host: nothing is enqueued and the earlier rows stay.  No reservation, or no upload yet:
 * NBODY_ERR_STATE.  nbody_batch_upload restarts the log at row 0 and keeps the reservation.
 * nbody_batch_diag_read synchronises, copies min(recorded, cap_samples) rows (out[k * systems + s]) and stores the number
 * recorded in *n_samples.  Row k is what nbody_batch_diagnostics would have returned at the moment it was recorded: step and
 * n_bodies come from each system's device-side state. */
int nbody_batch_diag_reserve(nbody_batch* b, int samples);
int nbody_batch_diag_record(nbody_batch* b);
int nbody_batch_diag_read(nbody_batch* b, nbody_diag* out, int cap_samples, int* n_samples);
/* The track log of a batch (NBODY_FLAG_TRACK_IDS in nbody_batch_desc.flags): nbody_track_reserve / _record / _read for every
 * system at once, with the one selection for all of them and `capacity` per system.  The same row contract per system - system
 * s's table is what an nbody_ctx gives for the same upload, steps and records, phi having the bits of
 * nbody_batch_diagnostics - and the same errors; one launch per record, two with NBODY_TRACK_PHI, whatever S is.  A sample is S
 * rows: rows[s * S + sys], and rec / index / phi [(s * S + sys) * columns + c].  nbody_batch_upload restarts the log at row 0
 * and keeps the reservation. */
int nbody_batch_track_reserve(nbody_batch* b, int samples, const int32_t* ids, int k, uint32_t fields);
int nbody_batch_track_record(nbody_batch* b);
int nbody_batch_track_read(nbody_batch* b, nbody_track_row* rows, void* rec, int32_t* index, double* phi,
                           int cap_samples, int* n_samples, int* columns);

/* ---------------------------------------------------------------------------------------------------
 * Reference-shaped launches on caller-owned DEVICE memory: one-to-one replacements of the two <<<>>> sites
 * src/nbody.cu:481-483.  d_bodyData is a device block in the reference layout for numBodies bodies;
 * velocities are updated in place, updatedMasses/updatedRadii are the scratch arrays of :463-464.  The
 * never-allocated `updatedVelocities` argument of the reference (:441) is dropped.  `stream` is a
 * hipStream_t (NULL = default stream).  numBlocks follows :473; pass nbody_num_blocks(numBodies): with that
 * block count the production kernel of nbody_step runs (same speed), through a process-wide workspace on the current
 * device that holds what a context keeps resident (the {x,y,m,r} replica and the staged output; grown to the largest
 * numBodies seen, released by nbody_launch_workspace_release; not re-entrant, as the reference's loop is one host
 * thread); any other count is honoured by a general kernel directly on the block (it changes which bodies are
 * active and how many tiles are walked).
 * ------------------------------------------------------------------------------------------------- */
int nbody_num_blocks(int numBodies);      /* src/nbody.cu:473 */
int nbody_launch_compute_forces_f32(void* d_bodyData, float* d_updatedMasses, float* d_updatedRadii,
                                    int numBodies, float timestep, int fieldWidth, int fieldHeight,
                                    int numBlocks, float growthRate, void* stream);
int nbody_launch_move_bodies_f32(void* d_bodyData, const float* d_updatedMasses, const float* d_updatedRadii,
                                 int numBodies, float timestep, int numBlocks, void* stream);
int nbody_launch_workspace_release(void);   /* frees the workspace of nbody_launch_compute_forces_f32 (if any) */

/* Device self-test used by the GPU test-suite, exhaustive over all 2^32 fp32 inputs: the kernels' general
 * sqrt and reciprocal against fp64-then-round, and the fast evaluation chain of the fp32 force kernel
 * (rsq/rcp + fma corrections) against the general code on its whole guarded domain.
 * mismatches = {sqrt, reciprocal, fast chain} mismatch counts; all must be 0. */
int nbody_selftest_ieee_f32(int device, uint64_t mismatches[3]);
/* The fp64 counterpart cannot be exhaustive: the fast chain of the fp64 force kernel against the compiler's IEEE
 * sqrt and 1/x on inputs_per_mode inputs of each of three families of its guarded domain [2^-500, 2^500] (random;
 * mantissas next to powers of two; perfect squares +- 4 ulps).  mismatches = {sqrt, 1/d^3}; both must be 0. */
int nbody_selftest_chain_f64(int device, uint64_t inputs_per_mode, uint64_t mismatches[2]);
/* The one known exception of Newton-type fp64 reciprocals (a significand of all ones: the last fma sees an exact tie and
 * rounds one ulp low), on c = (2 - 2^-52) 2^k for every k in [-750, 750] against the closed form 2^-(k+1) (1 + 2^-52):
 * result = {mismatches of the general code's reciprocal (must be 0), of the compiler's bare 1.0 / c (informational), of
 * the fast chain's refinement (informational: the reason the fp64 kernel screens such c and redoes them with the general
 * code), inputs the kernel's screen would miss (must be 0), inputs checked (1501)}. */
int nbody_selftest_rcp_ones_f64(int device, uint64_t result[5]);

/* The ring kernel's hand-off relies on a lane's 16-byte LDS record being written (ds_write_b128) and read
 * (ds_read_b128) in one LDS-array cycle, i.e. never seen half old, half new.  512 workgroups: one wave rewrites its 64
 * records `iters` times while seven waves poll them.  result = {torn records seen, sequence numbers going
 * backwards, records read}; the first two must be 0. */
int nbody_selftest_lds_record(int device, int iters, uint64_t result[3]);

/* Profiling aid: launches ONLY the force kernel of the context's current state `reps` times, back to back; the
 * results land in the staging buffers and are never committed, so the state does not change (the pair and event
 * counters do count).  Lets one rank's kernel of a G-rank partition be timed / profiled in steady state on one GPU. */
int nbody_debug_force_only(nbody_ctx* ctx, int reps);

/* Testing aid: the bookkeeping the fp32 ring kernel's screens rest on, for the CURRENT replica (synchronises).
 * summary = Meta::summary; tile_rmax receives min(cap, n_tiles) floats (largest |radius| per aligned 128-body
 * tile, 0 for tiles past the end); *n_tiles = entries the context keeps.  Any output pointer may be NULL. */
int nbody_debug_screen_state(nbody_ctx* ctx, int* summary, float* tile_rmax, int cap, int* n_tiles);

/* Tuning aid (kernel_variant 58 and 59 only): cycle totals of the ring kernel's phases since upload, summed over waves:
 * {evaluate, wait, chain+publish, window check, polls, turns, shader clocks of one wave's life, the same in 100 MHz
 * ticks}. */
int nbody_debug_ring_probe(nbody_ctx* ctx, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_MI355X_H */
