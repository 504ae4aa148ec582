/* csrc/nbody_cli.c -- `nbody`: command-line driver with the reference binary's behaviour on the hot path
 * (main(), src/nbody.cu:373-551): reads ./nbodyConfig.txt from the current directory (:377), echoes the
 * settings, seeds the bodies (:401-416), runs totalIterations steps and prints the elapsed time (:548).
 * Image output (:512-539) is produced with --images: iteration_<k>.ppm in cfg.imagePath for every k that is a
 * multiple of save_Image_Every_Xth_Iteration and not the last iteration (the reference saves the image of
 * iteration k during iteration k+1, :513-522, so the last one is never written).  Without --images the run is
 * the pure stepping loop.  --lineage PATH (single GPU) runs with NBODY_FLAG_RECORD_EVENTS | NBODY_FLAG_TRACK_IDS and writes
 * the merger history in identity space after the run: one line `step kind id_i id_j` per record of nbody_get_lineage,
 * sorted by (step, kind, id_i, id_j), then one line `survivors` and the identities of the final bodies, one per line in
 * index order.  --diagnostics K prints one `diag ...` line (nbody_get_diagnostics / nbody_group_diagnostics,
 * %.17g: the values round-trip) after the upload, after every K-th step and after the last one.  Host code in C over
 * the C ABI. */
#include "nbody.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

static double now(void) {   /* jbutil::gettime, include/jbutil.h:98-104 */
    struct timeval tv;
    gettimeofday(&tv, NULL);
    return (double)tv.tv_sec + (double)tv.tv_usec * 1e-6;
}

static int print_diag(nbody_ctx** ctxs, int gpus) {
    nbody_diag d;
    int rc = gpus > 1 ? nbody_group_diagnostics(ctxs, gpus, &d, NULL) : nbody_get_diagnostics(ctxs[0], &d, NULL);
    if (rc != NBODY_OK) return rc;
    printf("diag step=%lld n=%lld mass=%.17g px=%.17g py=%.17g cx=%.17g cy=%.17g L=%.17g kinetic=%.17g potential=%.17g "
           "coincident=%lld\n",
           (long long)d.step, (long long)d.n_bodies, d.mass, d.momentum[0], d.momentum[1], d.center_of_mass[0],
           d.center_of_mass[1], d.angular_momentum, d.kinetic, d.potential, (long long)d.coincident_pairs);
    return NBODY_OK;
}

static int cmp_lineage(const void* pa, const void* pb) {   /* by (step, kind, id_i, id_j) */
    const nbody_lineage *a = (const nbody_lineage*)pa, *b = (const nbody_lineage*)pb;
    if (a->step != b->step) return a->step < b->step ? -1 : 1;
    if (a->kind != b->kind) return a->kind < b->kind ? -1 : 1;
    if (a->id_i != b->id_i) return a->id_i < b->id_i ? -1 : 1;
    if (a->id_j != b->id_j) return a->id_j < b->id_j ? -1 : 1;
    return 0;
}

static int write_lineage(nbody_ctx* ctx, const char* path, int capacity) {
    int64_t total = 0;
    int rc = nbody_get_lineage(ctx, NULL, 0, &total);
    if (rc != NBODY_OK) return rc;
    nbody_ctx_desc d;
    rc = nbody_ctx_info(ctx, &d, NULL);
    if (rc != NBODY_OK) return rc;
    const int ev_cap = d.event_capacity > 0 ? d.event_capacity : (1 << 20);   /* the default of nbody_ctx_create */
    if (total > ev_cap) {
        fprintf(stderr, "lineage: %lld events were logged, the log holds %d: the history is incomplete\n", (long long)total,
                ev_cap);
        return NBODY_ERR_CAPACITY;
    }
    nbody_lineage* rec = (nbody_lineage*)malloc(sizeof(nbody_lineage) * (size_t)(total > 0 ? total : 1));
    int32_t* ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)(capacity > 0 ? capacity : 1));
    int n = 0;
    if (!rec || !ids) { free(rec); free(ids); return NBODY_ERR_NOMEM; }
    rc = nbody_get_lineage(ctx, rec, (int)total, &total);
    if (rc == NBODY_OK) rc = nbody_get_ids(ctx, ids, capacity, &n);
    FILE* f = rc == NBODY_OK ? fopen(path, "w") : NULL;
    if (rc == NBODY_OK && !f) {
        fprintf(stderr, "lineage: cannot write %s\n", path);
        rc = NBODY_ERR_IO;
    }
    if (f) {
        qsort(rec, (size_t)total, sizeof(nbody_lineage), cmp_lineage);
        for (int64_t k = 0; k < total; ++k) fprintf(f, "%d %d %d %d\n", rec[k].step, rec[k].kind, rec[k].id_i, rec[k].id_j);
        fprintf(f, "survivors\n");
        for (int i = 0; i < n; ++i) fprintf(f, "%d\n", ids[i]);
        if (fclose(f) != 0) rc = NBODY_ERR_IO;
    }
    free(rec);
    free(ids);
    return rc;
}

static int die(const char* what, int rc) {
    fprintf(stderr, "%s: %s: %s\n", what, nbody_status_string(rc), nbody_last_error_string());
    return 1;
}

int main(int argc, char** argv) {
    const char* path = "nbodyConfig.txt";
    const char* lineage_path = NULL;
    int precision = NBODY_F32, gpus = 1, dump = 0, images = 0, diag_every = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--config") && a + 1 < argc) path = argv[++a];
        else if (!strcmp(argv[a], "--fp64")) precision = NBODY_F64;
        else if (!strcmp(argv[a], "--gpus") && a + 1 < argc) gpus = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--dump")) dump = 1;
        else if (!strcmp(argv[a], "--images")) images = 1;
        else if (!strcmp(argv[a], "--lineage") && a + 1 < argc) lineage_path = argv[++a];
        else if (!strcmp(argv[a], "--diagnostics") && a + 1 < argc && atoi(argv[a + 1]) > 0) diag_every = atoi(argv[++a]);
        else {
            fprintf(stderr, "usage: nbody [--config FILE] [--fp64] [--gpus N] [--dump] [--images] [--diagnostics K] "
                            "[--lineage FILE]\n");
            return 2;
        }
    }
    if (gpus < 1 || gpus > 64) return 2;
    if (lineage_path && gpus > 1) {
        fprintf(stderr, "nbody: --lineage needs a single GPU (identities are not tracked across ranks)\n");
        return 2;
    }
    double startTime = now();
    printf("Running simulation with the following settings:\n");
    nbody_config cfg;
    int rc = nbody_config_parse(path, &cfg);
    if (rc != NBODY_OK) return 1;                     /* the reference exit(1)s here */
    printf("=====================\n");
    void* block = nbody_block_alloc(cfg.particleCount, precision);
    if (!block) return die("alloc", NBODY_ERR_NOMEM);
    printf("Bodies: %d\n", cfg.particleCount);
    rc = nbody_init_bodies(&cfg, block, precision);
    if (rc != NBODY_OK) return die("init", rc);

    nbody_ctx* ctxs[64];
    for (int g = 0; g < gpus; ++g) {
        nbody_ctx_desc d;
        nbody_ctx_desc_from_config(&d, &cfg, precision);
        d.device = g; d.rank = g; d.world = gpus;
        d.flags = gpus > 1 ? NBODY_FLAG_GROUP_EXCHANGE : 0;
        if (lineage_path) d.flags |= NBODY_FLAG_RECORD_EVENTS | NBODY_FLAG_TRACK_IDS;
        rc = nbody_ctx_create(&ctxs[g], &d);
        if (rc != NBODY_OK) return die("ctx_create", rc);
        rc = nbody_upload(ctxs[g], block, cfg.particleCount);
        if (rc != NBODY_OK) return die("upload", rc);
    }
    double t0 = now();
    if (diag_every > 0) {
        rc = print_diag(ctxs, gpus);
        if (rc != NBODY_OK) return die("diagnostics", rc);
    }
    const int every = images ? cfg.save_Image_Every_Xth_Iteration : 0;
    if (every <= 0 && diag_every <= 0) {
        rc = nbody_group_step(ctxs, gpus, cfg.totalIterations);
        if (rc != NBODY_OK) return die("step", rc);
    } else {
        unsigned char* img = every > 0 ? (unsigned char*)malloc((size_t)cfg.imgWidth * cfg.imgHeight) : NULL;
        if (every > 0 && !img) return die("image alloc", NBODY_ERR_NOMEM);
        int done = 0;
        while (done < cfg.totalIterations) {
            /* next iteration whose image the reference would save: k % every == 0 and k + 1 < totalIterations */
            int k = every > 0 ? ((done + every - 1) / every) * every : cfg.totalIterations;
            int upto = (k + 1 < cfg.totalIterations) ? k + 1 : cfg.totalIterations;
            /* and the next step count that gets a diagnostics line: a multiple of diag_every, or the last */
            if (diag_every > 0) {
                const int dnext = (done / diag_every + 1) * diag_every;
                if (dnext < upto) upto = dnext;
            }
            rc = nbody_group_step(ctxs, gpus, upto - done);
            if (rc != NBODY_OK) return die("step", rc);
            done = upto;
            if (diag_every > 0 && (done % diag_every == 0 || done == cfg.totalIterations)) {
                rc = print_diag(ctxs, gpus);
                if (rc != NBODY_OK) return die("diagnostics", rc);
            }
            if (every > 0 && k + 1 < cfg.totalIterations && done == k + 1) {
                char name[NBODY_IMAGE_PATH_MAX + 64];
                rc = nbody_render_image(ctxs[0], img, cfg.imgWidth, cfg.imgHeight);
                if (rc != NBODY_OK) return die("render", rc);
                snprintf(name, sizeof(name), "%s/iteration_%d.ppm", cfg.imagePath, k);      /* :518 */
                if (nbody_write_pgm(name, img, cfg.imgWidth, cfg.imgHeight) != NBODY_OK) return 1;   /* :369 */
            }
        }
        free(img);
    }
    int n = 0;
    rc = nbody_group_download(ctxs, gpus, block, &n);
    if (rc != NBODY_OK) return die("download", rc);
    double t1 = now();
    if (lineage_path) {
        rc = write_lineage(ctxs[0], lineage_path, cfg.particleCount);
        if (rc != NBODY_OK) return die("lineage", rc);
    }
    long long pairs = 0;
    for (int g = 0; g < gpus; ++g) {
        nbody_stats s;
        nbody_get_stats(ctxs[g], &s);
        pairs += s.pairs;
        nbody_ctx_destroy(ctxs[g]);
    }
    printf("Bodies left: %d\n", n);
    printf("Stepping: %.4f s, %.4e body-pair-interactions/sec\n", t1 - t0, (double)pairs / (t1 - t0));
    if (dump) fwrite(block, 1, nbody_block_bytes(n, precision), stdout);
    nbody_block_free(block);
    printf("Time taken: %.4f\n", now() - startTime);   /* src/nbody.cu:548 */
    return 0;
}
