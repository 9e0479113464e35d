/* maskpred_ref_harness.c -- MEASUREMENT INFRASTRUCTURE of tools/maskpred_timing.py: the reference's wedge / diff-weighted search of one block, composed from the
 * reference's own helper functions as pick_wedge and pick_interinter_seg compose them (use_rate == 0), called from C on N host threads.  The tool compiles this file
 * next to itself, hands it the library and the symbols to time and a file with one block's inputs, and reads one line of numbers back.  Nothing of the reference is
 * compiled in: the functions are looked up in the shared library at run time.
 *
 *   harness LIB sum_squares delta_squares sign_from_residuals sse_from_residuals diffwtd_mask INPUT bw bh threads blocks_per_thread
 *
 * INPUT: 32 masks of bw * bh bytes (wedge index, then sign), then r0, r1, d10 as int16_t[bw * bh], then p0, p1 as uint8_t[bw * bh].
 * Output: ns per block with all threads running, ns per block on one thread, then the 16 SSEs, the 16 signs and the two diff-weighted SSEs of the block. */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef uint64_t (*SumSq)(const int16_t *, uint32_t);
typedef void (*Delta)(int16_t *, const int16_t *, const int16_t *, int);
typedef int8_t (*Sign)(const int16_t *, const uint8_t *, int, int64_t);
typedef uint64_t (*Sse)(const int16_t *, const int16_t *, const uint8_t *, int);
typedef void (*Diffwtd)(uint8_t *, uint8_t, const uint8_t *, int, const uint8_t *, int, int, int);

static SumSq   f_sumsq;
static Delta   f_delta;
static Sign    f_sign;
static Sse     f_sse;
static Diffwtd f_diffwtd;
static int     bw, bh, n, blocks;
static uint8_t *in_masks, *in_p0, *in_p1;
static int16_t *in_r0, *in_r1, *in_d10;
static pthread_barrier_t barrier;

typedef struct { uint64_t sse[16], seg[2]; int8_t sign[16]; } Result;

static void *aligned(size_t bytes) {
    void *p = NULL;
    if (posix_memalign(&p, 64, (bytes + 63) & ~(size_t)63)) exit(3);
    return p;
}

static void search(const uint8_t *masks, const int16_t *r0, const int16_t *r1, const int16_t *d10, const uint8_t *p0, const uint8_t *p1, int16_t *ds, uint8_t *seg,
                   Result *out) {
    const int64_t limit = ((int64_t)f_sumsq(r0, (uint32_t)n) - (int64_t)f_sumsq(r1, (uint32_t)n)) * 32;
    f_delta(ds, r0, r1, n);
    for (int k = 0; k < 16; k++) {
        const int8_t s = f_sign(ds, masks + (size_t)(2 * k) * n, n, limit);
        out->sign[k]   = s;
        out->sse[k]    = f_sse(r1, d10, masks + (size_t)(2 * k + s) * n, n);
    }
    for (int t = 0; t < 2; t++) {
        f_diffwtd(seg, (uint8_t)t, p0, bw, p1, bw, bh, bw);
        out->seg[t] = f_sse(r1, d10, seg, n);
    }
}

static void *worker(void *arg) {
    Result  *out   = (Result *)arg;
    uint8_t *masks = aligned((size_t)32 * n), *p0 = aligned(n), *p1 = aligned(n), *seg = aligned(n);
    int16_t *r0 = aligned(2 * (size_t)n), *r1 = aligned(2 * (size_t)n), *d10 = aligned(2 * (size_t)n), *ds = aligned(2 * (size_t)n);
    memcpy(masks, in_masks, (size_t)32 * n);
    memcpy(p0, in_p0, n), memcpy(p1, in_p1, n);
    memcpy(r0, in_r0, 2 * (size_t)n), memcpy(r1, in_r1, 2 * (size_t)n), memcpy(d10, in_d10, 2 * (size_t)n);
    search(masks, r0, r1, d10, p0, p1, ds, seg, out); /* warm */
    pthread_barrier_wait(&barrier);
    for (int i = 0; i < blocks; i++) search(masks, r0, r1, d10, p0, p1, ds, seg, out);
    pthread_barrier_wait(&barrier);
    return NULL;
}

static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec * 1e9 + (double)t.tv_nsec;
}

static double run(int threads, Result *res) {
    pthread_t th[64];
    pthread_barrier_init(&barrier, NULL, (unsigned)threads + 1);
    for (int i = 0; i < threads; i++) pthread_create(&th[i], NULL, worker, &res[i]);
    pthread_barrier_wait(&barrier);
    const double t0 = now();
    pthread_barrier_wait(&barrier);
    const double t1 = now();
    for (int i = 0; i < threads; i++) pthread_join(th[i], NULL);
    pthread_barrier_destroy(&barrier);
    return (t1 - t0) / ((double)threads * blocks);
}

int main(int argc, char **argv) {
    if (argc != 12) return 2;
    void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 4; }
    f_sumsq   = (SumSq)dlsym(lib, argv[2]);
    f_delta   = (Delta)dlsym(lib, argv[3]);
    f_sign    = (Sign)dlsym(lib, argv[4]);
    f_sse     = (Sse)dlsym(lib, argv[5]);
    f_diffwtd = (Diffwtd)dlsym(lib, argv[6]);
    if (!f_sumsq || !f_delta || !f_sign || !f_sse || !f_diffwtd) return 5;
    bw = atoi(argv[8]), bh = atoi(argv[9]);
    int threads = atoi(argv[10]);
    blocks      = atoi(argv[11]);
    n           = bw * bh;
    if (n < 64 || n > 1024 || threads < 1 || threads > 64 || blocks < 1) return 2;
    in_masks = aligned((size_t)32 * n), in_p0 = aligned(n), in_p1 = aligned(n);
    in_r0 = aligned(2 * (size_t)n), in_r1 = aligned(2 * (size_t)n), in_d10 = aligned(2 * (size_t)n);
    FILE *f = fopen(argv[7], "rb");
    if (!f) return 6;
    size_t got = fread(in_masks, 1, (size_t)32 * n, f) + fread(in_r0, 2, n, f) + fread(in_r1, 2, n, f) + fread(in_d10, 2, n, f) + fread(in_p0, 1, n, f) + fread(in_p1, 1, n, f);
    fclose(f);
    if (got != (size_t)32 * n + 5 * (size_t)n) return 6;
    Result *res  = calloc(64, sizeof(Result));
    const double all = run(threads, res), one = run(1, res);
    printf("%.1f %.1f", all, one);
    for (int k = 0; k < 16; k++) printf(" %llu", (unsigned long long)res[0].sse[k]);
    for (int k = 0; k < 16; k++) printf(" %d", (int)res[0].sign[k]);
    printf(" %llu %llu\n", (unsigned long long)res[0].seg[0], (unsigned long long)res[0].seg[1]);
    return 0;
}
