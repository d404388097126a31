/* lbd_round_check: the sample-coordinate rounding of k_lbd_desc (csrc/lsd.hip, lbd_round_clamp) against the reference's, on the CPU.
 * gcc -O2 -ffp-contract=off -pthread lbd_round_check.c -lm && ./a.out
 *   reference   (short)round(x), then (t < 0) ? 0 : (t > hi) ? hi : t            (binary_descriptor_custom.cpp, computeLBD)
 *   kernel      y = x + copysign(0.49999997, x), the median of (y, 0, hi) as floats, truncated
 * Every float in [-70000, 70000] is walked by its bit pattern, for several image sizes hi + 1; where round(x) leaves a short the reference
 * wraps, so there the kernel's form is compared with round + clamp on an int (the kernels take that form only where no sample can get
 * there) and, separately, the add-and-truncate alone is compared with roundf at the edges of its range.  The exit status is the number
 * of mismatches (at most 255). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <pthread.h>

static inline float f_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static inline uint32_t b_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static inline float add_trunc(float x) { return truncf(x + copysignf(0x1.fffffep-2f, x)); }
static inline int kernel_form(float x, float hi)
{
    float y = x + copysignf(0x1.fffffep-2f, x);
    y = fminf(fmaxf(y, 0.f), hi);
    return (int)y;
}
/* t = round(x) as the reference forms it; inside a short the cast keeps the value, outside it the int stands for "no wrap" */
static inline int reference_form(float r, int hi) { const int i = (int)r, t = fabsf(r) <= 32767.f ? (int)(short)i : i; return (t < 0) ? 0 : (t > hi) ? hi : t; }

#define NHI 6
static const int his[NHI] = { 0, 1, 79, 95, 639, 15999 };
static long seen = 0;

/* mismatches at x; branch-free so the walk over 2.4e9 floats stays a matter of seconds (say = 1: print them) */
static inline long check(float x, int say)
{
    const float r = roundf(x), t = add_trunc(x);
    long bad = t != r;
    if (say && bad) printf("add-and-truncate %.9g -> %.9g, roundf %.9g\n", x, t, r);
    if (fabsf(x) >= 2147483648.f) return bad;
    for (int k = 0; k < NHI; k++) {
        const int a = kernel_form(x, (float)his[k]), b = reference_form(r, his[k]);
        bad += a != b;
        if (say && a != b) printf("x %.9g hi %d: kernel %d, reference %d\n", x, his[k], a, b);
    }
    return bad;
}

/* the walk is cut into slices for as many threads (2.4e9 floats x seven comparisons: a minute on one core) */
#define NTHREADS 8
struct slice { uint32_t lo, hi; long bad; };
static void *walk(void *arg)
{
    struct slice *s = (struct slice *)arg;
    long bad = 0;
    for (uint32_t b = s->lo; b < s->hi; b++) bad += check(f_of(b), 0) + check(f_of(b | 0x80000000u), 0);
    s->bad = bad;
    return NULL;
}

int main(void)
{
    const uint32_t top = b_of(70000.f);                                                          /* +-0 and the denormals are the first patterns */
    long bad = 0;
    pthread_t th[NTHREADS]; struct slice sl[NTHREADS];
    for (int i = 0; i < NTHREADS; i++) {
        sl[i].lo = (uint32_t)(((uint64_t)top + 1) * i / NTHREADS); sl[i].hi = (uint32_t)(((uint64_t)top + 1) * (i + 1) / NTHREADS); sl[i].bad = 0;
        if (pthread_create(&th[i], NULL, walk, &sl[i])) { printf("no thread\n"); return 255; }
    }
    for (int i = 0; i < NTHREADS; i++) { pthread_join(th[i], NULL); bad += sl[i].bad; }
    seen = 2 * ((long)top + 1);
    if (bad) {                                                                                   /* once more, naming the first few */
        long shown = 0;
        for (uint32_t b = 0; b <= top && shown < 10; b++) shown += check(f_of(b), 1) + check(f_of(b | 0x80000000u), 1);
    }
    const float edge[] = { 0.5f, 1.5f, 2.5f, 0.75f, 8388607.f, 8388608.f, 8388609.f, 4194303.5f, 4194304.5f, 16777216.f, 2147483520.f, 32767.5f, 32768.5f, 1e-45f, 1.17549435e-38f };
    for (unsigned k = 0; k < sizeof(edge) / sizeof(edge[0]); k++)
        for (int d = -2; d <= 2; d++) {                                                          /* the value and two neighbours on either side (0.5 - ulp among them) */
            const uint32_t b = b_of(edge[k]) + (uint32_t)d;
            if ((int32_t)b < 0) continue;
            bad += check(f_of(b), 1) + check(f_of(b | 0x80000000u), 1);
            seen += 2;
        }
    printf("floats %ld mismatches %ld\n", seen, bad);
    return bad > 255 ? 255 : (int)bad;
}
