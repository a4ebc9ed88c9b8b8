/* What the three sanitizer programs of the polar subsystem (polar_sanitize.c, polar_wide_sanitize.c, polar_list_sanitize.c) share: the check, the
 * stand-in for the library's error text, the generator, the draw of a code's information positions and the filler of a batch of beliefs. */
#ifndef POLAR_SANITIZE_COMMON_H
#define POLAR_SANITIZE_COMMON_H

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

/* the last refusal's text: the mirrors are linked without the library's own qldpc_set_error */
static char msg[256];
void qldpc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static inline int get(const uint32_t *row, long i) { return (int)((row[i >> 5] >> (31 - (i & 31))) & 1u); }

/* n_info distinct positions below N, the head of a shuffle of 0 .. N - 1: malloc'ed at exactly max(n_info, 1) entries */
static inline int *draw_info_pos(long N, int n_info)
{
    int *pos = (int *)malloc(sizeof(int) * (size_t)(n_info ? n_info : 1)), *perm = (int *)malloc(sizeof(int) * (size_t)N);
    for (long i = 0; i < N; i++) perm[i] = (int)i;
    for (long i = N - 1; i > 0; i--) { const long j = (long)(rnd() % (uint64_t)(i + 1)); const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
    for (int m = 0; m < n_info; m++) pos[m] = perm[m];
    free(perm);
    return pos;
}

/* `count` beliefs: floats k / div with k uniform in -half .. half, or every int8 value */
static inline void fill_llr(void *llr, long count, int f32, int half, float div)
{
    for (long i = 0; i < count; i++) {
        if (f32) ((float *)llr)[i] = (float)((double)(int64_t)(rnd() % (uint64_t)(2 * half + 1)) - (double)half) / div;
        else ((int8_t *)llr)[i] = (int8_t)(rnd() & 0xff);
    }
}

#endif /* POLAR_SANITIZE_COMMON_H */
