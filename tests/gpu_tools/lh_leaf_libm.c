/*
 * lh_leaf_libm.c -- TEST TOOL, part of libhipemu_leaf.so: the host libm over a sweep, for the math leaves of
 * csrc/lh_dev_math.h that restate it (powf, logf, log10f) and the two double expressions of the old VBR loop
 * (reference quantize.c:1419-1426).  tests/golden/make_leaf_math_golden.py records its digests on the libm the
 * reference was built with (glibc 2.35); tests/test_device_leaves.py compares the host-compiled leaves with it.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float
as_f32(uint32_t u)
{
    float   f;
    memcpy(&f, &u, 4);
    return f;
}

/* op: 0 powf(a, b), 1 logf(a), 2 log10f(a), 3 adjust(pe = a; flag: short block), 4 masking_lower(db = a) */
int
lh_leaf_libm(int op, long n, const uint32_t *a, const uint32_t *b, uint32_t *out, int flag)
{
    for (long k = 0; k < n; k++) {
        volatile float x = as_f32(a[k]);
        float   r;
        switch (op) {
        case 0:
            r = powf(x, as_f32(b[k]));
            break;
        case 1:
            r = logf(x);
            break;
        case 2:
            r = log10f(x);
            break;
        case 3:
            r = flag ? (float) (2.56 / (1 + exp(3.5 - x / 300.)) - 0.14) : (float) (1.28 / (1 + exp(3.5 - x / 300.)) - 0.05);
            break;
        case 4:
            r = (float) pow(10.0, x * 0.1);
            break;
        default:
            return -1;
        }
        memcpy(&out[k], &r, 4);
    }
    return 0;
}
