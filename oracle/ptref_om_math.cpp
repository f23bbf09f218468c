/*
 * ptref_om_math.cpp — sinf / cosf / expf of oracle/_ref/libptref_om.so.  TEST INFRASTRUCTURE ONLY.
 *
 * The reference calls CUDA's libdevice transcendentals, which no host libm reproduces bit for
 * bit; the oracle and the HIP kernels evaluate fixed polynomials in their place (pt_oracle.c,
 * orc_math_eval).  libptref_om.so is the reference's own headers with those polynomials behind
 * the same three calls, so everything AROUND the transcendentals is compared exactly.
 *
 * The definitions are hidden: they bind the calls inside libptref_om.so at link time and are
 * exported to nobody, so liboracle.so, numpy and the rest of the process keep libm's.  This
 * file includes no math header on purpose (it would declare the three with another linkage).
 */
#include <stdint.h>

extern "C" {

void orc_math_eval(int32_t fn, const float* x, float* out, int32_t n);

#define PTREF_LOCAL __attribute__((visibility("hidden")))

PTREF_LOCAL float sinf(float x) {
    float r;
    orc_math_eval(0, &x, &r, 1);
    return r;
}
PTREF_LOCAL float cosf(float x) {
    float r;
    orc_math_eval(1, &x, &r, 1);
    return r;
}
PTREF_LOCAL float expf(float x) {
    float r;
    orc_math_eval(2, &x, &r, 1);
    return r;
}

}  /* extern "C" */
