/*
 * cuda_runtime.h — host stand-in for the CUDA header the reference's device headers include
 * (glmCUDA.h).  TEST INFRASTRUCTURE ONLY; used by the oracle/_ref recipe (oracle/Makefile).
 *
 * The reference's BSDF, RNG and surface headers are plain C++ behind CUDA function
 * qualifiers.  With the qualifiers empty they compile with a host compiler, which is what
 * lets tests/test_oracle_vs_reference.py compare the hand-written oracle with the code it
 * restates.  Nothing here is taken from the reference or from CUDA.
 */
#ifndef PTREF_SHIM_CUDA_RUNTIME_H
#define PTREF_SHIM_CUDA_RUNTIME_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <math.h>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))

/* the device headers call these unqualified */
using std::isinf;
using std::isnan;

/* OptiX payload registers 0 and 1: the per-ray record pointer that IsDebugRay() reads.
 * ptref_capi.cpp defines them to point at one zeroed record. */
uint32_t optixGetPayload_0();
uint32_t optixGetPayload_1();

#endif
