// Stands in for <hip/hip_runtime.h> when csrc/kf_math.hpp is compiled for the HOST by a plain C++ compiler (tests only): the
// qualifiers vanish and the four single-instruction transcendentals become their libm forms.  rcp(1), sqrt(1) and log2(1) are
// exact in both, which is all the embedding argument of the missing-observation step needs.
#pragma once
#include <cmath>
#define __device__
#define __forceinline__ inline
static inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
static inline float __builtin_amdgcn_sqrtf(float x) { return std::sqrt(x); }
static inline float __builtin_amdgcn_logf(float x) { return std::log2(x); }
static inline float __builtin_amdgcn_exp2f(float x) { return std::exp2(x); }
