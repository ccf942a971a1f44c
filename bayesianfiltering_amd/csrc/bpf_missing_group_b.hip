// The MISSING = true instances (NaN observations are gaps: bpf_missing.hpp) of the bootstrap particle filter kernels for the
// rows of bpf_group_b.hip, in a translation unit of their own.
#include "bpf_wide.hpp"

namespace bf {

int launch_bpf_missing_group_b(const bf_bpf_model* bp, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int NP,
        float ess, int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out, hipStream_t stream, bool* matched) {
  const bf_model* p = &bp->ssm;
#define BF_MISSING_CASE(N_, DQ_, M_)                                                                        \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_) {                                                     \
    *matched = true;                                                                                  \
    return launch_bpf_dims<N_, DQ_, M_, true>(bp, y, u, B, T, NP, ess, resampler, key, cr, out, stream); \
  }
  BF_MISSING_CASE(1, 1, 1);
  BF_MISSING_CASE(3, 3, 3);
  BF_MISSING_CASE(4, 4, 2);
  BF_MISSING_CASE(8, 8, 4);
#undef BF_MISSING_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
