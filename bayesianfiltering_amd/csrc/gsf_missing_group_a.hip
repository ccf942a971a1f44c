// Missing-observation instances (MISSING = true) of the Gaussian-sum / EKF kernel (gsf_scan.hpp) for the (n, m, lanes-per-chain)
// rows of gsf_group_a.hip, both emitters and the EXT instances; split over several translation units to build in parallel.
#include "gsf_scan.hpp"

namespace bf {

int launch_gsf_missing_group_a(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
        const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes, bool* matched) {
#define BF_MISSING_CASE(N_, M_, NL_)                                                                            \
  if (p->n == N_ && p->m == M_ && (lanes == 0 || lanes == NL_)) {                                               \
    *matched = true;                                                                                            \
    return launch_gsf<N_, M_, NL_, SPEC_GENERIC, true>(p, y, u, B, T, K, carry, out, stream, force_mode);       \
  }
  BF_MISSING_CASE(1, 1, 1);
  BF_MISSING_CASE(3, 3, 1);
  BF_MISSING_CASE(4, 3, 2);
  BF_MISSING_CASE(5, 3, 1);
  BF_MISSING_CASE(6, 3, 2);
  BF_MISSING_CASE(8, 1, 2);
  BF_MISSING_CASE(8, 4, 4);
#undef BF_MISSING_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
