// Missing-observation instances (MISSING = true) of the unscented Gaussian-sum filter kernel (ugsf_scan.hpp): the
// (n, dq, m, dr) shapes ugsf_scan.hip compiles ahead of time, up to state dimension 4 (gsf_missing_group_v.hip holds (8, 8, 4, 4)).
#include "ugsf_scan.hpp"

namespace bf {

int launch_ugsf_missing_group_u(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
        long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool* matched) {
#define BF_MISSING_CASE(N_, DQ_, M_, DR_)                                                            \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_ && p->dr == DR_) {                                    \
    *matched = true;                                                                                 \
    return launch_ugsf<N_, DQ_, M_, DR_, true>(p, up, y, u, B, T, K, carry, out, stream);            \
  }
  BF_MISSING_CASE(1, 1, 1, 1);
  BF_MISSING_CASE(2, 2, 1, 1);
  BF_MISSING_CASE(2, 2, 2, 2);
  BF_MISSING_CASE(3, 3, 1, 1);
  BF_MISSING_CASE(3, 3, 3, 3);
  BF_MISSING_CASE(4, 2, 1, 1);
  BF_MISSING_CASE(4, 2, 2, 2);
  BF_MISSING_CASE(4, 4, 2, 2);
#undef BF_MISSING_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
