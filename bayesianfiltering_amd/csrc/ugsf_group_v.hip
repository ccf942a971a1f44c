// Instantiation of the unscented Gaussian-sum filter kernel (ugsf_scan.hpp) for the largest shape compiled ahead of time; a
// translation unit of its own, since it alone builds as long as the other eight (ugsf_group_u.hip).
// Built twice (bf_common.hpp): as it stands, and with -DBF_MISSING=true for the missing-observation instance of the same row.
#include "ugsf_scan.hpp"

namespace bf {

int BF_GROUP_FN(ugsf, v)(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
        long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool* matched) {
#define BF_CASE(N_, DQ_, M_, DR_)                                                               \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_ && p->dr == DR_) {                               \
    *matched = true;                                                                            \
    return launch_ugsf<N_, DQ_, M_, DR_, BF_MISSING>(p, up, y, u, B, T, K, carry, out, stream); \
  }
  BF_CASE(8, 8, 4, 4);   // Lorenz-96 with the even-state emission (nonlinearities.py:37-50)
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
