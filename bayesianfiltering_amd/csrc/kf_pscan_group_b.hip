// Instantiations of the parallel-in-time Kalman kernels (kf_pscan.hpp) for a slice of the (n, m) table; split over several
// translation units to build in parallel.
// Built twice (bf_common.hpp): as it stands, and with -DBF_MISSING=true for the missing-observation instances of the same rows.
#include "kf_pscan.hpp"

namespace bf {

int BF_GROUP_FN(kf_pscan, b)(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
        const bf_out_desc* out, float* workspace, int L, hipStream_t stream, bool* matched) {
#define BF_CASE(N_, M_)                                                                       \
  if (p->n == N_ && p->m == M_) {                                                             \
    *matched = true;                                                                          \
    return launch_pscan_nm<N_, M_, BF_MISSING>(p, y, B, T, carry, out, workspace, L, stream); \
  }
  BF_CASE(3, 1);
  BF_CASE(3, 2);
  BF_CASE(3, 3);
  BF_CASE(3, 4);
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
