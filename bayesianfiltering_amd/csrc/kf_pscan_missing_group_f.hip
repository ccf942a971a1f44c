// Missing-observation instances (MISSING = true) of the parallel-in-time Kalman kernels (kf_pscan.hpp) for the same slice of
// the (n, m) table as kf_pscan_group_f.hip; split over several translation units to build in parallel.
#include "kf_pscan.hpp"

namespace bf {

int launch_kf_pscan_missing_group_f(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
        const bf_out_desc* out, float* workspace, int L, hipStream_t stream, bool* matched) {
#define BF_MISSING_CASE(N_, M_)                                                          \
  if (p->n == N_ && p->m == M_) {                                                        \
    *matched = true;                                                                     \
    return launch_pscan_nm<N_, M_, true>(p, y, B, T, carry, out, workspace, L, stream); \
  }
  BF_MISSING_CASE(6, 1);
  BF_MISSING_CASE(6, 2);
  BF_MISSING_CASE(6, 3);
  BF_MISSING_CASE(6, 4);
#undef BF_MISSING_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
