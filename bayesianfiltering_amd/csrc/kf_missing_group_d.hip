// Missing-observation instances (MISSING = true) of the lane-group Kalman kernel (kf_scan_group.hpp) for a slice of the
// (n, m) table, each pair at its default lanes per trajectory; split over several translation units to build in parallel.
#include "kf_scan_group.hpp"

namespace bf {

int launch_kf_missing_group_d(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
        const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes, bool* matched) {
#define BF_MISSING_CASE(N_, M_, NL_)                                                   \
  if (p->n == N_ && p->m == M_ && (lanes == 0 || lanes == NL_)) {                      \
    *matched = true;                                                                   \
    return launch_nml<N_, M_, NL_, true>(p, y, B, T, carry, out, stream, force_mode); \
  }
  BF_MISSING_CASE(2, 1, 1);
  BF_MISSING_CASE(2, 2, 1);
  BF_MISSING_CASE(3, 2, 2);
  BF_MISSING_CASE(5, 4, 4);
  BF_MISSING_CASE(6, 4, 4);
  BF_MISSING_CASE(7, 4, 4);
  BF_MISSING_CASE(8, 4, 4);
#undef BF_MISSING_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
