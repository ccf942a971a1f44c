// Instantiations of the lane-group Kalman kernel (kf_scan_group.hpp) for a slice of the
// (n, m, lanes-per-trajectory) table; split over several translation units to build in parallel.
// Built twice (bf_common.hpp): as it stands, and with -DBF_MISSING=true for the missing-observation instances of the same rows.
#include "kf_scan_group.hpp"

namespace bf {

int BF_GROUP_FN(kf, b)(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
        const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes, bool* matched) {
#define BF_CASE(N_, M_, NL_)                                                                \
  if (p->n == N_ && p->m == M_ && (lanes == 0 || lanes == NL_)) {                           \
    *matched = true;                                                                        \
    return launch_nml<N_, M_, NL_, BF_MISSING>(p, y, B, T, carry, out, stream, force_mode); \
  }
  BF_CASE(4, 2, 2);
  BF_CASE(4, 4, 2);
  BF_CASE(5, 2, 4);
  BF_CASE(6, 2, 4);
  BF_CASE(7, 2, 4);
  BF_CASE(8, 2, 4);
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
