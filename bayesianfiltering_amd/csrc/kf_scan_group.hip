// Dispatch of the lane-group Kalman kernel over the compiled (n, m, lanes) table (instantiations live in
// kf_group_{a,b,c,d}.hip, each built plain and with MISSING = true for the missing-observation instances).
#include "bf_common.hpp"

namespace bf {

using KfGroup = int(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes, bool* matched);
KfGroup launch_kf_group_a, launch_kf_group_b, launch_kf_group_c, launch_kf_group_d, launch_kf_missing_group_a,
    launch_kf_missing_group_b, launch_kf_missing_group_c, launch_kf_missing_group_d;
static KfGroup* const kPlainGroups[] = {launch_kf_group_a, launch_kf_group_b, launch_kf_group_c, launch_kf_group_d};
static KfGroup* const kMissingGroups[] = {launch_kf_missing_group_a, launch_kf_missing_group_b, launch_kf_missing_group_c,
                                          launch_kf_missing_group_d};

// default lanes per trajectory, n = 1..8
static int default_lanes(int n) { return n <= 2 ? 1 : (n <= 4 ? 2 : 4); }

static int run_kf_groups(bool missing, const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                         const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  bool matched;
  const int rc = run_groups(missing ? kMissingGroups : kPlainGroups, std::size(kPlainGroups), &matched, p, y, B, T, carry, out,
                            stream, force_mode, lanes);
  if (matched) return rc;
  if (missing)
    return set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: (n=%d, m=%d, lanes=%d) is not compiled in", p->n,
                     p->m, lanes);
  return set_error(BF_EUNSUPPORTED,
                   "kalman filter: (n=%d, m=%d, lanes=%d) is not compiled in (n = 1..8 with m = 1..min(n,4); n = 64, m = 32)",
                   p->n, p->m, lanes);
}

// n = 1..8 with m = 1..min(n, 4); `lanes` = 0 picks the default lanes per trajectory.
int launch_kf_group(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  if (lanes == 0 && p->n >= 1 && p->n <= 8) lanes = default_lanes(p->n);
  return run_kf_groups(false, p, y, B, T, carry, out, stream, force_mode, lanes);
}

// The missing-observation route (bf_kalman_filter_missing_f32): every (n, m) pair of the table above, at its default lanes
// per trajectory only.  0 = no instance; the entry point asks before its first HIP call.
int kf_missing_default_lanes(int n, int m) {
  if (n < 1 || n > 8 || m < 1 || m > 4 || m > n) return 0;
  return default_lanes(n);
}

int launch_kf_missing_group(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                            const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  return run_kf_groups(true, p, y, B, T, carry, out, stream, force_mode, lanes);
}

}  // namespace bf
