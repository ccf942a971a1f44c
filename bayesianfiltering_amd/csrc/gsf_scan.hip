// Dispatch of the Gaussian-sum / EKF kernel over the compiled (n, m, lanes) table (instantiations live in
// gsf_group_{a,b,c,d,e}.hip, each built plain and with MISSING = true for the missing-observation instances).
#include "bf_common.hpp"

namespace bf {

using GsfGroup = int(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                     const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes, bool* matched);
GsfGroup launch_gsf_group_a, launch_gsf_group_b, launch_gsf_group_c, launch_gsf_group_d, launch_gsf_group_e,
    launch_gsf_missing_group_a, launch_gsf_missing_group_b, launch_gsf_missing_group_c, launch_gsf_missing_group_d,
    launch_gsf_missing_group_e;
// in the order they are tried: the structure-aware instances first (Lorenz-96 + pick-even emission)
static GsfGroup* const kPlainGroups[] = {launch_gsf_group_e, launch_gsf_group_a, launch_gsf_group_b, launch_gsf_group_c,
                                         launch_gsf_group_d};
static GsfGroup* const kMissingGroups[] = {launch_gsf_missing_group_e, launch_gsf_missing_group_a, launch_gsf_missing_group_b,
                                           launch_gsf_missing_group_c, launch_gsf_missing_group_d};

// default lanes per chain: the largest column block per lane that divides n (fewest redundant VALU ops)
static const int kGsfDefaultLanes[9] = {0, 1, 1, 1, 2, 1, 2, 1, 2};
int gsf_default_lanes(int n) { return (n >= 1 && n <= 8) ? kGsfDefaultLanes[n] : 0; }

Option g_gsf_structured{1, OPT_GSF_STRUCTURED};  // tuning / test hook (bf_set_option "gsf_structured")

static int run_gsf_groups(bool missing, const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                          const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  if (lanes == 0) lanes = gsf_default_lanes(p->n);
  const size_t skip = g_gsf_structured ? 0 : 1;   // (option off: past the structure-aware slice)
  bool matched;
  const int rc = run_groups((missing ? kMissingGroups : kPlainGroups) + skip, std::size(kPlainGroups) - skip, &matched, p, y, u, B,
                            T, K, carry, out, stream, force_mode, lanes);
  if (matched) return rc;
  if (missing)
    return set_error(BF_EUNSUPPORTED, "gaussian-sum filter with missing observations: (n=%d, m=%d, lanes=%d) is not compiled in "
                                      "(n = 1..8 with m = 1..min(n,4))", p->n, p->m, lanes);
  return set_error(BF_EUNSUPPORTED, "gaussian-sum filter: (n=%d, m=%d, lanes=%d) is not compiled in (n = 1..8 with m = 1..min(n,4))",
                   p->n, p->m, lanes);
}

// n = 1..8 with m = 1..min(n, 4); `lanes` = 0 picks the default lanes per chain.
int launch_gsf_ekf(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                   const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  return run_gsf_groups(false, p, y, u, B, T, K, carry, out, stream, force_mode, lanes);
}

// bf_gsf_ekf_missing_f32: the MISSING = true instances of the same table.  No other kernel takes gaps, so a shape without an
// instance is an error here, never a fallback.
int launch_gsf_ekf_missing(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                           const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes) {
  return run_gsf_groups(true, p, y, u, B, T, K, carry, out, stream, force_mode, lanes);
}

}  // namespace bf
