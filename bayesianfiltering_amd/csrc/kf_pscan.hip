// Host side of the parallel-in-time Kalman filter (kf_pscan.hpp): argument checks (all before the first HIP call), block
// geometry, workspace size, and the dispatch over the compiled (n, m) table (instantiations: kf_pscan_group_{a,...,f}.hip,
// each built plain and with MISSING = true for the missing-observation twins).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance n = 1 ... 6, m = 1 ... 4 of the
// three kernels builds without scratch; at n = 7 the scan kernel spills 860 bytes per lane (n = 8: fold 436, scan 1628), so
// the limit is n = 6.  The MISSING = true twins of fold and emit build without scratch at every (n, m) too (the fold stages
// the pattern table, at most 9 984 bytes, in LDS).  Tables per instance: DESIGN.md, section 6h.
#include "forward_host.hpp"
#include "pscan_host.hpp"

namespace bf {

using KfPscanGroup = int(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                         const bf_out_desc* out, float* workspace, int L, hipStream_t stream, bool* matched);
KfPscanGroup launch_kf_pscan_group_a, launch_kf_pscan_group_b, launch_kf_pscan_group_c, launch_kf_pscan_group_d,
    launch_kf_pscan_group_e, launch_kf_pscan_group_f, launch_kf_pscan_missing_group_a, launch_kf_pscan_missing_group_b,
    launch_kf_pscan_missing_group_c, launch_kf_pscan_missing_group_d, launch_kf_pscan_missing_group_e,
    launch_kf_pscan_missing_group_f;
static KfPscanGroup* const kPlainGroups[] = {launch_kf_pscan_group_a, launch_kf_pscan_group_b, launch_kf_pscan_group_c,
                                             launch_kf_pscan_group_d, launch_kf_pscan_group_e, launch_kf_pscan_group_f};
static KfPscanGroup* const kMissingGroups[] = {launch_kf_pscan_missing_group_a, launch_kf_pscan_missing_group_b,
                                               launch_kf_pscan_missing_group_c, launch_kf_pscan_missing_group_d,
                                               launch_kf_pscan_missing_group_e, launch_kf_pscan_missing_group_f};

static const char NAME[] = "parallel kalman filter";
constexpr int PSCAN_M_MAX = 4;

static Option g_pkf_block{0, OPT_PKF_BLOCK};   // 0 = from (B, T)
Option& pkf_block_option() { return g_pkf_block; }

// Default block length: pscan_default_block (pscan_host.hpp) with one lane per (trajectory, block) and the balance constant
// from the measurements in profiles/parallel_kalman_probe.txt (n = 4, m = 2): the scan is one workgroup per trajectory and
// costs about 80 ns per block, a lane's fold and emit about 4 us per step: T / L * 80 ns + L * 4 us is smallest at
// L = sqrt(T / 50) (B = 1, T = 10^6: 1.6 ms at L = 64 ... 256 against 5.1 ms at L = 16).  The floor of 16 keeps the fold's
// aggregate (56 floats at n = 4) a small fraction of a block's streams.
int kf_pscan_default_block(long long B, long long T) { return pscan_default_block(B, T, 50); }

static int check_dims(int n, int m) {
  if (const int rc = check_dimensions(n, 1, m, 1)) return rc;
  if (n > PSCAN_N_MAX || m > PSCAN_M_MAX)
    return set_error(BF_EUNSUPPORTED,
                     "parallel kalman filter: (n=%d, m=%d) is not compiled in (register kernels for n = 1..%d, m = 1..%d; the scan needs scratch from n = %d)", n, m,
                     PSCAN_N_MAX, PSCAN_M_MAX, PSCAN_N_MAX + 1);
  return BF_OK;
}

// 4 B ceil(T / L) (4 n^2 + 3 n) bytes: per (trajectory, block) one span (3 n^2 + 2 n floats) and one start state (n^2 + n)
long long kf_pscan_workspace_bytes(int n, int m, long long B, long long T, int block) {
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  int rc = check_dims(n, m);
  if (rc != BF_OK) return rc;
  const int L = resolve_block(NAME, g_pkf_block, block, kf_pscan_default_block(B, T));
  if (L < 0) return L;
  const long long NB = pscan_blocks(NAME, B, 0, T, L);
  return NB < 0 ? NB : 4LL * B * NB * (4LL * n * n + 3LL * n);
}

// `missing`: bf_kalman_filter_pscan_missing_f32 -- the same checks in the same order and words, then the MISSING = true twins.
int launch_kf_pscan(const bf_lgssm* model, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, void* workspace, long long workspace_bytes, hipStream_t stream, bool missing) {
  if (!model || !y || !carry || !out || !workspace) return set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  int rc = check_lgssm(model);
  if (rc != BF_OK) return rc;
  if (model->Q_steps > 1 || model->R_steps > 1)
    return set_error(BF_EUNSUPPORTED, "parallel kalman filter: constant Q and R only (Q_steps=%d, R_steps=%d)", model->Q_steps,
                     model->R_steps);
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return set_error(BF_EUNSUPPORTED, "parallel kalman filter: collapsed streams are not produced (with one component they equal means / covs)");
  if ((rc = check_dims(model->n, model->m)) != BF_OK || (rc = check_streams(y, carry)) != BF_OK) return rc;
  const int L = resolve_block(NAME, g_pkf_block, 0, kf_pscan_default_block(B, T));
  if (L < 0) return L;
  const long long need = kf_pscan_workspace_bytes(model->n, model->m, B, T, L);
  if (need < 0) return (int)need;
  if ((rc = pscan_check_workspace(NAME, "bf_kalman_pscan_workspace_bytes", workspace, workspace_bytes, need, B, T, 0, L)) != BF_OK)
    return rc;

  bool matched;
  rc = run_groups(missing ? kMissingGroups : kPlainGroups, std::size(kPlainGroups), &matched, model, y, B, T, carry, out,
                  static_cast<float*>(workspace), L, stream);
  if (matched) return rc;
  return set_error(BF_EUNSUPPORTED, "parallel kalman filter: (n=%d, m=%d) is not compiled in", model->n, model->m);
}

}  // namespace bf
