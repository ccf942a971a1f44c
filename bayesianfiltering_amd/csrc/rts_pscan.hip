// Host side of the parallel-in-time RTS smoother (rts_pscan.hpp): its two C entry points, the argument checks (all before the
// first HIP call), block geometry, workspace size, and the dispatch over the compiled table n = 1 ... 6 x {predictions given,
// recomputed} (instantiations: rts_pscan_group_{a,...,d}.hip).  The model validation, the route's constants and the views are
// the serial smoother's (backward_host.hpp).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance of the three kernels, n = 1 ... 6,
// both routes, builds without scratch.  Table per instance: DESIGN.md, section 6i.  n <= 6 is the parallel filter's limit
// (kf_pscan.hip), whose streams this pass smooths.
#include "backward_host.hpp"
#include "pscan_host.hpp"

namespace bf {

using RtsPscanGroup = int(const BackwardRoute& r, const RtsViews& v, long long B, long long T, float* workspace, int L,
                          hipStream_t stream, bool* matched);
RtsPscanGroup launch_rts_pscan_group_a, launch_rts_pscan_group_b, launch_rts_pscan_group_c, launch_rts_pscan_group_d;

static const char NAME[] = "parallel rts smoother";

static Option g_prs_block{0, OPT_PRS_BLOCK};   // 0 = from (B, T)
Option& prs_block_option() { return g_prs_block; }

// Default block length: kf_pscan_default_block(B, T), the parallel filter's rule -- the largest of ceil(B T / 65 536), the smallest s with
// 50 s^2 >= T, and 16, at most 4096 --, kept after the sweep in profiles/parallel_smoother_probe.txt (n = 4): at B = 1, T = 10^6
// the rule's L = 142 takes 0.833 ms (predictions given) / 0.750 ms (recomputed) where the best swept L takes 0.749 ms (L = 64) /
// 0.703 ms (L = 128), L = 16 takes 1.985 / 1.873 ms and L = 1024 4.192 / 3.855 ms; at B = 64, T = 10^5 the rule's L = 98 is the
// fastest recomputed and 5 % behind L = 256 given; at B = 1024, T = 10^4 its L = 157 is 23 % / 8 % behind the best fixed L.  The
// combination has no solve, so the optimum sits somewhat below the filter's; at these margins one rule for both passes (one
// workspace for parallel_kalman_smoother) is worth more than a second formula.  DESIGN.md, section 6i.

// 4 B ceil(T / L) (3 n^2 + 2 n) bytes: per (trajectory, block) one span (2 n^2 + n floats) and one start state (n^2 + n)
long long rts_pscan_workspace_bytes(int n, long long B, long long T, int block) {
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  const int rc = pscan_check_n(NAME, n);
  if (rc != BF_OK) return rc;
  const int L = resolve_block(NAME, g_prs_block, block, kf_pscan_default_block(B, T));
  if (L < 0) return L;
  const long long NB = pscan_blocks(NAME, B, 0, T, L);
  return NB < 0 ? NB : 4LL * B * NB * (3LL * n * n + 2LL * n);
}

int launch_rts_pscan(const bf_lgssm* model, const bf_out_desc* filtered, long long B, long long T, const bf_smooth_carry* carry,
                     const bf_smooth_desc* out, void* workspace, long long workspace_bytes, hipStream_t stream) {
  if (!model || !filtered || !out || !workspace) return set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  int rc = backward_check_lgssm(model);
  if (rc != BF_OK || (rc = pscan_check_n(NAME, model->n)) != BF_OK) return rc;
  if (model->Q_steps > 1)
    return set_error(BF_EUNSUPPORTED, "parallel rts smoother: constant Q only (Q_steps=%d)", model->Q_steps);
  const bool has_pm = filtered->pred_means.ptr != nullptr, has_pP = filtered->pred_covs.ptr != nullptr;
  if (has_pm != has_pP) return set_error(BF_EINVAL, "pred_means and pred_covs are given together or not at all");
  const bool recompute = !has_pm;
  if (recompute && (rc = backward_check_recompute(model, T)) != BF_OK) return rc;
  RtsViews v;
  if ((rc = rts_views(filtered, carry, out, nullptr, false, v)) != BF_OK) return rc;
  const int L = resolve_block(NAME, g_prs_block, 0, kf_pscan_default_block(B, T));
  if (L < 0) return L;
  const long long need = rts_pscan_workspace_bytes(model->n, B, T, L);
  if (need < 0) return (int)need;
  if ((rc = pscan_check_workspace(NAME, "bf_rts_pscan_workspace_bytes", workspace, workspace_bytes, need, B, T, 0, L)) != BF_OK)
    return rc;

  BackwardRoute r;
  if ((rc = backward_route(model, recompute, r)) != BF_OK) return rc;
  RtsPscanGroup* const groups[] = {launch_rts_pscan_group_a, launch_rts_pscan_group_b, launch_rts_pscan_group_c,
                                   launch_rts_pscan_group_d};
  bool matched;
  rc = run_groups(groups, std::size(groups), &matched, r, v, B, T, static_cast<float*>(workspace), L, stream);
  if (matched) return rc;
  return set_error(BF_EUNSUPPORTED, "parallel rts smoother: n=%d is not compiled in", model->n);
}

}  // namespace bf

extern "C" {

int64_t bf_rts_pscan_workspace_bytes(int32_t n, int64_t B, int64_t T, int32_t block) {
  return bf::rts_pscan_workspace_bytes(n, B, T, block);
}

int bf_rts_smoother_pscan_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T,
                              const bf_smooth_carry* carry, const bf_smooth_desc* out, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  bf::CallOptionScope call_option_scope;
  return bf::launch_rts_pscan(model, filtered, B, T, carry, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
