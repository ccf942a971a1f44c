// Host side of the parallel-in-time posterior sampler (ffbs_pscan.hpp): its two C entry points, the argument checks (all before
// the first HIP call), block geometry, workspace size, and the dispatch over the compiled table n = 1 ... 6 x {predictions given,
// recomputed} x SPL = 1, 2, 4 samples per lane (instantiations: ffbs_pscan_group_{a,...,e}.hip).  The model validation and the
// route's constants are the backward family's (backward_host.hpp), the views and their checks the serial sampler's (ffbs_views).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance of the three kernels, n = 1 ... 6,
// both routes, SPL = 1, 2, 4, builds without scratch.  Table per instance: DESIGN.md, section 6j.  n <= 6 is the parallel
// filter's limit (kf_pscan.hip), whose streams this pass samples from.
#include "backward_host.hpp"
#include "pscan_host.hpp"

namespace bf {

using FfbsPscanGroup = int(const BackwardRoute& r, const FfbsViews& v, long long B, long long T, int S, int spl, float* workspace,
                           int L, hipStream_t stream, bool* matched);
FfbsPscanGroup launch_ffbs_pscan_group_a, launch_ffbs_pscan_group_b, launch_ffbs_pscan_group_c, launch_ffbs_pscan_group_d,
    launch_ffbs_pscan_group_e;

static const char NAME[] = "parallel sampler";
constexpr int PFS_SPL_MAX = 4;

static Option g_pfs_block{0, OPT_PFS_BLOCK};   // 0 = from (B, S, T)
Option& pfs_block_option() { return g_pfs_block; }

// Default block length: the largest of ceil(B ceil(S / 4) T / 65 536), the smallest s with 250 s^2 >= T, and 16; at most
// 4096.  It started as the parallel filter's rule (kf_pscan.hip) applied to (B S, T) and was CHANGED after the sweep in
// profiles/parallel_sampler_probe.txt (n = 4; its rows marked *), where that rule's L = 142 at (B, S, T) = (1, 1, 10^6)
// takes 0.636 ms (predictions given) / 0.573 ms (recomputed) against 0.465 / 0.454 ms at L = 64; L = 245 at (1, 16, 10^6):
// 2.659 / 2.573 ms against 1.666 / 1.458 ms at L = 64; L = 391 at (64, 4, 10^5): 4.549 / 4.426 ms against 2.750 / 2.309 ms
// at L = 98; L = 625 at (1024, 4, 10^4): 7.664 / 7.526 ms against 4.586 / 3.880 ms at L = 157 (the second figures are this
// rule's).  Two reasons: the lanes of fold and emit are (trajectory, block, block of up to four samples), not (trajectory,
// block, sample), so the first term counts B ceil(S / 4); and a span is n^2 + n floats with one product to combine, so the
// scan is cheaper against a lane's step than the filter's and the balance sits at sqrt(T / 250) (64 at T = 10^6), not
// sqrt(T / 50).  The count is that of the default samples per lane whatever "ffbs_spl" says: the block length, and with it
// a sample's bits, must not depend on that option.  DESIGN.md, section 6j.
static int default_block(long long B, int S, long long T) {
  return pscan_default_block(B * ((S + PFS_SPL_MAX - 1) / PFS_SPL_MAX), T, 250);
}

// 4 B ceil(T / L) (n^2 + 2 S n) bytes: per (trajectory, block) E (n^2 floats) and, per sample, g and the start sample (n each)
long long ffbs_pscan_workspace_bytes(int n, long long B, long long T, int S, int block) {
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  if (S <= 0) return set_error(BF_EINVAL, "the number of samples S must be positive (S=%d)", S);
  const int rc = pscan_check_n(NAME, n);
  if (rc != BF_OK) return rc;
  const int L = resolve_block(NAME, g_pfs_block, block, default_block(B, S, T));
  if (L < 0) return L;
  const long long NB = pscan_blocks(NAME, B, S, T, L);
  return NB < 0 ? NB : 4LL * B * NB * ((long long)n * n + 2LL * S * n);
}

// samples per lane: option "ffbs_spl" where it names a count compiled here, else the smallest compiled count that holds all S
// samples of a trajectory in one lane, 4 for S > 4
static int resolve_spl(int S, int* spl) {
  const int forced = ffbs_spl_option().load();
  if (forced != 0 && forced != 1 && forced != 2 && forced != 4)
    return set_error(BF_EINVAL, "parallel sampler: ffbs_spl must be 0 or one of the compiled counts 1, 2, 4");
  int s = forced;
  if (s == 0) {
    s = 1;
    while (s < PFS_SPL_MAX && s < S) s *= 2;
  }
  *spl = s;
  return BF_OK;
}

int launch_ffbs_pscan(const bf_lgssm* model, const bf_out_desc* filtered, long long B, long long T, int S, const bf_sample_carry* carry,
                      const bf_sample_desc* out, void* workspace, long long workspace_bytes, hipStream_t stream) {
  if (!model || !filtered || !out || !workspace) return set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  if (S <= 0) return set_error(BF_EINVAL, "the number of samples S must be positive (S=%d)", S);
  int rc = backward_check_lgssm(model);
  if (rc != BF_OK || (rc = pscan_check_n(NAME, model->n)) != BF_OK) return rc;
  if (model->Q_steps > 1)
    return set_error(BF_EUNSUPPORTED, "parallel sampler: constant Q only (Q_steps=%d)", model->Q_steps);
  FfbsViews v;
  if ((rc = ffbs_views(filtered, carry, out, nullptr, B, T, S, model->n, false, v)) != BF_OK) return rc;
  if (out->noise.ptr && out->keys) return set_error(BF_EINVAL, "parallel sampler: give the noise stream or the keys, not both");
  const bool recompute = v.pm.p == nullptr;
  if (recompute && (rc = backward_check_recompute(model, T)) != BF_OK) return rc;
  int spl;
  if ((rc = resolve_spl(S, &spl)) != BF_OK) return rc;
  const int L = resolve_block(NAME, g_pfs_block, 0, default_block(B, S, T));
  if (L < 0) return L;
  const long long need = ffbs_pscan_workspace_bytes(model->n, B, T, S, L);
  if (need < 0) return (int)need;
  if ((rc = pscan_check_workspace(NAME, "bf_ffbs_pscan_workspace_bytes", workspace, workspace_bytes, need, B, T, S, L)) != BF_OK)
    return rc;

  BackwardRoute r;
  if ((rc = backward_route(model, recompute, r)) != BF_OK) return rc;
  FfbsPscanGroup* const groups[] = {launch_ffbs_pscan_group_a, launch_ffbs_pscan_group_b, launch_ffbs_pscan_group_c,
                                    launch_ffbs_pscan_group_d, launch_ffbs_pscan_group_e};
  bool matched;
  rc = run_groups(groups, std::size(groups), &matched, r, v, B, T, S, spl, static_cast<float*>(workspace), L, stream);
  if (matched) return rc;
  return set_error(BF_EUNSUPPORTED, "parallel sampler: n=%d is not compiled in", model->n);
}

}  // namespace bf

extern "C" {

int64_t bf_ffbs_pscan_workspace_bytes(int32_t n, int64_t B, int64_t T, int32_t S, int32_t block) {
  return bf::ffbs_pscan_workspace_bytes(n, B, T, S, block);
}

int bf_ffbs_sample_pscan_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T, int32_t S,
                             const bf_sample_carry* carry, const bf_sample_desc* out, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  bf::CallOptionScope call_option_scope;
  return bf::launch_ffbs_pscan(model, filtered, B, T, S, carry, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
