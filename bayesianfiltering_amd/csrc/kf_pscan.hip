// Host side of the parallel-in-time Kalman filter (kf_pscan.hpp): argument checks (all before the first HIP call), block
// geometry, workspace size, and the dispatch over the compiled (n, m) table (instantiations: kf_pscan_group_{a,...,f}.hip).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance n = 1 ... 6, m = 1 ... 4 of the
// three kernels builds without scratch; at n = 7 the scan kernel spills 860 bytes per lane (n = 8: fold 436, scan 1628), so
// the limit is n = 6.  Table per instance: DESIGN.md, section 6h.
#include "forward_host.hpp"

namespace bf {

#define BF_DECL(F_)                                                                                                     \
  int F_(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry, const bf_out_desc* out, \
         float* workspace, int L, hipStream_t stream, bool* matched)
BF_DECL(launch_kf_pscan_group_a);
BF_DECL(launch_kf_pscan_group_b);
BF_DECL(launch_kf_pscan_group_c);
BF_DECL(launch_kf_pscan_group_d);
BF_DECL(launch_kf_pscan_group_e);
BF_DECL(launch_kf_pscan_group_f);
#undef BF_DECL

constexpr int PSCAN_N_MAX = 6;   // register kernels: the scan's combination (two spans of 3 n^2 + 2 n floats) needs scratch from n = 7
constexpr int PSCAN_M_MAX = 4;
constexpr int PSCAN_L_MIN = 4, PSCAN_L_MAX = 4096;

static Option g_pkf_block{0, OPT_PKF_BLOCK};   // 0 = from (B, T)
Option& pkf_block_option() { return g_pkf_block; }

// Default block length, from the measurements in profiles/parallel_kalman_probe.txt (n = 4, m = 2): the largest of
//   ceil(B T / 65 536)  as many (trajectory, block) lanes as fill the device once (256 CUs x 4 SIMDs x 64 lanes),
//   s, 50 s^2 >= T      the scan is one workgroup per trajectory and costs about 80 ns per block, a lane's fold and emit about
//                       4 us per step: T / L * 80 ns + L * 4 us is smallest at L = sqrt(T / 50) (B = 1, T = 10^6: 1.6 ms at
//                       L = 64 ... 256 against 5.1 ms at L = 16),
//   16                  so that the fold's aggregate (56 floats at n = 4) stays a small fraction of a block's streams.
int kf_pscan_default_block(long long B, long long T) {
  const long long device_lanes = 256LL * 4 * 64;
  long long L = (B * T + device_lanes - 1) / device_lanes;
  long long s = 1;
  while (50 * s * s < T && s < PSCAN_L_MAX) ++s;
  if (L < s) L = s;
  if (L < 16) L = 16;
  if (L > PSCAN_L_MAX) L = PSCAN_L_MAX;
  return (int)L;
}

// `block` = 0: the call option "pkf_block", else the default for (B, T).  < 0: BF_E* (text set).
static int resolve_block(long long B, long long T, int block) {
  if (block == 0) block = g_pkf_block.load();
  if (block == 0) return kf_pscan_default_block(B, T);
  if (block < PSCAN_L_MIN || block > PSCAN_L_MAX)
    return set_error(BF_EINVAL, "parallel kalman filter: block length %d is outside %d..%d", block, PSCAN_L_MIN, PSCAN_L_MAX);
  return block;
}

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
  const int L = resolve_block(B, T, block);
  if (L < 0) return L;
  const long long NB = (T + L - 1) / L;
  if ((double)B * (double)NB >= 2147483648.0)
    return set_error(BF_EINVAL, "parallel kalman filter: B * ceil(T / block) = %lld * %lld must stay below 2^31", B, NB);
  return 4LL * B * NB * (4LL * n * n + 3LL * n);
}

int launch_kf_pscan(const bf_lgssm* model, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, void* workspace, long long workspace_bytes, hipStream_t stream) {
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
  const int L = resolve_block(B, T, 0);
  if (L < 0) return L;
  const long long need = kf_pscan_workspace_bytes(model->n, model->m, B, T, L);
  if (need < 0) return (int)need;
  if (workspace_bytes < need)
    return set_error(BF_EINVAL, "parallel kalman filter: workspace of %lld bytes is too small: B=%lld, T=%lld, block=%d need %lld bytes (bf_kalman_pscan_workspace_bytes)",
                     workspace_bytes, B, T, L, need);
  if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return set_error(BF_EINVAL, "parallel kalman filter: workspace must be 4-byte aligned");

  float* ws = static_cast<float*>(workspace);
  bool matched = false;
  int r = launch_kf_pscan_group_a(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  r = launch_kf_pscan_group_b(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  r = launch_kf_pscan_group_c(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  r = launch_kf_pscan_group_d(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  r = launch_kf_pscan_group_e(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  r = launch_kf_pscan_group_f(model, y, B, T, carry, out, ws, L, stream, &matched);
  if (matched) return r;
  return set_error(BF_EUNSUPPORTED, "parallel kalman filter: (n=%d, m=%d) is not compiled in", model->n, model->m);
}

}  // namespace bf
