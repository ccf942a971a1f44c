// Host side the three parallel-in-time passes share (kf_pscan.hip, rts_pscan.hip, ffbs_pscan.hip and the launch templates of
// their headers): the limits, the block length, the block count, the workspace refusals and the launch geometry (the walk
// over the group translation units is run_groups, bf_common.hpp).  `name` is the family's display name, the head of every message ("parallel kalman filter",
// "parallel rts smoother", "parallel sampler"); S = 0 stands for a family without samples, and the texts then leave S out.
#pragma once
#include <cstddef>
#include "bf_common.hpp"

namespace bf {

// Register kernels for n = 1 ... 6: the filter's scan holds two spans of 3 n^2 + 2 n floats in a combination and needs scratch
// from n = 7 (kf_pscan.hip); the smoother and the sampler read the filter's streams and keep its limit.
constexpr int PSCAN_N_MAX = 6;
constexpr int PSCAN_L_MIN = 4, PSCAN_L_MAX = 4096;   // the block length, and what "pkf_block" / "prs_block" / "pfs_block" take

// Default block length, the largest of
//   ceil(lanes_per_step T / 65 536)   as many fold / emit lanes as fill the device once (256 CUs x 4 SIMDs x 64 lanes),
//   s, balance s^2 >= T               where the scan's time per block meets a lane's time per step: L = sqrt(T / balance),
//   16                                so that a block's span stays a small fraction of its streams,
// and at most PSCAN_L_MAX.  The families' constants and the measurements behind them: kf_pscan.hip, ffbs_pscan.hip.
inline int pscan_default_block(long long lanes_per_step, long long T, int balance) {
  const long long device_lanes = 256LL * 4 * 64;
  long long L = (lanes_per_step * T + device_lanes - 1) / device_lanes;
  long long s = 1;
  while (balance * s * s < T && s < PSCAN_L_MAX) ++s;
  if (L < s) L = s;
  if (L < 16) L = 16;
  if (L > PSCAN_L_MAX) L = PSCAN_L_MAX;
  return (int)L;
}
int kf_pscan_default_block(long long B, long long T);   // kf_pscan.hip: the filter's rule, which the smoother keeps

// the smoother's and the sampler's state dimension
inline int pscan_check_n(const char* name, int n) {
  if (n <= 0) return set_error(BF_EINVAL, "non-positive model dimension");
  if (n > PSCAN_N_MAX)
    return set_error(BF_EUNSUPPORTED, "%s: n=%d is not compiled in (register kernels for n = 1..%d, the parallel filter's limit)", name, n,
                     PSCAN_N_MAX);
  return BF_OK;
}

// `block` = 0: the family's call option, else `fallback`, its default for the call's sizes.  < 0: BF_E* (text set).
inline int resolve_block(const char* name, const Option& option, int block, int fallback) {
  if (block == 0) block = option.load();
  if (block == 0) return fallback;
  if (block < PSCAN_L_MIN || block > PSCAN_L_MAX)
    return set_error(BF_EINVAL, "%s: block length %d is outside %d..%d", name, block, PSCAN_L_MIN, PSCAN_L_MAX);
  return block;
}

// NB = ceil(T / L); the lanes' columns B * NB (B * S * NB with samples) are 32-bit grid material.  < 0: BF_E* (text set).
inline long long pscan_blocks(const char* name, long long B, int S, long long T, int L) {
  const long long NB = (T + L - 1) / L;
  if ((double)B * (double)(S ? S : 1) * (double)NB < 2147483648.0) return NB;
  if (S) return set_error(BF_EINVAL, "%s: B * S * ceil(T / block) = %lld * %d * %lld must stay below 2^31", name, B, S, NB);
  return set_error(BF_EINVAL, "%s: B * ceil(T / block) = %lld * %lld must stay below 2^31", name, B, NB);
}

// the caller's workspace against `need`, the result of `bytes_fn` (the family's bf_*_pscan_workspace_bytes) for these sizes
inline int pscan_check_workspace(const char* name, const char* bytes_fn, const void* workspace, long long workspace_bytes,
                                 long long need, long long B, long long T, int S, int L) {
  if (workspace_bytes < need) {
    char samples[32] = "";
    if (S) std::snprintf(samples, sizeof(samples), " S=%d,", S);
    return set_error(BF_EINVAL, "%s: workspace of %lld bytes is too small: B=%lld, T=%lld,%s block=%d need %lld bytes (%s)", name,
                     workspace_bytes, B, T, samples, L, need, bytes_fn);
  }
  if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return set_error(BF_EINVAL, "%s: workspace must be 4-byte aligned", name);
  return BF_OK;
}

// The three launches' geometry: fold and emit run `lanes` = B NSB NB lanes in `grid` workgroups of 64 (NSB = 1 without
// samples); the scan runs one workgroup of `scan_threads` per trajectory or sample over NB - 1 spans, and only if NB > 1.
struct PscanGeom {
  long long NB, lanes;
  unsigned grid, scan_threads;
};
inline PscanGeom pscan_geom(long long B, long long NSB, long long T, int L) {
  PscanGeom g;
  g.NB = (T + L - 1) / L;
  g.lanes = B * NSB * g.NB;   // < 2^31 (pscan_blocks)
  g.grid = (unsigned)((g.lanes + 63) / 64);
  g.scan_threads = g.NB - 1 <= 64 ? 64 : 256;
  return g;
}

}  // namespace bf
