// Host side of the Gaussian-sum backward passes' register instances (rts_gs_reg_kernel, rts_smoother.hpp; ffbs_gs_reg_kernel,
// ffbs_sampler.hpp): one launch function per (n, route) and product, defined by explicit instantiation in gs_group_a.hip
// (extended registry route) and gs_group_b.hip (unscented route) so that the instances build in parallel; gs_smoother.hip and
// gs_sampler.hip hold the entry points and everything else.
#pragma once
#include "backward_host.hpp"

namespace bf {

// lanes per trajectory of the fused kernel: the power of two >= K
inline int gs_lanes(int K) {
  int kp = 1;
  while (kp < K) kp <<= 1;
  return kp;
}
// The fused collapsed moments serve K <= 64 (one wave holds a trajectory's chains) and n <= 6: at n = 7 and 8 the fused
// instances do not build without scratch (the table in gs_smoother.hip), so they are not compiled and not offered.
enum { GS_FUSED_KMAX = 64, GS_FUSED_NMAX = 6 };
inline bool gs_fused_ok(int n, long long K) { return n <= GS_FUSED_NMAX && K <= GS_FUSED_KMAX; }

// `out`: GS_COMP, GS_COLL or both.  The grid: 64 chains per workgroup (GS_COMP alone), 64 / KP trajectories otherwise.
inline int gs_reg_grid(const RtsGsViews& gv, int out, long long B, unsigned* grid) {
  const long long blocks = (out & GS_COLL) ? (B + 64 / gv.KP - 1) / (64 / gv.KP) : (B * gv.K + 63) / 64;
  if (blocks > 0x7fffffffLL) return set_error(BF_EINVAL, "Gaussian-sum smoother: B x K too large for one launch");
  *grid = (unsigned)blocks;
  return BF_OK;
}

template <int N, int KIND, class Arg>
int gs_rts_launch(const Arg& c, int out, const RtsGsViews& gv, long long B, long long T, hipStream_t stream);

#define BF_GS_RTS_LAUNCH_DEFINE                                                                                              \
  template <int N, int KIND, class Arg>                                                                                      \
  int gs_rts_launch(const Arg& c, int out, const RtsGsViews& gv, long long B, long long T, hipStream_t stream) {             \
    unsigned grid;                                                                                                           \
    const int rc = gs_reg_grid(gv, out, B, &grid);                                                                           \
    if (rc != BF_OK) return rc;                                                                                              \
    if (out == GS_COMP) {                                                                                                    \
      hipLaunchKernelGGL((rts_gs_reg_kernel<N, KIND, GS_COMP, Arg>), dim3(grid), dim3(64), 0, stream, c, gv, B, T);          \
    } else if constexpr (N <= GS_FUSED_NMAX) {                                                                               \
      if (out == GS_COLL) hipLaunchKernelGGL((rts_gs_reg_kernel<N, KIND, GS_COLL, Arg>), dim3(grid), dim3(64), 0, stream, c, gv, B, T); \
      else hipLaunchKernelGGL((rts_gs_reg_kernel<N, KIND, GS_COMP | GS_COLL, Arg>), dim3(grid), dim3(64), 0, stream, c, gv, B, T); \
    } else {                                                                                                                 \
      return set_error(BF_EUNSUPPORTED, "Gaussian-sum smoother: no fused instance for n = %d", N);                           \
    }                                                                                                                        \
    BF_HIP_CHECK(hipGetLastError());                                                                                         \
    return BF_OK;                                                                                                            \
  }

template <int N, int KIND, class Arg>
int gs_ffbs_launch(const Arg& c, const FfbsViews& v, const GsDraw& gd, long long B, long long T, int S, hipStream_t stream);

#define BF_GS_FFBS_LAUNCH_DEFINE                                                                                             \
  template <int N, int KIND, class Arg>                                                                                      \
  int gs_ffbs_launch(const Arg& c, const FfbsViews& v, const GsDraw& gd, long long B, long long T, int S, hipStream_t stream) { \
    const long long blocks = (B * S + 63) / 64;                                                                              \
    if (blocks > 0x7fffffffLL) return set_error(BF_EINVAL, "Gaussian-sum sampler: B x S too large for one launch");          \
    hipLaunchKernelGGL((ffbs_gs_reg_kernel<N, KIND, Arg>), dim3((unsigned)blocks), dim3(64), 0, stream, c, v, gd, B, T, S);  \
    BF_HIP_CHECK(hipGetLastError());                                                                                         \
    return BF_OK;                                                                                                            \
  }

}  // namespace bf
