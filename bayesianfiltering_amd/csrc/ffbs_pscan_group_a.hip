// Instantiations of the parallel-in-time posterior sampler's kernels (ffbs_pscan.hpp) for a slice of the table n = 1 ... 6 x both
// routes, SPL = 1, 2, 4 each; split over several translation units to build in parallel.
#include "backward_host.hpp"
#include "ffbs_pscan.hpp"

namespace bf {

int launch_ffbs_pscan_group_a(const BackwardRoute& r, const FfbsViews& v, long long B, long long T, int S, int spl, float* workspace,
        int L, hipStream_t stream, bool* matched) {
#define BF_CASE(N_)                                                                                                            \
  if (r.n == N_) {                                                                                                             \
    *matched = true;                                                                                                           \
    if (r.kind == RTS_LIN) return launch_ffbs_pscan_n<N_, RTS_LIN>(rts_lin_arg<N_>(r), v, B, T, S, spl, workspace, L, stream); \
    return launch_ffbs_pscan_n<N_, RTS_LIN_RECOMPUTE>(rts_lin_arg<N_>(r), v, B, T, S, spl, workspace, L, stream);              \
  }
  BF_CASE(1);
  BF_CASE(2);
  BF_CASE(3);
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
