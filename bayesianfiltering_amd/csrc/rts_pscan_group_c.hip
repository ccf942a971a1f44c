// Instantiations of the parallel-in-time RTS smoother's kernels (rts_pscan.hpp) for a slice of the table n = 1 ... 6, both routes
// each; split over several translation units to build in parallel.
#include "backward_host.hpp"
#include "rts_pscan.hpp"

namespace bf {

int launch_rts_pscan_group_c(const BackwardRoute& r, const RtsViews& v, long long B, long long T, float* workspace, int L,
        hipStream_t stream, bool* matched) {
#define BF_CASE(N_)                                                                                              \
  if (r.n == N_) {                                                                                               \
    *matched = true;                                                                                             \
    if (r.kind == RTS_LIN) return launch_rts_pscan_n<N_, RTS_LIN>(rts_lin_arg<N_>(r), v, B, T, workspace, L, stream); \
    return launch_rts_pscan_n<N_, RTS_LIN_RECOMPUTE>(rts_lin_arg<N_>(r), v, B, T, workspace, L, stream);        \
  }
  BF_CASE(5);
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
