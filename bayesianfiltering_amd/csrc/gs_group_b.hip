// Gaussian-sum smoother and sampler, register instances of the unscented route (RTS_UNSC): n = 1 ... 8; the smoother in
// three output sets (gs_smoother.hpp; the resource tables are in gs_smoother.hip and gs_sampler.hip).
#include "gs_smoother.hpp"

namespace bf {

BF_GS_RTS_LAUNCH_DEFINE
BF_GS_FFBS_LAUNCH_DEFINE

#define BF_GS_INST(N_) template int gs_rts_launch<N_, RTS_UNSC, RtsUnsc<N_>>(const RtsUnsc<N_>&, int, const RtsGsViews&, long long, long long, hipStream_t); \
  template int gs_ffbs_launch<N_, RTS_UNSC, RtsUnsc<N_>>(const RtsUnsc<N_>&, const FfbsViews&, const GsDraw&, long long, long long, int, hipStream_t);
BF_GS_INST(1) BF_GS_INST(2) BF_GS_INST(3) BF_GS_INST(4) BF_GS_INST(5) BF_GS_INST(6) BF_GS_INST(7) BF_GS_INST(8)
#undef BF_GS_INST

}  // namespace bf
