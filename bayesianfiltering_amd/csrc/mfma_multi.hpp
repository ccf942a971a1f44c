// What the two matrix-core launchers (kf_scan_mfma.hip, kf_scan_bf32.hip) share beyond the model packing: the weight pass of
// a Gaussian-sum launch and the per-step covariance tables.  Defined once, in mfma_multi.hip.
#pragma once
#include "bf_common.hpp"

namespace bf {

// MULTI launches: the per-step log-likelihoods go to the caller's stream when there is one, else to a stream-ordered scratch
// [B][K][T] (freed by finish_multi after the weight pass, gsf_reweight_kernel)
int begin_multi(long long B, long long T, int K, hipStream_t stream, OutViews& ov, float** scratch);
int finish_multi(const OutViews& ov, const bf_carry* carry, long long B, long long T, int K, hipStream_t stream, float* scratch);

// out[t] = W C_t W^T, zero-padded into NP x NP with diag_from .. NP - 1 set to 1, formed on the device (tv_table_kernel).
// d_out: a stream-ordered allocation the caller frees with hipFreeAsync after its launch
int tv_table_on_device(const float* W_host, const float* C_host, long long T, int rows, int d, int NP, int diag_from,
                       hipStream_t stream, float** d_out);

}  // namespace bf
