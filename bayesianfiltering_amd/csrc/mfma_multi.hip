// The parts of a matrix-core Kalman launch that do not depend on the tile size (mfma_multi.hpp): the weight recursion that
// follows the independent chains of a Gaussian-sum launch, and the per-step covariance tables.
#include "mfma_multi.hpp"
#include "kf_math.hpp"

namespace bf {

// The weight recursion of the Gaussian-sum filter (inference.py:347-350) on stored per-step log-likelihoods: one wave per
// trajectory, component k in lane k (K <= 64), w_t = exp(ll_t - max ll_t) w_{t-1} / sum, the max and the sum as xor-butterflies
// over the lanes = the oracle's adjacent-pair trees (lanes beyond K carry -inf / 0, the trees' identities).
__global__ void __launch_bounds__(64)
gsf_reweight_kernel(SView ll, SView wout, const float* __restrict__ w_in, float* __restrict__ w_out, long long T, int K) {
  const long long b = blockIdx.x;
  const int lane = threadIdx.x;
  float w = lane < K ? (w_in ? w_in[b * K + lane] : 1.0f / (float)K) : 0.f;
  for (long long t = 0; t < T; ++t) {
    const float l = lane < K ? ll.p[b * ll.sB + lane * ll.sK + t * ll.sT] : -__builtin_inff();
    float mx = l;
    BF_UNROLL for (int off = 1; off < 64; off <<= 1) {
      const float o = __shfl_xor(mx, off, 64);
      mx = (mx != mx || o != o) ? __builtin_nanf("") : fmaxf(mx, o);   // jnp.max propagates NaN
    }
    const float e = lane < K ? expf(l - mx) * w : 0.f;
    float tot = e;
    BF_UNROLL for (int off = 1; off < 64; off <<= 1) tot += __shfl_xor(tot, off, 64);
    w = e / tot;
    if (lane < K && wout.p) wout.p[b * wout.sB + lane * wout.sK + t * wout.sT] = w;
  }
  if (w_out && lane < K) w_out[b * K + lane] = w;
}

int begin_multi(long long B, long long T, int K, hipStream_t stream, OutViews& ov, float** scratch) {
  *scratch = nullptr;
  if (!ov.ll.p) {
    BF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(scratch), sizeof(float) * (size_t)B * K * T, stream));
    ov.ll = SView{*scratch, (long long)K * T, T, 1, 1};
  }
  return BF_OK;
}
int finish_multi(const OutViews& ov, const bf_carry* carry, long long B, long long T, int K, hipStream_t stream, float* scratch) {
  hipLaunchKernelGGL(gsf_reweight_kernel, dim3((unsigned)B), dim3(64), 0, stream, ov.ll, ov.w, carry->w_in, carry->w_out, T, K);
  const hipError_t le = hipGetLastError();
  if (scratch) (void)hipFreeAsync(scratch, stream);
  BF_HIP_CHECK(le);
  return BF_OK;
}

// Per-step covariance products for the matrix-core kernels, formed ON THE DEVICE: out[t] = W C_t W^T zero-padded into an
// NP x NP block (W = G, C = Q: n x dq; or W = D, C = R: m x dr), with diag_from .. NP - 1 set to 1 (the unit noise of padded
// observations).  Same association and the same k-ascending fma chains as the host code for constant covariances
// (inference.py:69,:100: (W C) W^T) -- noise_cov in lgssm_pack.hpp is the host twin these loops must match -- so a constant
// table equals the constant block bit for bit.  One workgroup per step.
__global__ void __launch_bounds__(256)
tv_table_kernel(const float* __restrict__ W, const float* __restrict__ C, int rows, int d, int NP, int diag_from, float* __restrict__ out) {
  extern __shared__ float wc[];   // [rows][d]  W C_t
  const float* Ct = C + (size_t)blockIdx.x * d * d;
  float* o = out + (size_t)blockIdx.x * NP * NP;
  for (int e = threadIdx.x; e < rows * d; e += blockDim.x) {
    const int i = e / d, l = e % d;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(W ? W[i * d + k] : (i == k ? 1.f : 0.f), Ct[k * d + l], s);
    wc[e] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NP * NP; e += blockDim.x) {
    const int i = e / NP, j = e % NP;
    float s = 0.f;
    if (i < rows && j < rows) {
      for (int l = 0; l < d; ++l) s = fmaf(wc[i * d + l], W ? W[j * d + l] : (j == l ? 1.f : 0.f), s);
    } else if (i == j && i >= diag_from) {
      s = 1.0f;
    }
    o[e] = s;
  }
}

int tv_table_on_device(const float* W_host, const float* C_host, long long T, int rows, int d, int NP, int diag_from,
                              hipStream_t stream, float** d_out) {
  const void* dW = nullptr;
  const void* dC = nullptr;
  int rc = BF_OK;
  if (W_host && (rc = device_constants(W_host, sizeof(float) * (size_t)rows * d, stream, &dW)) != BF_OK) return rc;
  if ((rc = device_constants(C_host, sizeof(float) * (size_t)T * d * d, stream, &dC)) != BF_OK) return rc;
  BF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(d_out), sizeof(float) * (size_t)T * NP * NP, stream));
  hipLaunchKernelGGL(tv_table_kernel, dim3((unsigned)T), dim3(256), sizeof(float) * (size_t)rows * d, stream,
                     static_cast<const float*>(dW), static_cast<const float*>(dC), rows, d, NP, diag_from, *d_out);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

}  // namespace bf
