// sample_ssm: synthetic trajectories of a registry state-space model on the device.
//
// Replaces NonlinearSSM.sample (gaussfiltax/models.py:240-289): split the key three ways, draw
// z_1 ~ N(m0, P0) and r_1, then for t >= 2 draw (q_t, r_t) with the two halves of
// split(next_keys[t-1]) and apply f, h -- the step before the filtering path in every
// experiment script (docs/experiments/BOT_Experiment_script.py:95).  One lane per trajectory
// (the recursion is sequential in t); all randomness is per-lane Threefry with JAX's layout, so
// trajectory b depends only on keys[b].
#include <cstring>
#include <vector>
#include "sample_ssm.hpp"
#include "user_model.hpp"

namespace bf {

// Launch preparation, shared by the compiled instances and the kernel built at run time: one constant block
// [BpfModel<N, DQ, M> words][EmissionNoise<M>: 4 ints, Dm (M x M), LRn (M x M), r0 (M)].  user_flags: bit 0 = dynamics, bit 1 =
// emission from the caller's source.
static int prepare_sample(const bf_bpf_model* bp, int user_flags, hipStream_t stream, const void** d_mdl, const void** d_en) {
  const bf_model* p = &bp->ssm;
  const int N = p->n, DQ = p->dq, M = p->m;
  if (p->dr != M) return set_error(BF_EUNSUPPORTED, "sample_ssm: emission noise dimension must equal the emission dimension");
  const size_t mw = bpf_model_words(N, DQ, M), ew = 4 + 2 * (size_t)M * M + M;
  std::vector<uint32_t> words(mw + ew, 0u);   // zeroed: the constant cache compares contents
  const BpfModelView view = bpf_model_view_flat(words.data(), N, DQ, M);
  // reuse the particle-filter model fill with the emission-noise covariance standing in for the
  // log-density covariance and r_eval = 0; the stochastic-volatility emission is evaluated here
  bf_bpf_model tmp = *bp;
  tmp.lp_cov = p->R;
  tmp.r_eval = nullptr;
  const bool sv = !(user_flags & 2) && p->emi_id == EMI_STOCH_VOL;
  int rc;
  if (sv) {
    // fill the dynamics side through a linear-emission placeholder of the right shape
    std::vector<float> zeros((size_t)M * N + (size_t)M * M, 0.f);
    for (int i = 0; i < M; ++i) zeros[(size_t)M * N + i * M + i] = 1.f;
    tmp.ssm.emi_id = EMI_LINEAR;
    tmp.ssm.emi_theta = zeros.data();
    tmp.ssm.n_emi_theta = M * N + M * M;
    rc = fill_bpf_model_view(&tmp, view, user_flags, nullptr, 0);
    if (rc == BF_OK) {
      if (p->n_emi_theta != 3 || M != N) return set_error(BF_EINVAL, "stoch_vol: m = n, theta = (sigma, beta, c)");
      *view.emi_id = EMI_STOCH_VOL;
      for (int i = 0; i < 3; ++i) view.eth[i] = p->emi_theta[i];
    }
  } else {
    rc = fill_bpf_model_view(&tmp, view, user_flags, nullptr, 0);
  }
  if (rc != BF_OK) return rc;
  int* ei = reinterpret_cast<int*>(words.data() + mw);   // d_identity, emi_sv, two pads
  float* ef = reinterpret_cast<float*>(words.data() + mw + 4);
  ei[0] = 1;
  ei[1] = sv ? 1 : 0;
  if (!(user_flags & 2) && p->emi_id == EMI_LINEAR) {
    ei[0] = 0;
    for (int i = 0; i < M * M; ++i) ef[i] = p->emi_theta[M * N + i];
  }
  for (int i = 0; i < M * M; ++i) ef[M * M + i] = view.LR[i];
  for (int i = 0; i < M; ++i) ef[2 * M * M + i] = p->r0 ? p->r0[i] : 0.f;
  rc = device_constants(words.data(), sizeof(uint32_t) * words.size(), stream, d_mdl);
  if (rc != BF_OK) return rc;
  *d_en = static_cast<const uint32_t*>(*d_mdl) + mw;
  return BF_OK;
}

template <int N, int DQ, int M>
static int launch_sample_dims(const bf_bpf_model* bp, const uint32_t* d_keys, const bf_cstream* u, long long B, long long T,
                              float* d_states, float* d_emis, hipStream_t stream) {
  static_assert(sizeof(BpfModel<N, DQ, M>) == 4 * bpf_model_words(N, DQ, M) && sizeof(EmissionNoise<M>) == 4 * (4 + 2 * M * M + M),
                "BpfModel / EmissionNoise: 4-byte members in declaration order, no padding");
  const void *d_mdl = nullptr, *d_en = nullptr;
  const int rc = prepare_sample(bp, 0, stream, &d_mdl, &d_en);
  if (rc != BF_OK) return rc;
  hipLaunchKernelGGL((sample_ssm_kernel<N, DQ, M>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, static_cast<const BpfModel<N, DQ, M>*>(d_mdl),
                     static_cast<const EmissionNoise<M>*>(d_en), d_keys, (u && u->ptr) ? u->ptr : nullptr, u ? u->sB : 0, u ? u->sT : 0, d_states,
                     d_emis, B, T);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

// NonlinearSSM.sample with the caller's f(x, q, u) / h(x, r, u): sample_ssm.hpp compiled around them at run time (user_model.hpp)
static int launch_sample_user_impl(const bf_bpf_model* bp, const uint32_t* d_keys, const bf_cstream* u, long long B, long long T, float* d_states,
                                   float* d_emis, hipStream_t stream) {
  const bf_model* p = &bp->ssm;
  int rc = check_user_model(p->user, p);
  if (rc != BF_OK) return rc;
  if (p->dr != p->m) return set_error(BF_EUNSUPPORTED, "sample_ssm: emission noise dimension must equal the emission dimension");
  if (p->n > 32 || p->dq > 32 || p->m > 32) return set_error(BF_EUNSUPPORTED, "sample_ssm with functions from source: dimensions up to 32 (a trajectory's state lives in registers)");
  if (!p->user->has_emi && p->emi_id == EMI_STOCH_VOL)
    return set_error(BF_EUNSUPPORTED, "sample_ssm: the stochastic-volatility emission beside a dynamics function from source is not built; give h as source too");
  hipFunction_t fn = nullptr;
  if ((rc = user_kernel(p->user, JIT_SAMPLE, 0, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
  const void *d_mdl = nullptr, *d_en = nullptr;
  if ((rc = prepare_sample(bp, p->user->user_flags() & 3, stream, &d_mdl, &d_en)) != BF_OK) return rc;
  const float* uptr = (u && u->ptr) ? u->ptr : nullptr;
  long long u_sB = u ? u->sB : 0, u_sT = u ? u->sT : 0;
  void* args[] = {&d_mdl, &d_en, &d_keys, &uptr, &u_sB, &u_sT, &d_states, &d_emis, &B, &T};
  BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)((B + 63) / 64), 1, 1, 64, 1, 1, 0, stream, args, nullptr));
  return BF_OK;
}

int launch_sample_generic(const bf_bpf_model* bp, const uint32_t* d_keys, const bf_cstream* u, long long B, long long T,
                          float* d_states, float* d_emis, hipStream_t stream);

int launch_sample_ssm(const bf_bpf_model* bp, const uint32_t* d_keys, const bf_cstream* u, long long B, long long T,
                      float* d_states, float* d_emis, hipStream_t stream) {
  const bf_model* p = &bp->ssm;
  if (p->user)   // functions from the caller's source: the same kernel compiled at run time around them
    return launch_sample_user_impl(bp, d_keys, u, B, T, d_states, d_emis, stream);
#define BF_CASE(N_, DQ_, M_) \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_ && p->dr == M_) return launch_sample_dims<N_, DQ_, M_>(bp, d_keys, u, B, T, d_states, d_emis, stream)
  BF_CASE(1, 1, 1);
  BF_CASE(2, 2, 1);
  BF_CASE(2, 2, 2);
  BF_CASE(3, 3, 1);
  BF_CASE(3, 3, 3);
  BF_CASE(4, 4, 1);
  BF_CASE(4, 4, 2);
  BF_CASE(4, 2, 2);
  BF_CASE(4, 2, 1);
  BF_CASE(6, 6, 3);
  BF_CASE(8, 8, 4);
  BF_CASE(16, 16, 8);
  BF_CASE(4, 4, 4);
#undef BF_CASE
  // any other shape: the run-time-dimension kernel (generic_scan.hip), one wave per trajectory
  return launch_sample_generic(bp, d_keys, u, B, T, d_states, d_emis, stream);
}

}  // namespace bf
