// Instances and dispatch of the augmented Gaussian-sum filter kernel with unscented nodes (agsf_scan.hpp), and the launch of
// the same kernel built at run time around functions from source (user_model.hpp).
#include "agsf_scan.hpp"
#include "user_model.hpp"

namespace bf {

// The augmented Gaussian-sum scan (agsf_scan.hpp: a lane per leaf of the [N0, N1, N2] tree) around the caller's functions.
// up != NULL: unscented nodes (speedy_unscented_agsf / unscented_agsf, inference.py:966-1156 / 813-965), either function may
// also come from the registry.  up == NULL: extended-Kalman nodes (inference.py:621-812 / 458-620 / 1157-1300) with the
// Jacobians by dual numbers -- both functions from source (a registry function has its analytic Jacobian in the compiled kernels).
int launch_agsf_user_impl(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                          const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                          int* d_leaf_idx, int variant, hipStream_t stream) {
  const bf_user_model* um = p->user;
  int rc = check_user_model(um, p);
  if (rc != BF_OK) return rc;
  if (um->has_lp) return set_error(BF_EINVAL, "a log-density from source belongs to the particle filter, not to the augmented filter");
  if (!up && !((um->has_dyn || p->dyn_id == DYN_LINEAR) && (um->has_emi || p->emi_id == EMI_LINEAR)))
    return set_error(BF_EUNSUPPORTED, "augmented filter with extended-Kalman nodes: give BOTH functions as source (beside a function from source "
                                      "only the registry's linear one can stand: its Jacobian needs no differentiation)");
  if (p->n > 8 || p->dq > 8 || p->m > 8 || p->dr > 8)
    return set_error(BF_EUNSUPPORTED, "augmented filter with functions from source: dimensions up to 8 (a leaf lives in registers)");
  if (p->flags != 0) return set_error(BF_EUNSUPPORTED, "legacy-class flags do not apply to the augmented filter");
  AgsfLaunch L;
  if ((rc = prepare_agsf(p->n, y, u, B, nc, carry, out, d_leaf_idx, L)) != BF_OK) return rc;
  hipFunction_t fn = nullptr;
  if ((rc = user_kernel(um, up ? JIT_AGSF_UKF : JIT_AGSF_EKF, 0, L.nw, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
  UkfLaunch ML;   // user_flags bit 2: the extended-Kalman nodes take the covariances themselves, not their roots
  if ((rc = prepare_ukf_model(p, up, (um->user_flags() & 3) | (up ? 0 : 4), T, stream, ML)) != BF_OK) return rc;
  int N0 = nc[0], N1 = nc[1], N2 = nc[2];
  float a0 = opt[0], a1 = opt[1];
  uint32_t k0 = key[0], k1 = key[1];
  void* args[] = {&ML.d_mdl, &L.y, &L.u, &L.carry, &L.out, &B, &T, &N0, &N1, &N2, &L.MP, &a0, &a1, &k0, &k1, &variant, &L.carry_records, &ML.d_tvq, &ML.d_tvr};
  BF_HIP_CHECK(hipModuleLaunchKernel(fn, L.grid, 1, 1, (unsigned)L.nt, 1, 1, (unsigned)L.lds_bytes, stream, args, nullptr));
  return BF_OK;
}

int launch_agsf_ukf(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                    const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                    int* d_leaf_idx, int variant, hipStream_t stream) {
  // beyond the registers (or on request), registry functions: the node in turn in LDS (agsf_generic.hip)
  if (agsf_beyond_registers(p) || (!p->user && g_agsf_force_generic.load() != 0))
    return launch_agsf_generic(p, up, y, u, B, T, nc, key, opt, carry, out, d_leaf_idx, variant, stream);
  if (p->user) return launch_agsf_user_impl(p, up, y, u, B, T, nc, key, opt, carry, out, d_leaf_idx, variant, stream);
#define BF_CASE(N_, DQ_, M_, DR_)                                     \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_ && p->dr == DR_)       \
    return launch_uagsf<N_, DQ_, M_, DR_>(p, up, y, u, B, T, nc, key, opt, carry, out, d_leaf_idx, variant, stream);
  BF_CASE(1, 1, 1, 1);
  BF_CASE(3, 3, 1, 1);
  BF_CASE(4, 2, 1, 1);
  BF_CASE(4, 2, 2, 2);
  BF_CASE(4, 4, 2, 2);
#undef BF_CASE
  // no compiled instance for these dimensions: the same kernel, compiled now (needs hiprtc; dimensions up to 8)
  bf_model jit = *p;
  jit.user = registry_jit_handle(p, false);
  if (!jit.user) return set_error(BF_ENOGPU, "no current device");
  return launch_agsf_user_impl(&jit, up, y, u, B, T, nc, key, opt, carry, out, d_leaf_idx, variant, stream);
}

}  // namespace bf
