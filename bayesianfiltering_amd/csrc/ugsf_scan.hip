// Dispatch of the unscented Gaussian-sum filter kernel (ugsf_scan.hpp) over the compiled (n, dq, m, dr) table (instantiations:
// ugsf_group_{u,v}.hip), and the launches of the same kernel built at run time (user_model.hpp).  Any dimension above 8 -- or
// bf_set_option "ugsf_force_generic" = 1 -- goes to the run-time-dimension kernel instead (ugsf_generic.hip).
#include "ugsf_scan.hpp"
#include "user_model.hpp"

namespace bf {

extern Option g_ugsf_force_generic;   // ugsf_generic.hip

// the compiled (n, dq, m, dr) table: ugsf_group_{u,v}.hip, each built plain and with MISSING = true
using UgsfGroup = int(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                      int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool* matched);
UgsfGroup launch_ugsf_group_u, launch_ugsf_group_v, launch_ugsf_missing_group_u, launch_ugsf_missing_group_v;
static UgsfGroup* const kPlainGroups[] = {launch_ugsf_group_u, launch_ugsf_group_v};
static UgsfGroup* const kMissingGroups[] = {launch_ugsf_missing_group_u, launch_ugsf_missing_group_v};

// ugsf_scan_body built around the handle's functions: `kind` JIT_UGSF (sigma points through f and h) or JIT_GSF_REGS
// (extended-Kalman operations, Jacobians by dual numbers; user_flags bit 2: the covariances themselves, not their roots)
// missing: the kernel's MISSING = true twin (its own module of the handle: variant 1)
static int launch_ugsf_jit(int kind, const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
                           long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool missing = false) {
  const bf_user_model* um = p->user;
  hipFunction_t fn = nullptr;
  int rc = user_kernel(um, kind, missing ? 1 : 0, 0, JIT_SPEC_USER, &fn);
  if (rc != BF_OK) return rc;
  UgsfLaunch L;
  rc = prepare_ugsf(p, up, (um->user_flags() & 3) | (kind == JIT_GSF_REGS ? 4 : 0), y, u, B, T, K, carry, out, stream, L);
  if (rc != BF_OK) return rc;
  void* args[] = {&L.d_mdl, &L.y, &L.uptr, &L.u_sB, &L.u_sT, &L.carry, &L.out, &B, &T, &K, &L.KP, &L.d_tvq, &L.d_tvr};
  BF_HIP_CHECK(hipModuleLaunchKernel(fn, L.grid, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
  return BF_OK;
}

// The unscented Gaussian-sum scan with the caller's functions: state in registers up to dimension 8 (like the compiled
// instances), in LDS above (ugsf_generic.hip)
static int launch_ugsf_user_impl(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                                 int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream) {
  const int rc = check_user_model(p->user, p);
  if (rc != BF_OK) return rc;
  if (p->user->has_lp) return set_error(BF_EINVAL, "a log-density from source belongs to the particle filter, not to the unscented filter");
  if (p->n > 8 || p->dq > 8 || p->m > 8 || p->dr > 8 || g_ugsf_force_generic.load() != 0)
    return launch_ugsf_generic(p, up, y, u, B, T, K, carry, out, stream);
  return launch_ugsf_jit(JIT_UGSF, p, up, y, u, B, T, K, carry, out, stream);
}

// bf_gsf_ekf_f32 with functions from source and small dimensions: the Gaussian-sum scan of inference.py:333-371 with one lane per
// (trajectory, component), mean and covariance in registers, the Jacobians by dual numbers (ugsf_scan.hpp: UserEkfNodes) -- two
// orders of magnitude faster than the run-time-dimension kernel the same handle also carries (state in LDS, any n), which remains
// the path for n > 8, for a nonlinear registry function beside one from source, legacy flags, collapsed streams and K > 256.
bool gsf_user_regs_eligible(const bf_model* p, int K, const bf_out_desc* out) {
  const bf_user_model* um = p->user;
  if (!um || um->has_lp || p->flags != 0) return false;
  if (p->n > 8 || p->dq > 8 || p->m > 8 || p->dr > 8 || K > 256) return false;
  if (out->coll_mean.ptr || out->coll_cov.ptr) return false;
  if (!(um->has_dyn || p->dyn_id == DYN_LINEAR) || !(um->has_emi || p->emi_id == EMI_LINEAR)) return false;
  return true;
}

int launch_gsf_user_regs_impl(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K, const bf_carry* carry,
                              const bf_out_desc* out, hipStream_t stream) {
  const int rc = check_user_model(p->user, p);
  if (rc != BF_OK) return rc;
  return launch_ugsf_jit(JIT_GSF_REGS, p, nullptr, y, u, B, T, K, carry, out, stream);
}

int launch_ugsf_ukf(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
                    long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream) {
  if (p->user)   // functions from the caller's source: the kernel compiled at run time for this model
    return launch_ugsf_user_impl(p, up, y, u, B, T, K, carry, out, stream);
  if (p->dyn_id == BF_FN_USER || p->emi_id == BF_FN_USER)
    return set_error(BF_EINVAL, "dyn_id / emi_id = BF_FN_USER needs bf_model.user (bf_user_model_create)");
  if (p->n > 8 || p->dq > 8 || p->m > 8 || p->dr > 8 || g_ugsf_force_generic.load() != 0)   // beyond the registers: state in LDS, ahead-of-time instance
    return launch_ugsf_generic(p, up, y, u, B, T, K, carry, out, stream);
  bool matched;
  const int rc = run_groups(kPlainGroups, std::size(kPlainGroups), &matched, p, up, y, u, B, T, K, carry, out, stream);
  if (matched) return rc;
  // no compiled instance for these dimensions: the same kernel, compiled now (needs hiprtc; dimensions up to 8)
  bf_model jit = *p;
  jit.user = registry_jit_handle(p, false);
  if (!jit.user) return set_error(BF_ENOGPU, "no current device");
  return launch_ugsf_user_impl(&jit, up, y, u, B, T, K, carry, out, stream);
}

// ---- missing observations (NaN entries): the MISSING = true twins of the register kernels above.  Nothing else takes gaps, so
// whatever the plain route would send to a run-time-dimension kernel is refused here (bf_api.hip checks before any HIP call).
int launch_gsf_user_regs_missing_impl(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                                      const bf_carry* carry, const bf_out_desc* out, hipStream_t stream) {
  const int rc = check_user_model(p->user, p);
  if (rc != BF_OK) return rc;
  return launch_ugsf_jit(JIT_GSF_REGS, p, nullptr, y, u, B, T, K, carry, out, stream, true);
}

int launch_ugsf_ukf_missing(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
                            long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream) {
  if (p->user) {
    const int rc = check_user_model(p->user, p);
    if (rc != BF_OK) return rc;
    return launch_ugsf_jit(JIT_UGSF, p, up, y, u, B, T, K, carry, out, stream, true);
  }
  bool matched;
  const int rc = run_groups(kMissingGroups, std::size(kMissingGroups), &matched, p, up, y, u, B, T, K, carry, out, stream);
  if (matched) return rc;
  // no compiled instance for these dimensions: the same kernel, compiled now (needs hiprtc; dimensions up to 8)
  bf_model jit = *p;
  jit.user = registry_jit_handle(p, false);
  if (!jit.user) return set_error(BF_ENOGPU, "no current device");
  const int rc2 = check_user_model(jit.user, &jit);
  if (rc2 != BF_OK) return rc2;
  return launch_ugsf_jit(JIT_UGSF, &jit, up, y, u, B, T, K, carry, out, stream, true);
}

}  // namespace bf
