// ugsf_generic: the unscented Gaussian-sum filter for ANY dimensions (run-time n, dq, m, dr, K) -- host side and dispatch of
// ugsf_generic_device.hpp.
//
// Same recursion as the register kernel (ugsf_scan.hpp) -- the lax.scan body of unscented_gaussian_sum_filter
// (gaussfiltax/inference.py:379-456): _ukf_condition_on_nonadditive (:198-224) per component, reweight (:424-427),
// _ukf_predict_nonadditive (:146-174) per component, sigma points of utils.py:247-254 -- for the shapes that kernel's registers
// do not hold: any of n, dq, m, dr above 8, or more than 256 components.  The reference's functions are plain jnp on arbitrary
// shapes; this is the engine's counterpart.
//
// Mapping (gfx950).  One workgroup per trajectory, the component being advanced in LDS, exactly as generic_scan.hip maps the
// extended filter (components take turns through the caller's carry buffers or a stream-ordered scratch; reweight once per step
// over all K in adjacent-pair tree order; LU solve in getrf order, Cholesky log-likelihood: generic_device.hpp's routines).
// New here, twice per step and component:
//   * sqrtm(P) = V diag(sqrt(max(lambda, 0))) V^T by a parallel Jacobi eigen-decomposition in LDS, round-robin (Brent-Luk)
//     pairing: ceil(n / 2) disjoint rotations per stage (odd n: one idle index), n - 1 (n even) or n (n odd) stages per sweep,
//     three barriers per stage (angles by the first lanes | columns of A and V | rows of A), then one Newton step on R^2 = P
//     (five n^3 LDS products) that takes the root from the ~1e-6 an accumulated V gives to float32 resolution.  A, V and the root have an odd row
//     pitch (n | 1): a rotation walks down two columns, one row per lane, and an odd pitch spreads 32 consecutive rows over the 32
//     banks of ds_read_b32 / ds_write_b32.  The sweep loop has the compile-time bound UG_MAX_SWEEPS = 24 and leaves when the
//     off-diagonal mass, reduced to one LDS value that every lane reads, is below 1e-14 of the diagonal's: uniform, so no lane can
//     be left at another barrier, and a NaN / Inf matrix leaves at the first test and yields NaN.
//   * the 2 L + 1 images of the sigma points and the centre, one work item per (point, output row), kept in LDS; the block
//     structure of blockdiag(P, noise covariance) is used as it is: the 2 n state-block points carry the noise bias, the 2 d
//     noise-block points carry the mean and take their rows from the host's sqrtm(Q_t) / sqrtm(R_t), and only the state-block
//     points enter the cross-covariance.  Mean, deviations, then dev^T dev as an LDS product (one lane per 1 x 4 block).
// NT = 64 threads (one wave: the barriers are free) while max(n, dq, m, dr) <= 16, 256 above (measured, K = 4, no streams: n = 16
// 6.6e6 component-steps/s with one wave against 4.4e6 with four, n = 24 1.2e6 against 1.8e6; BAYESFILT_UGSF_NT64_MAX moves it).
//
// LDS (floats; r4 = round up to 4, ldn = r4(n) + 4, ldm = r4(m) + 4, ldj = n | 1, KPa = r4(K rounded up to a power of two)):
//   n ldn + 3 r4(n ldj) + 4 r4(n) + max(r4(n), r4(m)) + 4 r4(m) + 4 r4(ceil(n / 2)) + 3 KPa
//   + max((2 (n + dq) + 1) ldn,  (2 (n + dr) + 1) ldm + m ldn + 2 n ldm + 3 m ldm)            (ug_carve)
// n = dq = 40, m = dr = 20, K = 4: 56,784 bytes.  With dq = n, m = dr = n / 2 the 160 KiB of a workgroup hold n <= 68 (n = 68:
// 159,120 bytes; n = 69: 164,992); functions from source are bounded by the handle's 64.  Above 160 KiB: BF_EUNSUPPORTED with
// the byte count.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; LDS is dynamic):
//   ugsf_generic_kernel<64>:  126 VGPRs, 0 AGPRs, 106 SGPRs, scratch 0, static LDS 0, 4 waves / SIMD by registers
//   ugsf_generic_kernel<256>: 127 VGPRs, 0 AGPRs, 106 SGPRs, scratch 0, static LDS 0, 4 waves / SIMD by registers
// (a run-time build around a caller's f / h keeps one sigma point in registers at the handle's dimensions: 215 VGPRs, scratch 0,
// for sine dynamics + a dense linear emission at n = 12, m = 6)
#include <cstdlib>
#include <vector>
#include "forward_host.hpp"
#include "ugsf_scan.hpp"
#include "ugsf_generic_device.hpp"
#include "user_model.hpp"

namespace bf {

// one wave per workgroup (its barriers are free) up to this largest dimension, four waves above
static int ug_nt64_max() {
  static const int v = [] {
    const char* e = std::getenv("BAYESFILT_UGSF_NT64_MAX");
    const int x = e ? std::atoi(e) : 16;
    return x > 0 ? x : 16;
  }();
  return v;
}

Option g_ugsf_force_generic{0, OPT_UGSF_FORCE_GENERIC};   // bf_set_option "ugsf_force_generic": 1 = this kernel also where every dimension is <= 8

// The kernel-argument model of the run-time-dimension unscented kernels (this file's and agsf_generic.hip's): one constant block
// on the device -- the flat words of a UkfModel<n, dq, m, dr> (validation, sqrtm(Q) / sqrtm(R) and the unscented constants:
// fill_ukf_model_view), then the caller's parameter vectors at full length -- and the per-step sqrtm tables.
int ug_model_prepare(const bf_model* p, const bf_ukf_params* up, int user_flags, hipStream_t stream, UgModel& g) {
  const int n = p->n, dq = p->dq, m = p->m, dr = p->dr;
  const bool udyn = (user_flags & 1) != 0, uemi = (user_flags & 2) != 0;
  bf_model q = *p;
  if (udyn) q.n_dyn_theta = 0;
  if (uemi) q.n_emi_theta = 0;
  const size_t nw = ukf_model_words(n, dq, m, dr);
  const size_t nth_d = udyn && p->n_dyn_theta > 0 ? (size_t)p->n_dyn_theta : 0, nth_e = uemi && p->n_emi_theta > 0 ? (size_t)p->n_emi_theta : 0;
  std::vector<uint32_t> words(nw + nth_d + nth_e + 2, 0u);
  std::vector<float> tvq, tvr;
  const UkfModelView e = ukf_model_view_flat(words.data(), n, dq, m, dr);
  int rc = fill_ukf_model_view(&q, up, e, user_flags, &tvq, &tvr);
  if (rc != BF_OK) return rc;
  float* thd = reinterpret_cast<float*>(words.data()) + nw;
  float* the = thd + nth_d + 1;
  for (size_t i = 0; i < nth_d; ++i) thd[i] = p->dyn_theta[i];
  for (size_t i = 0; i < nth_e; ++i) the[i] = p->emi_theta[i];
  const void* dv = nullptr;
  if ((rc = device_constants(words.data(), sizeof(uint32_t) * words.size(), stream, &dv)) != BF_OK) return rc;
  g.dyn_id = p->dyn_id; g.emi_id = p->emi_id; g.n = n; g.dq = dq; g.m = m; g.dr = dr;
  for (int i = 0; i < 8; ++i) { g.dth[i] = e.dth[i]; g.eth[i] = e.eth[i]; }
  const float* base = static_cast<const float*>(dv);
  const float* host = reinterpret_cast<const float*>(words.data());
  auto dev = [&](const float* h) { return base + (h - host); };
  g.A = dev(e.A); g.Gm = dev(e.Gm); g.Hm = dev(e.Hm); g.Dm = dev(e.Dm); g.q0 = dev(e.q0); g.r0 = dev(e.r0); g.sQ = dev(e.sQ); g.sR = dev(e.sR);
  g.dyn_theta = dev(thd); g.emi_theta = dev(the);
  g.c_u = e.cu[0]; g.ws_u = e.cu[1]; g.w0_u = e.cu[2]; g.wc_u = e.cu[3];
  g.c_p = e.cp[0]; g.ws_p = e.cp[1]; g.w0_p = e.cp[2]; g.wc_p = e.cp[3];
  if ((rc = upload_table(tvq, stream, &g.tvsq)) != BF_OK || (rc = upload_table(tvr, stream, &g.tvsr)) != BF_OK) return rc;
  return BF_OK;
}

int launch_ugsf_generic(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                        int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream) {
  const int n = p->n, dq = p->dq, m = p->m, dr = p->dr;
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return set_error(BF_EUNSUPPORTED, "collapsed streams are produced by bf_gsf_ekf_f32 only");
  const bf_user_model* um = p->user;
  int user_flags = 0;
  if (um) {
    const int rc = check_user_model(um, p);
    if (rc != BF_OK) return rc;
    if (um->has_lp) return set_error(BF_EINVAL, "a log-density from source belongs to the particle filter, not to the unscented filter");
    user_flags = um->user_flags() & 3;
  }
  const bool udyn = (user_flags & 1) != 0, uemi = (user_flags & 2) != 0;
  if (!udyn && p->dyn_id != DYN_LINEAR && p->dyn_id != DYN_LORENZ96 && p->dyn_id != DYN_SINE)
    return set_error(BF_EUNSUPPORTED, "run-time-dimension unscented filter: dynamics id %d runs on the compiled (n <= 8) instances only", p->dyn_id);
  if (!uemi && p->emi_id != EMI_LINEAR && p->emi_id != EMI_QUADRATIC && p->emi_id != EMI_STOCH_VOL)
    return set_error(BF_EUNSUPPORTED, "run-time-dimension unscented filter: emission id %d runs on the compiled (n <= 8) instances only", p->emi_id);
  if ((p->Q_steps > 1 && p->Q_steps != T) || (p->R_steps > 1 && p->R_steps != T))
    return set_error(BF_EINVAL, "time-varying covariances need one matrix per step (Q_steps / R_steps = T = %lld)", T);
  int KP = 1;
  while (KP < K) KP <<= 1;
  const UgCarve cv = ug_carve(n, dq, m, dr, KP);
  const size_t lds_bytes = sizeof(float) * (size_t)cv.total;
  if (lds_bytes > 160 * 1024)
    return set_error(BF_EUNSUPPORTED, "run-time-dimension unscented filter: n = %d, dq = %d, m = %d, dr = %d, K = %d need %zu bytes of LDS (160 KiB per workgroup)",
                     n, dq, m, dr, K, lds_bytes);

  UgModel g;
  int rc = ug_model_prepare(p, up, user_flags, stream, g);
  if (rc != BF_OK) return rc;

  // K > 1: carried means / covariances of the components that are not in the LDS tile (launch_gsf_generic's scheme)
  float* gm = nullptr;
  float* gP = nullptr;
  float* scratch = nullptr;
  if (K > 1) {
    gm = carry->m_out;
    gP = carry->P_out;
    if (!gm || !gP) {
      const size_t fl = (size_t)B * K * ((size_t)n + (size_t)n * n);
      BF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&scratch), sizeof(float) * fl, stream));
      if (!gm) gm = scratch;
      if (!gP) gP = scratch + (size_t)B * K * n;
    }
  }
  auto [yv, cr, ov] = forward_views(y, carry, out);
  UViewG uv = input_view<UViewG>(u);
  int dmax = n > dq ? n : dq;
  dmax = dmax > m ? dmax : m;
  dmax = dmax > dr ? dmax : dr;
  const int nt = dmax <= ug_nt64_max() ? 64 : 256;
  if (um) {  // the run-time build of the same kernel around the caller's f / h (jit_source.hip: JIT_UGSF_GENERIC)
    hipFunction_t fn = nullptr;
    rc = user_kernel(um, JIT_UGSF_GENERIC, 0, nt / 64, JIT_SPEC_USER, &fn);
    if (rc == BF_OK) {
      int kp = KP;
      void* args[] = {&g, &yv, &uv, &cr, &ov, &gm, &gP, &B, &T, &K, &kp};
      rc = launch_user_kernel(um, nt, (unsigned)B, lds_bytes, stream, args, fn);
    }
    if (scratch) (void)hipFreeAsync(scratch, stream);
    return rc;
  }
  hipError_t le;
  if (nt == 64) {
    auto kern = ugsf_generic_kernel<64>;
    if (lds_bytes > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds_bytes, stream, g, yv, uv, cr, ov, gm, gP, B, T, K, KP);
    le = hipGetLastError();
  } else {
    auto kern = ugsf_generic_kernel<256>;
    if (lds_bytes > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(256), lds_bytes, stream, g, yv, uv, cr, ov, gm, gP, B, T, K, KP);
    le = hipGetLastError();
  }
  if (scratch) (void)hipFreeAsync(scratch, stream);
  BF_HIP_CHECK(le);
  return BF_OK;
}

}  // namespace bf
