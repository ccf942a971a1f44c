// Gaussian-sum posterior sampler (include/bayesfilt.h: bf_gs_sample_f32, where the contract is stated; the component draw is
// gs_draw_component of ffbs_sampler.hpp): sample (b, s) draws its component z once and is then the family's backward-sampling
// recursion on chain (b, z).  A call is the family's route and dispatch with the product FfbsGsProduct:
//   regs / user_regs        ffbs_gs_reg_kernel = ffbs_reg_body<N, 1, KIND, Arg, GS = true> (gs_group_a.hip, gs_group_b.hip; around
//                           source: JIT_GS_FFBS_REGS), n <= 8: one lane per (trajectory, sample).  Every lane repeats the
//                           factorization of its chain, as the one-component kernel's lanes repeat their trajectory's, so the
//                           component only changes the addresses a lane reads; the kernel's prologue draws it.
//   generic / user_generic  ffbs_generic_body<.., GS = true>: one workgroup per (trajectory, component) serving the samples of
//                           its component; a workgroup without samples exits at once.  LDS: the one-component kernel's plus
//                           S sample indices.
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs (arch + acc) / waves per SIMD, no scratch:
//   n          1        2        3        4         5         6         7         8
//   extended   83 / 5   77 / 6   96 / 5   156 / 3   194 / 2   196 / 2   264 / 1   309 / 1
//   unscented  72 / 7   81 / 5   103 / 4  161 / 3   206 / 2   292 / 1   354 / 1   384 / 1
// Run-time-dimension kernel: ffbs_gs_generic_kernel<false> 117 VGPRs / 4 waves, <true> (unscented) 135 / 3, no scratch.
#include "gs_smoother.hpp"

namespace bf {

template <bool UNSC>
__global__ void __launch_bounds__(64) ffbs_gs_generic_kernel(FfbsGen fc, GenModel g, FfbsViews v, long long T, GsDraw gd) {
  ffbs_generic_body<UNSC, false, true>(fc, g, v, T, &gd);
}

namespace {

struct FfbsGsProduct {
  const FfbsViews& v;
  const GsDraw& gd;
  long long B, T;
  int S;
  hipStream_t stream;

  template <int N, int KIND, class Arg>
  int regs(const Arg& c, const float*) const {
    if constexpr (KIND == RTS_EXT || KIND == RTS_UNSC) return gs_ffbs_launch<N, KIND, Arg>(c, v, gd, B, T, S, stream);
    else return set_error(BF_EINVAL, "Gaussian-sum sampler: no such route");  // (bf_model routes only)
  }

  int user_regs(const bf_user_model* um, int, RtsUserHost& h) const {
    const long long blocks = (B * S + 63) / 64;
    if (blocks > 0x7fffffffLL) return set_error(BF_EINVAL, "Gaussian-sum sampler: B x S too large for one launch");
    hipFunction_t fn = nullptr;
    const int rc = user_kernel(um, JIT_GS_FFBS_REGS, 0, 0, JIT_SPEC_USER, &fn);
    if (rc != BF_OK) return rc;
    FfbsViews w = v;
    GsDraw d = gd;
    long long B_ = B, T_ = T;
    int S_ = S;
    void* args[] = {&h, &w, &d, &B_, &T_, &S_};
    BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)blocks, 1, 1, 64, 1, 1, 0, stream, args, nullptr));
    return BF_OK;
  }

  // c.SB and the LDS bytes: the one-component kernel's plan (matrices, three sample buffers of SB x n) plus S sample indices
  int plan(FfbsGen& c, size_t* lds_bytes) const {
    const size_t cap = 160 * 1024 / sizeof(float);
    const int n = c.r.n;
    const size_t mat = ffbs_gen_mat_floats(n, c.r.kind) + (size_t)S;
    if (mat + 3 * (size_t)n > cap)
      return set_error(BF_EUNSUPPORTED, "Gaussian-sum sampler: n = %d with S = %d samples needs %zu bytes of LDS (160 KiB per workgroup)", n, S,
                       sizeof(float) * (mat + 3 * (size_t)n));
    size_t sb = 2048 / (size_t)n;
    if (sb < 1) sb = 1;
    if (sb > (cap - mat) / (3 * (size_t)n)) sb = (cap - mat) / (3 * (size_t)n);
    if (sb > (size_t)S) sb = (size_t)S;
    c.SB = (int)sb;
    *lds_bytes = sizeof(float) * (mat + 3 * sb * n);
    if (B * gd.K > 0x7fffffffLL) return set_error(BF_EINVAL, "Gaussian-sum sampler: B x K too large for the run-time-dimension kernel");
    return BF_OK;
  }

  int generic(const RtsGen& r, const GenModel& g, const std::vector<float>& blk) const {
    FfbsGen c{r, S, 0};
    size_t lds = 0;
    int rc = plan(c, &lds);
    if (rc != BF_OK) return rc;
    GenModel gg = g;
    if ((rc = rts_gen_upload(c.r, gg, blk, stream)) != BF_OK) return rc;
    auto kern = r.kind == RTS_UNSC ? ffbs_gs_generic_kernel<true> : ffbs_gs_generic_kernel<false>;
    if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * gd.K)), dim3(64), lds, stream, c, gg, v, T, gd);
    BF_HIP_CHECK(hipGetLastError());
    return BF_OK;
  }

  int user_generic(const bf_model* p, const RtsGen& r) const {  // (jit_source.hip: JIT_GS_FFBS_GENERIC)
    FfbsGen c{r, S, 0};
    size_t lds = 0;
    const int rc = plan(c, &lds);
    if (rc != BF_OK) return rc;
    FfbsViews w = v;
    GsDraw d = gd;
    return backward_launch_user_generic(p, JIT_GS_FFBS_GENERIC, "Gaussian-sum sampler", &c, &w, B, T, lds, stream, gd.K, &d);
  }
};

}  // namespace
}  // namespace bf

extern "C" {

int bf_gs_sample_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered, int64_t B,
                     int64_t T, int64_t K, int32_t S, const bf_sample_carry* carry, const bf_gs_sample_desc* out, void* stream) {
  using namespace bf;
  CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return set_error(BF_EINVAL, "NULL argument");
  int rc = backward_check_source(model, uparams ? "unscented Gaussian-sum sampler" : "extended Gaussian-sum sampler", uparams != nullptr);
  if (rc == BF_OK) rc = backward_check_dims(model);
  if (rc != BF_OK) return rc;
  const int n = model->n;
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (K < 1) return set_error(BF_EINVAL, "K must be at least 1 (K=%lld)", (long long)K);
  if (K > 0x7fffffffLL) return set_error(BF_EINVAL, "K too large (K=%lld)", (long long)K);
  if (S <= 0) return set_error(BF_EINVAL, "the number of samples S must be positive (S=%d)", (int)S);
  if (!filtered->means.ptr || !filtered->covs.ptr) return set_error(BF_EINVAL, "filtered means and covariances are required");
  if (!filtered->pred_means.ptr || !filtered->pred_covs.ptr)
    return set_error(BF_EINVAL, "the Gaussian-sum sampler needs the predicted means and covariances (pred_means, pred_covs)");
  if (!out->samples.ptr) return set_error(BF_EINVAL, "the samples stream is a required output");
  if (!out->noise.ptr && !out->keys) return set_error(BF_EINVAL, "give the noise stream or the keys");
  if (!out->noise.ptr && (long long)S * T * n > 0x7fffffffLL)
    return set_error(BF_EINVAL, "drawing from keys serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T");
  if (S > 0x7fffffff / n) return set_error(BF_EINVAL, "S too large");
  if (!out->comp_in) {
    if (!out->weights) return set_error(BF_EINVAL, "out->weights is required to draw the components (or give out->comp_in)");
    if ((out->comp_noise != nullptr) == (out->comp_keys != nullptr))
      return set_error(BF_EINVAL, "give exactly one of out->comp_noise and out->comp_keys (or out->comp_in)");
  }
  FfbsViews v;
  std::memset(&v, 0, sizeof(v));
  v.m = make_sview(filtered->means);
  v.P = make_sview(filtered->covs);
  v.pm = make_sview(filtered->pred_means);
  v.pP = make_sview(filtered->pred_covs);
  v.x = make_sview(out->samples);
  v.xi = SView{const_cast<float*>(out->noise.ptr), out->noise.sB, out->noise.sK, out->noise.sT, out->noise.sE};
  v.keys = out->keys;
  if (carry) {
    v.x_in = carry->x_in;
    v.x_out = carry->x_out;
  }
  if (u && u->ptr) {
    v.u = u->ptr;
    v.u_sB = u->sB;
    v.u_sT = u->sT;
  }
  const GsDraw gd{out->weights, out->comp_noise, out->comp_keys, out->comp_in, out->comp_out, (int)K};
  BackwardRoute r;
  if ((rc = uparams ? backward_route(model, uparams, r) : backward_route(model, T, r)) != BF_OK) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return backward_dispatch(r, force_generic_option().load() != 0, FfbsGsProduct{v, gd, B, T, (int)S, s}, s);
}

}  // extern "C"
