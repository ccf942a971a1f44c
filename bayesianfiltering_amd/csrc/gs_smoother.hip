// Gaussian-sum smoother (include/bayesfilt.h: bf_gs_smoother_f32; the contract is stated there and the kernels' chain indexing
// in rts_smoother.hpp / rts_generic.hpp): the backward pass of a K-component filter.  Chain (b, k) is the family's RTS
// recursion on its own streams, so a call is the family's route (backward_route) and dispatch (backward_dispatch) with one
// more product, RtsGsProduct, whose launches index chains:
//   regs / user_regs   rts_gs_reg_kernel (gs_group_a.hip, gs_group_b.hip; built around source: JIT_GS_RTS_REGS), n <= 8:
//                      GS_COMP alone: one lane per chain, densely packed; with collapsed moments: KP = 2^ceil(log2 K) <= 64 adjacent
//                      lanes per trajectory and the moments reduced across them after every step;
//   generic / user_generic   rts_generic_body<.., GS = true>: one workgroup per chain.
// Where only per-component streams are asked for and every stream flattens (sB == K sK, inputs shared by the batch), the
// chains ARE B K one-component trajectories: the call goes to the one-component smoother (rts_run) and with it to the staged
// data path.  K > 64, n > 8 and "force_generic": collapsed moments come from bf_collapse_f32's kernel over the per-component
// streams with a broadcast weight view (sT = 0), on the same stream.
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs (arch + acc) / waves per SIMD; every listed
// instance builds without scratch:
//   route, output set           n = 1     2        3        4        5        6        7        8
//   extended, components        48 / 8    68 / 7   112 / 4  177 / 2  241 / 2  286 / 1  449 / 1  489 / 1
//   extended, collapsed only    48 / 8    71 / 7   124 / 4  184 / 2  267 / 1  312 / 1  -        -
//   extended, both              54 / 7    82 / 5   130 / 3  211 / 2  306 / 1  362 / 1  -        -
//   unscented, components       35 / 8    69 / 7   103 / 4  172 / 2  242 / 2  346 / 1  482 / 1  494 / 1
//   unscented, collapsed only   35 / 8    68 / 7   119 / 4  191 / 2  263 / 1  388 / 1  -        -
//   unscented, both             42 / 7    87 / 5   133 / 3  213 / 2  296 / 1  434 / 1  -        -
// The fused instances at n = 7 and 8 spill (12 ... 576 bytes of scratch per lane; only "extended, collapsed only" at n = 8 does
// not), so none of them is compiled and the fused moments stop at n = 6 (GS_FUSED_NMAX, gs_smoother.hpp): with the
// per-component streams present those n collapse afterwards, collapsed output alone is refused with the limit in the message.
// Run-time-dimension kernel: rts_gs_generic_kernel<false> 113 VGPRs / 4 waves, <true> (unscented) 130 / 3, no scratch.  The
// kernels built around source (JIT_GS_RTS_REGS) share the bodies; their registers depend on the caller's function.
#include "gs_smoother.hpp"

namespace bf {

template <bool UNSC>
__global__ void __launch_bounds__(64) rts_gs_generic_kernel(RtsGen c, GenModel g, RtsViews v, long long T, int K) {
  rts_generic_body<UNSC, false, true>(c, g, v, T, K);
}

namespace {

struct GsCall {
  RtsGsViews gv;
  long long B, T;
  int out;                 // GS_COMP | GS_COLL
  const bf_gs_smooth_desc* desc;
  hipStream_t stream;
};

// contiguous [B][T][E]
bool gs_contig(const bf_stream& s, long long T, long long E) { return s.ptr == nullptr || (s.sE == 1 && s.sT == E && s.sB == T * E); }

// collapsed moments from the per-component streams just written: bf_collapse_f32's kernel, weights broadcast over t
int gs_collapse_streams(const GsCall& k, int n) {
  bf_stream w{const_cast<float*>(k.gv.w), k.gv.K, 1, 0, 1};
  return launch_collapse(&w, &k.desc->means, k.desc->coll_cov.ptr ? &k.desc->covs : nullptr, k.B, k.T, k.gv.K, n, k.desc->coll_mean.ptr,
                         k.desc->coll_cov.ptr, k.stream);
}

struct RtsGsProduct {
  const GsCall& k;

  // the output set of the register launch; *after: collapse the streams afterwards
  int reg_out(int n, int* out, bool* after) const {
    *after = false;
    *out = k.out;
    if ((k.out & GS_COLL) && !gs_fused_ok(n, k.gv.K)) {
      if (!(k.out & GS_COMP))
        return set_error(BF_EUNSUPPORTED, "Gaussian-sum smoother: collapsed moments alone serve K <= %d components and n <= %d, where the "
                         "fused instances build without scratch (K = %d, n = %d); ask for the per-component streams too",
                         (int)GS_FUSED_KMAX, (int)GS_FUSED_NMAX, k.gv.K, n);
      *out = GS_COMP;
      *after = true;
    }
    return BF_OK;
  }

  template <int N, int KIND, class Arg>
  int regs(const Arg& c, const float*) const {
    if constexpr (KIND == RTS_EXT || KIND == RTS_UNSC) {
      int out;
      bool after;
      int rc = reg_out(N, &out, &after);
      if (rc != BF_OK) return rc;
      if ((rc = gs_rts_launch<N, KIND, Arg>(c, out, k.gv, k.B, k.T, k.stream)) != BF_OK) return rc;
      return after ? gs_collapse_streams(k, N) : BF_OK;
    } else {
      return set_error(BF_EINVAL, "Gaussian-sum smoother: no such route");  // (bf_model routes only)
    }
  }

  int user_regs(const bf_user_model* um, int n, RtsUserHost& h) const {
    int out;
    bool after;
    int rc = reg_out(n, &out, &after);
    if (rc != BF_OK) return rc;
    unsigned grid;
    if ((rc = gs_reg_grid(k.gv, out, k.B, &grid)) != BF_OK) return rc;
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(um, JIT_GS_RTS_REGS, out, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
    RtsGsViews w = k.gv;
    long long B_ = k.B, T_ = k.T;
    void* args[] = {&h, &w, &B_, &T_};
    BF_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, 64, 1, 1, 0, k.stream, args, nullptr));
    return after ? gs_collapse_streams(k, n) : BF_OK;
  }

  int plan(const RtsGen& c, size_t* lds_bytes) const {
    if (!(k.out & GS_COMP))
      return set_error(BF_EUNSUPPORTED, "Gaussian-sum smoother: collapsed moments alone serve n <= %d on the register kernel (n = %d%s); ask "
                       "for the per-component streams too", (int)GS_FUSED_NMAX, c.n, c.n <= BACKWARD_REG_MAX ? ", force_generic" : "");
    const size_t lds = sizeof(float) * rts_gen_lds_floats(c.n, c.kind);
    if (lds > 160 * 1024)
      return set_error(BF_EUNSUPPORTED, "Gaussian-sum smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup)", c.n, lds);
    if (k.B * k.gv.K > 0x7fffffffLL) return set_error(BF_EINVAL, "Gaussian-sum smoother: B x K too large for the run-time-dimension kernel");
    *lds_bytes = lds;
    return BF_OK;
  }

  int generic(const RtsGen& c0, const GenModel& g, const std::vector<float>& blk) const {
    size_t lds = 0;
    int rc = plan(c0, &lds);
    if (rc != BF_OK) return rc;
    RtsGen c = c0;
    GenModel gg = g;
    if ((rc = rts_gen_upload(c, gg, blk, k.stream)) != BF_OK) return rc;
    auto kern = c.kind == RTS_UNSC ? rts_gs_generic_kernel<true> : rts_gs_generic_kernel<false>;
    if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(k.B * k.gv.K)), dim3(64), lds, k.stream, c, gg, k.gv.v, k.T, k.gv.K);
    BF_HIP_CHECK(hipGetLastError());
    return (k.out & GS_COLL) ? gs_collapse_streams(k, c.n) : BF_OK;
  }

  int user_generic(const bf_model* p, const RtsGen& c0) const {  // (jit_source.hip: JIT_GS_RTS_GENERIC)
    size_t lds = 0;
    int rc = plan(c0, &lds);
    if (rc != BF_OK) return rc;
    RtsGen c = c0;
    RtsViews w = k.gv.v;
    if ((rc = backward_launch_user_generic(p, JIT_GS_RTS_GENERIC, "Gaussian-sum smoother", &c, &w, k.B, k.T, lds, k.stream, k.gv.K)) != BF_OK)
      return rc;
    return (k.out & GS_COLL) ? gs_collapse_streams(k, c.n) : BF_OK;
  }
};

}  // namespace
}  // namespace bf

extern "C" {

int bf_gs_abi_check(size_t sizeof_gs_smooth_desc, size_t sizeof_gs_sample_desc) {
  BF_ABI_SIZE(sizeof_gs_smooth_desc, bf_gs_smooth_desc)
  BF_ABI_SIZE(sizeof_gs_sample_desc, bf_gs_sample_desc)
  return BF_OK;
}

int bf_gs_smoother_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered, int64_t B,
                       int64_t T, int64_t K, const bf_smooth_carry* carry, const bf_gs_smooth_desc* out, void* stream) {
  using namespace bf;
  CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return set_error(BF_EINVAL, "NULL argument");
  int rc = backward_check_source(model, uparams ? "unscented Gaussian-sum smoother" : "extended Gaussian-sum smoother", uparams != nullptr);
  if (rc != BF_OK) return rc;
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (K < 1) return set_error(BF_EINVAL, "K must be at least 1 (K=%lld)", (long long)K);
  if (K > 0x7fffffffLL) return set_error(BF_EINVAL, "K too large (K=%lld)", (long long)K);
  if ((rc = backward_check_dims(model)) != BF_OK) return rc;
  const int n = model->n;
  if (!filtered->means.ptr || !filtered->covs.ptr) return set_error(BF_EINVAL, "filtered means and covariances are required");
  if (!filtered->pred_means.ptr || !filtered->pred_covs.ptr)
    return set_error(BF_EINVAL, "the Gaussian-sum smoother needs the predicted means and covariances (pred_means, pred_covs)");
  const bool comp = out->means.ptr || out->covs.ptr, coll = out->coll_mean.ptr || out->coll_cov.ptr;
  if (comp && (!out->means.ptr || !out->covs.ptr)) return set_error(BF_EINVAL, "out->means and out->covs are given together or not at all");
  if (out->cross_covs.ptr && !comp) return set_error(BF_EINVAL, "out->cross_covs needs out->means and out->covs");
  if (!comp && !coll)
    return set_error(BF_EINVAL, "at least one output is required: out->means / covs or out->coll_mean / coll_cov");
  if (coll && !out->weights) return set_error(BF_EINVAL, "out->weights is required with collapsed outputs (coll_mean, coll_cov)");
  if (carry && ((carry->m_in == nullptr) != (carry->P_in == nullptr)))
    return set_error(BF_EINVAL, "carry.m_in and carry.P_in are given together or not at all");
  if (carry && ((carry->m_out == nullptr) != (carry->P_out == nullptr)))
    return set_error(BF_EINVAL, "carry.m_out and carry.P_out are given together or not at all");
  const bool force_generic = force_generic_option().load() != 0;
  const bool reg = !force_generic && n <= BACKWARD_REG_MAX;
  if (coll && comp && !(reg && gs_fused_ok(n, K)) && (!gs_contig(out->coll_mean, T, n) || !gs_contig(out->coll_cov, T, (long long)n * n)))
    return set_error(BF_EUNSUPPORTED, "out->coll_mean / coll_cov must be contiguous [B][T][E] for K > %d, n > %d and force_generic",
                     (int)GS_FUSED_KMAX, (int)GS_FUSED_NMAX);
  const int load_mode = rts_load_mode_option().load();
  if (uparams && load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 is not offered on the unscented route");

  GsCall k;
  std::memset(&k, 0, sizeof(k));
  RtsViews& v = k.gv.v;
  v.m = make_sview(filtered->means);
  v.P = make_sview(filtered->covs);
  v.pm = make_sview(filtered->pred_means);
  v.pP = make_sview(filtered->pred_covs);
  v.ms = make_sview(out->means);
  v.Ps = make_sview(out->covs);
  v.Cs = make_sview(out->cross_covs);
  if (carry) {
    v.m_in = carry->m_in;
    v.P_in = carry->P_in;
    v.m_out = carry->m_out;
    v.P_out = carry->P_out;
  }
  if (u && u->ptr) {
    v.u = u->ptr;
    v.u_sB = u->sB;
    v.u_sT = u->sT;
  }
  k.gv.cm = make_sview(out->coll_mean);
  k.gv.cP = make_sview(out->coll_cov);
  k.gv.w = out->weights;
  k.gv.K = (int)K;
  k.gv.KP = K <= GS_FUSED_KMAX ? gs_lanes((int)K) : 64;
  k.gv.b_inner = v.m.sB < v.m.sK ? 1 : 0;
  k.B = B;
  k.T = T;
  k.out = (comp ? GS_COMP : 0) | (coll ? GS_COLL : 0);
  k.desc = out;
  k.stream = static_cast<hipStream_t>(stream);

  BackwardRoute r;
  if ((rc = uparams ? backward_route(model, uparams, r) : backward_route(model, T, r)) != BF_OK) return rc;

  // per-component output over streams that flatten: B K one-component trajectories (K = 1: any layout)
  bool flat = !coll && (v.u == nullptr || v.u_sB == 0 || K == 1);
  for (const SView* s : {&v.m, &v.P, &v.pm, &v.pP, &v.ms, &v.Ps, &v.Cs}) flat = flat && (s->p == nullptr || K == 1 || s->sB == K * s->sK);
  if (flat) {
    RtsViews f = v;
    if (K > 1) for (SView* s : {&f.m, &f.P, &f.pm, &f.pP, &f.ms, &f.Ps, &f.Cs}) s->sB = s->sK;
    return rts_run(r, f, B * K, T, stream);
  }
  if (load_mode == RTS_STAGED)
    return set_error(BF_EINVAL, "rts_load_mode = 2 serves per-component output on the contiguous reference layout only");
  return backward_dispatch(r, force_generic, RtsGsProduct{k}, k.stream);
}

}  // extern "C"
