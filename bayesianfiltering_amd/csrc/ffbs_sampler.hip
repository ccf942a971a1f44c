// Host side of the posterior sampler (ffbs_sampler.hpp): the two C entry points, the register instances for n <= 8 and
// the run-time-dimension kernel for every other n (one wave per trajectory, matrices and a block of samples in LDS).
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance, n = 1 ... 8, SPL = 1, 2, 4, 8 samples
// per lane, all three dynamics kinds, builds without scratch.  VGPRs (arch + acc) / waves per SIMD, range over the kinds:
//   n    SPL = 1         SPL = 2         SPL = 4         SPL = 8
//   1    61-83 / 5-8     89-113 / 4-5    133-157 / 3     95-114 / 4-5
//   2    53-78 / 6-8     86-104 / 4-5    79-100 / 4-6    111-132 / 3-4
//   3    70-99 / 4-7     108-133 / 3-4   102-125 / 4     142-165 / 3
//   4    108-155 / 3-4   117-155 / 3-4   141-180 / 2-3   189-228 / 2
//   5    146-193 / 2-3   147-186 / 2-3   184-214 / 2     240-268 / 1-2
//   6    173-193 / 2     182-233 / 2     223-261 / 1-2   286-322 / 1
//   7    218-266 / 1-2   225-280 / 1-2   266-308 / 1     334-370 / 1
//   8    288-333 / 1     288-327 / 1     322-360 / 1     406-426 / 1
// (above 256 the per-sample states and the step's matrices spill into the accumulation registers, not to memory).  The
// run-time-dimension kernel: 116 VGPRs, 4 waves per SIMD.  "ffbs_spl" = 0 (default) picks the smallest compiled SPL that holds all S samples
// of a trajectory in one lane, 8 for S > 8 (S = 5 runs SPL = 8 with three idle slots).  It rests on the one sweep of DESIGN.md
// 6b (n = 4, B = 65 536, S = 8 and 64): SPL = 8 was the fastest there except in noise mode at S = 64.
//
// Unscented route (RTS_UNSC: X_t through rts_linearize, the root and the sigma-point images before the factorization): every
// instance n = 1 ... 8 at every SPL builds without scratch, so the register limit is 8 for all four counts
// (ffbs_unsc_reg_max).  VGPRs (arch + acc) / waves per SIMD:
//   n    SPL = 1    SPL = 2    SPL = 4    SPL = 8
//   1    72 / 7     101 / 4    145 / 3    102 / 4
//   2    80 / 6     102 / 4    98 / 4     130 / 3
//   3    103 / 4    119 / 4    139 / 3    179 / 2
//   4    160 / 3    178 / 2    202 / 2    250 / 2
//   5    207 / 2    225 / 2    253 / 2    310 / 1
//   6    293 / 1    315 / 1    349 / 1    414 / 1
//   7    360 / 1    380 / 1    408 / 1    469 / 1
//   8    388 / 1    406 / 1    440 / 1    500 / 1
// Run-time-dimension kernel: ffbs_generic_kernel<true> 134 VGPRs, 3 waves per SIMD; ffbs_generic_kernel<false> (every other
// kind) 116 VGPRs, 4 waves, as before the route existed.
//
// Source route (RTS_EXT_USER, kernels compiled at run time: jit_source.hip JIT_FFBS_REGS / JIT_FFBS_GENERIC), measured on a
// Lorenz-96 twin written as source (dq = n, -ffp-contract=off): every instance builds without scratch, so the register limit
// is 8 at all four counts (RTS_USER_REG_MAX).  VGPRs (arch + acc) / waves per SIMD:
//   n    SPL = 1    SPL = 2    SPL = 4    SPL = 8
//   1    65 / 7     93 / 5     137 / 3    99 / 4
//   2    62 / 8     90 / 5     85 / 5     117 / 4
//   3    76 / 6     113 / 4    105 / 4    145 / 3
//   4    128 / 4    125 / 4    149 / 3    199 / 2
//   5    185 / 2    171 / 2    199 / 2    255 / 2
//   6    188 / 2    224 / 2    251 / 2    316 / 1
//   7    246 / 2    272 / 1    306 / 1    372 / 1
//   8    336 / 1    292 / 1    328 / 1    398 / 1
// Run-time-dimension kernel: n = 3: 83 VGPRs / 5 waves, n = 10: 97 / 4, n = 64: 315 / 1, no scratch.
#include "ffbs_sampler.hpp"
#include "rts_generic.hpp"

namespace bf {

// ---- run-time-dimension kernel -----------------------------------------------------------------------------------
// One 64-lane workgroup per trajectory.  LDS: five n x ld matrices (P, P-, X, W, Sg), three vectors and three sample
// buffers of SB x n (state x, noise xi, result); RTS_UNSC: one more matrix (the root Rt) and the root's vectors -- its
// iterate, Newton scratch and eigenvectors alias W, X and Sg, dead until the solve -- which bounds the route at n <= 81.  Per step, with the smoother's helpers (rts_generic.hpp): W <- F_t,
// X = F P, [recompute: P-, m-], W <- chol(P-), X <- L^-1 X, then Sg = P - X^T X (lower triangle), X <- L^-T X,
// Sg <- psdchol(Sg; diag P) in place, then the samples in blocks of SB: lanes split over (sample, row) in
// x = m + X^T (x+ - m-) + Sg xi.  With one block the state stays in LDS from step to step; with more, a block's x+ is read
// back from the sample stream (each element by the lane that wrote it one step earlier).
template <bool UNSC>
__global__ void __launch_bounds__(64) ffbs_generic_kernel(FfbsGen fc, GenModel g, FfbsViews v, long long T) {
  ffbs_generic_body<UNSC, false>(fc, g, v, T);
}

// ---- host helpers --------------------------------------------------------------------------------------------------
static Option g_ffbs_spl{0, OPT_FFBS_SPL};
Option& ffbs_spl_option() { return g_ffbs_spl; }

// Largest n of the unscented route on the register kernel for a samples-per-lane count: every instance up to it builds
// without scratch (header comment).  All four counts reach n = 8.
constexpr int ffbs_unsc_reg_max(int /* spl */) { return 8; }

// the smallest compiled count that holds all S samples of a trajectory in one lane, 8 for S > 8 (header comment)
static int ffbs_pick_spl(int S, int forced) {
  if (forced) return forced;
  int spl = 1;
  while (spl < 8 && spl < S) spl *= 2;
  return spl;
}

template <int N, int KIND, class Arg>
static int launch_ffbs_n(const Arg& c, const float* d_gqg, const FfbsViews& v, long long B, long long T, int S, int forced_spl,
                         hipStream_t stream) {
  const int spl = ffbs_pick_spl(S, forced_spl);
  const long long lanes = B * ((S + spl - 1) / spl);
  if ((lanes + 63) / 64 > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B x S too large for one launch");
  const dim3 grid((unsigned)((lanes + 63) / 64));
  // an unscented instance exists only up to its SPL's limit (ffbs_unsc_reg_max; the host sends the rest to the other kernel)
  auto go = [&](auto SC) {
    constexpr int SPL = decltype(SC)::value;
    if constexpr (KIND != RTS_UNSC || N <= ffbs_unsc_reg_max(SPL))
      hipLaunchKernelGGL((ffbs_reg_kernel<N, SPL, KIND, Arg>), grid, dim3(64), 0, stream, c, d_gqg, v, B, T, S);
  };
  switch (spl) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
  }
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

// c.SB and the LDS bytes of the run-time-dimension kernel; BF_EUNSUPPORTED with the byte count when 160 KiB do not hold the model
static int ffbs_gen_plan(FfbsGen& c, size_t* lds_bytes) {
  const size_t cap = 160 * 1024 / sizeof(float);
  const int n = c.r.n;
  const int kind = c.r.kind;
  const size_t mat = ffbs_gen_mat_floats(n, kind);
  if (mat + 3 * (size_t)n > cap) {
    int nmax = 1;
    while (ffbs_gen_mat_floats(nmax + 1, kind) + 3 * (size_t)(nmax + 1) <= cap) ++nmax;
    return set_error(BF_EUNSUPPORTED, "sampler: n = %d needs %zu bytes of LDS (160 KiB per workgroup: n <= %d)", n,
                     sizeof(float) * (mat + 3 * (size_t)n), nmax);
  }
  // samples per LDS block: up to 2048 floats per buffer (keeps several workgroups per CU), at least one sample
  size_t sb = 2048 / (size_t)n;
  if (sb < 1) sb = 1;
  if (sb > (cap - mat) / (3 * (size_t)n)) sb = (cap - mat) / (3 * (size_t)n);
  if (sb > (size_t)c.S) sb = (size_t)c.S;
  c.SB = (int)sb;
  *lds_bytes = sizeof(float) * (mat + 3 * sb * n);
  return BF_OK;
}

static int launch_ffbs_generic(const FfbsGen& c0, const GenModel& g, const std::vector<float>& blk, const FfbsViews& v,
                               long long B, long long T, hipStream_t stream) {
  const int kind = c0.r.kind;
  FfbsGen c = c0;
  size_t lds = 0;
  const int prc = ffbs_gen_plan(c, &lds);
  if (prc != BF_OK) return prc;
  GenModel gg = g;
  const int rc = rts_gen_upload(c.r, gg, blk, stream);
  if (rc != BF_OK) return rc;
  if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B too large for the run-time-dimension kernel");
  auto kern = kind == RTS_UNSC ? ffbs_generic_kernel<true> : ffbs_generic_kernel<false>;
  if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds, stream, c, gg, v, T);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

static int launch_ffbs_linear(const bf_lgssm* p, const FfbsViews& v, long long B, long long T, int S, bool recompute,
                              bool force_generic, int spl, hipStream_t stream) {
  const int n = p->n;
  std::vector<float> A, GQG, Gq0;
  rts_lin_fill(p, A, GQG, Gq0);
  const bool tv = recompute && p->Q_steps > 1;
  if (!force_generic && n <= 8) {
    const float* d_gqg = nullptr;
    if (tv) {
      const void* dv = nullptr;
      const int rc = device_constants(GQG.data(), sizeof(float) * GQG.size(), stream, &dv);
      if (rc != BF_OK) return rc;
      d_gqg = static_cast<const float*>(dv);
    }
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      const RtsLin<N> c = rts_lin_arg<N>(A, GQG, Gq0);
      if (recompute) return launch_ffbs_n<N, RTS_LIN_RECOMPUTE>(c, d_gqg, v, B, T, S, spl, stream);
      return launch_ffbs_n<N, RTS_LIN>(c, nullptr, v, B, T, S, spl, stream);
    };
    BF_RTS_DIMS(n, go)
  }
  std::vector<float> blk;
  FfbsGen c;
  std::memset(&c, 0, sizeof(c));
  rts_gen_lin_block(p, recompute, A, GQG, Gq0, c.r, blk);
  c.S = S;
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  return launch_ffbs_generic(c, g, blk, v, B, T, stream);
}

// Source route (RTS_EXT_USER): the register kernel compiled at run time around the caller's dynamics, one entry point per
// samples-per-lane count (jit_source.hip: JIT_FFBS_REGS)
static int launch_ffbs_user(const bf_model* p, const FfbsViews& v, long long B, long long T, int S, bool force_generic, int forced_spl,
                            hipStream_t stream) {
  const int n = p->n;
  if (force_generic || n > RTS_USER_REG_MAX) {  // the run-time-dimension kernel (JIT_FFBS_GENERIC), launch_ffbs_generic's LDS plan
    FfbsGen c;
    std::memset(&c, 0, sizeof(c));
    c.r.n = n;
    c.r.kind = RTS_EXT_USER;
    c.S = S;
    size_t lds = 0;
    int rc = ffbs_gen_plan(c, &lds);
    if (rc != BF_OK) return rc;
    if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B too large for the run-time-dimension kernel");
    GenModel g;
    if ((rc = rts_user_gen_model(p, g, stream)) != BF_OK) return rc;
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(p->user, JIT_FFBS_GENERIC, 0, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
    FfbsViews w = v;
    long long T_ = T;
    void* args[] = {&c, &g, &w, &T_};
    return launch_user_kernel(p->user, 64, (unsigned)B, lds, stream, args, fn);
  }
  RtsUserHost h;
  int rc = rts_user_fill(p, h);
  if (rc != BF_OK) return rc;
  const int spl = ffbs_pick_spl(S, forced_spl);
  const long long lanes = B * ((S + spl - 1) / spl);
  if ((lanes + 63) / 64 > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B x S too large for one launch");
  hipFunction_t fn = nullptr;
  if ((rc = user_kernel(p->user, JIT_FFBS_REGS, spl, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
  FfbsViews w = v;
  long long B_ = B, T_ = T;
  int S_ = S;
  void* args[] = {&h, &w, &B_, &T_, &S_};
  BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)((lanes + 63) / 64), 1, 1, 64, 1, 1, 0, stream, args, nullptr));
  return BF_OK;
}

static int launch_ffbs_ext(const bf_model* p, const FfbsViews& v, long long B, long long T, int S, bool force_generic, int spl,
                           hipStream_t stream) {
  if (p->user && p->dyn_id == BF_FN_USER) return launch_ffbs_user(p, v, B, T, S, force_generic, spl, stream);
  GenModel g;
  std::vector<float> blk;
  int rc = gen_fill(p, T, g, blk);  // validates the registry ids and theta layouts
  if (rc != BF_OK) return rc;
  const int n = p->n;
  if (!force_generic && n <= 8) {
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      return launch_ffbs_n<N, RTS_EXT>(rts_ekf_arg<N>(p, g), nullptr, v, B, T, S, spl, stream);
    };
    BF_RTS_DIMS(n, go)
  }
  FfbsGen c;
  std::memset(&c, 0, sizeof(c));
  c.r.n = n;
  c.r.kind = RTS_EXT;
  c.S = S;
  return launch_ffbs_generic(c, g, blk, v, B, T, stream);
}

static int launch_ffbs_unsc(const bf_model* p, const bf_ukf_params* up, const FfbsViews& v, long long B, long long T, int S,
                            bool force_generic, int spl, hipStream_t stream) {
  RtsUnscHost h;
  int rc = rts_unsc_fill(p, up, h);
  if (rc != BF_OK) return rc;
  const int n = p->n;
  if (!force_generic && n <= ffbs_unsc_reg_max(ffbs_pick_spl(S, spl))) {
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      return launch_ffbs_n<N, RTS_UNSC>(rts_unsc_arg<N>(h), nullptr, v, B, T, S, spl, stream);
    };
    BF_RTS_DIMS(n, go)
  }
  FfbsGen c;
  std::memset(&c, 0, sizeof(c));
  std::vector<float> blk;
  if ((rc = rts_gen_unsc_block(h, n, c.r, blk)) != BF_OK) return rc;
  c.S = S;
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  return launch_ffbs_generic(c, g, blk, v, B, T, stream);
}

// bf_out_desc / bf_sample_carry / bf_sample_desc -> FfbsViews, with the checks both entry points share
static int ffbs_views(const bf_out_desc* f, const bf_sample_carry* carry, const bf_sample_desc* out, const bf_cstream* u,
                      long long B, long long T, int S, int n, bool need_pred, FfbsViews& v) {
  if (B <= 0 || T <= 0) return set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", B, T);
  if (S <= 0) return set_error(BF_EINVAL, "the number of samples S must be positive (S=%d)", S);
  if (!f->means.ptr || !f->covs.ptr) return set_error(BF_EINVAL, "filtered means and covariances are required");
  const bool has_pm = f->pred_means.ptr != nullptr, has_pP = f->pred_covs.ptr != nullptr;
  if (has_pm != has_pP) return set_error(BF_EINVAL, "pred_means and pred_covs are given together or not at all");
  if (need_pred && !has_pm) return set_error(BF_EINVAL, "the extended and the unscented sampler need the predicted means and covariances");
  if (!out->samples.ptr) return set_error(BF_EINVAL, "the samples stream is a required output");
  if (!out->noise.ptr && !out->keys) return set_error(BF_EINVAL, "give the noise stream or the keys");
  if (!out->noise.ptr && (long long)S * T * n > 0x7fffffffLL)
    return set_error(BF_EINVAL, "drawing from keys serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T");
  if (S > 0x7fffffff / n) return set_error(BF_EINVAL, "S too large");
  std::memset(&v, 0, sizeof(v));
  v.m = make_sview(f->means);
  v.P = make_sview(f->covs);
  v.pm = make_sview(f->pred_means);
  v.pP = make_sview(f->pred_covs);
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
  return BF_OK;
}

static int ffbs_spl_checked(int* spl) {
  *spl = g_ffbs_spl.load();
  if (*spl != 0 && *spl != 1 && *spl != 2 && *spl != 4 && *spl != 8)
    return set_error(BF_EINVAL, "ffbs_spl must be 0 or one of the compiled counts 1, 2, 4, 8");
  return BF_OK;
}

Option& force_generic_option();  // bf_api.hip

}  // namespace bf

extern "C" {

int bf_sampler_abi_check(size_t sizeof_sample_desc, size_t sizeof_sample_carry) {
#define BF_ABI_SIZE(NAME_, T_)                                                                                  \
  if (NAME_ != 0 && NAME_ != sizeof(T_)) \
    return bf::set_error(BF_EINVAL, "binding's sizeof(" #T_ ") = %zu, the library's is %zu: the struct layouts differ", NAME_, sizeof(T_));
  BF_ABI_SIZE(sizeof_sample_desc, bf_sample_desc)
  BF_ABI_SIZE(sizeof_sample_carry, bf_sample_carry)
#undef BF_ABI_SIZE
  return BF_OK;
}

int bf_ffbs_sample_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T, int32_t S,
                       const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (model->n <= 0 || model->dq <= 0) return bf::set_error(BF_EINVAL, "non-positive model dimension");
  if (!model->A) return bf::set_error(BF_EINVAL, "A is required");
  if (!model->G && model->dq != model->n) return bf::set_error(BF_EINVAL, "G == NULL requires dq == n");
  bf::FfbsViews v;
  int rc = bf::ffbs_views(filtered, carry, out, nullptr, B, T, S, model->n, false, v);
  if (rc != BF_OK) return rc;
  const bool recompute = v.pm.p == nullptr;
  if (recompute) {
    if (!model->Q) return bf::set_error(BF_EINVAL, "recomputing the predictions needs Q");
    if (model->Q_steps < 1 || (model->Q_steps > 1 && model->Q_steps != T))
      return bf::set_error(BF_EINVAL, "Q_steps must be 1 or T = %lld", (long long)T);
  }
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  bf_lgssm lg = *model;
  if (!recompute || lg.Q_steps < 1) lg.Q_steps = 1;  // the table is read on the recompute path only
  return bf::launch_ffbs_linear(&lg, v, B, T, S, recompute, bf::force_generic_option().load() != 0, spl,
                                static_cast<hipStream_t>(stream));
}

int bf_effbs_sample_f32(const bf_model* model, const bf_cstream* u, const bf_out_desc* filtered, int64_t B, int64_t T,
                        int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (!model->user && (model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER))
    return bf::set_error(BF_EUNSUPPORTED, "the extended sampler serves functions given as source through bf_model.user (bf_user_model_create); it is NULL");
  if (model->flags != 0)
    return bf::set_error(BF_EUNSUPPORTED, "the extended sampler needs the JAX path's update -> predict streams (flags = 0)");
  if (model->user) {  // dynamics from source: the kernel built around them; an emission from source is never read
    int rc = bf::check_user_model(model->user, model);
    if (rc == BF_OK && model->dyn_id == BF_FN_USER) rc = bf::check_user_device(model->user);
    if (rc != BF_OK) return rc;
  }
  if (model->n <= 0 || model->m <= 0 || model->dq <= 0 || model->dr <= 0)
    return bf::set_error(BF_EINVAL, "non-positive model dimension");
  if (!model->Q || !model->R) return bf::set_error(BF_EINVAL, "Q and R are required");
  bf::FfbsViews v;
  int rc = bf::ffbs_views(filtered, carry, out, u, B, T, S, model->n, true, v);
  if (rc != BF_OK) return rc;
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  return bf::launch_ffbs_ext(model, v, B, T, S, bf::force_generic_option().load() != 0, spl, static_cast<hipStream_t>(stream));
}

int bf_uffbs_sample_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered,
                        int64_t B, int64_t T, int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !uparams || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (model->user || model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER)
    return bf::set_error(BF_EUNSUPPORTED, "the unscented sampler serves registry dynamics; functions given as source are not supported");
  if (model->flags != 0)
    return bf::set_error(BF_EUNSUPPORTED, "the unscented sampler needs the JAX path's update -> predict streams (flags = 0)");
  if (model->n <= 0 || model->m <= 0 || model->dq <= 0 || model->dr <= 0)
    return bf::set_error(BF_EINVAL, "non-positive model dimension");
  if (!model->Q || !model->R) return bf::set_error(BF_EINVAL, "Q and R are required");
  bf::FfbsViews v;
  int rc = bf::ffbs_views(filtered, carry, out, u, B, T, S, model->n, true, v);
  if (rc != BF_OK) return rc;
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  return bf::launch_ffbs_unsc(model, uparams, v, B, T, S, bf::force_generic_option().load() != 0, spl, static_cast<hipStream_t>(stream));
}

}  // extern "C"
