// Host side of the posterior sampler (ffbs_sampler.hpp): its three C entry points, the run-time-dimension kernel (one wave
// per trajectory, matrices and a block of samples in LDS) and the sampler as a product of the backward family's dispatch --
// the launches of the register instances for n <= 8 at a samples-per-lane count, and of the run-time-dimension kernel for
// every other n.  The model validation, the route resolution and the register-versus-run-time-dimension decision are shared
// with the smoother: backward_host.hpp.
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
// instance n = 1 ... 8 at every SPL builds without scratch, so the family's register limit of 8 holds at all four
// counts (BACKWARD_REG_MAX).  VGPRs (arch + acc) / waves per SIMD:
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
// Lorenz-96 twin written as source (dq = n, -ffp-contract=off): every instance builds without scratch, so the family's register
// limit of 8 holds at all four counts (BACKWARD_REG_MAX).  VGPRs (arch + acc) / waves per SIMD:
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
#include "backward_host.hpp"

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

// the smallest compiled count that holds all S samples of a trajectory in one lane, 8 for S > 8 (header comment)
static int ffbs_pick_spl(int S, int forced) {
  if (forced) return forced;
  int spl = 1;
  while (spl < 8 && spl < S) spl *= 2;
  return spl;
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

// The sampler as a product of backward_dispatch (backward_host.hpp): the four launches of one call
struct FfbsProduct {
  const FfbsViews& v;
  long long B, T;
  int S, forced_spl;
  hipStream_t stream;

  // samples per lane of the register kernels and their grid
  int lanes_grid(int* spl, unsigned* grid) const {
    *spl = ffbs_pick_spl(S, forced_spl);
    const long long lanes = B * ((S + *spl - 1) / *spl);
    if ((lanes + 63) / 64 > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B x S too large for one launch");
    *grid = (unsigned)((lanes + 63) / 64);
    return BF_OK;
  }

  template <int N, int KIND, class Arg>
  int regs(const Arg& c, const float* d_gqg) const {
    int spl;
    unsigned grid;
    const int rc = lanes_grid(&spl, &grid);
    if (rc != BF_OK) return rc;
    auto go = [&](auto SC) {
      constexpr int SPL = decltype(SC)::value;
      hipLaunchKernelGGL((ffbs_reg_kernel<N, SPL, KIND, Arg>), dim3(grid), dim3(64), 0, stream, c, d_gqg, v, B, T, S);
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

  // the register kernel compiled at run time around the caller's dynamics, one entry point per samples-per-lane count
  // (jit_source.hip: JIT_FFBS_REGS)
  int user_regs(const bf_user_model* um, int /* n */, RtsUserHost& h) const {
    int spl;
    unsigned grid;
    int rc = lanes_grid(&spl, &grid);
    if (rc != BF_OK) return rc;
    hipFunction_t fn = nullptr;
    if ((rc = user_kernel(um, JIT_FFBS_REGS, spl, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
    FfbsViews w = v;
    long long B_ = B, T_ = T;
    int S_ = S;
    void* args[] = {&h, &w, &B_, &T_, &S_};
    BF_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, 64, 1, 1, 0, stream, args, nullptr));
    return BF_OK;
  }

  int generic(const RtsGen& r, const GenModel& g, const std::vector<float>& blk) const {
    FfbsGen c{r, S, 0};
    size_t lds = 0;
    int rc = ffbs_gen_plan(c, &lds);
    if (rc != BF_OK) return rc;
    GenModel gg = g;
    if ((rc = rts_gen_upload(c.r, gg, blk, stream)) != BF_OK) return rc;
    if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "sampler: B too large for the run-time-dimension kernel");
    auto kern = r.kind == RTS_UNSC ? ffbs_generic_kernel<true> : ffbs_generic_kernel<false>;
    if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds, stream, c, gg, v, T);
    BF_HIP_CHECK(hipGetLastError());
    return BF_OK;
  }

  int user_generic(const bf_model* p, const RtsGen& r) const {  // (jit_source.hip: JIT_FFBS_GENERIC)
    FfbsGen c{r, S, 0};
    size_t lds = 0;
    const int rc = ffbs_gen_plan(c, &lds);
    if (rc != BF_OK) return rc;
    FfbsViews w = v;
    return backward_launch_user_generic(p, JIT_FFBS_GENERIC, "sampler", &c, &w, B, T, lds, stream);
  }
};

// bf_out_desc / bf_sample_carry / bf_sample_desc -> FfbsViews, with the checks the sampler entry points share (the parallel
// sampler, ffbs_pscan.hip, among them)
int ffbs_views(const bf_out_desc* f, const bf_sample_carry* carry, const bf_sample_desc* out, const bf_cstream* u,
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

static int ffbs_run(const BackwardRoute& r, const FfbsViews& v, long long B, long long T, int S, int spl, void* stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return backward_dispatch(r, force_generic_option().load() != 0, FfbsProduct{v, B, T, S, spl, s}, s);
}

}  // namespace bf

extern "C" {

int bf_sampler_abi_check(size_t sizeof_sample_desc, size_t sizeof_sample_carry) {
  BF_ABI_SIZE(sizeof_sample_desc, bf_sample_desc)
  BF_ABI_SIZE(sizeof_sample_carry, bf_sample_carry)
  return BF_OK;
}

int bf_ffbs_sample_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T, int32_t S,
                       const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  int rc = bf::backward_check_lgssm(model);
  if (rc != BF_OK) return rc;
  bf::FfbsViews v;
  if ((rc = bf::ffbs_views(filtered, carry, out, nullptr, B, T, S, model->n, false, v)) != BF_OK) return rc;
  const bool recompute = v.pm.p == nullptr;
  if (recompute && (rc = bf::backward_check_recompute(model, T)) != BF_OK) return rc;
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  bf_lgssm lg = *model;
  if (!recompute || lg.Q_steps < 1) lg.Q_steps = 1;  // the table is read on the recompute path only
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(&lg, recompute, r)) != BF_OK) return rc;
  return bf::ffbs_run(r, v, B, T, S, spl, stream);
}

int bf_effbs_sample_f32(const bf_model* model, const bf_cstream* u, const bf_out_desc* filtered, int64_t B, int64_t T,
                        int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  int rc = bf::backward_check_source(model, "extended sampler", false);
  if (rc == BF_OK) rc = bf::backward_check_dims(model);
  if (rc != BF_OK) return rc;
  bf::FfbsViews v;
  if ((rc = bf::ffbs_views(filtered, carry, out, u, B, T, S, model->n, true, v)) != BF_OK) return rc;
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(model, T, r)) != BF_OK) return rc;
  return bf::ffbs_run(r, v, B, T, S, spl, stream);
}

int bf_uffbs_sample_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered,
                        int64_t B, int64_t T, int32_t S, const bf_sample_carry* carry, const bf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !uparams || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  int rc = bf::backward_check_source(model, "unscented sampler", true);
  if (rc == BF_OK) rc = bf::backward_check_dims(model);
  if (rc != BF_OK) return rc;
  bf::FfbsViews v;
  if ((rc = bf::ffbs_views(filtered, carry, out, u, B, T, S, model->n, true, v)) != BF_OK) return rc;
  int spl;
  if ((rc = bf::ffbs_spl_checked(&spl)) != BF_OK) return rc;
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(model, uparams, r)) != BF_OK) return rc;
  return bf::ffbs_run(r, v, B, T, S, spl, stream);
}

}  // extern "C"
