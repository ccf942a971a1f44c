// Host side of the RTS smoother (rts_smoother.hpp): its three C entry points, the run-time-dimension kernel (one wave per
// trajectory, the smoother's matrices in LDS) and the smoother as a product of the backward family's dispatch -- the launches
// of the register instances for n <= 8 with their data path, and of the run-time-dimension kernel for every other n.  The
// model validation, the route resolution and the register-versus-run-time-dimension decision are shared with the posterior
// sampler: backward_host.hpp.
//
// Register instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): every instance, n = 1 ... 8, both data paths,
// all three dynamics kinds, builds without scratch.  Strided path, VGPRs (arch + acc) / waves per SIMD: n = 1: 24-48 / 8,
// n = 2: 44-67 / 7-8, n = 3: 79-104 / 4-6, n = 4: 131-168 / 3, n = 5: 189-206 / 2, n = 6 ... 8: 266-481 / 1 (the five
// n x n matrices of a step plus the carry spill into the accumulation registers, not to memory).  Staged path (n <= 4,
// plus the chunk's prefetch registers): n = 1: 76-114 / 4-6, n = 2: 125-180 / 2-4, n = 3: 261-357 / 1, n = 4: 255-343 / 1-2.
// The run-time-dimension kernel serves n > 8 and "force_generic" = 1.
//
// Unscented route (RTS_UNSC: sym_sqrt<N> and the 2 n sigma-point images before the step; strided path only -- the route is
// bound by the root's arithmetic, not by its loads).  The predictions are loaded after the root, when its 2 n^2 registers
// are free again; with that every instance n = 1 ... 8 builds without scratch, so the family's register limit of 8 holds
// here (BACKWARD_REG_MAX).
// VGPRs (arch + acc) / waves per SIMD: n = 1: 35 / 8, n = 2: 62 / 8, n = 3: 105 / 4, n = 4: 170 / 2, n = 5: 235 / 2,
// n = 6: 346 / 1, n = 7: 447 / 1, n = 8: 496 / 1.  Run-time-dimension kernel: rts_generic_kernel<true> 130 VGPRs, 3 waves per
// SIMD; rts_generic_kernel<false> (every other kind) 112 VGPRs, 4 waves, as before the route existed.
//
// Source route (RTS_EXT_USER: F_t from n dual-number evaluations of the caller's dynamics; kernels compiled at run time,
// jit_source.hip JIT_RTS_REGS / JIT_RTS_GENERIC).  Measured on a Lorenz-96 twin written as source (a loop over BF_N, dq = n),
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950, -ffp-contract=off: every instance n = 1 ... 8 builds without scratch,
// so the family's register limit of 8 (BACKWARD_REG_MAX) holds for that function; a caller's function with more live values
// may spill where this one does not.  VGPRs (arch + acc) / waves per SIMD, strided path: n = 1: 25 / 8, n = 2: 58 / 8,
// n = 3: 82 / 5, n = 4: 135 / 3, n = 5: 207 / 2, n = 6: 280 / 1, n = 7: 438 / 1, n = 8: 420 / 1; staged path: n = 1: 94 / 5,
// n = 2: 166 / 3, n = 3: 341 / 1, n = 4: 330 / 1.  Run-time-dimension kernel (lane d evaluates the function with the seed
// in state direction d; the per-lane arrays are BF_N long): n = 3: 87 VGPRs / 5 waves, n = 10: 101 / 4, n = 64: 281 / 1, no
// scratch.
#include "backward_host.hpp"

namespace bf {

// ---- run-time-dimension kernel -----------------------------------------------------------------------------------
// One 64-lane workgroup per trajectory.  LDS: five n x ld matrices (P, P^s, P-, X, W) and four vectors; RTS_UNSC: two more
// matrices (V, Rt) and the root's vectors -- the root's iterate and its Newton scratch alias W and X, dead until the solve --
// which bounds the route at n <= 75 in 160 KiB (the host computes it from rts_gen_lds_floats).  Per step, with
// the helpers of rts_generic.hpp: W <- F_t, X = F P, [recompute: P-, m-], W <- chol(P-), X <- L^-T L^-1 X,
// C = X^T P^s (straight to HBM), m^s <- m + X^T (m^s - m-), P^s <- P^s - P-, P- <- X^T (P^s), P <- P + P- X, swap P / P^s.
// RTS_UNSC: two more matrices (the root's eigenvectors and the root) and the root's vectors (rts_generic.hpp: RtsUnscLds)
template <bool UNSC>
__global__ void __launch_bounds__(64) rts_generic_kernel(RtsGen c, GenModel g, RtsViews v, long long T) {
  rts_generic_body<UNSC, false>(c, g, v, T);
}

// ---- host helpers --------------------------------------------------------------------------------------------------
// contiguous reference rows of `rows` steps, every row 16-byte aligned
static inline bool rts_ref_stream(const SView& s, long long E, long long rows) {
  return s.p == nullptr || (s.sE == 1 && s.sT == E && s.sB == rows * E && (reinterpret_cast<uintptr_t>(s.p) % 16 == 0) &&
                            (rows * E) % 4 == 0);
}

static Option g_rts_load_mode{-1, OPT_RTS_LOAD_MODE};
Option& rts_load_mode_option() { return g_rts_load_mode; }

// The data path of a register launch: staged for whole waves of contiguous reference rows (stage_ok: RtsStage<N>::OK), strided
// otherwise.  Without a carry the cross-covariances have T-1 entries: their rows may be T-1 steps long as well as T (the kernel
// takes the row pitch from the view and never touches entry T-1; rts_ref_stream's ((T-1) E) % 4 test keeps every row on 16 bytes)
static int rts_pick_path(int n, bool stage_ok, bool load_pred, const RtsViews& v, long long B, long long T, int load_mode, bool* staged) {
  const bool cs_ok = rts_ref_stream(v.Cs, n * n, T) || (v.m_in == nullptr && T > 1 && rts_ref_stream(v.Cs, n * n, T - 1));
  bool staged_ok = stage_ok && rts_ref_stream(v.m, n, T) && rts_ref_stream(v.P, n * n, T) && rts_ref_stream(v.ms, n, T) &&
                   rts_ref_stream(v.Ps, n * n, T) && cs_ok;
  if (load_pred) staged_ok = staged_ok && rts_ref_stream(v.pm, n, T) && rts_ref_stream(v.pP, n * n, T);
  if (load_mode == RTS_STAGED && !staged_ok)
    return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 and the contiguous reference layout with 16-byte aligned rows");
  *staged = staged_ok && load_mode != RTS_STRIDED && B >= 64;
  return BF_OK;
}

// the views of the trajectories from b_begin on
static RtsViews rts_shifted(const RtsViews& v, long long b_begin, int n) {
  RtsViews w = v;
  for (SView* s : {&w.m, &w.P, &w.pm, &w.pP, &w.ms, &w.Ps, &w.Cs}) if (s->p) s->p += b_begin * s->sB;
  if (w.m_in) w.m_in += b_begin * n;
  if (w.P_in) w.P_in += b_begin * n * n;
  if (w.m_out) w.m_out += b_begin * n;
  if (w.P_out) w.P_out += b_begin * n * n;
  if (w.u) w.u += b_begin * w.u_sB;
  return w;
}

// The smoother as a product of backward_dispatch (backward_host.hpp): the four launches of one call.  The data path -- staged
// or strided, "rts_load_mode" -- is the smoother's own business, with its refusals.
struct RtsProduct {
  const RtsViews& v;
  long long B, T;
  int load_mode;
  hipStream_t stream;

  template <int N, int KIND, class Arg>
  int regs(const Arg& c, const float* d_gqg) const {
    using S = RtsStage<N>;
    bool staged = false;
    const int rc = rts_pick_path(N, S::OK, KIND != RTS_LIN_RECOMPUTE, v, B, T, load_mode, &staged);
    if (rc != BF_OK) return rc;
    long long b_main = 0;
    if constexpr (S::OK && KIND != RTS_UNSC) {  // (the unscented route is compute-bound: strided loads only)
      if (staged) {
        // the staged kernel takes whole waves; a ragged remainder goes through the strided one
        b_main = (B / 64) * 64;
        hipLaunchKernelGGL((rts_reg_kernel<N, RTS_STAGED, KIND, Arg>), dim3((unsigned)(b_main / 64)), dim3(64),
                           sizeof(float) * S::FLOATS, stream, c, d_gqg, v, b_main, T);
      }
    }
    if (b_main < B) {
      const long long nb = B - b_main;
      hipLaunchKernelGGL((rts_reg_kernel<N, RTS_STRIDED, KIND, Arg>), dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, stream, c,
                         d_gqg, rts_shifted(v, b_main, N), nb, T);
    }
    BF_HIP_CHECK(hipGetLastError());
    return BF_OK;
  }

  // the register kernels compiled at run time around the caller's dynamics (jit_source.hip: JIT_RTS_REGS), one per data path
  int user_regs(const bf_user_model* um, int n, RtsUserHost& h) const {
    bool staged = false;
    size_t stage_bytes = 0;
    auto dims = [&](auto NC) -> int {
      using S = RtsStage<decltype(NC)::value>;
      stage_bytes = sizeof(float) * S::FLOATS;
      return rts_pick_path(decltype(NC)::value, S::OK, true, v, B, T, load_mode, &staged);
    };
    auto pick = [&]() -> int { BF_RTS_DIMS(n, dims) };
    int rc = pick();
    if (rc != BF_OK) return rc;
    long long b_main = 0, T_ = T;
    if (staged) {  // whole waves; a ragged remainder goes through the strided kernel, as in regs
      hipFunction_t fn = nullptr;
      if ((rc = user_kernel(um, JIT_RTS_REGS, RTS_STAGED, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
      b_main = (B / 64) * 64;
      RtsViews w = v;
      void* args[] = {&h, &w, &b_main, &T_};
      BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)(b_main / 64), 1, 1, 64, 1, 1, (unsigned)stage_bytes, stream, args, nullptr));
    }
    if (b_main < B) {
      hipFunction_t fn = nullptr;
      if ((rc = user_kernel(um, JIT_RTS_REGS, RTS_STRIDED, 0, JIT_SPEC_USER, &fn)) != BF_OK) return rc;
      long long nb = B - b_main;
      RtsViews w = rts_shifted(v, b_main, n);
      void* args[] = {&h, &w, &nb, &T_};
      BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)((nb + 63) / 64), 1, 1, 64, 1, 1, 0, stream, args, nullptr));
    }
    return BF_OK;
  }

  // the LDS bytes of the run-time-dimension kernel, which has the strided data path only
  int plan(const RtsGen& c, size_t* lds_bytes) const {
    if (load_mode == RTS_STAGED) return set_error(BF_EINVAL, "rts_load_mode = 2 needs n <= 4 on the register kernel");
    const size_t lds = sizeof(float) * rts_gen_lds_floats(c.n, c.kind);
    if (lds > 160 * 1024) {
      if (c.kind == RTS_UNSC) {
        int nmax = 1;
        while (sizeof(float) * rts_gen_lds_floats(nmax + 1, RTS_UNSC) <= 160 * 1024) ++nmax;
        return set_error(BF_EUNSUPPORTED, "unscented smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup: n <= %d)", c.n, lds, nmax);
      }
      return set_error(BF_EUNSUPPORTED, "smoother: n = %d needs %zu bytes of LDS (160 KiB per workgroup)", c.n, lds);
    }
    *lds_bytes = lds;
    return BF_OK;
  }

  int generic(const RtsGen& c0, const GenModel& g, const std::vector<float>& blk) const {
    size_t lds = 0;
    int rc = plan(c0, &lds);
    if (rc != BF_OK) return rc;
    RtsGen c = c0;
    GenModel gg = g;
    if ((rc = rts_gen_upload(c, gg, blk, stream)) != BF_OK) return rc;
    if (B > 0x7fffffffLL) return set_error(BF_EINVAL, "smoother: B too large for the run-time-dimension kernel");
    auto kern = c.kind == RTS_UNSC ? rts_generic_kernel<true> : rts_generic_kernel<false>;
    if (lds > 64 * 1024) BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), lds, stream, c, gg, v, T);
    BF_HIP_CHECK(hipGetLastError());
    return BF_OK;
  }

  int user_generic(const bf_model* p, const RtsGen& c0) const {  // (jit_source.hip: JIT_RTS_GENERIC)
    size_t lds = 0;
    const int rc = plan(c0, &lds);
    if (rc != BF_OK) return rc;
    RtsGen c = c0;
    RtsViews w = v;
    return backward_launch_user_generic(p, JIT_RTS_GENERIC, "smoother", &c, &w, B, T, lds, stream);
  }
};

// bf_out_desc / bf_smooth_carry / bf_smooth_desc -> RtsViews, with the checks the entry points share (the parallel-in-time
// smoother, rts_pscan.hip, among them)
int rts_views(const bf_out_desc* f, const bf_smooth_carry* carry, const bf_smooth_desc* out, const bf_cstream* u, bool need_pred,
              RtsViews& v) {
  if (!f->means.ptr || !f->covs.ptr) return set_error(BF_EINVAL, "filtered means and covariances are required");
  if (need_pred && (!f->pred_means.ptr || !f->pred_covs.ptr))
    return set_error(BF_EINVAL, "the extended and the unscented smoother need the predicted means and covariances");
  if (!out->means.ptr || !out->covs.ptr) return set_error(BF_EINVAL, "smoothed means and covariances are required outputs");
  if (carry && ((carry->m_in == nullptr) != (carry->P_in == nullptr)))
    return set_error(BF_EINVAL, "carry.m_in and carry.P_in are given together or not at all");
  if (carry && ((carry->m_out == nullptr) != (carry->P_out == nullptr)))
    return set_error(BF_EINVAL, "carry.m_out and carry.P_out are given together or not at all");
  std::memset(&v, 0, sizeof(v));
  v.m = make_sview(f->means);
  v.P = make_sview(f->covs);
  v.pm = make_sview(f->pred_means);
  v.pP = make_sview(f->pred_covs);
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
  return BF_OK;
}

int rts_run(const BackwardRoute& r, const RtsViews& v, long long B, long long T, void* stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return backward_dispatch(r, force_generic_option().load() != 0, RtsProduct{v, B, T, g_rts_load_mode.load(), s}, s);
}

}  // namespace bf

extern "C" {

int bf_smoother_abi_check(size_t sizeof_smooth_desc, size_t sizeof_smooth_carry) {
  BF_ABI_SIZE(sizeof_smooth_desc, bf_smooth_desc)
  BF_ABI_SIZE(sizeof_smooth_carry, bf_smooth_carry)
  return BF_OK;
}

int bf_rts_smoother_f32(const bf_lgssm* model, const bf_out_desc* filtered, int64_t B, int64_t T,
                        const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  int rc = bf::backward_check_lgssm(model);
  if (rc != BF_OK) return rc;
  const bool has_pm = filtered->pred_means.ptr != nullptr, has_pP = filtered->pred_covs.ptr != nullptr;
  if (has_pm != has_pP) return bf::set_error(BF_EINVAL, "pred_means and pred_covs are given together or not at all");
  const bool recompute = !has_pm;
  if (recompute && (rc = bf::backward_check_recompute(model, T)) != BF_OK) return rc;
  bf::RtsViews v;
  if ((rc = bf::rts_views(filtered, carry, out, nullptr, false, v)) != BF_OK) return rc;
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(model, recompute, r)) != BF_OK) return rc;
  return bf::rts_run(r, v, B, T, stream);
}

int bf_eks_smoother_f32(const bf_model* model, const bf_cstream* u, const bf_out_desc* filtered, int64_t B, int64_t T,
                        const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  int rc = bf::backward_check_source(model, "extended smoother", false);
  if (rc != BF_OK) return rc;
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if ((rc = bf::backward_check_dims(model)) != BF_OK) return rc;
  bf::RtsViews v;
  if ((rc = bf::rts_views(filtered, carry, out, u, true, v)) != BF_OK) return rc;
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(model, T, r)) != BF_OK) return rc;
  return bf::rts_run(r, v, B, T, stream);
}

int bf_uks_smoother_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* u, const bf_out_desc* filtered,
                        int64_t B, int64_t T, const bf_smooth_carry* carry, const bf_smooth_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !uparams || !filtered || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  int rc = bf::backward_check_source(model, "unscented smoother", true);
  if (rc != BF_OK) return rc;
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if ((rc = bf::backward_check_dims(model)) != BF_OK) return rc;
  bf::RtsViews v;
  if ((rc = bf::rts_views(filtered, carry, out, u, true, v)) != BF_OK) return rc;
  bf::BackwardRoute r;
  if ((rc = bf::backward_route(model, uparams, r)) != BF_OK) return rc;
  if (bf::g_rts_load_mode.load() == bf::RTS_STAGED)
    return bf::set_error(BF_EINVAL, "rts_load_mode = 2 is not offered on the unscented route");
  return bf::rts_run(r, v, B, T, stream);
}

}  // extern "C"
