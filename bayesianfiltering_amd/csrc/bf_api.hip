// C-ABI entry points (include/bayesfilt.h).  Validation and dispatch only; the kernels live in
// the kf_*/gsf_*/bpf_* translation units.  (The smoothers' and the samplers' entry points sit with
// their launchers: rts_smoother.hip, ffbs_sampler.hip, pf_sampler.hip.)
#include <cstring>
#include "bf_common.hpp"
#include "../../include/bayesfilt_ext2.h"
#include "forward_host.hpp"
#include "pscan_host.hpp"
#include "user_model.hpp"
#include "bf_rng.hpp"

namespace bf {

char* last_error_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

int launch_kf_group(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes);

int kf_missing_default_lanes(int n, int m);  // kf_scan_group.hip: 0 = the pair has no missing-observation instance
int launch_kf_missing_group(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                            const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes);

int launch_kf_mfma(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                   const bf_out_desc* out, hipStream_t stream, int K, bool multi, int dyn_kind, const float* dth);
int launch_kf_bf32(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry, const bf_out_desc* out,
                   hipStream_t stream, int K, bool multi, int dyn_kind, const float* dth, bool missing);   // missing: the MISSING = true twins (kf_scan_bf32_missing.hip)
int launch_kf_generic(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                      const bf_out_desc* out, hipStream_t stream, bool missing);   // missing: NaN observations are gaps (generic_scan_missing.hip)
int launch_gsf_generic(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                       const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool missing);
int launch_collapse(const bf_stream* w, const bf_stream* m, const bf_stream* P, long long B, long long T, int K, int n,
                    float* mean_out, float* cov_out, hipStream_t stream);
int launch_gsf_ekf(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                   const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes);

int launch_ugsf_ukf(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
                    long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream);
// the MISSING = true instances (gsf_scan.hip, ugsf_scan.hip)
int gsf_default_lanes(int n);
int launch_gsf_ekf_missing(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                           const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, int force_mode, int lanes);
int launch_gsf_user_regs_missing_impl(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                                      const bf_carry* carry, const bf_out_desc* out, hipStream_t stream);
int launch_ugsf_ukf_missing(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
                            long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream);
int launch_agsf_ekf(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, const int32_t nc[3],
                    const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out, int* d_leaf_idx,
                    int variant, hipStream_t stream);
int launch_agsf_ukf(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                    const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                    int* d_leaf_idx, int variant, hipStream_t stream);
int launch_optimal_resample(const float* d_w, const uint32_t key[2], long long B, int M, int N, int* d_idx, float* d_wout,
                            hipStream_t stream);
int launch_bpf(const bf_bpf_model* bp, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int NP,
               float ess, int resampler, const uint32_t key[2], const bf_bpf_carry* carry, const bf_bpf_out* o,
               hipStream_t stream, bool missing);   // missing: the MISSING = true kernels (NaN observations are gaps)
int launch_sample_ssm(const bf_bpf_model* bp, const uint32_t* d_keys, const bf_cstream* u, long long B, long long T,
                      float* d_states, float* d_emis, hipStream_t stream);
int launch_resample(const float* d_w, const uint32_t* d_keys, long long B, int NP, int resampler, int* d_idx,
                    hipStream_t stream);

CallOverrides& call_overrides() {
  static thread_local CallOverrides c = {};
  return c;
}

// tuning options: process-wide defaults (atomics) with per-call overrides (bf_common.hpp: Option)
extern Option g_bpf_variant;
extern Option g_bpf_hbm_mode;
extern Option g_bpf_spec;
extern Option g_bpf_arith;
extern Option g_gsf_structured;
extern Option g_ugsf_force_generic;   // ugsf_generic.hip
extern Option g_agsf_force_generic;   // agsf_generic.hip
static Option g_kf_emit_mode{-1, OPT_KF_EMIT_MODE};  // -1 = choose from the layout
static Option g_kf_lanes{0, OPT_KF_LANES};       // 0 = default lanes per trajectory for the (n, m) pair
// op 0 log, 1 exp, 2 bits -> normal, 3 sin, 4 cos, 5 atan2(in[i], in[n + i])
__host__ __device__ inline float canon_eval_one(int op, const float* in, long long n, long long i) {
  const float x = in[i];
  float s, c;
  switch (op) {
    case 0: return canon_log(x);
    case 1: return canon_exp(x);
    case 2: return bits_to_normal(canon_f_bits(x));
    case 3: canon_sincos(x, &s, &c); return s;
    case 4: canon_sincos(x, &s, &c); return c;
    default: return canon_atan2(x, in[n + i]);
  }
}
__global__ void canon_eval_kernel(int op, const float* __restrict__ in, long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = canon_eval_one(op, in, n, i);
}

Option& rts_load_mode_option();  // rts_smoother.hip: -1 = from the layout, 0 = strided, 2 = LDS-staged
static Option g_kf_small_mode{1, OPT_KF_SMALL_MODE};   // bf_set_option "kf_small_mode": 1 = one-wave matrix-core kernel for 9 <= n <= 32 (default), 0 = off
static Option g_force_generic{0, OPT_FORCE_GENERIC};  // 1 = run the run-time-dimension kernel even where a compiled instance exists
Option& force_generic_option() { return g_force_generic; }  // read by the backward family's entry points (backward_host.hpp)

// The shapes of the one-wave matrix-core kernel (kf_scan_bf32.hip) -- 9 <= n <= 32, m <= 32 and (n >= 16 or m > 8) -- unless
// "kf_small_mode" is 0
static bool kf_small_tiles(int n, int m) { return n >= 9 && n <= 32 && m <= 32 && (n >= 16 || m > 8) && g_kf_small_mode.load() != 0; }

// A Gaussian-sum model the matrix-core Kalman kernels can run as K chains of a linear model: a linear emission, no legacy class,
// K <= 64 and either linear dynamics or registry dynamics with an analytic, sparse Jacobian and identity noise input
// (dyn_kind 1 = Lorenz-96, 2 = sine: extended Kalman chains on the one-wave kernel).  `lg` points into the model's arrays.
struct GsfTiles {
  bool linear;
  bf_lgssm lg;
  int dyn_kind;
  float dth[8];
};
static GsfTiles gsf_tiles(const bf_model* model, int K) {
  GsfTiles t;
  std::memset(&t, 0, sizeof(t));
  const bool lin_emi = model->emi_id == 0 && model->n_emi_theta == model->m * model->n + model->m * model->dr;
  const bool lin_dyn = model->dyn_id == 0 && model->n_dyn_theta == model->n * model->n + model->n * model->dq;
  t.dyn_kind = (model->dyn_id == 1 && model->n_dyn_theta == 5 && model->dq == model->n) ? 1
             : (model->dyn_id == 4 && model->n_dyn_theta == 1 && model->dq == model->n) ? 2 : 0;
  t.linear = lin_emi && model->flags == 0 && K <= 64 && (lin_dyn || t.dyn_kind != 0);
  if (!t.linear) return t;
  bf_lgssm& lg = t.lg;
  lg.n = model->n; lg.dq = model->dq; lg.m = model->m; lg.dr = model->dr;
  if (lin_dyn) { lg.A = model->dyn_theta; lg.G = model->dyn_theta + model->n * model->n; t.dyn_kind = 0; }
  lg.H = model->emi_theta; lg.D = model->emi_theta + model->m * model->n;
  lg.q0 = model->q0; lg.r0 = model->r0; lg.Q = model->Q; lg.R = model->R;
  lg.Q_steps = model->Q_steps > 0 ? model->Q_steps : 1; lg.R_steps = model->R_steps > 0 ? model->R_steps : 1;
  if (!lin_dyn) for (int i = 0; i < model->n_dyn_theta && i < 8; ++i) t.dth[i] = model->dyn_theta[i];
  return t;
}
Option& ffbs_spl_option();  // ffbs_sampler.hip: 0 = from S and n, else samples per lane of the register kernel
Option& pkf_block_option();  // kf_pscan.hip: 0 = from (B, T), else the block length of the parallel-in-time Kalman filter
Option& prs_block_option();  // rts_pscan.hip: 0 = from (B, T), else the block length of the parallel-in-time RTS smoother
Option& pfs_block_option();  // ffbs_pscan.hip: 0 = from (B, S, T), else the block length of the parallel-in-time posterior sampler
long long kf_pscan_workspace_bytes(int n, int m, long long B, long long T, int block);
int launch_kf_pscan(const bf_lgssm* model, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                    const bf_out_desc* out, void* workspace, long long workspace_bytes, hipStream_t stream, bool missing);

// A shape / option the compiled instances do not cover falls through to the run-time-dimension kernel
// (generic_scan.hip); if that cannot run it either, both reasons are reported.
template <class F>
static int with_generic_fallback(int rc, F&& generic) {
  if (rc != BF_EUNSUPPORTED) return rc;
  char first[512];
  std::snprintf(first, sizeof(first), "%s", last_error_buf());
  const int rc2 = generic();
  if (rc2 == BF_OK) return BF_OK;
  char second[512];
  std::snprintf(second, sizeof(second), "%s", last_error_buf());
  return set_error(rc2, "%.240s; generic kernel: %.240s", first, second);
}

}  // namespace bf

extern "C" {

int bf_version(void) { return BF_VERSION; }

int bf_abi_check(int32_t header_version, size_t sizeof_out_desc, size_t sizeof_lgssm, size_t sizeof_model,
                 size_t sizeof_bpf_model, size_t sizeof_bpf_out) {
  if (header_version / 100 != BF_VERSION / 100)
    return bf::set_error(BF_EINVAL, "binding was written against header version %d, the library is %d", (int)header_version, BF_VERSION);
  BF_ABI_SIZE(sizeof_out_desc, bf_out_desc)
  BF_ABI_SIZE(sizeof_lgssm, bf_lgssm)
  BF_ABI_SIZE(sizeof_model, bf_model)
  BF_ABI_SIZE(sizeof_bpf_model, bf_bpf_model)
  BF_ABI_SIZE(sizeof_bpf_out, bf_bpf_out)
  return BF_OK;
}

const char* bf_last_error(void) { return bf::last_error_buf(); }

int bf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

static int set_option_impl(const char* name, int value, bool this_call_only) {
  // {name, the option, which values it takes, what a refusal says}
  struct Row {
    const char* name;
    bf::Option& option;
    bool (*accept)(int);
    const char* message;
  };
  const auto flag = [](int v) { return v == 0 || v == 1; };
  const auto pscan_block = [](int v) { return v == 0 || (v >= bf::PSCAN_L_MIN && v <= bf::PSCAN_L_MAX); };
  static_assert(bf::PSCAN_L_MIN == 4 && bf::PSCAN_L_MAX == 4096, "the *_block messages below spell the limits out");
  const Row rows[] = {
      {"kf_emit_mode", bf::g_kf_emit_mode, [](int v) { return v >= -1 && v <= 2; }, "kf_emit_mode must be -1..2"},
      {"kf_lanes", bf::g_kf_lanes, [](int v) { return v >= 0 && v <= 64 && (v & (v - 1)) == 0; }, "kf_lanes must be 0 or a power of two <= 64"},
      {"kf_small_mode", bf::g_kf_small_mode, flag, "kf_small_mode must be 0 or 1"},
      {"force_generic", bf::g_force_generic, flag, "force_generic must be 0 or 1"},
      {"ugsf_force_generic", bf::g_ugsf_force_generic, flag, "ugsf_force_generic must be 0 or 1"},
      {"agsf_force_generic", bf::g_agsf_force_generic, flag, "agsf_force_generic must be 0 or 1"},
      {"rts_load_mode", bf::rts_load_mode_option(), [](int v) { return v == -1 || v == 0 || v == 2; }, "rts_load_mode must be -1, 0 or 2"},
      {"ffbs_spl", bf::ffbs_spl_option(), [](int v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8; }, "ffbs_spl must be 0, 1, 2, 4 or 8"},
      {"pkf_block", bf::pkf_block_option(), pscan_block, "pkf_block must be 0 or 4..4096"},
      {"prs_block", bf::prs_block_option(), pscan_block, "prs_block must be 0 or 4..4096"},
      {"pfs_block", bf::pfs_block_option(), pscan_block, "pfs_block must be 0 or 4..4096"},
      {"gsf_structured", bf::g_gsf_structured, flag, "gsf_structured must be 0 or 1"},
      {"bpf_variant", bf::g_bpf_variant, flag, "bpf_variant must be 0 or 1"},
      {"bpf_hbm_mode", bf::g_bpf_hbm_mode, [](int v) { return v >= 0 && v <= 2; }, "bpf_hbm_mode must be 0, 1 or 2"},
      {"bpf_arith", bf::g_bpf_arith, flag, "bpf_arith must be 0 or 1"},
      {"bpf_spec", bf::g_bpf_spec, flag, "bpf_spec must be 0 or 1"},
  };
  for (const Row& r : rows) {
    if (!name || std::strcmp(name, r.name) != 0) continue;
    if (!r.accept(value)) return bf::set_error(BF_EINVAL, "%s", r.message);
    if (this_call_only) {
      bf::CallOverrides& c = bf::call_overrides();
      c.value[r.option.id] = value;
      c.armed[r.option.id] = true;
    } else {
      r.option = value;
    }
    return BF_OK;
  }
  return bf::set_error(BF_EINVAL, "unknown option '%s'", name ? name : "(null)");
}

int bf_set_option(const char* name, int value) { return set_option_impl(name, value, false); }

int bf_set_call_option(const char* name, int value) { return set_option_impl(name, value, true); }

int64_t bf_bytes_per_step(int32_t n, int32_t m, int32_t K, const bf_out_desc* out) {
  int64_t per = 0;
  if (!out) {
    per = 1 + 2 * (int64_t)n + 2 * (int64_t)n * n;
  } else {
    if (out->weights.ptr) per += 1;
    if (out->means.ptr) per += n;
    if (out->covs.ptr) per += (int64_t)n * n;
    if (out->pred_means.ptr) per += n;
    if (out->pred_covs.ptr) per += (int64_t)n * n;
    if (out->loglik.ptr) per += 1;
  }
  int64_t once = 0;  // collapsed streams: one Gaussian per step whatever K is
  if (out && out->coll_mean.ptr) once += n;
  if (out && out->coll_cov.ptr) once += (int64_t)n * n;
  return 4 * (int64_t)m + 4 * (int64_t)K * per + 4 * once;
}

int bf_kalman_filter_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                         const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (out && (out->coll_mean.ptr || out->coll_cov.ptr))
    return bf::set_error(BF_EINVAL, "collapsed streams are produced by bf_gsf_ekf_f32 (with one component they equal means / covs)");
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (int rc; (rc = bf::check_lgssm(model)) || (rc = bf::check_streams(y, carry))) return rc;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  auto generic = [&]() { return bf::launch_kf_generic(model, y, B, T, carry, out, hs, false); };
  if (bf::g_force_generic.load()) return generic();
  // dense products large enough for the matrix cores: (64, 32) itself and, zero-padded into its tiles, every model from
  // n = 24 up (4.9e7 steps/s whatever the size; the run-time-dimension kernel does 3.8e7 at n = 24, 1.6e7 at 32, 1.2e6 at 64)
  // 9 <= n <= 32: one wave per trajectory on single 32 x 32 tiles, 1.8e8 steps/s whatever the size; the run-time-dimension
  // kernel is faster only for the smallest of them (n = 12, m = 4: 1.7e8; n = 16, m = 8: 1.0e8; (32, 32): 3.5e6)
  if (bf::kf_small_tiles(model->n, model->m))
    return bf::with_generic_fallback(bf::launch_kf_bf32(model, y, B, T, carry, out, hs, 1, false, 0, nullptr, false), generic);
  if (model->n >= 24 && model->n <= 64 && model->m <= 32)
    return bf::with_generic_fallback(bf::launch_kf_mfma(model, y, B, T, carry, out, hs, 1, false, 0, nullptr), generic);
  return bf::with_generic_fallback(
      bf::launch_kf_group(model, y, B, T, carry, out, hs, bf::g_kf_emit_mode.load(), bf::g_kf_lanes.load()), generic);
}

int bf_kalman_filter_missing_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                                 const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: collapsed streams are not produced (with one component they equal means / covs)");
  if (int rc; (rc = bf::check_lgssm(model)) || (rc = bf::check_streams(y, carry))) return rc;
  // the register kernels only: no matrix-core or run-time-dimension instance takes gaps
  if (model->n > 8 || model->m > 4)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: n <= 8 and m <= 4 only (n=%d, m=%d)", (int)model->n,
                         (int)model->m);
  const int lanes = bf::g_kf_lanes.load();
  const int have = bf::kf_missing_default_lanes(model->n, model->m);
  if (have == 0)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: (n=%d, m=%d) is not compiled in (n = 1..8 with m = 1..min(n,4))",
                         (int)model->n, (int)model->m);
  if (lanes != 0 && lanes != have)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: kf_lanes=%d has no instance at (n=%d, m=%d); the compiled one is %d (or 0)",
                         lanes, (int)model->n, (int)model->m, have);
  return bf::launch_kf_missing_group(model, y, B, T, carry, out, static_cast<hipStream_t>(stream), bf::g_kf_emit_mode.load(), lanes);
}

int64_t bf_kalman_pscan_workspace_bytes(int32_t n, int32_t m, int64_t B, int64_t T, int32_t block) {
  return bf::kf_pscan_workspace_bytes(n, m, B, T, block);
}

int bf_kalman_filter_pscan_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                               const bf_out_desc* out, void* workspace, int64_t workspace_bytes, void* stream) {
  bf::CallOptionScope call_option_scope;
  return bf::launch_kf_pscan(model, y, B, T, carry, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), false);
}

int bf_kalman_filter_pscan_missing_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                                       const bf_out_desc* out, void* workspace, int64_t workspace_bytes, void* stream) {
  bf::CallOptionScope call_option_scope;
  return bf::launch_kf_pscan(model, y, B, T, carry, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), true);
}

int bf_gsf_ekf_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                   const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry))) return rc;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  auto generic = [&]() { return bf::launch_gsf_generic(model, y, u, B, T, K, carry, out, hs, false); };
  if (model->user && bf::g_force_generic.load() == 0 && bf::gsf_user_regs_eligible(model, K, out))   // from source, n <= 8: state in registers
    return bf::launch_gsf_user_regs_impl(model, y, u, B, T, K, carry, out, hs);
  if (model->user || model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER) return generic();  // compiled from source
  if (bf::g_force_generic.load()) return generic();
  // a LINEAR model beyond the register kernels (n >= 9): the Gaussian-sum filter's K components take turns on the matrix-core
  // kernels (bf16 three-term products: one wave per trajectory on single 32 x 32 tiles up to n = 32, four waves on 64 x 64 up
  // to n = 64), per-step Q_t / R_t tables included
  const bf::GsfTiles tl = bf::gsf_tiles(model, K);
  const bool small_tiles = bf::kf_small_tiles(model->n, model->m);
  const bool big_tiles = !small_tiles && model->n >= 24 && model->n <= 64 && model->m <= 32;
  if (tl.linear && !out->coll_mean.ptr && !out->coll_cov.ptr && (small_tiles || big_tiles)) {
    const bool multi = tl.dyn_kind != 0 || K > 1;
    const float* dth = tl.dyn_kind != 0 ? tl.dth : nullptr;
    if (small_tiles) return bf::with_generic_fallback(bf::launch_kf_bf32(&tl.lg, y, B, T, carry, out, hs, K, multi, tl.dyn_kind, dth, false), generic);
    return bf::with_generic_fallback(bf::launch_kf_mfma(&tl.lg, y, B, T, carry, out, hs, K, multi, tl.dyn_kind, dth), generic);   // 33 <= n <= 64: four waves per trajectory
  }
  return bf::with_generic_fallback(
      bf::launch_gsf_ekf(model, y, u, B, T, K, carry, out, hs, bf::g_kf_emit_mode.load(), bf::g_kf_lanes.load()), generic);
}

int bf_ugsf_ukf_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u,
                    int64_t B, int64_t T, int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !uparams || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry)) || (rc = bf::check_alpha(uparams))) return rc;
  return bf::launch_ugsf_ukf(model, uparams, y, u, B, T, K, carry, out, static_cast<hipStream_t>(stream));
}

// Missing observations (NaN entries of y) on the register kernels of the two Gaussian-sum filters.  Both entry points refuse,
// before their first HIP call, whatever the plain route would hand to a kernel that reads a NaN as poison: there is no fallback.
int bf_gsf_ekf_missing_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                           const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  static const char* const who = "gaussian-sum filter with missing observations";
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry))) return rc;
  if (model->flags != 0) return bf::set_error(BF_EUNSUPPORTED, "%s: the legacy classes (flags != 0) are not served", who);
  if (bf::g_force_generic.load())
    return bf::set_error(BF_EUNSUPPORTED, "%s: force_generic is set, and the run-time-dimension kernel takes no gaps", who);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (model->user) {   // functions from source: the register kernel built at run time, or nothing
    if (model->n > 8 || model->dq > 8 || model->m > 8 || model->dr > 8)
      return bf::set_error(BF_EUNSUPPORTED, "%s: models from source need every dimension <= 8 (n=%d, dq=%d, m=%d, dr=%d)", who,
                           (int)model->n, (int)model->dq, (int)model->m, (int)model->dr);
    if (K > 256) return bf::set_error(BF_EUNSUPPORTED, "%s: models from source take at most 256 components (K=%d)", who, (int)K);
    if (out->coll_mean.ptr || out->coll_cov.ptr)
      return bf::set_error(BF_EUNSUPPORTED, "%s: models from source produce no collapsed streams", who);
    if (!bf::gsf_user_regs_eligible(model, K, out))
      return bf::set_error(BF_EUNSUPPORTED, "%s: this model from source is not eligible for the register kernel (a log-density, or a "
                                            "nonlinear registry function beside one from source)", who);
    return bf::launch_gsf_user_regs_missing_impl(model, y, u, B, T, K, carry, out, hs);
  }
  if (model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER)
    return bf::set_error(BF_EINVAL, "dyn_id / emi_id = BF_FN_USER needs bf_model.user (bf_user_model_create)");
  // the register kernels only: no matrix-core or run-time-dimension instance takes gaps
  if (model->n > 8 || model->m > 4)
    return bf::set_error(BF_EUNSUPPORTED, "%s: n <= 8 and m <= 4 only (n=%d, m=%d)", who, (int)model->n, (int)model->m);
  const int lanes = bf::g_kf_lanes.load();
  if (lanes != 0 && lanes != bf::gsf_default_lanes(model->n))
    return bf::set_error(BF_EUNSUPPORTED, "%s: kf_lanes=%d is not served at n=%d; the compiled default is %d (or 0)", who, lanes,
                         (int)model->n, bf::gsf_default_lanes(model->n));
  return bf::launch_gsf_ekf_missing(model, y, u, B, T, K, carry, out, hs, bf::g_kf_emit_mode.load(), lanes);
}

int bf_ugsf_ukf_missing_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u,
                            int64_t B, int64_t T, int32_t K, const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  static const char* const who = "unscented gaussian-sum filter with missing observations";
  if (!model || !uparams || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry)) || (rc = bf::check_alpha(uparams))) return rc;
  if (model->flags != 0) return bf::set_error(BF_EUNSUPPORTED, "%s: the legacy classes (flags != 0) are not served", who);
  if (bf::g_ugsf_force_generic.load())
    return bf::set_error(BF_EUNSUPPORTED, "%s: ugsf_force_generic is set, and the run-time-dimension kernel takes no gaps", who);
  if (model->n > 8 || model->dq > 8 || model->m > 8 || model->dr > 8)
    return bf::set_error(BF_EUNSUPPORTED, "%s: every dimension <= 8 only (n=%d, dq=%d, m=%d, dr=%d)", who, (int)model->n,
                         (int)model->dq, (int)model->m, (int)model->dr);
  if (K > 256) return bf::set_error(BF_EUNSUPPORTED, "%s: at most 256 components (K=%d)", who, (int)K);
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "%s: collapsed streams are produced by bf_gsf_ekf_missing_f32 only", who);
  if (!model->user && (model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER))
    return bf::set_error(BF_EINVAL, "dyn_id / emi_id = BF_FN_USER needs bf_model.user (bf_user_model_create)");
  if (model->user && model->user->has_lp)
    return bf::set_error(BF_EINVAL, "a log-density from source belongs to the particle filter, not to the unscented filter");
  return bf::launch_ugsf_ukf_missing(model, uparams, y, u, B, T, K, carry, out, static_cast<hipStream_t>(stream));
}

// Missing observations at any dimension (include/bayesfilt_ext.h): always the run-time-dimension kernel, MISSING = true
// (generic_scan_missing.hip).  "force_generic" is what these two are, so it changes nothing.  The LDS capacity is the last
// refusal, made by launch_gsf_generic before its first HIP call.
int bf_kalman_filter_missing_anydim_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                                        const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (int rc; (rc = bf::check_lgssm(model)) || (rc = bf::check_streams(y, carry))) return rc;
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: collapsed streams are not produced (with one component they equal means / covs)");
  return bf::launch_kf_generic(model, y, B, T, carry, out, static_cast<hipStream_t>(stream), true);
}

int bf_gsf_ekf_missing_anydim_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                                  const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  static const char* const who = "gaussian-sum filter with missing observations (run-time dimensions)";
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry))) return rc;
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "%s: collapsed streams inside the scan need a compiled instance; use bf_collapse_f32 on the emitted streams", who);
  if (model->flags != 0) return bf::set_error(BF_EUNSUPPORTED, "%s: the legacy classes (flags != 0) are not served", who);
  if (model->user && !model->user->has_dyn && !model->user->has_emi)
    return bf::set_error(BF_EINVAL, "%s: bf_model.user carries only a log-density, which belongs to the particle filter", who);
  return bf::launch_gsf_generic(model, y, u, B, T, K, carry, out, static_cast<hipStream_t>(stream), true);
}

// Missing observations on the one-wave matrix-core kernel (include/bayesfilt_ext2.h): where the plain twin would take that
// kernel, its MISSING = true instance; everywhere else -- and when that launch answers BF_EUNSUPPORTED -- the two entry points
// above, refusal for refusal and bit for bit.
int bf_kalman_filter_missing_tiles_f32(const bf_lgssm* model, const bf_cstream* y, int64_t B, int64_t T, const bf_carry* carry,
                                       const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive (B=%lld, T=%lld)", (long long)B, (long long)T);
  if (int rc; (rc = bf::check_lgssm(model)) || (rc = bf::check_streams(y, carry))) return rc;
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "kalman filter with missing observations: collapsed streams are not produced (with one component they equal means / covs)");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  auto generic = [&]() { return bf::launch_kf_generic(model, y, B, T, carry, out, hs, true); };
  if (bf::g_force_generic.load() == 0 && bf::kf_small_tiles(model->n, model->m))
    return bf::with_generic_fallback(bf::launch_kf_bf32(model, y, B, T, carry, out, hs, 1, false, 0, nullptr, true), generic);
  return generic();
}

int bf_gsf_ekf_missing_tiles_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t K,
                                 const bf_carry* carry, const bf_out_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  static const char* const who = "gaussian-sum filter with missing observations (run-time dimensions)";
  if (!model || !y || !carry || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return bf::set_error(BF_EINVAL, "B, T and K must be positive");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry))) return rc;
  if (out->coll_mean.ptr || out->coll_cov.ptr)
    return bf::set_error(BF_EUNSUPPORTED, "%s: collapsed streams inside the scan need a compiled instance; use bf_collapse_f32 on the emitted streams", who);
  if (model->flags != 0) return bf::set_error(BF_EUNSUPPORTED, "%s: the legacy classes (flags != 0) are not served", who);
  if (model->user && !model->user->has_dyn && !model->user->has_emi)
    return bf::set_error(BF_EINVAL, "%s: bf_model.user carries only a log-density, which belongs to the particle filter", who);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  auto generic = [&]() { return bf::launch_gsf_generic(model, y, u, B, T, K, carry, out, hs, true); };
  const bool from_source = model->user || model->dyn_id == BF_FN_USER || model->emi_id == BF_FN_USER;
  if (!from_source && bf::g_force_generic.load() == 0 && bf::kf_small_tiles(model->n, model->m)) {
    const bf::GsfTiles tl = bf::gsf_tiles(model, K);
    if (tl.linear)
      return bf::with_generic_fallback(bf::launch_kf_bf32(&tl.lg, y, B, T, carry, out, hs, K, tl.dyn_kind != 0 || K > 1, tl.dyn_kind,
                                                          tl.dyn_kind != 0 ? tl.dth : nullptr, true), generic);
  }
  return generic();
}

int bf_agsf_ekf_f32(const bf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T,
                    const int32_t num_components[3], const uint32_t key[2], const float opt_args[2], const bf_carry* carry,
                    const bf_out_desc* out, int32_t* leaf_idx, int32_t variant, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (variant < 0 || variant > 2)
    return bf::set_error(BF_EINVAL, "variant must be 0 (speedy), 1 (container branches) or 2 (container branches + optimal resampling)");
  if (!model || !y || !carry || !out || !num_components || !key || !opt_args) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive");
  if (num_components[0] <= 0 || num_components[1] <= 0 || num_components[2] <= 0)
    return bf::set_error(BF_EINVAL, "num_components must be three positive counts");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_noise_steps(model->Q_steps, model->R_steps)) || (rc = bf::check_streams(y, carry)))
    return rc;
  return bf::launch_agsf_ekf(model, y, u, B, T, num_components, key, opt_args, carry, out, leaf_idx, variant,
                             static_cast<hipStream_t>(stream));
}

int bf_agsf_ukf_f32(const bf_model* model, const bf_ukf_params* uparams, const bf_cstream* y, const bf_cstream* u, int64_t B,
                    int64_t T, const int32_t num_components[3], const uint32_t key[2], const float opt_args[2],
                    const bf_carry* carry, const bf_out_desc* out, int32_t* leaf_idx, int32_t variant, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (variant != 0 && variant != 1) return bf::set_error(BF_EINVAL, "variant must be 0 (speedy) or 1 (container branches)");
  if (!model || !uparams || !y || !carry || !out || !num_components || !key || !opt_args) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive");
  if (num_components[0] <= 0 || num_components[1] <= 0 || num_components[2] <= 0)
    return bf::set_error(BF_EINVAL, "num_components must be three positive counts");
  if (int rc; (rc = bf::check_model(model)) || (rc = bf::check_streams(y, carry)) || (rc = bf::check_alpha(uparams))) return rc;
  return bf::launch_agsf_ukf(model, uparams, y, u, B, T, num_components, key, opt_args, carry, out, leaf_idx, variant,
                             static_cast<hipStream_t>(stream));
}

int bf_optimal_resample_f32(const float* d_weights, const uint32_t key[2], int64_t B, int32_t M, int32_t N, int32_t* d_idx,
                            float* d_weights_out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!d_weights || !key || !d_idx || !d_weights_out) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || M <= 0) return bf::set_error(BF_EINVAL, "B and M must be positive");
  return bf::launch_optimal_resample(d_weights, key, B, M, N, d_idx, d_weights_out, static_cast<hipStream_t>(stream));
}

int bf_collapse_f32(const bf_stream* weights, const bf_stream* means, const bf_stream* covs, int64_t B, int64_t T,
                    int32_t K, int32_t n, float* mean_out, float* cov_out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!weights || !means || !weights->ptr || !means->ptr) return bf::set_error(BF_EINVAL, "weights and means are required");
  if (cov_out && (!covs || !covs->ptr)) return bf::set_error(BF_EINVAL, "cov_out needs the covariance stream");
  if (B <= 0 || T <= 0 || K <= 0 || n <= 0) return bf::set_error(BF_EINVAL, "non-positive size");
  if (!mean_out && !cov_out) return bf::set_error(BF_EINVAL, "nothing to compute");
  return bf::launch_collapse(weights, means, covs, B, T, K, n, mean_out, cov_out, static_cast<hipStream_t>(stream));
}

// the argument checks of the two particle-filter entry points, before any HIP call
static int check_bpf_call(const bf_bpf_model* model, const bf_cstream* y, int64_t B, int64_t T, int32_t N, const uint32_t key[2],
                          int32_t resampler, const bf_bpf_carry* carry, const bf_bpf_out* out) {
  if (!model || !y || !out || !key) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0 || N <= 0) return bf::set_error(BF_EINVAL, "B, T and N must be positive");
  if (!y->ptr) return bf::set_error(BF_EINVAL, "observations pointer is NULL");
  if (!model->ssm.Q || !model->m0 || !model->P0 || !model->lp_cov) return bf::set_error(BF_EINVAL, "Q, m0, P0, lp_cov are required");
  if (resampler != 0 && resampler != 1) return bf::set_error(BF_EINVAL, "resampler must be 0 (multinomial) or 1 (systematic)");
  if (carry && carry->x_in && !carry->w_in) return bf::set_error(BF_EINVAL, "carry.x_in needs carry.w_in");
  return BF_OK;
}

int bf_bpf_f32(const bf_bpf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t N,
               const uint32_t key[2], float ess_threshold, int32_t resampler, const bf_bpf_carry* carry,
               const bf_bpf_out* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (int rc = check_bpf_call(model, y, B, T, N, key, resampler, carry, out)) return rc;
  return bf::launch_bpf(model, y, u, B, T, N, ess_threshold, resampler, key, carry, out, static_cast<hipStream_t>(stream), false);
}

// Missing observations (NaN entries of y) on every route of the particle filter: the same dispatch, the MISSING = true kernels.
int bf_bpf_missing_f32(const bf_bpf_model* model, const bf_cstream* y, const bf_cstream* u, int64_t B, int64_t T, int32_t N,
                       const uint32_t key[2], float ess_threshold, int32_t resampler, const bf_bpf_carry* carry,
                       const bf_bpf_out* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (int rc = check_bpf_call(model, y, B, T, N, key, resampler, carry, out)) return rc;
  return bf::launch_bpf(model, y, u, B, T, N, ess_threshold, resampler, key, carry, out, static_cast<hipStream_t>(stream), true);
}

int bf_sample_ssm_f32(const bf_bpf_model* model, const uint32_t* d_keys, const bf_cstream* u, int64_t B, int64_t T,
                      float* d_states, float* d_emissions, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !d_keys || (!d_states && !d_emissions)) return bf::set_error(BF_EINVAL, "NULL argument");
  if (B <= 0 || T <= 0) return bf::set_error(BF_EINVAL, "B and T must be positive");
  if (!model->ssm.Q || !model->ssm.R || !model->m0 || !model->P0) return bf::set_error(BF_EINVAL, "Q, R, m0, P0 are required");
  return bf::launch_sample_ssm(model, d_keys, u, B, T, d_states, d_emissions, static_cast<hipStream_t>(stream));
}

int bf_resample_f32(const float* d_w, const uint32_t* d_keys, int64_t B, int32_t N, int32_t resampler, int32_t* d_idx,
                    void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!d_w || !d_keys || !d_idx || B <= 0 || N <= 0) return bf::set_error(BF_EINVAL, "bad argument");
  return bf::launch_resample(d_w, d_keys, B, N, resampler, d_idx, static_cast<hipStream_t>(stream));
}

int bf_canon_eval_f32(int32_t op, const float* in, int64_t n, float* out, int32_t on_device, void* stream) {
  if (op < 0 || op > 5 || !in || !out || n < 0) return bf::set_error(BF_EINVAL, "bad argument");
  if (n == 0) return BF_OK;
  if (!on_device) {
    for (int64_t i = 0; i < n; ++i) out[i] = bf::canon_eval_one(op, in, n, i);
    return BF_OK;
  }
  hipLaunchKernelGGL(bf::canon_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), op, in, n, out);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

int bf_random_normal_f32(const uint32_t key[2], int64_t count, float* host_out) {
  if (!key || !host_out || count < 0 || count > 0x7fffffff) return bf::set_error(BF_EINVAL, "bad argument");
  for (int64_t i = 0; i < count; ++i)
    host_out[i] = bf::bits_to_normal(bf::threefry_bits(key[0], key[1], (uint32_t)i, (uint32_t)count));
  return BF_OK;
}

int bf_random_split(const uint32_t key[2], int64_t num, uint32_t* host_out) {
  if (!key || !host_out || num <= 0 || num > 0x3fffffff) return bf::set_error(BF_EINVAL, "bad argument");
  for (int64_t i = 0; i < num; ++i) {
    const bf::U32x2 k = bf::threefry_split(key[0], key[1], (uint32_t)i, (uint32_t)num);
    host_out[2 * i] = k.x;
    host_out[2 * i + 1] = k.y;
  }
  return BF_OK;
}

}  // extern "C"
