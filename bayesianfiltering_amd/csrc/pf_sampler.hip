// Host side of the particle smoother (pf_sampler.hpp): the C entry points, the checks, the model block (float64 Cholesky of
// F_q Q F_q^T and its inverse) and the instances of the backward kernel: n = 1 ... 16 x {16, 64} register rows per lane.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: no instance uses scratch.  VGPRs / waves per SIMD, range over
// n = 1 ... 16: 16 rows (N <= 1024, up to 16 samples per workgroup) 62-122 / 4-7; 64 rows (N <= 4096, up to 8 samples per
// workgroup) 107-174 / 2-4; the genealogy kernel 23 / 8.  The table per n is in DESIGN.md section 6c.
#include "pf_sampler.hpp"

namespace bf {

template <int N, int RMAX, int WAVES>
static int launch_pfs_inst(const PfsModel<N>& m, const PfsViews& v, long long B, long long T, int NP, int S, hipStream_t stream) {
  // samples per workgroup: all WAVES when the grid fills the device anyway, fewer (f is then evaluated once per smaller
  // group) when trajectories are few; a sample's arithmetic does not depend on it
  int wpb = WAVES < S ? WAVES : S;
  while (wpb > 4 && B * ((S + wpb - 1) / wpb) < 512) wpb = (wpb + 1) / 2;
  const long long groups = (S + wpb - 1) / wpb;
  if (B * groups > 0x7fffffffLL) return set_error(BF_EINVAL, "particle smoother: B x S too large for one launch");
  const PfsModel<N>* dm = nullptr;
  if (N > 8) {   // beyond n = 8 the kernel reads the model from memory (content-keyed constant cache, stream-ordered upload)
    const void* dv = nullptr;
    const int rc = device_constants(&m, sizeof(m), stream, &dv);
    if (rc != BF_OK) return rc;
    dm = static_cast<const PfsModel<N>*>(dv);
  }
  hipLaunchKernelGGL((pfs_backward_kernel<N, RMAX, WAVES>), dim3((unsigned)(B * groups)), dim3(64 * wpb), 0, stream, m, dm, v, T, NP, S,
                     (int)groups);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

template <int N>
static int launch_pfs_n(const std::vector<float>& A, const std::vector<float>& c, const std::vector<float>& Li, int dyn_id,
                        const float* dth, const PfsViews& v, long long B, long long T, int NP, int S, hipStream_t stream) {
  PfsModel<N> m;
  std::memset(&m, 0, sizeof(m));
  m.dyn_id = dyn_id;
  for (int i = 0; i < 8; ++i) m.dth[i] = dth[i];
  for (int i = 0; i < N * N; ++i) m.A[i] = A[i];
  for (int i = 0; i < N; ++i) m.c[i] = c[i];
  for (int i = 0; i < N * N; ++i) m.Li[i] = Li[i];
  if (NP <= 1024) return launch_pfs_inst<N, 16, 16>(m, v, B, T, NP, S, stream);
  return launch_pfs_inst<N, 64, 8>(m, v, B, T, NP, S, stream);
}

// registry dynamics -> (A, F_q, dth) with the dimension rules of fill_bpf_model_view (ssm_device.hpp)
static int pfs_dynamics(const bf_model* p, std::vector<float>& A, std::vector<double>& G, float* dth) {
  const int n = p->n, dq = p->dq;
  const float* th = p->dyn_theta;
  A.assign((size_t)n * n, 0.f);
  G.assign((size_t)n * dq, 0.0);
  for (int i = 0; i < 8; ++i) dth[i] = 0.f;
  auto identity = [&]() {
    for (int i = 0; i < n; ++i) G[(size_t)i * dq + i] = 1.0;
  };
  switch (p->dyn_id) {
    case DYN_LINEAR:
      if (p->n_dyn_theta != n * n + n * dq || !th) return set_error(BF_EINVAL, "linear dynamics: theta must hold A and G");
      for (int i = 0; i < n * n; ++i) A[i] = th[i];
      for (int i = 0; i < n * dq; ++i) G[i] = th[n * n + i];
      break;
    case DYN_LORENZ96:
      if (p->n_dyn_theta != 5 || dq != n || !th) return set_error(BF_EINVAL, "lorenz96: theta = (alpha, beta, gamma, dt, mode), dq = n");
      for (int i = 0; i < 5; ++i) dth[i] = th[i];
      identity();
      break;
    case DYN_LORENZ63:
      if (n != 3 || p->n_dyn_theta != 4 || dq != 3 || !th) return set_error(BF_EINVAL, "lorenz63: n = dq = 3");
      for (int i = 0; i < 4; ++i) dth[i] = th[i];
      identity();
      break;
    case DYN_MANEUVER_BOT: {
      if (n != 4 || p->n_dyn_theta != 2 || dq != 2 || !th) return set_error(BF_EINVAL, "maneuver_bot: n = 4, dq = 2");
      dth[0] = th[0];
      dth[1] = th[1];
      const double Gb[8] = {0.5, 0, 1, 0, 0, 0.5, 0, 1};
      for (int i = 0; i < 8; ++i) G[i] = Gb[i];
    } break;
    case DYN_SINE:
      if (p->n_dyn_theta != 1 || dq != n || !th) return set_error(BF_EINVAL, "sine: theta = (w0), dq = n");
      dth[0] = th[0];
      identity();
      break;
    case DYN_GROWTH:
      if (n != 1 || dq != 1) return set_error(BF_EINVAL, "growth: n = dq = 1");
      identity();
      break;
    default: return set_error(BF_EUNSUPPORTED, "unknown dynamics function id %d", p->dyn_id);
  }
  return BF_OK;
}

// the checks and the view both entry points share
static int pfs_views(const bf_pf_history* h, const bf_pf_sample_carry* carry, const bf_pf_sample_desc* out, const bf_cstream* u,
                     long long B, long long T, long long N, long long S, int n, bool genealogy, PfsViews& v) {
  if (B < 1 || T < 1 || N < 1 || S < 1)
    return set_error(BF_EINVAL, "B, T, N and S must be at least 1 (B=%lld, T=%lld, N=%lld, S=%lld)", B, T, N, S);
  if (n < 1) return set_error(BF_EINVAL, "non-positive state dimension");
  if (!h->weights || !h->particles) return set_error(BF_EINVAL, "the history's weights and particles are required");
  if (genealogy && !h->ancestors) return set_error(BF_EINVAL, "the genealogy method needs the history's ancestors");
  if (!out->samples.ptr) return set_error(BF_EINVAL, "the samples stream is a required output");
  if (!out->noise && !out->keys) return set_error(BF_EINVAL, "give the noise (uniforms) or the keys");
  if (out->noise && out->keys) return set_error(BF_EINVAL, "give either the noise (uniforms) or the keys, not both");
  if (S * T > 0x7fffffffLL) return set_error(BF_EINVAL, "S*T must not exceed 2^31 - 1; sample in chunks of T");
  if (N > 0x7fffffffLL || S * n > 0x7fffffffLL) return set_error(BF_EINVAL, "N or S too large");
  std::memset(&v, 0, sizeof(v));
  v.w = h->weights; v.w_sB = h->w_sB; v.w_sN = h->w_sN; v.w_sT = h->w_sT;
  v.x = h->particles; v.x_sB = h->x_sB; v.x_sN = h->x_sN; v.x_sT = h->x_sT;
  v.a = h->ancestors;
  if (u && u->ptr) { v.u = u->ptr; v.u_sB = u->sB; v.u_sT = u->sT; }
  v.out = out->samples.ptr; v.o_sB = out->samples.sB; v.o_sS = out->samples.sK; v.o_sT = out->samples.sT; v.o_sE = out->samples.sE;
  v.idx = out->indices;
  v.noise = out->noise; v.z_sB = out->z_sB; v.z_sS = out->z_sS; v.z_sT = out->z_sT;
  v.keys = out->keys;
  if (carry) {
    v.x_in = carry->x_in; v.u_in = carry->u_in; v.a_in = carry->a_in;
    v.x_out = carry->x_out; v.a_out = carry->a_out;
  }
  return BF_OK;
}

static int launch_pfs_backward(const bf_model* p, const PfsViews& v, long long B, long long T, int NP, int S, hipStream_t stream) {
  const int n = p->n, dq = p->dq;
  std::vector<float> A;
  std::vector<double> G;
  float dth[8];
  int rc = pfs_dynamics(p, A, G, dth);
  if (rc != BF_OK) return rc;
  // M = F_q Q F_q^T in float64, its Cholesky factor with the samplers' pivot rule (tau = 2^-17 of the diagonal), L^-1
  std::vector<double> GQ((size_t)n * dq, 0.0), Mx((size_t)n * n, 0.0), L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < dq; ++k) {
      double s = 0;
      for (int l = 0; l < dq; ++l) s += G[(size_t)i * dq + l] * (double)p->Q[l * dq + k];
      GQ[(size_t)i * dq + k] = s;
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0;
      for (int k = 0; k < dq; ++k) s += GQ[(size_t)i * dq + k] * G[(size_t)j * dq + k];
      Mx[(size_t)i * n + j] = s;
    }
  const double tau = 1.0 / 131072.0;
  for (int j = 0; j < n; ++j) {
    double d = Mx[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(d > tau * Mx[(size_t)j * n + j]) || !(d > 0.0))
      return set_error(BF_EUNSUPPORTED,
                       "backward simulation needs a transition density: F_q Q F_q^T is not positive definite (pivot %d); use the "
                       "genealogy method (bf_pf_trace_sample_f32, method=\"genealogy\")", j);
    d = std::sqrt(d);
    L[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = Mx[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = s / d;
    }
  }
  for (int j = 0; j < n; ++j) {   // column j of L^-1 by forward substitution
    Li[(size_t)j * n + j] = 1.0 / L[(size_t)j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0;
      for (int k = j; k < i; ++k) s -= L[(size_t)i * n + k] * Li[(size_t)k * n + j];
      Li[(size_t)i * n + j] = s / L[(size_t)i * n + i];
    }
  }
  std::vector<float> Lif((size_t)n * n), c(n);
  for (size_t i = 0; i < Lif.size(); ++i) Lif[i] = (float)Li[i];
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int k = 0; k < dq; ++k) s += G[(size_t)i * dq + k] * (p->q0 ? (double)p->q0[k] : 0.0);
    c[i] = (float)s;
  }
  switch (n) {
#define BF_PFS_CASE(N_) case N_: return launch_pfs_n<N_>(A, c, Lif, p->dyn_id, dth, v, B, T, NP, S, stream);
    BF_PFS_CASE(1) BF_PFS_CASE(2) BF_PFS_CASE(3) BF_PFS_CASE(4) BF_PFS_CASE(5) BF_PFS_CASE(6) BF_PFS_CASE(7) BF_PFS_CASE(8)
    BF_PFS_CASE(9) BF_PFS_CASE(10) BF_PFS_CASE(11) BF_PFS_CASE(12) BF_PFS_CASE(13) BF_PFS_CASE(14) BF_PFS_CASE(15) BF_PFS_CASE(16)
#undef BF_PFS_CASE
    default: break;
  }
  return set_error(BF_EUNSUPPORTED, "backward simulation serves state dimensions 1 ... %d (n = %d)", PFS_MAX_DIM, n);
}

}  // namespace bf

extern "C" {

int bf_pf_sampler_abi_check(size_t sizeof_history, size_t sizeof_sample_desc, size_t sizeof_sample_carry) {
#define BF_ABI_SIZE(NAME_, T_)                                                                                  \
  if (NAME_ != 0 && NAME_ != sizeof(T_)) \
    return bf::set_error(BF_EINVAL, "binding's sizeof(" #T_ ") = %zu, the library's is %zu: the struct layouts differ", NAME_, sizeof(T_));
  BF_ABI_SIZE(sizeof_history, bf_pf_history)
  BF_ABI_SIZE(sizeof_sample_desc, bf_pf_sample_desc)
  BF_ABI_SIZE(sizeof_sample_carry, bf_pf_sample_carry)
#undef BF_ABI_SIZE
  return BF_OK;
}

int bf_pf_backward_sample_f32(const bf_bpf_model* model, const bf_cstream* u, const bf_pf_history* history, int64_t B, int64_t T,
                              int32_t N, int32_t S, const bf_pf_sample_carry* carry, const bf_pf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!model || !history || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  const bf_model* p = &model->ssm;
  if (p->user || p->dyn_id == BF_FN_USER)
    return bf::set_error(BF_EUNSUPPORTED, "backward simulation serves registry dynamics; for dynamics given as source use the "
                                          "genealogy method (bf_pf_trace_sample_f32, method=\"genealogy\")");
  if (p->flags != 0) return bf::set_error(BF_EUNSUPPORTED, "the particle smoother serves the JAX path's models (flags = 0)");
  if (p->n <= 0 || p->dq <= 0) return bf::set_error(BF_EINVAL, "non-positive model dimension");
  if (p->Q_steps > 1) return bf::set_error(BF_EUNSUPPORTED, "backward simulation needs a constant Q (Q_steps 0 or 1)");
  if (!p->Q) return bf::set_error(BF_EINVAL, "Q is required");
  if (p->n > bf::PFS_MAX_DIM)
    return bf::set_error(BF_EUNSUPPORTED, "backward simulation serves state dimensions 1 ... %d (n = %d)", bf::PFS_MAX_DIM, (int)p->n);
  bf::PfsViews v;
  const int rc = bf::pfs_views(history, carry, out, u, B, T, N, S, p->n, false, v);
  if (rc != BF_OK) return rc;
  if (N > bf::PFS_MAX_PARTICLES)
    return bf::set_error(BF_EUNSUPPORTED, "backward simulation serves N <= %d particles (N = %d); the genealogy method "
                                          "(bf_pf_trace_sample_f32, method=\"genealogy\") has no cap", bf::PFS_MAX_PARTICLES, (int)N);
  return bf::launch_pfs_backward(p, v, B, T, N, S, static_cast<hipStream_t>(stream));
}

int bf_pf_trace_sample_f32(const bf_pf_history* history, int64_t B, int64_t T, int32_t N, int32_t n, int32_t S,
                           const bf_pf_sample_carry* carry, const bf_pf_sample_desc* out, void* stream) {
  bf::CallOptionScope call_option_scope;
  if (!history || !out) return bf::set_error(BF_EINVAL, "NULL argument");
  bf::PfsViews v;
  const int rc = bf::pfs_views(history, carry, out, nullptr, B, T, N, S, n, true, v);
  if (rc != BF_OK) return rc;
  const long long waves = (long long)B * S;
  if ((waves + 3) / 4 > 0x7fffffffLL) return bf::set_error(BF_EINVAL, "particle smoother: B x S too large for one launch");
  hipLaunchKernelGGL(bf::pfs_trace_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), v,
                     (long long)B, (long long)T, (int)N, (int)n, (int)S);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

int bf_random_uniform_f32(const uint32_t key[2], int64_t count, float* host_out) {
  if (!key || !host_out || count < 0 || count > 0x7fffffff) return bf::set_error(BF_EINVAL, "bad argument");
  for (int64_t i = 0; i < count; ++i) host_out[i] = bf::bits_to_unit(bf::threefry_bits(key[0], key[1], (uint32_t)i, (uint32_t)count));
  return BF_OK;
}

}  // extern "C"
