// user_model: dynamics / emission functions given as SOURCE TEXT at run time.
//
// The reference takes arbitrary Python callables f(x, q, u), h(x, r, u) (gaussfiltax/models.py:46-49) and differentiates
// them with jacfwd (gaussfiltax/inference.py:328-329).  A Python callable cannot run inside a HIP kernel; what can cross
// the C-ABI is the function's source.  bf_user_model_create compiles, with hiprtc (jit_cache.hip), the run-time-dimension scan
// kernel together with the caller's functions (jit_source.hip); every other kernel of the handle is built on first use
// (user_kernel) and launched by its family's host code, next to the compiled instances.  Handles are cached by source hash.
#include <mutex>
#include "user_model.hpp"

namespace bf {

namespace {
std::mutex g_mu;                                 // handles and every build
std::map<std::string, bf_user_model*> g_models;  // by source hash: a model compiled once is shared (never freed while cached)
}  // namespace

int check_user_model(const bf_user_model* um, const bf_model* p) {
  // the JIT kernel indexes LDS and registers with the COMPILE-TIME dimensions of bf_user_model_create while the launch
  // carves LDS from the run-time bf_model: they must be the same model
  if (um->n != p->n || um->dq != p->dq || um->m != p->m || um->dr != p->dr)
    return set_error(BF_EINVAL, "bf_model.user was compiled for (n, dq, m, dr) = (%d, %d, %d, %d) but the model says (%d, %d, %d, %d)",
                     um->n, um->dq, um->m, um->dr, p->n, p->dq, p->m, p->dr);
  if (p->dyn_id == BF_FN_USER && !um->has_dyn)
    return set_error(BF_EINVAL, "dyn_id = BF_FN_USER but bf_model.user was created without dynamics source");
  if (p->emi_id == BF_FN_USER && !um->has_emi)
    return set_error(BF_EINVAL, "emi_id = BF_FN_USER but bf_model.user was created without emission source");
  if (p->dyn_id != BF_FN_USER && um->has_dyn)
    return set_error(BF_EINVAL, "bf_model.user holds dynamics source: dyn_id must be BF_FN_USER");
  if (p->emi_id != BF_FN_USER && um->has_emi)
    return set_error(BF_EINVAL, "bf_model.user holds emission source: emi_id must be BF_FN_USER");
  return BF_OK;
}

int check_user_device(const bf_user_model* um) {   // a module is loaded on ONE device
  int dev = -1;
  (void)hipGetDevice(&dev);
  if (dev != um->device)
    return set_error(BF_EINVAL, "bf_model.user was loaded on device %d, the current device is %d (create one handle per device)", um->device, dev);
  return BF_OK;
}

int launch_user_kernel(const bf_user_model* um, int nt, unsigned grid, size_t lds_bytes, hipStream_t stream, void** args, hipFunction_t fn) {
  const int rc = check_user_device(um);
  if (rc != BF_OK) return rc;
  hipFunction_t f = fn ? fn : (nt == 64 ? um->k64 : um->k256);
  // (a module function needs no opt-in for more than 64 KiB of dynamic LDS on gfx950: the launch itself checks the 160 KiB limit)
  BF_HIP_CHECK(hipModuleLaunchKernel(f, grid, 1, 1, (unsigned)nt, 1, 1, (unsigned)lds_bytes, stream, args, nullptr));
  return BF_OK;
}

int user_kernel(const bf_user_model* handle, int kind, int ppt, int nw, int spec, hipFunction_t* fn) {
  bf_user_model* um = const_cast<bf_user_model*>(handle);
  int rc = check_user_device(um);
  if (rc != BF_OK) return rc;
  auto key_of = [&](int variant) { return ((kind * 10 + spec) * 100 + variant) * 100 + nw; };
  const int key = key_of(ppt);
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = um->kernels.find(key);
  if (it != um->kernels.end()) {
    *fn = it->second;
    return BF_OK;
  }
  if (kind == JIT_RTS_REGS || kind == JIT_FFBS_REGS) {
    // the smoother's data paths / the sampler's samples-per-lane counts (ppt) share one module: a build fills the map for all
    const bool rts = kind == JIT_RTS_REGS;
    const int variants[4] = {rts ? 0 : 1, 2, 4, 8};
    const int nv = rts ? 2 : 4;
    hipFunction_t f[4] = {nullptr, nullptr, nullptr, nullptr};
    const std::string src = jit_source(*um, kind, 0, nw, spec);
    rc = rts ? jit_load(src, {{jit_entry_name(kind, 0), &f[0]}, {jit_entry_name(kind, 2), &f[1]}})
             : jit_load(src, {{jit_entry_name(kind, 1), &f[0]}, {jit_entry_name(kind, 2), &f[1]}, {jit_entry_name(kind, 4), &f[2]},
                              {jit_entry_name(kind, 8), &f[3]}});
    if (rc != BF_OK) return rc;
    for (int i = 0; i < nv; ++i) um->kernels[key_of(variants[i])] = f[i];
    it = um->kernels.find(key);
    if (it == um->kernels.end()) return set_error(BF_EINVAL, "no such variant of the kernel (kind %d, variant %d)", kind, ppt);
    *fn = it->second;
    return BF_OK;
  }
  if (kind == JIT_GS_RTS_REGS) {  // the three output sets (ppt = GS_COMP, GS_COLL, both) share one module
    hipFunction_t f[3] = {nullptr, nullptr, nullptr};
    rc = jit_load(jit_source(*um, kind, 0, nw, spec), {{jit_entry_name(kind, 1), &f[0]}, {jit_entry_name(kind, 2), &f[1]}, {jit_entry_name(kind, 3), &f[2]}});
    if (rc != BF_OK) return rc;
    for (int i = 0; i < 3; ++i) um->kernels[key_of(i + 1)] = f[i];
    it = um->kernels.find(key);
    if (it == um->kernels.end()) return set_error(BF_EINVAL, "no such variant of the kernel (kind %d, variant %d)", kind, ppt);
    *fn = it->second;
    return BF_OK;
  }
  rc = jit_load(jit_source(*um, kind, ppt, nw, spec), {{jit_entry_name(kind), fn}});
  if (rc == BF_OK) um->kernels[key] = *fn;
  return rc;
}

// An internal handle without sources, per (dimensions, device, arithmetic): the sampling kernels compiled at run time for a
// REGISTRY model -- bf_set_option "bpf_arith" = 1 (v_log_f32 / v_exp_f32 in place of the defined arithmetic: BF_BPF_HW_ARITH in
// bf_canon_math.hpp / bf_rng.hpp), and every (n, dq, m, dr) the compiled instance tables of the particle / unscented / augmented
// kernels do not hold (bpf_scan.hip, ugsf_scan.hip, agsf_ukf.hip, agsf_scan.hip put it into a copy of the model and take the
// from-source path: "not compiled in" becomes "compiled now").
const bf_user_model* registry_jit_handle(const bf_model* p, bool hw_arith) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  const std::string mem_key = std::string(hw_arith ? "hw_arith:" : "registry:") + std::to_string(p->n) + "," + std::to_string(p->dq) + "," +
                              std::to_string(p->m) + "," + std::to_string(p->dr) + "@" + std::to_string(dev);
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_models.find(mem_key);
  if (it != g_models.end()) return it->second;
  bf_user_model* um = new bf_user_model;
  um->n = p->n; um->dq = p->dq; um->m = p->m; um->dr = p->dr; um->device = dev; um->hw_arith = hw_arith;
  g_models[mem_key] = um;
  return um;
}

}  // namespace bf

extern "C" {

int bf_user_model_create(const char* dynamics_src, const char* emission_src, int32_t n, int32_t dq, int32_t m, int32_t dr,
                         bf_user_model** model) {
  return bf_user_model_create_lp(dynamics_src, emission_src, nullptr, n, dq, m, dr, model);
}

int bf_user_model_create_lp(const char* dynamics_src, const char* emission_src, const char* log_prob_src, int32_t n, int32_t dq,
                            int32_t m, int32_t dr, bf_user_model** model) {
  using namespace bf;
  if (!model || (!dynamics_src && !emission_src && !log_prob_src)) return set_error(BF_EINVAL, "bf_user_model_create: no source given");
  if (n <= 0 || dq <= 0 || m <= 0 || dr <= 0 || n > 64 || dq > 64 || m > 64 || dr > 64)
    return set_error(BF_EINVAL, "bf_user_model_create: dimensions must be in 1..64");
  bf_user_model made;
  made.n = n; made.dq = dq; made.m = m; made.dr = dr;
  made.has_dyn = dynamics_src != nullptr;
  made.has_emi = emission_src != nullptr;
  made.has_lp = log_prob_src != nullptr;
  if (dynamics_src) made.dyn_src = dynamics_src;
  if (emission_src) made.emi_src = emission_src;
  if (log_prob_src) made.lp_src = log_prob_src;
  // (the log-density belongs to the particle kernel, built on first use; here it only makes the handle's key unique: every
  // line of it as a comment)
  std::string lp_comment;
  if (log_prob_src) {
    lp_comment = "// lp: ";
    for (const char* c = log_prob_src; *c; ++c) {
      lp_comment += *c;
      if (*c == '\n') lp_comment += "// ";
    }
    lp_comment += "\n";
  }
  const std::string src = jit_source(made, JIT_GSF_GENERIC, 0, 0, JIT_SPEC_USER) + lp_comment;
  if (hipGetDevice(&made.device) != hipSuccess) {
    made.device = -1;
    (void)hipGetLastError();
  }
  const std::string mem_key = jit_source_key(src) + "@" + std::to_string(made.device);   // a module is loaded on ONE device
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_models.find(mem_key);
  if (it != g_models.end()) {
    *model = it->second;
    return BF_OK;
  }
  // the Gaussian-sum scan is built now (a log-density alone: nothing to build before the first particle-filter call)
  if (dynamics_src || emission_src) {
    const int rc = jit_load(src, {{"bf_user_scan_64", &made.k64}, {"bf_user_scan_256", &made.k256}});
    if (rc != BF_OK) return rc;
  }
  *model = g_models[mem_key] = new bf_user_model(made);
  return BF_OK;
}

void bf_user_model_destroy(bf_user_model* model) {
  (void)model;  // compiled models are shared through the cache and live as long as the process
}

}  // extern "C"
