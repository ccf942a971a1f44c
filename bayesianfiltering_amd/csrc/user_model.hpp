// The run-time-build layer as the other translation units see it: the handle behind bf_model.user (user_model.hip), the
// source assembler (jit_source.hip) and hiprtc with its code-object cache (jit_cache.hip).  Every filter family's host code
// prepares a launch once (prepare_* in its header) and fires either its compiled instance or the kernel it gets from here.
#pragma once
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include "bf_common.hpp"

// kernels compiled at run time around the caller's functions -- or around the registry's, for dimensions without a compiled instance
enum bf_jit_kind { JIT_GSF_GENERIC, JIT_BPF, JIT_UGSF, JIT_AGSF_UKF, JIT_AGSF_EKF, JIT_GSF_REGS, JIT_SAMPLE, JIT_BPF_BIG, JIT_UGSF_GENERIC,
                   JIT_RTS_REGS, JIT_FFBS_REGS, JIT_RTS_GENERIC, JIT_FFBS_GENERIC,     // the smoother's / the posterior sampler's kernels around dynamics from source
                   JIT_GS_RTS_REGS, JIT_GS_RTS_GENERIC, JIT_GS_FFBS_REGS, JIT_GS_FFBS_GENERIC,     // the Gaussian-sum smoother's / sampler's (K chains per trajectory)
                   JIT_BPF_MISSING, JIT_BPF_BIG_MISSING,     // the particle filter's MISSING = true twins (NaN observations are gaps)
                   JIT_GSF_GENERIC_MISSING };   // ... and the run-time-dimension Gaussian-sum scan's, one entry point per workgroup size (nw = 1 or 4 waves)
// the model structure a sampling kernel is compiled for: the handle's own functions, or (registry models) bpf_scan.hpp's specs
enum bf_jit_spec { JIT_SPEC_USER = 0, JIT_SPEC_RUNTIME = 1, JIT_SPEC_L96_PICK = 2 };

struct bf_user_model {
  int n = 0, dq = 0, m = 0, dr = 0;
  int device = -1;
  bool has_dyn = false, has_emi = false, has_lp = false;
  bool hw_arith = false;                  // internal handle of bf_set_option "bpf_arith" = 1: registry functions, hardware transcendentals
  std::string dyn_src, emi_src, lp_src;  // kept: all kernels but the run-time-dimension scan are built on first use
  hipFunction_t k64 = nullptr, k256 = nullptr;   // the run-time-dimension Gaussian-sum scan, built at creation when f or h is given
  std::map<int, hipFunction_t> kernels;   // built on first use, by (kind, spec, particles per thread -- the smoother's data path / the sampler's samples per lane --, waves): user_kernel
  int user_flags() const { return (has_dyn ? 1 : 0) | (has_emi ? 2 : 0) | (has_lp ? 4 : 0); }   // fill_*_model_view's user_flags
};

namespace bf {

// ---- jit_cache.hip: source -> module through the on-disk code-object cache (hit: load; miss or unloadable file: compile with
// hiprtc, write atomically, load), then the named entry points.  jit_source_key: the cache key of a source (16 hex digits).
std::string jit_source_key(const std::string& src);
int jit_load(const std::string& src, std::initializer_list<std::pair<const char*, hipFunction_t*>> entries, bool contract_off = true,
             hipModule_t* mod = nullptr);

// ---- jit_source.hip: the text hiprtc compiles for one kernel of a handle, and that kernel's entry point
std::string jit_source(const bf_user_model& um, int kind, int ppt, int nw, int spec);
const char* jit_entry_name(int kind, int variant = 0);   // variant: the data path (JIT_RTS_REGS) / samples per lane (JIT_FFBS_REGS)

// ---- user_model.hip
int check_user_model(const bf_user_model* um, const bf_model* p);   // the handle was created for this model's dimensions and functions
int check_user_device(const bf_user_model* um);                     // ... and on the current device
const bf_user_model* registry_jit_handle(const bf_model* p, bool hw_arith);
// the handle's kernel of this kind, built under the lock on first use (checks the device)
int user_kernel(const bf_user_model* um, int kind, int ppt, int nw, int spec, hipFunction_t* fn);
// launches the handle's run-time-dimension Gaussian-sum scan, or `fn` (another kernel of the handle with dynamic LDS) when given
int launch_user_kernel(const bf_user_model* um, int nt, unsigned grid, size_t lds_bytes, hipStream_t stream, void** args,
                       hipFunction_t fn = nullptr);

// ---- launches of the kernels built at run time, next to their compiled twins
int launch_ugsf_generic(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K,
                        const bf_carry* carry, const bf_out_desc* out, hipStream_t stream);   // ugsf_generic.hip: registry or from source, any dimensions
bool gsf_user_regs_eligible(const bf_model* p, int K, const bf_out_desc* out);   // ugsf_scan.hip
int launch_gsf_user_regs_impl(const bf_model* p, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int K, const bf_carry* carry,
                              const bf_out_desc* out, hipStream_t stream);
int launch_agsf_user_impl(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                          const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                          int* d_leaf_idx, int variant, hipStream_t stream);   // agsf_ukf.hip

}  // namespace bf
