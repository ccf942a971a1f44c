// Dispatch of the bootstrap particle filter over the compiled (n, dq, m) table (instantiations in
// bpf_group_{a,b,c}.hip, each built plain and with MISSING = true), the launch of the same kernels built at run time, and the
// stand-alone resampler.
#include "bpf_big.hpp"   // (brings bpf_scan.hpp)
#include "user_model.hpp"

namespace bf {

Option g_bpf_variant{0, OPT_BPF_VARIANT};   // tuning hook (bf_set_option "bpf_variant")
Option g_bpf_hbm_mode{0, OPT_BPF_HBM_MODE};  // bf_set_option "bpf_hbm_mode"
Option g_bpf_spec{1, OPT_BPF_SPEC};      // bf_set_option "bpf_spec"
Option g_bpf_arith{0, OPT_BPF_ARITH};    // bf_set_option "bpf_arith": 0 = canonical fp32 arithmetic (bit-exact ancestry), 1 = hardware v_exp_f32 / v_log_f32

// Stand-alone resampler: idx[b][:] = choice(key_b, N, (N,), p = w[b]) (the index draw of utils.py:210)
template <int PPT, int NW>
__global__ void __launch_bounds__(64 * NW)
resample_kernel(const float* __restrict__ w, const uint32_t* __restrict__ keys, int NP, int resampler, int* __restrict__ idx) {
  constexpr int CAP = 64 * NW * PPT;
  __shared__ float cdf[cdf_words(CAP)];
  __shared__ float red[64];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  float wn[PPT];
  bool valid[PPT];
  int anc[PPT];
  BF_UNROLL for (int p = 0; p < PPT; ++p) {
    valid[p] = tid * PPT + p < NP;
    wn[p] = valid[p] ? w[b * NP + tid * PPT + p] : 0.f;
  }
  resample_indices<PPT, NW>(wn, valid, NP, U32x2{keys[b * 2], keys[b * 2 + 1]}, resampler, cdf, red, anc);
  BF_UNROLL for (int p = 0; p < PPT; ++p) if (valid[p]) idx[b * NP + tid * PPT + p] = anc[p];
}

int launch_resample(const float* d_w, const uint32_t* d_keys, long long B, int NP, int resampler, int* d_idx,
                    hipStream_t stream) {
  if (NP <= 64) hipLaunchKernelGGL((resample_kernel<1, 1>), dim3((unsigned)B), dim3(64), 0, stream, d_w, d_keys, NP, resampler, d_idx);
  else if (NP <= 256) hipLaunchKernelGGL((resample_kernel<1, 4>), dim3((unsigned)B), dim3(256), 0, stream, d_w, d_keys, NP, resampler, d_idx);
  else if (NP <= 1024) hipLaunchKernelGGL((resample_kernel<1, 16>), dim3((unsigned)B), dim3(1024), 0, stream, d_w, d_keys, NP, resampler, d_idx);
  else if (NP <= 4096) hipLaunchKernelGGL((resample_kernel<4, 16>), dim3((unsigned)B), dim3(1024), 0, stream, d_w, d_keys, NP, resampler, d_idx);
  else return set_error(BF_EUNSUPPORTED, "resample: %d particles exceed the compiled capacity of 4096", NP);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

// the compiled (n, dq, m) table: bpf_group_{a,b,c}.hip, each built plain and with MISSING = true
using BpfGroup = int(const bf_bpf_model* bp, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int NP, float ess,
                     int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out, hipStream_t stream, bool* matched);
BpfGroup launch_bpf_group_a, launch_bpf_group_b, launch_bpf_group_c, launch_bpf_missing_group_a, launch_bpf_missing_group_b,
    launch_bpf_missing_group_c;
static BpfGroup* const kPlainGroups[] = {launch_bpf_group_a, launch_bpf_group_b, launch_bpf_group_c};
static BpfGroup* const kMissingGroups[] = {launch_bpf_missing_group_a, launch_bpf_missing_group_b, launch_bpf_missing_group_c};

// The particle filter built at run time (user_model.hpp): around the functions of a handle from source (the caller's functions
// see the CANONICAL arithmetic of the weight path, so a function written like its registry twin gives the registry twin's bits),
// or -- an internal handle without sources -- around the registry's, for dimensions without a compiled instance and for
// bf_set_option "bpf_arith" = 1.  State in registers at the compile-time dimensions of the handle, one kernel per particle
// capacity; beyond the register capacities the particles live in HBM (bpf_big.hpp), up to 2^20 per trajectory.  missing: the
// MISSING = true twins (JIT_BPF_MISSING, JIT_BPF_BIG_MISSING: kernels of their own in the handle's map and in the on-disk cache).
static int launch_bpf_jit(const bf_user_model* um, const bf_bpf_model* bp, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                          int NP, float ess, int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out, hipStream_t stream,
                          bool missing) {
  int rc = check_user_model(um, &bp->ssm);
  if (rc != BF_OK || (rc = check_user_device(um)) != BF_OK) return rc;
  const int N = bp->ssm.n;
  BpfModelLaunch L;
  if ((rc = prepare_bpf_model(bp, um->user_flags(), stream, L, missing)) != BF_OK) return rc;
  // registry models (the hardware-arithmetic build): the model structure as a compile-time spec where bpf_scan.hpp has one
  const int spec = !um->hw_arith ? JIT_SPEC_USER : (L.l96_pick ? JIT_SPEC_L96_PICK : JIT_SPEC_RUNTIME);
  int ppt, nw;
  bpf_capacity(NP, N, &ppt, &nw);
  hipFunction_t fn = nullptr;
  const int kind = ppt == 0 ? (missing ? JIT_BPF_BIG_MISSING : JIT_BPF_BIG) : (missing ? JIT_BPF_MISSING : JIT_BPF);
  if ((rc = user_kernel(um, kind, ppt, ppt == 0 ? 0 : nw, spec, &fn)) != BF_OK) return rc;
  if (ppt == 0) {
    BigScratch sc;
    float* buf = nullptr;
    if ((rc = prepare_bpf_big(N, B, NP, stream, sc, &buf)) != BF_OK) return rc;
    BpfInputs in = bpf_inputs(y, u);
    BpfCarry crv = cr;
    BpfOut ov = out;
    uint32_t k0 = key[0], k1 = key[1];
    void* args[] = {&L.d_mdl, &in.y, &in.u, &in.u_sB, &in.u_sT, &crv, &ov, &sc, &B, &T, &NP, &ess, &resampler, &k0, &k1};
    const hipError_t le = hipModuleLaunchKernel(fn, (unsigned)B, 1, 1, BIG_NT, 1, 1, 0, stream, args, nullptr);
    const hipError_t fe = hipFreeAsync(buf, stream);
    BF_HIP_CHECK(le);
    BF_HIP_CHECK(fe);
    return BF_OK;
  }
  const size_t lds_bytes = bpf_lds_bytes(N, ppt, nw, missing ? bpf_density_words(bp->ssm.m) : 0);
  if (lds_bytes > 160 * 1024) return set_error(BF_EUNSUPPORTED, "particle tile exceeds the 160 KiB LDS");
  struct { const void* mdl; BpfArgs<1, 1, 1> a; } packed;   // the kernarg segment: the model pointer, then the struct
  packed.mdl = L.d_mdl;
  fill_bpf_args(packed.a, y, u, B, T, NP, ess, resampler, key, cr, out);
  size_t psz = sizeof(packed);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &packed, HIP_LAUNCH_PARAM_BUFFER_SIZE, &psz, HIP_LAUNCH_PARAM_END};
  BF_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)B, 1, 1, (unsigned)(64 * nw), 1, 1, (unsigned)lds_bytes, stream, nullptr, config));
  return BF_OK;
}

int launch_bpf(const bf_bpf_model* bp, const bf_cstream* y, const bf_cstream* u, long long B, long long T, int NP,
               float ess, int resampler, const uint32_t key[2], const bf_bpf_carry* carry, const bf_bpf_out* o,
               hipStream_t stream, bool missing) {
  const BpfCarry cr = make_bpf_carry(carry);
  const BpfOut out = make_bpf_out(o);
  if (bp->ssm.user)   // functions from the caller's source: the kernel compiled at run time for this model
    return launch_bpf_jit(bp->ssm.user, bp, y, u, B, T, NP, ess, resampler, key, cr, out, stream, missing);
  if (bp->ssm.dyn_id == BF_FN_USER || bp->ssm.emi_id == BF_FN_USER)
    return set_error(BF_EINVAL, "dyn_id / emi_id = BF_FN_USER needs bf_model.user (bf_user_model_create)");
  if (g_bpf_arith != 1) {   // (1: the same kernel with the hardware's transcendentals, compiled at run time)
    bool matched;
    const int rc = run_groups(missing ? kMissingGroups : kPlainGroups, std::size(kPlainGroups), &matched, bp, y, u, B, T, NP, ess,
                              resampler, key, cr, out, stream);
    if (matched) return rc;
  }
  // hardware arithmetic, or no compiled instance for these dimensions: the same kernel, compiled now (needs hiprtc)
  const bf_user_model* um = registry_jit_handle(&bp->ssm, g_bpf_arith == 1);
  if (!um) return set_error(BF_ENOGPU, "no current device");
  return launch_bpf_jit(um, bp, y, u, B, T, NP, ess, resampler, key, cr, out, stream, missing);
}

}  // namespace bf
