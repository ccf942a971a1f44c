// bpf_big: bootstrap particle filter for particle counts beyond the in-register kernel (bpf_scan.hpp).
//
// Same recursion as bpf_scan_kernel -- the lax.scan body of bootstrap_particle_filter
// (gaussfiltax/inference.py:1330-1377) with _resample (utils.py:207-214) -- for N up to 2^20 particles
// per trajectory, the counts the reference's own scripts use (5e4 in BOT_Experiment_script.py:138,
// 5e5 in Experiment_TSP_2023.ipynb).  The particles of a trajectory live in HBM (two buffers, the
// resampling gather goes from one to the other); one 1024-thread workgroup per trajectory walks them
// in chunks of 1024, so every reduction and the cumulative sum keep the binary-tree order of the small
// kernel and of the oracle:
//   * max / sum: adjacent-pair tree inside a chunk (block_tree_reduce of scan_common.hpp), then the same tree over
//     the chunk results (chunks_reduce; N' = next_pow2 chunks, zero / -inf padded);
//   * CDF = lax.associative_scan order (Brent-Kung) over N' elements: per chunk the up-sweep yields the chunk
//     total (block_total_assoc); the totals are scanned by the same algorithm; then every chunk redoes its up-sweep
//     and runs the down-sweep with the inclusive value at the end of the previous chunk as the element "before" it
//     (block_cumsum_assoc with a prefix);
//   * inverse-CDF draw by binary search over the CDF in global memory, gather through global memory.
// The workgroup of a trajectory is alone on its data: no grid-wide synchronisation, any batch size.
//
// The pieces that define a step's bits -- the collectives above, the particle at step 0, the ancestor draw, the key
// chain, the reduction functors -- stand in front of the kernel; the workgroup-per-chunk kernels of bpf_wide.hpp are
// written from the same ones.
#pragma once
#include "bpf_scan.hpp"

namespace bf {

struct BigScratch {
  float* xa;     // [B][NP][n]   particles
  float* xb;     // [B][NP][n]   gather target
  float* w;      // [B][NP]      weights
  float* ll;     // [B][NP]      log-likelihoods, then unnormalised weights, then normalised weights
  float* cdf;    // [B][NP]
  int* anc;      // [B][NP]
};

constexpr int BIG_NT = 1024;       // threads per trajectory
constexpr int BIG_NW = BIG_NT / 64;
constexpr int BIG_MAXCH = 1024;    // chunks per trajectory (N <= 2^20)

struct BpfAdd {
  __device__ __forceinline__ float operator()(float a, float c) const { return a + c; }
};
struct BpfMax {
  __device__ __forceinline__ float operator()(float a, float c) const { return nanmax(a, c); }
};

// the tree of block_tree_reduce continued over the chunk partials src[0 .. nchp) (LDS or global memory), nchp a power of
// two <= 1024: one value per thread; the butterfly of the first nchp threads only pairs them among themselves.  The caller
// orders the writers of src before the call.  red: 17 floats of LDS scratch.
template <class OP>
__device__ __forceinline__ float chunks_reduce(const float* src, int nchp, float* red, OP op) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float v = src[tid < nchp ? tid : 0];
  for (int off = 1; off < nchp && off < 64; off <<= 1) v = op(v, __shfl_xor(v, off, 64));
  if (nchp > 64) {
    lds_barrier();
    if (lane == 0) red[wave] = v;
    lds_barrier();
    const int nw = nchp / 64;
    float r = red[lane < nw ? lane : 0];
    for (int off = 1; off < nw; off <<= 1) r = op(r, __shfl_xor(r, off, 64));
    v = __shfl(r, 0, 64);
  } else {
    lds_barrier();
    if (tid == 0) red[16] = v;
    lds_barrier();
    v = red[16];
  }
  return v;
}

// the key a trajectory starts from: its carried key, else the launch key
__device__ __forceinline__ U32x2 bpf_start_key(const BpfCarry& carry, long long b, uint32_t key0, uint32_t key1) {
  if (carry.key_in) return U32x2{carry.key_in[b * 2], carry.key_in[b * 2 + 1]};
  return U32x2{key0, key1};
}

// particle i of trajectory b at step 0 and its weight: carried in, or drawn from the prior with key i + 1 of
// split(k, NP + 1) (whose key 0 the caller then goes on with)
template <int N, int DQ, int M>
__device__ __forceinline__ void initial_particle(const BpfModel<N, DQ, M>* __restrict__ mdlp, const BpfCarry& carry, long long b, int i, int NP,
                                                 U32x2 k, float* x, float* w) {
  if (carry.x_in) {
    BF_UNROLL for (int d = 0; d < N; ++d) x[d] = carry.x_in[(b * NP + i) * N + d];
    *w = carry.w_in[b * NP + i];
  } else {
    draw_initial_particle<N, DQ, M>(mdlp, k.x, k.y, (uint32_t)i, (uint32_t)NP, x);
    *w = 1.0f / (float)NP;
  }
}

// keys of a step that starts with key k: key 0 of split(k, NP + 1) (the particles' noise takes keys 1 .. NP), which a
// step that resamples splits once more into the key of the ancestor draw and the next step's
struct StepKeys {
  U32x2 draw, next;
};
__device__ __forceinline__ StepKeys bpf_step_keys(uint32_t k0, uint32_t k1, int NP, bool do_resample) {
  const U32x2 nk = threefry_split(k0, k1, 0u, (uint32_t)NP + 1u);
  if (!do_resample) return StepKeys{nk, nk};
  return StepKeys{threefry_split(nk.x, nk.y, 0u, 2u), threefry_split(nk.x, nk.y, 1u, 2u)};
}

// ancestor of particle i: systematic (resampler == 1) or multinomial position in [0, total], total = gc[NP - 1]; the first
// index whose CDF value reaches it (searchsorted side='left' over gc[0 .. NP) in global memory), clamped to NP - 1
__device__ __forceinline__ int draw_ancestor(U32x2 kc, int resampler, float total, const float* gc, int NP, int i) {
  float r;
  if (resampler == 1) r = (((float)i + bits_to_unit(threefry_bits(kc.x, kc.y, 0u, 1u))) / (float)NP) * total;
  else r = total * (1.0f - bits_to_unit(threefry_bits(kc.x, kc.y, (uint32_t)i, (uint32_t)NP)));
  int lo = 0, hi = NP;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gc[mid] < r) lo = mid + 1; else hi = mid;
  }
  return lo < NP - 1 ? lo : NP - 1;
}

// one particle through the dynamics with its own noise draw (inference.py:1342-1345: q = q0 + chol(Q) z from the
// particle's key), written back in place, and its emission log-density (:1348-1349)
// (MISSING: the log-density of the observed components, from the step's pattern and step density: emission_loglik_missing)
template <int N, int DQ, int M, class SP = SpecRuntime, bool MISSING = false>
__device__ __forceinline__ float propagate_particle(const BpfModel<N, DQ, M>& mdl, U32x2 ki, float* xp, float u0, const float* yv,
                                                    const float* sdens = nullptr, uint64_t obs = 0) {
  float x[N], q[DQ], xn[N];
  BF_UNROLL for (int d = 0; d < N; ++d) x[d] = xp[d];
  draw_dynamics_noise<N, DQ, M, SP>(mdl, ki, q);
  dyn_value<N, DQ, M, SP>(mdl, x, q, u0, xn);       // (SP::user_dyn / user_emi / user_lp: the caller's functions from source)
  BF_UNROLL for (int d = 0; d < N; ++d) xp[d] = xn[d];
  if constexpr (MISSING) return emission_loglik_missing<N, DQ, M, SP>(mdl, sdens, obs, xn, u0, yv);
  else return emission_loglik<N, DQ, M, SP>(mdl, xn, u0, yv);
}

// MISSING kernels with the particles in HBM: the observation pattern of a step, and the step density of a partly observed
// step of a Gaussian density from thread 0 into `sdens` (LDS).  Every thread of the workgroup calls it; the previous readers of
// `sdens` are a barrier back.  Every thread read the same y, so the pattern is the same in every lane; the readfirstlane says so
// to the compiler, and the barrier below stands in control flow that is convergent by construction.
template <int N, int DQ, int M, class SP>
__device__ __forceinline__ uint64_t bpf_step_pattern(const BpfModel<N, DQ, M>* mdlp, const float* yv, float* sdens) {
  const uint64_t o = bpf_observed_bits<M>(yv);
  const uint64_t obs = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o >> 32)) << 32);
  if (!SP::user_lp && obs != 0ull && obs != bpf_all_observed<M>()) {
    if (threadIdx.x == 0) bpf_step_density<M>(bpf_model_lp_cov(mdlp), obs, sdens);
    lds_barrier();
  }
  return obs;
}

template <int N, int DQ, int M, class SP = SpecRuntime, bool MISSING = false>
__device__ __forceinline__ void
bpf_big_body(const BpfModel<N, DQ, M>* __restrict__ mdlp, CView y, const float* __restrict__ uptr, long long u_sB, long long u_sT,
             BpfCarry carry, BpfOut out, BigScratch sc, long long B, long long T, int NP, float ess_threshold, int resampler,
             uint32_t key0, uint32_t key1) {
  const BpfModel<N, DQ, M>& mdl = *mdlp;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int nch = (NP + BIG_NT - 1) / BIG_NT;
  int nchp = 1;
  while (nchp < nch) nchp <<= 1;

  __shared__ float red[64];           // [0, 16) scan totals, [32, 49) reductions
  __shared__ float cpart[BIG_MAXCH];  // per-chunk partial results (max / sums / CDF totals)
  float* sdens = nullptr;             // MISSING: the step density of a partly observed step
  if constexpr (MISSING) {
    __shared__ float sdens_[bpf_density_words(M)];
    sdens = sdens_;
  }
  float* xa = sc.xa + b * (long long)NP * N;
  float* xb = sc.xb + b * (long long)NP * N;
  float* gw = sc.w + b * (long long)NP;
  float* gl = sc.ll + b * (long long)NP;
  float* gc = sc.cdf + b * (long long)NP;
  int* ganc = sc.anc + b * (long long)NP;

  // ---- initial particles
  U32x2 k = bpf_start_key(carry, b, key0, key1);
  for (int i = tid; i < NP; i += BIG_NT) initial_particle<N, DQ, M>(mdlp, carry, b, i, NP, k, xa + (long long)i * N, gw + i);
  if (!carry.x_in) k = threefry_split(k.x, k.y, 0u, (uint32_t)NP + 1u);
  __syncthreads();  // global-memory state written by other threads is read below

  for (long long t = 0; t < T; ++t) {
    float yv[M];
    BF_UNROLL for (int a = 0; a < M; ++a) yv[a] = y.p[b * y.sB + t * y.sT + a * y.sE];
    const float u0 = uptr ? uptr[b * u_sB + t * u_sT] : 0.f;
    uint64_t obs = 0;
    if constexpr (MISSING) obs = bpf_step_pattern<N, DQ, M, SP>(mdlp, yv, sdens);

    // ---- pass 1: propagate, log-weight, chunk maxima
    for (int c = 0; c < nch; ++c) {
      const int i = c * BIG_NT + tid;
      const bool valid = i < NP;
      float ll = -__builtin_inff();
      if (valid) {
        const U32x2 ki = threefry_split(k.x, k.y, (uint32_t)i + 1u, (uint32_t)NP + 1u);
        ll = propagate_particle<N, DQ, M, SP, MISSING>(mdl, ki, xa + (long long)i * N, u0, yv, sdens, obs);
        gl[i] = ll;
      }
      const float cm = block_tree_reduce<BIG_NW>(ll, red + 32, BpfMax());
      if (tid == 0) cpart[c] = cm;
    }
    for (int c = nch + tid; c < nchp; c += BIG_NT) cpart[c] = -__builtin_inff();
    lds_barrier();
    const float mx = chunks_reduce(cpart, nchp, red + 32, BpfMax());

    // ---- pass 2: unnormalised weights and their sum
    for (int c = 0; c < nch; ++c) {
      const int i = c * BIG_NT + tid;
      float e = 0.f;
      if (i < NP) {
#pragma clang fp contract(off)
        e = canon_exp(gl[i] - mx) * gw[i];
        gl[i] = e;
      }
      const float cs = block_tree_reduce<BIG_NW>(e, red + 32, BpfAdd());
      lds_barrier();
      if (tid == 0) cpart[c] = cs;
    }
    for (int c = nch + tid; c < nchp; c += BIG_NT) cpart[c] = 0.f;
    lds_barrier();
    const float tot = chunks_reduce(cpart, nchp, red + 32, BpfAdd());

    // ---- pass 3: normalise, effective sample size
    for (int c = 0; c < nch; ++c) {
      const int i = c * BIG_NT + tid;
      float w2 = 0.f;
      if (i < NP) {
#pragma clang fp contract(off)  // the product is rounded before it enters the tree
        const float wn = gl[i] / tot;
        gl[i] = wn;
        w2 = wn * wn;
      }
      const float cs = block_tree_reduce<BIG_NW>(w2, red + 32, BpfAdd());
      lds_barrier();
      if (tid == 0) cpart[c] = cs;
    }
    for (int c = nch + tid; c < nchp; c += BIG_NT) cpart[c] = 0.f;
    lds_barrier();
    const float ess = 1.0f / chunks_reduce(cpart, nchp, red + 32, BpfAdd());
    const bool do_resample = ess < ess_threshold * (float)NP;
    const StepKeys sk = bpf_step_keys(k.x, k.y, NP, do_resample);

    float* xcur = xa;
    if (do_resample) {
      // ---- pass 4a: chunk totals of the normalised weights (up-sweep order)
      for (int c = 0; c < nch; ++c) {
        const int i = c * BIG_NT + tid;
        const float ct = block_total_assoc<BIG_NW>(i < NP ? gl[i] : 0.f, red);
        lds_barrier();
        if (tid == 0) cpart[c] = ct;
      }
      for (int c = nch + tid; c < nchp; c += BIG_NT) cpart[c] = 0.f;
      lds_barrier();
      // scan of the chunk totals (nchp <= 1024 values, one per thread, same algorithm)
      {
        const float v = cpart[tid < nchp ? tid : 0];
        const float sv = block_cumsum_assoc<BIG_NW, true>(tid < nchp ? v : 0.f, red);
        lds_barrier();
        if (tid < nchp) cpart[tid] = sv;  // inclusive value at the end of chunk tid
        lds_barrier();
      }
      // ---- pass 4b: the CDF chunk by chunk, prefixed by the end of the previous chunk
      for (int c = 0; c < nch; ++c) {
        const int i = c * BIG_NT + tid;
        const float before = c > 0 ? cpart[c - 1] : 0.f;
        const float cv = block_cumsum_assoc<BIG_NW, true>(i < NP ? gl[i] : 0.f, red, before, true, cpart[c]);
        if (i < NP) gc[i] = cv;
      }
      __syncthreads();  // the CDF is read by every thread below
      // ---- pass 5: inverse-CDF draw and gather
      const float total = gc[NP - 1];
      for (int i = tid; i < NP; i += BIG_NT) {
        const int a = draw_ancestor(sk.draw, resampler, total, gc, NP, i);
        ganc[i] = a;
        BF_UNROLL for (int d = 0; d < N; ++d) xb[(long long)i * N + d] = xa[(long long)a * N + d];
        gw[i] = 1.0f / (float)NP;
      }
      xcur = xb;
    } else {
      for (int i = tid; i < NP; i += BIG_NT) {
        gw[i] = gl[i];
        ganc[i] = i;
      }
    }
    k = sk.next;
    __syncthreads();

    // ---- emit
    if (out.w || out.x || out.anc) {
      for (int i = tid; i < NP; i += BIG_NT) {
        if (out.w) out.w[b * out.w_sB + (long long)i * out.w_sN + t * out.w_sT] = gw[i];
        if (out.anc) out.anc[b * out.w_sB + (long long)i * out.w_sN + t * out.w_sT] = ganc[i];
        if (out.x) BF_UNROLL for (int d = 0; d < N; ++d)
            out.x[b * out.x_sB + (long long)i * out.x_sN + t * out.x_sT + d] = xcur[(long long)i * N + d];
      }
    }
    if (out.mean) {
      float part[N];
      BF_UNROLL for (int d = 0; d < N; ++d) part[d] = 0.f;
      for (int i = tid; i < NP; i += BIG_NT)
        BF_UNROLL for (int d = 0; d < N; ++d) part[d] = fmaf(gw[i], xcur[(long long)i * N + d], part[d]);
      BF_UNROLL for (int d = 0; d < N; ++d) {
        const float s = block_tree_reduce<BIG_NW>(part[d], red + 32, BpfAdd());
        if (tid == 0) out.mean[(b * T + t) * N + d] = s;
      }
    }
    if (tid == 0) {
      if (out.ess) out.ess[b * T + t] = ess;
      if (out.logz) out.logz[b * T + t] = mx + canon_log(tot);
      if (out.resampled) out.resampled[b * T + t] = do_resample ? 1.0f : 0.0f;
    }
    if (do_resample) {  // the gather target becomes the current buffer
      float* tmp = xa;
      xa = xb;
      xb = tmp;
    }
    __syncthreads();
  }

  for (int i = tid; i < NP; i += BIG_NT) {
    if (carry.x_out) BF_UNROLL for (int d = 0; d < N; ++d) carry.x_out[(b * NP + i) * N + d] = xa[(long long)i * N + d];
    if (carry.w_out) carry.w_out[b * NP + i] = gw[i];
  }
  if (tid == 0 && carry.key_out) {
    carry.key_out[b * 2] = k.x;
    carry.key_out[b * 2 + 1] = k.y;
  }
}

template <int N, int DQ, int M, bool MISSING = false>
__global__ void __launch_bounds__(BIG_NT)
bpf_big_kernel(const BpfModel<N, DQ, M>* __restrict__ mdlp, CView y, const float* __restrict__ uptr, long long u_sB, long long u_sT,
               BpfCarry carry, BpfOut out, BigScratch sc, long long B, long long T, int NP, float ess_threshold, int resampler,
               uint32_t key0, uint32_t key1) {
  bpf_big_body<N, DQ, M, SpecRuntime, MISSING>(mdlp, y, uptr, u_sB, u_sT, carry, out, sc, B, T, NP, ess_threshold, resampler, key0, key1);
}

#ifndef BF_JIT
// launch preparation of every particles-in-HBM kernel, the one built at run time (bpf_scan.hip) included: the capacity check
// and the stream-ordered scratch of a launch, carved from one allocation (*buf: the caller frees it on the stream after the
// launch) with `tail_bytes` left behind the BigScratch fields (*tail) for what a launcher adds
static inline int prepare_bpf_big(int n, long long B, int NP, hipStream_t stream, BigScratch& sc, float** buf, size_t tail_bytes = 0,
                                  void** tail = nullptr) {
  if (NP > BIG_NT * BIG_MAXCH)
    return set_error(BF_EUNSUPPORTED, "bootstrap particle filter: %d particles exceed the capacity of %d per trajectory", NP,
                     BIG_NT * BIG_MAXCH);
  const size_t per = (size_t)B * NP;
  BF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(buf), sizeof(float) * per * (2 * (size_t)n + 3) + sizeof(int) * per + tail_bytes, stream));
  sc.xa = *buf;
  sc.xb = sc.xa + per * n;
  sc.w = sc.xb + per * n;
  sc.ll = sc.w + per;
  sc.cdf = sc.ll + per;
  sc.anc = reinterpret_cast<int*>(sc.cdf + per);
  if (tail) *tail = sc.anc + per;
  return BF_OK;
}

// the observation and input arguments of the kernels, from the caller's descriptors (`u` NULL or u->ptr NULL: no inputs)
struct BpfInputs {
  CView y;
  const float* u;
  long long u_sB, u_sT;
};
static inline BpfInputs bpf_inputs(const bf_cstream* y, const bf_cstream* u) {
  return BpfInputs{CView{y->ptr, y->sB, y->sT, y->sE}, (u && u->ptr) ? u->ptr : nullptr, u ? u->sB : 0, u ? u->sT : 0};
}

template <int N, int DQ, int M, bool MISSING = false>
static inline int launch_bpf_big_dims(const BpfModel<N, DQ, M>* d_mdl, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                                 int NP, float ess, int resampler, const uint32_t key[2], const BpfCarry& cr, const BpfOut& out,
                                 hipStream_t stream) {
  BigScratch sc;
  float* buf = nullptr;
  const int rc = prepare_bpf_big(N, B, NP, stream, sc, &buf);
  if (rc != BF_OK) return rc;
  const BpfInputs in = bpf_inputs(y, u);
  hipLaunchKernelGGL((bpf_big_kernel<N, DQ, M, MISSING>), dim3((unsigned)B), dim3(BIG_NT), 0, stream, d_mdl, in.y, in.u, in.u_sB, in.u_sT, cr, out,
                     sc, B, T, NP, ess, resampler, key[0], key[1]);
  const hipError_t le = hipGetLastError();
  const hipError_t fe = hipFreeAsync(buf, stream);
  BF_HIP_CHECK(le);
  BF_HIP_CHECK(fe);
  return BF_OK;
}
#endif  // BF_JIT

}  // namespace bf
