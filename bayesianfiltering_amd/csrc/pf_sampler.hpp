// Particle smoothing: joint draws x_{0:T-1} ~ p(x_{0:T-1} | y_{0:T-1}) from the history a bootstrap particle filter stored
// (bf_bpf_f32: weights w[i,t], particles x[i,t,:], ancestors a[i,t]), by backward simulation (Godsill, Doucet & West 2004)
// or by tracing the filter's own genealogy.
//
// THE CONTRACT (restated in include/bayesfilt.h; the float64 oracle of tests/test_particle_sampler_cpu.py implements it).
// Per trajectory b, sample s and step t a uniform v[s,t] in [0,1) is given.
//
//   draw(l, v):  M = max_i l_i;  e_i = exp(l_i - M);  c = inclusive cumulative sum of e in index order;
//                the result is the smallest j with c_j > v c_{N-1}, clamped to N-1 ("greater than": in exact arithmetic a
//                drawn particle never has e_j = 0).  M not finite (NaN, or every logit -inf / +inf): the draw is INVALID.
//
//   backward simulation:
//     t = T-1 without a carry:   l_i = log w[i,T-1]
//     every other step (and T-1 with a carry):
//                                l_i = log w[i,t] - 1/2 |L^-1 (x~_{t+1} - mu_i)|^2,   mu_i = f(x[i,t], q0, u_{t+1}),
//                                L = lower Cholesky factor of F_q Q F_q^T (constant for every registry dynamics function);
//                                the Gaussian's normalising constant is common to all i and dropped
//     j_t = draw(l, v[s,t]),  x~_t = x[j_t,t,:]  -- an exact copy of a stored particle
//
//   genealogy:  j_{T-1} = draw(log w[:,T-1], v[s,T-1]) (or the carried slot), j_{t-1} = a[j_t,t], x~_t = x[j_t,t,:].
//               With the same uniforms both methods return the same x~_{T-1}, bit for bit.
//
//   An invalid draw writes NaN and index -1 at that step and at every earlier step of that sample, and into the carry;
//   other samples and trajectories are untouched.
//
//   Carry (chunks run backwards in time): a chunk hands x~ at its first step (B,S,n) to the chunk before it, which also
//   needs the input u of that step (B,) -- the u_{t+1} of its own last step -- and, for the genealogy, the slot
//   a[j_{t0},t0] (B,S).
//
//   Uniforms: given (noise mode), or from keys[b] (key mode): v[s,t] = bits_to_unit(threefry_bits(keys[b], s T + t, S T)),
//   which is jax.random.uniform(keys[b], (S,T)).  The two modes agree bit for bit.
//
// THE ARITHMETIC (fp32).  Particle i sits in lane i / R, register row i % R of the sample's wave, R = ceil(N / 64) -- a
// function of N alone, so a sample's bits do not depend on S, on B or on which samples share a launch.  The logit is
// log w - 1/2 sum_k (z~_k - z_ik)^2 with the WHITENED z~ = L^-1 x~_{t+1}, z_i = L^-1 mu_i (direct differences, summed in k
// order by fma; not |z~|^2 + |z_i|^2 - 2 z~ . z_i, which cancels).  log / exp are the hardware's v_log_f32 / v_exp_f32.  c_i is
// formed in two levels: a running sum over a lane's rows, plus the exclusive 64-lane scan (Hillis-Steele) of the lanes'
// totals; c_{N-1} is the value of the last slot.  Two slots on either side of a lane boundary may therefore disagree by a
// rounding, which the parity test's tolerance covers.
//
// THE MAPPING.  Backward simulation: one workgroup per (trajectory, group of samples), one wave per sample.  Per step the
// WORKGROUP evaluates f and the whitening once per particle into LDS (float4 chunks of z_i plus log w_i, laid out so that a
// wave's reads are consecutive 16-byte slots), tile by tile when N exceeds a tile; each WAVE keeps its <= 64 logits per lane in registers,
// takes the maximum and the prefix sum with wave operations, and every lane loads the drawn particle (one address).  Cost per
// step and sample: O(N n) VALU for the quadratic forms; f costs O(N) per group, not per sample.
// Genealogy: one wave per (trajectory, sample): the same draw streamed from memory, then a dependent gather chain.
#pragma once
#include <cstring>
#include <vector>
#include "bf_common.hpp"
#include "bf_rng.hpp"
#include "kf_math.hpp"
#include "models.hpp"
#include "ssm_device.hpp"

namespace bf {

constexpr int PFS_MAX_PARTICLES = 4096;  // backward simulation: 64 lanes x 64 register rows
constexpr int PFS_MAX_DIM = 16;          // the particle filter's range of state dimensions

// what the backward kernel needs of the model: g(x, u) through dyn_base_t (dyn_id, dth, A), the bias F_q q0 and the inverse
// of the Cholesky factor of F_q Q F_q^T
template <int N>
struct PfsModel {
  int dyn_id, pad0_;
  float dth[8];
  float A[N * N];
  float c[N];        // F_q q0
  float Li[N * N];   // L^-1, lower triangular, row-major
};

struct PfsViews {
  const float* w;      // weights (b, i, t)
  long long w_sB, w_sN, w_sT;
  const float* x;      // particles (b, i, t, :), innermost stride 1
  long long x_sB, x_sN, x_sT;
  const int* a;        // ancestors, the weights' strides
  const float* u;      // inputs (b, t), NULL = zeros
  long long u_sB, u_sT;
  float* out;          // samples (b, s, t, e)
  long long o_sB, o_sS, o_sT, o_sE;
  int* idx;            // optional [B][S][T]
  const float* noise;  // uniforms (b, s, t), NULL = from keys
  long long z_sB, z_sS, z_sT;
  const uint32_t* keys;
  const float* x_in;   // carry
  const float* u_in;
  const int* a_in;
  float* x_out;
  int* a_out;
};

// particles per LDS tile of the backward kernel: (4 ceil(n / 4) + 1) floats per particle, at most 52 KiB
template <int N>
constexpr int pfs_tile() { return N <= 12 ? 1024 : 512; }

__device__ __forceinline__ float pfs_wave_max(float v) {
  BF_UNROLL for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// inclusive sum over the 64 lanes in a fixed order (Hillis-Steele)
__device__ __forceinline__ float pfs_wave_scan(float v, int lane) {
  BF_UNROLL for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ float pfs_nan() { return __builtin_nanf(""); }

__device__ __forceinline__ float pfs_uniform(const PfsViews& v, long long b, int s, long long t, long long T, int S) {
  if (v.noise) return v.noise[b * v.z_sB + s * v.z_sS + t * v.z_sT];
  return bits_to_unit(threefry_bits(v.keys[2 * b], v.keys[2 * b + 1], (uint32_t)s * (uint32_t)T + (uint32_t)t,
                                    (uint32_t)S * (uint32_t)T));
}

// From a lane's running sum `run` (its total) to the lane's offset and the threshold v * c_{N-1}.
__device__ __forceinline__ void pfs_offsets(float run, float unif, int lane, float& off, float& th) {
  const float incl = pfs_wave_scan(run, lane);
  off = __shfl_up(incl, 1);
  if (lane == 0) off = 0.f;
  const float total = __shfl(off + run, 63);   // c of the last slot
  th = unif * total;
}
// rhit: the lane's first row with c > th (-1: none).  Smallest index overall: the first lane with a hit.
__device__ __forceinline__ int pfs_pick(int rhit, int R, int NP) {
  const unsigned long long mask = __ballot(rhit >= 0);
  if (mask == 0ull) return NP - 1;
  const int L = __ffsll((long long)mask) - 1;
  const int j = L * R + __shfl(rhit, L);
  return j < NP ? j : NP - 1;
}

// ---- backward simulation ---------------------------------------------------------------------------------------------
// RMAX: register rows per lane (N <= 64 RMAX); WAVES: samples per workgroup at most (launch bound)
template <int N, int RMAX, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) pfs_backward_kernel(PfsModel<N> kmdl, const PfsModel<N>* __restrict__ dmdl, PfsViews v, long long T, int NP, int S, int groups) {
  constexpr int NC4 = (N + 3) / 4;
  constexpr int TP = pfs_tile<N>();
  constexpr int RT = TP / 64;   // register rows per tile
  constexpr int LDR = 65;       // slots per row: the staging threads' writes (consecutive rows of one lane) spread over the banks
  __shared__ float4 zs[NC4 * RT * LDR];
  __shared__ float lw[RT * LDR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  // The model's matrices are scalar operands read from the kernel argument up to n = 8.  Beyond, there are more of them than
  // scalar registers, and hoisted out of the loops they would spill: they are then read from memory (dmdl, the same block)
  // through a pointer the compiler cannot see through, i.e. where they are used.
  auto model = [&]() -> const PfsModel<N>& {
    if constexpr (N > 8) {
      long long zero;
      asm volatile("s_mov_b64 %0, 0" : "=s"(zero));
      return *reinterpret_cast<const PfsModel<N>*>(reinterpret_cast<const char*>(dmdl) + zero);
    } else {
      return kmdl;
    }
  };
  const long long b = blockIdx.x / groups;
  const int s = (int)(blockIdx.x % groups) * nw + wave;
  const bool active = s < S;
  const int R = (NP + 63) / 64;
  float p[RMAX];
  float zt[N];   // L^-1 x~_{t+1}
  BF_UNROLL for (int k = 0; k < N; ++k) zt[k] = 0.f;
  bool dead = false;

  auto whiten = [&](const float* xv, float* z) {
    const PfsModel<N>& mdl = model();
    BF_UNROLL for (int k = 0; k < N; ++k) {
      float a = mdl.Li[k * N] * xv[0];
      BF_UNROLL for (int l = 1; l <= k; ++l) a = fmaf(mdl.Li[k * N + l], xv[l], a);
      z[k] = a;
    }
  };
  if (v.x_in && active) {
    float xn[N];
    BF_UNROLL for (int k = 0; k < N; ++k) xn[k] = v.x_in[((long long)b * S + s) * N + k];
    whiten(xn, zt);
  }

  for (long long t = T - 1; t >= 0; --t) {
    const bool trans = t < T - 1 || v.x_in != nullptr;
    float u1 = 0.f;
    if (trans) {
      if (t == T - 1) u1 = v.u_in ? v.u_in[b] : 0.f;
      else u1 = v.u ? v.u[b * v.u_sB + (t + 1) * v.u_sT] : 0.f;
    }
    float M = -__builtin_inff();
    bool isnan_ = false;
    for (int r0 = 0; r0 < R; r0 += RT) {   // tiles of RT rows: uniform over the workgroup
      {
        __syncthreads();   // the previous tile (or step) has been read
        const int rows = (R - r0) < RT ? (R - r0) : RT;
        for (int q = tid; q < 64 * rows; q += blockDim.x) {
          const int ln = q / rows, rr = q - ln * rows;
          const int i = ln * R + r0 + rr, pos = rr * LDR + ln;
          float z[4 * NC4];
          BF_UNROLL for (int k = 0; k < 4 * NC4; ++k) z[k] = 0.f;
          float l = -__builtin_inff();
          if (i < NP) {
            l = fast_log(v.w[b * v.w_sB + i * v.w_sN + t * v.w_sT]);
            if (trans) {
              const float* xp = v.x + b * v.x_sB + i * v.x_sN + t * v.x_sT;
              const PfsModel<N>& mdl = model();
              float xv[N], mu[N];
              BF_UNROLL for (int k = 0; k < N; ++k) xv[k] = xp[k];
              dyn_base_t<N, N, PfsModel<N>>(mdl, xv, u1, mu);
              BF_UNROLL for (int k = 0; k < N; ++k) mu[k] += mdl.c[k];
              whiten(mu, z);
            }
          }
          lw[pos] = l;
          BF_UNROLL for (int c = 0; c < NC4; ++c) zs[c * RT * LDR + pos] = make_float4(z[4 * c], z[4 * c + 1], z[4 * c + 2], z[4 * c + 3]);
        }
        __syncthreads();
        if (active && !dead) {
          // the tile's rows into the registers p[r0 ... r0 + RT): compile-time register indices, one copy of the body per row
          BF_UNROLL for (int r = 0; r < RMAX; ++r) {
            const int rr = r % RT;
            if (r / RT == r0 / RT && r < R) {
              const int pos = rr * LDR + lane;
              float l = lw[pos];
              if (trans) {
                float qd = 0.f;
                BF_UNROLL for (int c = 0; c < NC4; ++c) {
                  const float4 zz = zs[c * RT * LDR + pos];
                  const float zc[4] = {zz.x, zz.y, zz.z, zz.w};
                  BF_UNROLL for (int k = 0; k < 4; ++k)
                    if (4 * c + k < N) {
                      const float d = zt[4 * c + k] - zc[k];
                      qd = fmaf(d, d, qd);
                    }
                }
                l = fmaf(-0.5f, qd, l);
              }
              p[r] = l;
              isnan_ = isnan_ || (l != l);
              M = fmaxf(M, l);
            }
          }
        }
      }
    }
    if (active && !dead) {
      M = pfs_wave_max(M);
      const bool bad = __ballot(isnan_) != 0ull || !(fabsf(M) < __builtin_inff());
      if (bad) {
        dead = true;
      } else {
        float run = 0.f;
        BF_UNROLL for (int r = 0; r < RMAX; ++r)
          if (r < R) {
            run += fast_exp(p[r] - M);
            p[r] = run;
          }
        float off, th;
        pfs_offsets(run, pfs_uniform(v, b, s, t, T, S), lane, off, th);
        int rhit = -1;
        BF_UNROLL for (int r = RMAX - 1; r >= 0; --r)
          if (r < R && off + p[r] > th) rhit = r;
        const int j = pfs_pick(rhit, R, NP);
        const float* xp = v.x + b * v.x_sB + (long long)j * v.x_sN + t * v.x_sT;
        float xn[N];
        BF_UNROLL for (int k = 0; k < N; ++k) xn[k] = xp[k];
        whiten(xn, zt);
        float* op = v.out + b * v.o_sB + s * v.o_sS + t * v.o_sT;
        BF_UNROLL for (int k = 0; k < N; ++k)
          if (lane == k) op[k * v.o_sE] = xn[k];
        if (v.idx && lane == 0) v.idx[((long long)b * S + s) * T + t] = j;
        if (t == 0 && v.x_out)
          BF_UNROLL for (int k = 0; k < N; ++k)
            if (lane == k) v.x_out[((long long)b * S + s) * N + k] = xn[k];
      }
    }
    if (active && dead) {
      float* op = v.out + b * v.o_sB + s * v.o_sS + t * v.o_sT;
      if (lane < N) op[lane * v.o_sE] = pfs_nan();
      if (v.idx && lane == 0) v.idx[((long long)b * S + s) * T + t] = -1;
      if (t == 0 && v.x_out && lane < N) v.x_out[((long long)b * S + s) * N + lane] = pfs_nan();
    }
  }
}

// ---- genealogy -------------------------------------------------------------------------------------------------------
// One wave per (trajectory, sample), four per workgroup.  The draw at T-1 is the backward kernel's, operation for operation,
// with the logits recomputed from memory in each of its three passes instead of held in registers (any N).
__global__ void __launch_bounds__(256) pfs_trace_kernel(PfsViews v, long long B, long long T, int NP, int n, int S) {
  const int lane = threadIdx.x & 63;
  const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= B * S) return;
  const long long b = gw / S;
  const int s = (int)(gw - b * S);
  const int R = (NP + 63) / 64;
  int j;
  if (v.a_in) {
    j = v.a_in[b * S + s];
  } else {
    const float* wp = v.w + b * v.w_sB + (T - 1) * v.w_sT;
    const int i0 = lane * R;
    float M = -__builtin_inff();
    bool isnan_ = false;
    for (int r = 0; r < R; ++r) {
      const float l = (i0 + r < NP) ? fast_log(wp[(long long)(i0 + r) * v.w_sN]) : -__builtin_inff();
      isnan_ = isnan_ || (l != l);
      M = fmaxf(M, l);
    }
    M = pfs_wave_max(M);
    if (__ballot(isnan_) != 0ull || !(fabsf(M) < __builtin_inff())) {
      j = -1;
    } else {
      float run = 0.f;
      for (int r = 0; r < R; ++r) {
        const float l = (i0 + r < NP) ? fast_log(wp[(long long)(i0 + r) * v.w_sN]) : -__builtin_inff();
        run += fast_exp(l - M);
      }
      float off, th;
      pfs_offsets(run, pfs_uniform(v, b, s, T - 1, T, S), lane, off, th);
      int rhit = -1;
      run = 0.f;
      for (int r = 0; r < R; ++r) {
        const float l = (i0 + r < NP) ? fast_log(wp[(long long)(i0 + r) * v.w_sN]) : -__builtin_inff();
        run += fast_exp(l - M);
        if (rhit < 0 && off + run > th) rhit = r;
      }
      j = pfs_pick(rhit, R, NP);
    }
  }
  for (long long t = T - 1; t >= 0; --t) {
    if (j < 0 || j >= NP) j = -1;   // an invalid draw, or an ancestor slot that is no particle index
    float* op = v.out + b * v.o_sB + s * v.o_sS + t * v.o_sT;
    const float* xp = v.x + b * v.x_sB + (long long)(j < 0 ? 0 : j) * v.x_sN + t * v.x_sT;
    for (int k = lane; k < n; k += 64) {
      const float xv = j < 0 ? pfs_nan() : xp[k];
      op[k * v.o_sE] = xv;
      if (t == 0 && v.x_out) v.x_out[((long long)b * S + s) * n + k] = xv;
    }
    if (v.idx && lane == 0) v.idx[((long long)b * S + s) * T + t] = j;
    if (j >= 0) j = v.a[b * v.w_sB + (long long)j * v.w_sN + t * v.w_sT];
  }
  if (v.a_out && lane == 0) v.a_out[b * S + s] = (j < 0 || j >= NP) ? -1 : j;
}

}  // namespace bf
