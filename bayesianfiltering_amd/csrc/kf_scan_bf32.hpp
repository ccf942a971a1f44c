// kf_scan_bf32: batched Kalman filter for n <= 32, m <= 32 on the matrix cores, ONE WAVE per chain.
//
// The same recursion and the same three-term bf16 products as kf_scan_mfma.hip (which explains both).  Every matrix is a
// single 32 x 32 tile, so the whole step --
// Z = P-^T H^T, S^T = H Z, the two factorizations, P+ = P- - W^T W + c c^T, Y^T = P+^T A^T, P- = Y A^T + G Q G^T, all as
// three-term bf16 products -- runs inside one wave without a single barrier (a wave's LDS traffic executes in issue
// order), no wave ever waits for another's factorization, and the CU holds eight independent trajectories (16.6 KB of LDS
// each, two per workgroup) instead of two workgroups with three of four waves idle through the serial phase.
// Smaller models ride zero-padded in the tile exactly as in launch_kf_mfma.
//
// This header holds the kernel and what its instances share; kf_scan_bf32.hip instantiates the eight plain kernels (and holds
// the launcher, launch_kf_bf32), kf_scan_bf32_missing.hip their eight MISSING = true twins, so that the plain ones are compiled
// exactly as before.
#pragma once
#include "forward_host.hpp"
#include "lgssm_pack.hpp"
#include "mfma_multi.hpp"
#include "mfma_tiles.hpp"

namespace bf {

struct Bf32Const {
  unsigned short A3[3][32 * 32], H3[3][32 * 32];
  float GQG[32 * 32], DRD[32 * 32], Gq0[32], Dr0[32];
  float dth[8];   // DYN != 0: the registry dynamics' scalars (Lorenz-96: alpha, beta, gamma, dt, mode; sine: w0)
};
__device__ __forceinline__ float dot_terms32(const u32x4 (*x)[2], const float* v, int lk) {  // sum over the lane's 16 k
  float s = 0.f;
  BF_UNROLL for (int c = 0; c < 2; ++c) BF_UNROLL for (int d = 0; d < 4; ++d) {
    const float x0 = (bf_lo(x[0][c][d]) + bf_lo(x[1][c][d])) + bf_lo(x[2][c][d]);
    const float x1 = (bf_hi(x[0][c][d]) + bf_hi(x[1][c][d])) + bf_hi(x[2][c][d]);
    s = fmaf(x0, v[16 * c + 8 * lk + 2 * d], s);
    s = fmaf(x1, v[16 * c + 8 * lk + 2 * d + 1], s);
  }
  return s;
}
// one 32 x 32 accumulator tile of a [nr][nr] stream entry at (b, t)
__device__ __forceinline__ void store_tile32(const SView& sv, long long b, long long t, int lane, const f32x16& acc, int nr, int k = 0) {
  if (!sv.p) return;
  const int lr = lane & 31, lk = lane >> 5;
  gl_f* base = per_step(sv.p + b * sv.sB + k * sv.sK + t * sv.sT);
  const long long sE = sv.sE + (long long)opaque_szero();
  BF_UNROLL for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * lk;
    if (lr < nr && row < nr) __builtin_nontemporal_store(acc[r], base + (long long)(row * nr + lr) * sE);
  }
}

// the step's ONE factorization (LL: the log-likelihood comes from it too), out of line: a register allocation of its own
inline __device__ __attribute__((noinline)) float chol_w_rows_bf32(lds_f* sc, lds_f* sT, lds_f* sv, lds_f* mcur, lds_f* mnxt, lds_f* scv, lds_c* wt,
                                                            int lane) {
  return chol_w_rows_impl<32, true>(sc, sT, sv, mcur, mnxt, scv, wt, lane);
}

// bytes per trajectory: [P-/P+ terms | fp32 H P and S, which live only between the last read of P-'s terms (phase A) and the
// factorization's first instructions, while that buffer is idle] + [Z / W^T / Y^T terms] + four 32-vectors
constexpr int BF32_PN_BYTES = 2 * 32 * 33 * 4;   // 8 448 >= 3 * 32 * 80
constexpr int BF32_WAVE_LDS = BF32_PN_BYTES + 3 * 32 * 80 + 4 * 32 * 4;

// MULTI: the K Gaussian-sum components of a LINEAR model (inference.py:345-353 vmaps _condition_on / _predict over them).  Their
// mean / covariance recursions do not depend on the weights, so every (trajectory, component) pair is a chain of its own:
// chain c = trajectory * K + component reads trajectory c / K's observations, writes component c % K's streams and its
// per-step log-likelihood; the weight recursion (the only coupling) runs afterwards over the stored log-likelihoods
// (gsf_reweight_kernel).  B counts chains.  TV: per-step G Q_t G^T / D R_t D^T tables (_get_params(x, 2, t),
// inference.py:21,337-340) instead of the constants of Bf32Const.
// DYN: 0 = linear dynamics (A as constant operand registers); 1 = Lorenz-96, 2 = sine (models.hpp: DYN_LORENZ96 / DYN_SINE):
// an extended Kalman filter chain -- row lr of F = df/dx at the filtered mean is evaluated analytically every step
// (inference.py:328, :61-62 take it with jacfwd), split into its three bf16 terms in the SAME operand registers, and the
// predicted mean is f(m+) + F_q q0 instead of A m+ + G q0 (identity noise input).
// MISSING: a NaN y(b, t, a) is a component that was not observed at step t (include/bayesfilt_ext2.h).  A missing row is a
// PADDED row for that step -- the mechanism that lets m < 32 ride in the tile: its row of H is zero, D R D^T has a unit
// diagonal entry and nothing else in its row and column, its innovation is 0, and its log N(0; 0, 1) leaves the
// log-likelihood through ll_pad.  One wave owns one trajectory, so the step's pattern is a wave-uniform word (a ballot of
// the prefetched observation) and nothing diverges; every component chain of a MULTI trajectory derives it from the same y.
// Everything is a select or a bit mask, never a multiplication: the NaN never reaches arithmetic.  A step with no observed
// row skips the update altogether (a wave-uniform branch; this kernel has no workgroup barrier): m+ = m-, P+ = P- with its
// terms still intact in Pn (the fp32 overlay was never written), log-likelihood exactly 0.
template <bool MULTI, bool TV, int DYN = 0, bool MISSING = false>
__global__ void __launch_bounds__(128, 2)
kf_scan_bf32_kernel(const Bf32Const* __restrict__ cst, CView y, CarryView carry, OutViews out, long long B, long long T, int nr, int mr,
                    int K, const float* __restrict__ tvq, const float* __restrict__ tvr) {
  constexpr int PITCH = 80, TERM = 32 * PITCH, PS = 33;
  const int lane = threadIdx.x & 63;
  const int lr = lane & 31, lk = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long b_raw = (long long)blockIdx.x * 2 + wv;
  if (b_raw >= B) return;   // (no workgroup barrier anywhere below)
  const long long b = b_raw;                       // chain: carry index
  const long long bt = MULTI ? b / K : b;          // trajectory: observations, stream batch index
  const int kc = MULTI ? (int)(b % K) : 0;         // component: stream component index

  extern __shared__ __attribute__((aligned(16))) float lds[];
  lds_c* L = (lds_c*)reinterpret_cast<char*>(lds) + wv * BF32_WAVE_LDS;
  lds_c* Pn = L;                       // [3][32][80 B]  P- / P+, transposed terms
  lds_c* Zn = L + BF32_PN_BYTES;       // [3][32][80 B]  Z = (H P-)^T; later W^T, then Y^T
  lds_c* Wt = Zn;
  lds_c* Yn = Zn;
  float* sHP = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + wv * BF32_WAVE_LDS);   // [32][33] H P- (fp32), over Pn
  float* sc = sHP + 32 * PS;           // [32][33]  S, over Pn
  float* sm = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + wv * BF32_WAVE_LDS + BF32_PN_BYTES + 3 * TERM);   // [32] predicted mean
  float* sm2 = sm + 32;                // [32] filtered mean
  float* sv = sm2 + 32;                // [32] innovation
  float* scv = sv + 32;                // [32] 1e-3 W^T g

  u32x4 hop[3][2], aop[3][2];          // row lr of H and of A as bf16 terms
  BF_UNROLL for (int q = 0; q < 3; ++q) BF_UNROLL for (int c = 0; c < 2; ++c) {
    hop[q][c] = *reinterpret_cast<const u32x4*>(&cst->H3[q][lr * 32 + 16 * c + 8 * lk]);
    if constexpr (DYN == 0) aop[q][c] = *reinterpret_cast<const u32x4*>(&cst->A3[q][lr * 32 + 16 * c + 8 * lk]);
  }
  const float dr0 = cst->Dr0[lr], gq0 = cst->Gq0[lr];
  f32x16 Pacc;
  BF_UNROLL for (int r = 0; r < 16; ++r) {
    const int row = c_row(r, lane);
    Pacc[r] = (lr < nr && row < nr) ? carry.P_in[b * nr * nr + row * nr + lr] : 0.f;
  }
  store_terms_transposed(Pn, TERM, PITCH, 0, 0, lane, Pacc);
  sm[lr] = lr < nr ? carry.m_in[b * nr + lr] : 0.f;
  float w = (!MULTI && carry.w_in) ? carry.w_in[b] : 1.0f;
  float ynext = lr < mr ? y.p[bt * y.sB + lr * y.sE] : 0.f;
  const float ll_pad = 0.5f * 1.8378770664093453f * (float)(32 - mr);
  wave_lds_order();

  for (long long t = 0; t < T; ++t) {
    const float yv = ynext;
    {
      const long long tn = t + 1 < T ? t + 1 : t;
      if (lr < mr) ynext = y.p[bt * y.sB + tn * y.sT + lr * y.sE];
    }
    gl_cf* const drd_t = TV && tvr ? per_step(tvr + t * 1024) : per_step(cst->DRD);
    gl_cf* const gqg_t = TV && tvq ? per_step(tvq + t * 1024) : per_step(cst->GQG);
    // MISSING: the step's pattern.  Bit a of `obs` (wave-uniform): component a is observed; bits at or above mr are never set.
    // +-Inf is observed (and poisons).  `here`: this lane's row lr; `upd`: the step has an update at all.
    unsigned obs = 0;
    bool here = true, upd = true;
    if constexpr (MISSING) {
      obs = (unsigned)__builtin_amdgcn_ballot_w64(lr < mr && yv == yv);   // (lanes 32 .. 63 repeat rows 0 .. 31)
      here = (obs >> lr) & 1u;
      upd = obs != 0u;
    }
    float ll = 0.f;
    if (upd) {
      u32x4 hst[3][2];   // row lr of H for this step; MISSING: zero while the row is missing (a bit mask on the packed bf16 words)
      BF_UNROLL for (int q = 0; q < 3; ++q) BF_UNROLL for (int c = 0; c < 2; ++c) hst[q][c] = MISSING ? hop[q][c] & (here ? 0xffffffffu : 0u) : hop[q][c];
      // ---- Z = P-^T H^T; H P- in fp32 for the forward substitution; innovation
      {
        f32x16 z = {0};
        BF_UNROLL for (int c = 0; c < 2; ++c) {
          u32x4 a[3];
          load_terms(a, Pn, TERM, PITCH, lr, c, lk);
          const u32x4 bh[3] = {hst[0][c], hst[1][c], hst[2][c]};
          z = mfma_bf6(a, bh, z);
        }
        wave_lds_order();   // P-'s terms have been read: their buffer now takes H P (fp32) and, below, S
        BF_UNROLL for (int r = 0; r < 16; ++r) sHP[lr * PS + c_row(r, lane)] = z[r];
        store_terms_transposed(Zn, TERM, PITCH, 0, 0, lane, z);
        float s = dot_terms32(hst, sm, lk);
        s += __shfl_xor(s, 32, 64);
        sv[lr] = here ? yv - (s + dr0) : 0.f;   // (MISSING: a select, so the NaN of a missing entry goes nowhere)
      }
      wave_lds_order();
      // ---- S^T = H Z + (D R D^T)^T
      {
        f32x16 acc;
        BF_UNROLL for (int r = 0; r < 16; ++r) acc[r] = drd_t[lr * 32 + c_row(r, lane)];
        if constexpr (MISSING) {   // a missing row or column of D R D^T is a padded one: unit diagonal, nothing else
          const unsigned obs_lk = obs >> (4 * lk);   // bit (r & 3) + 8 (r >> 2): row c_row(r, lane)
          BF_UNROLL for (int r = 0; r < 16; ++r) {
            const bool both = here && ((obs_lk >> ((r & 3) + 8 * (r >> 2))) & 1u);
            acc[r] = both ? acc[r] : (lr == c_row(r, lane) ? 1.0f : 0.f);
          }
        }
        BF_UNROLL for (int c = 0; c < 2; ++c) {
          u32x4 bz[3];
          load_terms(bz, Zn, TERM, PITCH, lr, c, lk);
          const u32x4 ah[3] = {hst[0][c], hst[1][c], hst[2][c]};
          acc = mfma_bf6(ah, bz, acc);
        }
        BF_UNROLL for (int r = 0; r < 16; ++r) sc[lr * PS + c_row(r, lane)] = acc[r];
      }
      wave_lds_order();
      // ---- ONE factorization, chol(S + 1e-6): W^T (over Z's terms), c, m+, and the log-likelihood of the un-jittered S
      // (MISSING: the padding is the step's -- with every row observed the same float as the constant)
      float pad = ll_pad;
      if constexpr (MISSING) {
#pragma clang fp contract(off)   // a product rounded on its own, like ll_pad: fused into the sum below it is another float
        pad = 0.5f * 1.8378770664093453f * (float)(32 - __builtin_popcount(obs));
      }
      ll = chol_w_rows_bf32((lds_f*)sc, (lds_f*)sHP, (lds_f*)sv, (lds_f*)sm, (lds_f*)sm2, (lds_f*)scv, Wt, lane) + pad;
    } else {
      sm2[lr] = sm[lr];   // nothing observed: m+ = m-; P+ = P- is Pacc, its terms still stand in Pn; ll = 0
    }
    wave_lds_order();
    // ---- P+ = P- - W^T W + c c^T; filtered streams
    {
      f32x16 acc = Pacc;
      if (upd) {
        BF_UNROLL for (int c = 0; c < 2; ++c) {
          u32x4 a[3], bw[3];
          load_terms(bw, Wt, TERM, PITCH, lr, c, lk);
          BF_UNROLL for (int q = 0; q < 3; ++q) a[q] = bw[q] ^ 0x80008000u;
          acc = mfma_bf6(a, bw, acc);
        }
        const float cv = lk == 0 ? scv[lr] : 0.f;
        acc = mfma2(cv, cv, acc);
      }
      store_tile32(out.P, bt, t, lane, acc, nr, kc);
      wave_lds_order();   // (W^T's terms are read before Y^T overwrites them below; P-'s before P+'s here)
      if (upd) store_terms_transposed(Pn, TERM, PITCH, 0, 0, lane, acc);
      if (out.m.p && lane < nr) out.m.p[bt * out.m.sB + kc * out.m.sK + t * out.m.sT + lane * out.m.sE] = sm2[lane];
      if (lane == 0) {
        if constexpr (!MULTI) {
          w = reweight_single(ll, w);
          if (out.w.p) out.w.p[b * out.w.sB + t * out.w.sT] = w;
        }
        if (out.ll.p) out.ll.p[bt * out.ll.sB + kc * out.ll.sK + t * out.ll.sT] = ll;   // (MULTI: the launcher always provides it)
      }
    }
    wave_lds_order();
    float fval = 0.f;
    if constexpr (DYN != 0) {   // F's row lr at the filtered mean (sm2), columns 16 c + 8 lk + e, and f_lr(m+)
      gl_cf* th = per_step(cst->dth);
      float fr[2][8];
      BF_UNROLL for (int c = 0; c < 2; ++c) BF_UNROLL for (int e = 0; e < 8; ++e) fr[c][e] = 0.f;
      if (lr < nr) {
        if constexpr (DYN == 1) {   // models.hpp: DYN_LORENZ96 (gaussfiltax/nonlinearities.py:37-50)
          const float alpha = th[0], beta = th[1], gamma = th[2], dt = th[3];
          const bool mp = th[4] != 0.f;
          const int im1 = (lr + nr - 1) % nr, ip1 = (lr + 1) % nr, im2 = (lr + 2 * nr - 2) % nr;
          const float xi = sm2[lr], ax = sm2[im1];
          const float bx = mp ? (sm2[ip1] - sm2[im2]) : 0.f;
          fval = xi + dt * (alpha * (ax * bx) - beta * xi + gamma);
          BF_UNROLL for (int c = 0; c < 2; ++c) BF_UNROLL for (int e = 0; e < 8; ++e) {
            const int j = 16 * c + 8 * lk + e;
            float v = 0.f;
            if (j == lr) v += 1.0f - dt * beta;
            if (mp) {
              if (j == im1) v += dt * alpha * bx;
              if (j == ip1) v += dt * alpha * ax;
              if (j == im2) v -= dt * alpha * ax;
            }
            fr[c][e] = v;
          }
        } else {                    // models.hpp: DYN_SINE
          const float w0 = th[0], xi = sm2[lr];
          fval = sinf(w0 * xi);
          const float d = w0 * cosf(w0 * xi);
          BF_UNROLL for (int c = 0; c < 2; ++c) BF_UNROLL for (int e = 0; e < 8; ++e) fr[c][e] = (16 * c + 8 * lk + e == lr) ? d : 0.f;
        }
      }
      BF_UNROLL for (int c = 0; c < 2; ++c) BF_UNROLL for (int d = 0; d < 4; ++d) {
        const Split3 sp = split_pair(fr[c][2 * d], fr[c][2 * d + 1]);
        aop[0][c][d] = sp.hi; aop[1][c][d] = sp.mid; aop[2][c][d] = sp.lo;
      }
    }
    // ---- Y^T = P+^T A^T; m- = A m+ + G q0 (DYN: f(m+) + F_q q0)
    {
      f32x16 acc = {0};
      BF_UNROLL for (int c = 0; c < 2; ++c) {
        u32x4 a[3];
        load_terms(a, Pn, TERM, PITCH, lr, c, lk);
        const u32x4 ba[3] = {aop[0][c], aop[1][c], aop[2][c]};
        acc = mfma_bf6(a, ba, acc);
      }
      store_terms_transposed(Yn, TERM, PITCH, 0, 0, lane, acc);
      if constexpr (DYN == 0) {
        float s = dot_terms32(aop, sm2, lk);
        s += __shfl_xor(s, 32, 64);
        sm[lr] = s + gq0;
      } else {
        sm[lr] = fval + gq0;
      }
    }
    wave_lds_order();
    // ---- P- = Y A^T + G Q G^T; predicted streams
    {
      float gq[16];
      BF_UNROLL for (int r = 0; r < 16; ++r) gq[r] = gqg_t[c_row(r, lane) * 32 + lr];
      BF_UNROLL for (int r = 0; r < 16; ++r) Pacc[r] = 0.f;
      BF_UNROLL for (int c = 0; c < 2; ++c) {
        u32x4 a[3];
        load_terms(a, Yn, TERM, PITCH, lr, c, lk);
        const u32x4 ba[3] = {aop[0][c], aop[1][c], aop[2][c]};
        Pacc = mfma_bf6(a, ba, Pacc);
      }
      BF_UNROLL for (int r = 0; r < 16; ++r) Pacc[r] += gq[r];
      store_tile32(out.pP, bt, t, lane, Pacc, nr, kc);
      store_terms_transposed(Pn, TERM, PITCH, 0, 0, lane, Pacc);
      if (out.pm.p && lane < nr) out.pm.p[bt * out.pm.sB + kc * out.pm.sK + t * out.pm.sT + lane * out.pm.sE] = sm[lane];
    }
    wave_lds_order();
  }

  // MISSING: the carry's sixteen rows are formed here, from a lane the compiler cannot match with the prologue's -- the plain
  // instances carry them through the time loop and spill twelve of them around it (mfma_tiles.hpp: per_step)
  const int lane_out = MISSING ? lane + opaque_zero() : lane;
  if (carry.P_out && lr < nr) BF_UNROLL for (int r = 0; r < 16; ++r) {
      const int row = c_row(r, lane_out);
      if (row < nr) carry.P_out[b * nr * nr + row * nr + lr] = Pacc[r];
    }
  if (carry.m_out && lane < nr) carry.m_out[b * nr + lane] = sm[lane];
  if (!MULTI && carry.w_out && lane == 0) carry.w_out[b] = w;
}

// The eight instances of one MISSING value, chosen at run time; each translation unit instantiates its own eight through this
// (kf_scan_bf32.hip: bf32_launch_plain, kf_scan_bf32_missing.hip: bf32_launch_missing).  `chains`: two per 128-thread workgroup.
struct Bf32Args {
  const Bf32Const* dc;
  CView y;
  CarryView carry;
  OutViews out;
  long long chains, T;
  int nr, mr, K;
  const float *tvq, *tvr;
};
template <bool MISSING>
hipError_t bf32_launch_instance(const Bf32Args& a, bool multi, int dyn_kind, hipStream_t stream) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.chains + 1) / 2)), dim3(128), 2 * BF32_WAVE_LDS, stream, a.dc, a.y, a.carry, a.out, a.chains,
                       a.T, a.nr, a.mr, a.K, a.tvq, a.tvr);
    return hipGetLastError();
  };
  const bool tv = a.tvq || a.tvr;
  if (multi && dyn_kind == 1) return tv ? go(kf_scan_bf32_kernel<true, true, 1, MISSING>) : go(kf_scan_bf32_kernel<true, false, 1, MISSING>);
  if (multi && dyn_kind == 2) return tv ? go(kf_scan_bf32_kernel<true, true, 2, MISSING>) : go(kf_scan_bf32_kernel<true, false, 2, MISSING>);
  if (multi) return tv ? go(kf_scan_bf32_kernel<true, true, 0, MISSING>) : go(kf_scan_bf32_kernel<true, false, 0, MISSING>);
  return tv ? go(kf_scan_bf32_kernel<false, true, 0, MISSING>) : go(kf_scan_bf32_kernel<false, false, 0, MISSING>);
}
hipError_t bf32_launch_plain(const Bf32Args& a, bool multi, int dyn_kind, hipStream_t stream);     // kf_scan_bf32.hip
hipError_t bf32_launch_missing(const Bf32Args& a, bool multi, int dyn_kind, hipStream_t stream);   // kf_scan_bf32_missing.hip

}  // namespace bf
