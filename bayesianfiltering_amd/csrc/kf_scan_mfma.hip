// kf_scan_mfma: batched Kalman filter for 33 <= n <= 64, m <= 32 on the matrix cores, four waves per chain.
//
// The recursion is the lax.scan body of gaussian_sum_filter (gaussfiltax/inference.py:333-371) for one component:
// _condition_on (:72-105), reweight (:347-350), _predict (:51-70).  At state_dim 64 one step is ~2 MFLOP of dense 64x64 /
// 32x64 products (60-120 flop per output byte, above the fp32 ridge).  One workgroup of 4 waves per
// chain; wave w owns the 32x32 output tile (ti, tj) = (w >> 1, w & 1) of every 64x64 product.
//
// The five matrix products stay off the fp32 datapath.  On gfx950 v_mfma_f32_32x32x2_f32 and the fp32 vector
// instructions share ONE datapath per SIMD (profiles/r02_f32_pipe_probe.txt), so fp32 products (13.3 us of the
// 20.4 us of SIMD-time a step needs) cannot hide behind the factorization.  v_mfma_f32_32x32x16_bf16 runs at 16x the
// rate; with every operand written as the EXACT sum of three bf16 terms (x = hi + mid + lo: 8 + 8 + 8 significand bits)
// and the six cross terms of weight >= 2^-16 accumulated in fp32, a product costs 6/16 of the fp32 MFMA time at the same
// rounding (scripts/probes/bf16x3_check.hip: 9.3e-8 of sum |terms| against 1.1e-7 for the fp32 MFMA).
//
// Layouts.  The bf16 MFMA wants 8 consecutive k per lane for both operands: A-operand X[m][k] row-major, B-operand as
// Yt[n][k] = Y[k][n].  An accumulator tile holds, per lane, one column and four groups of four consecutive rows, so its
// cheap store is the TRANSPOSED one, T[col][row] (8-byte stores of 4 terms): stored that way a result Z serves as the
// A-operand of Z^T . and as the B-operand of . Z.  The products are arranged so that nothing else is ever needed:
//   A   Z = (H P-)^T = P-^T H^T        A-op: P- as stored (J), B-op: H (registers)          -> Z stored; H P also fp32
//   B   S^T = H Z                       A-op: H (registers),    B-op: Z as stored
//   C   the two factorizations (mfma_tiles.hpp: the gain is never formed); W^T written as bf16 terms row-major (each lane
//       owns a column of W)
//   H   P+ = P- - W^T W + c c^T         A-op: -W^T, B-op: W^T (the same array); P- from the accumulators of J
//   I   Y^T = (A P+)^T = P+^T A^T       A-op: P+ as stored (H), B-op: A rows (registers)    -> Y^T stored
//   J   P- = Y A^T + G Q G^T            A-op: Y^T as stored (I) = Y row-major, B-op: A rows (registers)
// A and H live in registers as bf16 terms (2 x 48 VGPRs per wave); the matrix-vector products rebuild their fp32
// values from the terms (hi + mid + lo is exact).  LDS: 72.8 KB per workgroup, two workgroups per CU.
// The m x m system is solved through a Cholesky factor instead of the reference's LU with partial pivoting
// (utils.py:256-259): S + 1e-6 is symmetric positive definite, the solution is the same linear system's, and the two
// factorizations agree to ~1e-6 relative for the conditioned S of a filter (the parity budget is 1e-5); the log-likelihood
// uses the Cholesky factor of the un-jittered S exactly like the reference (inference.py:104, :24).
// The kernels this one superseded, and what was measured on them: DESIGN.md, "Retired matrix-core variants".
#include <cstdlib>
#include "forward_host.hpp"
#include "lgssm_pack.hpp"
#include "mfma_multi.hpp"
#include "mfma_tiles.hpp"

namespace bf {

template <int N, int M>
struct MfmaConst {  // device-resident (too large for kernel arguments)
  // 24 KB of zeros where the retired fp32-MFMA kernels had their copies of A and H.  Taking them out moves every other
  // member's offset, and the compiler answers with another register allocation in all eight instances (the benchmarked one:
  // 3 730 -> 3 732 instructions, 112 -> 91 spilled SGPRs): a change to the kernel's code, to be made and measured on its own
  float reserved[N * N + M * N];
  float GQG[N * N], DRD[M * M], Gq0[N], Dr0[M];
  float dth[8];   // DYN != 0: the registry dynamics' scalars
  unsigned short A3[3][N * N], H3[3][M * N];  // A = A3[0] + A3[1] + A3[2] exactly, three bf16 terms (row-major)
};

// the factorizing waves' two chains, out of line (a register allocation of their own): wave 3's chol(S + 1e-6) with W, c, m+
// and wave 2's chol(S) with the log-likelihood.  `used` keeps the second an ordinary function of its arguments: left internal
// with this one kind of caller, the compiler specialises it on the caller's LDS addresses -- the dynamic-LDS base from a table
// plus an address add per ds_read2, whose immediate offsets no longer reach: 1 251 instructions for 1 223, and 32 more
// bytes of scratch per lane in the <false, true, 0> kernel instance.
__device__ __attribute__((noinline)) void chol_w_rows_bf(lds_f* sc, lds_f* sT, lds_f* sv, lds_f* mcur, lds_f* mnxt, lds_f* scv, lds_c* wt,
                                                         int lane) {
  chol_w_rows_impl<64>(sc, sT, sv, mcur, mnxt, scv, wt, lane);
}
__device__ __attribute__((noinline, used)) float chol_loglik_rows(lds_f* sc, lds_f* sv, int lane) { return chol_loglik_rows_impl(sc, sv, lane); }

// one 32x32 accumulator tile (pi, pj) of a [N][N] stream entry at (b, t)
template <int N>
__device__ __forceinline__ void store_tile(const SView& sv, long long b, long long t, int pi, int pj, int lane, const f32x16& acc, int k = 0) {
  if (!sv.p) return;
  const int lr = lane & 31, lk = lane >> 5;
  gl_f* base = per_step(sv.p + b * sv.sB + k * sv.sK + t * sv.sT);
  const unsigned e0 = (unsigned)((32 * pi + 4 * lk) * N + 32 * pj + lr);
  if (sv.sE == 1) {
    BF_UNROLL for (int r = 0; r < 16; ++r) __builtin_nontemporal_store(acc[r], base + (e0 + ((r & 3) + 8 * (r >> 2)) * N));
  } else {
    const long long sE = sv.sE + (long long)opaque_szero();  // the sixteen 64-bit products below are per-step work too, not pre-loop registers
    const unsigned e0s = e0 + (unsigned)opaque_zero();
    BF_UNROLL for (int r = 0; r < 16; ++r) __builtin_nontemporal_store(acc[r], base + (long long)(e0s + ((r & 3) + 8 * (r >> 2)) * N) * sE);
  }
}
// store_tile for a model of nr <= N states riding zero-padded in the N x N tiles: entries (row, col) with both < nr, at the
// model's own row length
template <int N>
__device__ __forceinline__ void store_tile_n(const SView& sv, long long b, long long t, int pi, int pj, int lane, const f32x16& acc, int nr, int k = 0) {
  if (nr == N) return store_tile<N>(sv, b, t, pi, pj, lane, acc, k);
  if (!sv.p) return;
  const int lr = lane & 31, lk = lane >> 5;
  gl_f* base = per_step(sv.p + b * sv.sB + k * sv.sK + t * sv.sT);
  const int col = 32 * pj + lr;
  const long long sE = sv.sE + (long long)opaque_szero();
  BF_UNROLL for (int r = 0; r < 16; ++r) {
    const int row = 32 * pi + (r & 3) + 8 * (r >> 2) + 4 * lk;
    if (col < nr && row < nr) __builtin_nontemporal_store(acc[r], base + (long long)(row * nr + col) * sE);
  }
}

// sum_k X[row][k] v[k] over half of the k range (chunks 2 h, 2 h + 1; the lane's k are 16 c + 8 lk + 0..7) from the register
// terms of X
__device__ __forceinline__ float dot_terms_half(const u32x4 (*x)[4], const float* v, int lk, int h) {
  float s = 0.f;
  BF_UNROLL for (int cc = 0; cc < 2; ++cc) BF_UNROLL for (int d = 0; d < 4; ++d) {
    const u32x4 x0v = h ? x[0][2 + cc] : x[0][cc], x1v = h ? x[1][2 + cc] : x[1][cc], x2v = h ? x[2][2 + cc] : x[2][cc];
    const float x0 = (bf_lo(x0v[d]) + bf_lo(x1v[d])) + bf_lo(x2v[d]);
    const float x1 = (bf_hi(x0v[d]) + bf_hi(x1v[d])) + bf_hi(x2v[d]);
    const int k = 16 * (2 * h + cc) + 8 * lk + 2 * d;
    s = fmaf(x0, v[k], s);
    s = fmaf(x1, v[k + 1], s);
  }
  return s;
}

// MULTI: the K Gaussian-sum components of a LINEAR model as independent chains (see kf_scan_bf32_kernel): workgroup c =
// trajectory * K + component reads trajectory c / K's observations and writes component c % K's streams and per-step
// log-likelihood; the weights follow in gsf_reweight_kernel.  TV: per-step G Q_t G^T / D R_t D^T tables (64 x 64 and 32 x 32
// floats per step) instead of the constants -- inference.py:21,337-353.
// DYN: 0 = linear; 1 = Lorenz-96, 2 = sine dynamics as extended Kalman chains (see kf_scan_bf32_kernel): the wave's rows of
// F = df/dx at the filtered mean are re-evaluated and re-split into the A operand registers every step.
template <int N, int M, bool MULTI = false, bool TV = false, int DYN = 0>
__global__ void __launch_bounds__(256, 2)
kf_scan_mfma5_kernel(const MfmaConst<N, M>* __restrict__ cst, CView y, CarryView carry, OutViews out, long long B, long long T,
                     int rot_mode, int nr, int mr, int K, const float* __restrict__ tvq, const float* __restrict__ tvr) {
  // nr <= 64, mr <= 32: the model's own dimensions (streams and carry are laid out for them); inside, everything is (64, 32)
  static_assert(N == 64 && M == 32, "tile assignment is written for n = 64, m = 32");
  constexpr int PS = M + 1, HPP = N + 1;
  constexpr int PITCH = 144, PN_TERM = 64 * PITCH, ZN_TERM = 32 * PITCH, WT_PITCH = 80, WT_TERM = 64 * WT_PITCH;
  constexpr int OFF_ZN = 3 * PN_TERM, OFF_WT = OFF_ZN + 3 * ZN_TERM, OFF_YN = OFF_ZN, OFF_F32 = OFF_WT + 3 * WT_TERM;
  static_assert(3 * PN_TERM <= 3 * ZN_TERM + 3 * WT_TERM, "Y^T aliases Z and W^T");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int lr = lane & 31, lk = lane >> 5;
  __shared__ int s_rot;
  if (tid == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    const unsigned k = (hw >> 4) & 3, pos = ((k & 1) << 1) | (k >> 1);
    s_rot = rot_mode == 0 ? (int)blockIdx.x : (int)(pos + 2 * (hw & 15));
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(((tid >> 6) + s_rot) & 3);
  const int ti = wave >> 1, tj = wave & 1;
  const long long b = blockIdx.x;                  // chain: carry index
  const long long bt = MULTI ? b / K : b;          // trajectory: observations, stream batch index
  const int kc = MULTI ? (int)(b % K) : 0;         // component: stream component index

  extern __shared__ __attribute__((aligned(16))) float lds[];
  lds_c* L = (lds_c*)reinterpret_cast<char*>(lds);
  lds_c* Pn = L;             // [3][64][144 B]  P- (after J) / P+ (after H), transposed terms
  lds_c* Zn = L + OFF_ZN;    // [3][32][144 B]  Z = (H P-)^T
  lds_c* Wt = L + OFF_WT;    // [3][64][80 B]   W^T, row-major terms
  lds_c* Yn = L + OFF_YN;    // [3][64][144 B]  Y^T (aliases Zn, Wt)
  float* sHP = lds + OFF_F32 / 4;   // [32][65]  H P- in fp32 for the forward substitution
  float* sc2 = sHP + M * HPP;       // [32][33]  S as wave 2 sees it
  float* sc3 = sc2 + M * PS;        // [32][33]  S as wave 3 sees it
  float* sm = sc3 + M * PS;         // [64] mean
  float* sm2 = sm + N;              // [64] mean (ping-pong)
  float* sv = sm2 + N;              // [32] innovation
  float* scv = sv + M;              // [64] 1e-3 W^T g
  float* part = scv + N;            // [2][64] halves (over k) of the two matrix-vector products
  float* sv3 = part + 2 * N;        // [32] innovation, wave 3's copy

  // A rows 32 tj + lr and H row lr as bf16 terms: the wave's B-operand in phases A, I, J and A-operand in phase B
  u32x4 hop[3][4], aop[3][4];
  BF_UNROLL for (int t = 0; t < 3; ++t) BF_UNROLL for (int c = 0; c < 4; ++c) {
    hop[t][c] = *reinterpret_cast<const u32x4*>(&cst->H3[t][lr * N + 16 * c + 8 * lk]);
    if constexpr (DYN == 0) aop[t][c] = *reinterpret_cast<const u32x4*>(&cst->A3[t][(32 * tj + lr) * N + 16 * c + 8 * lk]);
  }
  f32x16 Pacc;  // the wave's tile of P-: carried in registers from phase J to phase H
  const bool col_ok = 32 * tj + lr < nr;
  BF_UNROLL for (int r = 0; r < 16; ++r) {
    const int row = 32 * ti + c_row(r, lane);
    Pacc[r] = (col_ok && row < nr) ? carry.P_in[b * nr * nr + row * nr + 32 * tj + lr] : 0.f;
  }
  store_terms_transposed(Pn, PN_TERM, PITCH, ti, tj, lane, Pacc);
  if (tid < N) sm[tid] = tid < nr ? carry.m_in[b * nr + tid] : 0.f;
  float w = (!MULTI && carry.w_in) ? carry.w_in[b] : 1.0f;
  float ynext = (wave >= 2 && lane < mr) ? y.p[bt * y.sB + lane * y.sE] : 0.f;
  const float ll_pad = 0.5f * 1.8378770664093453f * (float)(M - mr);   // the padded observations' log N(0; 0, 1), taken off
  const float dr0 = cst->Dr0[lr], gq0 = cst->Gq0[lane];
  __syncthreads();

#ifdef BF_MFMA_PHASE_TIMERS
  long long tacc[12] = {0};
  long long tprev = wall_clock64();
#define BF_TICK5(i) { const long long tn_ = wall_clock64(); tacc[i] += tn_ - tprev; tprev = tn_; }
#else
#define BF_TICK5(i)
#endif
  float* mcur = sm;
  float* mnxt = sm2;
  for (long long t = 0; t < T; ++t) {
    float yv_t = ynext;                      // this step's observation (waves 2, 3), the same for every component
    if (wave >= 2) {
      const long long tn = t + 1 < T ? t + 1 : t;
      if (lane < mr) ynext = y.p[bt * y.sB + tn * y.sT + lane * y.sE];  // prefetch
    }
    gl_cf* const drd_t = TV && tvr ? per_step(tvr + t * (M * M)) : per_step(cst->DRD);
    gl_cf* const gqg_t = TV && tvq ? per_step(tvq + t * (N * N)) : per_step(cst->GQG);
    // ================= phase A: Z = P-^T H^T (waves 0, 1: row tile = wave); innovation (wave 2)
    if (wave < 2) {
      f32x16 z = {0};
      BF_UNROLL for (int c = 0; c < 4; ++c) {
        u32x4 a[3];
        load_terms(a, Pn, PN_TERM, PITCH, 32 * wave + lr, c, lk);
        const u32x4 bh[3] = {hop[0][c], hop[1][c], hop[2][c]};
        z = mfma_bf6(a, bh, z);
      }
      BF_UNROLL for (int r = 0; r < 16; ++r) sHP[lr * HPP + 32 * wave + c_row(r, lane)] = z[r];   // (H P-)[lr][.]
      store_terms_transposed(Zn, ZN_TERM, PITCH, wave, 0, lane, z);
    } else {
      // H m-: waves 2 and 3 (idle in this phase) take half of the k range each; the halves meet after the barrier
      float s = dot_terms_half(hop, mcur, lk, wave - 2);
      s += __shfl_xor(s, 32, 64);
      if (lane < M) part[(wave - 2) * N + lane] = s;
    }
    BF_TICK5(0)
    lds_barrier();
    BF_TICK5(1)
    // ================= phases B + C (waves 2 and 3): S^T = H Z + (D R D^T)^T, the factorizations, W^T, c, m+
    float ll = 0.f;
    if (wave >= 2) {
      {  // innovation v = y - (H m- + D r0): both factorizing waves form it (same bits) for their own use
        if (lane < M) (wave == 2 ? sv : sv3)[lane] = yv_t - ((part[lane] + part[N + lane]) + dr0);
      }
      f32x16 acc;
      BF_UNROLL for (int r = 0; r < 16; ++r) acc[r] = drd_t[lr * M + c_row(r, lane)];
      BF_UNROLL for (int c = 0; c < 4; ++c) {
        u32x4 bz[3];
        load_terms(bz, Zn, ZN_TERM, PITCH, lr, c, lk);
        const u32x4 ah[3] = {hop[0][c], hop[1][c], hop[2][c]};
        acc = mfma_bf6(ah, bz, acc);
      }
      float* sc = wave == 2 ? sc2 : sc3;
      BF_UNROLL for (int r = 0; r < 16; ++r) sc[lr * PS + c_row(r, lane)] = acc[r];   // S[lr][.] = S^T[.][lr]
      wave_lds_order();
      BF_TICK5(10)
      if (wave == 3) chol_w_rows_bf((lds_f*)sc3, (lds_f*)sHP, (lds_f*)sv3, (lds_f*)mcur, (lds_f*)mnxt, (lds_f*)scv, Wt, lane);
      else ll = chol_loglik_rows((lds_f*)sc2, (lds_f*)sv, lane) + ll_pad;
    }
    BF_TICK5(2)
    lds_barrier();
    BF_TICK5(3)
    // ================= phase H: P+ = P- - W^T W + c c^T (K = 32 + 2); emit filtered streams; P+ stored as terms
    {
      f32x16 acc = Pacc;
      BF_UNROLL for (int c = 0; c < 2; ++c) {
        u32x4 a[3], bw[3];
        load_terms(a, Wt, WT_TERM, WT_PITCH, 32 * ti + lr, c, lk);
        load_terms(bw, Wt, WT_TERM, WT_PITCH, 32 * tj + lr, c, lk);
        BF_UNROLL for (int q = 0; q < 3; ++q) a[q] ^= 0x80008000u;   // -W^T
        acc = mfma_bf6(a, bw, acc);
      }
      acc = mfma2(lk == 0 ? scv[32 * ti + lr] : 0.f, lk == 0 ? scv[32 * tj + lr] : 0.f, acc);
      store_tile_n<N>(out.P, bt, t, ti, tj, lane, acc, nr, kc);
      store_terms_transposed(Pn, PN_TERM, PITCH, ti, tj, lane, acc);
    }
    if (wave == 1 && out.m.p && lane < nr) out.m.p[bt * out.m.sB + kc * out.m.sK + t * out.m.sT + lane * out.m.sE] = mnxt[lane];
    if (wave == 2 && lane == 0) {
      if constexpr (!MULTI) {
        w = reweight_single(ll, w);
        if (out.w.p) out.w.p[b * out.w.sB + t * out.w.sT] = w;
      }
      if (out.ll.p) out.ll.p[bt * out.ll.sB + kc * out.ll.sK + t * out.ll.sT] = ll;   // (MULTI: the launcher always provides it)
    }
    BF_TICK5(4)
    lds_barrier();
    BF_TICK5(5)
    // ================= phase I: Y^T = P+^T A^T (K = 64); m- = A m+ + G q0 (waves 0, 1: rows 32 tj + lr)
    // Fetched here, a phase ahead of its use: the tile of G Q G^T (added after phase J's products) -- an L2 round trip under
    // this load is ~1 us
    float gq[16];
    BF_UNROLL for (int r = 0; r < 16; ++r) gq[r] = gqg_t[(32 * ti + c_row(r, lane)) * N + 32 * tj + lr];
    if constexpr (DYN != 0) {   // row 32 tj + lr of F at the filtered mean (mnxt), columns 16 c + 8 lk + e; f of that row
      gl_cf* th = per_step(cst->dth);
      const int row = 32 * tj + lr;
      float fv = 0.f;
      BF_UNROLL for (int c = 0; c < 4; ++c) {
        float fr[8];
        BF_UNROLL for (int e = 0; e < 8; ++e) fr[e] = 0.f;
        if (row < nr) {
          if constexpr (DYN == 1) {
            const float alpha = th[0], beta = th[1], gamma = th[2], dt = th[3];
            const bool mp = th[4] != 0.f;
            const int im1 = (row + nr - 1) % nr, ip1 = (row + 1) % nr, im2 = (row + 2 * nr - 2) % nr;
            const float xi = mnxt[row], ax = mnxt[im1];
            const float bx = mp ? (mnxt[ip1] - mnxt[im2]) : 0.f;
            fv = xi + dt * (alpha * (ax * bx) - beta * xi + gamma);
            BF_UNROLL for (int e = 0; e < 8; ++e) {
              const int j = 16 * c + 8 * lk + e;
              float v = 0.f;
              if (j == row) v += 1.0f - dt * beta;
              if (mp) {
                if (j == im1) v += dt * alpha * bx;
                if (j == ip1) v += dt * alpha * ax;
                if (j == im2) v -= dt * alpha * ax;
              }
              fr[e] = v;
            }
          } else {
            const float w0 = th[0], xi = mnxt[row];
            fv = sinf(w0 * xi);
            const float d = w0 * cosf(w0 * xi);
            BF_UNROLL for (int e = 0; e < 8; ++e) fr[e] = (16 * c + 8 * lk + e == row) ? d : 0.f;
          }
        }
        BF_UNROLL for (int d = 0; d < 4; ++d) {
          const Split3 sp = split_pair(fr[2 * d], fr[2 * d + 1]);
          aop[0][c][d] = sp.hi; aop[1][c][d] = sp.mid; aop[2][c][d] = sp.lo;
        }
      }
      if (ti == 0 && lane < 32) { part[32 * tj + lane] = fv; part[N + 32 * tj + lane] = 0.f; }   // (read back as part[.] + part[N + .])
    }
    {
      f32x16 acc = {0};
      BF_UNROLL for (int c = 0; c < 4; ++c) {
        u32x4 a[3];
        load_terms(a, Pn, PN_TERM, PITCH, 32 * ti + lr, c, lk);
        const u32x4 ba[3] = {aop[0][c], aop[1][c], aop[2][c]};
        acc = mfma_bf6(a, ba, acc);
      }
      store_terms_transposed(Yn, PN_TERM, PITCH, ti, tj, lane, acc);
    }
    if constexpr (DYN == 0) {  // A m+: the two waves holding rows 32 tj + lr take half of the k range each
      float s = dot_terms_half(aop, mnxt, lk, ti);
      s += __shfl_xor(s, 32, 64);
      if (lane < 32) part[ti * N + 32 * tj + lane] = s;
    }
    BF_TICK5(6)
    lds_barrier();
    BF_TICK5(7)
    // ================= phase J: P- = Y A^T + G Q G^T (K = 64); emit predicted streams; P- stored as terms
    {
      if (wave == 2) mcur[lane] = (part[lane] + part[N + lane]) + gq0;   // predicted mean m- = A m+ + G q0
      BF_UNROLL for (int r = 0; r < 16; ++r) Pacc[r] = 0.f;
      BF_UNROLL for (int c = 0; c < 4; ++c) {
        u32x4 a[3];
        load_terms(a, Yn, PN_TERM, PITCH, 32 * ti + lr, c, lk);
        const u32x4 ba[3] = {aop[0][c], aop[1][c], aop[2][c]};
        Pacc = mfma_bf6(a, ba, Pacc);
      }
      BF_UNROLL for (int r = 0; r < 16; ++r) Pacc[r] += gq[r];
      store_tile_n<N>(out.pP, bt, t, ti, tj, lane, Pacc, nr, kc);
      store_terms_transposed(Pn, PN_TERM, PITCH, ti, tj, lane, Pacc);
    }
    if (wave == 2 && out.pm.p && lane < nr) out.pm.p[bt * out.pm.sB + kc * out.pm.sK + t * out.pm.sT + lane * out.pm.sE] = (part[lane] + part[N + lane]) + gq0;
    BF_TICK5(8)
    lds_barrier();
    BF_TICK5(9)
  }

  if (carry.P_out && col_ok) BF_UNROLL for (int r = 0; r < 16; ++r) {
      const int row = 32 * ti + c_row(r, lane);
      if (row < nr) carry.P_out[b * nr * nr + row * nr + 32 * tj + lr] = Pacc[r];
    }
  if (carry.m_out && tid < nr) carry.m_out[b * nr + tid] = mcur[tid];
  if (!MULTI && carry.w_out && wave == 2 && lane == 0) carry.w_out[b] = w;
#ifdef BF_MFMA_PHASE_TIMERS
  __syncthreads();
  if (b == 0 && lane == 0 && carry.P_out) for (int i = 0; i < 12; ++i) carry.P_out[wave * 16 + i] = (float)tacc[i];
#endif
}

// ---------------------------------------------------------------------------------------
// K = 1, multi = false: bf_kalman_filter_f32; multi: the Gaussian-sum filter of a linear model (bf_gsf_ekf_f32), components in turn.
// dyn_kind: 0 = linear (p->A), 1 = Lorenz-96, 2 = sine with scalars dth (identity noise input: p->G == NULL, dq == n); nonlinear
// chains always run as `multi` (K >= 1).
int launch_kf_mfma(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry,
                   const bf_out_desc* out, hipStream_t stream, int K, bool multi, int dyn_kind, const float* dth) {
  constexpr int N = 64, M = 32;
  // Smaller models ride in the (64, 32) tiles zero-padded: A, H, G Q G^T padded with zeros keep the padded block of P at
  // exactly zero; the padded observations are y = 0 with unit noise and H rows of zero, independent of the real ones up to
  // the 1e-6 jitter's O(1e-12) coupling; each contributes log N(0; 0, 1) to the log-likelihood, taken off again in the kernel.
  const int nr = p->n, mr = p->m, dq = p->dq, dr = p->dr;
  if (nr > N || mr > M) return set_error(BF_EUNSUPPORTED, "MFMA Kalman kernel: n <= 64 and m <= 32");
  if (dyn_kind != 0 && (!multi || p->G || dq != nr)) return set_error(BF_EINVAL, "nonlinear chains: identity noise input, multi launch");
  if (K > 64) return set_error(BF_EUNSUPPORTED, "MFMA Kalman kernel: at most 64 components (one per lane in the weight update)");
  if ((p->Q_steps > 1 && p->Q_steps != T) || (p->R_steps > 1 && p->R_steps != T))
    return set_error(BF_EINVAL, "time-varying covariances need one matrix per step (Q_steps / R_steps = T = %lld)", T);
  MfmaConst<N, M>* h = new MfmaConst<N, M>();  // zero-filled: the constant cache compares contents
  for (int i = 0; i < 8; ++i) h->dth[i] = (dyn_kind != 0 && dth) ? dth[i] : 0.f;
  if (dyn_kind == 0) split_bf16x3(p->A, nr, nr, nr, h->A3, N);
  split_bf16x3(p->H, mr, nr, nr, h->H3, N);
  noise_cov(p->G, p->Q, nr, dq, h->GQG, N);
  noise_cov(p->D, p->R, mr, dr, h->DRD, M);
  for (int i = mr; i < M; ++i) h->DRD[i * M + i] = 1.0f;   // padded observations: unit noise
  noise_mean(p->G, p->q0, nr, dq, h->Gq0);
  noise_mean(p->D, p->r0, mr, dr, h->Dr0);
  const void* dv = nullptr;
  const int crc = device_constants(h, sizeof(*h), stream, &dv);
  delete h;
  if (crc != BF_OK) return crc;
  const MfmaConst<N, M>* d = static_cast<const MfmaConst<N, M>*>(dv);

  auto [yv, cv, ov] = forward_views(y, carry, out);
  // per-step tables (_get_params(x, 2, t), inference.py:21), formed on the device; MULTI: somewhere for the log-likelihoods
  float *d_tvq = nullptr, *d_tvr = nullptr, *llscratch = nullptr;
  auto free_tables = [&]() {
    if (d_tvq) (void)hipFreeAsync(d_tvq, stream);
    if (d_tvr) (void)hipFreeAsync(d_tvr, stream);
  };
  int rc = BF_OK;
  if (p->Q_steps > 1) rc = tv_table_on_device(p->G, p->Q, T, nr, dq, N, N, stream, &d_tvq);
  if (rc == BF_OK && p->R_steps > 1) rc = tv_table_on_device(p->D, p->R, T, mr, dr, M, mr, stream, &d_tvr);
  if (rc == BF_OK && multi) rc = begin_multi(B, T, K, stream, ov, &llscratch);
  if (rc != BF_OK) { free_tables(); return rc; }

  static const int rot_mode = [] { const char* e = std::getenv("BAYESFILT_MFMA_ROT"); return e ? std::atoi(e) : 1; }();
  const size_t lds5 = 3 * 64 * 144 + 3 * 32 * 144 + 3 * 64 * 80 + sizeof(float) * (size_t)(M * (N + 1) + 2 * M * (M + 1) + 5 * N + 2 * M);
  const long long chains = multi ? B * K : B;
  auto go = [&](auto kern5) {
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(kern5), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds5);
    if (ae != hipSuccess) return ae;
    hipLaunchKernelGGL(kern5, dim3((unsigned)chains), dim3(256), lds5, stream, d, yv, cv, ov, chains, T, rot_mode, nr, mr, K, d_tvq, d_tvr);
    return hipGetLastError();
  };
  const bool tv = d_tvq || d_tvr;
  hipError_t le;
  if (multi && dyn_kind == 1) le = tv ? go(kf_scan_mfma5_kernel<N, M, true, true, 1>) : go(kf_scan_mfma5_kernel<N, M, true, false, 1>);
  else if (multi && dyn_kind == 2) le = tv ? go(kf_scan_mfma5_kernel<N, M, true, true, 2>) : go(kf_scan_mfma5_kernel<N, M, true, false, 2>);
  else if (multi) le = tv ? go(kf_scan_mfma5_kernel<N, M, true, true>) : go(kf_scan_mfma5_kernel<N, M, true, false>);
  else le = tv ? go(kf_scan_mfma5_kernel<N, M, false, true>) : go(kf_scan_mfma5_kernel<N, M, false, false>);
  free_tables();
  if (le != hipSuccess && llscratch) (void)hipFreeAsync(llscratch, stream);
  BF_HIP_CHECK(le);
  if (multi) return finish_multi(ov, carry, B, T, K, stream, llscratch);
  return BF_OK;
}

}  // namespace bf
