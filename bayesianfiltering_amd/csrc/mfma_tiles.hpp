// Device helpers of the two matrix-core Kalman kernels (kf_scan_mfma.hip: n <= 64, four waves per chain; kf_scan_bf32.hip:
// n <= 32, one wave per chain): the 32x32 accumulator-tile layout, three-term bf16 operands in LDS, the per-step laundering
// of loop-invariant addresses, and the in-register Cholesky factorizations of the 32 x 32 innovation covariance.
#pragma once
#include "bf_common.hpp"
#include "kf_math.hpp"
#include "lane_group.hpp"
#include "scan_common.hpp"

namespace bf {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using lds_f = __attribute__((address_space(3))) float;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
using lds_u32x2 = __attribute__((address_space(3))) u32x2;
using lds_u32x4 = __attribute__((address_space(3))) u32x4;
using lds_c = __attribute__((address_space(3))) char;
typedef __attribute__((address_space(1))) float gl_f;              // global memory: the laundered pointer must not decay to a flat one
typedef const __attribute__((address_space(1))) float gl_cf;

__device__ __forceinline__ f32x16 mfma2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of accumulator register r inside a 32x32 tile (C/D layout of the 32x32 MFMA shapes)
__device__ __forceinline__ int c_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ float rdlane_u(float v, int l) {  // v_readlane_b32: lane l's value as a wave-uniform scalar
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// A zero the compiler cannot see through, produced inside the time loop: LDS addresses formed from it
// are loop-variant, so they stay "register + immediate offset" operands instead of being hoisted out
// of the loop as hundreds of loop-invariant address registers (which then spill).
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}
__device__ __forceinline__ int opaque_szero() {  // the scalar-register sibling of opaque_zero(): addresses stay wave-uniform
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}

// Loop-invariant operands are NOT to be kept in registers across steps: the compiler hoists the 16 + 16 + 32 loads of
// G Q G^T, D R D^T and A and the sixteen 64-bit store addresses of every output stream out of the time loop, and then
// spills them (106 scratch stores ahead of the loop, ~90 reloads per step at three workgroups per CU).  A wave-uniform
// base laundered through an empty asm once per step keeps each access a (scalar base + lane offset + immediate) form.
__device__ __forceinline__ gl_f* per_step(float* p) { return (gl_f*)p + opaque_szero(); }
__device__ __forceinline__ gl_cf* per_step(const float* p) { return (gl_cf*)p + opaque_szero(); }

__device__ __forceinline__ void wave_lds_order() {  // order one wave's LDS traffic (the hardware runs it in issue order)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__device__ __forceinline__ float rsqrt_newton(float d) {
  // 1 / sqrt(d): v_rsq_f32 plus one Newton step (~1 ulp; the raw approximation alone costs the 1e-5
  // parity budget over 32 columns, the IEEE sqrt + division sequences are ~35 dependent instructions
  // per column on the serial path).  NaN for d < 0 (matrix not positive definite).
  const float y0 = __builtin_amdgcn_rsqf(d);
  const float e0 = fmaf(-(d * y0), y0, 1.0f);
  return fmaf(0.5f * y0, e0, y0);
}

// x0, x1 -> three packed pairs of bf16 (round to nearest even, v_cvt_pk_bf16_f32) with x = hi + mid + lo EXACTLY: the
// residual of a 24-bit significand after an 8-bit term has at most 16 bits, after two terms at most 8.
struct Split3 {
  unsigned hi, mid, lo;
};
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ float bf_lo(unsigned pk) { return __builtin_bit_cast(float, pk << 16); }
__device__ __forceinline__ float bf_hi(unsigned pk) { return __builtin_bit_cast(float, pk & 0xffff0000u); }
__device__ __forceinline__ Split3 split_pair(float x0, float x1) {
  Split3 o;
  o.hi = pk_bf16(x0, x1);
  const float r0 = x0 - bf_lo(o.hi), r1 = x1 - bf_hi(o.hi);
  o.mid = pk_bf16(r0, r1);
  const float q0 = r0 - bf_lo(o.mid), q1 = r1 - bf_hi(o.mid);
  o.lo = pk_bf16(q0, q1);
  return o;
}

// c += a b for operands given as three bf16 terms each (kf_scan_mfma.hip's header: why, and the operand layouts): the six
// cross terms of weight >= 2^-16 on v_mfma_f32_32x32x16_bf16, accumulated in fp32
__device__ __forceinline__ f32x16 mfma_bf6(const u32x4* a, const u32x4* b, f32x16 c) {  // smallest cross terms first
  auto m = [](u32x4 x, u32x4 y, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), acc, 0, 0, 0);
  };
  c = m(a[1], b[1], c);
  c = m(a[0], b[2], c);
  c = m(a[2], b[0], c);
  c = m(a[0], b[1], c);
  c = m(a[1], b[0], c);
  c = m(a[0], b[0], c);
  return c;
}
// accumulator tile (row tile rt, column tile ct) -> dst[term][32 ct + col][32 rt + row] as bf16 terms, `pitch` bytes per column
__device__ __forceinline__ void store_terms_transposed(lds_c* dst, int term_bytes, int pitch, int rt, int ct, int lane, const f32x16& acc) {
  const int lr = lane & 31, lk = lane >> 5;
  lds_c* base = dst + (32 * ct + lr) * pitch + (32 * rt + 4 * lk) * 2;
  BF_UNROLL for (int g = 0; g < 4; ++g) {  // rows 8 g + 4 lk + 0..3 of the tile
    const Split3 a = split_pair(acc[4 * g], acc[4 * g + 1]), b = split_pair(acc[4 * g + 2], acc[4 * g + 3]);
    *reinterpret_cast<lds_u32x2*>(base + 16 * g) = u32x2{a.hi, b.hi};
    *reinterpret_cast<lds_u32x2*>(base + term_bytes + 16 * g) = u32x2{a.mid, b.mid};
    *reinterpret_cast<lds_u32x2*>(base + 2 * term_bytes + 16 * g) = u32x2{a.lo, b.lo};
  }
}
__device__ __forceinline__ void load_terms(u32x4* dst, const lds_c* arr, int term_bytes, int pitch, int row, int chunk, int lk) {
  const lds_c* p = arr + row * pitch + (16 * chunk + 8 * lk) * 2;
  BF_UNROLL for (int t = 0; t < 3; ++t) dst[t] = *reinterpret_cast<const lds_u32x4*>(p + t * term_bytes);
}

#ifndef BF_MFMA_RDB
#define BF_MFMA_RDB 8  // broadcasts issued ahead of their consumers
#endif
// S (acc layout in `sc`, [32][33]) -> rows; chol(S + 1e-6); W = L^-1 (H P) with H P in `sT`; c -> scv, m+ -> mnxt.
// The gain is never formed.  With L L^T = S + 1e-6 (every entry: the psd_solve jitter J = 1e-6 1 1^T), W = L^-1 (H P),
// g = L^-1 1 and z = L^-1 v:
//     K S K^T = X^T (S_j - J) X = W^T W - 1e-6 (W^T g)(W^T g)^T          (X = S_j^-1 H P = L^-T W)
//     K v     = X^T v = W^T z
// -- the same quantities as P - K S K^T and m + K (y - h(m)) of inference.py:102-103, to rounding.  Lane r holds row r of
// S + 1e-6; by symmetry the multipliers L[k][j] of column j are lane j's own row entries, broadcast with v_readlane (no LDS
// round trip per column), and every lane carries a column of H P through the forward substitution in the same loop, fed by
// the same broadcasts.
// The function is VALU-issue bound (a wave64 instruction occupies the SIMD for 4 cycles; ~2 300 of them were the 3.8 us of
// this phase), so entry k of the lane's row of S and entry k of its column of H P travel as ONE register pair and every
// elimination step is one v_pk_fma_f32 on (a[k], w[k]) with the broadcast multiplier as its scalar operand -- the same
// fmas in the same order as the unpacked form, half the instructions.
// W^T leaves as three bf16 terms, wt[p][lane][k], 80-byte rows.
// NCOL = 64: every lane carries its own column of H P (pitch 65); NCOL = 32 (the one-wave kernel for n <= 32): the upper
// half-wave repeats the lower one's columns (pitch 33), its stores land on the same addresses with the same values.
// LL: also returns log N(v; 0, S) for the UN-jittered S, from this factorization of S_j = S + eps 1 1^T (eps = 1e-6) by
// the matrix determinant lemma and Sherman-Morrison: with g = L^-1 1, z = L^-1 v (both carried through the loop anyway)
//   det S = det S_j (1 - eps g^T g),   v^T S^-1 v = z^T z + eps (g^T z)^2 / (1 - eps g^T g)
// -- exact identities, evaluated in fp32 (eps g^T g is O(1e-4) for a conditioned S): the separate factorization of S that
// inference.py:104 implies (a second 1 200-instruction serial chain) is not needed.  Measured: on the one-wave kernel, where
// both chains would be serial, that gains 33 %; on the four-wave kernel it COSTS 7 % (4.23e7 against 4.56e7 steps/s on one
// box) -- the extra sums lengthen the critical wave's chain, the factorization they replace runs beside it on another wave
// (chol_loglik_rows_impl) -- so that kernel keeps LL = false.
template <int NCOL = 64, bool LL = false>
__device__ __forceinline__ float chol_w_rows_impl(lds_f* sc, lds_f* sT, lds_f* sv, lds_f* mcur, lds_f* mnxt, lds_f* scv,
                                                  lds_c* wt, int lane_in) {
  constexpr int PP = NCOL + 1, PS = 33, WT_TERM_B = NCOL * 80;
  const int r = lane_in & 31;
  const int lane = NCOL == 64 ? lane_in : r;
  f32x2 aw[32];  // .x: row r of S + 1e-6 (psd_solve's jitter on every entry, utils.py:258); .y: column `lane` of H P
  BF_UNROLL for (int k = 0; k < 32; ++k) aw[k] = f32x2{sc[r * PS + k] + 1e-6f, sT[k * PP + lane]};
  f32x2 rgz = f32x2{1.0f, sv[r]};  // residuals of g = L^-1 1, z = L^-1 v (row r)
  f32x2 acc_cm = f32x2{0.f, 0.f};  // (W^T g)[lane], (W^T z)[lane]
  float s_gg = 0.f, s_gz = 0.f, s_zz = 0.f, rprod = 1.f;   // LL: g^T g, g^T z, z^T z, prod 1 / L_jj (wave-uniform)
  Split3 wsp[4];
  static_for<0, 32>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const float rinv = rsqrt_newton(rdlane_u(aw[j].x, j));             // 1 / L[j][j], wave-uniform
    const f32x2 lw = aw[j] * rinv;                                     // L[r][j] (meaningful for r >= j), W[j][lane] (final)
    const f32x2 gz = f32x2{rdlane_u(rgz.x, j), rdlane_u(rgz.y, j)} * rinv;   // g[j], z[j]: wave-uniform
    aw[j] = lw;
    rgz = __builtin_elementwise_fma(f32x2{-lw.x, -lw.x}, gz, rgz);
    acc_cm = __builtin_elementwise_fma(f32x2{lw.y, lw.y}, gz, acc_cm);
    if constexpr (LL) {
      s_gg = fmaf(gz.x, gz.x, s_gg);
      s_gz = fmaf(gz.x, gz.y, s_gz);
      s_zz = fmaf(gz.y, gz.y, s_zz);
      rprod *= rinv;
    }
    const f32x2 ntq = -(lw * rinv);                                    // -a[r][j] / d_j, -w[j] / d_j
    // L[k][j] sqrt(d_j) = a[k][j] = a[j][k] by symmetry: lane j's own entries, read BEFORE this step updates them.
    // The broadcasts go out in batches of BF_MFMA_RDB ahead of the multiply-adds that consume them: a v_readlane's
    // scalar result takes several issue slots to become readable, and back-to-back (readlane, fma) pairs stall on it.
    static_for<0, (31 - j + BF_MFMA_RDB - 1) / BF_MFMA_RDB>([&](auto Cb) {
      constexpr int k0 = j + 1 + decltype(Cb)::value * BF_MFMA_RDB;
      constexpr int nk = (32 - k0) < BF_MFMA_RDB ? (32 - k0) : BF_MFMA_RDB;
      float sb[BF_MFMA_RDB];
      static_for<0, nk>([&](auto I) { sb[decltype(I)::value] = rdlane_u(aw[k0 + decltype(I)::value].x, j); });
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, nk>([&](auto I) {
        constexpr int k = k0 + decltype(I)::value;
        aw[k] = __builtin_elementwise_fma(ntq, f32x2{sb[decltype(I)::value], sb[decltype(I)::value]}, aw[k]);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    // rows j - 1, j of W are final; their bf16 terms are formed here, in the issue gaps of the dependent
    // chain (the loop runs at ~55 % of the issue rate), and go out eight rows per 16-byte store
    if constexpr (j & 1) {
      wsp[(j >> 1) & 3] = split_pair(aw[j - 1].y, aw[j].y);
      if constexpr ((j & 7) == 7) {
        constexpr int q = j >> 3;
        *reinterpret_cast<lds_u32x4*>(wt + 0 * WT_TERM_B + lane * 80 + q * 16) = u32x4{wsp[0].hi, wsp[1].hi, wsp[2].hi, wsp[3].hi};
        *reinterpret_cast<lds_u32x4*>(wt + 1 * WT_TERM_B + lane * 80 + q * 16) = u32x4{wsp[0].mid, wsp[1].mid, wsp[2].mid, wsp[3].mid};
        *reinterpret_cast<lds_u32x4*>(wt + 2 * WT_TERM_B + lane * 80 + q * 16) = u32x4{wsp[0].lo, wsp[1].lo, wsp[2].lo, wsp[3].lo};
      }
    }
  });
  scv[lane] = acc_cm.x * 1e-3f;                            // sqrt(1e-6) (W^T g): enters P+ as + c c^T
  mnxt[lane] = mcur[lane] + acc_cm.y;                      // filtered mean
  if constexpr (LL) {
    const float one_m = fmaf(-1e-6f, s_gg, 1.0f);                                   // 1 - eps g^T g
    const float quad = s_zz + (1e-6f * s_gz) * s_gz / one_m;
    return -0.5f * quad - 0.5f * 32.0f * 1.8378770664093453f + fast_log(rprod) - 0.5f * fast_log(one_m);
  } else {
    return 0.f;
  }
}

// chol(S) (no jitter), z = L^-1 v, log N(v; 0, S) -- inference.py:104, :24
// Packed like chol_w_rows_impl, here two neighbouring entries of the row per register pair and two broadcasts per scalar pair.
__device__ __forceinline__ float chol_loglik_rows_impl(lds_f* sc, lds_f* sv, int lane) {
  constexpr int PS = 33;
  const int r = lane & 31;
  f32x2 ap[16];  // (a[2 i], a[2 i + 1]) of row r
  BF_UNROLL for (int i = 0; i < 16; ++i) ap[i] = f32x2{sc[r * PS + 2 * i], sc[r * PS + 2 * i + 1]};
  float rz = sv[r], quad = 0.f, rprod = 1.f;
  static_for<0, 32>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const float ajj = (j & 1) ? ap[j / 2].y : ap[j / 2].x;
    const float rinv = rsqrt_newton(rdlane_u(ajj, j));
    const float lj = ajj * rinv;
    const float zj = rdlane_u(rz, j) * rinv;
    rz = fmaf(-lj, zj, rz);
    quad = fmaf(zj, zj, quad);
    rprod *= rinv;
    const float nt = -(lj * rinv);
    // pairs i >= (j + 1) / 2; for even j the first pair is (a[j], a[j + 1]) and its .x -- the finished column entry,
    // never read again -- is updated along with the live .y
    constexpr int i_first = (j + 1) / 2;
    static_for<0, (16 - i_first + BF_MFMA_RDB / 2 - 1) / (BF_MFMA_RDB / 2)>([&](auto Cb) {
      constexpr int i0 = i_first + decltype(Cb)::value * (BF_MFMA_RDB / 2);
      constexpr int ni = (16 - i0) < BF_MFMA_RDB / 2 ? (16 - i0) : BF_MFMA_RDB / 2;
      f32x2 sb[BF_MFMA_RDB / 2];
      static_for<0, ni>([&](auto I) {
        constexpr int i = i0 + decltype(I)::value;
        sb[decltype(I)::value] = f32x2{rdlane_u(ap[i].x, j), rdlane_u(ap[i].y, j)};
      });
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, ni>([&](auto I) {
        constexpr int i = i0 + decltype(I)::value;
        ap[i] = __builtin_elementwise_fma(f32x2{nt, nt}, sb[decltype(I)::value], ap[i]);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  });
  // -sum log L_jj = log prod (1 / L_jj) (32 factors of O(1) stay in range)
  return -0.5f * quad - 0.5f * 32.0f * 1.8378770664093453f + fast_log(rprod);
}

}  // namespace bf
