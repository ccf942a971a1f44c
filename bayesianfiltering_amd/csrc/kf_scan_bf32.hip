// kf_scan_bf32: the one-wave matrix-core Kalman kernel's eight plain instances (kf_scan_bf32.hpp: the kernel) and its launcher.
#include "kf_scan_bf32.hpp"

namespace bf {

hipError_t bf32_launch_plain(const Bf32Args& a, bool multi, int dyn_kind, hipStream_t stream) {
  return bf32_launch_instance<false>(a, multi, dyn_kind, stream);
}

// K = 1: bf_kalman_filter_f32; K >= 1: the Gaussian-sum filter of a linear model (bf_gsf_ekf_f32), components in turn.
// dyn_kind: 0 = linear (p->A), 1 = Lorenz-96, 2 = sine with scalars dth (identity noise input: p->G == NULL, dq == n); nonlinear
// chains always run as `multi` (K >= 1).  missing: the MISSING = true twins (NaN observations are gaps; the packing is the same).
int launch_kf_bf32(const bf_lgssm* p, const bf_cstream* y, long long B, long long T, const bf_carry* carry, const bf_out_desc* out,
                   hipStream_t stream, int K, bool multi, int dyn_kind, const float* dth, bool missing) {
  constexpr int N = 32;
  const int nr = p->n, mr = p->m, dq = p->dq, dr = p->dr;
  if (nr > N || mr > N) return set_error(BF_EUNSUPPORTED, "one-wave matrix-core Kalman kernel: n <= 32 and m <= 32");
  if (K > 64) return set_error(BF_EUNSUPPORTED, "one-wave matrix-core kernel: at most 64 components (one per lane in the weight update)");
  if ((p->Q_steps > 1 && p->Q_steps != T) || (p->R_steps > 1 && p->R_steps != T))
    return set_error(BF_EINVAL, "time-varying covariances need one matrix per step (Q_steps / R_steps = T = %lld)", T);
  if (dyn_kind != 0 && (!multi || p->G || dq != nr)) return set_error(BF_EINVAL, "nonlinear chains: identity noise input, multi launch");
  Bf32Const* h = new Bf32Const();  // zero-filled: the constant cache compares contents
  for (int i = 0; i < 8; ++i) h->dth[i] = (dyn_kind != 0 && dth) ? dth[i] : 0.f;
  if (dyn_kind == 0) split_bf16x3(p->A, nr, nr, nr, h->A3, N);
  split_bf16x3(p->H, mr, nr, nr, h->H3, N);
  noise_cov(p->G, p->Q, nr, dq, h->GQG, N);
  noise_cov(p->D, p->R, mr, dr, h->DRD, N);
  for (int i = mr; i < N; ++i) h->DRD[i * N + i] = 1.0f;   // padded observations: unit noise
  noise_mean(p->G, p->q0, nr, dq, h->Gq0);
  noise_mean(p->D, p->r0, mr, dr, h->Dr0);
  const void* dv = nullptr;
  const int crc = device_constants(h, sizeof(*h), stream, &dv);
  delete h;
  if (crc != BF_OK) return crc;
  const Bf32Const* dc = static_cast<const Bf32Const*>(dv);

  auto [yv, cv, ov] = forward_views(y, carry, out);
  // per-step tables (_get_params(x, 2, t), inference.py:21): T blocks of 32 x 32, formed on the device; MULTI: somewhere for
  // the log-likelihoods
  float *d_tvq = nullptr, *d_tvr = nullptr, *llscratch = nullptr;
  auto free_tables = [&]() {
    if (d_tvq) (void)hipFreeAsync(d_tvq, stream);
    if (d_tvr) (void)hipFreeAsync(d_tvr, stream);
  };
  int rc = BF_OK;
  if (p->Q_steps > 1) rc = tv_table_on_device(p->G, p->Q, T, nr, dq, N, N, stream, &d_tvq);
  if (rc == BF_OK && p->R_steps > 1) rc = tv_table_on_device(p->D, p->R, T, mr, dr, N, mr, stream, &d_tvr);
  if (rc == BF_OK && multi) rc = begin_multi(B, T, K, stream, ov, &llscratch);
  if (rc != BF_OK) { free_tables(); return rc; }

  const Bf32Args args{dc, yv, cv, ov, multi ? B * K : B, T, nr, mr, multi ? K : 1, d_tvq, d_tvr};
  const hipError_t le = missing ? bf32_launch_missing(args, multi, dyn_kind, stream) : bf32_launch_plain(args, multi, dyn_kind, stream);
  free_tables();
  if (le != hipSuccess && llscratch) (void)hipFreeAsync(llscratch, stream);
  BF_HIP_CHECK(le);
  if (multi) return finish_multi(ov, carry, B, T, K, stream, llscratch);
  return BF_OK;
}

}  // namespace bf
