// agsf_generic: the five augmented Gaussian-sum filters for ANY dimensions (run-time n, dq, m, dr) -- host side and dispatch of
// agsf_generic_device.hpp.
//
// Same recursion as the register kernel (agsf_scan.hpp) -- the lax.scan bodies of speedy_augmented_gaussian_sum_filter,
// augmented_gaussian_sum_filter, augmented_gaussian_sum_filter_optimal, speedy_unscented_agsf and unscented_agsf
// (gaussfiltax/inference.py:458-1300) -- for the shapes that kernel's registers do not hold: any of n, dq, m, dr above 8, more than
// 64 leaves above n = 4, a nonlinear registry model outside the eight compiled (n, m) pairs.
//
// Mapping (gfx950).  One workgroup advances one trajectory; the tree's nodes take turns in LDS.  Per step:
//   * predict phase, per carried component i0: A = P - a0 P, L = chol((A + A^T) / 2) in an LDS tile of its own (left-looking, a row
//     per lane, chol_jax's all-NaN rule), then per z-sample i1 the node (m + L eps_z[i0][:, i1], a0 P) goes through the
//     run-time-dimension filters' prediction (extended: gsf_generic_body's _predict sequence; unscented: ugsf_generic_body's
//     _ukf_predict_nonadditive sequence) and lands in a per-workgroup HBM scratch of N0 N1 records;
//   * update phase, per predicted node j: the same with a1 and eps_s[j][:, i2]; the node conditions on y_t (S + 1e-6 LU solve,
//     P - K S K^T with the un-jittered S, Cholesky log-likelihood) and lands in a scratch of M = N0 N1 N2 leaf records, its
//     log-likelihood in LDS;
//   * reweight and resample, one lane per leaf: agsf_scan.hpp's block helpers (adjacent-pair trees, Brent-Kung cumulative sum over
//     the padded leaves, jr.choice under PRNGKey(0) or optimal_resampling_block), then the drawn leaves are copied into the carry
//     records and the output streams by the whole workgroup.
// The records are rewritten at every step, so they stay in L2; a workgroup's scratch is (N0 + N0 N1 + M)(n + n^2) floats and the grid
// is capped at AG_MAX_GRID workgroups, each looping over trajectories blockIdx.x, blockIdx.x + gridDim.x, ...  The reference never
// advances rng_key, so the normals are the same at every step and for every trajectory: a small kernel fills the two arrays
// (N0 n N1 and N0 N1 n N2 floats) once per call with agsf_scan.hpp's keys and counters -- the register kernel's bits.
//
// NT = 64 threads (one wave: the barriers are free) while every dimension is <= 36 (extended nodes) or <= 16 (unscented nodes) and
// the leaves fit one wave (padded count <= 64); 256 otherwise.  Both thresholds are measured (ag_nt64_max below);
// BAYESFILT_AGSF_NT64_MAX moves both.
// Limits: M <= 256 leaves (one lane per leaf of a 256-thread workgroup); registry functions (functions from source stay on the
// register kernel, dimensions up to 8).
//
// LDS (floats; r4 = round up to 4, ldn = r4(n) + 4, ldm = r4(m) + 4):
//   nodes + n ldn (factor tile) + r4(n) (sampled-from mean) + 8 NT + 64 (leaf arrays, block helpers, resampling tables), with
//   nodes = n ldn + 2 r4(n) + 5 r4(m) + max(3 m ldn + 3 n ldm + 4 m ldm, 3 n ldn)      extended   (generic_scan.hip's carve)
//   nodes = ug_carve(n, dq, m, dr, K = 4).total                                        unscented  (ugsf_generic.hip's carve)
// Above 160 KiB: BF_EUNSUPPORTED with the byte count.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; LDS is dynamic): DESIGN.md 4d.
#include <cstdlib>
#include <vector>
#include "forward_host.hpp"
#include "agsf_generic_device.hpp"
#include "user_model.hpp"

namespace bf {

int gen_fill(const bf_model* p, long long T, GenModel& g, std::vector<float>& blk);                                   // generic_scan.hip
int ug_model_prepare(const bf_model* p, const bf_ukf_params* up, int user_flags, hipStream_t stream, UgModel& g);     // ugsf_generic.hip

enum { AG_MAX_GRID = 2048 };   // workgroups (and HBM scratches) of a launch: 8 per compute unit

// one wave per workgroup (its barriers are free) up to this largest dimension, four waves above: 36 for extended nodes, 16 for
// unscented ones (ugsf_generic.hip's threshold: the Jacobi stages want the lanes).  Measured on Lorenz-96, tree (3, 2, 2), in
// M leaf-steps/s with one wave / four waves: extended n = 16 54.2 / 14.8, 24 26.9 / 8.3, 32 8.5 / 5.3, 36 6.4 / 4.2, 40 2.8 / 3.6;
// unscented n = 16 8.3 / 4.7, 24 1.5 / 1.9, 32 0.38 / 0.95, 40 0.19 / 0.47
static int ag_nt64_max(bool unscented) {
  static const int v = [] {
    const char* e = std::getenv("BAYESFILT_AGSF_NT64_MAX");
    const int x = e ? std::atoi(e) : 0;
    return x > 0 ? x : 0;
  }();
  return v > 0 ? v : (unscented ? 16 : 36);
}

Option g_agsf_force_generic{0, OPT_AGSF_FORCE_GENERIC};   // bf_set_option "agsf_force_generic": 1 = this kernel also where every dimension is <= 8

template <int NT, class NODES>
static int launch_ag(const typename NODES::Model& g, const AgTree& tr, const CView& yv, const UViewG& uv, const CarryView& cr,
                     const AgsfOut& ov, float* gs, const float* ez, const float* es, long long B, long long T, unsigned grid,
                     size_t lds_bytes, hipStream_t stream) {
  auto kern = agsf_generic_kernel<NT, NODES>;
  if (lds_bytes > 64 * 1024)
    BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, stream, g, tr, yv, uv, cr, ov, gs, ez, es, B, T);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

// up == NULL: extended-Kalman nodes; else unscented nodes
int launch_agsf_generic(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                        const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                        int* d_leaf_idx, int variant, hipStream_t stream) {
  const int n = p->n, dq = p->dq, m = p->m, dr = p->dr;
  if (p->user || p->dyn_id == DYN_USER || p->emi_id == EMI_USER)
    return set_error(BF_EUNSUPPORTED, "the augmented filters take registry functions above dimension 8 (functions from source and recorded "
                                      "Python functions: dimensions up to 8, a leaf lives in registers)");
  if (out->pred_means.ptr || out->pred_covs.ptr || out->coll_mean.ptr || out->coll_cov.ptr || out->loglik.ptr)
    return set_error(BF_EINVAL, "the augmented filter emits weights, means and covariances only (inference.py:771-775)");
  if (p->flags != 0) return set_error(BF_EUNSUPPORTED, "legacy-class flags do not apply to the augmented filter");
  const long long Mleaf = (long long)nc[0] * nc[1] * nc[2];
  if (Mleaf > AG_MAX_LEAVES)
    return set_error(BF_EUNSUPPORTED, "augmented Gaussian-sum filter, run-time dimensions: %lld leaves per trajectory exceed the limit of %d "
                                      "(one lane per leaf of a workgroup)", Mleaf, (int)AG_MAX_LEAVES);
  if ((p->Q_steps > 1 && p->Q_steps != T) || (p->R_steps > 1 && p->R_steps != T))
    return set_error(BF_EINVAL, "time-varying covariances need one matrix per step (Q_steps / R_steps = T = %lld)", T);
  if (up) {
    if (p->dyn_id != DYN_LINEAR && p->dyn_id != DYN_LORENZ96 && p->dyn_id != DYN_SINE)
      return set_error(BF_EUNSUPPORTED, "run-time-dimension augmented filter, unscented nodes: dynamics id %d runs on the compiled (n <= 8) instances only", p->dyn_id);
    if (p->emi_id != EMI_LINEAR && p->emi_id != EMI_QUADRATIC && p->emi_id != EMI_STOCH_VOL)
      return set_error(BF_EUNSUPPORTED, "run-time-dimension augmented filter, unscented nodes: emission id %d runs on the compiled (n <= 8) instances only", p->emi_id);
  }
  int MP = 1;
  while (MP < Mleaf) MP <<= 1;
  int dmax = n > dq ? n : dq;
  dmax = dmax > m ? dmax : m;
  dmax = dmax > dr ? dmax : dr;
  const int nt = (dmax <= ag_nt64_max(up != nullptr) && MP <= 64) ? 64 : 256;
  size_t lds_floats;
  if (up) lds_floats = nt == 64 ? ag_lds_floats<64, AgUkfNodes<64>>(n, dq, m, dr) : ag_lds_floats<256, AgUkfNodes<256>>(n, dq, m, dr);
  else lds_floats = nt == 64 ? ag_lds_floats<64, AgEkfNodes<64>>(n, dq, m, dr) : ag_lds_floats<256, AgEkfNodes<256>>(n, dq, m, dr);
  const size_t lds_bytes = sizeof(float) * lds_floats;
  if (lds_bytes > 160 * 1024)
    return set_error(BF_EUNSUPPORTED, "run-time-dimension augmented filter: n = %d, dq = %d, m = %d, dr = %d with %s nodes need %zu bytes of LDS "
                                      "(160 KiB per workgroup)", n, dq, m, dr, up ? "unscented" : "extended", lds_bytes);

  GenModel ge;
  UgModel gu;
  int rc;
  if (up) {
    if ((rc = ug_model_prepare(p, up, 0, stream, gu)) != BF_OK) return rc;
  } else {
    std::vector<float> blk;
    if ((rc = gen_fill(p, T, ge, blk)) != BF_OK) return rc;
    const void* dv = nullptr;
    if ((rc = device_constants(blk.data(), sizeof(float) * blk.size(), stream, &dv)) != BF_OK) return rc;
    const float* base = static_cast<const float*>(dv);
    auto fix = [&](const float*& q) { q = base + reinterpret_cast<size_t>(q); };
    fix(ge.A); fix(ge.Hm); fix(ge.Gq0); fix(ge.Dr0); fix(ge.R); fix(ge.r0); fix(ge.GQG); fix(ge.DRD);
    fix(ge.q0); fix(ge.Q); fix(ge.dyn_theta); fix(ge.emi_theta);
  }

  AgTree tr;
  tr.N0 = nc[0]; tr.N1 = nc[1]; tr.N2 = nc[2]; tr.M = (int)Mleaf; tr.variant = variant;
  tr.a0 = opt[0]; tr.a1 = opt[1];
  {  // utils.optimal_resampling(weights, N0, key) with the key left by the two splits (:1203, :1229)
    const U32x2 kz = threefry_split(key[0], key[1], 0u, 2u);
    const U32x2 ko = threefry_split(kz.x, kz.y, 0u, 2u);
    tr.ko0 = ko.x; tr.ko1 = ko.y;
  }
  const unsigned grid = (unsigned)(B < AG_MAX_GRID ? B : AG_MAX_GRID);
  const size_t cz = (size_t)nc[0] * n * nc[1], cs = (size_t)nc[0] * nc[1] * n * nc[2];
  const size_t per_wg = ag_scratch_floats(n, nc[0], nc[1], nc[2]);
  float* scratch = nullptr;
  BF_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&scratch), sizeof(float) * (cz + cs + (size_t)grid * per_wg), stream));
  float* ez = scratch;
  float* es = ez + cz;
  float* gs = es + cs;
  {
    const size_t tot = cz + cs;
    const unsigned nb = (unsigned)((tot + 255) / 256 < 1024 ? (tot + 255) / 256 : 1024);
    hipLaunchKernelGGL(agsf_normals_kernel, dim3(nb), dim3(256), 0, stream, ez, es, nc[0], nc[1], nc[2], n, key[0], key[1], variant);
  }
  rc = hipGetLastError() == hipSuccess ? BF_OK : set_error(BF_EHIP, "launch of the normals kernel failed");
  if (rc == BF_OK) {
    const ForwardViews fv = forward_views(y, carry, out);   // (of its streams the tree emits three: AgsfOut)
    const UViewG uv = input_view<UViewG>(u);
    const AgsfOut ov{make_sview(out->weights), make_sview(out->means), make_sview(out->covs), d_leaf_idx};
    if (up) rc = nt == 64 ? launch_ag<64, AgUkfNodes<64>>(gu, tr, fv.y, uv, fv.carry, ov, gs, ez, es, B, T, grid, lds_bytes, stream)
                          : launch_ag<256, AgUkfNodes<256>>(gu, tr, fv.y, uv, fv.carry, ov, gs, ez, es, B, T, grid, lds_bytes, stream);
    else rc = nt == 64 ? launch_ag<64, AgEkfNodes<64>>(ge, tr, fv.y, uv, fv.carry, ov, gs, ez, es, B, T, grid, lds_bytes, stream)
                       : launch_ag<256, AgEkfNodes<256>>(ge, tr, fv.y, uv, fv.carry, ov, gs, ez, es, B, T, grid, lds_bytes, stream);
  }
  (void)hipFreeAsync(scratch, stream);
  return rc;
}

}  // namespace bf
