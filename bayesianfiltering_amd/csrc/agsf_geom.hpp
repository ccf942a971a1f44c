// agsf_geom: the output block and launch preparation of the augmented Gaussian-sum scan (agsf_scan.hpp), shared by the compiled
// instances and the kernels built at run time from the caller's source (agsf_ukf.hip).
#pragma once
#include "scan_common.hpp"

namespace bf {

struct AgsfOut {
  SView w, m, P;
  int* anc;  // [B][T][N0] index of the leaf each carried component was drawn from (NULL = not emitted)
};

#ifndef BF_JIT
// everything of a launch but the model: a lane per leaf of the [N0, N1, N2] tree, MP lanes per trajectory on nw waves
struct AgsfLaunch {
  CView y;
  UView u;
  CarryView carry;
  AgsfOut out;
  int MP, nw, nt, carry_records;
  size_t lds_bytes;
  unsigned grid;
};
static inline int prepare_agsf(int n, const bf_cstream* y, const bf_cstream* u, long long B, const int32_t nc[3], const bf_carry* carry,
                               const bf_out_desc* out, int* d_leaf_idx, AgsfLaunch& L) {
  const long long Mleaf = (long long)nc[0] * nc[1] * nc[2];
  if (Mleaf > 1024)
    return set_error(BF_EUNSUPPORTED, "augmented Gaussian-sum filter: %lld leaves per trajectory exceed one workgroup (1024)", Mleaf);
  if (out->pred_means.ptr || out->pred_covs.ptr || out->coll_mean.ptr || out->coll_cov.ptr || out->loglik.ptr)
    return set_error(BF_EINVAL, "the augmented filter emits weights, means and covariances only (inference.py:771-775)");
  L.MP = 1;
  while (L.MP < Mleaf) L.MP <<= 1;
  L.nw = 1;
  if (L.MP > 64) {  // e.g. the [5, 5, 5] tree of the reference's own test: 125 leaves on 2 waves; [100, 2, 2] of BOT_Experiment_script.py:118: 400 on 8
    if (n > 4)      // the multi-wave geometries are built for the small state dimensions only (build time, LDS)
      return set_error(BF_EUNSUPPORTED, "augmented Gaussian-sum filter: more than 64 leaves per trajectory need state_dim <= 4");
    L.nw = L.MP / 64;   // 2, 4, 8 or 16
  }
  L.nt = L.nw == 1 ? 256 : 64 * L.nw;
  L.carry_records = L.nw == 1 ? 256 : ((nc[0] + 3) & ~3);
  // dynamic LDS: leaf records, carried records, cumulative weights, carried weights, cross-wave scratch, resampling tables
  const int rec = n + n * n;
  L.lds_bytes = sizeof(float) * ((size_t)L.nt * rec + (size_t)L.carry_records * rec + L.nt + L.carry_records + 64 + (L.nw > 1 ? 4 * L.nt : 0));
  if (L.lds_bytes > 160 * 1024)
    return set_error(BF_EUNSUPPORTED, "augmented Gaussian-sum filter: %d leaves and %d components of dimension %d exceed the 160 KiB LDS",
                     (int)Mleaf, nc[0], n);
  L.y = CView{y->ptr, y->sB, y->sT, y->sE};
  L.u = UView{u && u->ptr ? u->ptr : nullptr, u ? u->sB : 0, u ? u->sT : 0};
  L.carry = CarryView{carry->w_in, carry->m_in, carry->P_in, carry->w_out, carry->m_out, carry->P_out};
  L.out = AgsfOut{make_sview(out->weights), make_sview(out->means), make_sview(out->covs), d_leaf_idx};
  const int tpb = L.nt / L.MP;
  L.grid = (unsigned)((B + tpb - 1) / tpb);
  return BF_OK;
}

// agsf_generic.hip: the same filters on the run-time-dimension kernel (the node in turn in LDS; registry functions, any of n, dq, m,
// dr above 8 -- or bf_set_option "agsf_force_generic" = 1).  up == NULL: extended-Kalman nodes, else unscented nodes.
extern Option g_agsf_force_generic;
int launch_agsf_generic(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B, long long T,
                        const int32_t nc[3], const uint32_t key[2], const float opt[2], const bf_carry* carry, const bf_out_desc* out,
                        int* d_leaf_idx, int variant, hipStream_t stream);
static inline bool agsf_beyond_registers(const bf_model* p) { return p->n > 8 || p->dq > 8 || p->m > 8 || p->dr > 8; }
#endif

}  // namespace bf
