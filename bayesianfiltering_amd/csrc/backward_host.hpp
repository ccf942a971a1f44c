// Host side of the backward family -- the RTS smoother (rts_smoother.hip) and the posterior sampler (ffbs_sampler.hip) over
// a filter's streams.  Host only: rts_generic.hpp, whose text the run-time compiles embed, holds the device half.
//
// A call resolves its ROUTE once (backward_route: the kind, n and the host constants that kind needs; backward_host.hip),
// and backward_dispatch sends the route to a PRODUCT: it decides between the register kernels and the run-time-dimension
// kernel, builds the kernel argument of either and calls one of the product's four launches.  A product is a small struct
//   template <int N, int KIND, class Arg> int regs(const Arg& c, const float* d_gqg) const;   // compiled register instance
//   int user_regs(const bf_user_model* um, int n, RtsUserHost& h) const;                      // ... built around source
//   int generic(const RtsGen& c, const GenModel& g, const std::vector<float>& blk) const;     // compiled LDS kernel
//   int user_generic(const bf_model* p, const RtsGen& c) const;                                // ... built around source
// holding the call's views, sizes and stream (RtsProduct, FfbsProduct).  A new route touches backward_route, backward_dispatch
// and the device side's rts_linearize / rts_gen_linearize; no product.
#pragma once
#include <cstring>
#include <vector>
#include "user_model.hpp"
#include "rts_generic.hpp"

namespace bf {

// Largest n on the register kernels, for every route and both products: every instance up to it -- both data paths of the
// smoother, the four samples-per-lane counts of the sampler, the source route measured on a Lorenz-96 twin -- builds without
// scratch (the tables in the headers of rts_smoother.hip and ffbs_sampler.hip).  BF_RTS_DIMS instantiates exactly these.
enum { BACKWARD_REG_MAX = 8 };

// return GO_(std::integral_constant<int, n>{}) for n = 1 ... BACKWARD_REG_MAX
#define BF_RTS_DIMS(N_, GO_)                                     \
  switch (N_) {                                                  \
    case 1: return GO_(std::integral_constant<int, 1>{});        \
    case 2: return GO_(std::integral_constant<int, 2>{});        \
    case 3: return GO_(std::integral_constant<int, 3>{});        \
    case 4: return GO_(std::integral_constant<int, 4>{});        \
    case 5: return GO_(std::integral_constant<int, 5>{});        \
    case 6: return GO_(std::integral_constant<int, 6>{});        \
    case 7: return GO_(std::integral_constant<int, 7>{});        \
    default: return GO_(std::integral_constant<int, 8>{});       \
  }

Option& force_generic_option();  // bf_api.hip

// ---- model validation, one per family; `noun`: "extended smoother", "unscented sampler", ... -----------------------------
int backward_check_lgssm(const bf_lgssm* p);                        // dimensions, A, G
int backward_check_recompute(const bf_lgssm* p, long long T);       // the recompute path: Q, Q_steps in {1, T}
int backward_check_source(const bf_model* p, const char* noun, bool unscented);   // functions from source, flags, the handle
int backward_check_dims(const bf_model* p);                         // dimensions, Q, R

// ---- host constants ----------------------------------------------------------------------------------------------------
int gen_fill(const bf_model* p, long long T, GenModel& g, std::vector<float>& blk);  // generic_scan.hip
// The unscented route's model on the host: the filter's own model fill (ugsf_scan.hpp: fill_ukf_model_view validates the
// registry ids and forms the constants), reduced to what X_t reads.  BF_EINVAL for ParamsUKF values with L + lambda <= 0.
struct RtsUnscHost {
  int dyn_id;
  float dth[8];
  std::vector<float> A, Gq0;
  float cu, wu;
};
// Source route: the kernel argument of the register kernels built at run time (RtsUser<DQ> of rts_smoother.hpp is its first
// 64 + dq floats)
struct RtsUserHost {
  float theta[64];
  float q0[64];
};

struct BackwardRoute {
  int kind = RTS_LIN, n = 0;
  const bf_lgssm* lin = nullptr;          // RTS_LIN, RTS_LIN_RECOMPUTE
  std::vector<float> A, GQG, Gq0;         // ... A, G Q_s G^T for every step s of Q (zeros without Q), G q0
  const bf_model* model = nullptr;        // RTS_EXT; RTS_EXT_USER: with the bf_user_model handle, theta and q0
  GenModel g;                             // RTS_EXT: gen_fill's model, pointers as offsets into ...
  std::vector<float> blk;                 // ... its constant block
  RtsUnscHost unsc;                       // RTS_UNSC
};
// (the route keeps `p`: it must outlive the dispatch)
int backward_route(const bf_lgssm* p, bool recompute, BackwardRoute& r);
int backward_route(const bf_model* p, long long T, BackwardRoute& r);             // validates the registry ids and theta layouts
int backward_route(const bf_model* p, const bf_ukf_params* up, BackwardRoute& r);

// the linear kinds' constant block A | Gq0 | GQG[qs], with c's pointers as offsets into it
void rts_gen_lin_block(const BackwardRoute& r, RtsGen& c, std::vector<float>& blk);
// the run-time-dimension kernels' constant block A | Gq0 and c for RTS_UNSC
void rts_gen_unsc_block(const RtsUnscHost& h, int n, RtsGen& c, std::vector<float>& blk);
// theta and q0 of the source route's register kernels; they hold 64 parameters, more are refused (the LDS kernels read
// them from memory and take any number, so this belongs to the register branch)
int rts_user_fill(const bf_model* p, RtsUserHost& h);
// uploads blk (content-keyed cache) and turns the offsets of c (linear kinds, RTS_UNSC) or g (RTS_EXT) into device pointers
int rts_gen_upload(RtsGen& c, GenModel& g, const std::vector<float>& blk, hipStream_t stream);
// The source route's run-time-dimension launch once the product has planned its LDS: the B range check (`noun`: "smoother" /
// "sampler"), q0 | theta uploaded behind a GenModel, the handle's kernel of `jit_kind`, one workgroup per trajectory.
// `c` and `views` are the product's first and third kernel arguments.  K > 0 (the Gaussian-sum kinds): one workgroup per chain,
// B K in all, and K -- or `last`, when given -- as the kernel's last argument.
int backward_launch_user_generic(const bf_model* p, int jit_kind, const char* noun, void* c, void* views, long long B, long long T,
                                 size_t lds, hipStream_t stream, int K = 0, void* last = nullptr);
// the smoother of one-component streams on the route `r` (rts_smoother.hip): the register kernels with their data path, or the
// run-time-dimension kernel.  The Gaussian-sum smoother calls it with B K trajectories where the layout flattens.
int rts_run(const BackwardRoute& r, const RtsViews& v, long long B, long long T, void* stream);
Option& rts_load_mode_option();  // rts_smoother.hip
// bf_out_desc / bf_smooth_carry / bf_smooth_desc -> RtsViews with the checks every smoother entry point makes (rts_smoother.hip):
// required streams and outputs, the carry's pairs
int rts_views(const bf_out_desc* f, const bf_smooth_carry* carry, const bf_smooth_desc* out, const bf_cstream* u, bool need_pred,
              RtsViews& v);
// bf_out_desc / bf_sample_carry / bf_sample_desc -> FfbsViews with the checks every linear or extended sampler entry point makes
// (ffbs_sampler.hip): sizes, required streams and output, noise or keys, the key mode's count limit
int ffbs_views(const bf_out_desc* f, const bf_sample_carry* carry, const bf_sample_desc* out, const bf_cstream* u, long long B,
               long long T, int S, int n, bool need_pred, FfbsViews& v);
Option& ffbs_spl_option();  // ffbs_sampler.hip
int launch_collapse(const bf_stream* w, const bf_stream* m, const bf_stream* P, long long B, long long T, int K, int n,
                    float* mean_out, float* cov_out, hipStream_t stream);  // collapse.hip

template <int N>
inline RtsLin<N> rts_lin_arg(const BackwardRoute& r) {
  RtsLin<N> c;
  std::memcpy(c.A, r.A.data(), sizeof(c.A));
  std::memcpy(c.GQG, r.GQG.data(), sizeof(c.GQG));
  std::memcpy(c.Gq0, r.Gq0.data(), sizeof(c.Gq0));
  return c;
}
template <int N>
inline EkfModel<N, 1> rts_ekf_arg(const BackwardRoute& r) {
  EkfModel<N, 1> e;
  std::memset(&e, 0, sizeof(e));
  e.dyn_id = r.model->dyn_id;
  for (int i = 0; i < 8; ++i) e.dth[i] = r.g.dth[i];
  if (r.model->dyn_id == DYN_LINEAR) for (int i = 0; i < N * N; ++i) e.A[i] = r.model->dyn_theta[i];
  return e;
}
template <int N>
inline RtsUnsc<N> rts_unsc_arg(const RtsUnscHost& h) {
  RtsUnsc<N> c;
  std::memset(&c, 0, sizeof(c));
  c.dyn_id = h.dyn_id;
  for (int i = 0; i < 8; ++i) c.dth[i] = h.dth[i];
  std::memcpy(c.A, h.A.data(), sizeof(c.A));
  std::memcpy(c.Gq0, h.Gq0.data(), sizeof(c.Gq0));
  c.c = h.cu;
  c.w = h.wu;
  return c;
}

// The one place that decides between the register kernels (n <= BACKWARD_REG_MAX unless "force_generic") and the
// run-time-dimension kernel, for every route and both products.
template <class Product>
int backward_dispatch(const BackwardRoute& r, bool force_generic, const Product& prod, hipStream_t stream) {
  const int n = r.n;
  if (!force_generic && n <= BACKWARD_REG_MAX) {
    if (r.kind == RTS_EXT_USER) {
      RtsUserHost h;
      const int rc = rts_user_fill(r.model, h);
      if (rc != BF_OK) return rc;
      return prod.user_regs(r.model->user, n, h);
    }
    const float* d_gqg = nullptr;
    if (r.kind == RTS_LIN_RECOMPUTE && r.lin->Q_steps > 1) {  // the time-varying table; the constant one travels in RtsLin
      const void* dv = nullptr;
      const int rc = device_constants(r.GQG.data(), sizeof(float) * r.GQG.size(), stream, &dv);
      if (rc != BF_OK) return rc;
      d_gqg = static_cast<const float*>(dv);
    }
    auto go = [&](auto NC) -> int {
      constexpr int N = decltype(NC)::value;
      switch (r.kind) {
        case RTS_LIN: return prod.template regs<N, RTS_LIN>(rts_lin_arg<N>(r), nullptr);
        case RTS_LIN_RECOMPUTE: return prod.template regs<N, RTS_LIN_RECOMPUTE>(rts_lin_arg<N>(r), d_gqg);
        case RTS_EXT: return prod.template regs<N, RTS_EXT>(rts_ekf_arg<N>(r), nullptr);
        default: return prod.template regs<N, RTS_UNSC>(rts_unsc_arg<N>(r.unsc), nullptr);
      }
    };
    BF_RTS_DIMS(n, go)
  }
  RtsGen c;
  std::memset(&c, 0, sizeof(c));
  c.n = n;
  c.kind = r.kind;
  if (r.kind == RTS_EXT_USER) return prod.user_generic(r.model, c);
  if (r.kind == RTS_EXT) return prod.generic(c, r.g, r.blk);
  GenModel g;
  std::memset(&g, 0, sizeof(g));
  std::vector<float> blk;
  if (r.kind == RTS_UNSC) rts_gen_unsc_block(r.unsc, n, c, blk);
  else rts_gen_lin_block(r, c, blk);
  return prod.generic(c, g, blk);
}

}  // namespace bf
