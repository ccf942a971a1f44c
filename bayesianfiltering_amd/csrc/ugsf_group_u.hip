// Instantiations of the unscented Gaussian-sum filter kernel (ugsf_scan.hpp) for the (n, dq, m, dr) shapes compiled ahead of
// time, up to state dimension 4 (ugsf_group_v.hip holds (8, 8, 4, 4)).
// Built twice (bf_common.hpp): as it stands, and with -DBF_MISSING=true for the missing-observation instances of the same rows.
#include "ugsf_scan.hpp"

namespace bf {

int BF_GROUP_FN(ugsf, u)(const bf_model* p, const bf_ukf_params* up, const bf_cstream* y, const bf_cstream* u, long long B,
        long long T, int K, const bf_carry* carry, const bf_out_desc* out, hipStream_t stream, bool* matched) {
#define BF_CASE(N_, DQ_, M_, DR_)                                                               \
  if (p->n == N_ && p->dq == DQ_ && p->m == M_ && p->dr == DR_) {                               \
    *matched = true;                                                                            \
    return launch_ugsf<N_, DQ_, M_, DR_, BF_MISSING>(p, up, y, u, B, T, K, carry, out, stream); \
  }
  BF_CASE(1, 1, 1, 1);   // growth / sine + quadratic (Experiment_TSP_2023.ipynb cell 2)
  BF_CASE(2, 2, 1, 1);
  BF_CASE(2, 2, 2, 2);   // stochastic volatility (adaptive_experiment.py:51-54)
  BF_CASE(3, 3, 1, 1);   // Lorenz-63 + quadratic (exp_lorentz63.py)
  BF_CASE(3, 3, 3, 3);
  BF_CASE(4, 2, 1, 1);   // manoeuvring target + bearing only (docs/tests/test_inference.py)
  BF_CASE(4, 2, 2, 2);   // manoeuvring target + bearing / range, constant-velocity models (BOT_Experiment_script.py)
  BF_CASE(4, 4, 2, 2);
#undef BF_CASE
  *matched = false;
  return BF_OK;
}

}  // namespace bf
