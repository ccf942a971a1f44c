// Kernel-argument views: the structs the host fills and the kernels take BY VALUE, so host and device must agree on them byte
// for byte.  Defined here once, with no includes: bf_common.hpp brings this file into the ahead-of-time build, jit_embed.py
// embeds its text for the kernels compiled at run time (jit_source.hip).
#pragma once

namespace bf {

// Device-side view of one strided stream with the component axis folded in by the caller.
struct SView {
  float* p;
  long long sB, sK, sT, sE;
};
struct CView {
  const float* p;
  long long sB, sT, sE;
};

struct OutViews {
  SView w, m, P, pm, pP, ll;
  SView cm, cP;  // collapsed mean / covariance of the filtered mixture (Gaussian-sum kernel only)
};

struct CarryView {
  const float* w_in;
  const float* m_in;
  const float* P_in;
  float* w_out;
  float* m_out;
  float* P_out;
};

struct UView {
  const float* p;  // NULL: inputs = zeros((T, 1)) as inference.py:23
  long long sB, sT;
};
struct UViewG {  // (the same, under the name the run-time-dimension kernels carry in their signatures)
  const float* p;
  long long sB, sT;
};

}  // namespace bf
