// Host-side packing of a linear-Gaussian model's noise terms, shared by every launcher that uploads them (kf_scan_group.hpp,
// gsf_scan.hpp, generic_scan.hip, rts_smoother.hip, kf_scan_mfma.hip, kf_scan_bf32.hip).  Everything is fp32 with explicit
// fmaf chains in a fixed order, so two launchers given the same model upload the same bits -- and tv_table_kernel
// (mfma_multi.hip), which forms the per-step tables on the device, runs the same chains.  Host only; plain functions.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bf {

// dst[i * pitch + j] = sum_l (sum_k W[i][k] C[k][l]) W[j][l] for i, j < rows: (W C) W^T with the association of
// inference.py:69,:100, k then l ascending.  W is [rows][d] row-major, C is [d][d]; W == nullptr is the identity.
inline void noise_cov(const float* W, const float* C, int rows, int d, float* dst, int pitch) {
  auto Wat = [&](int i, int k) { return W ? W[(size_t)i * d + k] : (i == k ? 1.f : 0.f); };
  std::vector<float> WC((size_t)rows * d);
  for (int i = 0; i < rows; ++i)
    for (int l = 0; l < d; ++l) {
      float s = 0.f;
      for (int k = 0; k < d; ++k) s = std::fmaf(Wat(i, k), C[(size_t)k * d + l], s);
      WC[(size_t)i * d + l] = s;
    }
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < rows; ++j) {
      float s = 0.f;
      for (int l = 0; l < d; ++l) s = std::fmaf(WC[(size_t)i * d + l], Wat(j, l), s);
      dst[(size_t)i * pitch + j] = s;
    }
}

// dst[i] = sum_k W[i][k] c0[k] for i < rows, k ascending; W == nullptr is the identity, c0 == nullptr is zero.
inline void noise_mean(const float* W, const float* c0, int rows, int d, float* dst) {
  for (int i = 0; i < rows; ++i) {
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = std::fmaf(W ? W[(size_t)i * d + k] : (i == k ? 1.f : 0.f), c0 ? c0[k] : 0.f, s);
    dst[i] = s;
  }
}

// x = dst[0] + dst[1] + dst[2] exactly for finite x: three bf16 terms, each the round-to-nearest-even of what the earlier
// ones left (the residual of a 24-bit significand after an 8-bit term has at most 16 bits, after two at most 8).  Entry
// (i, j) of the [rows][cols] source goes to dst[t][i * dst_pitch + j]; what the caller zero-filled around it stays zero.
template <size_t TERM>
inline void split_bf16x3(const float* src, int rows, int cols, int src_pitch, unsigned short (&dst)[3][TERM], int dst_pitch) {
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      float x = src[(size_t)i * src_pitch + j];
      for (int t = 0; t < 3; ++t) {
        uint32_t u;
        std::memcpy(&u, &x, 4);
        u += 0x7FFFu + ((u >> 16) & 1u);
        const unsigned short hb = (unsigned short)(u >> 16);
        dst[t][(size_t)i * dst_pitch + j] = hb;
        u = (uint32_t)hb << 16;
        float f;
        std::memcpy(&f, &u, 4);
        x -= f;
      }
    }
}

}  // namespace bf
