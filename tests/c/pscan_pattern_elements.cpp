// The pattern table of the parallel-in-time Kalman filter's missing-observation route (csrc/kf_pscan_patterns.hpp), built for
// the host by a plain C++ compiler: the header has no HIP dependence.
//
//   pscan_pattern_elements MODEL     MODEL: binary, int32 n, int32 m, then float32 A (n n), H (m n), Qb (n n), Rb (m m)
//
// prints one line per pattern p = 0 ... 2^m - 1, "p" followed by the entry's 3 n^2 + 2 n m floats (A_e | C_e | J_e | K | W, %.9g
// round-trips fp32), then a line "plain" with what ps_fill_const hands the plain route (the element of the complete pattern,
// formed on its own), and checks on the way that every entry is, bit for bit, the complete-pattern element of the model
// COMPACTED to the observed rows (its K and W columns scattered back): the embedding adds exact zeros and nothing else.
// Exit status 0 = the table was built and no entry differed; 2 = a singular S_o.
#include "kf_pscan_patterns.hpp"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace bf;

template <int N, int M>
static void print_entry(const char* tag, const PsPattern<N, M>& e) {
  std::printf("%s", tag);
  const float* f = e.Ae;   // the struct is packed floats (static_assert in the header)
  for (int i = 0; i < PsPattern<N, M>::F; ++i) std::printf(" %.9g", f[i]);
  std::printf("\n");
}

// the entry of `pattern` against the complete-pattern element of the compacted model with MR rows
template <int N, int M, int MR>
static int against_compacted(const float* A, const float* H, const float* Qb, const float* Rb, unsigned pattern,
                             const PsPattern<N, M>& e) {
  int idx[M], r = 0;
  for (int a = 0; a < M; ++a) if (pattern >> a & 1u) idx[r++] = a;
  if (r != MR) return 0;
  PsPattern<N, M> want;
  std::memset(&want, 0, sizeof(want));
  if constexpr (MR == 0) {
    for (int i = 0; i < N * N; ++i) want.Ae[i] = A[i];
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) want.Ce[i * N + j] = (float)(0.5 * ((double)Qb[i * N + j] + (double)Qb[j * N + i]));
  } else {
    float Hr[MR * N], Rr[MR * MR];
    for (int a = 0; a < MR; ++a) {
      for (int i = 0; i < N; ++i) Hr[a * N + i] = H[idx[a] * N + i];
      for (int b = 0; b < MR; ++b) Rr[a * MR + b] = Rb[idx[a] * M + idx[b]];
    }
    PsPattern<N, MR> c;
    if (!ps_pattern_element<N, MR>(A, Hr, Qb, Rr, (1u << MR) - 1u, c)) return 1;
    std::memcpy(want.Ae, c.Ae, sizeof(c.Ae));
    std::memcpy(want.Ce, c.Ce, sizeof(c.Ce));
    std::memcpy(want.Je, c.Je, sizeof(c.Je));
    for (int i = 0; i < N; ++i) for (int a = 0; a < MR; ++a) { want.K[i * M + idx[a]] = c.K[i * MR + a]; want.W[i * M + idx[a]] = c.W[i * MR + a]; }
  }
  int bad = 0;
  const float *x = e.Ae, *y = want.Ae;
  for (int i = 0; i < PsPattern<N, M>::F; ++i) bad += !(x[i] == y[i]);   // (== : +0 and -0 are the same number)
  if (bad) std::fprintf(stderr, "n=%d m=%d pattern=%x: %d entries differ from the compacted model's\n", N, M, pattern, bad);
  return bad;
}

template <int N, int M>
static int run(const float* A, const float* H, const float* Qb, const float* Rb) {
  static PsPatternTable<N, M> t;
  if (!ps_pattern_table<N, M>(A, H, Qb, Rb, t)) return 2;
  int bad = 0;
  for (unsigned p = 0; p < (1u << M); ++p) {
    char tag[16];
    std::snprintf(tag, sizeof(tag), "%u", p);
    print_entry<N, M>(tag, t.p[p]);
    bad += against_compacted<N, M, 0>(A, H, Qb, Rb, p, t.p[p]) + against_compacted<N, M, 1>(A, H, Qb, Rb, p, t.p[p]);
    if constexpr (M >= 2) bad += against_compacted<N, M, 2>(A, H, Qb, Rb, p, t.p[p]);
    if constexpr (M >= 3) bad += against_compacted<N, M, 3>(A, H, Qb, Rb, p, t.p[p]);
    if constexpr (M >= 4) bad += against_compacted<N, M, 4>(A, H, Qb, Rb, p, t.p[p]);
  }
  PsPattern<N, M> plain;
  if (!ps_pattern_element<N, M>(A, H, Qb, Rb, (1u << M) - 1u, plain)) return 2;
  print_entry<N, M>("plain", plain);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::FILE* f = std::fopen(argv[1], "rb");
  int32_t dims[2];
  if (!f || std::fread(dims, 4, 2, f) != 2) return 65;
  const int n = dims[0], m = dims[1];
  if (n < 1 || n > 6 || m < 1 || m > 4) return 66;
  std::vector<float> v((size_t)(2 * n * n + m * n + m * m));
  if (std::fread(v.data(), 4, v.size(), f) != v.size()) return 65;
  std::fclose(f);
  const float *A = v.data(), *H = A + n * n, *Qb = H + m * n, *Rb = Qb + n * n;
#define BF_ROW(N_)                                   \
  if (n == N_ && m == 1) return run<N_, 1>(A, H, Qb, Rb); \
  if (n == N_ && m == 2) return run<N_, 2>(A, H, Qb, Rb); \
  if (n == N_ && m == 3) return run<N_, 3>(A, H, Qb, Rb); \
  if (n == N_ && m == 4) return run<N_, 4>(A, H, Qb, Rb);
  BF_ROW(1) BF_ROW(2) BF_ROW(3) BF_ROW(4) BF_ROW(5) BF_ROW(6)
#undef BF_ROW
  return 66;
}
