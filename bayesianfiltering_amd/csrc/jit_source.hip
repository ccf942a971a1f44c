// jit_source: the text hiprtc compiles for a kernel built at run time -- the device headers embedded in the library
// (jit_sources.hip, written by jit_embed.py) around the caller's
//     template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* theta, T* out);
//     template <class T> __device__ void emission(const T* x, const T* r, T u, const float* theta, T* out);
// with the Jacobians from forward-mode dual numbers (T = bfu::Dual), i.e. exactly what jacfwd computes (gaussfiltax/inference.py:328-329).
#include "user_model.hpp"

namespace bf {

extern const char* const kViewsSource;          // bf_views.hpp, embedded at build time (jit_sources.hip)
extern const char* const kGenericDeviceSource;  // generic_device.hpp
extern const char* const kUgsfGenericSource;    // ugsf_generic_device.hpp
extern const char* const kSamplingSourceA;      // kf_math.hpp + bf_canon_math.hpp
extern const char* const kSamplingSourceB;      // scan_common / bf_rng / models / ssm_device / bpf_scan
extern const char* const kAgsfSource;           // agsf_geom.hpp + agsf_scan.hpp
extern const char* const kSampleSource;         // sample_ssm.hpp
extern const char* const kBpfBigSource;         // bpf_big.hpp
extern const char* const kUgsfSource;           // ugsf_scan.hpp
extern const char* const kRtsSource;            // rts_smoother.hpp
extern const char* const kFfbsSource;           // ffbs_sampler.hpp
extern const char* const kRtsGenericSource;     // rts_generic.hpp

namespace {

// forward-mode dual numbers + the elementary functions a model may call, for float and Dual alike (namespace bfu: the
// caller's source is compiled inside it, so unqualified sin / exp / sqrt ... resolve for both instantiations)
const char* const kDualCore = R"BFSRC(
struct Dual {
  float v, d;
  __device__ Dual() : v(0.f), d(0.f) {}
  __device__ Dual(float a) : v(a), d(0.f) {}
  __device__ Dual(float a, float b) : v(a), d(b) {}
};
#pragma clang fp contract(off)
__device__ inline Dual operator+(Dual a, Dual b) { return Dual(a.v + b.v, a.d + b.d); }
__device__ inline Dual operator-(Dual a, Dual b) { return Dual(a.v - b.v, a.d - b.d); }
__device__ inline Dual operator*(Dual a, Dual b) { return Dual(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ inline Dual operator/(Dual a, Dual b) { const float q = a.v / b.v; return Dual(q, (a.d - q * b.d) / b.v); }
__device__ inline Dual operator-(Dual a) { return Dual(-a.v, -a.d); }
__device__ inline Dual operator+(Dual a) { return a; }
__device__ inline Dual operator+(Dual a, float b) { return Dual(a.v + b, a.d); }
__device__ inline Dual operator+(float a, Dual b) { return Dual(a + b.v, b.d); }
__device__ inline Dual operator-(Dual a, float b) { return Dual(a.v - b, a.d); }
__device__ inline Dual operator-(float a, Dual b) { return Dual(a - b.v, -b.d); }
__device__ inline Dual operator*(Dual a, float b) { return Dual(a.v * b, a.d * b); }
__device__ inline Dual operator*(float a, Dual b) { return Dual(a * b.v, a * b.d); }
__device__ inline Dual operator/(Dual a, float b) { return Dual(a.v / b, a.d / b); }
__device__ inline Dual operator/(float a, Dual b) { const float q = a / b.v; return Dual(q, -q * b.d / b.v); }
__device__ inline Dual& operator+=(Dual& a, Dual b) { a = a + b; return a; }
__device__ inline Dual& operator-=(Dual& a, Dual b) { a = a - b; return a; }
__device__ inline Dual& operator*=(Dual& a, Dual b) { a = a * b; return a; }
__device__ inline Dual& operator/=(Dual& a, Dual b) { a = a / b; return a; }
__device__ inline bool operator<(Dual a, Dual b) { return a.v < b.v; }
__device__ inline bool operator>(Dual a, Dual b) { return a.v > b.v; }
__device__ inline bool operator<=(Dual a, Dual b) { return a.v <= b.v; }
__device__ inline bool operator>=(Dual a, Dual b) { return a.v >= b.v; }
__device__ inline bool operator==(Dual a, Dual b) { return a.v == b.v; }
__device__ inline bool operator!=(Dual a, Dual b) { return a.v != b.v; }
)BFSRC";
const char* const kLibmMath = R"BFSRC(
__device__ inline float sin(float x) { return ::sinf(x); }
__device__ inline float cos(float x) { return ::cosf(x); }
__device__ inline float tan(float x) { return ::tanf(x); }
__device__ inline float exp(float x) { return ::expf(x); }
__device__ inline float log(float x) { return ::logf(x); }
__device__ inline float sqrt(float x) { return ::sqrtf(x); }
__device__ inline float tanh(float x) { return ::tanhf(x); }
__device__ inline float atan(float x) { return ::atanf(x); }
__device__ inline float atan2(float y, float x) { return ::atan2f(y, x); }
__device__ inline float pow(float x, float p) { return ::powf(x, p); }
__device__ inline float abs(float x) { return ::fabsf(x); }
__device__ inline void sincos(float x, float* s, float* c) { *s = ::sinf(x); *c = ::cosf(x); }
__device__ inline float fma(float a, float b, float c) { return ::fmaf(a, b, c); }
)BFSRC";
// (on top of whichever float functions precede it: libm's for the extended-Kalman scan, the canonical ones for the sampling kernels)
const char* const kDualMath = R"BFSRC(
__device__ inline Dual sin(Dual x) { return Dual(sin(x.v), cos(x.v) * x.d); }
__device__ inline Dual cos(Dual x) { return Dual(cos(x.v), -sin(x.v) * x.d); }
__device__ inline Dual tan(Dual x) { const float t = tan(x.v); return Dual(t, (1.f + t * t) * x.d); }
__device__ inline Dual exp(Dual x) { const float e = exp(x.v); return Dual(e, e * x.d); }
__device__ inline Dual log(Dual x) { return Dual(log(x.v), x.d / x.v); }
__device__ inline Dual sqrt(Dual x) { const float s = sqrt(x.v); return Dual(s, x.d / (2.f * s)); }
__device__ inline Dual tanh(Dual x) { const float t = tanh(x.v); return Dual(t, (1.f - t * t) * x.d); }
__device__ inline Dual atan(Dual x) { return Dual(atan(x.v), x.d / (1.f + x.v * x.v)); }
__device__ inline Dual atan2(Dual y, Dual x) { const float r2 = x.v * x.v + y.v * y.v; return Dual(atan2(y.v, x.v), (x.v * y.d - y.v * x.d) / r2); }
__device__ inline Dual pow(Dual x, float p) { const float w = pow(x.v, p - 1.f); return Dual(w * x.v, p * w * x.d); }
__device__ inline Dual abs(Dual x) { return x.v < 0.f ? -x : x; }
__device__ inline void sincos(Dual x, Dual* s, Dual* c) { float sv, cv; sincos(x.v, &sv, &cv); *s = Dual(sv, cv * x.d); *c = Dual(cv, -sv * x.d); }
__device__ inline Dual fma(Dual a, Dual b, Dual c) { return a * b + c; }
__device__ inline Dual fma(float a, Dual b, Dual c) { return a * b + c; }
__device__ inline Dual fma(Dual a, float b, Dual c) { return a * b + c; }
)BFSRC";

// The run-time-dimension Gaussian-sum scan (generic_device.hpp) with dual-number Jacobians: libm's float functions.
// nt_ugsf = 0: its two entry points; 64 / 256: the run-time-dimension unscented scan (ugsf_generic_device.hpp) instead, on the
// same headers and the same float functions -- values of f and h only, no Jacobians.  nt_missing = 64 / 256: the MISSING = true
// twin of the Gaussian-sum scan at that workgroup size (NaN observations are gaps), one entry point.
std::string generic_scan_source(const bf_user_model& um, int nt_ugsf, int nt_missing = 0) {
  std::string s;
  s += "#define BF_JIT 1\n";
  if (um.has_dyn) s += "#define BF_USER_DYN 1\n";
  if (um.has_emi) s += "#define BF_USER_EMI 1\n";
  s += "#define BF_N " + std::to_string(um.n) + "\n#define BF_DQ " + std::to_string(um.dq) + "\n#define BF_M " + std::to_string(um.m) +
       "\n#define BF_DR " + std::to_string(um.dr) + "\n";
  s += "namespace bfu {\n";
  s += kDualCore;
  s += kLibmMath;
  s += kDualMath;
  s += "\n// ---- the caller's functions\n";
  if (um.has_dyn) s += um.dyn_src + "\n";
  if (um.has_emi) s += um.emi_src + "\n";
  s += "}  // namespace bfu\n";
  s += kViewsSource;
  s += kGenericDeviceSource;
  if (nt_ugsf != 0) {
    const std::string nt = std::to_string(nt_ugsf);
    s += kUgsfGenericSource;
    s += "extern \"C\" __global__ void __launch_bounds__(" + nt + ") bf_user_ugsf_generic(bf::UgModel p, bf::CView y, bf::UViewG u, bf::CarryView carry,\n"
         "    bf::OutViews out, float* gm, float* gP, long long B, long long T, int K, int KP) {\n"
         "  bf::ugsf_generic_body<" + nt + ">(p, y, u, carry, out, gm, gP, B, T, K, KP);\n}\n";
    return s;
  }
  if (nt_missing != 0) {
    const std::string nt = std::to_string(nt_missing);
    s += "extern \"C\" __global__ void __launch_bounds__(" + nt + ") bf_user_scan_missing(bf::GenModel p, bf::CView y, bf::UViewG u, bf::CarryView carry,\n"
         "    bf::OutViews out, float* gm, float* gP, long long B, long long T, int K, int KP) {\n"
         "  bf::gsf_generic_body<" + nt + ", true>(p, y, u, carry, out, gm, gP, B, T, K, KP);\n}\n";
    return s;
  }
  s += R"BFSRC(
extern "C" __global__ void __launch_bounds__(64) bf_user_scan_64(bf::GenModel p, bf::CView y, bf::UViewG u, bf::CarryView carry,
    bf::OutViews out, float* gm, float* gP, long long B, long long T, int K, int KP) {
  bf::gsf_generic_body<64>(p, y, u, carry, out, gm, gP, B, T, K, KP);
}
extern "C" __global__ void __launch_bounds__(256) bf_user_scan_256(bf::GenModel p, bf::CView y, bf::UViewG u, bf::CarryView carry,
    bf::OutViews out, float* gm, float* gP, long long B, long long T, int K, int KP) {
  bf::gsf_generic_body<256>(p, y, u, carry, out, gm, gP, B, T, K, KP);
}
)BFSRC";
  return s;
}

// The particle-filter kernel (bpf_scan.hpp) with the caller's functions compiled in: state in registers at the compile-time
// dimensions of the handle, one entry per particle capacity.  The caller's functions see the CANONICAL arithmetic of the
// weight path (bf_canon_math.hpp: sin / cos / atan2 / exp / log as defined there, IEEE sqrt, no contraction), so a function
// written like its registry twin gives the registry twin's bits.
const char* const kSamplingUserMath = R"BFSRC(
#pragma clang fp contract(off)   // no contraction in the caller's functions, as in the registry's
namespace bfu {
__device__ inline float sin(float x) { return bf::canon_sin(x); }
__device__ inline float cos(float x) { float s, c; bf::canon_sincos(x, &s, &c); return c; }
__device__ inline void sincos(float x, float* s, float* c) { bf::canon_sincos(x, s, c); }
__device__ inline float exp(float x) { return bf::canon_exp(x); }
__device__ inline float log(float x) { return bf::canon_log(x); }
__device__ inline float sqrt(float x) { return __builtin_sqrtf(x); }
__device__ inline float atan2(float y, float x) { return bf::canon_atan2(y, x); }
__device__ inline float atan(float x) { return bf::canon_atan(x); }
__device__ inline float abs(float x) { return __builtin_fabsf(x); }
__device__ inline float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ inline float tan(float x) { return ::tanf(x); }       // (no canonical definition: none of the sampling paths' twins needs one)
__device__ inline float tanh(float x) { return ::tanhf(x); }
__device__ inline float pow(float x, float p) { return ::powf(x, p); }
)BFSRC";

}  // namespace

const char* jit_entry_name(int kind, int variant) {
  switch (kind) {
    case JIT_RTS_GENERIC: return "bf_user_rts_generic";
    case JIT_FFBS_GENERIC: return "bf_user_ffbs_generic";
    case JIT_RTS_REGS: return variant == 2 ? "bf_user_rts_staged" : "bf_user_rts_strided";   // RTS_STAGED / RTS_STRIDED
    case JIT_FFBS_REGS: return variant == 1 ? "bf_user_ffbs_spl1" : variant == 2 ? "bf_user_ffbs_spl2" : variant == 4 ? "bf_user_ffbs_spl4" : "bf_user_ffbs_spl8";
    case JIT_GS_RTS_GENERIC: return "bf_user_gs_rts_generic";
    case JIT_GS_FFBS_GENERIC: return "bf_user_gs_ffbs_generic";
    case JIT_GS_FFBS_REGS: return "bf_user_gs_ffbs";
    case JIT_GS_RTS_REGS: return variant == 1 ? "bf_user_gs_rts_comp" : variant == 2 ? "bf_user_gs_rts_coll" : "bf_user_gs_rts_both";   // GS_COMP / GS_COLL / both
    case JIT_BPF: return "bf_user_bpf";
    case JIT_BPF_MISSING: return "bf_user_bpf_missing";
    case JIT_BPF_BIG_MISSING: return "bf_user_bpf_big_missing";
    case JIT_UGSF: return "bf_user_ugsf";
    case JIT_AGSF_UKF: case JIT_AGSF_EKF: return "bf_user_agsf";
    case JIT_GSF_REGS: return "bf_user_gsf_regs";
    case JIT_SAMPLE: return "bf_user_sample";
    case JIT_BPF_BIG: return "bf_user_bpf_big";
    case JIT_UGSF_GENERIC: return "bf_user_ugsf_generic";
    case JIT_GSF_GENERIC_MISSING: return "bf_user_scan_missing";
    default: return "bf_user_scan_64";
  }
}

std::string jit_source(const bf_user_model& um, int kind, int ppt, int nw, int spec_id) {
  if (kind == JIT_GSF_GENERIC) return generic_scan_source(um, 0);
  if (kind == JIT_UGSF_GENERIC) return generic_scan_source(um, 64 * nw);   // nw = 1: one wave per trajectory, 4: four
  if (kind == JIT_GSF_GENERIC_MISSING) return generic_scan_source(um, 0, 64 * nw);
  if (kind == JIT_RTS_GENERIC || kind == JIT_FFBS_GENERIC || kind == JIT_GS_RTS_GENERIC || kind == JIT_GS_FFBS_GENERIC) {
    // The run-time-dimension kernels of the smoother / the posterior sampler around the caller's dynamics: libm's float functions
    // under the dual numbers, as in JIT_GSF_GENERIC, whose streams they read; the kernel bodies are rts_generic.hpp's, with every
    // header they include in front (BF_JIT_FULL_HEADERS: generic_device.hpp then brings no helpers of its own).
    std::string s = "#define BF_JIT 1\n#define BF_JIT_FULL_HEADERS 1\n#include <cstdint>\n#include <type_traits>\n#define BF_USER_DYN 1\n";
    s += "#define BF_N " + std::to_string(um.n) + "\n#define BF_DQ " + std::to_string(um.dq) + "\n#define BF_M " + std::to_string(um.m) +
         "\n#define BF_DR " + std::to_string(um.dr) + "\n";
    s += kViewsSource;
    s += kSamplingSourceA;
    s += "#pragma clang fp contract(off)\nnamespace bfu {\n";
    s += kDualCore;
    s += kLibmMath;
    s += kDualMath;
    s += "\n// ---- the caller's dynamics\n" + um.dyn_src + "\n}  // namespace bfu\n";
    s += kSamplingSourceB;
    s += kUgsfSource;
    s += kRtsSource;
    s += kFfbsSource;
    s += kGenericDeviceSource;
    s += kUgsfGenericSource;
    s += kRtsGenericSource;
    if (kind == JIT_GS_FFBS_GENERIC)
      s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_gs_ffbs_generic(bf::FfbsGen c, bf::GenModel g, bf::FfbsViews v, long long T, bf::GsDraw gd) {\n"
           "  bf::ffbs_generic_body<false, true, true>(c, g, v, T, &gd);\n}\n";
    else if (kind == JIT_GS_RTS_GENERIC)
      s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_gs_rts_generic(bf::RtsGen c, bf::GenModel g, bf::RtsViews v, long long T, int K) {\n"
           "  bf::rts_generic_body<false, true, true>(c, g, v, T, K);\n}\n";
    else if (kind == JIT_RTS_GENERIC)
      s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_rts_generic(bf::RtsGen c, bf::GenModel g, bf::RtsViews v, long long T) {\n"
           "  bf::rts_generic_body<false, true>(c, g, v, T);\n}\n";
    else
      s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_ffbs_generic(bf::FfbsGen c, bf::GenModel g, bf::FfbsViews v, long long T) {\n"
           "  bf::ffbs_generic_body<false, true>(c, g, v, T);\n}\n";
    return s;
  }
  if (kind == JIT_RTS_REGS || kind == JIT_FFBS_REGS || kind == JIT_GS_RTS_REGS || kind == JIT_GS_FFBS_REGS) {
    // The register kernels of the smoother / the posterior sampler around the caller's dynamics (RTS_EXT_USER), assembled as
    // JIT_GSF_REGS is: the caller's function sees the float functions of the register filter that produced the streams.  The
    // emission is not read by a backward pass and is left out.  One module holds every data path / samples-per-lane count.
    std::string s = "#define BF_JIT 1\n#include <cstdint>\n#include <type_traits>\n#define BF_USER_DYN 1\n";
    s += "#define BF_N " + std::to_string(um.n) + "\n#define BF_DQ " + std::to_string(um.dq) + "\n#define BF_M " + std::to_string(um.m) +
         "\n#define BF_DR " + std::to_string(um.dr) + "\n";
    s += kViewsSource;
    s += kSamplingSourceA;
    s += kSamplingUserMath;
    s += kDualCore;
    s += kDualMath;
    s += "\n// ---- the caller's dynamics\n" + um.dyn_src + "\n}  // namespace bfu\n";
    s += kSamplingSourceB;
    s += kUgsfSource;
    s += kRtsSource;
    if (kind == JIT_GS_RTS_REGS) {  // the Gaussian-sum smoother: one entry point per output set
      for (int out : {1, 2, 3})
        s += std::string("extern \"C\" __global__ void __launch_bounds__(64) ") + jit_entry_name(kind, out) +
             "(bf::RtsUser<BF_DQ> c, bf::RtsGsViews gv, long long B, long long T) {\n  bf::rts_gs_reg_body<BF_N, bf::RTS_EXT_USER, " +
             std::to_string(out) + ">(c, gv, B, T);\n}\n";
      return s;
    }
    if (kind == JIT_RTS_REGS) {
      for (int mode : {0, 2})
        s += std::string("extern \"C\" __global__ void __launch_bounds__(64) ") + jit_entry_name(kind, mode) +
             "(bf::RtsUser<BF_DQ> c, bf::RtsViews v, long long B, long long T) {\n  bf::rts_reg_body<BF_N, " + std::to_string(mode) +
             ", bf::RTS_EXT_USER>(c, nullptr, v, B, T);\n}\n";
      return s;
    }
    s += kFfbsSource;
    if (kind == JIT_GS_FFBS_REGS) {  // the Gaussian-sum sampler: one lane per (trajectory, sample)
      s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_gs_ffbs(bf::RtsUser<BF_DQ> c, bf::FfbsViews v, bf::GsDraw gd, long long B, long long T, int S) {\n"
           "  bf::ffbs_reg_body<BF_N, 1, bf::RTS_EXT_USER, bf::RtsUser<BF_DQ>, true>(c, nullptr, v, B, T, S, &gd);\n}\n";
      return s;
    }
    for (int spl : {1, 2, 4, 8})
      s += std::string("extern \"C\" __global__ void __launch_bounds__(64) ") + jit_entry_name(kind, spl) +
           "(bf::RtsUser<BF_DQ> c, bf::FfbsViews v, long long B, long long T, int S) {\n  bf::ffbs_reg_body<BF_N, " + std::to_string(spl) +
           ", bf::RTS_EXT_USER>(c, nullptr, v, B, T, S);\n}\n";
    return s;
  }
  std::string s = "#define BF_JIT 1\n#include <cstdint>\n#include <type_traits>\n";
  if (um.hw_arith) s += "#define BF_BPF_HW_ARITH 1\n";
  if (um.has_dyn) s += "#define BF_USER_DYN 1\n";
  if (um.has_emi) s += "#define BF_USER_EMI 1\n";
  if (um.has_lp) s += "#define BF_USER_LP 1\n";
  s += "#define BF_N " + std::to_string(um.n) + "\n#define BF_DQ " + std::to_string(um.dq) + "\n#define BF_M " + std::to_string(um.m) +
       "\n#define BF_DR " + std::to_string(um.dr) + "\n";
  s += kViewsSource;
  if (kind == JIT_AGSF_EKF || kind == JIT_GSF_REGS) s += "#define BF_USER_EKF_NODES 1\n";
  s += kSamplingSourceA;
  s += kSamplingUserMath;
  if (kind == JIT_AGSF_EKF || kind == JIT_GSF_REGS) {  // the Jacobians of the extended-Kalman nodes: dual numbers over the same float functions
    s += kDualCore;
    s += kDualMath;
  }
  s += "\n// ---- the caller's functions\n";
  if (um.has_dyn) s += um.dyn_src + "\n";
  if (um.has_emi) s += um.emi_src + "\n";
  if (um.has_lp) s += um.lp_src + "\n";
  s += "}  // namespace bfu\n";
  s += kSamplingSourceB;
  // the model structure: the handle's own functions, or (registry models) a spec of bpf_scan.hpp
  const std::string spec = spec_id == JIT_SPEC_L96_PICK ? "bf::SpecFixed<bf::DYN_LORENZ96, bf::EMI_LINEAR, true, true, true, true>"
                           : spec_id == JIT_SPEC_RUNTIME ? "bf::SpecRuntime"
                                                         : std::string("bf::SpecUser<") + (um.has_dyn ? "true" : "false") + ", " +
                                                               (um.has_emi ? "true" : "false") + ", " + (um.has_lp ? "true" : "false") + ">";
  if (kind == JIT_AGSF_UKF || kind == JIT_AGSF_EKF) {
    s += kUgsfSource;
    s += kAgsfSource;
    const std::string nodes = kind == JIT_AGSF_UKF ? "bf::UkfNodes<BF_N, BF_DQ, BF_M, BF_DR, " + spec + ">" : "bf::UserEkfNodes<BF_N, BF_DQ, BF_M, BF_DR, " + spec + ">";
    s += "extern \"C\" __global__ void __launch_bounds__(" + std::to_string(nw == 1 ? 256 : 64 * nw) + ") bf_user_agsf(const bf::UkfModel<BF_N, BF_DQ, BF_M, BF_DR>* "
         "__restrict__ mdlp, bf::CView y, bf::UView uin, bf::CarryView carry, bf::AgsfOut out, long long B, long long T, int N0, int N1, int N2, int MP, "
         "float a0, float a1, uint32_t key0, uint32_t key1, int variant, int carry_records, const float* __restrict__ tvq, const float* __restrict__ tvr) {\n"
         "  bf::agsf_scan_body<BF_N, BF_M, " + nodes + ", " + std::to_string(nw) + ">(mdlp, y, uin, carry, out, B, T, N0, N1, N2, MP, a0, a1, key0, key1, "
         "variant, carry_records, tvq, tvr);\n}\n";
    return s;
  }
  if (kind == JIT_BPF_BIG || kind == JIT_BPF_BIG_MISSING) {   // the particle filter with the particles in HBM (bpf_big.hpp): up to 2^20 particles per trajectory
    s += kBpfBigSource;
    s += std::string("extern \"C\" __global__ void __launch_bounds__(1024) ") + jit_entry_name(kind) + "(const bf::BpfModel<BF_N, BF_DQ, BF_M>* __restrict__ mdlp, bf::CView y, "
         "const float* __restrict__ uptr, long long u_sB, long long u_sT, bf::BpfCarry carry, bf::BpfOut out, bf::BigScratch sc, long long B, long long T, "
         "int NP, float ess_threshold, int resampler, uint32_t key0, uint32_t key1) {\n  bf::bpf_big_body<BF_N, BF_DQ, BF_M, " + spec +
         (kind == JIT_BPF_BIG_MISSING ? ", true" : "") + ">(mdlp, y, uptr, u_sB, u_sT, carry, out, sc, B, T, NP, ess_threshold, resampler, key0, key1);\n}\n";
    return s;
  }
  if (kind == JIT_SAMPLE) {   // NonlinearSSM.sample with the caller's functions (sample_ssm.hpp), a lane per trajectory
    s += kSampleSource;
    s += "extern \"C\" __global__ void __launch_bounds__(64) bf_user_sample(const bf::BpfModel<BF_N, BF_DQ, BF_M>* __restrict__ mdlp, "
         "const bf::EmissionNoise<BF_M>* __restrict__ enp, const uint32_t* __restrict__ keys, const float* __restrict__ uptr, long long u_sB, long long u_sT, "
         "float* __restrict__ states, float* __restrict__ emis, long long B, long long T) {\n  bf::sample_ssm_body<BF_N, BF_DQ, BF_M, " + spec +
         ">(mdlp, enp, keys, uptr, u_sB, u_sT, states, emis, B, T);\n}\n";
    return s;
  }
  // (ppt = 1 for the two Gaussian-sum scans: the MISSING = true twin, NaN observations are gaps)
  if (kind == JIT_GSF_REGS) {   // the Gaussian-sum scan with extended-Kalman operations, one lane per (trajectory, component)
    s += kUgsfSource;
    s += "extern \"C\" __global__ void __launch_bounds__(256) bf_user_gsf_regs(const bf::UkfModel<BF_N, BF_DQ, BF_M, BF_DR>* __restrict__ mdlp, bf::CView y, "
         "const float* __restrict__ uptr, long long u_sB, long long u_sT, bf::CarryView carry, bf::OutViews out, long long B, long long T, int K, int KP, "
         "const float* __restrict__ tvq, const float* __restrict__ tvr) {\n  bf::ugsf_scan_body<BF_N, BF_DQ, BF_M, BF_DR, " + spec +
         ", bf::UserEkfNodes<BF_N, BF_DQ, BF_M, BF_DR, " + spec + ">" + (ppt == 1 ? ", true" : "") + ">(mdlp, y, uptr, u_sB, u_sT, carry, out, B, T, K, KP, tvq, tvr);\n}\n";
    return s;
  }
  if (kind == JIT_UGSF) {
    s += kUgsfSource;
    s += "extern \"C\" __global__ void __launch_bounds__(256) bf_user_ugsf(const bf::UkfModel<BF_N, BF_DQ, BF_M, BF_DR>* __restrict__ mdlp, bf::CView y, "
         "const float* __restrict__ uptr, long long u_sB, long long u_sT, bf::CarryView carry, bf::OutViews out, long long B, long long T, int K, int KP, "
         "const float* __restrict__ tvsq, const float* __restrict__ tvsr) {\n  bf::ugsf_scan_body<BF_N, BF_DQ, BF_M, BF_DR, " + spec +
         (ppt == 1 ? ", void, true" : "") + ">(mdlp, y, uptr, u_sB, u_sT, carry, out, B, T, K, KP, tvsq, tvsr);\n}\n";
    return s;
  }
  // (JIT_BPF or its MISSING = true twin)
  s += "extern \"C\" __global__ void __launch_bounds__(" + std::to_string(64 * nw) + ") " + jit_entry_name(kind) + "(const bf::BpfModel<BF_N, BF_DQ, BF_M>* __restrict__ mdlp, "
       "const bf::BpfArgs<BF_N, BF_DQ, BF_M> args_by_value) {\n  (void)args_by_value;\n  bf::bpf_scan_body<BF_N, BF_DQ, BF_M, " +
       std::to_string(ppt) + ", " + std::to_string(nw) + ", " + spec + (kind == JIT_BPF_MISSING ? ", true" : "") + ">(mdlp);\n}\n";
  return s;
}

}  // namespace bf
