// generic_scan_missing: the MISSING = true instances of the run-time-dimension scan (generic_device.hpp: gsf_generic_body), where a
// NaN observation is a component that was not observed at that step.  They live in a translation unit of their own so that the
// plain instances of generic_scan.hip are compiled exactly as before; launch_gsf_generic (there) prepares the model, the LDS size
// and the views for both and calls this with `missing`.
#include "forward_host.hpp"
#include "kf_math.hpp"
#include "scan_common.hpp"
#include "models.hpp"
#include "generic_device.hpp"

namespace bf {

template <int NT>
static int launch_missing(unsigned grid, size_t lds_bytes, hipStream_t stream, const GenModel& g, const ForwardViews& v, UViewG uv,
                          float* gm, float* gP, long long B, long long T, int K, int KP) {
  auto kern = gsf_generic_kernel<NT, true>;
  if (lds_bytes > 64 * 1024)
    BF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, stream, g, v.y, uv, v.carry, v.out, gm, gP, B, T, K, KP);
  BF_HIP_CHECK(hipGetLastError());
  return BF_OK;
}

int launch_gsf_generic_missing_kernel(int nt, unsigned grid, size_t lds_bytes, hipStream_t stream, const GenModel& g, const ForwardViews& v,
                                      UViewG uv, float* gm, float* gP, long long B, long long T, int K, int KP) {
  return nt == 64 ? launch_missing<64>(grid, lds_bytes, stream, g, v, uv, gm, gP, B, T, K, KP)
                  : launch_missing<256>(grid, lds_bytes, stream, g, v, uv, gm, gP, B, T, K, KP);
}

}  // namespace bf
