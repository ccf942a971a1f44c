// kf_scan_bf32_missing: the MISSING = true twins of the one-wave matrix-core Kalman kernel's eight instances (kf_scan_bf32.hpp),
// where a NaN observation is a component that was not observed at that step.  They live in a translation unit of their own so
// that the plain instances of kf_scan_bf32.hip are compiled exactly as before; launch_kf_bf32 (there) packs the model, the
// tables and the views for both and calls this with `missing`.
#include "kf_scan_bf32.hpp"

namespace bf {

hipError_t bf32_launch_missing(const Bf32Args& a, bool multi, int dyn_kind, hipStream_t stream) {
  return bf32_launch_instance<true>(a, multi, dyn_kind, stream);
}

}  // namespace bf
