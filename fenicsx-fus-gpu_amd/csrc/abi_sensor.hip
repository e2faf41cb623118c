// libfusgpu.so -- the shock-capturing part of the C ABI (include/fus_gpu_sensor.h: fus_modal_sensor_*) over modal_sensor.hpp.  A
// translation unit of its own: of the operator kernels it shares only the launch shape helpers of stiffness.hpp.
#include "../../include/fus_gpu_sensor.h"

#include <hip/hip_runtime.h>

#include "modal_sensor.hpp"

static_assert(FUS_MIN_DEGREE == 1 && FUS_MAX_DEGREE == 10, "modal_sensor lists the supported degrees");
static_assert(fus::kSensorQuiet == (double)FUS_SENSOR_QUIET, "the header documents the sentinel the kernel stores");

namespace {

template <typename T>
int modal_sensor(const T* u, const int32_t* dofmap, const T* Vinv, const T* cc4_base, const T* scale, const double* eps_max, double* eps,
                 double* sensor, T* cc4, int P, int64_t ncell, double s0, double kappa, double floor, double hold, void* stream) {
  if (ncell < 0) return FUS_ERR_INVALID_ARGUMENT;
  if (P < FUS_MIN_DEGREE || P > FUS_MAX_DEGREE) return FUS_ERR_UNSUPPORTED_DEGREE;
  if (!(kappa > 0.0) || !(floor >= 0.0) || !(hold >= 0.0 && hold <= 1.0) || s0 != s0) return FUS_ERR_INVALID_ARGUMENT;
  if (ncell == 0) return FUS_OK;
  if (!u || !dofmap || !Vinv || !cc4_base || !scale || !eps_max || !eps || !sensor || !cc4) return FUS_ERR_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipErrorInvalidValue;
#define FUS_SENSOR_CASE(PP)                                                                                                          \
  case PP:                                                                                                                           \
    e = fus::launch_modal_sensor<T, PP>(u, dofmap, Vinv, cc4_base, scale, eps_max, eps, sensor, cc4, ncell, s0, kappa, floor, hold, s); \
    break;
  switch (P) {
    FUS_SENSOR_CASE(1)
    FUS_SENSOR_CASE(2)
    FUS_SENSOR_CASE(3)
    FUS_SENSOR_CASE(4)
    FUS_SENSOR_CASE(5)
    FUS_SENSOR_CASE(6)
    FUS_SENSOR_CASE(7)
    FUS_SENSOR_CASE(8)
    FUS_SENSOR_CASE(9)
    FUS_SENSOR_CASE(10)
  }
#undef FUS_SENSOR_CASE
  return e == hipSuccess ? FUS_OK : FUS_ERR_HIP_BASE - (int)e;
}

}  // namespace

extern "C" {

int fus_modal_sensor_f64(const double* u, const int32_t* dofmap, const double* Vinv, const double* cc4_base, const double* scale,
                         const double* eps_max, double* eps, double* sensor, double* cc4, int P, int64_t ncell, double s0, double kappa,
                         double floor, double hold, void* stream) {
  return modal_sensor<double>(u, dofmap, Vinv, cc4_base, scale, eps_max, eps, sensor, cc4, P, ncell, s0, kappa, floor, hold, stream);
}
int fus_modal_sensor_f32(const float* u, const int32_t* dofmap, const float* Vinv, const float* cc4_base, const float* scale,
                         const double* eps_max, double* eps, double* sensor, float* cc4, int P, int64_t ncell, double s0, double kappa,
                         double floor, double hold, void* stream) {
  return modal_sensor<float>(u, dofmap, Vinv, cc4_base, scale, eps_max, eps, sensor, cc4, P, ncell, s0, kappa, floor, hold, stream);
}

}  // extern "C"
