// Stand-alone check of include/fus_gpu.hpp (host side only: no GPU, no library to link): every functor class of the header is
// instantiated explicitly, which compiles ALL its members, for double and float and, where the degree is a template parameter, for
// every degree of [FUS_MIN_DEGREE, FUS_MAX_DEGREE] = 1 ... 10: twelve classes, two types, ten degrees.  A forward whose arguments do not match the
// prototype of include/fus_gpu.h, in either scalar type, is then a compile error here instead of waiting for the first user.
// tests/test_fus_gpu_hpp_host.py compiles it with hipcc, host pass only, -Wall -Wextra -Werror.  Prints FUS_GPU_HPP_OK.
#include "../../include/fus_gpu.hpp"

#include <cstdio>

#define FUS_CHECK_DEGREES(X, T) \
  template class fus_gpu::X<T, 1>; \
  template class fus_gpu::X<T, 2>; \
  template class fus_gpu::X<T, 3>; \
  template class fus_gpu::X<T, 4>; \
  template class fus_gpu::X<T, 5>; \
  template class fus_gpu::X<T, 6>; \
  template class fus_gpu::X<T, 7>; \
  template class fus_gpu::X<T, 8>; \
  template class fus_gpu::X<T, 9>; \
  template class fus_gpu::X<T, 10>;
#define FUS_CHECK_TYPE(T) \
  template struct fus_gpu::Geometry<T>; \
  FUS_CHECK_DEGREES(MassSpectral3D, T) \
  FUS_CHECK_DEGREES(StiffnessSpectral3D, T) \
  FUS_CHECK_DEGREES(GradientSpectral3D, T) \
  FUS_CHECK_DEGREES(NodalStiffnessSpectral3D, T) \
  FUS_CHECK_DEGREES(WesterveltNodalStiffnessSpectral3D, T) \
  FUS_CHECK_DEGREES(PointProbe, T) \
  FUS_CHECK_DEGREES(PointSource, T) \
  template class fus_gpu::FieldAccumulator<T>; \
  template class fus_gpu::BioheatStage<T>; \
  template class fus_gpu::FacetSourceArray<T>; \
  template class fus_gpu::ElementReceive<T>; \
  template class fus_gpu::RelaxStage<T>;

FUS_CHECK_TYPE(double)
FUS_CHECK_TYPE(float)

int main() {
  std::printf("FUS_GPU_HPP_OK\n");
  return 0;
}
