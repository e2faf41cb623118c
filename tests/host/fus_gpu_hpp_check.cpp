// Stand-alone check of include/fus_gpu.hpp (host side only: no GPU, no library to link): every functor class of the header is
// instantiated explicitly, which compiles ALL its members, for double and float and, where the degree is a template parameter, for
// P = 1, 4 and 10 (the edges of [FUS_MIN_DEGREE, FUS_MAX_DEGREE] and the headline degree).  A forward whose arguments do not match the
// prototype of include/fus_gpu.h, in either scalar type, is then a compile error here instead of waiting for the first user.
// tests/test_fus_gpu_hpp_host.py compiles it with hipcc, host pass only, -Wall -Wextra -Werror.  Prints FUS_GPU_HPP_OK.
#include "../../include/fus_gpu.hpp"

#include <cstdio>

#define FUS_CHECK_DEGREES(X, T) \
  template class fus_gpu::X<T, 1>; \
  template class fus_gpu::X<T, 4>; \
  template class fus_gpu::X<T, 10>;
#define FUS_CHECK_TYPE(T) \
  template struct fus_gpu::Geometry<T>; \
  FUS_CHECK_DEGREES(MassSpectral3D, T) \
  FUS_CHECK_DEGREES(StiffnessSpectral3D, T) \
  FUS_CHECK_DEGREES(GradientSpectral3D, T) \
  FUS_CHECK_DEGREES(PointProbe, T) \
  template class fus_gpu::FieldAccumulator<T>; \
  template class fus_gpu::BioheatStage<T>; \
  template class fus_gpu::FacetSourceArray<T>;

FUS_CHECK_TYPE(double)
FUS_CHECK_TYPE(float)

int main() {
  std::printf("FUS_GPU_HPP_OK\n");
  return 0;
}
