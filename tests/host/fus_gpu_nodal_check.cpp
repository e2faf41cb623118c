// Host-only compile check of the nodal stiffness functor of include/fus_gpu.hpp (tests/test_nodal.py): explicit instantiation for both
// scalar types, so the typed forward is checked against its prototype in include/fus_gpu_nodal.h.
#include "../../include/fus_gpu.hpp"

template class fus_gpu::NodalStiffnessSpectral3D<double, 1>;
template class fus_gpu::NodalStiffnessSpectral3D<double, 4>;
template class fus_gpu::NodalStiffnessSpectral3D<double, 10>;
template class fus_gpu::NodalStiffnessSpectral3D<float, 1>;
template class fus_gpu::NodalStiffnessSpectral3D<float, 4>;
template class fus_gpu::NodalStiffnessSpectral3D<float, 10>;
