// Host-only compile check of include/fus_gpu.hpp's WesterveltNodalStiffnessSpectral3D (tests/test_westervelt_nodal.py): the typed
// forward against the prototypes of include/fus_gpu_westervelt_nodal.h, both scalar types, the lowest, a middle and the highest degree.
#include "../../include/fus_gpu.hpp"

template class fus_gpu::WesterveltNodalStiffnessSpectral3D<double, 1>;
template class fus_gpu::WesterveltNodalStiffnessSpectral3D<double, 4>;
template class fus_gpu::WesterveltNodalStiffnessSpectral3D<double, 10>;
template class fus_gpu::WesterveltNodalStiffnessSpectral3D<float, 1>;
template class fus_gpu::WesterveltNodalStiffnessSpectral3D<float, 4>;
template class fus_gpu::WesterveltNodalStiffnessSpectral3D<float, 10>;
