// Element receivers: what each element of a transducer array receives after a time step -- the surface integral of the field over
// the element's face,  S_e = sum_k wgt[k] u[dof[k]]  over the element's entries k in [offsets[e], offsets[e + 1]).  The host sorts the
// facet-dof entries of the receiving facets by element into ONE list with CSR offsets (receivers.ElementReceivers); ``wgt`` is the scaled
// facet detJ the solvers already hold, so S_e is the GLL quadrature of  int_{Gamma_e} u dS.  Nothing is normalised here: a partitioned
// rank holds a partial integral and a partial area, and those must ADD before the host divides (receivers.merge).
//
// Outputs, each optional (null = off), of the value rounded to T (so that the harmonics are those of the recorded series):
//   rec[slot][e]                                            T      the time series row
//   hre[h][e] += S_e coef[2h],  him[h][e] += S_e coef[2h + 1]   double, h < H   (coef: this step's cos / sin factors, device memory)
// No peaks: the peak of a sum over ranks is not a sum of peaks.
//
// One workgroup of four waves per element: each lane strides the element's entries (a one-element array -- a whole face, ~75 k entries
// at config 3 -- is 256 lanes deep, never one), accumulates in double, the wave reduces by shuffles, the four wave partials meet in LDS
// and lane 0 adds them in a fixed order and writes.  No atomics anywhere: two runs give the same bits.  An element without entries on
// this rank writes 0 (and accumulates nothing).  32 bytes of LDS, no scratch, at most 64 VGPRs (tests/test_receivers.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fus {

constexpr int kReceiveThreads = 256;
constexpr int kReceiveWaves = kReceiveThreads / 64;

template <typename T>
__global__ void __launch_bounds__(kReceiveThreads, 8)
    element_receive_kernel(const T* __restrict__ u, const int32_t* __restrict__ dof, const T* __restrict__ wgt,
                           const int64_t* __restrict__ offsets, int64_t nelem, T* __restrict__ rec, double* __restrict__ hre,
                           double* __restrict__ him, const double* __restrict__ coef, int H) {
  __shared__ double part[kReceiveWaves];
  const int64_t e = blockIdx.x;
  const int64_t end = offsets[e + 1];
  // four independent partial sums per lane: four gathers in flight instead of one dependent chain (a whole face in ONE element is
  // ~285 entries per lane, latency-bound otherwise); they are added in a fixed order, so the result stays reproducible
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t k = offsets[e] + threadIdx.x;
  for (; k + 3 * kReceiveThreads < end; k += 4 * kReceiveThreads) {
    a0 += (double)wgt[k] * (double)u[dof[k]];
    a1 += (double)wgt[k + kReceiveThreads] * (double)u[dof[k + kReceiveThreads]];
    a2 += (double)wgt[k + 2 * kReceiveThreads] * (double)u[dof[k + 2 * kReceiveThreads]];
    a3 += (double)wgt[k + 3 * kReceiveThreads] * (double)u[dof[k + 3 * kReceiveThreads]];
  }
  for (; k < end; k += kReceiveThreads) a0 += (double)wgt[k] * (double)u[dof[k]];
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = part[0];
#pragma unroll
  for (int i = 1; i < kReceiveWaves; ++i) sum += part[i];
  const T vt = (T)sum;
  const double v = (double)vt;
  if (rec) rec[e] = vt;  // rec already points at row ``slot``
  for (int h = 0; h < H; ++h) {
    hre[h * nelem + e] += v * coef[2 * h];
    him[h * nelem + e] += v * coef[2 * h + 1];
  }
}

// nelem == 0: no launch
template <typename T>
inline hipError_t launch_element_receive(const T* u, const int32_t* dof, const T* wgt, const int64_t* offsets, int64_t nelem, T* rec,
                                         double* hre, double* him, const double* coef, int H, hipStream_t stream) {
  if (nelem <= 0) return hipSuccess;
  hipLaunchKernelGGL((element_receive_kernel<T>), dim3((unsigned)nelem), dim3(kReceiveThreads), 0, stream, u, dof, wgt, offsets, nelem, rec,
                     hre, him, coef, H);
  return hipGetLastError();
}

}  // namespace fus
