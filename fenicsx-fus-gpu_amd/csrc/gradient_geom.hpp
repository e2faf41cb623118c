// Planned weak gradient C(c) u with the geometry formed IN THE KERNEL from the cell's 8 vertices: three vectors, d = 0, 1, 2,
//   y_d[i] += sum_cells c_cell  sum_{q : dof(cell, q) = i}  w_q |det J_q| (du/dx_d)(q),     du/dx_d = sum_a inv(J_)[d][a] du/dxi_a
// Conventions of stiffness_geom.hpp (J_[a][d] = dx_d / dxi_a, trilinear 8-vertex cells, the tensor GLL rule q = qx n^2 + qy n + qz,
// w_q |det| as the weight).  With a, b, c the columns of adj(J_) (column_flux_at) and inv(J_) = adj / det,
//   w_q |det| grad u = w_q sign(det) (a vx + b vy + c vz)
// with (vx, vy, vz) of plan_grad_at: no reciprocal, no G, no flux cube, and -- the GLL points are the nodes -- no backward
// contraction: the n quadrature points along a thread's column are its own n dofs (sl[qx]).  A lighter sibling of
// stiffness_plan_geom_kernel: the same two-round-trip preamble (plan.hpp) from the same helpers, the same u cube; the three
// components are pre-reduced in LDS (PlanAcc, also for fp32 fields) and leave with one hardware atomic per distinct dof and component.
//
// LDS: the u cube must stay readable until the last plan_grad_at; the two flux cubes of the stiffness kernel do not exist.  Two builds
// of the accumulators (ONEACC), chosen per scalar type and degree by what tools/resource_usage.py reports (gradient_single_accumulator;
// DESIGN 3.10 has the table):
//   three at once        3 M doubles in place of the flux cubes (the x values of the gather live in the first until the u cube is
//                        written); one pass over the quadrature points, four barriers in all -- but more LDS than the stiffness
//                        kernel, which costs fp64 P = 4, 6, 7, 10 and every fp32 degree a wave per SIMD or more;
//   one, reused          M doubles; the x component is pre-reduced in the loop, the y and z components wait in 2 n registers for a
//                        pass of their own (flush + zero by the owner of a slot, barrier, ds_add, barrier): four more barriers,
//                        less LDS than the stiffness kernel and never fewer waves per SIMD than it.
#pragma once

#include "stiffness_geom.hpp"

namespace fus {

// w_q sign(det) c (a vx + b vy + c vz) at quadrature plane qx of the column: ``wx_s0`` = cell constant * w_x * w_y * w_z.
// Same rows of J_ and the same columns of adj(J_) as column_flux_at.
template <typename T>
__device__ __forceinline__ void column_wgrad_at(T ex, T wx_s0, const T (&J0)[3], const T (&Ja)[3], const T (&Jba)[3], const T (&Jc)[3],
                                                const T (&Jdc)[3], T vx, T vy, T vz, T (&r)[3]) {
  T J1[3], J2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    J1[d] = Ja[d] + ex * Jba[d];
    J2[d] = Jc[d] + ex * Jdc[d];
  }
  T a[3], b[3], c[3];
  a[0] = J1[1] * J2[2] - J1[2] * J2[1];
  a[1] = J1[2] * J2[0] - J1[0] * J2[2];
  a[2] = J1[0] * J2[1] - J1[1] * J2[0];
  b[0] = J0[2] * J2[1] - J0[1] * J2[2];
  b[1] = J0[0] * J2[2] - J0[2] * J2[0];
  b[2] = J0[1] * J2[0] - J0[0] * J2[1];
  c[0] = J0[1] * J1[2] - J0[2] * J1[1];
  c[1] = J0[2] * J1[0] - J0[0] * J1[2];
  c[2] = J0[0] * J1[1] - J0[1] * J1[0];
  const T det = J0[0] * a[0] + J0[1] * a[1] + J0[2] * a[2];
  const T s = det < T(0) ? -wx_s0 : wx_s0;
#pragma unroll
  for (int d = 0; d < 3; ++d) r[d] = s * (a[d] * vx + b[d] * vy + c[d] * vz);
}

// ONEACC per scalar type and degree: the single accumulator wherever it reaches more waves per SIMD than three at once (without scratch:
// fp64 P = 8 would spill 36 bytes with it and gains nothing), the three accumulators -- fewer barriers -- where the occupancy is the same.
template <typename T, int P>
__host__ __device__ constexpr bool gradient_single_accumulator() {
  return sizeof(T) == 4 || P == 4 || P == 6 || P == 7 || P == 10;
}

// y: T[3][ystride], component d at y + d * ystride (ystride >= number of dofs, in elements); contributions are added.
template <typename T, int P, int CPB, bool PADLDS, bool ONEACC, bool ORDERED, bool RUNS>
__global__ void __launch_bounds__((col_block_threads<P, CPB>()), 1)
    gradient_plan_geom_kernel(const T* __restrict__ x, const T* __restrict__ cell_constants, T* __restrict__ y, int64_t ystride,
                              const T* __restrict__ x_g, const int32_t* __restrict__ x_dofs, const T* __restrict__ pts,
                              const T* __restrict__ wts, const int32_t* __restrict__ nu, const int32_t* __restrict__ udofs,
                              const uint16_t* __restrict__ slot, const T* __restrict__ dphi, int64_t ncell,
                              const int32_t* __restrict__ order, const int32_t* __restrict__ runs, LaunchSignal sig) {
  using Sh = PlanShape<T, P, CPB, PADLDS>;
  constexpr int n = Sh::n, n2 = Sh::n2, Nd = Sh::Nd, S = Sh::S, BLOCK = Sh::BLOCK, M = Sh::M, SPT = Sh::SPT;
  launch_signal_publish(sig);
  constexpr int VPT = (CPB * 24 + BLOCK - 1) / BLOCK;  // vertex coordinates staged per thread (1 for P >= 4)

  __shared__ T sD[n2 + 1];  // + 1: plan_table_store
  __shared__ T sP[n + 1], sW[n + 1];
  __shared__ T sX[CPB * 24];
  __shared__ T su[CPB * S];
  __shared__ PlanAcc sacc[(ONEACC ? 1 : 3) * M];  // the partial sums of the three components (ONEACC: of one at a time)
  T* const sx = reinterpret_cast<T*>(sacc);   // x values of the batch's distinct dofs: dead once the u cube is written

  const int tid = threadIdx.x;
  const unsigned batch = blockIdx.x;
  const int lc = tid / n2;
  const int t = tid - lc * n2;
  const int ty = t / n, tz = t - ty * n;
  const int64_t cell0 = (int64_t)batch * CPB;
  const int64_t pos = cell0 + lc;  // position in the plan's cell order
  const bool active = (lc < CPB) && (pos < ncell);
  const int32_t* ud = udofs + (int64_t)batch * M;
  const int32_t* rn = runs + (int64_t)batch * (2 * kPlanMaxRuns);  // read only when RUNS

  // ---- round trip 1: everything that depends on the kernel arguments alone (the rules: plan.hpp, "the preamble every planned
  // kernel shares")
  const int64_t pos_ld = plan_load_pos<CPB>(cell0, lc, ncell);
  const uint32_t row = plan_row_issue<ORDERED>(order, pos_ld);
  const T dval = dphi[tid < n2 ? tid : 0];
  const T pval = pts[tid < n ? tid : 0];
  const T wval = wts[tid < n ? tid : 0];
  int32_t mydof[SPT];
  const RunWords rt = batch_dofs_issue<RUNS, SPT, BLOCK>(ud, rn, M, tid, mydof);
  int32_t vid[VPT];
  stage_vertex_ids<ORDERED, VPT, BLOCK, CPB>(x_dofs, order, cell0, ncell, tid, vid);
  uint16_t sl[n];
  if (plan_loads_by_all<n>() || active) {
    const uint16_t* sp = slot + pos_ld * Nd + t;
#pragma unroll
    for (int ix = 0; ix < n; ++ix) sl[ix] = sp[ix * n2];
  }
  // ---- round trip 2: what those point to -- (ORDERED: vertex ids and the cell's constant;) x and the vertex coordinates
  stage_vertex_ids_of_rows<ORDERED, VPT, BLOCK, CPB>(x_dofs, tid, vid);
  T coeff = T(0);
  if (plan_loads_by_all<n>() || active) coeff = cell_constants[plan_row<ORDERED>(row, pos_ld)];
  const int packed = nu[batch];
  const int nu_b = packed & 0xffff, nr_b = plan_runs_of<RUNS>(packed);
  plan_table_store<n, n2>(sD, tid, dval);
  plan_table_store<n, n>(sP, tid, pval);
  plan_table_store<n, n>(sW, tid, wval);
  batch_dofs_resolve<RUNS, SPT, BLOCK>(rt, ud, M, nu_b, nr_b, tid, reinterpret_cast<int32_t*>(su), mydof);

  // ---- gather x with the vertex coordinates (as stiffness_plan_geom_kernel)
  {
    T xv[SPT];
#pragma unroll
    for (int r = 0; r < SPT; ++r) xv[r] = x[mydof[r]];
    T cv[VPT];
    stage_vertex_coords_issue<T, VPT, BLOCK, CPB>(x_g, vid, tid, cv);
#pragma unroll
    for (int r = 0; r < SPT; ++r) {
      const int s = tid + r * BLOCK;
      if (s < nu_b) sx[s] = xv[r];
    }
    stage_vertex_coords_store<T, VPT, BLOCK, CPB>(cv, tid, sX);
  }
  __syncthreads();  // x values and vertex coordinates are in LDS

  T J0[3], Ja[3], Jba[3], Jc[3], Jdc[3];
  T s0 = T(0);
  T u[n];
  if (active) {
    column_jacobian_rows<T>(sX + lc * 24, sP[ty], sP[tz], J0, Ja, Jba, Jc, Jdc);
    s0 = coeff * sW[ty] * sW[tz];
    T* cu = su + lc * S + t;
#pragma unroll
    for (int ix = 0; ix < n; ++ix) {
      u[ix] = sx[sl[ix]];
      cu[ix * n2] = u[ix];
    }
  }
  __syncthreads();  // the u cube is readable; the x values are dead: their region becomes the first accumulator
#pragma unroll
  for (int d = 0; d < (ONEACC ? 1 : 3); ++d) plan_zero<T, SPT, BLOCK>(sacc + d * M, nu_b, tid);
  __syncthreads();

  T r1[ONEACC ? n : 1], r2[ONEACC ? n : 1];  // ONEACC: the y and z components of the column wait in registers for their pass
  if (active) {
    T dy[n], dz[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      dy[i] = sD[ty * n + i];
      dz[i] = sD[tz * n + i];
    }
    const T* cu_y = su + lc * S + tz;
    const T* cu_z = su + lc * S + ty * n;
#pragma unroll
    for (int qx = 0; qx < n; ++qx) {
      T vx, vy, vz;
      plan_grad_at<T, n, n2>(qx, dphi, u, dy, dz, cu_y, cu_z, vx, vy, vz);
      T r[3];
      column_wgrad_at<T>(pts[qx], wts[qx] * s0, J0, Ja, Jba, Jc, Jdc, vx, vy, vz, r);  // pts / wts with compile-time indices: scalar loads
      if constexpr (ONEACC) {
        lds_atomic_add(&sacc[sl[qx]], (PlanAcc)r[0]);
        r1[qx] = r[1];
        r2[qx] = r[2];
      } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) lds_atomic_add(&sacc[d * M + sl[qx]], (PlanAcc)r[d]);
      }
    }
  }
  __syncthreads();
  if constexpr (ONEACC) {
    // a thread flushes and zeroes the slots it owns (the same ones in plan_flush and plan_zero): no barrier between the two
    plan_flush<T, SPT, BLOCK>(y, mydof, nu_b, tid, sacc);
    plan_zero<T, SPT, BLOCK>(sacc, nu_b, tid);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int qx = 0; qx < n; ++qx) lds_atomic_add(&sacc[sl[qx]], (PlanAcc)r1[qx]);
    }
    __syncthreads();
    plan_flush<T, SPT, BLOCK>(y + ystride, mydof, nu_b, tid, sacc);
    plan_zero<T, SPT, BLOCK>(sacc, nu_b, tid);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int qx = 0; qx < n; ++qx) lds_atomic_add(&sacc[sl[qx]], (PlanAcc)r2[qx]);
    }
    __syncthreads();
    plan_flush<T, SPT, BLOCK>(y + (int64_t)2 * ystride, mydof, nu_b, tid, sacc);
  } else {
#pragma unroll
    for (int d = 0; d < 3; ++d) plan_flush<T, SPT, BLOCK>(y + (int64_t)d * ystride, mydof, nu_b, tid, sacc + d * M);
  }
}

template <typename T, int P, bool ONEACC = gradient_single_accumulator<T, P>(), bool PADLDS = true, int CPB = plan_cells_per_batch<P>()>
inline hipError_t launch_gradient_plan_geom(const T* x, const T* cc, T* y, int64_t ystride, const T* x_g, const int32_t* x_dofs,
                                            const T* pts, const T* wts, const void* workspace, const T* dphi, int64_t ncell,
                                            hipStream_t stream, bool ordered = false, bool use_runs = false) {
  return plan_launch(workspace, P, CPB, ncell, stream, ordered, use_runs, [&](auto o, auto r, const PlanView& v, LaunchSignal sig) {
    hipLaunchKernelGGL((gradient_plan_geom_kernel<T, P, CPB, PADLDS, ONEACC, decltype(o)::value, decltype(r)::value>), dim3((unsigned)v.nbatch),
                       dim3(col_block_threads<P, CPB>()), 0, stream, x, cc, y, ystride, x_g, x_dofs, pts, wts, v.nu, v.udofs, v.slot,
                       dphi, ncell, v.order, v.runs, sig);
  });
}

}  // namespace fus
