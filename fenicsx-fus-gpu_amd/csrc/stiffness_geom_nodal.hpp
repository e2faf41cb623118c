// Planned stiffness apply with a NODAL coefficient and the geometric factor formed in the kernel:
//   y += K(c_cell * kappa) x,    K = sum_q B_q^T (c_cell kappa(x_q) G_q) B_q
// kappa is a vector in the dof numbering of x.  The GLL rule is collocated, so kappa at the dofs is kappa at the quadrature
// points: the thread that owns the column (ty, tz) holds, in kappa[sl[ix]], the coefficients of its n quadrature points.
//
// This is stiffness_plan_geom_kernel (stiffness_geom.hpp) with a second gather in the round trip of the first, as
// westervelt_cell_geom_kernel gathers u and v: the x values of the batch's distinct dofs go to the f_y cube (or the array of the
// partial sums where the kernel does not alias), the kappa values to the f_z cube, both dead until the flux loop.  Between the
// two barriers of the gather every column reads its n coefficients and folds them into the scale of its quadrature planes,
//   k[qx] = c_cell w_y w_z w_x[qx] kappa[sl[qx]]
// which is what column_g_at / column_flux_at take as their scale anyway: the three flux components at qx come out multiplied
// by c_cell kappa[qx] and the flux loop holds no further operation.  PREG builds (the n x 6 factors formed before the
// contraction phases) take the scale there and keep no coefficient registers at all; the in-loop builds keep the n scales.
// Everything else -- preamble, vertex staging, contractions, LDS pre-reduction, one atomic per distinct dof -- is the per-cell
// kernel's, through the same device functions.  A kernel of its own so that the per-cell kernel keeps its code (stiffness_plan.hpp).
#pragma once

#include "stiffness_geom.hpp"

namespace fus {

template <typename T, int P, int CPB, bool ALIAS, bool PADLDS, int MINW, bool PREG, bool ORDERED, bool RUNS>
__global__ void __launch_bounds__((col_block_threads<P, CPB>()), MINW)
    stiffness_plan_geom_nodal_kernel(const T* __restrict__ x, const T* __restrict__ cell_constants, const T* __restrict__ nodal,
                                     T* __restrict__ y, const T* __restrict__ x_g, const int32_t* __restrict__ x_dofs,
                                     const T* __restrict__ pts, const T* __restrict__ wts, const int32_t* __restrict__ nu,
                                     const int32_t* __restrict__ udofs, const uint16_t* __restrict__ slot,
                                     const T* __restrict__ dphi, int64_t ncell, const int32_t* __restrict__ order,
                                     const int32_t* __restrict__ runs, LaunchSignal sig) {
  using Sh = PlanShape<T, P, CPB, PADLDS>;
  constexpr int n = Sh::n, n2 = Sh::n2, Nd = Sh::Nd, S = Sh::S, BLOCK = Sh::BLOCK, M = Sh::M, SPT = Sh::SPT;
  static_assert(CPB * S >= M, "the f_z cube holds the coefficients of the batch's distinct dofs");
  launch_signal_publish(sig);
  constexpr int VPT = (CPB * 24 + BLOCK - 1) / BLOCK;  // vertex coordinates staged per thread (1 for P >= 4)

  __shared__ T sD[n2 + 1];  // + 1: plan_table_store
  __shared__ T sP[n + 1], sW[n + 1];
  __shared__ T sX[CPB * 24];
  __shared__ T su[CPB * S];
  __shared__ T sfy[CPB * S];
  __shared__ T sfz[CPB * S];
  __shared__ PlanAcc sacc[PlanOwnAcc<T, ALIAS>::value ? M : 1];
  T* const sx = ALIAS ? sfy : reinterpret_cast<T*>(sacc);  // x values of the batch's distinct dofs
  T* const sk = sfz;                                       // their coefficients: read before the flux loop writes the cube
  PlanAcc* const sy = PlanOwnAcc<T, ALIAS>::value ? sacc : reinterpret_cast<PlanAcc*>(su);  // their y partial sums

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
  // ---- round trip 2: what those point to -- (ORDERED: vertex ids and the cell's constant;) x, kappa and the vertex coordinates
  stage_vertex_ids_of_rows<ORDERED, VPT, BLOCK, CPB>(x_dofs, tid, vid);
  T coeff = T(0);
  if (plan_loads_by_all<n>() || active) coeff = cell_constants[plan_row<ORDERED>(row, pos_ld)];
  const int packed = nu[batch];
  const int nu_b = packed & 0xffff, nr_b = plan_runs_of<RUNS>(packed);
  plan_table_store<n, n2>(sD, tid, dval);
  plan_table_store<n, n>(sP, tid, pval);
  plan_table_store<n, n>(sW, tid, wval);
  batch_dofs_resolve<RUNS, SPT, BLOCK>(rt, ud, M, nu_b, nr_b, tid, reinterpret_cast<int32_t*>(su), mydof);

  // ---- gather x and kappa (as westervelt_cell_geom_kernel gathers u and v) with the column geometry formed between the barriers
  {
    T xv[SPT], kv[SPT];
#pragma unroll
    for (int r = 0; r < SPT; ++r) {
      xv[r] = x[mydof[r]];
      kv[r] = nodal[mydof[r]];
    }
    T cv[VPT];
    stage_vertex_coords_issue<T, VPT, BLOCK, CPB>(x_g, vid, tid, cv);
#pragma unroll
    for (int r = 0; r < SPT; ++r) {
      const int s = tid + r * BLOCK;
      if (s < nu_b) {
        sx[s] = xv[r];
        sk[s] = kv[r];
      }
    }
    stage_vertex_coords_store<T, VPT, BLOCK, CPB>(cv, tid, sX);
  }
  __syncthreads();  // x values, coefficients and vertex coordinates are in LDS

  T J0[3], Ja[3], Jba[3], Jc[3], Jdc[3];
  T g[PREG ? n : 1][6];
  T k[PREG ? 1 : n];  // scale of the column's quadrature planes: c_cell w_y w_z w_x[qx] kappa(x_q)
  if (active) {
    column_jacobian_rows<T>(sX + lc * 24, sP[ty], sP[tz], J0, Ja, Jba, Jc, Jdc);
    const T s0 = coeff * sW[ty] * sW[tz];
#pragma unroll
    for (int qx = 0; qx < n; ++qx) {
      const T kq = wts[qx] * s0 * sk[sl[qx]];
      if constexpr (PREG) column_g_at<T>(pts[qx], kq, J0, Ja, Jba, Jc, Jdc, g[qx]);
      else k[qx] = kq;
    }
  }

  T u[n];
  if (active) {
    T* cu = su + lc * S + t;
#pragma unroll
    for (int ix = 0; ix < n; ++ix) {
      u[ix] = sx[sl[ix]];
      cu[ix * n2] = u[ix];
    }
  }
  __syncthreads();  // the u cube is written; the x values and the coefficients are dead
  if constexpr (!ALIAS) plan_zero<T, SPT, BLOCK>(sy, nu_b, tid);

  T fx[n];
  if (active) {
    T dy[n], dz[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      dy[i] = sD[ty * n + i];
      dz[i] = sD[tz * n + i];
    }
    const T* cu_y = su + lc * S + tz;
    const T* cu_z = su + lc * S + ty * n;
    T* cfy = sfy + lc * S + t;
    T* cfz = sfz + lc * S + t;
#pragma unroll
    for (int qx = 0; qx < n; ++qx) {
      T vx, vy, vz;
      plan_grad_at<T, n, n2>(qx, dphi, u, dy, dz, cu_y, cu_z, vx, vy, vz);
      if constexpr (!PREG && geom_flux_operator_form<T, P>()) {  // the flux without forming G (stiffness_geom.hpp)
        T fy, fz;
        column_flux_at<T>(pts[qx], k[PREG ? 0 : qx], J0, Ja, Jba, Jc, Jdc, vx, vy, vz, fx[qx], fy, fz);
        cfy[qx * n2] = fy;
        cfz[qx * n2] = fz;
      } else {
        T gl[6];
        if constexpr (!PREG) column_g_at<T>(pts[qx], k[PREG ? 0 : qx], J0, Ja, Jba, Jc, Jdc, gl);
        apply_g6<T>(PREG ? g[PREG ? qx : 0] : gl, vx, vy, vz, fx[qx], cfy[qx * n2], cfz[qx * n2]);
      }
    }
  }
  __syncthreads();
  if constexpr (ALIAS) {
    plan_zero<T, SPT, BLOCK>(sy, nu_b, tid);
    __syncthreads();
  }

  plan_backward<T, n, n2>(dphi, sD, ty, tz, active, fx, sfy + lc * S + tz, sfz + lc * S + ty * n, sl, sy);
  plan_flush<T, SPT, BLOCK>(y, mydof, nu_b, tid, sy);
}

// PREG of the nodal kernel per degree and scalar type: the per-cell kernel's choice (geom_factors_in_registers), so that both kernels
// form their factors in the same place and their results differ by the coefficient alone -- except fp32 P = 5, where the 36 factor
// registers leave 99 VGPRs (4 waves per SIMD, one fewer than westervelt_cell_geom_kernel<float, 5, ..., MASS = false>, which forms G in
// its loop): the in-loop build keeps 6 scales instead, 91 VGPRs, 5 waves.  fp64 P = 4 is compiled for the 4 waves of the per-cell
// kernel (unforced 129 VGPRs, one over the step; with the hint 128, no scratch: tools/resource_usage.py).
template <typename T, int P>
__host__ __device__ constexpr bool nodal_factors_in_registers() {
  return geom_factors_in_registers<T, P>() && !(sizeof(T) == 4 && P == 5);
}
// Occupancy hint of the shipped builds (waves per SIMD the register allocation must allow).
template <typename T, int P>
__host__ __device__ constexpr int nodal_min_waves() {
  return (sizeof(T) == 8 && P == 4) ? 4 : geom_min_waves<T, P>();
}

template <typename T, int P, bool ALIAS, bool PADLDS, int MINW, bool PREG, int CPB = plan_cells_per_batch<P>()>
inline hipError_t launch_stiffness_plan_geom_nodal(const T* x, const T* cc, const T* nodal, T* y, const T* x_g, const int32_t* x_dofs,
                                                   const T* pts, const T* wts, const void* workspace, const T* dphi, int64_t ncell,
                                                   hipStream_t stream, bool ordered = false, bool use_runs = false) {
  return plan_launch(workspace, P, CPB, ncell, stream, ordered, use_runs, [&](auto o, auto r, const PlanView& v, LaunchSignal sig) {
    hipLaunchKernelGGL((stiffness_plan_geom_nodal_kernel<T, P, CPB, ALIAS, PADLDS, MINW, PREG, decltype(o)::value, decltype(r)::value>),
                       dim3((unsigned)v.nbatch), dim3(col_block_threads<P, CPB>()), 0, stream, x, cc, nodal, y, x_g, x_dofs, pts, wts,
                       v.nu, v.udofs, v.slot, dphi, ncell, v.order, v.runs, sig);
  });
}

}  // namespace fus
