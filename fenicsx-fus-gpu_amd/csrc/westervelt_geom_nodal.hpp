// Westervelt cell pass with NODAL coefficients and the geometric factor formed in the kernel:
//   b += sum_q B_q^T G_q ( k3 kappa3(x_q) grad u(x_q) + k4 kappa4(x_q) grad v(x_q) )
// kappa3 / kappa4 are vectors in the dof numbering of u (the GLL rule is collocated: the coefficient at the dofs is the coefficient at
// the quadrature points), k3 / k4 a further factor per cell.  No mass part: the fused stage takes the mass terms from diagonals.
//
// westervelt_cell_geom_kernel<MASS = false> merges its two inputs BEFORE the contraction, K(c3 u + c4 v): that holds for cell constants
// only.  Here the coefficients sit between the gradient and G, so the pass contracts u and v separately -- two forward contractions --
// and merges the two scaled gradients at each quadrature point; G is applied once and ONE backward contraction, one LDS pre-reduction
// and one atomic per distinct dof follow, where two launches of stiffness_plan_geom_nodal_kernel make two of each.
//
// Three LDS cubes, as the twins (fp64 aliases the partial sums onto the dead u cube).  A fourth cube for v (no rewrite of the cube, two
// barriers fewer) was built and measured at fp64 P = 4 and P = 6: 10.9 / 14.4 KB more LDS per workgroup, more registers (165 / 204
// against 152 / 188), the same workgroups per CU as this form's registers allow, and no faster (242.0 against 240.4 us, 245.8 against
// 239.3 us); at fp64 P = 10 it would not fit a workgroup's share of LDS beside another.  Order:
//   1. gather kappa3 / kappa4 of the batch's distinct dofs into the f_y / f_z cubes (u, v wait in registers: all four gathers are one
//      round trip); every column takes its n + n coefficients, times k3 / k4, into registers
//   2. the staged u, v values replace them; every column takes u[n], v[n] and writes the u cube
//   3. grad u at each quadrature point: kappa3 grad u goes UN-transformed into (fx registers, the thread's own f_y / f_z slots)
//   4. the cube is overwritten with v
//   5. grad v: kappa4 grad v is added to the thread's own three slots, G applied once, in place
//   6. backward contraction, pre-reduction, flush: plan_backward / plan_flush
#pragma once

#include "stiffness_geom.hpp"

namespace fus {

template <typename T, int P, int CPB, int MINW, bool ORDERED, bool RUNS>
__global__ void __launch_bounds__((col_block_threads<P, CPB>()), MINW)
    westervelt_cell_geom_nodal_kernel(const T* __restrict__ u_in, const T* __restrict__ v_in, const T* __restrict__ c3,
                                      const T* __restrict__ c4, const T* __restrict__ nodal3, const T* __restrict__ nodal4,
                                      T* __restrict__ b, const T* __restrict__ x_g, const int32_t* __restrict__ x_dofs,
                                      const T* __restrict__ pts, const T* __restrict__ wts, const int32_t* __restrict__ nu,
                                      const int32_t* __restrict__ udofs, const uint16_t* __restrict__ slot,
                                      const T* __restrict__ dphi, int64_t ncell, const int32_t* __restrict__ order,
                                      const int32_t* __restrict__ runs, LaunchSignal sig) {
  constexpr int n = P + 1, n2 = n * n, Nd = n2 * n;
  launch_signal_publish(sig);
  constexpr int S = lds_cell_stride<T, P>();
  constexpr int BLOCK = col_block_threads<P, CPB>();
  constexpr int M = CPB * Nd;
  constexpr int SPT = (M + BLOCK - 1) / BLOCK;
  constexpr int VPT = (CPB * 24 + BLOCK - 1) / BLOCK;
  static_assert(CPB * S >= M, "a cube holds one value per distinct dof of the batch");

  __shared__ T sD[n2 + 1];  // + 1: plan_table_store
  __shared__ T sP[n + 1], sW[n + 1];
  __shared__ T sX[CPB * 24];
  __shared__ T su[CPB * S];
  __shared__ T sfy[CPB * S];
  __shared__ T sfz[CPB * S];
  // partial sums are accumulated in double (PlanAcc, stiffness_plan.hpp): fp64 kernels alias them onto the dead cube, fp32 kernels
  // get an array of their own
  constexpr bool OWN_ACC = sizeof(T) != sizeof(PlanAcc);
  __shared__ PlanAcc sacc_b[OWN_ACC ? M : 1];
  PlanAcc* const sb = OWN_ACC ? sacc_b : reinterpret_cast<PlanAcc*>(su);

  const int tid = threadIdx.x;
  const unsigned batch = blockIdx.x;
  const int lc = tid / n2;
  const int t = tid - lc * n2;
  const int ty = t / n, tz = t - ty * n;
  const int64_t cell0 = (int64_t)batch * CPB;
  const int64_t pos = cell0 + lc;
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
  // ---- round trip 2: what those point to -- (ORDERED: vertex ids and the cell's constants;) u, v, both coefficients and the vertex
  // coordinates
  stage_vertex_ids_of_rows<ORDERED, VPT, BLOCK, CPB>(x_dofs, tid, vid);
  T k3 = T(0), k4 = T(0);
  if (plan_loads_by_all<n>() || active) {
    const int64_t cell = plan_row<ORDERED>(row, pos_ld);
    k3 = c3[cell];
    k4 = c4[cell];
  }
  const int packed = nu[batch];
  const int nu_b = packed & 0xffff, nr_b = plan_runs_of<RUNS>(packed);
  plan_table_store<n, n2>(sD, tid, dval);
  plan_table_store<n, n>(sP, tid, pval);
  plan_table_store<n, n>(sW, tid, wval);
  batch_dofs_resolve<RUNS, SPT, BLOCK>(rt, ud, M, nu_b, nr_b, tid, reinterpret_cast<int32_t*>(su), mydof);

  T a3[n], a4[n];  // k3 kappa3, k4 kappa4 at the column's quadrature points
  T u[n], v[n];
  {
    T xu[SPT], xv[SPT];
    {
      T x3[SPT], x4[SPT];
#pragma unroll
      for (int r = 0; r < SPT; ++r) {
        x3[r] = nodal3[mydof[r]];
        x4[r] = nodal4[mydof[r]];
        xu[r] = u_in[mydof[r]];
        xv[r] = v_in[mydof[r]];
      }
      T cv[VPT];
      stage_vertex_coords_issue<T, VPT, BLOCK, CPB>(x_g, vid, tid, cv);
#pragma unroll
      for (int r = 0; r < SPT; ++r) {
        const int s = tid + r * BLOCK;
        if (s < nu_b) {
          sfy[s] = x3[r];
          sfz[s] = x4[r];
        }
      }
      stage_vertex_coords_store<T, VPT, BLOCK, CPB>(cv, tid, sX);
    }
    __syncthreads();  // B1: the coefficients and the vertex coordinates are in LDS
    if (active) {
#pragma unroll
      for (int ix = 0; ix < n; ++ix) {
        a3[ix] = k3 * sfy[sl[ix]];
        a4[ix] = k4 * sfz[sl[ix]];
      }
    }
    __syncthreads();  // B2: the coefficients are in registers; u and v take their place
#pragma unroll
    for (int r = 0; r < SPT; ++r) {
      const int s = tid + r * BLOCK;
      if (s < nu_b) {
        sfy[s] = xu[r];
        sfz[s] = xv[r];
      }
    }
  }
  __syncthreads();  // B3: u / v values are in LDS

  T J0[3], Ja[3], Jba[3], Jc[3], Jdc[3];
  T wyz = T(0);
  if (active) {
    column_jacobian_rows<T>(sX + lc * 24, sP[ty], sP[tz], J0, Ja, Jba, Jc, Jdc);
    wyz = sW[ty] * sW[tz];
    T* cu = su + lc * S + t;
#pragma unroll
    for (int ix = 0; ix < n; ++ix) {
      u[ix] = sfy[sl[ix]];
      v[ix] = sfz[sl[ix]];
      cu[ix * n2] = u[ix];
    }
  }
  __syncthreads();  // B4: the u cube is written; the staged values are dead

  T fx[n];
  T dy[n], dz[n];
  const T* cu_y = su + lc * S + tz;
  const T* cu_z = su + lc * S + ty * n;
  T* cfy = sfy + lc * S + t;
  T* cfz = sfz + lc * S + t;
  if (active) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
      dy[i] = sD[ty * n + i];
      dz[i] = sD[tz * n + i];
    }
#pragma unroll
    for (int qx = 0; qx < n; ++qx) {  // kappa3 grad u, un-transformed, into the thread's own three slots
      T vx, vy, vz;
      plan_grad_at<T, n, n2>(qx, dphi, u, dy, dz, cu_y, cu_z, vx, vy, vz);
      fx[qx] = a3[qx] * vx;
      cfy[qx * n2] = a3[qx] * vy;
      cfz[qx * n2] = a3[qx] * vz;
    }
  }
  __syncthreads();  // B5: every read of the u cube is done
  if (active) {
    T* cu = su + lc * S + t;
#pragma unroll
    for (int ix = 0; ix < n; ++ix) cu[ix * n2] = v[ix];
  }
  __syncthreads();  // B6: the cube holds v
  if (active) {
#pragma unroll
    for (int qx = 0; qx < n; ++qx) {  // + kappa4 grad v, then G once, in place
      T vx, vy, vz;
      plan_grad_at<T, n, n2>(qx, dphi, v, dy, dz, cu_y, cu_z, vx, vy, vz);
      const T gx = fx[qx] + a4[qx] * vx;
      const T gy = cfy[qx * n2] + a4[qx] * vy;
      const T gz = cfz[qx * n2] + a4[qx] * vz;
      if constexpr (sizeof(T) == 8 && P == 6) {  // the flux without forming G, where westervelt_cell_geom_kernel takes it
        T fy, fz;
        column_flux_at<T>(pts[qx], wts[qx] * wyz, J0, Ja, Jba, Jc, Jdc, gx, gy, gz, fx[qx], fy, fz);
        cfy[qx * n2] = fy;
        cfz[qx * n2] = fz;
      } else {
        T gq[6];
        column_g_at<T>(pts[qx], wts[qx] * wyz, J0, Ja, Jba, Jc, Jdc, gq);
        apply_g6<T>(gq, gx, gy, gz, fx[qx], cfy[qx * n2], cfz[qx * n2]);
      }
    }
  }
  __syncthreads();  // B7: the fluxes are written, the v cube is dead
  plan_zero<T, SPT, BLOCK>(sb, nu_b, tid);
  __syncthreads();

  plan_backward<T, n, n2>(dphi, sD, ty, tz, active, fx, sfy + lc * S + tz, sfz + lc * S + ty * n, sl, sb);
  plan_flush<T, SPT, BLOCK>(b, mydof, nu_b, tid, sb);
}

// Occupancy hint of the shipped builds (waves per SIMD the register allocation must allow): tools/resource_usage.py, DESIGN 3.15.
// fp32 P = 2, 3, 5 sit a few registers over a step unforced (81, 82, 102 VGPRs: 5, 5, 4 waves) and take the hint without scratch
// (76, 80, 96: 6, 6, 5 waves).  The fp64 builds do not: forced to the next step P = 1, 4, 6, 7 spill 20 to 128 bytes per lane, so
// they stay unforced and bound by their registers.
template <typename T, int P>
__host__ __device__ constexpr int westervelt_nodal_min_waves() {
  if (sizeof(T) == 4) return (P == 2 || P == 3) ? 6 : (P == 5 ? 5 : 1);
  return 1;
}

template <typename T, int P, int MINW = westervelt_nodal_min_waves<T, P>(), int CPB = plan_cells_per_batch<P>()>
inline hipError_t launch_westervelt_cell_geom_nodal(const T* u, const T* v, const T* c3, const T* c4, const T* nodal3, const T* nodal4,
                                                    T* b, const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts,
                                                    const void* workspace, const T* dphi, int64_t ncell, hipStream_t stream,
                                                    bool ordered = false, bool use_runs = false) {
  return plan_launch(workspace, P, CPB, ncell, stream, ordered, use_runs, [&](auto o, auto r, const PlanView& pv, LaunchSignal sig) {
    hipLaunchKernelGGL((westervelt_cell_geom_nodal_kernel<T, P, CPB, MINW, decltype(o)::value, decltype(r)::value>),
                       dim3((unsigned)pv.nbatch), dim3(col_block_threads<P, CPB>()), 0, stream, u, v, c3, c4, nodal3, nodal4, b, x_g,
                       x_dofs, pts, wts, pv.nu, pv.udofs, pv.slot, dphi, ncell, pv.order, pv.runs, sig);
  });
}

}  // namespace fus
