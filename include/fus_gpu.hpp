/*
 * fus_gpu.hpp -- header-only C++ functors over the C ABI of libfusgpu.so, shaped like the reference's
 *
 *     template <typename T, int P> class MassSpectral3D       cpp/common/spectral_op.hpp:29-107
 *     template <typename T, int P> class StiffnessSpectral3D  cpp/common/spectral_op.hpp:132-284
 *         void operator()(const la::Vector<T>& x, std::span<T> coeffs, la::Vector<T>& y)      (y += A(coeffs) x)
 *
 * The reference's constructors take a dolfinx FunctionSpace and do three things with it: reorder the dofmap to the
 * tensor-product order (cpp/common/permute.hpp), tabulate the GLL rule / 1-D derivative table (basix) and precompute the
 * geometry factors (cpp/common/precompute.hpp).  dolfinx / basix are not part of this library, so the constructors here
 * take what those steps produce or consume, as DEVICE arrays: the tensor-product dofmap, the P1 geometry (x_dofs, x_g)
 * with the tabulated P1 gradients + weights (the geometry factors are then computed on the device, the twin of
 * precompute.hpp:101-213) or the factors themselves, and the 1-D derivative table.  operator() takes device pointers
 * where the reference takes la::Vector / std::span (which live on the host there).
 *
 * Every call is asynchronous on ``stream``; errors are exceptions carrying fus_error_string().  The functors own the
 * batch-plan workspace (and the geometry factors they computed); everything else is caller-owned, as in the C ABI.
 */
#ifndef FUS_GPU_HPP
#define FUS_GPU_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#include "fus_gpu.h"
#include "fus_gpu_array.h"
#include "fus_gpu_relaxation.h"
#include "fus_gpu_nodal.h"
#include "fus_gpu_westervelt_nodal.h"
#include "fus_gpu_reduce.h"
#include "fus_gpu_sensor.h"

namespace fus_gpu {

inline void check(int rc, const char* what) {
  if (rc != FUS_OK) throw std::runtime_error(std::string(what) + ": " + fus_error_string(rc));
}
inline void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline void check_abi() {
  if (fus_abi_version() != FUS_ABI_VERSION)
    throw std::runtime_error("libfusgpu.so ABI version " + std::to_string(fus_abi_version()) + ", header " +
                             std::to_string(FUS_ABI_VERSION));
}

template <typename T>
struct Geometry {  // what compute_scaled_geometrical_factor / _jacobian_determinant read (device arrays)
  const T* x_g;           // [nvert][3]
  const int32_t* x_dofs;  // [ncell][8], vertex v = vx + 2 vy + 4 vz
  const T* dphi_p1;       // [3][nq][8] gradients of the P1 shape functions at the quadrature points
  const T* weights;       // [nq] tensor GLL weights
};

namespace detail {
// the entry point of a typed pair for T: f64 for double, f32 for float.  The call that follows is checked by the compiler against the
// prototype of fus_gpu.h, so a functor cannot pass what the C ABI does not declare.
template <typename T, typename F64, typename F32>
constexpr typename std::conditional<std::is_same<T, double>::value, F64, F32>::type typed(F64 f64, F32 f32) {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  return std::get<std::is_same<T, float>::value ? 1 : 0>(std::pair<F64, F32>(f64, f32));
}

// a device allocation owned by a functor: released when the functor's constructor throws after it, too (a member that is
// fully constructed is destroyed then; a raw pointer freed by the class's own destructor is not).  The stream the geometry
// kernel was enqueued on is drained first: the kernel may still be writing the buffer.
template <typename T>
struct DeviceBuffer {
  T* p = nullptr;
  hipStream_t stream = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void allocate(size_t count, hipStream_t s, const char* what) {
    stream = s;
    check_hip(hipMalloc(&p, sizeof(T) * count), what);
  }
  ~DeviceBuffer() {
    if (p) {
      (void)hipStreamSynchronize(stream);
      (void)hipFree(p);
    }
  }
};

// the batch plan of a dofmap (device workspace owned by the functor; registered with the library at this address)
struct Plan {
  void* ws = nullptr;
  int N = 0, epb = 0;
  int64_t nent = 0;
  Plan() = default;
  Plan(const Plan&) = delete;
  Plan& operator=(const Plan&) = delete;
  void build(const int32_t* dofmap, int ndof_per_entity, int64_t n_entities, hipStream_t stream) {
    N = ndof_per_entity;
    nent = n_entities;
    epb = fus_plan_entities_per_batch(N);
    check(epb < 0 ? epb : FUS_OK, "fus_plan_entities_per_batch");
    const int64_t bytes = fus_plan_bytes(N, epb, nent);
    check(bytes < 0 ? (int)bytes : FUS_OK, "fus_plan_bytes");
    check_hip(hipMalloc(&ws, (size_t)bytes), "hipMalloc(plan workspace)");
    check(fus_plan_build(dofmap, N, epb, nent, ws, bytes, stream), "fus_plan_build");
  }
  ~Plan() {
    if (ws) {
      (void)fus_plan_release(ws);
      (void)hipFree(ws);
    }
  }
};
// the transposed dofmap of the atomic-free mass apply (fus_mass_gather_plan_build); ``ok`` stays false when the library
// declines the dofmap (a dof in more than 255 entities): the functor then keeps to the atomic kernel
struct GatherPlan {
  void* ws = nullptr;
  bool ok = false;
  GatherPlan() = default;
  GatherPlan(const GatherPlan&) = delete;
  GatherPlan& operator=(const GatherPlan&) = delete;
  void release() {
    if (ws) {
      (void)fus_plan_release(ws);
      (void)hipFree(ws);
    }
    ws = nullptr;
    ok = false;
  }
  void build(const int32_t* dofmap, int ndof_per_entity, int64_t n_entities, int64_t ndofs, hipStream_t stream) {
    release();  // a second enable_gather() replaces the first plan instead of leaking it
    const int64_t bytes = fus_mass_gather_plan_bytes(ndof_per_entity, n_entities, ndofs);
    if (bytes < 0) return;  // 2^31 entries or more: atomic kernel
    check_hip(hipMalloc(&ws, (size_t)bytes), "hipMalloc(gather plan workspace)");
    const int rc = fus_mass_gather_plan_build(dofmap, ndof_per_entity, n_entities, ndofs, ws, bytes, stream);
    if (rc == FUS_ERR_UNSUPPORTED_ENTITY) return;
    check(rc, "fus_mass_gather_plan_build");
    ok = true;
  }
  ~GatherPlan() { release(); }
};
// the static companion of a transposed dofmap (fus_mass_gather_static_build): detJ in row order; ``ok`` stays false when the
// library declines (a block of 256 dofs spanning more than 65 535 entities): the functor then gathers detJ as before
struct GatherStaticPlan {
  void* ws = nullptr;
  bool ok = false;
  GatherStaticPlan() = default;
  GatherStaticPlan(const GatherStaticPlan&) = delete;
  GatherStaticPlan& operator=(const GatherStaticPlan&) = delete;
  void release() {
    if (ws) {
      (void)fus_plan_release(ws);
      (void)hipFree(ws);
    }
    ws = nullptr;
    ok = false;
  }
  template <typename T>
  void build(const void* gather_ws, const T* detJ, int ndof_per_entity, int64_t n_entities, hipStream_t stream) {
    release();
    const int64_t bytes = fus_mass_gather_static_bytes(ndof_per_entity, n_entities, (int)sizeof(T));
    if (bytes < 0) return;
    check_hip(hipMalloc(&ws, (size_t)bytes), "hipMalloc(static companion of the gather plan)");
    const int rc = typed<T>(fus_mass_gather_static_build_f64, fus_mass_gather_static_build_f32)(gather_ws, detJ, ws, bytes, stream);
    if (rc == FUS_ERR_UNSUPPORTED_ENTITY) return;
    check(rc, "fus_mass_gather_static_build");
    ok = true;
  }
  ~GatherStaticPlan() { release(); }
};
}  // namespace detail

/// y += M(coeffs) x, M the collocated (diagonal) GLL mass operator; cpp/common/spectral_op.hpp:29-107
template <typename T, int P>
class MassSpectral3D {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");

public:
  static constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  /// dofmap: device int32[ncells][(P+1)^3], tensor-product local order; the scaled Jacobian determinant is computed here
  MassSpectral3D(const int32_t* dofmap, int64_t ncells, const Geometry<T>& geo, hipStream_t stream = nullptr) : Nc(ncells) {
    check_abi();  // before anything is allocated
    detJ_own_.allocate((size_t)Nc * Nd, stream, "hipMalloc(detJ)");
    check(detail::typed<T>(fus_geometry_factors_f64, fus_geometry_factors_f32)(geo.x_g, geo.x_dofs, geo.dphi_p1, geo.weights, Nd, Nc, nullptr,
                                                                               detJ_own_.p, stream),
          "fus_geometry_factors (detJ)");
    detJ_ = detJ_own_.p;
    plan_.build(dofmap, Nd, Nc, stream);
  }
  /// with the factors the caller already has (device T[ncells][(P+1)^3])
  MassSpectral3D(const int32_t* dofmap, int64_t ncells, const T* detJ, hipStream_t stream = nullptr) : Nc(ncells), detJ_(detJ) {
    check_abi();
    plan_.build(dofmap, Nd, Nc, stream);
  }
  MassSpectral3D(const MassSpectral3D&) = delete;
  MassSpectral3D& operator=(const MassSpectral3D&) = delete;
  /// Opt in to the atomic-free kernel (one thread per dof over the transposed dofmap: no float atomics, bitwise
  /// reproducible, 0.091 against 0.133 ms at P = 4 / 10 M dofs): ``ndofs`` = length of the vectors the operator is applied to
  /// (every dofmap value < ndofs).  A launch then assumes that nothing else adds into y while it runs (other launches of the
  /// same stream are fine); ``apply_atomic`` stays safe next to concurrent writers (a halo receive, another stream).
  /// ``static_detJ``: detJ is ALSO kept in ROW order and the kernel streams that copy instead of gathering detJ through the
  /// transposed dofmap (0.080 against 0.091 ms; bitwise the same result) -- a snapshot that is never re-read.  kStaticAuto
  /// (default): only where the functor OWNS detJ (the constructor that computes it once, as the reference's does,
  /// cpp/common/spectral_op.hpp:60-66: nobody else can change it); a caller-owned detJ is gathered live unless the caller
  /// promises with kStaticAlways (or ``true``) that it stays constant; kStaticNever (or ``false``): never.  Calling
  /// enable_gather() again rebuilds both plans (and re-takes the snapshot).
  static constexpr int kStaticAuto = -1, kStaticNever = 0, kStaticAlways = 1;
  void enable_gather(const int32_t* dofmap, int64_t ndofs, hipStream_t stream = nullptr, int static_detJ = kStaticAuto) {
    static_.release();  // (belongs to the gather plan that is about to be replaced)
    gather_.build(dofmap, Nd, Nc, ndofs, stream);
    const bool snapshot = static_detJ == kStaticAuto ? detJ_own_.p != nullptr : static_detJ != kStaticNever;
    if (gather_.ok && snapshot) static_.template build<T>(gather_.ws, detJ_, Nd, Nc, stream);
  }
  bool gather_enabled() const { return gather_.ok; }
  bool static_detJ_enabled() const { return static_.ok; }
  /// y += M x   (x, y: device vectors of nlocal + nghost entries; coeffs: device T[ncells])
  void operator()(const T* x, const T* coeffs, T* y, hipStream_t stream = nullptr) const {
    if (static_.ok)
      check(detail::typed<T>(fus_mass_apply_gather_static_f64, fus_mass_apply_gather_static_f32)(x, coeffs, y, gather_.ws, static_.ws, Nd, Nc, stream),
            "fus_mass_apply_gather_static");
    else if (gather_.ok)
      check(detail::typed<T>(fus_mass_apply_gather_f64, fus_mass_apply_gather_f32)(x, coeffs, y, detJ_, gather_.ws, Nd, Nc, stream),
            "fus_mass_apply_gather");
    else
      apply_atomic(x, coeffs, y, stream);
  }
  void apply_atomic(const T* x, const T* coeffs, T* y, hipStream_t stream = nullptr) const {
    check(detail::typed<T>(fus_mass_apply_planned_f64, fus_mass_apply_planned_f32)(x, coeffs, y, detJ_, plan_.ws, Nd, plan_.epb, Nc, stream),
          "fus_mass_apply_planned");
  }
  const T* detJ() const { return detJ_; }

private:
  int64_t Nc;
  const T* detJ_ = nullptr;
  detail::DeviceBuffer<T> detJ_own_;  // members are released in reverse order, also when the constructor throws
  detail::Plan plan_;
  detail::GatherPlan gather_;
  detail::GatherStaticPlan static_;  // (declared after gather_: released before the plan it belongs to)
};

/// y += K(coeffs) x, the sum-factorised stiffness operator; cpp/common/spectral_op.hpp:132-284
template <typename T, int P>
class StiffnessSpectral3D {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");

public:
  static constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  /// dphi: device T[(P+1)][(P+1)] 1-D GLL derivative table [q][i]; G is computed here (device twin of precompute.hpp:101-213)
  StiffnessSpectral3D(const int32_t* dofmap, int64_t ncells, const Geometry<T>& geo, const T* dphi, hipStream_t stream = nullptr)
      : Nc(ncells), dphi_(dphi) {
    check_abi();  // before anything is allocated
    G_own_.allocate((size_t)Nc * Nd * 6, stream, "hipMalloc(G)");
    check(detail::typed<T>(fus_geometry_factors_f64, fus_geometry_factors_f32)(geo.x_g, geo.x_dofs, geo.dphi_p1, geo.weights, Nd, Nc, G_own_.p,
                                                                               nullptr, stream),
          "fus_geometry_factors (G)");
    G_ = G_own_.p;
    plan_.build(dofmap, Nd, Nc, stream);
  }
  /// with the factors the caller already has (device T[ncells][(P+1)^3][6])
  StiffnessSpectral3D(const int32_t* dofmap, int64_t ncells, const T* G, const T* dphi, hipStream_t stream = nullptr)
      : Nc(ncells), G_(G), dphi_(dphi) {
    check_abi();
    plan_.build(dofmap, Nd, Nc, stream);
  }
  StiffnessSpectral3D(const StiffnessSpectral3D&) = delete;
  StiffnessSpectral3D& operator=(const StiffnessSpectral3D&) = delete;
  /// y += K x
  void operator()(const T* x, const T* coeffs, T* y, hipStream_t stream = nullptr) const {
    check(detail::typed<T>(fus_stiffness_apply_planned_f64, fus_stiffness_apply_planned_f32)(x, coeffs, y, G_, plan_.ws, dphi_, P, Nc, stream),
          "fus_stiffness_apply_planned");
  }
  const T* G() const { return G_; }

private:
  int64_t Nc;
  const T* G_ = nullptr;
  detail::DeviceBuffer<T> G_own_;
  const T* dphi_ = nullptr;
  detail::Plan plan_;
};

/// y[d] += C_d(coeffs) x, d = 0, 1, 2: the weak gradient with the geometry formed in the kernel (fus_gradient_apply_planned_geom_*;
/// no reference counterpart).  Divided by the lumped mass M(1) 1 it is the nodal projection of coeffs * grad x.
template <typename T, int P>
class GradientSpectral3D {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");

public:
  static constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  /// x_g [nvert][3], x_dofs [ncells][8], pts / wts: 1-D GLL points on [0, 1] and weights T[P+1], dphi T[P+1][P+1]: device arrays
  GradientSpectral3D(const int32_t* dofmap, int64_t ncells, const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts, const T* dphi,
                     hipStream_t stream = nullptr)
      : Nc(ncells), x_g_(x_g), x_dofs_(x_dofs), pts_(pts), wts_(wts), dphi_(dphi) {
    check_abi();
    plan_.build(dofmap, Nd, Nc, stream);
  }
  GradientSpectral3D(const GradientSpectral3D&) = delete;
  GradientSpectral3D& operator=(const GradientSpectral3D&) = delete;
  /// y: T[3][ystride], ystride >= number of dofs; contributions are added
  void operator()(const T* x, const T* coeffs, T* y, int64_t ystride, hipStream_t stream = nullptr) const {
    check(detail::typed<T>(fus_gradient_apply_planned_geom_f64, fus_gradient_apply_planned_geom_f32)(x, coeffs, y, ystride, x_g_, x_dofs_, pts_, wts_,
                                                                                                     plan_.ws, dphi_, P, Nc, stream),
          "fus_gradient_apply_planned_geom");
  }

private:
  int64_t Nc;
  const T* x_g_ = nullptr;
  const int32_t* x_dofs_ = nullptr;
  const T *pts_ = nullptr, *wts_ = nullptr, *dphi_ = nullptr;
  detail::Plan plan_;
};

/// y += K(coeffs * nodal) x: the stiffness operator with a NODAL coefficient inside its contraction and the geometry formed in the kernel
/// (fus_stiffness_apply_planned_geom_nodal_*, include/fus_gpu_nodal.h; no reference counterpart: its coefficients are per cell).
/// ``nodal`` is a device vector in the dof numbering of x; the GLL rule is collocated, so it is the coefficient at the quadrature points.
template <typename T, int P>
class NodalStiffnessSpectral3D {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");

public:
  static constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  /// x_g [nvert][3], x_dofs [ncells][8], pts / wts: 1-D GLL points on [0, 1] and weights T[P+1], dphi T[P+1][P+1], nodal T[ndofs]: device arrays
  NodalStiffnessSpectral3D(const int32_t* dofmap, int64_t ncells, const T* x_g, const int32_t* x_dofs, const T* pts, const T* wts,
                           const T* dphi, const T* nodal, hipStream_t stream = nullptr)
      : Nc(ncells), x_g_(x_g), x_dofs_(x_dofs), pts_(pts), wts_(wts), dphi_(dphi), nodal_(nodal) {
    check_abi();
    plan_.build(dofmap, Nd, Nc, stream);
  }
  NodalStiffnessSpectral3D(const NodalStiffnessSpectral3D&) = delete;
  NodalStiffnessSpectral3D& operator=(const NodalStiffnessSpectral3D&) = delete;
  /// y += K x   (coeffs: device T[ncells], a further factor per cell)
  void operator()(const T* x, const T* coeffs, T* y, hipStream_t stream = nullptr) const {
    check(detail::typed<T>(fus_stiffness_apply_planned_geom_nodal_f64, fus_stiffness_apply_planned_geom_nodal_f32)(
              x, coeffs, nodal_, y, x_g_, x_dofs_, pts_, wts_, plan_.ws, dphi_, P, Nc, stream),
          "fus_stiffness_apply_planned_geom_nodal");
  }

private:
  int64_t Nc;
  const T* x_g_ = nullptr;
  const int32_t* x_dofs_ = nullptr;
  const T *pts_ = nullptr, *wts_ = nullptr, *dphi_ = nullptr, *nodal_ = nullptr;
  detail::Plan plan_;
};

/// b += sum_q B_q^T G_q (c3 nodal3 grad u + c4 nodal4 grad v): the stiffness part of the Westervelt cell pass with NODAL coefficients
/// on both inputs and the geometry formed in the kernel (fus_westervelt_stiffness_apply_planned_geom_nodal_*,
/// include/fus_gpu_westervelt_nodal.h; no reference counterpart).  ``nodal3`` / ``nodal4`` are device vectors in the dof numbering of u.
template <typename T, int P>
class WesterveltNodalStiffnessSpectral3D {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T: float or double");
  static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");

public:
  static constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  /// x_g [nvert][3], x_dofs [ncells][8], pts / wts: 1-D GLL points on [0, 1] and weights T[P+1], dphi T[P+1][P+1], nodal3 / nodal4
  /// T[ndofs]: device arrays
  WesterveltNodalStiffnessSpectral3D(const int32_t* dofmap, int64_t ncells, const T* x_g, const int32_t* x_dofs, const T* pts,
                                     const T* wts, const T* dphi, const T* nodal3, const T* nodal4, hipStream_t stream = nullptr)
      : Nc(ncells), x_g_(x_g), x_dofs_(x_dofs), pts_(pts), wts_(wts), dphi_(dphi), nodal3_(nodal3), nodal4_(nodal4) {
    check_abi();
    plan_.build(dofmap, Nd, Nc, stream);
  }
  WesterveltNodalStiffnessSpectral3D(const WesterveltNodalStiffnessSpectral3D&) = delete;
  WesterveltNodalStiffnessSpectral3D& operator=(const WesterveltNodalStiffnessSpectral3D&) = delete;
  /// b += K(c3 nodal3) u + K(c4 nodal4) v   (c3, c4: device T[ncells], a further factor per cell)
  void operator()(const T* u, const T* v, const T* c3, const T* c4, T* b, hipStream_t stream = nullptr) const {
    check(detail::typed<T>(fus_westervelt_stiffness_apply_planned_geom_nodal_f64, fus_westervelt_stiffness_apply_planned_geom_nodal_f32)(
              u, v, c3, c4, nodal3_, nodal4_, b, x_g_, x_dofs_, pts_, wts_, plan_.ws, dphi_, P, Nc, stream),
          "fus_westervelt_stiffness_apply_planned_geom_nodal");
  }

private:
  int64_t Nc;
  const T* x_g_ = nullptr;
  const int32_t* x_dofs_ = nullptr;
  const T *pts_ = nullptr, *wts_ = nullptr, *dphi_ = nullptr, *nodal3_ = nullptr, *nodal4_ = nullptr;
  detail::Plan plan_;
};

// Point sensors (fus_probe_eval_*): the field at fixed points after every step, in place of the reference's per-step
// ``u_n_.eval(x_eval, cell_eval)`` (cuda/demo_linear_piston.py).  The host locates the points once: ``cells`` [npts] (rows of
// ``dofmap``), ``weights`` [npts][3][P + 1] (1-D Lagrange rows at the reference coordinates).  All device arrays, caller-owned.
template <typename T, int P>
class PointProbe {
 public:
  PointProbe(const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights)
      : cells_(cells), npts_(npts), dofmap_(dofmap), ncells_(ncells), weights_(weights) {
    static_assert(P >= FUS_MIN_DEGREE && P <= FUS_MAX_DEGREE, "degree out of range");
    check_abi();
  }
  // out[npts] = u at the points
  void operator()(const T* u, T* out, void* stream = nullptr) const { (*this)(u, out, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream); }
  // the general launch: row ``slot`` of rec[capacity][npts], running max / min, H harmonic accumulators (null = off)
  void operator()(const T* u, T* rec, int64_t capacity, int slot, double* pmax, double* pmin, double* hre, double* him,
                  const double* coef, int H, void* stream = nullptr) const {
    check(detail::typed<T>(fus_probe_eval_f64, fus_probe_eval_f32)(u, cells_, npts_, dofmap_, ncells_, weights_, P, rec, capacity, slot, pmax, pmin,
                                                                   hre, him, coef, H, stream),
          "fus_probe_eval");
  }
  int64_t npts() const { return npts_; }

 private:
  const int32_t* cells_;
  int64_t npts_;
  const int32_t* dofmap_;
  int64_t ncells_;
  const T* weights_;
};

// Full-field monitors (fus_field_accumulate_*): running extrema, mean squares and harmonic sums of the owned dofs after every
// recorded step, in place of the reference's per-step dump of the whole field (cuda/demo_nonlinear_bowl.py:662-680).  The output
// arrays are device memory, caller-owned; a null pointer switches an output off.  ``hre`` / ``him``: [H][hstride], H <= 4.
template <typename T>
class FieldAccumulator {
 public:
  FieldAccumulator(int64_t n, T* pmax, T* pmin, double* usq, double* vsq, double* hre = nullptr, double* him = nullptr,
                   int64_t hstride = 0, int H = 0)
      : n_(n), pmax_(pmax), pmin_(pmin), usq_(usq), vsq_(vsq), hre_(hre), him_(him), hstride_(hstride), H_(H) {
    check_abi();
  }
  // one record of (u, v); ``coef``: the 2H factors of this step in device memory; ``init``: the first record of a window
  void operator()(const T* u, const T* v, const double* coef, bool init, void* stream = nullptr) const {
    check(detail::typed<T>(fus_field_accumulate_f64, fus_field_accumulate_f32)(u, v, n_, pmax_, pmin_, usq_, vsq_, hre_, him_, hstride_, coef, H_,
                                                                               init ? 1 : 0, stream),
          "fus_field_accumulate");
  }

 private:
  int64_t n_;
  T *pmax_, *pmin_;
  double *usq_, *vsq_, *hre_, *him_;
  int64_t hstride_;
  int H_;
};

// Pennes bioheat stage (fus_bioheat_stage_*): the vector pass between two stiffness applies of an explicit RK4 step of
// M(rho C) T' = -K(k) T - M(w)(T - Ta) + g M(1) q with b = -K(k) Tn assembled: k = minv b - pr (Tn - Ta) + gate s per owned dof.
// ``pr`` / ``s`` / ``cem43`` / ``tmax`` may be null (term off).  Device arrays, caller-owned: T0, Tn, acc, b [ntotal]; the rest [nlocal].
template <typename T>
class BioheatStage {
 public:
  enum Kind { FIRST = 0, MIDDLE = 1, LAST = 2 };
  BioheatStage(int64_t nlocal, int64_t ntotal, T arterial_temperature, const T* minv, const T* pr, const T* s, T* b, T* T0, T* Tn, T* acc,
               double* cem43 = nullptr, T* tmax = nullptr)
      : nlocal_(nlocal), ntotal_(ntotal), ta_(arterial_temperature), minv_(minv), pr_(pr), s_(s), b_(b), T0_(T0), Tn_(Tn), acc_(acc),
        cem43_(cem43), tmax_(tmax) {
    check_abi();
  }
  // stage ``i`` in 0..3 of the step of length ``dt``; ``gate``: g at the stage time; ``init`` (stage 3): the first step of a dose window
  void operator()(int i, double dt, T gate, bool init = false, void* stream = nullptr) const {
    static const double a[4] = {0.0, 0.5, 0.5, 1.0}, bq[4] = {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0};
    const int kind = i == 3 ? LAST : (i == 0 ? FIRST : MIDDLE);
    check(detail::typed<T>(fus_bioheat_stage_f64, fus_bioheat_stage_f32)((T)(bq[i] * dt), (T)(i == 3 ? 0.0 : a[i + 1] * dt), kind, gate, ta_, dt, minv_,
                                                                         pr_, s_, b_, T0_, Tn_, acc_, cem43_, tmax_, init ? 1 : 0, nlocal_, ntotal_,
                                                                         stream),
          "fus_bioheat_stage");
  }

 private:
  int64_t nlocal_, ntotal_;
  T ta_;
  const T *minv_, *pr_, *s_;
  T *b_, *T0_, *Tn_, *acc_;
  double* cem43_;
  T* tmax_;
};

// Phased-array source facets (fus_facet_source_array_*): the source-facet term of one RK4 stage with a per-element amplitude,
// phase and delay, and the absorbing term in the same launch.  Set A: ``eid`` [nA] (element of each facet, -1 = inactive,
// validated by the caller), ``amplitude`` / ``phase`` / ``delay`` [E] (fp64), ``c1`` / ``c2`` [nA] (c2 may be null), ``detJ`` /
// ``dofmap`` [nA][N].  Set B (optional): ``cB``, ``detJB``, ``dmB`` of nB facets.  All device arrays, caller-owned.
template <typename T>
class FacetSourceArray {
 public:
  FacetSourceArray(const T* c1, const T* c2, const T* detJ, const int32_t* dofmap, const int32_t* eid, int64_t nA, const double* amplitude,
                   const double* phase, const double* delay, int64_t E, int N, const T* cB = nullptr, const T* detJB = nullptr,
                   const int32_t* dmB = nullptr, int64_t nB = 0)
      : c1_(c1), c2_(c2), detJ_(detJ), dm_(dofmap), eid_(eid), nA_(nA), a_(amplitude), ph_(phase), tau_(delay), E_(E), N_(N), cB_(cB),
        detJB_(detJB), dmB_(dmB), nB_(nB) {
    check_abi();
  }
  // y += set A at the stage block {t, w0, A, f0, alpha, D} (host memory) + set B applied to xB (ignored when nB == 0)
  void operator()(T* y, const double* stage, const T* xB = nullptr, void* stream = nullptr) const { launch(y, stage, false, xB, stream); }
  // the same with the stage block read from device memory by the kernel (hipGraph replay with new times)
  void device_stage(T* y, const double* stage_dev, const T* xB = nullptr, void* stream = nullptr) const {
    launch(y, stage_dev, true, xB, stream);
  }

 private:
  void launch(T* y, const double* stage, bool dev, const T* xB, void* stream) const {
    const auto entry = dev ? detail::typed<T>(fus_facet_source_array_dev_f64, fus_facet_source_array_dev_f32)
                           : detail::typed<T>(fus_facet_source_array_f64, fus_facet_source_array_f32);
    check(entry(y, c1_, c2_, detJ_, dm_, eid_, nA_, a_, ph_, tau_, E_, xB, cB_, detJB_, dmB_, xB ? nB_ : 0, N_, stage, stream),
          "fus_facet_source_array");
  }
  const T *c1_, *c2_, *detJ_;
  const int32_t *dm_, *eid_;
  int64_t nA_;
  const double *a_, *ph_, *tau_;
  int64_t E_;
  int N_;
  const T *cB_, *detJB_;
  const int32_t* dmB_;
  int64_t nB_;
};

// Point sources (fus_point_source_*): monopoles inside the volume, the transpose of PointProbe over the same tables (``cells`` [npts],
// the dofmap rows they index, ``weights`` [npts][3][P + 1]) with a per-point ``amplitude`` / ``phase`` / ``delay`` (fp64).  All device
// arrays, caller-owned.
template <typename T, int P>
class PointSource {
 public:
  PointSource(const int32_t* cells, int64_t npts, const int32_t* dofmap, int64_t ncells, const T* weights, const double* amplitude,
              const double* phase, const double* delay)
      : cells_(cells), npts_(npts), dofmap_(dofmap), ncells_(ncells), weights_(weights), a_(amplitude), ph_(phase), tau_(delay) {
    check_abi();
  }
  // y += the points' terms at the stage block {t, w0, A, f0, alpha, D} (host memory): after the facet terms, before the reverse scatter of y
  void operator()(T* y, const double* stage, void* stream = nullptr) const {
    check(detail::typed<T>(fus_point_source_f64, fus_point_source_f32)(y, cells_, npts_, dofmap_, ncells_, weights_, P, a_, ph_, tau_, stage,
                                                                       stream),
          "fus_point_source");
  }

 private:
  const int32_t* cells_;
  int64_t npts_;
  const int32_t* dofmap_;
  int64_t ncells_;
  const T* weights_;
  const double *a_, *ph_, *tau_;
};

// Element receivers (fus_element_receive_*): S_e = sum wgt[k] u[dof[k]] over the entries [offsets[e], offsets[e + 1]) of each of
// ``nelem`` elements (the facet-dof entries sorted by element, ``wgt`` their scaled facet detJ).  Not normalised: the area is sum wgt.
template <typename T>
class ElementReceive {
 public:
  ElementReceive(const int32_t* dof, const T* wgt, const int64_t* offsets, int64_t nelem) : dof_(dof), wgt_(wgt), offsets_(offsets), nelem_(nelem) {
    check_abi();
  }
  // row ``slot`` of rec[capacity][nelem] and H harmonic accumulators hre / him [H][nelem] with this step's factors coef [2H] (null = off)
  void operator()(const T* u, T* rec, int64_t capacity, int slot, double* hre = nullptr, double* him = nullptr, const double* coef = nullptr,
                  int H = 0, void* stream = nullptr) const {
    check(detail::typed<T>(fus_element_receive_f64, fus_element_receive_f32)(u, dof_, wgt_, offsets_, nelem_, rec, capacity, slot, hre, him, coef,
                                                                             H, stream),
          "fus_element_receive");
  }
  int64_t nelem() const { return nelem_; }

 private:
  const int32_t* dof_;
  const T* wgt_;
  const int64_t* offsets_;
  int64_t nelem_;
};

// Relaxation stage (fus_relax_stage_*): the streaming pass that advances the memory variables of ``nr`` relaxation mechanisms
// (xi' = kappa v - xi / tau) through one RK4 stage and writes ur = u_n + sum xi of the next stage.  ``tau`` / ``kappa_scalar`` [nr]: host
// arrays (fp64); ``kappa`` [nr][stride]: per-dof weights on the device, or null (then ``kappa_scalar``); ``xi0`` / ``xin`` / ``acc``
// [nr][stride]: the state on the device, caller-owned and zeroed by the caller before the first step.
template <typename T>
class RelaxStage {
 public:
  enum Kind { FIRST = 0, MIDDLE = 1, LAST = 2 };
  RelaxStage(int nr, const double* tau, const double* kappa_scalar, const T* kappa, T* xi0, T* xin, T* acc, int64_t stride, int64_t nlocal)
      : nr_(nr), tau_(tau), ks_(kappa_scalar), kappa_(kappa), xi0_(xi0), xin_(xin), acc_(acc), stride_(stride), nlocal_(nlocal) {
    check_abi();
  }
  // stage ``i`` in 0..3 of the step of length ``dt``: ur = (u_base + a_{i+1} dt vn) + sum of the next stage's variables.  Stages 0..2 run
  // BEFORE the stage's vector pass (u_base = u0, vn = the stage's v_n), stage 3 after it (u_base = the new u0, vn = the stage's v_n)
  void operator()(int i, double dt, const T* u_base, const T* vn, T* ur, void* stream = nullptr) const {
    static const double a[4] = {0.0, 0.5, 0.5, 1.0}, bq[4] = {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0};
    const int kind = i == 3 ? LAST : (i == 0 ? FIRST : MIDDLE);
    const T aw = (T)(i == 3 ? 0.0 : a[i + 1] * dt);
    check(detail::typed<T>(fus_relax_stage_f64, fus_relax_stage_f32)((T)(bq[i] * dt), aw, aw, kind, nr_, tau_, ks_, kappa_, xi0_, xin_, acc_, stride_,
                                                                     u_base, vn, ur, nlocal_, stream),
          "fus_relax_stage");
  }

 private:
  int nr_;
  const double *tau_, *ks_;
  const T* kappa_;
  T *xi0_, *xin_, *acc_;
  int64_t stride_, nlocal_;
};

}  // namespace fus_gpu

#endif /* FUS_GPU_HPP */
