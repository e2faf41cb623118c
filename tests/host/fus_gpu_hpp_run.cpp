// Runs every functor class of include/fus_gpu.hpp on the device, as a user of the header would, for tests/test_fus_gpu_hpp_gpu.py.
// Plain C++17, no kernels; linked against libfusgpu.so.  It holds no tolerance and no model: it reads a case file (the container of
// tests/golden/export_raw.py, entries named <group>.<array>; tests/hpp_cases.py writes it), uploads the inputs (stored as float64 and
// exact in T, so narrowing loses nothing), constructs and applies the functors of the groups it finds, and writes every output array,
// widened to float64, into a file of the same format.  One line per functor call goes to stdout.
//
//   fus_gpu_hpp_run <float|double> <P> <case file> <output file>
//   fus_gpu_hpp_run lifetime <float|double> <P> <case file>      construct / apply / destroy the owning functors 50 times on the "cell"
//                                                               group and print the free device memory; then the refused constructors
//
// Exit status: 0, or 2 with the text of the exception on stderr (a functor that threw, a HIP error: nothing is launched after one).
#include "../../include/fus_gpu.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

namespace {

constexpr double kSentinel = -7.25;

struct Entry {
  int dtype = 0;  // 0 float64, 1 int32, 2 int64
  int64_t count = 0;
  std::vector<char> bytes;
};
using Entries = std::vector<std::pair<std::string, Entry>>;

void hip(hipError_t e, const char* what) { fus_gpu::check_hip(e, what); }

std::map<std::string, Entry> load(const char* path) {
  std::map<std::string, Entry> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  char magic[8];
  int64_t n = 0;
  bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "FUSGOLD1", 8) == 0 && std::fread(&n, 8, 1, f) == 1;
  for (int64_t i = 0; ok && i < n; ++i) {
    char name[33] = {0};
    int32_t hdr[2];
    Entry e;
    ok = std::fread(name, 1, 32, f) == 32 && std::fread(hdr, 4, 2, f) == 2 && std::fread(&e.count, 8, 1, f) == 1 && e.count >= 0;
    if (!ok) break;
    e.dtype = hdr[0];
    const size_t padded = ((size_t)e.count * (e.dtype == 1 ? 4 : 8) + 7) / 8 * 8;
    e.bytes.resize(padded);
    ok = padded == 0 || std::fread(e.bytes.data(), 1, padded, f) == padded;
    out[name] = std::move(e);
  }
  std::fclose(f);
  if (!ok) throw std::runtime_error(std::string("not a case file: ") + path);
  return out;
}

void save(const char* path, const Entries& entries) {
  FILE* f = std::fopen(path, "wb");
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
  const int64_t n = (int64_t)entries.size();
  std::fwrite("FUSGOLD1", 1, 8, f);
  std::fwrite(&n, 8, 1, f);
  for (const auto& [name, e] : entries) {
    char nm[32] = {0};
    std::strncpy(nm, name.c_str(), 31);
    const int32_t hdr[2] = {e.dtype, 0};
    std::fwrite(nm, 1, 32, f);
    std::fwrite(hdr, 4, 2, f);
    std::fwrite(&e.count, 8, 1, f);
    if (!e.bytes.empty()) std::fwrite(e.bytes.data(), 1, e.bytes.size(), f);
  }
  if (std::fclose(f) != 0) throw std::runtime_error(std::string("cannot write ") + path);
}

// a device array of ``n`` elements, ``shift`` elements into its allocation (allocations are 256-byte aligned)
template <typename U>
struct Dev {
  U* base = nullptr;
  U* p = nullptr;
  size_t n = 0;
  Dev() = default;
  Dev(size_t count, size_t shift = 0) : n(count) {
    hip(hipMalloc(&base, sizeof(U) * (count + shift + 1)), "hipMalloc");
    p = base + shift;
  }
  Dev(const std::vector<U>& h, size_t shift = 0) : Dev(h.size(), shift) { put(h); }
  Dev(Dev&& o) noexcept : base(o.base), p(o.p), n(o.n) { o.base = o.p = nullptr; }
  Dev& operator=(Dev&& o) noexcept {
    std::swap(base, o.base);
    std::swap(p, o.p);
    std::swap(n, o.n);
    return *this;
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() {
    if (base) (void)hipFree(base);
  }
  void put(const std::vector<U>& h) {
    if (h.size() != n) throw std::runtime_error("upload of another size");
    if (n) hip(hipMemcpy(p, h.data(), sizeof(U) * n, hipMemcpyHostToDevice), "hipMemcpy (upload)");
  }
  std::vector<U> get() const {
    std::vector<U> h(n);
    if (n) hip(hipMemcpy(h.data(), p, sizeof(U) * n, hipMemcpyDeviceToHost), "hipMemcpy (download)");
    return h;
  }
};

template <typename T>
struct Run {
  const std::map<std::string, Entry>& in;
  Entries out;
  std::string type, group;
  int P;

  const Entry& entry(const std::string& name, int dtype) const {
    const auto it = in.find(group + "." + name);
    if (it == in.end() || it->second.dtype != dtype) throw std::runtime_error("case file: no entry " + group + "." + name + " of the expected type");
    return it->second;
  }
  bool has(const std::string& g) const { return in.lower_bound(g + ".") != in.end() && in.lower_bound(g + ".")->first.compare(0, g.size() + 1, g + ".") == 0; }
  int64_t count(const std::string& name) const { return in.at(group + "." + name).count; }
  std::vector<double> f64(const std::string& name) const {
    const Entry& e = entry(name, 0);
    const double* d = reinterpret_cast<const double*>(e.bytes.data());
    return std::vector<double>(d, d + e.count);
  }
  std::vector<T> host(const std::string& name) const {  // narrowed: the values are exact in T
    const std::vector<double> d = f64(name);
    return std::vector<T>(d.begin(), d.end());
  }
  int64_t scalar(const std::string& name) const { return reinterpret_cast<const int64_t*>(entry(name, 2).bytes.data())[0]; }
  Dev<T> up(const std::string& name, size_t shift = 0) const { return Dev<T>(host(name), shift); }
  Dev<double> upd(const std::string& name, size_t shift = 0) const { return Dev<double>(f64(name), shift); }
  Dev<int32_t> upi(const std::string& name) const {
    const Entry& e = entry(name, 1);
    const int32_t* d = reinterpret_cast<const int32_t*>(e.bytes.data());
    return Dev<int32_t>(std::vector<int32_t>(d, d + e.count));
  }
  Dev<int64_t> upl(const std::string& name) const {
    const Entry& e = entry(name, 2);
    const int64_t* d = reinterpret_cast<const int64_t*>(e.bytes.data());
    return Dev<int64_t>(std::vector<int64_t>(d, d + e.count));
  }
  // one functor call: its errors surface here, and its line is printed
  void done(const char* what) {
    hip(hipGetLastError(), what);
    hip(hipDeviceSynchronize(), what);
    std::printf("[%s P=%d] %s: %s\n", type.c_str(), P, group.c_str(), what);
  }
  template <typename U>
  void dump(const std::string& name, const std::vector<U>& h, size_t first = 0, size_t n = (size_t)-1) {
    if (n == (size_t)-1) n = h.size() - first;
    Entry e;
    e.count = (int64_t)n;
    e.bytes.resize(8 * n);
    double* d = reinterpret_cast<double*>(e.bytes.data());
    for (size_t i = 0; i < n; ++i) d[i] = (double)h[first + i];
    out.emplace_back(group + "." + name, std::move(e));
  }
  template <typename U>
  void dump(const std::string& name, const Dev<U>& a) { dump(name, a.get()); }
  // the rows of a [rows][stride] array: ``name`` gets the first ``n`` entries of the rows in ``keep``, ``rest`` everything else
  template <typename U>
  void dump_rows(const std::string& name, const std::string& rest, const Dev<U>& a, size_t rows, size_t stride, size_t n, const std::vector<bool>& keep) {
    const std::vector<U> h = a.get();
    std::vector<U> k, r;
    for (size_t i = 0; i < rows; ++i)
      for (size_t j = 0; j < stride; ++j) (keep[i] && j < n ? k : r).push_back(h[i * stride + j]);
    dump(name, k);
    if (!rest.empty()) dump(rest, r);
  }
};

template <typename T>
Dev<T> filled(size_t n, double v, size_t shift = 0) {
  return Dev<T>(std::vector<T>(n, (T)v), shift);
}

// ---- the cell functors that take the geometry -----------------------------------------------------------------------------------------
template <typename T, int P>
void cell(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "cell";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  const int64_t nc = r.count("dofmap") / Nd, nd = r.scalar("ndofs"), ystride = r.scalar("ystride");
  const auto x_g = r.up("x_g"), pts = r.up("pts"), wts = r.up("wts"), dphi = r.up("dphi"), dphi_p1 = r.up("dphi_p1"), w3 = r.up("w3"), cc = r.up("cc");
  const auto x_dofs = r.upi("x_dofs"), dm = r.upi("dofmap");
  const Geometry<T> geo{x_g.p, x_dofs.p, dphi_p1.p, w3.p};
  {
    StiffnessSpectral3D<T, P> K(dm.p, nc, geo, dphi.p);
    r.done("StiffnessSpectral3D(Geometry)");
    const auto x = r.up("xs");
    auto y = r.up("ys0");
    K(x.p, cc.p, y.p);
    r.done("StiffnessSpectral3D::operator()");
    r.dump("stiff", y);
    Dev<T> G((size_t)nc * Nd * 6);
    hip(hipMemcpy(G.p, K.G(), sizeof(T) * G.n, hipMemcpyDeviceToDevice), "hipMemcpy (G)");
    r.done("StiffnessSpectral3D::G()");
    r.dump("G", G);
  }
  {
    using Mass = MassSpectral3D<T, P>;
    std::vector<double> flags;
    const auto x = r.up("xm");
    Mass M(dm.p, nc, geo);
    r.done("MassSpectral3D(Geometry)");
    auto apply = [&](const char* name, const char* what, bool atomic) {
      auto y = r.up("ym0");
      if (atomic)
        M.apply_atomic(x.p, cc.p, y.p);
      else
        M(x.p, cc.p, y.p);
      r.done(what);
      r.dump(name, y);
      flags.push_back(M.gather_enabled());
      flags.push_back(M.static_detJ_enabled());
    };
    apply("mass_op", "MassSpectral3D::operator() [atomic kernel]", false);
    flags.clear();
    apply("mass_atomic", "MassSpectral3D::apply_atomic", true);
    M.enable_gather(dm.p, nd, nullptr, Mass::kStaticNever);
    r.done("MassSpectral3D::enable_gather(kStaticNever)");
    apply("mass_gather", "MassSpectral3D::operator() [gather]", false);
    M.enable_gather(dm.p, nd);
    r.done("MassSpectral3D::enable_gather() [owned detJ: static]");
    apply("mass_static", "MassSpectral3D::operator() [gather, static detJ]", false);
    r.dump("flags", flags);
  }
  {
    GradientSpectral3D<T, P> C(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p);
    r.done("GradientSpectral3D()");
    const auto x = r.up("xg");
    const std::vector<T> y0 = r.host("yg0");
    std::vector<T> h((size_t)3 * ystride, (T)kSentinel);
    for (int d = 0; d < 3; ++d)
      for (int64_t j = 0; j < nd; ++j) h[d * ystride + j] = y0[d * nd + j];
    Dev<T> y(h);
    C(x.p, cc.p, y.p, ystride);
    r.done("GradientSpectral3D::operator() [ystride > ndofs]");
    r.dump_rows("grad_gx", "", y, 3, ystride, nd, {true, false, false});
    r.dump_rows("grad_gy", "", y, 3, ystride, nd, {false, true, false});
    r.dump_rows("grad_gz", "", y, 3, ystride, nd, {false, false, true});
    h = y.get();
    std::vector<T> pad;
    for (int d = 0; d < 3; ++d) pad.insert(pad.end(), h.begin() + d * ystride + nd, h.begin() + (d + 1) * ystride);
    r.dump("grad_pad", pad);
  }
  {
    const auto nodal = r.up("nodal"), x = r.up("xn");
    NodalStiffnessSpectral3D<T, P> K(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, nodal.p);
    r.done("NodalStiffnessSpectral3D()");
    auto y = r.up("yn0");
    K(x.p, cc.p, y.p);
    r.done("NodalStiffnessSpectral3D::operator()");
    r.dump("nodal", y);
  }
  {
    const auto n3 = r.up("nodal3"), n4 = r.up("nodal4"), u = r.up("u"), v = r.up("v"), c3 = r.up("c3"), c4 = r.up("c4");
    WesterveltNodalStiffnessSpectral3D<T, P> K(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, n3.p, n4.p);
    r.done("WesterveltNodalStiffnessSpectral3D()");
    auto b = r.up("b0");
    K(u.p, v.p, c3.p, c4.p, b.p);
    r.done("WesterveltNodalStiffnessSpectral3D::operator()");
    r.dump("wnodal", b);
  }
}

// ---- Stiffness and Mass on factors the caller owns; enable_gather's rules for them ------------------------------------------------------
template <typename T, int P>
void colliding(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "coll";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  using Mass = MassSpectral3D<T, P>;
  const int64_t nc = r.count("dofmap") / Nd, nd = r.scalar("ndofs");
  const auto dm = r.upi("dofmap");
  const auto G = r.up("G"), detJ = r.up("detJ"), cc = r.up("cc"), dphi = r.up("dphi");
  {
    StiffnessSpectral3D<T, P> K(dm.p, nc, G.p, dphi.p);
    r.done("StiffnessSpectral3D(G)");
    const auto x = r.up("xs");
    auto y = r.up("ys0");
    K(x.p, cc.p, y.p);
    r.done("StiffnessSpectral3D::operator() [caller-owned G]");
    r.dump("stiff", y);
  }
  Mass M(dm.p, nc, detJ.p);
  r.done("MassSpectral3D(detJ)");
  const auto x = r.up("xm");
  std::vector<double> flags;
  auto apply = [&](const char* name, const char* what, bool atomic) {
    auto y = r.up("ym0");
    if (atomic)
      M.apply_atomic(x.p, cc.p, y.p);
    else
      M(x.p, cc.p, y.p);
    r.done(what);
    r.dump(name, y);
  };
  auto note = [&]() {
    flags.push_back(M.gather_enabled());
    flags.push_back(M.static_detJ_enabled());
  };
  apply("mass_atomic", "MassSpectral3D::apply_atomic [caller-owned detJ]", true);
  M.enable_gather(dm.p, nd);
  r.done("MassSpectral3D::enable_gather() [caller-owned detJ: no snapshot]");
  note();
  apply("mass_gather", M.gather_enabled() ? "MassSpectral3D::operator() [gather]" : "MassSpectral3D::operator() [gather declined: atomic kernel]", false);
  M.enable_gather(dm.p, nd, nullptr, Mass::kStaticAlways);
  r.done("MassSpectral3D::enable_gather(kStaticAlways)");
  note();
  apply("mass_static", "MassSpectral3D::operator() [kStaticAlways]", false);
  M.enable_gather(dm.p, nd, nullptr, Mass::kStaticAlways);
  r.done("MassSpectral3D::enable_gather() a second time");
  note();
  apply("mass_again", "MassSpectral3D::operator() [after the second enable_gather]", false);
  r.dump("flags", flags);
}

template <typename T>
void declined(Run<T>& r) {  // P = 1: one dof in 300 cells
  using namespace fus_gpu;
  r.group = "decl";
  const int64_t nc = r.count("dofmap") / 8, nd = r.scalar("ndofs");
  const auto dm = r.upi("dofmap");
  const auto detJ = r.up("detJ"), cc = r.up("cc"), x = r.up("x");
  MassSpectral3D<T, 1> M(dm.p, nc, detJ.p);
  M.enable_gather(dm.p, nd);
  r.done("MassSpectral3D::enable_gather() [a dof in more than 255 cells]");
  auto y = r.up("y0");
  M(x.p, cc.p, y.p);
  r.done("MassSpectral3D::operator() [gather declined: atomic kernel]");
  r.dump("mass", y);
  r.dump("flags", std::vector<double>{(double)M.gather_enabled(), (double)M.static_detJ_enabled()});
}

// ---- probe and point source ---------------------------------------------------------------------------------------------------------------
template <typename T, int P>
void probe(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "probe";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1), K = 3, H = 2, capacity = 4, slot = 2;
  const auto cells = r.upi("cells"), dm = r.upi("dofmap");
  const auto w = r.up("weights"), u = r.up("u");
  const int64_t npts = (int64_t)cells.n, nc = (int64_t)dm.n / Nd, nd = (int64_t)u.n / K;
  const PointProbe<T, P> pr(cells.p, npts, dm.p, nc, w.p);
  if (pr.npts() != npts) throw std::runtime_error("PointProbe::npts()");
  for (int k = 0; k < K; ++k) {
    Dev<T> o = filled<T>(npts, kSentinel);
    pr(u.p + k * nd, o.p);
    r.done("PointProbe::operator() [short form]");
    r.dump("short" + std::to_string(k), o);
  }
  Dev<T> rec = filled<T>((size_t)capacity * npts, kSentinel);
  auto pmax = r.upd("pmax"), pmin = r.upd("pmin"), hre = r.upd("hre"), him = r.upd("him");
  const auto coef = r.upd("coef");
  for (int k = 0; k < K; ++k) {
    pr(u.p + k * nd, rec.p, capacity, slot, pmax.p, pmin.p, hre.p, him.p, coef.p + 2 * H * k, H);
    r.done("PointProbe::operator() [capacity 4, slot 2, peaks, H = 2]");
  }
  r.dump_rows("rec_row", "rec_rest", rec, capacity, npts, npts, {false, false, true, false});
  r.dump("pmax", pmax);
  r.dump("pmin", pmin);
  r.dump("hre", hre);
  r.dump("him", him);
}

template <typename T, int P>
void point_source(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "psrc";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  const auto cells = r.upi("cells"), dm = r.upi("dofmap");
  const auto w = r.up("weights");
  const auto a = r.upd("amplitude"), ph = r.upd("phase"), tau = r.upd("delay");
  const std::vector<double> stage = r.f64("stage");
  const PointSource<T, P> ps(cells.p, (int64_t)cells.n, dm.p, (int64_t)dm.n / Nd, w.p, a.p, ph.p, tau.p);
  auto y = r.up("y0");
  ps(y.p, stage.data());
  r.done("PointSource::operator()");
  r.dump("y", y);
}

// ---- the degree-free functors -------------------------------------------------------------------------------------------------------------
template <typename T>
void facet(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "facet";
  const int N = (int)r.scalar("N");
  const auto c1 = r.up("c1"), c2 = r.up("c2"), detJ = r.up("detJ"), xB = r.up("xB"), cB = r.up("cB"), detJB = r.up("detJB");
  const auto dm = r.upi("dofmap"), eid = r.upi("eid"), dmB = r.upi("dmB");
  const auto a = r.upd("amplitude"), ph = r.upd("phase"), tau = r.upd("delay"), stage_dev = r.upd("stage");
  const std::vector<double> stage = r.f64("stage");
  const int64_t nA = (int64_t)c1.n, nB = (int64_t)cB.n, E = (int64_t)a.n;
  {
    const FacetSourceArray<T> fa(c1.p, c2.p, detJ.p, dm.p, eid.p, nA, a.p, ph.p, tau.p, E, N, cB.p, detJB.p, dmB.p, nB);
    auto y = r.up("y0");
    fa(y.p, stage.data());
    r.done("FacetSourceArray::operator() [c2; set B given, xB null]");
    r.dump("with_c2", y);
    y = r.up("y0");
    fa.device_stage(y.p, stage_dev.p);
    r.done("FacetSourceArray::device_stage [c2; set B given, xB null]");
    r.dump("with_c2_dev", y);
  }
  {
    const FacetSourceArray<T> fa(c1.p, nullptr, detJ.p, dm.p, eid.p, nA, a.p, ph.p, tau.p, E, N, cB.p, detJB.p, dmB.p, nB);
    auto y = r.up("y0");
    fa(y.p, stage.data(), xB.p);
    r.done("FacetSourceArray::operator() [no c2; set B with xB]");
    r.dump("no_c2", y);
  }
}

template <typename T>
void receive(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "recv";
  constexpr int H = 2, capacity = 3, slot = 1;
  const auto dof = r.upi("dof");
  const auto offsets = r.upl("offsets");
  const auto wgt = r.up("wgt"), u = r.up("u");
  const auto coef = r.upd("coef");
  auto hre = r.upd("hre"), him = r.upd("him");
  const int64_t E = (int64_t)offsets.n - 1;
  const ElementReceive<T> er(dof.p, wgt.p, offsets.p, E);
  if (er.nelem() != E) throw std::runtime_error("ElementReceive::nelem()");
  for (int k = 0; k < 2; ++k) {
    Dev<T> rec = filled<T>((size_t)capacity * E, kSentinel);
    er(u.p, rec.p, capacity, slot, hre.p, him.p, coef.p + 2 * H * k, H);
    r.done("ElementReceive::operator() [capacity 3, slot 1, H = 2]");
    r.dump_rows("rec" + std::to_string(k + 1), "rest" + std::to_string(k + 1), rec, capacity, E, E, {false, true, false});
  }
  r.dump("hre", hre);
  r.dump("him", him);
}

template <typename T>
void monitor(Run<T>& r, const char* group, size_t shift) {
  using namespace fus_gpu;
  r.group = group;
  constexpr int K = 3, H = 2;
  const std::vector<T> u = r.host("u"), v = r.host("v");
  const auto coef = r.upd("coef");
  const int64_t n = (int64_t)u.size() / K, hstride = r.scalar("hstride");
  auto pmax = filled<T>(n, kSentinel, shift), pmin = filled<T>(n, kSentinel, shift);
  auto usq = filled<double>(n, kSentinel, shift), vsq = filled<double>(n, kSentinel, shift);
  auto hre = filled<double>((size_t)H * hstride, kSentinel, shift), him = filled<double>((size_t)H * hstride, kSentinel, shift);
  const FieldAccumulator<T> fa(n, pmax.p, pmin.p, usq.p, vsq.p, hre.p, him.p, hstride, H);
  for (int k = 0; k < K; ++k) {
    const Dev<T> uk(std::vector<T>(u.begin() + k * n, u.begin() + (k + 1) * n), shift), vk(std::vector<T>(v.begin() + k * n, v.begin() + (k + 1) * n), shift);
    fa(uk.p, vk.p, coef.p + 2 * H * k, k == 0);
    r.done(k == 0 ? "FieldAccumulator::operator() [init, H = 2, hstride > n]" : "FieldAccumulator::operator() [H = 2, hstride > n]");
  }
  r.dump("pmax", pmax);
  r.dump("pmin", pmin);
  r.dump("usq", usq);
  r.dump("vsq", vsq);
  r.dump_rows("hre", "", hre, H, hstride, n, {true, true});
  r.dump_rows("him", "", him, H, hstride, n, {true, true});
  std::vector<double> pad;
  for (const auto* a : {&hre, &him}) {
    const std::vector<double> h = a->get();
    for (int i = 0; i < H; ++i) pad.insert(pad.end(), h.begin() + i * hstride + n, h.begin() + (i + 1) * hstride);
  }
  r.dump("pad", pad);
}

template <typename T>
void bioheat(Run<T>& r, const char* group, size_t shift) {
  using namespace fus_gpu;
  r.group = group;
  const std::vector<double> sc = r.f64("scalars");  // dt, gate, Ta
  const int64_t nlocal = r.scalar("nlocal"), ntotal = r.count("b");
  const auto minv = r.up("minv", shift), pr = r.up("pr", shift), s = r.up("s", shift);
  auto one = [&](const std::string& tag, int i, bool on, bool init) {
    auto b = r.up("b", shift), T0 = r.up("T0", shift), Tn = r.up("Tn", shift), acc = r.up("acc", shift), tmax = r.up("tmax", shift);
    auto cem = r.upd("cem43", shift);
    const BioheatStage<T> st(nlocal, ntotal, (T)sc[2], minv.p, on ? pr.p : nullptr, on ? s.p : nullptr, b.p, T0.p, Tn.p, acc.p, on ? cem.p : nullptr,
                             on ? tmax.p : nullptr);
    if (init)
      st(i, sc[0], (T)sc[1], true);
    else
      st(i, sc[0], (T)sc[1]);
    r.done(("BioheatStage::operator() stage " + std::to_string(i) + (on ? (init ? " [pr, s, cem43, tmax, init]" : " [pr, s, cem43, tmax]") : " [bare]")).c_str());
    r.dump(tag + ".T0", T0);
    r.dump(tag + ".Tn", Tn);
    r.dump(tag + ".acc", acc);
    r.dump(tag + ".b", b);
    r.dump(tag + ".tmax", tmax);
    r.dump(tag + ".cem43", cem);
  };
  for (int i = 0; i < 4; ++i) {
    one("full" + std::to_string(i), i, true, false);
    one("bare" + std::to_string(i), i, false, false);
  }
  one("init3", 3, true, true);
}

template <typename T>
void relax(Run<T>& r, const char* group, size_t shift) {
  using namespace fus_gpu;
  r.group = group;
  const std::vector<double> tau = r.f64("tau"), ks = r.f64("ks");
  const double dt = r.f64("dt")[0];
  const int64_t nlocal = r.scalar("nlocal"), stride = r.count("xi0") / 4;
  const std::vector<T> kappa = r.host("kappa"), xi0 = r.host("xi0"), xin = r.host("xin"), acc = r.host("acc");
  const auto u_base = r.up("u_base", shift), vn = r.up("vn", shift);
  for (int nr : {1, 4})
    for (int perdof : {1, 0})
      for (int i = 0; i < 4; ++i) {
        auto rows = [&](const std::vector<T>& h) { return Dev<T>(std::vector<T>(h.begin(), h.begin() + (size_t)nr * stride), shift); };
        const Dev<T> kd = rows(kappa);
        Dev<T> x0 = rows(xi0), xn = rows(xin), ac = rows(acc), ur = r.up("ur", shift);
        const RelaxStage<T> rs(nr, tau.data(), ks.data(), perdof ? kd.p : nullptr, x0.p, xn.p, ac.p, stride, nlocal);
        rs(i, dt, u_base.p, vn.p, ur.p);
        const std::string tag = "n" + std::to_string(nr) + (perdof ? "d" : "s") + std::to_string(i);
        r.done(("RelaxStage::operator() stage " + std::to_string(i) + " nr " + std::to_string(nr) + (perdof ? " [per-dof kappa]" : " [kappa null: kappa_scalar]")).c_str());
        r.dump(tag + ".xi0", x0);
        r.dump(tag + ".xin", xn);
        r.dump(tag + ".acc", ac);
        r.dump(tag + ".ur", ur);
      }
}

// three RK4 steps of M(rho C) T' = -K(k) T - M(w)(T - Ta) + g M(1) q: a stiffness apply with the cell constants -k, then the stage
template <typename T, int P>
void loop(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "loop";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  const int64_t nd = r.scalar("ndofs"), nc = r.count("dofmap") / Nd;
  const auto x_g = r.up("x_g"), dphi = r.up("dphi"), dphi_p1 = r.up("dphi_p1"), w3 = r.up("w3"), negk = r.up("negk"), minv = r.up("minv"), pr = r.up("pr"),
             s = r.up("s");
  const auto x_dofs = r.upi("x_dofs"), dm = r.upi("dofmap");
  const std::vector<double> gates = r.f64("gates"), sc = r.f64("scalars");  // [steps][4]; dt, Ta
  const StiffnessSpectral3D<T, P> K(dm.p, nc, Geometry<T>{x_g.p, x_dofs.p, dphi_p1.p, w3.p}, dphi.p);
  auto T0 = r.up("T");
  auto Tn = filled<T>(nd, 0.0), acc = filled<T>(nd, 0.0), b = filled<T>(nd, 0.0), tmax = filled<T>(nd, 0.0);
  auto cem = filled<double>(nd, 0.0);
  const BioheatStage<T> st(nd, nd, (T)sc[1], minv.p, pr.p, s.p, b.p, T0.p, Tn.p, acc.p, cem.p, tmax.p);
  for (size_t step = 0; step < gates.size() / 4; ++step)
    for (int i = 0; i < 4; ++i) {
      K(i == 0 ? T0.p : Tn.p, negk.p, b.p);
      st(i, sc[0], (T)gates[4 * step + i], step == 0);
      r.done("StiffnessSpectral3D::operator() + BioheatStage::operator() [composed RK4 loop]");
    }
  r.dump("T", T0);
  r.dump("cem43", cem);
  r.dump("tmax", tmax);
}

template <typename T, int P>
void run_degree(Run<T>& r) {
  if (r.has("cell")) cell<T, P>(r);
  if (r.has("coll")) colliding<T, P>(r);
  if (r.has("probe")) probe<T, P>(r);
  if (r.has("psrc")) point_source<T, P>(r);
  if (r.has("loop")) loop<T, P>(r);
}

// ---- lifetime: no leak over 50 rounds of the owning functors; a refused constructor releases what it had allocated ------------------------
size_t free_bytes() {
  size_t f = 0, t = 0;
  hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
  hip(hipMemGetInfo(&f, &t), "hipMemGetInfo");
  return f;
}

template <typename Make>
void refused(const char* what, Make make) {
  const size_t before = free_bytes();
  bool threw = false;
  try {
    make();
  } catch (const std::runtime_error& e) {
    threw = true;
    std::printf("refused %s: %s\n", what, e.what());
  }
  if (!threw) throw std::runtime_error(std::string(what) + ": a null dofmap was not refused");
  std::printf("refused %s: free bytes before %zu after %zu\n", what, before, free_bytes());
}

template <typename T, int P>
void lifetime(Run<T>& r) {
  using namespace fus_gpu;
  r.group = "cell";
  constexpr int Nd = (P + 1) * (P + 1) * (P + 1);
  const int64_t nc = r.count("dofmap") / Nd, nd = r.scalar("ndofs");
  const auto x_g = r.up("x_g"), pts = r.up("pts"), wts = r.up("wts"), dphi = r.up("dphi"), dphi_p1 = r.up("dphi_p1"), w3 = r.up("w3"), cc = r.up("cc"), x = r.up("xs"),
             nodal = r.up("nodal");
  const auto x_dofs = r.upi("x_dofs"), dm = r.upi("dofmap");
  auto y = filled<T>((size_t)3 * nd, 0.0);
  const Geometry<T> geo{x_g.p, x_dofs.p, dphi_p1.p, w3.p};
  size_t first = 0, last = 0;
  for (int round = 1; round <= 50; ++round) {
    {
      MassSpectral3D<T, P> M(dm.p, nc, geo);
      M.enable_gather(dm.p, nd);
      if (!M.gather_enabled() || !M.static_detJ_enabled()) throw std::runtime_error("lifetime: the gather plans were declined");
      M(x.p, cc.p, y.p);
      StiffnessSpectral3D<T, P> K(dm.p, nc, geo, dphi.p);
      K(x.p, cc.p, y.p);
      GradientSpectral3D<T, P> C(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p);
      C(x.p, cc.p, y.p, nd);
      NodalStiffnessSpectral3D<T, P> Kn(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, nodal.p);
      Kn(x.p, cc.p, y.p);
      WesterveltNodalStiffnessSpectral3D<T, P> Kw(dm.p, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, nodal.p, nodal.p);
      Kw(x.p, x.p, cc.p, cc.p, y.p);
      hip(hipDeviceSynchronize(), "lifetime round");
    }
    (round == 1 ? first : last) = free_bytes();
  }
  std::printf("lifetime: free bytes after round 1: %zu after round 50: %zu\n", first, last);
  // fus_plan_build refuses a null dofmap before any device work of its own -- after the functor's allocations (the plan workspace; G / detJ)
  const int32_t* none = nullptr;
  refused("MassSpectral3D(Geometry)", [&] { MassSpectral3D<T, P> f(none, nc, geo); });
  refused("MassSpectral3D(detJ)", [&] { MassSpectral3D<T, P> f(none, nc, x.p); });
  refused("StiffnessSpectral3D(Geometry)", [&] { StiffnessSpectral3D<T, P> f(none, nc, geo, dphi.p); });
  refused("StiffnessSpectral3D(G)", [&] { StiffnessSpectral3D<T, P> f(none, nc, x.p, dphi.p); });
  refused("GradientSpectral3D", [&] { GradientSpectral3D<T, P> f(none, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p); });
  refused("NodalStiffnessSpectral3D", [&] { NodalStiffnessSpectral3D<T, P> f(none, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, nodal.p); });
  refused("WesterveltNodalStiffnessSpectral3D",
          [&] { WesterveltNodalStiffnessSpectral3D<T, P> f(none, nc, x_g.p, x_dofs.p, pts.p, wts.p, dphi.p, nodal.p, nodal.p); });
}

template <typename T, int P>
void run_one(Run<T>& r, bool life) {
  if (life)
    lifetime<T, P>(r);
  else
    run_degree<T, P>(r);
}

template <typename T>
int run(const char* type, int P, const char* case_file, const char* out_file) {
  const std::map<std::string, Entry> in = load(case_file);
  Run<T> r{in, {}, type, "", P};
  const bool life = out_file == nullptr;
  switch (P) {
    case 1: run_one<T, 1>(r, life); break;
    case 2: run_one<T, 2>(r, life); break;
    case 3: run_one<T, 3>(r, life); break;
    case 4: run_one<T, 4>(r, life); break;
    case 5: run_one<T, 5>(r, life); break;
    case 6: run_one<T, 6>(r, life); break;
    case 7: run_one<T, 7>(r, life); break;
    case 8: run_one<T, 8>(r, life); break;
    case 9: run_one<T, 9>(r, life); break;
    case 10: run_one<T, 10>(r, life); break;
    default: throw std::runtime_error("P: 1 .. 10");
  }
  if (life) return 0;
  if (P == 1 && r.has("decl")) declined<T>(r);
  if (r.has("facet")) facet<T>(r);
  if (r.has("recv")) receive<T>(r);
  for (size_t shift = 0; shift < 2; ++shift) {  // 16-byte aligned; sliced one element in
    const char* tag = shift ? "s" : "a";
    if (r.has(std::string("mon_") + tag)) monitor<T>(r, (std::string("mon_") + tag).c_str(), shift);
    if (r.has(std::string("bio_") + tag)) bioheat<T>(r, (std::string("bio_") + tag).c_str(), shift);
    if (r.has(std::string("rel_") + tag)) relax<T>(r, (std::string("rel_") + tag).c_str(), shift);
  }
  save(out_file, r.out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const bool life = argc == 5 && std::strcmp(argv[1], "lifetime") == 0;
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s <float|double> <P> <case file> <output file>\n       %s lifetime <float|double> <P> <case file>\n", argv[0], argv[0]);
    return 64;
  }
  const char* type = argv[life ? 2 : 1];
  const int P = std::atoi(argv[life ? 3 : 2]);
  const char* case_file = argv[life ? 4 : 3];
  try {
    if (std::strcmp(type, "double") == 0) return run<double>(type, P, case_file, life ? nullptr : argv[4]);
    if (std::strcmp(type, "float") == 0) return run<float>(type, P, case_file, life ? nullptr : argv[4]);
    throw std::runtime_error("type: float or double");
  } catch (const std::exception& e) {  // a functor that threw, or a HIP error: nothing more is launched
    std::fprintf(stderr, "fus_gpu_hpp_run: %s\n", e.what());
    return 2;
  }
}
