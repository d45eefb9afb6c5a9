// smplpp::Measure over the C ABI — header-only C++ shim of the body measurements (smplpp_measure_create / smplpp_measure /
// smplpp_measure_vjp): the surface area and enclosed volume of regions of the posed mesh, and the length of the curve a plane cuts
// from a region.  No reference counterpart: the reference fits to markers and says nothing of the body's size.  A region is a list of
// 0-based face ids; a section pairs a plane with the region whose faces it cuts.
#ifndef SMPLPP_SHIM_MEASURE_H
#define SMPLPP_SHIM_MEASURE_H

#include "SMPL.h"

namespace smplpp
{
class Measure
{
public:
  // regions: lists of face ids (they may overlap; one may be empty; the order of a list is the order of its sums); sectionRegion [S]:
  // the region each plane cuts
  Measure(const SMPL & smpl, const std::vector<std::vector<int64_t>> & regions, const std::vector<int64_t> & sectionRegion = {})
      : V_(smpl.vertexNum()), R_((int64_t)regions.size()), S_((int64_t)sectionRegion.size())
  {
    std::vector<int64_t> ptr(1, 0), face;
    for(const auto & r : regions)
    {
      face.insert(face.end(), r.begin(), r.end());
      ptr.push_back((int64_t)face.size());
    }
    check(smplpp_measure_create(smpl.handle(), R_, ptr.data(), face.data(), S_, sectionRegion.data(), &h_), "Measure");
  }
  ~Measure() { smplpp_measure_destroy(h_); }
  Measure(const Measure &) = delete;
  Measure & operator=(const Measure &) = delete;

  int64_t regionNum() const { return R_; }
  int64_t sectionNum() const { return S_; }
  struct smplpp_measure * handle() const { return h_; }

  // area [N,R], volume [N,R], section [N,S], crossings [N,S] kInt64 (the faces each plane crosses) of verts [N,V,3].  planes [N,S,4]
  // or [1,S,4] (one set for every frame): rows (nx, ny, nz, d) of the planes n . x = d, used as given; undefined only when S = 0.
  // center [N,3] (undefined: zeros): the point the volume's cones are taken from.
  struct Result
  {
    Tensor area, volume, section, crossings;
  };
  Result evaluate(const Tensor & verts, const Tensor & planes = Tensor(), const Tensor & center = Tensor()) const
  {
    const char * what = "Cannot measure the mesh!";
    int64_t pf;
    const int64_t n = frames(verts, planes, center, pf, what);
    Result r{Tensor({n, R_}), Tensor({n, R_}), Tensor({n, S_}), Tensor({n, S_}, kInt64)};
    std::vector<int32_t> crossed((size_t)(n * S_));
    check(smplpp_measure(h_, n, verts.ptr(), center.defined() ? center.ptr() : nullptr, S_ ? planes.ptr() : nullptr, pf, r.area.ptr(),
                         r.volume.ptr(), S_ ? r.section.ptr() : nullptr, S_ ? crossed.data() : nullptr, SMPLPP_HOST, nullptr),
          "Measure");
    for(size_t i = 0; i < crossed.size(); i++) r.crossings.idata[i] = crossed[i];
    return r;
  }
  // Its backward pass: dL/dverts [N,V,3] and dL/dplanes (the shape of planes) for the cotangents gradArea [N,R], gradVolume [N,R] and
  // gradSection [N,S]; an undefined cotangent is left out.  `accumulate` non-null: the products are added into its tensors (and it
  // is returned).  center has no gradient: it is a constant of the definition.
  struct Gradients
  {
    Tensor verts, planes;
  };
  Gradients evaluateBackward(const Tensor & verts, const Tensor & planes, const Tensor & center, const Tensor & gradArea,
                             const Tensor & gradVolume, const Tensor & gradSection, Gradients * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the measurements!";
    int64_t pf;
    const int64_t n = frames(verts, planes, center, pf, what);
    const bool ga = gradArea.defined(), gv = gradVolume.defined(), gs = gradSection.defined() && S_ > 0;
    if((ga && (gradArea.dtype != kFloat32 || gradArea.numel() != n * R_)) || (gv && (gradVolume.dtype != kFloat32 || gradVolume.numel() != n * R_)) ||
       (gs && (gradSection.dtype != kFloat32 || gradSection.numel() != n * S_)))
      throw Exception("Measure", what);
    Gradients local;
    Gradients & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(out.verts.dtype != kFloat32 || out.verts.numel() != n * V_ * 3 || out.planes.dtype != kFloat32 || out.planes.numel() != pf * S_ * 4)
        throw Exception("Measure", what);
    }
    else
      out = Gradients{Tensor({n, V_, 3}), Tensor({pf, S_, 4})};
    check(smplpp_measure_vjp(h_, n, verts.ptr(), center.defined() ? center.ptr() : nullptr, S_ ? planes.ptr() : nullptr, pf,
                             ga ? gradArea.ptr() : nullptr, gv ? gradVolume.ptr() : nullptr, gs ? gradSection.ptr() : nullptr, out.verts.ptr(),
                             S_ ? out.planes.ptr() : nullptr, accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "Measure");
    return out;
  }

private:
  int64_t frames(const Tensor & verts, const Tensor & planes, const Tensor & center, int64_t & pf, const char * what) const
  {
    if(verts.dtype != kFloat32 || verts.numel() == 0 || verts.numel() % (V_ * 3) != 0) throw Exception("Measure", what);
    const int64_t n = verts.numel() / (V_ * 3);
    pf = 1;
    if(S_ > 0)
    {
      if(planes.dtype != kFloat32 || (planes.numel() != S_ * 4 && planes.numel() != n * S_ * 4)) throw Exception("Measure", what);
      pf = planes.numel() / (S_ * 4);
    }
    if(center.defined() && (center.dtype != kFloat32 || center.numel() != n * 3)) throw Exception("Measure", what);
    return n;
  }
  int64_t V_, R_, S_;
  struct smplpp_measure * h_ = nullptr;
};
} // namespace smplpp
#endif
