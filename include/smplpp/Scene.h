// smplpp::Volume over the C ABI — header-only C++ shim of the scene term (smplpp_volume_create / _set / _info / _sample,
// smplpp_scene_term / _vjp): a signed-distance grid of a static scene on the device, sampled at the body's points, with the penetration
// and contact energies and their gradient to the points.  No reference counterpart: the reference has no scene.
#ifndef SMPLPP_SHIM_SCENE_H
#define SMPLPP_SHIM_SCENE_H

#include "SMPL.h"

namespace smplpp
{
class Volume
{
public:
  // values [Gz,Gy,Gx]: node (i, j, k) holds values[k][j][i] and sits at origin + (i hx, j hy, k hz) in volume coordinates;
  // worldToVolume [12] (or [3,4]) row-major [R|t], undefined: the identity
  Volume(const Tensor & values, const std::vector<float> & origin, const std::vector<float> & spacing, const Tensor & worldToVolume = Tensor(),
         int device = 0)
  {
    const char * what = "Cannot create the volume!";
    if(values.dtype != kFloat32 || values.dim() != 3 || origin.size() != 3 || spacing.size() != 3) throw Exception("Volume", what);
    if(worldToVolume.defined() && (worldToVolume.dtype != kFloat32 || worldToVolume.numel() != 12)) throw Exception("Volume", what);
    check(smplpp_volume_create(device, values.size(2), values.size(1), values.size(0), origin.data(), spacing.data(),
                               worldToVolume.defined() ? worldToVolume.ptr() : nullptr, values.ptr(), SMPLPP_HOST, &h_),
          "Volume");
    check(smplpp_volume_info(h_, G_, nullptr, nullptr, nullptr, &layout_), "Volume");
  }
  ~Volume() { smplpp_volume_destroy(h_); }
  Volume(const Volume &) = delete;
  Volume & operator=(const Volume &) = delete;

  int64_t Gx() const { return G_[0]; }
  int64_t Gy() const { return G_[1]; }
  int64_t Gz() const { return G_[2]; }
  int layout() const { return layout_; } // 0: linear, 1: cells
  struct smplpp_volume * handle() const { return h_; }

  // new node values [Gz,Gy,Gx]
  void set(const Tensor & values)
  {
    if(values.dtype != kFloat32 || values.numel() != G_[0] * G_[1] * G_[2]) throw Exception("Volume", "Cannot set the volume's values!");
    check(smplpp_volume_set(h_, values.ptr(), SMPLPP_HOST, nullptr), "Volume");
  }

  // The volume at world points [N,K,3]: value [N,K], gradient [N,K,3] (d value / d point), valid [N,K] kInt64 0 / 1
  struct Sample
  {
    Tensor value, gradient, valid;
  };
  Sample sample(const Tensor & points) const
  {
    int64_t n, K;
    shape(points, Tensor(), Tensor(), n, K, "Cannot sample the volume!");
    Sample r{Tensor({n, K}), Tensor({n, K, 3}), Tensor({n, K}, kInt64)};
    std::vector<uint8_t> ok((size_t)(n * K));
    check(smplpp_volume_sample(h_, n, K, points.ptr(), r.value.ptr(), r.gradient.ptr(), ok.data(), SMPLPP_HOST, nullptr), "Volume");
    r.valid.idata.assign(ok.begin(), ok.end());
    return r;
  }

  // Penetration (wPen [K], undefined: ones) and contact (wCon [K], undefined: zeros; rho > 0 for the Geman-McClure form) of world points
  // [N,K,3]: energy [N], pointEnergy [N,K], value [N,K], valid [N,K] kInt64 0 / 1
  struct Term
  {
    Tensor energy, pointEnergy, value, valid;
  };
  Term term(const Tensor & points, const Tensor & wPen = Tensor(), const Tensor & wCon = Tensor(), float rho = 0.0f) const
  {
    int64_t n, K;
    shape(points, wPen, wCon, n, K, "Cannot evaluate the scene term!");
    Term r{Tensor({n}), Tensor({n, K}), Tensor({n, K}), Tensor({n, K}, kInt64)};
    std::vector<uint8_t> ok((size_t)(n * K));
    check(smplpp_scene_term(h_, n, K, points.ptr(), wPen.defined() ? wPen.ptr() : nullptr, wCon.defined() ? wCon.ptr() : nullptr, rho, r.energy.ptr(),
                            r.pointEnergy.ptr(), r.value.ptr(), ok.data(), SMPLPP_HOST, nullptr),
          "Volume");
    r.valid.idata.assign(ok.begin(), ok.end());
    return r;
  }
  // its backward: dL/dpoints [N,K,3] for dL/denergy [N], dL/dpointEnergy [N,K] and dL/dvalue [N,K] (an undefined one is left out);
  // `accumulate` non-null: added into it (and it is returned)
  Tensor termBackward(const Tensor & points, const Tensor & gradEnergy, const Tensor & gradPointEnergy, const Tensor & gradValue,
                      const Tensor & wPen = Tensor(), const Tensor & wCon = Tensor(), float rho = 0.0f, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the scene term!";
    int64_t n, K;
    shape(points, wPen, wCon, n, K, what);
    const bool ge = gradEnergy.defined(), gp = gradPointEnergy.defined(), gv = gradValue.defined();
    if((ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != n)) || (gp && (gradPointEnergy.dtype != kFloat32 || gradPointEnergy.numel() != n * K)) ||
       (gv && (gradValue.dtype != kFloat32 || gradValue.numel() != n * K)))
      throw Exception("Volume", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(!accumulate) out = Tensor({n, K, 3});
    else if(out.dtype != kFloat32 || out.numel() != n * K * 3)
      throw Exception("Volume", what);
    check(smplpp_scene_term_vjp(h_, n, K, points.ptr(), wPen.defined() ? wPen.ptr() : nullptr, wCon.defined() ? wCon.ptr() : nullptr, rho,
                                ge ? gradEnergy.ptr() : nullptr, gp ? gradPointEnergy.ptr() : nullptr, gv ? gradValue.ptr() : nullptr, out.ptr(),
                                accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "Volume");
    return out;
  }

private:
  void shape(const Tensor & points, const Tensor & wPen, const Tensor & wCon, int64_t & n, int64_t & K, const char * what) const
  {
    if(points.dtype != kFloat32 || points.dim() != 3 || points.size(2) != 3 || points.numel() == 0) throw Exception("Volume", what);
    n = points.size(0), K = points.size(1);
    if((wPen.defined() && (wPen.dtype != kFloat32 || wPen.numel() != K)) || (wCon.defined() && (wCon.dtype != kFloat32 || wCon.numel() != K)))
      throw Exception("Volume", what);
  }
  int64_t G_[3] = {0, 0, 0};
  int layout_ = 0;
  struct smplpp_volume * h_ = nullptr;
};
} // namespace smplpp
#endif
