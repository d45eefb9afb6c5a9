// smplpp::alignPoints / alignPointsBackward over the C ABI — header-only C++ shim of the rigid and similarity alignment of point sets
// (smplpp_align, smplpp_align_vjp): per frame the R, t, s that minimise sum_k w_k |s R x_k + t - y_k|^2 over source [N,K,3], target
// [1 or N,K,3] and weight [1 or N,K], in closed form, with the gradient to both point sets.  The inner step of ICP before
// pointMeshDistance / meshPointDistance, and Procrustes-aligned evaluation.  No reference counterpart: the reference aligns nothing.
#ifndef SMPLPP_SHIM_ALIGN_H
#define SMPLPP_SHIM_ALIGN_H

#include "SMPL.h"

namespace smplpp
{
namespace detail
{
struct AlignShape
{
  int64_t n, K, Tn, Wn;
};
inline AlignShape alignShape(const Tensor & source, const Tensor & target, const Tensor & weight, const char * what)
{
  if(source.dtype != kFloat32 || source.dim() != 3 || source.size(2) != 3 || source.numel() == 0 || target.dtype != kFloat32)
    throw Exception("Align", what);
  AlignShape s{source.size(0), source.size(1), 1, 1};
  if(target.numel() != s.K * 3 && target.numel() != s.n * s.K * 3) throw Exception("Align", what);
  s.Tn = target.numel() == s.K * 3 ? 1 : s.n;
  if(weight.defined())
  {
    if(weight.dtype != kFloat32 || (weight.numel() != s.K && weight.numel() != s.n * s.K)) throw Exception("Align", what);
    s.Wn = weight.numel() == s.K ? 1 : s.n;
  }
  return s;
}
} // namespace detail

// transform [N,13] = R row-major, t, s; aligned [N,K,3] (every point moved); energy [N]; pointError [N,K]; gap [N]; status [N] kInt64
// (bit 0: no live point, bit 1: coincident source points, bit 2: gap <= minGap, the rotation is not unique)
struct Alignment
{
  Tensor transform, aligned, energy, pointError, gap, status;
};
inline Alignment alignPoints(const Tensor & source, const Tensor & target, const Tensor & weight = Tensor(), bool withScale = false,
                             float minGap = 1e-3f, int device = 0)
{
  const detail::AlignShape s = detail::alignShape(source, target, weight, "Cannot align the point sets!");
  Alignment r{Tensor({s.n, 13}), Tensor({s.n, s.K, 3}), Tensor({s.n}), Tensor({s.n, s.K}), Tensor({s.n}), Tensor({s.n}, kInt64)};
  std::vector<int32_t> st((size_t)s.n);
  check(smplpp_align(device, s.n, s.K, source.ptr(), target.ptr(), s.Tn, weight.defined() ? weight.ptr() : nullptr, s.Wn, withScale ? 1 : 0, minGap,
                     r.transform.ptr(), r.aligned.ptr(), r.energy.ptr(), r.pointError.ptr(), r.gap.ptr(), st.data(), SMPLPP_HOST, nullptr),
        "Align");
  r.status.idata.assign(st.begin(), st.end());
  return r;
}

// Its backward: dL/dsource [N,K,3] and dL/dtarget [N,K,3] (per frame: summed by the caller for a shared target) for dL/dtransform
// [N,13], dL/daligned [N,K,3] and dL/denergy [N] (an undefined one is left out).  `accumulate` non-null: the products are added into
// its tensors (and it is returned).
struct AlignGradients
{
  Tensor source, target;
};
inline AlignGradients alignPointsBackward(const Tensor & source, const Tensor & target, const Tensor & gradTransform, const Tensor & gradAligned,
                                          const Tensor & gradEnergy, const Tensor & weight = Tensor(), bool withScale = false,
                                          float minGap = 1e-3f, AlignGradients * accumulate = nullptr, int device = 0)
{
  const char * what = "Cannot back-propagate through the alignment!";
  const detail::AlignShape s = detail::alignShape(source, target, weight, what);
  const bool gt = gradTransform.defined(), ga = gradAligned.defined(), ge = gradEnergy.defined();
  if((gt && (gradTransform.dtype != kFloat32 || gradTransform.numel() != s.n * 13)) ||
     (ga && (gradAligned.dtype != kFloat32 || gradAligned.numel() != s.n * s.K * 3)) ||
     (ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != s.n)))
    throw Exception("Align", what);
  AlignGradients local;
  AlignGradients & out = accumulate ? *accumulate : local;
  if(accumulate)
  {
    if(out.source.dtype != kFloat32 || out.source.numel() != s.n * s.K * 3 || out.target.dtype != kFloat32 || out.target.numel() != s.n * s.K * 3)
      throw Exception("Align", what);
  }
  else
    out = AlignGradients{Tensor({s.n, s.K, 3}), Tensor({s.n, s.K, 3})};
  check(smplpp_align_vjp(device, s.n, s.K, source.ptr(), target.ptr(), s.Tn, weight.defined() ? weight.ptr() : nullptr, s.Wn, withScale ? 1 : 0,
                         minGap, gt ? gradTransform.ptr() : nullptr, ga ? gradAligned.ptr() : nullptr, ge ? gradEnergy.ptr() : nullptr,
                         out.source.ptr(), out.target.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
        "Align");
  return out;
}
} // namespace smplpp
#endif
