// smplpp::orientationTerm / orientationTermBackward over the C ABI — header-only C++ shim of the orientation term on world joint
// frames (smplpp_orientation_term, smplpp_orientation_term_vjp): per frame and sensor s the residual E = A O - T of the 3 x 3 block A
// of joint joint[s] in frames [N,J,3,4] (SMPL::skeleton's world, read in place) or [N,J,3,3], through a bone-to-sensor offset O
// [S,3,C], against a target T [1 or N,S,3,C]; its energy w |E|^2 (the Geman-McClure form of it for rho > 0), the frame's energy, and
// the gradients to the frames, the offsets and the target.  C = 3 compares whole orientations (an IMU), C = 1 or 2 the images of
// bone-frame axes.  No reference counterpart: the reference has no orientation constraint.
#ifndef SMPLPP_SHIM_ORIENTATION_H
#define SMPLPP_SHIM_ORIENTATION_H

#include "SMPL.h"

namespace smplpp
{
namespace detail
{
struct OrientationShape
{
  int64_t n, J, rs, S, C, Tn, Wn;
};
inline OrientationShape orientationShape(const Tensor & frames, const Tensor & joint, const Tensor & target, const Tensor & offset,
                                         const Tensor & weight, int64_t C, const char * what)
{
  if(frames.dtype != kFloat32 || frames.dim() != 4 || frames.size(2) != 3 || (frames.size(3) != 3 && frames.size(3) != 4) || frames.numel() == 0 ||
     joint.dtype != kInt64 || joint.numel() == 0 || target.dtype != kFloat32 || C < 1 || C > 3)
    throw Exception("Orientation", what);
  OrientationShape s{frames.size(0), frames.size(1), frames.size(3), joint.numel(), C, 1, 1};
  const int64_t block = s.S * 3 * C;
  if(target.numel() != block && target.numel() != s.n * block) throw Exception("Orientation", what);
  s.Tn = target.numel() == block ? 1 : s.n;
  if(offset.defined() && (offset.dtype != kFloat32 || offset.numel() != block)) throw Exception("Orientation", what);
  if(weight.defined())
  {
    if(weight.dtype != kFloat32 || (weight.numel() != s.S && weight.numel() != s.n * s.S)) throw Exception("Orientation", what);
    s.Wn = weight.numel() == s.S ? 1 : s.n;
  }
  return s;
}
} // namespace detail

// energy [N]; sensorEnergy [N,S]; residual [N,S,3,C] = A O - T.  A dead sensor (weight 0 or not finite, a joint index outside [0, J), an
// entry that is not finite) gives +0 everywhere.
struct OrientationTerm
{
  Tensor energy, sensorEnergy, residual;
};
// frames [N,J,3,4] or [N,J,3,3]; joint [S] kInt64; target [1 or N,S,3,C]; offset [S,3,C] (undefined: the first C columns of the
// identity); weight [1 or N,S] (undefined: ones)
inline OrientationTerm orientationTerm(const Tensor & frames, const Tensor & joint, const Tensor & target, const Tensor & offset = Tensor(),
                                       const Tensor & weight = Tensor(), float rho = 0.0f, int64_t C = 3, int device = 0)
{
  const detail::OrientationShape s = detail::orientationShape(frames, joint, target, offset, weight, C, "Cannot evaluate the orientation term!");
  OrientationTerm r{Tensor({s.n}), Tensor({s.n, s.S}), Tensor({s.n, s.S, 3, s.C})};
  check(smplpp_orientation_term(device, s.n, s.J, s.rs, frames.ptr(), s.S, s.C, joint.idata.data(), offset.defined() ? offset.ptr() : nullptr,
                                target.ptr(), s.Tn, weight.defined() ? weight.ptr() : nullptr, s.Wn, rho, r.energy.ptr(), r.sensorEnergy.ptr(),
                                r.residual.ptr(), SMPLPP_HOST, nullptr),
        "Orientation");
  return r;
}

// Its backward: dL/dframes (the shape of frames; the 3 x 3 entries only: column 3 of an [N,J,3,4] tensor is never written, so the
// grad_world of SMPL::skeletonBackward can be passed as `accumulate`), dL/doffset [S,3,C] summed over the frames, and dL/dtarget
// [1 or N,S,3,C] (summed over the frames for a shared target), for dL/denergy [N], dL/dsensorEnergy [N,S] and dL/dresidual [N,S,3,C]
// (an undefined one is left out).  `accumulate` non-null: the products are added into its tensors (and it is returned).
struct OrientationGradients
{
  Tensor frames, offset, target;
};
inline OrientationGradients orientationTermBackward(const Tensor & frames, const Tensor & joint, const Tensor & target, const Tensor & gradEnergy,
                                                    const Tensor & gradSensorEnergy, const Tensor & gradResidual,
                                                    const Tensor & offset = Tensor(), const Tensor & weight = Tensor(), float rho = 0.0f,
                                                    int64_t C = 3, OrientationGradients * accumulate = nullptr, int device = 0)
{
  const char * what = "Cannot back-propagate through the orientation term!";
  const detail::OrientationShape s = detail::orientationShape(frames, joint, target, offset, weight, C, what);
  const bool ge = gradEnergy.defined(), gs = gradSensorEnergy.defined(), gr = gradResidual.defined();
  const int64_t block = s.S * 3 * s.C;
  if((ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != s.n)) ||
     (gs && (gradSensorEnergy.dtype != kFloat32 || gradSensorEnergy.numel() != s.n * s.S)) ||
     (gr && (gradResidual.dtype != kFloat32 || gradResidual.numel() != s.n * block)))
    throw Exception("Orientation", what);
  OrientationGradients local;
  OrientationGradients & out = accumulate ? *accumulate : local;
  if(accumulate)
  {
    if(out.frames.dtype != kFloat32 || out.frames.numel() != frames.numel() || out.offset.dtype != kFloat32 || out.offset.numel() != block ||
       out.target.dtype != kFloat32 || out.target.numel() != s.Tn * block)
      throw Exception("Orientation", what);
  }
  else
    out = OrientationGradients{Tensor({s.n, s.J, 3, s.rs}), Tensor({s.S, 3, s.C}), Tensor({s.Tn, s.S, 3, s.C})}; // (zeros: column 3 stays 0)
  check(smplpp_orientation_term_vjp(device, s.n, s.J, s.rs, frames.ptr(), s.S, s.C, joint.idata.data(), offset.defined() ? offset.ptr() : nullptr,
                                    target.ptr(), s.Tn, weight.defined() ? weight.ptr() : nullptr, s.Wn, rho, ge ? gradEnergy.ptr() : nullptr,
                                    gs ? gradSensorEnergy.ptr() : nullptr, gr ? gradResidual.ptr() : nullptr, out.frames.ptr(), out.offset.ptr(),
                                    out.target.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
        "Orientation");
  return out;
}
} // namespace smplpp
#endif
