// smplpp::PosePrior over the C ABI — header-only C++ shim of the pose priors (smplpp_pose_prior_create / smplpp_pose_prior /
// smplpp_pose_prior_vjp): a max-mixture Gaussian prior over D pose coordinates and one-sided quadratic joint limits.  No reference
// counterpart: the reference's only pose prior is the VPoser decoder (VPoser.h).
#ifndef SMPLPP_SHIM_POSE_PRIOR_H
#define SMPLPP_SHIM_POSE_PRIOR_H

#include "SMPL.h"

namespace smplpp
{
class PosePrior
{
public:
  // mean [M,D], mat [M,D,D] (row j = output j), offset [M]; lo, hi, limitWeight [D] or all three empty.  M = 0 needs limits.
  PosePrior(int64_t M, int64_t D, const std::vector<float> & mean, const std::vector<float> & mat, const std::vector<float> & offset,
            const std::vector<float> & lo = {}, const std::vector<float> & hi = {}, const std::vector<float> & limitWeight = {}, int device = 0)
      : M_(M), D_(D), limits_(!lo.empty())
  {
    const bool lim = !lo.empty() || !hi.empty() || !limitWeight.empty();
    if(M < 0 || D < 1 || (int64_t)mean.size() != M * D || (int64_t)mat.size() != M * D * D || (int64_t)offset.size() != M ||
       (lim && ((int64_t)lo.size() != D || (int64_t)hi.size() != D || (int64_t)limitWeight.size() != D)))
      throw Exception("PosePrior", "mean [M,D], mat [M,D,D], offset [M] and lo, hi, limitWeight [D] (or none) are expected");
    check(smplpp_pose_prior_create(device, M, D, mean.data(), mat.data(), offset.data(), lim ? lo.data() : nullptr, lim ? hi.data() : nullptr,
                                   lim ? limitWeight.data() : nullptr, &h_),
          "PosePrior");
  }
  ~PosePrior() { smplpp_pose_prior_destroy(h_); }
  PosePrior(const PosePrior &) = delete;
  PosePrior & operator=(const PosePrior &) = delete;

  int64_t componentNum() const { return M_; }
  int64_t dim() const { return D_; }
  bool hasLimits() const { return limits_; }
  struct smplpp_pose_prior * handle() const { return h_; }

  // energy [N], component [N] kInt64, residual [N,D] (with a mixture) and limitEnergy [N] (with limits) of pose [N,D], or of theta
  // [N,25,3] when the prior is over the 69 body-pose coordinates (read in place: offset 6, ld 75); a part the prior lacks is undefined
  struct Terms
  {
    Tensor energy, component, residual, limitEnergy;
  };
  Terms evaluate(const Tensor & pose) const
  {
    int64_t n, ld, off;
    rows(pose, n, ld, off, "Cannot evaluate the pose prior!");
    Terms r;
    if(M_ > 0) r.energy = Tensor({n}), r.component = Tensor({n}, kInt64), r.residual = Tensor({n, D_});
    if(limits_) r.limitEnergy = Tensor({n});
    check(smplpp_pose_prior(h_, n, pose.ptr() + off, ld, M_ > 0 ? r.energy.ptr() : nullptr, M_ > 0 ? r.component.idata.data() : nullptr,
                            M_ > 0 ? r.residual.ptr() : nullptr, limits_ ? r.limitEnergy.ptr() : nullptr, SMPLPP_HOST, nullptr),
          "PosePrior");
    return r;
  }
  // Its backward pass: dL/dpose in the layout of pose ([N,D], or [N,25,3] with zeros outside the body pose) for dL/denergy = gradEnergy
  // [N], dL/dresidual = gradResidual [N,D], dL/dlimitEnergy = gradLimitEnergy [N]; an undefined cotangent is left out.  `component`
  // [N] kInt64 fixes the components (undefined: chosen as evaluate does).  `accumulate` non-null: added into it (and it is returned).
  Tensor evaluateBackward(const Tensor & pose, const Tensor & gradEnergy, const Tensor & gradResidual, const Tensor & gradLimitEnergy,
                          const Tensor & component = Tensor(), Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the pose prior!";
    int64_t n, ld, off;
    rows(pose, n, ld, off, what);
    const bool ge = gradEnergy.defined(), gr = gradResidual.defined(), gl = gradLimitEnergy.defined(), cp = component.defined();
    if((ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != n)) || (gr && (gradResidual.dtype != kFloat32 || gradResidual.numel() != n * D_)) ||
       (gl && (gradLimitEnergy.dtype != kFloat32 || gradLimitEnergy.numel() != n)) || (cp && (component.dtype != kInt64 || component.numel() != n)))
      throw Exception("PosePrior", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(out.dtype != kFloat32 || out.numel() != pose.numel()) throw Exception("PosePrior", what);
    }
    else
      out = Tensor(pose.shape);
    check(smplpp_pose_prior_vjp(h_, n, pose.ptr() + off, ld, cp ? component.idata.data() : nullptr, ge ? gradEnergy.ptr() : nullptr,
                                gr ? gradResidual.ptr() : nullptr, gl ? gradLimitEnergy.ptr() : nullptr, out.ptr() + off, accumulate ? 1 : 0,
                                SMPLPP_HOST, nullptr),
          "PosePrior");
    return out;
  }

private:
  void rows(const Tensor & pose, int64_t & n, int64_t & ld, int64_t & off, const char * what) const
  {
    if(pose.dtype != kFloat32 || pose.numel() == 0) throw Exception("PosePrior", what);
    const bool theta = pose.dim() == 3 && pose.size(1) == JOINT_NUM + 1 && pose.size(2) == 3 && D_ == 3 * (JOINT_NUM - 1);
    ld = theta ? 3 * (JOINT_NUM + 1) : D_;
    off = theta ? 6 : 0;
    if(pose.numel() % ld != 0) throw Exception("PosePrior", what);
    n = pose.numel() / ld;
  }
  int64_t M_, D_;
  bool limits_;
  struct smplpp_pose_prior * h_ = nullptr;
};
} // namespace smplpp
#endif
