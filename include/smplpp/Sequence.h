// smplpp::SequenceLayout over the C ABI — header-only C++ shim of the sequence terms (smplpp_sequence_create / _split / _merge / _sum /
// _smoothness / _smoothness_vjp): what a caller of smplpp::BatchedLbfgs(groups, D) needs to make the rows of a problem a sequence.
// No reference counterpart: the reference fits frame by frame.
#ifndef SMPLPP_SHIM_SEQUENCE_H
#define SMPLPP_SHIM_SEQUENCE_H

#include "SMPL.h"

namespace smplpp
{
class SequenceLayout
{
public:
  // problem p owns groups[p] consecutive rows of the optimiser buffer; its last sharedRows (0 or 1) rows are not frames
  SequenceLayout(const std::vector<int64_t> & groups, int sharedRows = 0, int device = 0)
  {
    std::vector<int64_t> start(1, 0);
    for(int64_t rows : groups) start.push_back(start.back() + rows);
    check(smplpp_sequence_create(device, (int64_t)groups.size(), start.data(), sharedRows, &h_), "SequenceLayout");
    frameStart_.resize(groups.size() + 1);
    check(smplpp_sequence_info(h_, &P_, &rows_, &F_, &shared_, frameStart_.data()), "SequenceLayout");
  }
  ~SequenceLayout() { smplpp_sequence_destroy(h_); }
  SequenceLayout(const SequenceLayout &) = delete;
  SequenceLayout & operator=(const SequenceLayout &) = delete;

  int64_t problemNum() const { return P_; }
  int64_t rowNum() const { return rows_; }
  int64_t frameNum() const { return F_; }
  int sharedRows() const { return shared_; }
  const std::vector<int64_t> & frameStart() const { return frameStart_; }
  struct smplpp_sequence * handle() const { return h_; }

  // frames [F,Cf] = the coordinates [offF, offF + Cf) of every frame's row of rows [n,D]; shared [F,Cs] = the first Cs coordinates of the
  // shared row of the frame's problem (Cs = 0: left undefined)
  struct Parts
  {
    Tensor frames, shared;
  };
  Parts split(const Tensor & rows, int64_t offF, int64_t Cf, int64_t Cs = 0) const
  {
    const int64_t D = width(rows, "Cannot split the rows!");
    Parts r;
    r.frames = Tensor({F_, Cf});
    if(Cs > 0) r.shared = Tensor({F_, Cs});
    check(smplpp_sequence_split(h_, rows.ptr(), D, offF, Cf, r.frames.ptr(), Cs, Cs > 0 ? r.shared.ptr() : nullptr, SMPLPP_HOST, nullptr),
          "SequenceLayout");
    return r;
  }
  // its backward: gradRows [n,D] from gradFrames [F,Cf] and gradShared [F,Cs] (an undefined one is left out); `accumulate` non-null:
  // added into it (and it is returned)
  Tensor merge(const Tensor & gradFrames, int64_t offF, const Tensor & gradShared, int64_t D, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot merge the gradients!";
    const bool gf = gradFrames.defined(), gs = gradShared.defined();
    if((gf && (gradFrames.dtype != kFloat32 || gradFrames.numel() % F_)) || (gs && (gradShared.dtype != kFloat32 || gradShared.numel() % F_)))
      throw Exception("SequenceLayout", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(!accumulate) out = Tensor({rows_, D});
    else if(out.dtype != kFloat32 || out.numel() != rows_ * D)
      throw Exception("SequenceLayout", what);
    check(smplpp_sequence_merge(h_, gf ? gradFrames.ptr() : nullptr, offF, gf ? gradFrames.numel() / F_ : 0, gs ? gradShared.ptr() : nullptr,
                                gs ? gradShared.numel() / F_ : 0, out.ptr(), D, D, accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SequenceLayout");
    return out;
  }
  // problemValues [P] = scale * the sum of frameValues [F] over each problem's frames; `accumulate` non-null: added into it
  Tensor sum(const Tensor & frameValues, float scale = 1.0f, Tensor * accumulate = nullptr) const
  {
    if(frameValues.dtype != kFloat32 || frameValues.numel() != F_ || (accumulate && (accumulate->dtype != kFloat32 || accumulate->numel() != P_)))
      throw Exception("SequenceLayout", "frameValues [F] (and problem values [P]) are expected");
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(!accumulate) out = Tensor({P_});
    check(smplpp_sequence_sum(h_, frameValues.ptr(), scale, out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr), "SequenceLayout");
    return out;
  }

  // The temporal term of x [F,K,C]: first (order 1) or second (order 2) differences between consecutive frames of a problem, weight [K]
  // (undefined: ones), rho > 0 for the Geman-McClure form.  frameEnergy [F], pointEnergy [F,K]
  struct Energies
  {
    Tensor frameEnergy, pointEnergy;
  };
  Energies smoothness(const Tensor & x, int order = 1, const Tensor & weight = Tensor(), float rho = 0.0f) const
  {
    int64_t K, C;
    points(x, weight, K, C, "Cannot evaluate the smoothness term!");
    Energies r;
    r.frameEnergy = Tensor({F_}), r.pointEnergy = Tensor({F_, K});
    check(smplpp_sequence_smoothness(h_, x.ptr(), K * C, K, C, order, weight.defined() ? weight.ptr() : nullptr, rho, r.frameEnergy.ptr(),
                                     r.pointEnergy.ptr(), SMPLPP_HOST, nullptr),
          "SequenceLayout");
    return r;
  }
  // its backward: dL/dx [F,K,C] for dL/dframeEnergy [F] and dL/dpointEnergy [F,K] (an undefined one is left out); `accumulate` non-null:
  // added into it (and it is returned)
  Tensor smoothnessBackward(const Tensor & x, const Tensor & gradFrameEnergy, const Tensor & gradPointEnergy, int order = 1,
                            const Tensor & weight = Tensor(), float rho = 0.0f, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the smoothness term!";
    int64_t K, C;
    points(x, weight, K, C, what);
    const bool ge = gradFrameEnergy.defined(), gp = gradPointEnergy.defined();
    if((ge && (gradFrameEnergy.dtype != kFloat32 || gradFrameEnergy.numel() != F_)) ||
       (gp && (gradPointEnergy.dtype != kFloat32 || gradPointEnergy.numel() != F_ * K)))
      throw Exception("SequenceLayout", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(!accumulate) out = Tensor(x.shape);
    else if(out.dtype != kFloat32 || out.numel() != x.numel())
      throw Exception("SequenceLayout", what);
    check(smplpp_sequence_smoothness_vjp(h_, x.ptr(), K * C, K, C, order, weight.defined() ? weight.ptr() : nullptr, rho,
                                         ge ? gradFrameEnergy.ptr() : nullptr, gp ? gradPointEnergy.ptr() : nullptr, out.ptr(), accumulate ? 1 : 0,
                                         SMPLPP_HOST, nullptr),
          "SequenceLayout");
    return out;
  }

private:
  int64_t width(const Tensor & rows, const char * what) const
  {
    if(rows.dtype != kFloat32 || rows.numel() == 0 || rows.numel() % rows_) throw Exception("SequenceLayout", what);
    return rows.numel() / rows_;
  }
  void points(const Tensor & x, const Tensor & weight, int64_t & K, int64_t & C, const char * what) const
  {
    if(x.dtype != kFloat32 || x.dim() != 3 || x.size(0) != F_ || x.numel() == 0) throw Exception("SequenceLayout", what);
    K = x.size(1), C = x.size(2);
    if(weight.defined() && (weight.dtype != kFloat32 || weight.numel() != K)) throw Exception("SequenceLayout", what);
  }
  int64_t P_ = 0, rows_ = 0, F_ = 0;
  int shared_ = 0;
  std::vector<int64_t> frameStart_;
  struct smplpp_sequence * h_ = nullptr;
};
} // namespace smplpp
#endif
