// smplpp::BatchedLbfgs over the C ABI — header-only C++ shim of the batched L-BFGS (smplpp_lbfgs_create / smplpp_lbfgs_step /
// smplpp_lbfgs_state / smplpp_lbfgs_best): n independent frames of D unknowns, each with its own history, line search and status; or,
// from the constructor that takes row counts (smplpp_lbfgs_create_grouped), P problems of consecutive rows, each with one history, line
// search and status for all its rows.
// No reference counterpart: the reference's fitting loop is the IK iteration of node/node.cpp.
#ifndef SMPLPP_SHIM_LBFGS_H
#define SMPLPP_SHIM_LBFGS_H

#include "SMPL.h"

namespace smplpp
{
// the options of smplpp_lbfgs_create, with their usual values
struct LbfgsOptions
{
  float c1 = 1e-4f, tolGrad = 1e-5f, tolF = 0.0f;
  int maxLs = 20;
  float curvEps = 1e-10f;
};

class BatchedLbfgs
{
public:
  using Options = LbfgsOptions;
  BatchedLbfgs(int64_t n, int64_t D, int64_t history = 10, const Options & o = Options(), int device = 0) : n_(n), D_(D), m_(history), P_(n)
  {
    check(smplpp_lbfgs_create(device, n, D, history, o.c1, o.tolGrad, o.tolF, o.maxLs, o.curvEps, &h_), "BatchedLbfgs");
  }
  // P = groups.size() problems: problem p is the groups[p] consecutive rows after those of problem p - 1 (the counts sum to n); f and
  // every array of state() then have P entries
  BatchedLbfgs(const std::vector<int64_t> & groups, int64_t D, int64_t history = 10, const Options & o = Options(), int device = 0)
      : n_(0), D_(D), m_(history), P_((int64_t)groups.size())
  {
    std::vector<int64_t> start(1, 0);
    for(int64_t rows : groups) start.push_back(n_ += rows);
    check(smplpp_lbfgs_create_grouped(device, n_, D, history, P_, start.data(), o.c1, o.tolGrad, o.tolF, o.maxLs, o.curvEps, &h_), "BatchedLbfgs");
  }
  ~BatchedLbfgs() { smplpp_lbfgs_destroy(h_); }
  BatchedLbfgs(const BatchedLbfgs &) = delete;
  BatchedLbfgs & operator=(const BatchedLbfgs &) = delete;

  int64_t frameNum() const { return n_; }
  int64_t problemNum() const { return P_; } // = frameNum() without groups
  int64_t dim() const { return D_; }
  int64_t history() const { return m_; }
  struct smplpp_lbfgs * handle() const { return h_; }

  // One evaluation: f [P] and g [n,D] are the energies and gradients at x [n,D], which is overwritten with the next points
  void step(Tensor & x, const Tensor & f, const Tensor & g)
  {
    if(x.dtype != kFloat32 || f.dtype != kFloat32 || g.dtype != kFloat32 || x.numel() != n_ * D_ || g.numel() != n_ * D_ || f.numel() != P_)
      throw Exception("BatchedLbfgs", "x [n,D], f [P] and g [n,D] are expected");
    check(smplpp_lbfgs_step(h_, x.ptr(), D_, f.ptr(), g.ptr(), D_, SMPLPP_HOST, nullptr), "BatchedLbfgs");
  }
  struct State
  {
    std::vector<int32_t> status, iterations, evaluations;
    Tensor fBest, step;
    int64_t running = 0;
  };
  State state() const
  {
    State s;
    s.status.resize((size_t)P_), s.iterations.resize((size_t)P_), s.evaluations.resize((size_t)P_);
    s.fBest = Tensor({P_}), s.step = Tensor({P_});
    check(smplpp_lbfgs_state(h_, s.status.data(), s.iterations.data(), s.evaluations.data(), s.fBest.ptr(), s.step.ptr(), &s.running, SMPLPP_HOST,
                             nullptr),
          "BatchedLbfgs");
    return s;
  }
  // every frame's last accepted point into x [n,D]; its energy is state().fBest
  void best(Tensor & x) const
  {
    if(x.dtype != kFloat32 || x.numel() != n_ * D_) throw Exception("BatchedLbfgs", "x [n,D] is expected");
    check(smplpp_lbfgs_best(h_, x.ptr(), D_, nullptr, SMPLPP_HOST, nullptr), "BatchedLbfgs");
  }
  void reset() { check(smplpp_lbfgs_reset(h_, nullptr), "BatchedLbfgs"); }

private:
  int64_t n_, D_, m_, P_;
  struct smplpp_lbfgs * h_ = nullptr;
};
} // namespace smplpp
#endif
