// The host tables of a pose prior: what smplpp_pose_prior_create (pose_prior.hip) computes from the caller's arrays before it uploads
// anything.  Plain C++17, no HIP: a CPU test runs the builder as a stand-alone program (tests/cpp/pose_prior_tables_dump.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace smplpp_hip
{
constexpr int64_t PRIOR_MAX_M = 32;
constexpr int64_t PRIOR_MAX_D = 128;

// The prior as the kernels read it.  mat [M][D][D] as given (row j = output j): the backward's lanes own k and read consecutive k.
// matT [M][D][D] with matT[m][k][j] = mat[m][j][k]: the forward's lanes own j and read consecutive j.
struct PosePriorTables
{
  const char * refusal = nullptr; // why the prior is refused, or null
  int64_t M = 0, D = 0;
  bool limits = false;
  std::vector<float> mean;   // [M][D]
  std::vector<float> mat;    // [M][D][D]
  std::vector<float> matT;   // [M][D][D]
  std::vector<float> offset; // [M]
  std::vector<float> lo, hi, weight; // [D] each, or empty
};

inline PosePriorTables pose_prior_tables(int64_t M, int64_t D, const float * mean, const float * mat, const float * offset, const float * lo,
                                         const float * hi, const float * limit_weight)
{
  PosePriorTables t;
  if(M < 0 || M > PRIOR_MAX_M) return t.refusal = "M must be in [0, 32]", t;
  if(D < 1 || D > PRIOR_MAX_D) return t.refusal = "D must be in [1, 128]", t;
  const bool any = lo || hi || limit_weight, all = lo && hi && limit_weight;
  if(any && !all) return t.refusal = "lo, hi and limit_weight must all be given or all be NULL", t;
  if(M == 0 && !all) return t.refusal = "a prior without components needs limits", t;
  if(M > 0 && (!mean || !mat || !offset)) return t.refusal = "mean, mat or offset is NULL", t;
  for(int64_t i = 0; i < M * D; i++)
    if(!std::isfinite(mean[i])) return t.refusal = "a mean is not finite", t;
  for(int64_t i = 0; i < M * D * D; i++)
    if(!std::isfinite(mat[i])) return t.refusal = "a mat is not finite", t;
  for(int64_t i = 0; i < M; i++)
    if(!std::isfinite(offset[i])) return t.refusal = "an offset is not finite", t;
  if(all)
    for(int64_t k = 0; k < D; k++)
    {
      if(std::isnan(lo[k]) || std::isnan(hi[k])) return t.refusal = "a limit is NaN", t;
      if(lo[k] > hi[k]) return t.refusal = "lo must not exceed hi", t;
      if(!(std::isfinite(limit_weight[k]) && limit_weight[k] >= 0.0f)) return t.refusal = "a limit_weight is negative or not finite", t;
    }
  t.M = M, t.D = D, t.limits = all;
  if(M > 0)
  {
    t.mean.assign(mean, mean + M * D);
    t.mat.assign(mat, mat + M * D * D);
    t.offset.assign(offset, offset + M);
    t.matT.resize((size_t)(M * D * D));
    for(int64_t m = 0; m < M; m++)
      for(int64_t j = 0; j < D; j++)
        for(int64_t k = 0; k < D; k++) t.matT[(size_t)((m * D + k) * D + j)] = mat[(m * D + j) * D + k];
  }
  if(all)
  {
    t.lo.assign(lo, lo + D);
    t.hi.assign(hi, hi + D);
    t.weight.assign(limit_weight, limit_weight + D);
  }
  return t;
}
} // namespace smplpp_hip
