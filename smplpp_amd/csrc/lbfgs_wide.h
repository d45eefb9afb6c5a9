// What lbfgs.hip (the handle and the entry points) needs of lbfgs_wide.hip (the kernels of a grouped handle).
#pragma once
#include "common.h"
#include "lbfgs_wide_plan.h"

namespace smplpp_hip
{
// the device view of a grouped handle (lbfgs_wide_plan.h: LbfgsWideSizes)
struct LbfgsWideState
{
  int * ints;
  float *floats, *sy, *vec, *hist;
  const int * rows; // row_start [P+1]
  LbfgsOptions o;
  int64_t n;
  int P, D, m;
};

// one evaluation of every running problem: one kernel on `st` (device: the handle's, for the LDS opt-in)
hipError_t lbfgs_wide_step(int device, const LbfgsWideState & s, const LbfgsWideLaunch & L, float * x, int64_t ld_x, const float * f, const float * g,
                           int64_t ld_g, hipStream_t st);
// the accepted points into the caller's rows, and their energies into f [P] (nullable)
hipError_t lbfgs_wide_best(const LbfgsWideState & s, float * x, int64_t ld_x, float * f, hipStream_t st);
} // namespace smplpp_hip
