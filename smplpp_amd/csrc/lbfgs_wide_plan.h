// The host decisions of a grouped L-BFGS handle (smplpp_lbfgs_create_grouped, lbfgs.hip): P problems, problem p a run
// of consecutive rows row_start[p] .. row_start[p+1]-1 of the caller's x and g, carried by one workgroup of LBFGS_W_T threads under the
// 1024-partial sum rule.  What the entry point refuses, where a problem's blocks lie in the handle's buffers, the launch, where the
// working vector of the two-loop recursion lives, and the arithmetic by which a thread walks its elements j = t, t + 1024, ... of a
// problem through the caller's rows without a division per element.  Plain C++17, no HIP: the kernel includes it for the walk, and a CPU
// test runs it as a stand-alone program (tests/cpp/lbfgs_wide_plan_dump.cpp).  Options, ring arithmetic and the scalar enums are those of
// lbfgs_plan.h.
#pragma once

#include "lbfgs_plan.h"

namespace smplpp_hip
{
constexpr int LBFGS_W_T = 1024;              // threads of a problem's workgroup: one partial of the sum rule each
constexpr int64_t LBFGS_W_LDS_N = 32768;     // up to this N (the longest problem of the handle) the working vector stays in LDS (128 of the
                                             // compute unit's 160 KiB; above 64 KiB the launch opts in)

// why the groups are refused, or null (after lbfgs_shape_refusal(n, D, m) has passed)
inline const char * lbfgs_groups_refusal(int64_t n, int64_t P, const int64_t * row_start)
{
  if(P <= 0) return "P must be positive";
  if(!row_start) return "row_start is NULL";
  if(row_start[0] != 0) return "row_start[0] must be 0";
  for(int64_t p = 0; p < P; p++)
    if(row_start[p + 1] <= row_start[p]) return "row_start must strictly increase";
  if(row_start[P] != n) return "row_start[P] must be n";
  return nullptr;
}

// The handle's buffers.  ints [LBFGS_INTS][P] and floats [LBFGS_FLOATS][P] are the per-problem scalars, sy [P][m]; vec [LBFGS_VECS][n D]
// holds x0, g0 and d with problem p's N_p = rows_p D elements at row_start[p] D; hist holds problem p's ring in one block of 2 m N_p
// floats at 2 m D row_start[p], s of slot i at i N_p and y of slot i at (m + i) N_p inside it; rows [P+1] int32 is row_start.
struct LbfgsWideSizes
{
  size_t ints, floats, sy, vec, hist, rows; // elements
};
inline LbfgsWideSizes lbfgs_wide_sizes(int64_t n, int64_t D, int64_t m, int64_t P)
{
  return LbfgsWideSizes{(size_t)(LBFGS_INTS * P), (size_t)(LBFGS_FLOATS * P), (size_t)(P * m), (size_t)(LBFGS_VECS * n * D), (size_t)(2 * n * m * D),
                        (size_t)(P + 1)};
}
// where problem p's elements start in vector `which` of vec (n D <= int32 by lbfgs_shape_refusal, LBFGS_VECS n D by int64)
constexpr int64_t lbfgs_wide_vec_offset(int which, int64_t n, int64_t D, int64_t row0)
{
  return ((int64_t)which * n + row0) * D;
}
// where problem p's ring starts in hist, and slot i of s (y = 0) or of y (y = 1) inside it
constexpr int64_t lbfgs_wide_hist_offset(int64_t D, int64_t m, int64_t row0)
{
  return 2 * m * D * row0;
}
constexpr int64_t lbfgs_wide_slot_offset(int64_t N, int64_t m, int y, int slot)
{
  return ((int64_t)y * m + slot) * N;
}

// The grouped step kernel's launch: one workgroup per problem, and the working vector in LDS when the longest problem allows
inline LbfgsLaunch lbfgs_wide_launch(int64_t D, int64_t P, const int64_t * row_start)
{
  int64_t longest = 0;
  for(int64_t p = 0; p < P; p++)
    if(row_start[p + 1] - row_start[p] > longest) longest = row_start[p + 1] - row_start[p];
  const bool lds = longest * D <= LBFGS_W_LDS_N;
  return LbfgsLaunch{(unsigned)P, LBFGS_W_T, lds, lds ? sizeof(float) * (size_t)(longest * D) : 0};
}

// The walk of thread t through a problem's elements j = t, t + LBFGS_W_T, ...: element j is coordinate k = j mod D of the problem's row
// j / D, at `at` = (j / D) ld + k floats from the problem's first row in a caller's buffer of leading dimension ld.  One division when
// the walk starts; then a step adds the stride's constants and wraps k at most once.  (constexpr: the kernel calls them too.)
// (`at` in int64: the step past a problem's last element may leave the int32 range that n ld keeps.)
struct LbfgsWideStride
{
  int dk;       // LBFGS_W_T mod D
  int64_t wrap; // ld - D: what a wrap of k adds
  int64_t dat;  // (LBFGS_W_T / D) ld + dk
};
struct LbfgsWideCursor
{
  int k;
  int64_t at;
};
constexpr LbfgsWideStride lbfgs_wide_stride(int D, int64_t ld)
{
  return LbfgsWideStride{LBFGS_W_T % D, ld - D, (LBFGS_W_T / D) * ld + LBFGS_W_T % D};
}
constexpr LbfgsWideCursor lbfgs_wide_first(int t, int D, int64_t ld)
{
  return LbfgsWideCursor{t % D, (t / D) * ld + t % D};
}
constexpr void lbfgs_wide_advance(LbfgsWideCursor & c, const LbfgsWideStride & s, int D)
{
  c.k += s.dk, c.at += s.dat;
  if(c.k >= D) c.k -= D, c.at += s.wrap;
}
} // namespace smplpp_hip
