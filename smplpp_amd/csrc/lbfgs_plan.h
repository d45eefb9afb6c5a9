// The host decisions of the batched L-BFGS (lbfgs.hip): what smplpp_lbfgs_create refuses, the ring arithmetic of a
// frame's history, the sizes of the handle's buffers and the launch of the step kernel, as functions of (n, D, m).  Plain C++17, no
// HIP: the kernel includes it for the ring arithmetic, and a CPU test runs it as a stand-alone program (tests/cpp/lbfgs_plan_dump.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace smplpp_hip
{
constexpr int LBFGS_MAX_M = 32;       // pairs of a frame's history at the most (a lane keeps alpha_i of pair i: at most 64)
constexpr int LBFGS_MAX_LS = 64;      // rejections in one line search at the most
constexpr int LBFGS_T = 256;          // threads of the step kernel
constexpr int LBFGS_FT = LBFGS_T / 64; // frames of a workgroup: one wavefront each
constexpr int LBFGS_LDS_D = 2048;     // up to this D the working vector of the two-loop recursion stays in LDS (8 KiB a frame)
constexpr int64_t LBFGS_INT32_MAX = 0x7fffffffLL;

struct LbfgsOptions
{
  float c1, tol_grad, tol_f;
  int max_ls;
  float curv_eps;
};

// why the options are refused, or null
inline const char * lbfgs_options_refusal(const LbfgsOptions & o)
{
  if(!(std::isfinite(o.c1) && o.c1 > 0.0f && o.c1 < 1.0f)) return "c1 must be in (0, 1)";
  if(!(std::isfinite(o.tol_grad) && o.tol_grad >= 0.0f)) return "tol_grad must be finite and not negative";
  if(!(std::isfinite(o.tol_f) && o.tol_f >= 0.0f)) return "tol_f must be finite and not negative";
  if(o.max_ls < 1 || o.max_ls > LBFGS_MAX_LS) return "max_ls must be in [1, 64]";
  if(!(std::isfinite(o.curv_eps) && o.curv_eps >= 0.0f && o.curv_eps < 1.0f)) return "curv_eps must be in [0, 1)";
  return nullptr;
}

// why the shape is refused, or null
inline const char * lbfgs_shape_refusal(int64_t n, int64_t D, int64_t m)
{
  if(n <= 0) return "n must be positive";
  if(D <= 0) return "D must be positive";
  if(m < 1 || m > LBFGS_MAX_M) return "m must be in [1, 32]";
  if(n > LBFGS_INT32_MAX || D > LBFGS_INT32_MAX || n * D > LBFGS_INT32_MAX || n * D * m > LBFGS_INT32_MAX) return "n * m * D beyond int32 indexing";
  return nullptr;
}

// why the rows of a caller's buffer are refused, or null
inline const char * lbfgs_rows_refusal(int64_t n, int64_t D, int64_t ld)
{
  if(ld < D) return "ld must be at least D";
  if(ld > LBFGS_INT32_MAX || n * ld > LBFGS_INT32_MAX) return "n * ld beyond int32 indexing";
  return nullptr;
}

// The history of a frame is a ring of m slots: `count` pairs, the oldest in slot `head`.  (constexpr: the kernel calls them too.)
// the slot of the i-th newest pair, i = 0 .. count-1
constexpr int lbfgs_ring_slot(int head, int count, int m, int i)
{
  return (head + count - 1 - i) % m;
}
// the slot a new pair is written to; then head and count are those after the push (a full ring loses its oldest pair)
constexpr int lbfgs_ring_push(int & head, int & count, int m)
{
  if(count < m) return (head + count++) % m;
  const int slot = head;
  head = (head + 1) % m;
  return slot;
}
// the history is dropped
constexpr void lbfgs_ring_drop(int & head, int & count)
{
  head = 0, count = 0;
}

// The handle's buffers.  ints [LBFGS_INTS][n] and floats [LBFGS_FLOATS][n] are the per-frame scalars, sy [n][m] the curvature of
// each slot, vec [LBFGS_VECS][n][D] the accepted point, its gradient and the direction, hist [2][n][m][D] the pairs (s, then y).
enum { LBFGS_STATUS, LBFGS_ITER, LBFGS_EVAL, LBFGS_LS, LBFGS_HEAD, LBFGS_COUNT, LBFGS_INTS };
enum { LBFGS_F0, LBFGS_STEP, LBFGS_GTD, LBFGS_GAMMA, LBFGS_FLOATS };
enum { LBFGS_X0, LBFGS_G0, LBFGS_DIR, LBFGS_VECS };
struct LbfgsSizes
{
  size_t ints, floats, sy, vec, hist; // elements
};
inline LbfgsSizes lbfgs_sizes(int64_t n, int64_t D, int64_t m)
{
  return LbfgsSizes{(size_t)(LBFGS_INTS * n), (size_t)(LBFGS_FLOATS * n), (size_t)(n * m), (size_t)(LBFGS_VECS * n * D), (size_t)(2 * n * m * D)};
}

// The step kernel's launch: LBFGS_FT frames a workgroup, and the working vector in LDS when D allows
struct LbfgsLaunch
{
  unsigned grid;
  int threads;
  bool lds_vector;
  size_t lds_bytes;
};
inline LbfgsLaunch lbfgs_launch(int64_t n, int64_t D)
{
  const bool lds = D <= LBFGS_LDS_D;
  return LbfgsLaunch{(unsigned)((n + LBFGS_FT - 1) / LBFGS_FT), LBFGS_T, lds, lds ? sizeof(float) * (size_t)(LBFGS_FT * D) : 0};
}
} // namespace smplpp_hip
