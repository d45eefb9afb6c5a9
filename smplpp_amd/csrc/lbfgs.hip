// A batched L-BFGS with a device-side backtracking line search: n independent frames of D unknowns, each with its own
// history of m pairs, its own step length and its own status, all kept on the device between calls.  A handle from
// smplpp_lbfgs_create_grouped has P problems of consecutive rows, N = rows D unknowns each, where this one has n frames:
// the same entry points, state struct and buffers, the scalars [.][P].  The rule is in include/smplpp_hip.h; every fp32 operation below
// is rounded on its own (no contraction to FMA), every sum is one fixed-order sum, and there are no atomics.  The two step kernels each
// write the rule out for their team of threads, and hist has its own layout for each: one body and one layout for both were built,
// measured slower for frames and not kept ("One state, one file").
//
//  lbfgs_step_kernel       one wavefront per frame, LBFGS_FT frames a workgroup, no barrier: sums by sum64 (fixed_sum.h).  The working
//                          vector of the two-loop recursion lives in LDS when D <= LBFGS_LDS_D, else in the frame's direction row.
//  lbfgs_wide_step_kernel  one workgroup of 1024 threads per problem: sums by sum1024 (fixed_sum.h).  The working vector lives in LDS when
//                          the handle's longest problem has N <= LBFGS_W_LDS_N, else in the problem's direction block.
//  lbfgs_best_kernel, lbfgs_wide_best_kernel  the accepted points into the caller's rows: a flat grid over n D, or a workgroup per problem.
//  lbfgs_running_kernel    one workgroup counts the problems with status 0.
#include <vector>

#include "fixed_sum.h"
#include "lbfgs_wide_plan.h"
#include "staging.h"

#pragma clang fp contract(off)

struct smplpp_lbfgs
{
  int device = 0;
  int64_t n = 0, D = 0, m = 0;
  smplpp_hip::LbfgsOptions opt{};
  smplpp_hip::DevBuf ints, floats, sy, vec, hist; // lbfgs_plan.h: LbfgsSizes
  smplpp_hip::DevBuf running;                    // one int64: the count smplpp_lbfgs_state reports
  // a grouped handle: P problems, problem p the rows row_start[p] .. row_start[p+1]-1 (lbfgs_wide_plan.h); else P = n
  bool grouped = false;
  int64_t P = 0;
  std::vector<int64_t> row_start;
  smplpp_hip::DevBuf rows;        // row_start as int32, for the kernels (empty without groups)
  smplpp_hip::LbfgsLaunch launch{}; // the step kernel's launch, decided once
  smplpp_hip::Arena arena;        // staging of the host-space calls on this handle
};

namespace smplpp_hip
{
using Lbfgs = struct ::smplpp_lbfgs;

// the device view of a handle (lbfgs_plan.h: LbfgsSizes).  rows: row_start [P+1], or null for a handle without groups: problem p is row p,
// P = n and N = D
struct LbfgsState
{
  int * ints;
  float *floats, *sy, *vec, *hist;
  const int * rows;
  LbfgsOptions o;
  int64_t n, P;
  int D, m;
};

// grid: ceil(n / LBFGS_FT); dynamic LDS: LBFGS_FT * D floats when LDS_VECTOR.  A frame whose status is not 0 returns before it reads
// or writes anything of the caller's.  Lane l owns the coordinates k = l, l + 64, ... of every vector of its frame: partial l of each
// sum and the element-wise updates need those alone, so a frame's passes are ordered by its own wavefront's program order.  alpha_i
// stays in a register of lane i.  Each update of the working vector (q, then r) is folded into the pass that takes the next dot product,
// so the recursion over c pairs is 2 c + 1 passes over the working vector and 4 c rows of history.
template<bool LDS_VECTOR>
__global__ __launch_bounds__(LBFGS_T) void lbfgs_step_kernel(LbfgsState s, float * x, int64_t ld_x, const float * __restrict__ f,
                                                             const float * __restrict__ g, int64_t ld_g)
{
  extern __shared__ __attribute__((aligned(16))) float lb_smem[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, D = s.D, m = s.m;
  const int64_t n = s.n, frame = (int64_t)blockIdx.x * LBFGS_FT + w;
  if(frame >= n) return;
  int * I = s.ints + frame;     // scalar j of the frame: I[j n]
  float * F = s.floats + frame; // likewise
  if(I[LBFGS_STATUS * n] != 0) return;
  float * xr = x + frame * ld_x;
  const float * gr = g + frame * ld_g;
  float * x0 = s.vec + (LBFGS_X0 * n + frame) * D;
  float * g0 = s.vec + (LBFGS_G0 * n + frame) * D;
  float * dir = s.vec + (LBFGS_DIR * n + frame) * D;
  float * S = s.hist + frame * m * D; // without groups hist is [2][n][m][D]: the frame layout of §3.20 measured slower here
  float * Y = S + n * m * D;
  float * sy = s.sy + frame * m;
  const float fv = f[frame];
  const int evals = I[LBFGS_EVAL * n];

  // one pass over g: is it finite, max |g_k|, the partials of sum |g_k|
  int fin = fabsf(fv) < INFINITY;
  float gmax = 0.0f, pa = 0.0f;
#pragma unroll 4
  for(int k = lane; k < D; k += 64)
  {
    const float a = fabsf(gr[k]);
    fin &= a < INFINITY;
    gmax = fmaxf(gmax, a);
    pa = pa + a;
  }
  fin = __all(fin);
  gmax = max64_meet(gmax);

  if(evals == 0) // the first evaluation of the frame
  {
    if(lane == 0) I[LBFGS_EVAL * n] = 1, F[LBFGS_F0 * n] = fv;
#pragma unroll 4
    for(int k = lane; k < D; k += 64) x0[k] = xr[k];
    if(!fin || gmax <= s.o.tol_grad)
    {
      if(lane == 0) I[LBFGS_STATUS * n] = fin ? 1 : 4;
      return;
    }
    const float t = fminf(1.0f, 1.0f / sum64_meet(pa));
    float p = 0.0f;
#pragma unroll 4
    for(int k = lane; k < D; k += 64)
    {
      const float gk = gr[k], dk = -gk;
      g0[k] = gk, dir[k] = dk;
      p = p + gk * dk;
      xr[k] = x0[k] + t * dk;
    }
    const float gtd = sum64_meet(p);
    if(lane == 0) F[LBFGS_STEP * n] = t, F[LBFGS_GTD * n] = gtd, I[LBFGS_LS * n] = 0;
    return;
  }

  const float f0 = F[LBFGS_F0 * n], t = F[LBFGS_STEP * n];
  float gtd = F[LBFGS_GTD * n];
  if(lane == 0) I[LBFGS_EVAL * n] = evals + 1;
  if(!(fin && fv <= f0 + (s.o.c1 * t) * gtd)) // rejected
  {
    const int ls = I[LBFGS_LS * n] + 1;
    if(lane == 0) I[LBFGS_LS * n] = ls;
    if(ls > s.o.max_ls)
    {
      if(lane == 0) I[LBFGS_STATUS * n] = 3;
#pragma unroll 4
      for(int k = lane; k < D; k += 64) xr[k] = x0[k];
      return;
    }
    float tn = 0.5f * t;
    if(fabsf(fv) < INFINITY)
    {
      const float den = 2.0f * ((fv - f0) - gtd * t);
      if(den > 0.0f)
      {
        const float lo = 0.1f * t, hi = 0.5f * t;
        tn = -((gtd * t) * t) / den;
        if(!(tn >= lo)) tn = lo;
        if(tn > hi) tn = hi;
      }
    }
    if(lane == 0) F[LBFGS_STEP * n] = tn;
#pragma unroll 4
    for(int k = lane; k < D; k += 64) xr[k] = x0[k] + tn * dir[k];
    return;
  }

  // accepted: the pair, then the accepted point moves
  int head = I[LBFGS_HEAD * n], count = I[LBFGS_COUNT * n];
  float psy = 0.0f, pyy = 0.0f;
#pragma unroll 4
  for(int k = lane; k < D; k += 64)
  {
    const float sk = xr[k] - x0[k], yk = gr[k] - g0[k];
    psy = psy + sk * yk;
    pyy = pyy + yk * yk;
  }
  const float sy_new = sum64_meet(psy), yy = sum64_meet(pyy);
  const bool push = yy > 0.0f && sy_new > s.o.curv_eps * yy;
  float gamma = F[LBFGS_GAMMA * n];
  int slot = 0;
  if(push)
  {
    slot = lbfgs_ring_push(head, count, m);
    gamma = sy_new / yy;
    if(lane == 0) sy[slot] = sy_new, F[LBFGS_GAMMA * n] = gamma;
  }
#pragma unroll 4
  for(int k = lane; k < D; k += 64)
  {
    const float xk = xr[k], gk = gr[k];
    if(push) S[slot * D + k] = xk - x0[k], Y[slot * D + k] = gk - g0[k];
    x0[k] = xk, g0[k] = gk;
  }
  int status = 0;
  if(gmax <= s.o.tol_grad) status = 1;
  else if(s.o.tol_f > 0.0f && f0 - fv <= s.o.tol_f * fmaxf(fmaxf(fabsf(f0), fabsf(fv)), 1.0f))
    status = 2;
  if(lane == 0)
  {
    I[LBFGS_ITER * n] = I[LBFGS_ITER * n] + 1;
    F[LBFGS_F0 * n] = fv;
    I[LBFGS_STATUS * n] = status;
  }
  if(status == 0)
  {
    // the two-loop recursion.  v: q, then r; every pass first applies the update the pass before it found (v = v + c u), then sums
    float * v = LDS_VECTOR ? lb_smem + w * D : dir;
    float akeep = 0.0f, c = 0.0f;
    const float * u = nullptr;
    for(int i = 0; i < count; i++) // newest to oldest
    {
      const int sl = lbfgs_ring_slot(head, count, m, i);
      const float * si = S + sl * D;
      float p = 0.0f;
#pragma unroll 4
      for(int k = lane; k < D; k += 64)
      {
        const float qk = u ? v[k] - c * u[k] : gr[k];
        v[k] = qk;
        p = p + si[k] * qk;
      }
      c = sum64_meet(p) / sy[sl];
      if(lane == i) akeep = c;
      u = Y + sl * D;
    }
    if(count > 0)
    {
#pragma unroll 4
      for(int k = lane; k < D; k += 64) v[k] = gamma * (v[k] - c * u[k]);
    }
    else
#pragma unroll 4
      for(int k = lane; k < D; k += 64) v[k] = gr[k];
    u = nullptr;
    for(int i = count - 1; i >= 0; i--) // oldest to newest
    {
      const int sl = lbfgs_ring_slot(head, count, m, i);
      const float * yi = Y + sl * D;
      float p = 0.0f;
#pragma unroll 4
      for(int k = lane; k < D; k += 64)
      {
        float rk = v[k];
        if(u) rk = rk + c * u[k], v[k] = rk;
        p = p + yi[k] * rk;
      }
      c = __shfl(akeep, i) - sum64_meet(p) / sy[sl];
      u = S + sl * D;
    }
    float p = 0.0f;
#pragma unroll 4
    for(int k = lane; k < D; k += 64)
    {
      float rk = v[k];
      if(u) rk = rk + c * u[k];
      const float dk = -rk;
      dir[k] = dk;
      p = p + gr[k] * dk;
    }
    gtd = sum64_meet(p);
    if(!(gtd < 0.0f)) // not a descent direction: the history is dropped
    {
      lbfgs_ring_drop(head, count);
      p = 0.0f;
#pragma unroll 4
      for(int k = lane; k < D; k += 64)
      {
        const float gk = gr[k];
        dir[k] = -gk;
        p = p + gk * gk;
      }
      gtd = -sum64_meet(p);
    }
#pragma unroll 4
    for(int k = lane; k < D; k += 64) xr[k] = x0[k] + dir[k];
    if(lane == 0) F[LBFGS_STEP * n] = 1.0f, F[LBFGS_GTD * n] = gtd, I[LBFGS_LS * n] = 0;
  }
  if(lane == 0) I[LBFGS_HEAD * n] = head, I[LBFGS_COUNT * n] = count;
}

// grid: P; dynamic LDS: the longest problem's N floats when LDS_VECTOR.  Thread t owns the elements j = t, t + 1024, ... of every vector
// of its problem, that is partial t of every sum, so that the only traffic between threads is the meeting of the partials.  Every branch
// is decided by values all threads hold alike (the sums after a meeting, or scalars that every thread read before the first barrier and
// thread 0 writes after it), so the workgroup reaches every barrier whole; a stopped problem's workgroup reads its status and returns
// whole.  The handle's own vectors are contiguous per problem and indexed by j; the caller's rows are walked by the cursor of
// lbfgs_wide_plan.h.  The 2 c + 1 folded passes are those of lbfgs_step_kernel.
template<bool LDS_VECTOR>
__global__ __launch_bounds__(LBFGS_W_T) void lbfgs_wide_step_kernel(LbfgsState s, float * x, int64_t ld_x, const float * __restrict__ f,
                                                                    const float * __restrict__ g, int64_t ld_g)
{
  extern __shared__ __attribute__((aligned(16))) float lbw_smem[];
  __shared__ float cross[2][3][SUM1024_WAVES];
  const int t = threadIdx.x, lane = t & 63, P = s.P, p = blockIdx.x, D = s.D, m = s.m;
  int * I = s.ints + p;     // scalar j of the problem: I[j P]
  float * F = s.floats + p; // likewise
  if(I[LBFGS_STATUS * P] != 0) return;
  const int row0 = s.rows[p];
  const unsigned N = (unsigned)(s.rows[p + 1] - row0) * (unsigned)D;
  float * xr = x + row0 * ld_x;
  const float * gr = g + row0 * ld_g;
  float * x0 = s.vec + lbfgs_wide_vec_offset(LBFGS_X0, s.n, D, row0);
  float * g0 = s.vec + lbfgs_wide_vec_offset(LBFGS_G0, s.n, D, row0);
  float * dir = s.vec + lbfgs_wide_vec_offset(LBFGS_DIR, s.n, D, row0);
  float * S = s.hist + lbfgs_wide_hist_offset(D, m, row0);
  float * Y = S + lbfgs_wide_slot_offset(N, m, 1, 0);
  float * sy = s.sy + (int64_t)p * m;
  // every scalar of the problem is read here, by every thread, before the first barrier; thread 0 writes them after it
  const float fv = f[p], f0 = F[LBFGS_F0 * P], tstep = F[LBFGS_STEP * P];
  float gtd = F[LBFGS_GTD * P], gamma = F[LBFGS_GAMMA * P];
  const int evals = I[LBFGS_EVAL * P], ls0 = I[LBFGS_LS * P];
  int head = I[LBFGS_HEAD * P], count = I[LBFGS_COUNT * P];
  const LbfgsWideStride sx = lbfgs_wide_stride(D, ld_x), sg = lbfgs_wide_stride(D, ld_g);
  const LbfgsWideCursor cx0 = lbfgs_wide_first(t, D, ld_x), cg0 = lbfgs_wide_first(t, D, ld_g);
  int turn = 0;

  // one pass over g: max |g_j|, is anything not finite, the partials of sum |g_j|
  float a3[3] = {0.0f, fabsf(fv) < INFINITY ? 0.0f : 1.0f, 0.0f};
  {
    LbfgsWideCursor cg = cg0;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      const float a = fabsf(gr[cg.at]);
      if(!(a < INFINITY)) a3[1] = 1.0f;
      a3[0] = fmaxf(a3[0], a);
      a3[2] = a3[2] + a;
      lbfgs_wide_advance(cg, sg, D);
    }
  }
  sum1024_meet_many<3, 3u>(a3, cross, turn);
  const float gmax = a3[0];
  const bool fin = a3[1] == 0.0f;

  if(evals == 0) // the first evaluation of the problem
  {
    {
      LbfgsWideCursor cx = cx0;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        x0[j] = xr[cx.at];
        lbfgs_wide_advance(cx, sx, D);
      }
    }
    if(!fin || gmax <= s.o.tol_grad)
    {
      if(t == 0) I[LBFGS_EVAL * P] = 1, F[LBFGS_F0 * P] = fv, I[LBFGS_STATUS * P] = fin ? 1 : 4;
      return;
    }
    const float tt = fminf(1.0f, 1.0f / a3[2]);
    float pp = 0.0f;
    {
      LbfgsWideCursor cx = cx0, cg = cg0;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        const float gk = gr[cg.at], dk = -gk;
        g0[j] = gk, dir[j] = dk;
        pp = pp + gk * dk;
        xr[cx.at] = x0[j] + tt * dk;
        lbfgs_wide_advance(cx, sx, D);
        lbfgs_wide_advance(cg, sg, D);
      }
    }
    gtd = sum1024_meet_one(pp, cross, turn);
    if(t == 0) I[LBFGS_EVAL * P] = 1, F[LBFGS_F0 * P] = fv, F[LBFGS_STEP * P] = tt, F[LBFGS_GTD * P] = gtd, I[LBFGS_LS * P] = 0;
    return;
  }

  if(!(fin && fv <= f0 + (s.o.c1 * tstep) * gtd)) // rejected
  {
    const int ls = ls0 + 1;
    if(ls > s.o.max_ls)
    {
      LbfgsWideCursor cx = cx0;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        xr[cx.at] = x0[j];
        lbfgs_wide_advance(cx, sx, D);
      }
      if(t == 0) I[LBFGS_EVAL * P] = evals + 1, I[LBFGS_LS * P] = ls, I[LBFGS_STATUS * P] = 3;
      return;
    }
    float tn = 0.5f * tstep;
    if(fabsf(fv) < INFINITY)
    {
      const float den = 2.0f * ((fv - f0) - gtd * tstep);
      if(den > 0.0f)
      {
        const float lo = 0.1f * tstep, hi = 0.5f * tstep;
        tn = -((gtd * tstep) * tstep) / den;
        if(!(tn >= lo)) tn = lo;
        if(tn > hi) tn = hi;
      }
    }
    LbfgsWideCursor cx = cx0;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      xr[cx.at] = x0[j] + tn * dir[j];
      lbfgs_wide_advance(cx, sx, D);
    }
    if(t == 0) I[LBFGS_EVAL * P] = evals + 1, I[LBFGS_LS * P] = ls, F[LBFGS_STEP * P] = tn;
    return;
  }

  // accepted: the pair, then the accepted point moves
  float a2[2] = {0.0f, 0.0f};
  {
    LbfgsWideCursor cx = cx0, cg = cg0;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      const float sk = xr[cx.at] - x0[j], yk = gr[cg.at] - g0[j];
      a2[0] = a2[0] + sk * yk;
      a2[1] = a2[1] + yk * yk;
      lbfgs_wide_advance(cx, sx, D);
      lbfgs_wide_advance(cg, sg, D);
    }
  }
  sum1024_meet_many<2, 0u>(a2, cross, turn);
  const float sy_new = a2[0], yy = a2[1];
  const bool push = yy > 0.0f && sy_new > s.o.curv_eps * yy;
  int slot = -1;
  if(push)
  {
    slot = lbfgs_ring_push(head, count, m);
    gamma = sy_new / yy;
  }
  {
    float * sn = S + lbfgs_wide_slot_offset(N, m, 0, push ? slot : 0);
    float * yn = Y + lbfgs_wide_slot_offset(N, m, 0, push ? slot : 0);
    LbfgsWideCursor cx = cx0, cg = cg0;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      const float xk = xr[cx.at], gk = gr[cg.at];
      if(push) sn[j] = xk - x0[j], yn[j] = gk - g0[j];
      x0[j] = xk, g0[j] = gk;
      lbfgs_wide_advance(cx, sx, D);
      lbfgs_wide_advance(cg, sg, D);
    }
  }
  int status = 0;
  if(gmax <= s.o.tol_grad) status = 1;
  else if(s.o.tol_f > 0.0f && f0 - fv <= s.o.tol_f * fmaxf(fmaxf(fabsf(f0), fabsf(fv)), 1.0f))
    status = 2;
  if(t == 0)
  {
    I[LBFGS_EVAL * P] = evals + 1;
    I[LBFGS_ITER * P] = I[LBFGS_ITER * P] + 1;
    F[LBFGS_F0 * P] = fv;
    I[LBFGS_STATUS * P] = status;
    if(push) sy[slot] = sy_new, F[LBFGS_GAMMA * P] = gamma;
  }
  if(status == 0)
  {
    // the two-loop recursion on g0 = g.  v: q, then r; every pass first applies the update the pass before it found (v = v + c u), then
    // sums.  (sy of the slot just written is in sy_new: only thread 0 wrote it to memory.)
    float * v = LDS_VECTOR ? lbw_smem : dir;
    float akeep = 0.0f, c = 0.0f;
    const float * u = nullptr;
    for(int i = 0; i < count; i++) // newest to oldest
    {
      const int sl = lbfgs_ring_slot(head, count, m, i);
      const float * si = S + lbfgs_wide_slot_offset(N, m, 0, sl);
      float pp = 0.0f;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        const float qk = u ? v[j] - c * u[j] : g0[j];
        v[j] = qk;
        pp = pp + si[j] * qk;
      }
      c = sum1024_meet_one(pp, cross, turn) / (sl == slot ? sy_new : sy[sl]);
      if(lane == i) akeep = c;
      u = Y + lbfgs_wide_slot_offset(N, m, 0, sl);
    }
    if(count > 0)
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T) v[j] = gamma * (v[j] - c * u[j]);
    else
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T) v[j] = g0[j];
    u = nullptr;
    for(int i = count - 1; i >= 0; i--) // oldest to newest
    {
      const int sl = lbfgs_ring_slot(head, count, m, i);
      const float * yi = Y + lbfgs_wide_slot_offset(N, m, 0, sl);
      float pp = 0.0f;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        float rk = v[j];
        if(u) rk = rk + c * u[j], v[j] = rk;
        pp = pp + yi[j] * rk;
      }
      c = __shfl(akeep, i) - sum1024_meet_one(pp, cross, turn) / (sl == slot ? sy_new : sy[sl]);
      u = S + lbfgs_wide_slot_offset(N, m, 0, sl);
    }
    float pp = 0.0f;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      float rk = v[j];
      if(u) rk = rk + c * u[j];
      const float dk = -rk;
      dir[j] = dk;
      pp = pp + g0[j] * dk;
    }
    gtd = sum1024_meet_one(pp, cross, turn);
    if(!(gtd < 0.0f)) // not a descent direction: the history is dropped
    {
      lbfgs_ring_drop(head, count);
      pp = 0.0f;
#pragma unroll 4
      for(unsigned j = t; j < N; j += LBFGS_W_T)
      {
        const float gk = g0[j];
        dir[j] = -gk;
        pp = pp + gk * gk;
      }
      gtd = -sum1024_meet_one(pp, cross, turn);
    }
    LbfgsWideCursor cx = cx0;
#pragma unroll 4
    for(unsigned j = t; j < N; j += LBFGS_W_T)
    {
      xr[cx.at] = x0[j] + dir[j];
      lbfgs_wide_advance(cx, sx, D);
    }
    if(t == 0) F[LBFGS_STEP * P] = 1.0f, F[LBFGS_GTD * P] = gtd, I[LBFGS_LS * P] = 0;
  }
  if(t == 0) I[LBFGS_HEAD * P] = head, I[LBFGS_COUNT * P] = count;
}

// The accepted points into the caller's rows: x, f the caller's; f may be null.  A problem that has not been evaluated yet has no accepted
// point: left alone.  Without groups, grid: ceil(n D / 256)
__global__ __launch_bounds__(256) void lbfgs_best_kernel(LbfgsState s, float * __restrict__ x, int64_t ld_x, float * __restrict__ f)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if(i >= s.n * s.D) return;
  const int64_t frame = i / s.D, k = i % s.D;
  if(s.ints[LBFGS_EVAL * s.P + frame] == 0) return;
  x[frame * ld_x + k] = s.vec[LBFGS_X0 * s.n * s.D + i];
  if(f && k == 0) f[frame] = s.floats[LBFGS_F0 * s.P + frame];
}

// with groups, grid: P
__global__ __launch_bounds__(256) void lbfgs_wide_best_kernel(LbfgsState s, float * __restrict__ x, int64_t ld_x, float * __restrict__ f)
{
  const int p = blockIdx.x, D = s.D;
  if(s.ints[LBFGS_EVAL * s.P + p] == 0) return;
  const int row0 = s.rows[p];
  const unsigned N = (unsigned)(s.rows[p + 1] - row0) * (unsigned)D;
  const float * x0 = s.vec + lbfgs_wide_vec_offset(LBFGS_X0, s.n, D, row0);
  for(unsigned j = threadIdx.x; j < N; j += 256) x[(row0 + (int64_t)(j / D)) * ld_x + j % D] = x0[j];
  if(f && threadIdx.x == 0) f[p] = s.floats[LBFGS_F0 * s.P + p];
}

// one workgroup of 256: *running = the number of problems with status 0
__global__ __launch_bounds__(256) void lbfgs_running_kernel(LbfgsState s, int64_t * running)
{
  __shared__ int part[4];
  int c = 0;
  for(int64_t i = threadIdx.x; i < s.P; i += 256) c += s.ints[LBFGS_STATUS * s.P + i] == 0;
  for(int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if(threadIdx.x == 0) *running = (int64_t)part[0] + part[1] + part[2] + part[3];
}

static LbfgsState lb_state(const Lbfgs * o)
{
  return LbfgsState{o->ints.as<int>(), o->floats.as<float>(), o->sy.as<float>(), o->vec.as<float>(), o->hist.as<float>(), o->rows.as<int>(),
                    o->opt,            o->n,                  o->P,              (int)o->D,          (int)o->m};
}

// one evaluation of every running problem: one kernel on `st`, chosen by the handle's kind and by where the working vector lives
static hipError_t lb_step(const Lbfgs * o, float * x, int64_t ld_x, const float * f, const float * g, int64_t ld_g, hipStream_t st)
{
  const LbfgsLaunch & L = o->launch;
  void (*kernel)(LbfgsState, float *, int64_t, const float *, const float *, int64_t) =
    o->grouped ? (L.lds_vector ? lbfgs_wide_step_kernel<true> : lbfgs_wide_step_kernel<false>)
               : (L.lds_vector ? lbfgs_step_kernel<true> : lbfgs_step_kernel<false>);
  if(L.lds_bytes > 64 * 1024) // only lbfgs_wide_step_kernel<true> asks for so much: its largest working vector, once per device
  {
    static PerDeviceOnce once;
    if(hipError_t e = lds_opt_in(once, o->device, reinterpret_cast<const void *>(kernel), (int)(sizeof(float) * LBFGS_W_LDS_N))) return e;
  }
  kernel<<<dim3(L.grid), dim3(L.threads), L.lds_bytes, st>>>(lb_state(o), x, ld_x, f, g, ld_g);
  return hipGetLastError();
}

// every scalar of every frame (of every problem: P of them, P = n without groups) to zero: status 0 (running), no evaluation yet, an
// empty ring
static hipError_t lb_clear(Lbfgs * o, hipStream_t st)
{
  const LbfgsSizes z = lbfgs_sizes(o->P, o->D, o->m);
  hipError_t e = hipMemsetAsync(o->ints.p.get(), 0, sizeof(int) * z.ints, st);
  if(e == hipSuccess) e = hipMemsetAsync(o->floats.p.get(), 0, sizeof(float) * z.floats, st);
  if(e == hipSuccess) e = hipMemsetAsync(o->sy.p.get(), 0, sizeof(float) * z.sy, st);
  return e;
}

// what the calls on rows of the caller's refuse alike
static int lb_check_rows(const char * fn, Lbfgs * o, const void * x, int64_t ld_x, int space)
{
  if(!o) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no optimiser");
  if(const char * why = lbfgs_rows_refusal(o->n, o->D, ld_x)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
  if(!x) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": x is NULL");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// row_start: null for a handle without groups (every row its own frame), else P + 1 row numbers
static int lb_create(const char * fn, int device, int64_t n, int64_t D, int64_t m, int64_t P, const int64_t * row_start, bool grouped,
                     const LbfgsOptions & opt, struct smplpp_lbfgs ** out)
{
  if(!out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no out");
  *out = nullptr;
  if(const char * why = lbfgs_shape_refusal(n, D, m)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
  if(const char * why = lbfgs_options_refusal(opt)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
  if(grouped)
    if(const char * why = lbfgs_groups_refusal(n, P, row_start)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<Lbfgs> o(new Lbfgs());
  o->device = device, o->n = n, o->D = D, o->m = m, o->opt = opt, o->grouped = grouped, o->P = grouped ? P : n;
  o->launch = grouped ? lbfgs_wide_launch(D, P, row_start) : lbfgs_launch(n, D);
  const LbfgsSizes z = lbfgs_sizes(n, D, m); // (vec and hist are as large with groups: lbfgs_wide_sizes)
  const LbfgsSizes zs = lbfgs_sizes(o->P, D, m);
  HIP_TRY(o->ints.reserve(sizeof(int) * zs.ints));
  HIP_TRY(o->floats.reserve(sizeof(float) * zs.floats));
  HIP_TRY(o->sy.reserve(sizeof(float) * zs.sy));
  HIP_TRY(o->vec.reserve(sizeof(float) * z.vec));
  HIP_TRY(o->hist.reserve(sizeof(float) * z.hist));
  HIP_TRY(o->running.reserve(sizeof(int64_t)));
  if(grouped)
  {
    o->row_start.assign(row_start, row_start + P + 1);
    const std::vector<int> rows(o->row_start.begin(), o->row_start.end()); // n <= int32 by lbfgs_shape_refusal
    HIP_TRY(o->rows.reserve(sizeof(int) * rows.size()));
    HIP_TRY(hipMemcpy(o->rows.p.get(), rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(lb_clear(o.get(), nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *out = o.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_lbfgs_create(int device, int64_t n, int64_t D, int64_t m, float c1, float tol_grad, float tol_f, int max_ls,
                                   float curv_eps, struct smplpp_lbfgs ** out)
{
  return lb_create("smplpp_lbfgs_create", device, n, D, m, n, nullptr, false, LbfgsOptions{c1, tol_grad, tol_f, max_ls, curv_eps}, out);
}

extern "C" int smplpp_lbfgs_create_grouped(int device, int64_t n, int64_t D, int64_t m, int64_t P, const int64_t * row_start, float c1,
                                           float tol_grad, float tol_f, int max_ls, float curv_eps, struct smplpp_lbfgs ** out)
{
  return lb_create("smplpp_lbfgs_create_grouped", device, n, D, m, P, row_start, true, LbfgsOptions{c1, tol_grad, tol_f, max_ls, curv_eps}, out);
}

extern "C" int smplpp_lbfgs_groups(const struct smplpp_lbfgs * opt, int64_t * P, int64_t * row_start)
{
  if(!opt) return fail(SMPLPP_ERR_INVALID, "smplpp_lbfgs_groups: no optimiser");
  if(P) *P = opt->P;
  if(row_start)
    for(int64_t p = 0; p <= opt->P; p++) row_start[p] = opt->grouped ? opt->row_start[(size_t)p] : p;
  return SMPLPP_OK;
}

extern "C" int smplpp_lbfgs_destroy(struct smplpp_lbfgs * opt)
{
  if(!opt) return SMPLPP_OK;
  (void)hipSetDevice(opt->device);
  delete opt;
  return SMPLPP_OK;
}

extern "C" int smplpp_lbfgs_info(const struct smplpp_lbfgs * opt, int64_t * n, int64_t * D, int64_t * m)
{
  if(!opt) return fail(SMPLPP_ERR_INVALID, "smplpp_lbfgs_info: no optimiser");
  if(n) *n = opt->n;
  if(D) *D = opt->D;
  if(m) *m = opt->m;
  return SMPLPP_OK;
}

extern "C" int smplpp_lbfgs_reset(struct smplpp_lbfgs * opt, void * stream)
{
  if(!opt) return fail(SMPLPP_ERR_INVALID, "smplpp_lbfgs_reset: no optimiser");
  HIP_TRY(hipSetDevice(opt->device));
  HIP_TRY(lb_clear(opt, static_cast<hipStream_t>(stream)));
  return SMPLPP_OK;
}

extern "C" int smplpp_lbfgs_step(struct smplpp_lbfgs * opt, float * x, int64_t ld_x, const float * f, const float * g, int64_t ld_g, int space,
                                 void * stream)
{
  const char * fn = "smplpp_lbfgs_step";
  if(int rc = lb_check_rows(fn, opt, x, ld_x, space)) return rc;
  if(const char * why = lbfgs_rows_refusal(opt->n, opt->D, ld_g)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": (g) " + why);
  if(!f || !g) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": f or g is NULL");
  const int64_t n = opt->n, D = opt->D;
  Frame fr(opt->device, &opt->arena, space, stream, "lbfgs step");
  // (a host-space row travels whole, and comes back as it went where the kernel leaves it alone)
  float * xd = fr.out(x, (size_t)((n - 1) * ld_x + D), true);
  const float * fd = fr.in(f, (size_t)opt->P);
  const float * gd = fr.in(g, (size_t)((n - 1) * ld_g + D));
  return fr.run([&] {
    HIP_TRY(lb_step(opt, xd, ld_x, fd, gd, ld_g, fr.st));
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_lbfgs_state(struct smplpp_lbfgs * opt, int32_t * status, int32_t * iterations, int32_t * evaluations, float * f_best,
                                  float * step, int64_t * running, int space, void * stream)
{
  const char * fn = "smplpp_lbfgs_state";
  if(!opt) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no optimiser");
  if(!status && !iterations && !evaluations && !f_best && !step && !running) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": every output is NULL");
  if(int rc = check_space(space, fn)) return rc;
  const size_t n = (size_t)opt->P; // the scalars are [.][P]; P = n without groups
  Frame fr(opt->device, &opt->arena, space, stream, "lbfgs state");
  return fr.run([&] {
    const int * I = opt->ints.as<int>();
    const float * F = opt->floats.as<float>();
    fr.fetch(status, I + LBFGS_STATUS * n, n);
    fr.fetch(iterations, I + LBFGS_ITER * n, n);
    fr.fetch(evaluations, I + LBFGS_EVAL * n, n);
    fr.fetch(f_best, F + LBFGS_F0 * n, n);
    fr.fetch(step, F + LBFGS_STEP * n, n);
    if(running)
    {
      lbfgs_running_kernel<<<dim3(1), dim3(256), 0, fr.st>>>(lb_state(opt), opt->running.as<int64_t>());
      HIP_TRY(hipGetLastError());
      fr.fetch(running, opt->running.as<int64_t>(), 1);
    }
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_lbfgs_best(struct smplpp_lbfgs * opt, float * x, int64_t ld_x, float * f, int space, void * stream)
{
  const char * fn = "smplpp_lbfgs_best";
  if(int rc = lb_check_rows(fn, opt, x, ld_x, space)) return rc;
  const int64_t n = opt->n, D = opt->D;
  Frame fr(opt->device, &opt->arena, space, stream, "lbfgs best");
  float * xd = fr.out(x, (size_t)((n - 1) * ld_x + D), ld_x > D);
  float * fd = fr.out(f, (size_t)opt->P);
  return fr.run([&] {
    if(opt->grouped)
      lbfgs_wide_best_kernel<<<dim3((unsigned)opt->P), dim3(256), 0, fr.st>>>(lb_state(opt), xd, ld_x, fd);
    else
      lbfgs_best_kernel<<<dim3((unsigned)((n * D + 255) / 256)), dim3(256), 0, fr.st>>>(lb_state(opt), xd, ld_x, fd);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
