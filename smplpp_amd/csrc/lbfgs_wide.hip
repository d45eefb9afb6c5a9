// The kernels of a grouped L-BFGS handle (smplpp_lbfgs_create_grouped): P problems, each a run of consecutive rows of the
// caller's x and g, N = rows D unknowns.  The rule is in include/smplpp_hip.h: the per-frame rule of smplpp_lbfgs_step on the problem's N
// elements with every sum by the 1024-partial rule; every fp32 operation below is rounded on its own (no contraction to FMA) and there
// are no atomics.
//
//  lbfgs_wide_step_kernel  one workgroup of 1024 threads per problem, one launch per evaluation.  Thread t owns the elements j = t, t + 1024,
//                          ... of every vector of its problem, that is partial t of every sum, so that the only traffic between threads
//                          is the meeting of the partials: __shfl_xor inside a wavefront, then the 16 wavefront sums through LDS and one
//                          workgroup barrier, after which every thread holds the same bits.  Every branch is decided by such values (or
//                          by scalars that every thread read before the first barrier, and thread 0 writes after it), so the workgroup
//                          reaches every barrier whole; a stopped problem's workgroup reads its status and returns whole.  The handle's
//                          own vectors are contiguous per problem and indexed by j; the caller's rows are walked by the cursor of
//                          lbfgs_wide_plan.h.  The working vector of the two-loop recursion lives in LDS when the handle's longest
//                          problem has N <= LBFGS_W_LDS_N, else in the problem's direction block; the 2 c + 1 folded passes are those
//                          of lbfgs_step_kernel.
//  lbfgs_wide_best_kernel  the accepted points into the caller's rows: one workgroup of 256 per problem.
#include "lbfgs_wide.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
// K partials per thread meet at once: p_i = p_i op p_(i xor s) for s = 32, 16, 8, 4, 2, 1 inside the wavefront, then 512, 256, 128, 64
// across the wavefronts (op: + , or max where MAXES has the value's bit).  cross[2][3][16]: two banks taken in turn, so that one barrier
// per meeting is enough: a wavefront writes a bank again only after passing the barrier of the meeting in between, which every other
// wavefront reaches after it has read that bank.  Every thread of the workgroup calls it, and ends with the same bits.
template<int K, unsigned MAXES>
__device__ inline void lbw_meet(float (&v)[K], float (*cross)[3][LBFGS_W_WAVES], int & turn)
{
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for(int i = 0; i < K; i++)
#pragma unroll
    for(int s = 32; s >= 1; s >>= 1)
    {
      const float o = __shfl_xor(v[i], s);
      v[i] = (MAXES >> i & 1u) ? fmaxf(v[i], o) : v[i] + o;
    }
  if(lane == 0)
  {
#pragma unroll
    for(int i = 0; i < K; i++) cross[turn][i][w] = v[i];
  }
  __syncthreads();
#pragma unroll
  for(int i = 0; i < K; i++)
  {
    v[i] = cross[turn][i][lane & (LBFGS_W_WAVES - 1)]; // lane u of every 16 holds wavefront u's value: xor 8, 4, 2, 1 there is xor 512 .. 64 of the partials
#pragma unroll
    for(int s = LBFGS_W_WAVES / 2; s >= 1; s >>= 1)
    {
      const float o = __shfl_xor(v[i], s);
      v[i] = (MAXES >> i & 1u) ? fmaxf(v[i], o) : v[i] + o;
    }
  }
  turn ^= 1;
}
__device__ inline float lbw_sum(float p, float (*cross)[3][LBFGS_W_WAVES], int & turn)
{
  float v[1] = {p};
  lbw_meet<1, 0u>(v, cross, turn);
  return v[0];
}

// grid: P; dynamic LDS: the longest problem's N floats when LDS_VECTOR
template<bool LDS_VECTOR>
__global__ __launch_bounds__(LBFGS_W_T) void lbfgs_wide_step_kernel(LbfgsWideState s, float * x, int64_t ld_x, const float * __restrict__ f,
                                                                    const float * __restrict__ g, int64_t ld_g)
{
  extern __shared__ __attribute__((aligned(16))) float lbw_smem[];
  __shared__ float cross[2][3][LBFGS_W_WAVES];
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
  lbw_meet<3, 3u>(a3, cross, turn);
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
    gtd = lbw_sum(pp, cross, turn);
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
  lbw_meet<2, 0u>(a2, cross, turn);
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
      c = lbw_sum(pp, cross, turn) / (sl == slot ? sy_new : sy[sl]);
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
      c = __shfl(akeep, i) - lbw_sum(pp, cross, turn) / (sl == slot ? sy_new : sy[sl]);
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
    gtd = lbw_sum(pp, cross, turn);
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
      gtd = -lbw_sum(pp, cross, turn);
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

// grid: P.  x, f: the caller's; f may be null.  A problem that has not been evaluated yet has no accepted point: left alone
__global__ __launch_bounds__(256) void lbfgs_wide_best_kernel(LbfgsWideState s, float * __restrict__ x, int64_t ld_x, float * __restrict__ f)
{
  const int p = blockIdx.x, P = s.P, D = s.D;
  if(s.ints[LBFGS_EVAL * P + p] == 0) return;
  const int row0 = s.rows[p];
  const unsigned N = (unsigned)(s.rows[p + 1] - row0) * (unsigned)D;
  const float * x0 = s.vec + lbfgs_wide_vec_offset(LBFGS_X0, s.n, D, row0);
  for(unsigned j = threadIdx.x; j < N; j += 256) x[(row0 + (int64_t)(j / D)) * ld_x + j % D] = x0[j];
  if(f && threadIdx.x == 0) f[p] = s.floats[LBFGS_F0 * P + p];
}

hipError_t lbfgs_wide_step(int device, const LbfgsWideState & s, const LbfgsWideLaunch & L, float * x, int64_t ld_x, const float * f, const float * g,
                           int64_t ld_g, hipStream_t st)
{
  if(L.lds_vector)
  {
    static PerDeviceOnce once; // the largest working vector, once per device
    if(L.lds_bytes > 64 * 1024)
      if(hipError_t e = lds_opt_in(once, device, reinterpret_cast<const void *>(&lbfgs_wide_step_kernel<true>), (int)(sizeof(float) * LBFGS_W_LDS_N)))
        return e;
    lbfgs_wide_step_kernel<true><<<dim3(L.grid), dim3(L.threads), L.lds_bytes, st>>>(s, x, ld_x, f, g, ld_g);
  }
  else
    lbfgs_wide_step_kernel<false><<<dim3(L.grid), dim3(L.threads), 0, st>>>(s, x, ld_x, f, g, ld_g);
  return hipGetLastError();
}

hipError_t lbfgs_wide_best(const LbfgsWideState & s, float * x, int64_t ld_x, float * f, hipStream_t st)
{
  lbfgs_wide_best_kernel<<<dim3((unsigned)s.P), dim3(256), 0, st>>>(s, x, ld_x, f);
  return hipGetLastError();
}
} // namespace smplpp_hip
