// The fixed-order sums: every energy and every shared gradient of the library is one of two rules, stated here once.
//
//  sum64    element k goes to partial k mod 64 in ascending k from +0; the partials meet as p_i = p_i + p_(i xor s), s = 32, 16, 8, 4, 2, 1.
//  sum1024  the same with 1024 partials, the meeting continued by s = 512, 256, 128, 64.
//
// The sum is p_0's bits.  Two facts make the work split bit-neutral: a partial that no element reaches is +0, and a partial that elements
// reach is never -0 (it starts from +0).  So leaving out the additions of untouched partials changes no bit, and who holds which partial
// may follow the size.  Every fp32 operation is rounded on its own, whatever the includer set before.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#pragma clang fp contract(off)

namespace smplpp_hip
{
// Which form sums a frame's K elements by sum1024: nq = 0, a wavefront per frame while they fit its lanes (the partials past 63 are +0),
// else a workgroup per frame of 1024 / nq threads, nq partials each (above K = 1024: 16 wavefronts a compute unit where 256 would leave 4).
struct FrameSumSplit
{
  int nq, threads;
};
inline FrameSumSplit frame_sum_split(long long K)
{
  return K <= 64 ? FrameSumSplit{0, 64} : K <= 1024 ? FrameSumSplit{4, 256} : FrameSumSplit{1, 1024};
}

#ifdef __HIPCC__
constexpr int SUM1024_WAVES = 1024 / 64; // the wavefronts of a workgroup that holds a partial per thread

// sum64: the 64 partials of a wavefront meet (every lane ends with p_0's bits); max64_meet is the same tree under max
__device__ inline float sum64_meet(float p)
{
  for(int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s);
  return p;
}
__device__ inline float max64_meet(float p)
{
  for(int s = 32; s >= 1; s >>= 1) p = fmaxf(p, __shfl_xor(p, s));
  return p;
}
// N sums at once, level by level
template<int N>
__device__ inline void sum64_meet(float (&v)[N])
{
#pragma unroll
  for(int s = 32; s >= 1; s >>= 1)
#pragma unroll
    for(int e = 0; e < N; e++) v[e] = v[e] + __shfl_xor(v[e], s);
}

// sum1024, one sum: a workgroup of 1024 / NQ threads holds the partials, thread t the partials t + (1024 / NQ) q in v[q].  The first six
// meetings are shuffles, the next log2(NQ) stay inside the thread, the rest cross the wavefronts through `cross` [1024 / NQ / 64] (one
// barrier; every thread of the workgroup calls; a single wavefront needs no `cross`).  The result is p_0's bits, in every thread.
template<int NQ>
__device__ inline float sum1024_meet(float (&v)[NQ], float * cross)
{
  constexpr int WAVES = 1024 / NQ / 64;
#pragma unroll
  for(int q = 0; q < NQ; q++)
#pragma unroll
    for(int s = 32; s >= 1; s >>= 1) v[q] = v[q] + __shfl_xor(v[q], s);
#pragma unroll
  for(int h = NQ / 2; h >= 1; h >>= 1)
#pragma unroll
    for(int q = 0; q < h; q++) v[q] = v[q] + v[q + h];
  if constexpr(WAVES == 1) return v[0];
  else
  {
    if((threadIdx.x & 63) == 0) cross[threadIdx.x >> 6] = v[0];
    __syncthreads();
    float r[WAVES];
#pragma unroll
    for(int u = 0; u < WAVES; u++) r[u] = cross[u];
#pragma unroll
    for(int h = WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
      for(int u = 0; u < h; u++) r[u] = r[u] + r[u + h];
    return r[0];
  }
}

// sum_j load(j), j < n, by sum1024 in one wavefront: lane l owns the partials l + 64 q, q < 16
template<class Load>
__device__ inline float sum1024_wave(int n, int lane, Load load)
{
  float v[16];
#pragma unroll
  for(int q = 0; q < 16; q++) v[q] = 0.0f;
  for(int j0 = 0; j0 < n; j0 += 1024)
#pragma unroll
    for(int q = 0; q < 16; q++)
    {
      const int j = j0 + 64 * q + lane;
      if(j < n) v[q] = v[q] + load(j);
    }
  return sum1024_meet<16>(v, nullptr);
}

// sum1024, K values at once, a partial of each per thread of a workgroup of 1024: p_i = p_i op p_(i xor s) for s = 32, 16, 8, 4, 2, 1
// inside the wavefront, then 512, 256, 128, 64 across the wavefronts (op: + , or max where MAXES has the value's bit).  cross[2][3][16]:
// two banks taken in turn, so that one barrier per meeting is enough: a wavefront writes a bank again only after passing the barrier of
// the meeting in between, which every other wavefront reaches after it has read that bank.  Every thread of the workgroup calls it, and
// ends with the same bits.  (A second body beside sum1024_meet: K sums of a partial per thread, against one sum of NQ.)
template<int K, unsigned MAXES>
__device__ inline void sum1024_meet_many(float (&v)[K], float (*cross)[3][SUM1024_WAVES], int & turn)
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
    v[i] = cross[turn][i][lane & (SUM1024_WAVES - 1)]; // lane u of every 16 holds wavefront u's value: xor 8, 4, 2, 1 there is xor 512 .. 64 of the partials
#pragma unroll
    for(int s = SUM1024_WAVES / 2; s >= 1; s >>= 1)
    {
      const float o = __shfl_xor(v[i], s);
      v[i] = (MAXES >> i & 1u) ? fmaxf(v[i], o) : v[i] + o;
    }
  }
  turn ^= 1;
}
__device__ inline float sum1024_meet_one(float p, float (*cross)[3][SUM1024_WAVES], int & turn)
{
  float v[1] = {p};
  sum1024_meet_many<1, 0u>(v, cross, turn);
  return v[0];
}
#endif
} // namespace smplpp_hip
