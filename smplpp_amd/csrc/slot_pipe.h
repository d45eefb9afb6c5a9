// Helpers shared by the slot-pipelined fused kernels (skin_b.hip, skin_e.hip, skin_h.hip).  What each form counts — the
// vector-memory and LDS instructions a barrier lets stay in flight — stays in that form's file.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace smplpp_hip
{
template<class F, int... I>
__device__ __forceinline__ void static_for_impl(F && f, std::integer_sequence<int, I...>)
{
  (f(std::integral_constant<int, I>{}), ...);
}
// f(std::integral_constant<int, i>{}) for i = 0 .. N-1, unrolled at compile time
template<int N, class F>
__device__ __forceinline__ void static_for(F && f)
{
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// bf16x3 piece products in issue order (index into the A pieces, index into the B pieces): small terms first
constexpr int PIECE_A[6] = {2, 0, 1, 1, 0, 0};
constexpr int PIECE_B[6] = {0, 2, 1, 0, 1, 0};

// hipcc does not order LDS reads behind LDS-DMA writes: a barrier that publishes DMA data waits for a counted number of
// in-flight instructions.  VM = vector-memory instructions that may stay in flight, LGKM = LDS instructions that may.
// BARRIER = false keeps the wait and drops the s_barrier (development ablations only: results are wrong).
template<int VM, int LGKM, bool BARRIER = true>
__device__ __forceinline__ void waitcnt_barrier()
{
  if constexpr(BARRIER)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(%1)\n\ts_barrier" ::"n"(VM), "n"(LGKM) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(%1)" ::"n"(VM), "n"(LGKM) : "memory");
}

__device__ __forceinline__ void full_barrier()
{
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
} // namespace smplpp_hip

// keeps the compiler from moving instructions across this point: the slots of a pipeline are placed by hand
#define SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
