// The backward pass both scan distances share ("The record gather").  Each distance's record kernel writes one record
// per (frame, query): the keys of the targets it touches (its first 16 bytes; -1: none) and their shares.  record_gather_kernel
// gives each target one thread, GATHER_T per workgroup; the frame's records pass through LDS GATHER_TILE at a time, compacted in
// record order (__ballot / __popcll, then a prefix over rows and wavefronts) to those that touch the workgroup's targets [lo, hi),
// and each thread adds its shares in ascending record, then key: one fixed-order sum per target, no floating-point atomics.  An add
// may be branch-free: +0 added for another target's share leaves acc's bits (acc starts at +0; a sum is -0 only if both terms are).
// A record type supplies its LDS image Tile and touches(head, lo, hi), stage(tile, pos, head, rec), add(acc, tile, h, u).  With
// `nvalid` (device, [n]) a frame's records past nvalid[frame] are not read.  distance_vjp() is the host side the VJP entries of
// the scan distances share; it runs on its caller's call frame (staging.h), so an entry point that stages an argument of its own
// first (the signed distance's `inside`) still has one frame, and one run of arena slots, for the whole call.
#pragma once
#include "staging.h"

namespace smplpp_hip
{
constexpr int GATHER_T = 256;                 // targets (and threads) per workgroup
constexpr int GATHER_R = 4;                   // records per thread per tile
constexpr int GATHER_TILE = GATHER_T * GATHER_R; // records per LDS tile

template<class Rec>
__global__ __launch_bounds__(GATHER_T) void record_gather_kernel(const Rec * __restrict__ rec, float * __restrict__ out, int accumulate,
                                                                 int64_t nrec, int64_t ntarget, int64_t blocks_per_frame,
                                                                 const int64_t * __restrict__ nvalid)
{
  __shared__ typename Rec::Tile s_tile;
  __shared__ int s_cnt[GATHER_R][GATHER_T / 64];
  const int64_t frame = blockIdx.x / blocks_per_frame;
  const int lo = (int)(blockIdx.x % blocks_per_frame) * GATHER_T;
  const int hi = (int)(lo + GATHER_T < ntarget ? lo + GATHER_T : ntarget);
  const int u = lo + (int)threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Rec * rf = rec + frame * nrec;
  if(nvalid) nrec = nvalid[frame] < nrec ? nvalid[frame] : nrec;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for(int64_t base = 0; base < nrec; base += GATHER_TILE)
  {
    int4 head[GATHER_R];
    bool hit[GATHER_R];
    int pos[GATHER_R];
#pragma unroll
    for(int r = 0; r < GATHER_R; r++)
    {
      const int64_t i = base + r * GATHER_T + threadIdx.x;
      head[r] = i < nrec ? *reinterpret_cast<const int4 *>(rf + i) : make_int4(-1, -1, -1, -1);
      hit[r] = Rec::touches(head[r], lo, hi);
      const uint64_t mask = __ballot(hit[r]);
      pos[r] = (int)__popcll(mask & ((1ull << lane) - 1ull));
      if(lane == 0) s_cnt[r][wave] = (int)__popcll(mask);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for(int r = 0; r < GATHER_R; r++)
      for(int w = 0; w < GATHER_T / 64; w++)
      {
        if(w == wave) pos[r] += total; // records before this one: earlier rows, then earlier wavefronts of this row
        total += s_cnt[r][w];
      }
#pragma unroll
    for(int r = 0; r < GATHER_R; r++)
      if(hit[r]) Rec::stage(s_tile, pos[r], head[r], rf[base + r * GATHER_T + threadIdx.x]);
    __syncthreads();
    if(u < hi)
#pragma unroll 8
      for(int h = 0; h < total; h++) Rec::add(acc, s_tile, h, u); // (unrolled: independent LDS reads in flight; the adds keep their order)
    __syncthreads();
  }
  if(u >= hi) return;
  float * o = out + (frame * ntarget + u) * 3;
  for(int x = 0; x < 3; x++) o[x] = accumulate ? o[x] + acc[x] : acc[x];
}

// n frames of nrec records each (the first nvalid[frame] of them, with nvalid) into [n][ntarget][3] floats
template<class Rec>
int record_gather(const Rec * rec, float * out, int accumulate, int64_t n, int64_t nrec, int64_t ntarget, hipStream_t st,
                  const int64_t * nvalid = nullptr)
{
  const int64_t bpf = (ntarget + GATHER_T - 1) / GATHER_T;
  record_gather_kernel<Rec><<<dim3((unsigned)(n * bpf)), dim3(GATHER_T), 0, st>>>(rec, out, accumulate, nrec, ntarget, bpf, nvalid);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// The host side of both VJP entries after their own checks, on the entry point's frame: the arguments staged, the outputs loaded
// when the call adds into them, device() on device pointers, the outputs copied back.  ids and gsq hold nids entries.
template<class State, class Device>
int distance_vjp(Frame & fr, const Device & device, smplpp_model * m, State * s, int64_t n, const float * verts, int64_t K,
                 const float * points, const int64_t * ids, int64_t nids, const float * grad_sqdist, float * grad_verts,
                 float * grad_points, int accumulate)
{
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  const int64_t * id = fr.in(ids, (size_t)nids);
  const float * g = fr.in(grad_sqdist, (size_t)nids);
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  float * gp = fr.out(grad_points, (size_t)n * K * 3, accumulate);
  return fr.run([&] { return device(m, s, n, v, K, p, id, g, gv, gp, accumulate, fr.st); });
}
} // namespace smplpp_hip
