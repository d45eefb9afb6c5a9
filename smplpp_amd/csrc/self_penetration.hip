// Self-intersection of each frame's posed mesh and a self-penetration energy on the intersecting face pairs, with its
// vector-Jacobian product to the vertices.
//
// Detection (sort and sweep along the frame's longest axis; the AABB prefilter is exact, so the axis and the sort change only the
// work, never the pair list):
//  sp_box_kernel       per (frame, face): the closed fp32 AABB; a face with a non-finite coordinate gets lo = +inf, hi = -inf
//                      (it overlaps nothing) and the last sort key.
//  sp_frame_kernel     per frame: the longest axis of the valid faces' union box.
//  sp_sort_lds_kernel  per frame, F <= SP_LDS_SORT: the keys (ordered bits of lo[axis] << 32 | face) built and bitonic-sorted in
//                      LDS (16384 x 8 bytes = 128 KiB of the 160 KiB).  Larger F: sp_key_kernel and hipcub's segmented radix sort
//                      of the same unique keys, so both give the same order.
//  sp_scatter_kernel   the boxes in sorted order, the face id in lo.w, for a contiguous sweep.
//  sp_sweep_kernel     per (frame, sorted position, split): face f scans forwards only (SP_SPLIT threads, interleaved), while lo <= hi_f, so each AABB-overlapping pair
//                      is met once, by the face that sorts first, and kept when it passes the shared-vertex and crossing tests.
//                      The count pass counts each pair at its lower face id (integer atomics: counts do not depend on order);
//                      sp_scan_kernel gives each frame's exclusive prefix in face order and the true count; the write pass puts
//                      each pair in a slot of its lower face's range, and sp_order_kernel sorts each range by the partner (few
//                      per face), so the stored order is ascending (f, g) whatever order the slots were taken in.  The one
//                      range that straddles max_pairs is collected whole in a scratch row and its lowest partners stored.
//  sp_finish_kernel    per (frame, row): the energy of a stored pair, -1 ids and 0 energy past min(count, max_pairs).
// Backward (the pair set is an input and held fixed):
//  sp_vjp_record_kernel  per (frame, row): 6 records, one per (receiver, intruder corner), each touching the receiver's three
//                        vertices and the intruder corner.  A zero cotangent, a row past min(count, max_pairs) or an id out of
//                        [0, F) gives no records.
//  record_gather_kernel<SpRecord>  (distance_vjp.h) grad_verts: one fixed-order sum per vertex, over the 6 min(count, max_pairs)
//                        records of the frame.
#include "distance_vjp.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

namespace smplpp_hip
{
constexpr int SP_LDS_SORT = 16384; // faces per frame the LDS sort takes (keys: 128 KiB)
constexpr int SP_SORT_T = 1024;    // threads of the LDS sort and of the prefix
constexpr int SP_T = 256;          // threads of the per-item kernels
constexpr int SP_SCAN = 8;         // candidate boxes a sweep thread loads at once
constexpr int SP_SPLIT = 8;        // sweep threads per face, each taking every SP_SPLIT-th candidate: a long face's window (a face
                                   // spanning much of the body on the axis meets thousands) is shared, so no one thread sets the time

struct SpFrame
{
  int axis;
};

struct SelfPenState
{
  DevBuf box, sbox;       // [n][F] AABB (lo, hi as two float4): by face, then in sorted order
  DevBuf keys, keys_in;   // [n][F] sorted keys (and, large F, the unsorted ones)
  DevBuf frame;           // [n] SpFrame
  DevBuf cnt, off;        // [n][F] partners per face (int32) and their offsets (int64)
  DevBuf fill, strad;     // [n][F] slots taken per face in the write pass, and the partners of the range straddling max_pairs
  DevBuf seg, temp;       // large F: segment offsets [n + 1] and hipcub's workspace
  DevBuf rec, nrec;       // [n][max_pairs][6] SpRecord and [n] records per frame
};
void StateDelete::operator()(SelfPenState * s) const
{
  delete s;
}

struct SpRecord
{
  int32_t u[4]; // the receiver's three vertices, the intruder corner (-1: no record)
  float g[12];  // the shares of u[0..3], 3 each

  struct Tile
  {
    int4 u[GATHER_TILE];
    float g[GATHER_TILE][12];
  };
  __device__ static bool touches(const int4 & U, int lo, int hi)
  {
    return (U.x >= lo && U.x < hi) || (U.y >= lo && U.y < hi) || (U.z >= lo && U.z < hi) || (U.w >= lo && U.w < hi);
  }
  __device__ static void stage(Tile & t, int pos, const int4 & U, const SpRecord & r)
  {
    t.u[pos] = U;
    for(int e = 0; e < 12; e++) t.g[pos][e] = r.g[e];
  }
  __device__ static void add(float * acc, const Tile & t, int h, int u)
  {
    const int4 U = t.u[h];
    const int k[4] = {U.x, U.y, U.z, U.w};
    for(int j = 0; j < 4; j++)
      if(k[j] == u)
        for(int x = 0; x < 3; x++) acc[x] += t.g[h][3 * j + x];
  }
};
static_assert(sizeof(SpRecord) == 64, "SpRecord: four 16-byte loads");

// ---- the contract's arithmetic: every operation rounded on its own
__device__ inline float sp_orient(const float3 & a, const float3 & b, const float3 & c, const float3 & d)
{
#pragma clang fp contract(off)
  const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const float vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
  const float wx = d.x - a.x, wy = d.y - a.y, wz = d.z - a.z;
  const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  return (cx * wx + cy * wy) + cz * wz;
}

// edge pq of one triangle against triangle abc, given op = orient(a,b,c,p) and oq = orient(a,b,c,q)
__device__ inline bool sp_edge_crosses(float op, float oq, const float3 & p, const float3 & q, const float3 & a, const float3 & b,
                                       const float3 & c)
{
  if(!((op > 0.0f && oq < 0.0f) || (op < 0.0f && oq > 0.0f))) return false;
  const float s0 = sp_orient(p, q, a, b), s1 = sp_orient(p, q, b, c), s2 = sp_orient(p, q, c, a);
  return (s0 > 0.0f && s1 > 0.0f && s2 > 0.0f) || (s0 < 0.0f && s1 < 0.0f && s2 < 0.0f);
}

// some edge (x0 x1, x1 x2, x2 x0) of triangle x crosses triangle y
__device__ inline bool sp_edges_cross(const float3 * x, const float3 * y)
{
  const float o0 = sp_orient(y[0], y[1], y[2], x[0]), o1 = sp_orient(y[0], y[1], y[2], x[1]), o2 = sp_orient(y[0], y[1], y[2], x[2]);
  return sp_edge_crosses(o0, o1, x[0], x[1], y[0], y[1], y[2]) || sp_edge_crosses(o1, o2, x[1], x[2], y[0], y[1], y[2]) ||
         sp_edge_crosses(o2, o0, x[2], x[0], y[0], y[1], y[2]);
}

__device__ inline float3 sp_vert(const float * vf, int v)
{
  return make_float3(vf[3 * v], vf[3 * v + 1], vf[3 * v + 2]);
}

__device__ inline float sp_axis(const float4 & b, int axis)
{
  return axis == 0 ? b.x : axis == 1 ? b.y : b.z;
}

// float -> uint32 in the order of the floats (-0 just below +0)
__device__ inline uint32_t sp_ordered(float x)
{
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- detection
__global__ __launch_bounds__(SP_T) void sp_box_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                      float4 * __restrict__ box, int64_t V, int64_t F, int64_t nf)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= nf) return;
  const int64_t frame = i / F, f = i % F;
  const float * vf = verts + frame * V * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool ok = true;
  for(int j = 0; j < 3; j++)
  {
    const int v = faces[f * 3 + j];
    for(int x = 0; x < 3; x++)
    {
      const float c = vf[(int64_t)v * 3 + x];
      ok = ok && isfinite(c);
      lo[x] = fminf(lo[x], c);
      hi[x] = fmaxf(hi[x], c);
    }
  }
  if(!ok)
    for(int x = 0; x < 3; x++)
    {
      lo[x] = INFINITY;
      hi[x] = -INFINITY;
    }
  box[2 * i] = make_float4(lo[0], lo[1], lo[2], 0.0f);
  box[2 * i + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

__global__ __launch_bounds__(SP_T) void sp_frame_kernel(const float4 * __restrict__ box, SpFrame * __restrict__ info, int64_t F)
{
  __shared__ float s_r[6][SP_T / 64];
  const int64_t frame = blockIdx.x;
  const float4 * bf = box + frame * F * 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float r[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY}; // min lo, min -hi
  for(int64_t f = threadIdx.x; f < F; f += SP_T)
  {
    const float4 lo = bf[2 * f], hi = bf[2 * f + 1];
    if(!(lo.x <= hi.x)) continue;
    r[0] = fminf(r[0], lo.x), r[1] = fminf(r[1], lo.y), r[2] = fminf(r[2], lo.z);
    r[3] = fminf(r[3], -hi.x), r[4] = fminf(r[4], -hi.y), r[5] = fminf(r[5], -hi.z);
  }
  for(int k = 0; k < 6; k++)
  {
    for(int o = 32; o > 0; o >>= 1) r[k] = fminf(r[k], __shfl_xor(r[k], o));
    if(lane == 0) s_r[k][wave] = r[k];
  }
  __syncthreads();
  if(threadIdx.x == 0)
  {
    float e[3];
    for(int x = 0; x < 3; x++)
    {
      float mlo = INFINITY, mhi = INFINITY;
      for(int w = 0; w < SP_T / 64; w++) mlo = fminf(mlo, s_r[x][w]), mhi = fminf(mhi, s_r[3 + x][w]);
      e[x] = -mhi - mlo; // -inf when no face is valid: axis 0
    }
    int axis = 0;
    for(int x = 1; x < 3; x++)
      if(e[x] > e[axis]) axis = x;
    info[frame] = SpFrame{axis};
  }
}

__device__ inline uint64_t sp_key(const float4 * bf, int64_t f, int axis)
{
  const float4 lo = bf[2 * f], hi = bf[2 * f + 1];
  const uint32_t k = lo.x <= hi.x ? sp_ordered(sp_axis(lo, axis)) : 0xffffffffu; // invalid faces last
  return ((uint64_t)k << 32) | (uint32_t)f;
}

__global__ __launch_bounds__(SP_SORT_T) void sp_sort_lds_kernel(const float4 * __restrict__ box, const SpFrame * __restrict__ info,
                                                                uint64_t * __restrict__ keys, int64_t F)
{
  __shared__ uint64_t s_k[SP_LDS_SORT];
  const int64_t frame = blockIdx.x;
  const float4 * bf = box + frame * F * 2;
  const int axis = info[frame].axis;
  int P = 1;
  while(P < F) P <<= 1;
  for(int i = threadIdx.x; i < P; i += SP_SORT_T) s_k[i] = i < F ? sp_key(bf, i, axis) : ~0ull;
  __syncthreads();
  for(int k = 2; k <= P; k <<= 1)
    for(int j = k >> 1; j > 0; j >>= 1)
    {
      for(int t = threadIdx.x; t < (P >> 1); t += SP_SORT_T)
      {
        const int i = 2 * t - (t & (j - 1)); // the lower index of the t-th compare-exchange
        const int l = i + j;
        const bool up = (i & k) == 0;
        const uint64_t a = s_k[i], b = s_k[l];
        if((a > b) == up)
        {
          s_k[i] = b;
          s_k[l] = a;
        }
      }
      __syncthreads();
    }
  uint64_t * kf = keys + frame * F;
  for(int i = threadIdx.x; i < F; i += SP_SORT_T) kf[i] = s_k[i];
}

__global__ __launch_bounds__(SP_T) void sp_key_kernel(const float4 * __restrict__ box, const SpFrame * __restrict__ info,
                                                      uint64_t * __restrict__ keys, int64_t F, int64_t nf)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= nf) return;
  const int64_t frame = i / F;
  keys[i] = sp_key(box + frame * F * 2, i % F, info[frame].axis);
}

__global__ void sp_seg_kernel(int * __restrict__ seg, int64_t F, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i <= n) seg[i] = (int)(i * F);
}

__global__ __launch_bounds__(SP_T) void sp_scatter_kernel(const uint64_t * __restrict__ keys, const float4 * __restrict__ box,
                                                          float4 * __restrict__ sbox, int64_t F, int64_t nf)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= nf) return;
  const int64_t frame = i / F;
  const uint32_t f = (uint32_t)keys[i];
  const float4 * b = box + (frame * F + f) * 2;
  float4 lo = b[0];
  lo.w = __uint_as_float(f);
  sbox[2 * i] = lo;
  sbox[2 * i + 1] = b[1];
}

// face g (box glo, ghi) against face f (its box, vertex ids fv and corners fx): the AABBs overlap, no shared vertex, an edge crosses
__device__ inline bool sp_pair(const float4 & flo, const float4 & fhi, const int * fv, const float3 * fx, const float4 & glo,
                               const float4 & ghi, int g, const int32_t * faces, const float * vf)
{
  if(!(glo.x <= fhi.x && flo.x <= ghi.x && glo.y <= fhi.y && flo.y <= ghi.y && glo.z <= fhi.z && flo.z <= ghi.z)) return false;
  int gv[3];
  float3 gx[3];
  for(int j = 0; j < 3; j++) gv[j] = faces[(int64_t)g * 3 + j];
  for(int j = 0; j < 3; j++)
    if(gv[j] == fv[0] || gv[j] == fv[1] || gv[j] == fv[2]) return false;
  for(int j = 0; j < 3; j++) gx[j] = sp_vert(vf, gv[j]);
  return sp_edges_cross(fx, gx) || sp_edges_cross(gx, fx);
}

// Write = false: cnt[frame][a] counts the pairs (a, b), a < b, found.  Write = true: each pair goes to a slot of a's range from
// off[frame][a] (the slot from an integer counter, fill: the order within a range is fixed afterwards by sp_order_kernel); a range
// that straddles max_pairs goes to strad[frame] whole, a range past it nowhere.  Thread p scans forwards only, while lo <= hi_p:
// every pair whose AABBs overlap is met exactly once, by the one of the two faces that sorts first (by one of its SP_SPLIT threads).
template<bool Write>
__global__ __launch_bounds__(SP_T) void sp_sweep_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                        const float4 * __restrict__ sbox, const SpFrame * __restrict__ info,
                                                        int32_t * __restrict__ cnt, int32_t * __restrict__ fill,
                                                        const int64_t * __restrict__ off, int32_t * __restrict__ strad,
                                                        int64_t * __restrict__ pairs, int64_t max_pairs, int64_t V, int64_t F, int64_t nf)
{
  const int64_t t = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(t >= nf * SP_SPLIT) return;
  const int64_t i = t / SP_SPLIT, split = t % SP_SPLIT;
  const int64_t frame = i / F, p = i % F;
  const float4 * sb = sbox + frame * F * 2;
  const float4 flo = sb[2 * p], fhi = sb[2 * p + 1];
  if(!(flo.x <= fhi.x)) return; // a non-finite face: no partners
  const int f = (int)__float_as_uint(flo.w);
  const int axis = info[frame].axis;
  const float * vf = verts + frame * V * 3;
  int fv[3];
  float3 fx[3];
  for(int j = 0; j < 3; j++) fv[j] = faces[(int64_t)f * 3 + j];
  for(int j = 0; j < 3; j++) fx[j] = sp_vert(vf, fv[j]);
  const float hi_f = sp_axis(fhi, axis);
  for(int64_t q0 = p + 1 + split; q0 < F; q0 += SP_SCAN * SP_SPLIT)
  {
    // the next SP_SCAN boxes' lo loaded together (one memory latency per SP_SCAN candidates); lo is sorted, so the candidates
    // within reach on the axis are a prefix of them
    uint32_t in = 0;
#pragma unroll
    for(int j = 0; j < SP_SCAN; j++)
      if(q0 + j * SP_SPLIT < F && sp_axis(sb[2 * (q0 + j * SP_SPLIT)], axis) <= hi_f) in |= 1u << j;
    const bool done = in != (1u << SP_SCAN) - 1u;
    for(; in; in &= in - 1u)
    {
      const int64_t q = q0 + __builtin_ctz(in) * SP_SPLIT;
      const float4 glo = sb[2 * q];
      const int g = (int)__float_as_uint(glo.w);
      if(!sp_pair(flo, fhi, fv, fx, glo, sb[2 * q + 1], g, faces, vf)) continue;
      const int64_t fa = frame * F + (f < g ? f : g);
      if(!Write)
      {
        atomicAdd(cnt + fa, 1);
        continue;
      }
      const int s = atomicAdd(fill + fa, 1);
      const int64_t base = off[fa], k = cnt[fa];
      if(base + k <= max_pairs)
      {
        int64_t * o = pairs + (frame * max_pairs + base + s) * 2;
        o[0] = f < g ? f : g;
        o[1] = f < g ? g : f;
      }
      else if(base < max_pairs)
        strad[frame * F + s] = f < g ? g : f;
    }
    if(done) break;
  }
}

// per (frame, face a): a's partners in ascending b.  A range below max_pairs is sorted in place; the range that straddles
// max_pairs is sorted in strad and its lowest max_pairs - off[a] partners stored.
__global__ __launch_bounds__(SP_T) void sp_order_kernel(const int32_t * __restrict__ cnt, const int64_t * __restrict__ off,
                                                        int32_t * __restrict__ strad, int64_t * __restrict__ pairs, int64_t max_pairs,
                                                        int64_t F, int64_t nf)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= nf) return;
  const int64_t frame = i / F, a = i % F;
  const int64_t k = cnt[i], base = off[i];
  if(k == 0 || base >= max_pairs) return;
  if(base + k <= max_pairs)
  {
    int64_t * o = pairs + (frame * max_pairs + base) * 2;
    for(int64_t x = 1; x < k; x++) // insertion sort of the partners (few per face)
    {
      const int64_t b = o[2 * x + 1];
      int64_t y = x - 1;
      for(; y >= 0 && o[2 * y + 1] > b; y--) o[2 * y + 3] = o[2 * y + 1];
      o[2 * y + 3] = b;
    }
    return;
  }
  int32_t * t = strad + frame * F;
  for(int64_t x = 1; x < k; x++)
  {
    const int32_t b = t[x];
    int64_t y = x - 1;
    for(; y >= 0 && t[y] > b; y--) t[y + 1] = t[y];
    t[y + 1] = b;
  }
  for(int64_t x = 0; x < max_pairs - base; x++)
  {
    int64_t * o = pairs + (frame * max_pairs + base + x) * 2;
    o[0] = a;
    o[1] = t[x];
  }
}

// per frame: off = exclusive prefix of cnt in face order, count = the total
__global__ __launch_bounds__(SP_SORT_T) void sp_scan_kernel(const int32_t * __restrict__ cnt, int64_t * __restrict__ off,
                                                            int64_t * __restrict__ count, int64_t F)
{
  __shared__ int64_t s_w[SP_SORT_T / 64];
  const int64_t frame = blockIdx.x;
  const int32_t * c = cnt + frame * F;
  int64_t * o = off + frame * F;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t per = (F + SP_SORT_T - 1) / SP_SORT_T;
  const int64_t b = t * per, e = b + per < F ? b + per : F;
  int64_t sum = 0;
  for(int64_t f = b; f < e; f++) sum += c[f];
  int64_t inc = sum; // inclusive scan over the wavefront
  for(int d = 1; d < 64; d <<= 1)
  {
    const int64_t y = __shfl_up(inc, d);
    if(lane >= d) inc += y;
  }
  if(lane == 63) s_w[wave] = inc;
  __syncthreads();
  int64_t run = inc - sum;
  for(int w = 0; w < wave; w++) run += s_w[w];
  for(int64_t f = b; f < e; f++)
  {
    o[f] = run;
    run += c[f];
  }
  if(t == SP_SORT_T - 1) count[frame] = run;
}

// ---- energy
// receiver (a, b, c), intruder x: the corner's term, and its gradient to a, b, c, x scaled by gamma when grad != nullptr, in T.  The
// forward's energies are computed in double (one thread per pair, off the hot path): the cone's 1 - q^2 / (sigma^2 rho^2) cancels
// for small sigma, and fp32 there would miss the float64 reference by more than an fp32 evaluation of the same graph does.
template<class T>
__device__ inline T sp_corner(const float3 & a, const float3 & b, const float3 & c, const float3 & x, T s2, T gamma, T (*grad)[3])
{
  const T ox = (T(a.x) + T(b.x) + T(c.x)) / T(3), oy = (T(a.y) + T(b.y) + T(c.y)) / T(3), oz = (T(a.z) + T(b.z) + T(c.z)) / T(3);
  const T e1[3] = {T(b.x) - T(a.x), T(b.y) - T(a.y), T(b.z) - T(a.z)}, e2[3] = {T(c.x) - T(a.x), T(c.y) - T(a.y), T(c.z) - T(a.z)};
  const T m[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const T len = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
  if(!(len > T(0))) return T(0); // zero area
  const T nn[3] = {m[0] / len, m[1] / len, m[2] / len};
  const T ra[3] = {T(a.x) - ox, T(a.y) - oy, T(a.z) - oz}, rb[3] = {T(b.x) - ox, T(b.y) - oy, T(b.z) - oz};
  const T rc[3] = {T(c.x) - ox, T(c.y) - oy, T(c.z) - oz};
  const T r2 =
    ((ra[0] * ra[0] + ra[1] * ra[1] + ra[2] * ra[2]) + (rb[0] * rb[0] + rb[1] * rb[1] + rb[2] * rb[2]) + (rc[0] * rc[0] + rc[1] * rc[1] + rc[2] * rc[2])) /
    T(3);
  const T d[3] = {T(x.x) - ox, T(x.y) - oy, T(x.z) - oz};
  const T h = d[0] * nn[0] + d[1] * nn[1] + d[2] * nn[2];
  if(!(h < T(0))) return T(0);
  const T q2 = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - h * h;
  const T sr = s2 * r2;
  const T phi = T(1) - q2 / sr;
  if(!(phi > T(0))) return T(0);
  if(grad)
  {
    // dE = cD d.dd + cH dh + cR dr2; dd = dx - do; dh = n.dd + p.dm with p = (d - h n) / |m|; dr2 = 2/3 sum_k (k - o).dk
    const T A = -T(2) * phi * h * h / sr;
    const T cD = T(2) * A, cH = T(2) * phi * phi * h - T(2) * h * A, cR = T(2) * phi * h * h * q2 / (sr * r2);
    T gx[3], pp[3];
    for(int k = 0; k < 3; k++)
    {
      gx[k] = gamma * (cD * d[k] + cH * nn[k]);
      pp[k] = gamma * cH * (d[k] - h * nn[k]) / len;
    }
    const T t1[3] = {e2[1] * pp[2] - e2[2] * pp[1], e2[2] * pp[0] - e2[0] * pp[2], e2[0] * pp[1] - e2[1] * pp[0]}; // e2 x p: to e1
    const T t2[3] = {pp[1] * e1[2] - pp[2] * e1[1], pp[2] * e1[0] - pp[0] * e1[2], pp[0] * e1[1] - pp[1] * e1[0]}; // p x e1: to e2
    const T cr = gamma * cR * (T(2) / T(3));
    for(int k = 0; k < 3; k++)
    {
      const T go = -gx[k] / T(3);
      grad[0][k] = go - t1[k] - t2[k] + cr * ra[k];
      grad[1][k] = go + t1[k] + cr * rb[k];
      grad[2][k] = go + t2[k] + cr * rc[k];
      grad[3][k] = gx[k];
    }
  }
  return phi * phi * (h * h);
}

__device__ inline void sp_pair_corners(const float * vf, const int32_t * faces, int64_t f, int64_t g, int * fv, int * gv, float3 * fx,
                                       float3 * gx)
{
  for(int j = 0; j < 3; j++)
  {
    fv[j] = faces[f * 3 + j];
    gv[j] = faces[g * 3 + j];
  }
  for(int j = 0; j < 3; j++)
  {
    fx[j] = sp_vert(vf, fv[j]);
    gx[j] = sp_vert(vf, gv[j]);
  }
}

__global__ __launch_bounds__(SP_T) void sp_finish_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                         const int64_t * __restrict__ count, int64_t * __restrict__ pairs,
                                                         float * __restrict__ energy, float s2, int64_t max_pairs, int64_t V,
                                                         int64_t np)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= np) return;
  const int64_t frame = i / max_pairs, row = i % max_pairs;
  if(row >= count[frame])
  {
    pairs[2 * i] = pairs[2 * i + 1] = -1;
    if(energy) energy[i] = 0.0f;
    return;
  }
  if(!energy) return;
  int fv[3], gv[3];
  float3 fx[3], gx[3];
  sp_pair_corners(verts + frame * V * 3, faces, pairs[2 * i], pairs[2 * i + 1], fv, gv, fx, gx);
  double e = 0.0;
  for(int j = 0; j < 3; j++) e += sp_corner<double>(fx[0], fx[1], fx[2], gx[j], s2, 0.0, nullptr);
  for(int j = 0; j < 3; j++) e += sp_corner<double>(gx[0], gx[1], gx[2], fx[j], s2, 0.0, nullptr);
  energy[i] = (float)e;
}

// ---- backward
__global__ __launch_bounds__(SP_T) void sp_vjp_record_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                             const int64_t * __restrict__ pairs, const int64_t * __restrict__ count,
                                                             const float * __restrict__ gpe, SpRecord * __restrict__ rec,
                                                             int64_t * __restrict__ nrec, float s2, int64_t max_pairs, int64_t V,
                                                             int64_t F, int64_t np)
{
  const int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x;
  if(i >= np) return;
  const int64_t frame = i / max_pairs, row = i % max_pairs;
  int64_t m = count[frame];
  m = m < 0 ? 0 : m > max_pairs ? max_pairs : m;
  if(row == 0) nrec[frame] = 6 * m;
  if(row >= m) return; // past the frame's records: the gather does not read them
  SpRecord * r = rec + (frame * max_pairs + row) * 6;
  const float gamma = gpe[i];
  const int64_t f = pairs[2 * i], g = pairs[2 * i + 1];
  if(gamma == 0.0f || f < 0 || f >= F || g < 0 || g >= F)
  {
    for(int k = 0; k < 6; k++) r[k].u[0] = r[k].u[1] = r[k].u[2] = r[k].u[3] = -1;
    return;
  }
  int fv[3], gv[3];
  float3 fx[3], gx[3];
  sp_pair_corners(verts + frame * V * 3, faces, f, g, fv, gv, fx, gx);
  for(int k = 0; k < 6; k++)
  {
    const bool fr = k < 3; // receiver f, intruder g's corner k; then receiver g, intruder f's corner k - 3
    const int * rv = fr ? fv : gv;
    const float3 * rx = fr ? fx : gx;
    const int iv = fr ? gv[k] : fv[k - 3];
    const float3 ix = fr ? gx[k] : fx[k - 3];
    SpRecord o;
    float grad[4][3];
    if(sp_corner<float>(rx[0], rx[1], rx[2], ix, s2, gamma, grad) != 0.0f)
    {
      o.u[0] = rv[0], o.u[1] = rv[1], o.u[2] = rv[2], o.u[3] = iv;
      for(int j = 0; j < 4; j++)
        for(int x = 0; x < 3; x++) o.g[3 * j + x] = grad[j][x];
    }
    else
    {
      o.u[0] = o.u[1] = o.u[2] = o.u[3] = -1;
      for(int j = 0; j < 4; j++)
        for(int x = 0; x < 3; x++) o.g[3 * j + x] = 0.0f;
    }
    r[k] = o;
  }
}

static SelfPenState * sp_state(smplpp_model * m)
{
  if(!m->sp) m->sp.reset(new SelfPenState());
  return m->sp.get();
}

static unsigned sp_grid(int64_t items)
{
  return (unsigned)((items + SP_T - 1) / SP_T);
}

// all pointers on the device; energy null: detection only
static int sp_forward_device(smplpp_model * m, SelfPenState * s, int64_t n, const float * verts, int64_t max_pairs, float s2,
                             int64_t * pairs, int64_t * count, float * energy, hipStream_t st)
{
  const int64_t V = m->V, F = m->F, nf = n * F;
  const int32_t * faces = m->faces.get();
  HIP_TRY(s->box.reserve(sizeof(float4) * 2 * (size_t)nf));
  HIP_TRY(s->sbox.reserve(sizeof(float4) * 2 * (size_t)nf));
  HIP_TRY(s->keys.reserve(sizeof(uint64_t) * (size_t)nf));
  HIP_TRY(s->frame.reserve(sizeof(SpFrame) * (size_t)n));
  HIP_TRY(s->cnt.reserve(sizeof(int32_t) * (size_t)nf));
  HIP_TRY(s->off.reserve(sizeof(int64_t) * (size_t)nf));
  HIP_TRY(s->fill.reserve(sizeof(int32_t) * (size_t)nf));
  HIP_TRY(s->strad.reserve(sizeof(int32_t) * (size_t)nf));
  float4 * box = s->box.as<float4>();
  float4 * sbox = s->sbox.as<float4>();
  uint64_t * keys = s->keys.as<uint64_t>();
  SpFrame * info = s->frame.as<SpFrame>();
  int32_t * cnt = s->cnt.as<int32_t>();
  int64_t * off = s->off.as<int64_t>();
  int32_t * fill = s->fill.as<int32_t>();
  int32_t * strad = s->strad.as<int32_t>();
  sp_box_kernel<<<dim3(sp_grid(nf)), dim3(SP_T), 0, st>>>(verts, faces, box, V, F, nf);
  HIP_TRY(hipGetLastError());
  sp_frame_kernel<<<dim3((unsigned)n), dim3(SP_T), 0, st>>>(box, info, F);
  HIP_TRY(hipGetLastError());
  if(F <= SP_LDS_SORT)
  {
    sp_sort_lds_kernel<<<dim3((unsigned)n), dim3(SP_SORT_T), 0, st>>>(box, info, keys, F);
    HIP_TRY(hipGetLastError());
  }
  else
  {
    HIP_TRY(s->keys_in.reserve(sizeof(uint64_t) * (size_t)nf));
    HIP_TRY(s->seg.reserve(sizeof(int) * (size_t)(n + 1)));
    uint64_t * kin = s->keys_in.as<uint64_t>();
    int * seg = s->seg.as<int>();
    sp_key_kernel<<<dim3(sp_grid(nf)), dim3(SP_T), 0, st>>>(box, info, kin, F, nf);
    HIP_TRY(hipGetLastError());
    sp_seg_kernel<<<dim3(sp_grid(n + 1)), dim3(SP_T), 0, st>>>(seg, F, n);
    HIP_TRY(hipGetLastError());
    size_t bytes = 0;
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, bytes, kin, keys, (int)nf, (int)n, seg, seg + 1, 0, 64, st));
    HIP_TRY(s->temp.reserve(bytes ? bytes : 1));
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(s->temp.as<void>(), bytes, kin, keys, (int)nf, (int)n, seg, seg + 1, 0, 64, st));
  }
  sp_scatter_kernel<<<dim3(sp_grid(nf)), dim3(SP_T), 0, st>>>(keys, box, sbox, F, nf);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)nf, st));
  sp_sweep_kernel<false><<<dim3(sp_grid(nf * SP_SPLIT)), dim3(SP_T), 0, st>>>(verts, faces, sbox, info, cnt, fill, off, strad, pairs,
                                                                              max_pairs, V, F, nf);
  HIP_TRY(hipGetLastError());
  sp_scan_kernel<<<dim3((unsigned)n), dim3(SP_SORT_T), 0, st>>>(cnt, off, count, F);
  HIP_TRY(hipGetLastError());
  if(max_pairs == 0) return SMPLPP_OK;
  HIP_TRY(hipMemsetAsync(fill, 0, sizeof(int32_t) * (size_t)nf, st));
  sp_sweep_kernel<true><<<dim3(sp_grid(nf * SP_SPLIT)), dim3(SP_T), 0, st>>>(verts, faces, sbox, info, cnt, fill, off, strad, pairs,
                                                                             max_pairs, V, F, nf);
  HIP_TRY(hipGetLastError());
  sp_order_kernel<<<dim3(sp_grid(nf)), dim3(SP_T), 0, st>>>(cnt, off, strad, pairs, max_pairs, F, nf);
  HIP_TRY(hipGetLastError());
  sp_finish_kernel<<<dim3(sp_grid(n * max_pairs)), dim3(SP_T), 0, st>>>(verts, faces, count, pairs, energy, s2, max_pairs, V,
                                                                          n * max_pairs);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int sp_vjp_device(smplpp_model * m, SelfPenState * s, int64_t n, const float * verts, int64_t max_pairs, float s2,
                         const int64_t * pairs, const int64_t * count, const float * gpe, float * gv, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, F = m->F, np = n * max_pairs;
  if(np == 0)
  {
    if(!accumulate) HIP_TRY(hipMemsetAsync(gv, 0, sizeof(float) * (size_t)(n * V * 3), st));
    return SMPLPP_OK;
  }
  HIP_TRY(s->rec.reserve(sizeof(SpRecord) * 6 * (size_t)np));
  HIP_TRY(s->nrec.reserve(sizeof(int64_t) * (size_t)n));
  SpRecord * rec = s->rec.as<SpRecord>();
  int64_t * nrec = s->nrec.as<int64_t>();
  sp_vjp_record_kernel<<<dim3(sp_grid(np)), dim3(SP_T), 0, st>>>(verts, m->faces.get(), pairs, count, gpe, rec, nrec, s2, max_pairs, V,
                                                                   F, np);
  HIP_TRY(hipGetLastError());
  return record_gather(rec, gv, accumulate, n, 6 * max_pairs, V, st, nrec);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

static int sp_check(const char * fn, smplpp_model * m, int64_t n, int64_t max_pairs, int space)
{
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": the model has no faces");
  if(max_pairs < 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": max_pairs < 0");
  // every [n,F], [n,V] and [n,max_pairs] index and every grid below stays in int32
  if(n > 0x7fffffffLL || max_pairs > 0x7fffffffLL || n * max_pairs > 0x7fffffffLL || n * m->F > 0x7fffffffLL || n * m->V > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * max_pairs, n * F or n * V beyond int32 indexing");
  return check_space(space, fn);
}

static int sp_sigma(const char * fn, float sigma)
{
  if(!(std::isfinite(sigma) && sigma > 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": sigma must be finite and > 0");
  return SMPLPP_OK;
}

static int sp_forward(const char * fn, const char * trace, smplpp_model * m, int64_t n, const float * verts, int64_t max_pairs,
                      float sigma, int64_t * pairs, int64_t * count, float * energy, int space, void * stream)
{
  int rc = sp_check(fn, m, n, max_pairs, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, trace);
  SelfPenState * s = sp_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  int64_t * po = fr.out(pairs, (size_t)(n * max_pairs * 2));
  int64_t * co = fr.out(count, (size_t)n);
  float * eo = fr.out(energy, (size_t)(n * max_pairs));
  return fr.run([&] { return sp_forward_device(m, s, n, v, max_pairs, sigma * sigma, po, co, eo, fr.st); });
}

extern "C" int smplpp_self_intersections(smplpp_model * m, int64_t n, const float * verts, int64_t max_pairs, int64_t * pairs,
                                         int64_t * count, int space, void * stream)
{
  const char * fn = "smplpp_self_intersections";
  if(!m || n <= 0 || !verts || !count || (max_pairs > 0 && !pairs)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  return sp_forward(fn, "self intersections", m, n, verts, max_pairs, 1.0f, pairs, count, nullptr, space, stream);
}

extern "C" int smplpp_self_penetration(smplpp_model * m, int64_t n, const float * verts, int64_t max_pairs, float sigma, int64_t * pairs,
                                       int64_t * count, float * pair_energy, int space, void * stream)
{
  const char * fn = "smplpp_self_penetration";
  if(!m || n <= 0 || !verts || !count || (max_pairs > 0 && (!pairs || !pair_energy)))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = sp_sigma(fn, sigma);
  if(rc) return rc;
  return sp_forward(fn, "self penetration", m, n, verts, max_pairs, sigma, pairs, count, pair_energy, space, stream);
}

extern "C" int smplpp_self_penetration_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t max_pairs, float sigma,
                                           const int64_t * pairs, const int64_t * count, const float * grad_pair_energy,
                                           float * grad_verts, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_self_penetration_vjp";
  if(!m || n <= 0 || !verts || !count || !grad_verts || (max_pairs > 0 && (!pairs || !grad_pair_energy)))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = sp_sigma(fn, sigma);
  if(!rc) rc = sp_check(fn, m, n, max_pairs, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST)
    for(int64_t i = 0; i < n; i++) // the rows of a frame that its count makes live
    {
      const int64_t rows = count[i] < 0 ? 0 : count[i] > max_pairs ? max_pairs : count[i];
      if((rc = ids_in(fn, "face id", pairs + i * max_pairs * 2, rows * 2, 0, m->F))) return rc;
    }
  Frame fr(m->device, &m->arena, space, stream, "self penetration VJP");
  SelfPenState * s = sp_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const int64_t * p = fr.in(pairs, (size_t)(n * max_pairs * 2));
  const int64_t * c = fr.in(count, (size_t)n);
  const float * g = fr.in(grad_pair_energy, (size_t)(n * max_pairs));
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  return fr.run([&] { return sp_vjp_device(m, s, n, v, max_pairs, sigma * sigma, p, c, g, gv, accumulate, fr.st); });
}
