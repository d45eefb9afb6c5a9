// Mesh-to-point distance (the other half of a two-sided scan registration loss): for every posed vertex, the nearest point of the
// frame's cloud, and its vector-Jacobian product to the vertices and the points.  A brute-force scan over the cloud; faces are not used.
//
// Forward:
//  mpd_scan_kernel    256 lanes, MPD_VPL vertices of one frame per lane in registers (vertex vb 1024 + i 256 + lane), the frame's
//                     points (or one chunk of them) streamed through LDS MPD_TILE at a time as float4: every lane reads the same
//                     point, so each LDS read is a broadcast.  Each vertex keeps a running (best_d, best_k), updated on a strict
//                     d < best_d in ascending k: the lowest k among equal distances, and a NaN or inf distance never chosen
//                     (best_d starts at +inf).  d = ((dx dx + dy dy) + dz dz), d = v - p, every operation rounded on its own.
//  mpd_reduce_kernel  when the call splits K (few frames: the grid would not fill the device), each chunk wrote a partial (d, k);
//                     one thread per (frame, vertex) takes the lexicographic (d, k) minimum over the chunks.  A minimum over a total
//                     order does not depend on how K was cut, so the bits do not depend on the split, on n or on the frame's slot.
// Backward (no search: the forward's index is an input), r = v - p[index], g = grad_sqdist:
//  mpd_vjp_record_kernel  per (frame, vertex): grad_verts = 2 g r, and the record (index, -2 g r) for grad_points.  A zero
//                         cotangent or an index out of [0, K) gives no record (key -1) and a zero grad_verts.
//  record_gather_kernel<MpdRecord>  (distance_vjp.h) grad_points: one fixed-order sum per point, ascending vertex.
#include "distance_vjp.h"
#include "scan_compat.h"

#include <cmath>

namespace smplpp_hip
{
struct MeshPointDistState
{
  DevBuf part_d, part_k; // [n][chunks][V] partial (d, k) of a split forward
  DevBuf rec;            // [n][V] MpdRecord of the backward pass
};
void StateDelete::operator()(MeshPointDistState * s) const
{
  delete s;
}

constexpr int MPD_THREADS = 256;
constexpr int MPD_VPL = 4;                            // vertices per lane
constexpr int MPD_VBLOCK = MPD_THREADS * MPD_VPL;     // vertices per workgroup
constexpr int MPD_TILE = 1024;                        // points per LDS tile (float4: 16 KiB)
constexpr int64_t MPD_TARGET_WG = 2048;               // below this many (frame, vertex block) workgroups the call splits K ...
constexpr int64_t MPD_MIN_CHUNK = 256;                // ... into chunks of at least this many points

struct MpdRecord
{
  int32_t k;   // the point (-1: no record)
  float g[3];  // -2 g r

  // record_gather_kernel's pieces: the record staged whole, as float4 (with int4 the loop branched round the reads: 2-4x slower)
  struct Tile
  {
    float4 r[GATHER_TILE];
  };
  __device__ static bool touches(const int4 & R, int lo, int hi) { return R.x >= lo && R.x < hi; }
  __device__ static void stage(Tile & t, int pos, const int4 & R, const MpdRecord &)
  {
    t.r[pos] = make_float4(__int_as_float(R.x), __int_as_float(R.y), __int_as_float(R.z), __int_as_float(R.w));
  }
  __device__ static void add(float * acc, const Tile & t, int h, int u)
  {
    const float4 R = t.r[h];
    const bool mine = __float_as_int(R.x) == u;
    acc[0] += mine ? R.y : 0.0f;
    acc[1] += mine ? R.z : 0.0f;
    acc[2] += mine ? R.w : 0.0f;
  }
};
static_assert(sizeof(MpdRecord) == 16, "MpdRecord: one 16-byte load");

// the contract's distance: ((dx dx + dy dy) + dz dz), no contraction to FMA
__device__ inline float mpd_sqdist(float vx, float vy, float vz, float px, float py, float pz)
{
#pragma clang fp contract(off)
  const float dx = vx - px, dy = vy - py, dz = vz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// K chunks of one call: from (n, K) alone (the model's V fixes the vertex blocks), so the same call always splits the same way
static int64_t mpd_chunk_len(int64_t n, int64_t K, int64_t vblocks)
{
  const int64_t wg = n * vblocks;
  if(wg >= MPD_TARGET_WG || K < 2 * MPD_MIN_CHUNK) return K;
  int64_t s = (MPD_TARGET_WG + wg - 1) / wg;
  if(s > K / MPD_MIN_CHUNK) s = K / MPD_MIN_CHUNK;
  return (K + s - 1) / s;
}

// ---- forward
__global__ __launch_bounds__(MPD_THREADS) void mpd_scan_kernel(const float * __restrict__ verts, const float * __restrict__ points,
                                                               int64_t * __restrict__ index_out, float * __restrict__ sq_out,
                                                               float * __restrict__ part_d, int32_t * __restrict__ part_k, int64_t V,
                                                               int64_t K, int64_t vblocks, int64_t chunks, int64_t chunk)
{
  __shared__ float4 s_p[MPD_TILE];
  const uint32_t b = blockIdx.x; // (the grid is below 2^31: 32-bit index arithmetic)
  const int64_t vb = b % (uint32_t)vblocks;
  const int64_t fc = b / (uint32_t)vblocks; // frame * chunks + c
  const int64_t c = (uint32_t)fc % (uint32_t)chunks, frame = (uint32_t)fc / (uint32_t)chunks;
  const int64_t k0 = c * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
  const int t = threadIdx.x;
  const float * vf = verts + frame * V * 3;
  const float * pf = points + frame * K * 3;
  float vx[MPD_VPL], vy[MPD_VPL], vz[MPD_VPL], bd[MPD_VPL];
  int bk[MPD_VPL];
#pragma unroll
  for(int i = 0; i < MPD_VPL; i++)
  {
    int64_t v = vb * MPD_VBLOCK + i * MPD_THREADS + t;
    if(v >= V) v = V - 1; // lanes past V repeat the last vertex and write nothing
    vx[i] = vf[v * 3];
    vy[i] = vf[v * 3 + 1];
    vz[i] = vf[v * 3 + 2];
    bd[i] = INFINITY;
    bk[i] = -1;
  }
  for(int64_t base = k0; base < k1; base += MPD_TILE)
  {
    const int cnt = (int)(k1 - base < MPD_TILE ? k1 - base : MPD_TILE);
    __syncthreads();
    for(int j = t; j < cnt; j += MPD_THREADS)
    {
      const float * p = pf + (base + j) * 3;
      s_p[j] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    __syncthreads();
#pragma unroll 4
    for(int j = 0; j < cnt; j++)
    {
      const float4 p = s_p[j];
      const int k = (int)base + j;
#pragma unroll
      for(int i = 0; i < MPD_VPL; i++)
      {
        const float d = mpd_sqdist(vx[i], vy[i], vz[i], p.x, p.y, p.z);
        if(d < bd[i])
        {
          bd[i] = d;
          bk[i] = k;
        }
      }
    }
  }
#pragma unroll
  for(int i = 0; i < MPD_VPL; i++)
  {
    const int64_t v = vb * MPD_VBLOCK + i * MPD_THREADS + t;
    if(v >= V) continue;
    if(chunks == 1)
    {
      index_out[frame * V + v] = bk[i];
      sq_out[frame * V + v] = bk[i] < 0 ? 0.0f : bd[i];
    }
    else
    {
      part_d[fc * V + v] = bd[i];
      part_k[fc * V + v] = bk[i];
    }
  }
}

// smplpp_mesh_point_distance_compatible: mpd_scan_kernel's scan restricted to the points with d <= max_sq whose normal passes
// compat_normals (scan_compat.h) against the vertex's (NORMALS).  The vertex normal (m, mm) sits in registers beside the vertex, the
// point normals (q, qq) pass through LDS in a second float4 tile; a non-finite normal is staged as NaN, which fails the test.  The
// same K chunks, partials and mpd_reduce_kernel: a chunk without an eligible point writes (+inf, -1).
template<bool NORMALS>
__global__ __launch_bounds__(MPD_THREADS) void mpdc_scan_kernel(const float * __restrict__ verts, const float * __restrict__ vnormals,
                                                                const float * __restrict__ points, const float * __restrict__ pnormals,
                                                                float c2, float max_sq, int64_t * __restrict__ index_out,
                                                                float * __restrict__ sq_out, float * __restrict__ part_d,
                                                                int32_t * __restrict__ part_k, int64_t V, int64_t K, int64_t vblocks,
                                                                int64_t chunks, int64_t chunk)
{
  __shared__ float4 s_p[MPD_TILE];
  __shared__ float4 s_q[NORMALS ? MPD_TILE : 1];
  const uint32_t b = blockIdx.x; // (the grid is below 2^31: 32-bit index arithmetic)
  const int64_t vb = b % (uint32_t)vblocks;
  const int64_t fc = b / (uint32_t)vblocks; // frame * chunks + c
  const int64_t c = (uint32_t)fc % (uint32_t)chunks, frame = (uint32_t)fc / (uint32_t)chunks;
  const int64_t k0 = c * chunk, k1 = k0 + chunk < K ? k0 + chunk : K;
  const int t = threadIdx.x;
  const float * vf = verts + frame * V * 3;
  const float * pf = points + frame * K * 3;
  float vx[MPD_VPL], vy[MPD_VPL], vz[MPD_VPL], bd[MPD_VPL];
  float4 vm[MPD_VPL];
  int bk[MPD_VPL];
#pragma unroll
  for(int i = 0; i < MPD_VPL; i++)
  {
    int64_t v = vb * MPD_VBLOCK + i * MPD_THREADS + t;
    if(v >= V) v = V - 1; // lanes past V repeat the last vertex and write nothing
    vx[i] = vf[v * 3];
    vy[i] = vf[v * 3 + 1];
    vz[i] = vf[v * 3 + 2];
    vm[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr(NORMALS)
    {
      const float * nf = vnormals + (frame * V + v) * 3;
      const float nx = nf[0], ny = nf[1], nz = nf[2];
      vm[i] = compat_finite3(nx, ny, nz) ? make_float4(nx, ny, nz, compat_dot(nx, ny, nz, nx, ny, nz)) : make_float4(NAN, NAN, NAN, NAN);
    }
    bd[i] = INFINITY;
    bk[i] = -1;
  }
  for(int64_t base = k0; base < k1; base += MPD_TILE)
  {
    const int cnt = (int)(k1 - base < MPD_TILE ? k1 - base : MPD_TILE);
    __syncthreads();
    for(int j = t; j < cnt; j += MPD_THREADS)
    {
      const float * p = pf + (base + j) * 3;
      s_p[j] = make_float4(p[0], p[1], p[2], 0.0f);
      if constexpr(NORMALS)
      {
        const float * qf = pnormals + (frame * K + base + j) * 3;
        const float qx = qf[0], qy = qf[1], qz = qf[2];
        s_q[j] = compat_finite3(qx, qy, qz) ? make_float4(qx, qy, qz, compat_dot(qx, qy, qz, qx, qy, qz)) : make_float4(NAN, NAN, NAN, NAN);
      }
    }
    __syncthreads();
#pragma unroll 4
    for(int j = 0; j < cnt; j++)
    {
      const float4 p = s_p[j];
      const int k = (int)base + j;
#pragma unroll
      for(int i = 0; i < MPD_VPL; i++)
      {
        const float d = mpd_sqdist(vx[i], vy[i], vz[i], p.x, p.y, p.z);
        if(d < bd[i] && d <= max_sq)
        {
          bool take = true;
          if constexpr(NORMALS) take = compat_normals(vm[i], s_q[j], c2);
          if(take)
          {
            bd[i] = d;
            bk[i] = k;
          }
        }
      }
    }
  }
#pragma unroll
  for(int i = 0; i < MPD_VPL; i++)
  {
    const int64_t v = vb * MPD_VBLOCK + i * MPD_THREADS + t;
    if(v >= V) continue;
    if(chunks == 1)
    {
      index_out[frame * V + v] = bk[i];
      sq_out[frame * V + v] = bk[i] < 0 ? 0.0f : bd[i];
    }
    else
    {
      part_d[fc * V + v] = bd[i];
      part_k[fc * V + v] = bk[i];
    }
  }
}

__global__ __launch_bounds__(256) void mpd_reduce_kernel(const float * __restrict__ part_d, const int32_t * __restrict__ part_k,
                                                         int64_t * __restrict__ index_out, float * __restrict__ sq_out, int64_t V,
                                                         int64_t chunks, int64_t nv)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nv) return;
  const int64_t frame = i / V, v = i % V;
  float bd = INFINITY;
  int bk = -1;
#pragma unroll 8
  for(int64_t c = 0; c < chunks; c++) // (unrolled: the partials' loads are independent and go out together)
  {
    const int64_t j = (frame * chunks + c) * V + v;
    const int k = part_k[j];
    const float d = part_d[j];
    if(k >= 0 && (bk < 0 || d < bd || (d == bd && k < bk)))
    {
      bd = d;
      bk = k;
    }
  }
  index_out[i] = bk;
  sq_out[i] = bk < 0 ? 0.0f : bd;
}

// ---- backward
__global__ __launch_bounds__(256) void mpd_vjp_record_kernel(const float * __restrict__ verts, const float * __restrict__ points,
                                                             const int64_t * __restrict__ index, const float * __restrict__ gsq,
                                                             MpdRecord * __restrict__ rec, float * __restrict__ gv, int accumulate,
                                                             int64_t V, int64_t K, int64_t nv)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nv) return;
  const float g = gsq[i];
  const int64_t k = index[i];
  MpdRecord r;
  r.k = -1;
  r.g[0] = r.g[1] = r.g[2] = 0.0f;
  float gvt[3] = {0.0f, 0.0f, 0.0f};
  if(g != 0.0f && k >= 0 && k < K)
  {
    const float * p = points + ((i / V) * K + k) * 3;
    const float rr[3] = {verts[i * 3] - p[0], verts[i * 3 + 1] - p[1], verts[i * 3 + 2] - p[2]};
    const float s = 2.0f * g, sn = -2.0f * g;
    r.k = (int32_t)k;
    for(int x = 0; x < 3; x++)
    {
      gvt[x] = s * rr[x];
      r.g[x] = sn * rr[x];
    }
  }
  if(rec) rec[i] = r;
  if(gv)
    for(int x = 0; x < 3; x++) gv[i * 3 + x] = accumulate ? gv[i * 3 + x] + gvt[x] : gvt[x];
}

static MeshPointDistState * mpd_state(smplpp_model * m)
{
  if(!m->mpd) m->mpd.reset(new MeshPointDistState());
  return m->mpd.get();
}

// all pointers on the device
static int mpd_forward_device(smplpp_model * m, MeshPointDistState * s, int64_t n, const float * verts, int64_t K, const float * points,
                              int64_t * index, float * sqdist, hipStream_t st)
{
  const int64_t V = m->V;
  const int64_t vblocks = (V + MPD_VBLOCK - 1) / MPD_VBLOCK;
  const int64_t chunk = mpd_chunk_len(n, K, vblocks);
  const int64_t chunks = (K + chunk - 1) / chunk;
  float * pd = nullptr;
  int32_t * pk = nullptr;
  if(chunks > 1)
  {
    HIP_TRY(s->part_d.reserve(sizeof(float) * (size_t)(n * chunks * V)));
    HIP_TRY(s->part_k.reserve(sizeof(int32_t) * (size_t)(n * chunks * V)));
    pd = s->part_d.as<float>();
    pk = s->part_k.as<int32_t>();
  }
  mpd_scan_kernel<<<dim3((unsigned)(n * chunks * vblocks)), dim3(MPD_THREADS), 0, st>>>(verts, points, index, sqdist, pd, pk, V, K, vblocks,
                                                                                        chunks, chunk);
  HIP_TRY(hipGetLastError());
  if(chunks > 1)
  {
    mpd_reduce_kernel<<<dim3((unsigned)((n * V + 255) / 256)), dim3(256), 0, st>>>(pd, pk, index, sqdist, V, chunks, n * V);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}

// smplpp_mesh_point_distance_compatible, all pointers on the device: NORMALS when both normal arrays are given
template<bool NORMALS>
static int mpdc_forward_device(smplpp_model * m, MeshPointDistState * s, int64_t n, const float * verts, const float * vnormals, int64_t K,
                               const float * points, const float * pnormals, float c2, float max_sq, int64_t * index, float * sqdist,
                               hipStream_t st)
{
  const int64_t V = m->V;
  const int64_t vblocks = (V + MPD_VBLOCK - 1) / MPD_VBLOCK;
  const int64_t chunk = mpd_chunk_len(n, K, vblocks);
  const int64_t chunks = (K + chunk - 1) / chunk;
  float * pd = nullptr;
  int32_t * pk = nullptr;
  if(chunks > 1)
  {
    HIP_TRY(s->part_d.reserve(sizeof(float) * (size_t)(n * chunks * V)));
    HIP_TRY(s->part_k.reserve(sizeof(int32_t) * (size_t)(n * chunks * V)));
    pd = s->part_d.as<float>();
    pk = s->part_k.as<int32_t>();
  }
  mpdc_scan_kernel<NORMALS><<<dim3((unsigned)(n * chunks * vblocks)), dim3(MPD_THREADS), 0, st>>>(verts, vnormals, points, pnormals, c2, max_sq,
                                                                                                  index, sqdist, pd, pk, V, K, vblocks, chunks,
                                                                                                  chunk);
  HIP_TRY(hipGetLastError());
  if(chunks > 1)
  {
    mpd_reduce_kernel<<<dim3((unsigned)((n * V + 255) / 256)), dim3(256), 0, st>>>(pd, pk, index, sqdist, V, chunks, n * V);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}

static int mpd_vjp_device(smplpp_model * m, MeshPointDistState * s, int64_t n, const float * verts, int64_t K, const float * points,
                          const int64_t * index, const float * gsq, float * gv, float * gp, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, nv = n * V;
  MpdRecord * rec = nullptr;
  if(gp)
  {
    HIP_TRY(s->rec.reserve(sizeof(MpdRecord) * (size_t)nv));
    rec = s->rec.as<MpdRecord>();
  }
  mpd_vjp_record_kernel<<<dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st>>>(verts, points, index, gsq, rec, gv, accumulate, V, K, nv);
  HIP_TRY(hipGetLastError());
  return gp ? record_gather(rec, gp, accumulate, n, V, K, st) : SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

static int mpd_check(const char * fn, smplpp_model * m, int64_t n, int64_t K, int space)
{
  // every [n,K] and [n,V] index, every partial [n][chunks][V] index and every grid below stays in int32
  if(n > 0x7fffffffLL || K > 0x7fffffffLL || n * K > 0x7fffffffLL || n * m->V > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * K or n * V beyond int32 indexing");
  return check_space(space, fn);
}

extern "C" int smplpp_mesh_point_distance(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points, int64_t * index,
                                          float * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_mesh_point_distance";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !index || !sqdist) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = mpd_check(fn, m, n, K, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "mesh-point distance");
  MeshPointDistState * s = mpd_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  int64_t * io = fr.out(index, (size_t)n * m->V);
  float * so = fr.out(sqdist, (size_t)n * m->V);
  return fr.run([&] { return mpd_forward_device(m, s, n, v, K, p, io, so, fr.st); });
}

extern "C" int smplpp_mesh_point_distance_compatible(smplpp_model * m, int64_t n, const float * verts, const float * vert_normals, int64_t K,
                                                     const float * points, const float * point_normals, float cos_min, float max_sqdist,
                                                     int64_t * index, float * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_mesh_point_distance_compatible";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !index || !sqdist) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = compat_args(fn, cos_min, max_sqdist);
  if(rc) return rc;
  if((rc = mpd_check(fn, m, n, K, space))) return rc;
  const bool normals = vert_normals && point_normals; // the test needs both sides
  Frame fr(m->device, &m->arena, space, stream, "mesh-point distance (compatible)");
  MeshPointDistState * s = mpd_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * vn = normals ? fr.in(vert_normals, (size_t)n * m->V * 3) : nullptr;
  const float * p = fr.in(points, (size_t)n * K * 3);
  const float * pn = normals ? fr.in(point_normals, (size_t)n * K * 3) : nullptr;
  int64_t * io = fr.out(index, (size_t)n * m->V);
  float * so = fr.out(sqdist, (size_t)n * m->V);
  const float c2 = cos_min * cos_min;
  return fr.run([&] {
    return normals ? mpdc_forward_device<true>(m, s, n, v, vn, K, p, pn, c2, max_sqdist, io, so, fr.st)
                   : mpdc_forward_device<false>(m, s, n, v, nullptr, K, p, nullptr, c2, max_sqdist, io, so, fr.st);
  });
}

extern "C" int smplpp_mesh_point_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                              const int64_t * index, const float * grad_sqdist, float * grad_verts, float * grad_points,
                                              int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_mesh_point_distance_vjp";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !index || !grad_sqdist || (!grad_verts && !grad_points))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = mpd_check(fn, m, n, K, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "point index", index, n * m->V, -1, K))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "mesh-point distance VJP");
  return distance_vjp(fr, mpd_vjp_device, m, mpd_state(m), n, verts, K, points, index, n * m->V, grad_sqdist, grad_verts, grad_points,
                      accumulate);
}
