// Ray casting against each frame's posed mesh: the first hit of K rays per frame, the hit counts, and the
// vector-Jacobian product of the range.  The rule is in ray_cast_device.h and in full in include/smplpp_hip.h; every fp32 operation
// is rounded on its own, every output is decided by integers or by one fixed-order sum, and there are no floating-point atomics.
//
//  rc_scan_kernel    wn_scan_kernel's loop: one ray per lane, in registers (64..256 lanes per workgroup, from K), the frame's faces
//                    gathered into LDS 256 at a time (every lane reads the same face: broadcasts).  A lane keeps the least key
//                    bits(t) << 32 | face of its accepted candidates and their front and back counts.  With few (frame, ray block)
//                    workgroups the call deals the 256-face chunks over `slices` workgroups (from n and K alone, or
//                    SMPLPP_RAY_SLICES); the slices meet in key [n,K] through a 64-bit integer minimum and in hits through integer adds,
//                    both set up by the call, so no bit depends on the split.
//  rc_finish_kernel  per (frame, ray): the key unpacked into face and t, and the barycentrics of the hit recomputed on its face.
//  rc_record_kernel  backward: per (frame, ray) the range recomputed on the named face (ray_plane, as the scan forms it), one record of
//                    the three corners, their shares beta and vec = (g / nd) n for record_gather (distance_vjp.h), and the ray's own
//                    terms -vec and -t vec, stored, added, or kept per frame for the sum over the frames of shared rays.
//  rc_frames_kernel  shared rays: per element the frames' terms in the two-level tile order of smplpp_vertex_offsets_vjp.
#include "distance_vjp.h"
#include "ray_cast_device.h"

#include <cmath>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int RC_CHUNK = 256;             // faces per LDS chunk
constexpr int64_t RC_TARGET_WAVES = 8192; // below this many wavefronts (256 CUs x 32) the call splits the chunks
constexpr int RC_FT = SMPLPP_VERTEX_OFFSETS_TILE; // frames per tile of a shared ray's sum

struct RcRecord
{
  int32_t u[4]; // the face's vertex ids (-1: no record), pad
  float w[3];   // the corners' shares: the barycentrics of the hit
  float vec[3]; // (g / nd) n
  float pad[2];

  struct Tile
  {
    int4 u[GATHER_TILE];
    float s[GATHER_TILE][6];
  };
  __device__ static bool touches(const int4 & U, int lo, int hi)
  {
    return (U.x >= lo && U.x < hi) || (U.y >= lo && U.y < hi) || (U.z >= lo && U.z < hi);
  }
  __device__ static void stage(Tile & t, int pos, const int4 & U, const RcRecord & r)
  {
    t.u[pos] = U;
    for(int e = 0; e < 3; e++) t.s[pos][e] = r.w[e], t.s[pos][3 + e] = r.vec[e];
  }
  __device__ static void add(float * acc, const Tile & t, int h, int u)
  {
    const int4 U = t.u[h];
    if(U.x == u)
      for(int x = 0; x < 3; x++) acc[x] += t.s[h][0] * t.s[h][3 + x];
    if(U.y == u)
      for(int x = 0; x < 3; x++) acc[x] += t.s[h][1] * t.s[h][3 + x];
    if(U.z == u)
      for(int x = 0; x < 3; x++) acc[x] += t.s[h][2] * t.s[h][3 + x];
  }
};
static_assert(sizeof(RcRecord) == 48, "RcRecord: three 16-byte loads");

struct RayCastState
{
  DevBuf key;   // [n][K] uint64: the least bits(t) << 32 | face of each ray
  DevBuf rec;   // [n][K] RcRecord of the backward pass
  DevBuf terms; // [2][n][K][3] per-frame terms of grad_origin and grad_dir of shared rays
};
void StateDelete::operator()(RayCastState * s) const
{
  delete s;
}

static int64_t rc_threads(int64_t K) // lanes per workgroup: 256, or K rounded up to whole wavefronts
{
  return K >= 256 ? 256 : (K + 63) / 64 * 64;
}

// chunks per slice: from (n, K) alone, or from the model's fixed slice count
static int64_t rc_per_slice(const smplpp_model * m, int64_t n, int64_t K, int64_t chunks)
{
  int64_t s;
  if(m->ray_slices > 0) s = m->ray_slices;
  else
  {
    const int64_t T = rc_threads(K);
    const int64_t waves = n * ((K + T - 1) / T) * (T / 64);
    if(waves >= RC_TARGET_WAVES) return chunks;
    s = (RC_TARGET_WAVES + waves - 1) / waves;
  }
  if(s > chunks) s = chunks;
  return (chunks + s - 1) / s;
}

// the face's corners into t[9]; all NaN when one is not finite (such a face covers nothing)
__device__ inline void rc_load_face(const float * __restrict__ vf, const int32_t * __restrict__ face, float * t)
{
  bool fin = true;
#pragma unroll
  for(int v = 0; v < 3; v++)
  {
    const float * x = vf + 3 * (int64_t)face[v];
    for(int c = 0; c < 3; c++)
    {
      t[v * 3 + c] = x[c];
      fin = fin && fabsf(x[c]) < INFINITY;
    }
  }
  if(!fin)
    for(int e = 0; e < 9; e++) t[e] = NAN;
}

__global__ __launch_bounds__(256) void rc_scan_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                      const float * __restrict__ origin, const float * __restrict__ dir,
                                                      unsigned long long * __restrict__ key, int32_t * __restrict__ hits, int64_t V, int64_t F,
                                                      int64_t K, int64_t kblocks, int64_t slices, int64_t per_slice, int shared, float t_min,
                                                      float t_max, int facing)
{
  __shared__ float tri[RC_CHUNK][9];
  const uint32_t b = blockIdx.x; // (the grid is below 2^31)
  const int64_t kb = b % (uint32_t)kblocks, fs = b / (uint32_t)kblocks;
  const int64_t s = (uint32_t)fs % (uint32_t)slices, frame = (uint32_t)fs / (uint32_t)slices;
  const int64_t k = kb * blockDim.x + threadIdx.x;
  const bool live = k < K;
  const int64_t q = (shared ? 0 : frame) * K + (live ? k : K - 1); // lanes past K repeat the last ray and write nothing
  const Ray r = ray_setup(origin + q * 3, dir + q * 3);
  const float * vf = verts + frame * V * 3;
  const int64_t chunks = (F + RC_CHUNK - 1) / RC_CHUNK;
  const int64_t c0 = s * per_slice, c1 = c0 + per_slice < chunks ? c0 + per_slice : chunks;
  unsigned long long best = RAY_NONE;
  int nfront = 0, nback = 0;
  for(int64_t c = c0; c < c1; c++)
  {
    const int64_t f0 = c * RC_CHUNK;
    for(int j = threadIdx.x; j < RC_CHUNK; j += blockDim.x)
      if(f0 + j < F) rc_load_face(vf, faces + (f0 + j) * 3, tri[j]);
    __syncthreads();
    const int cnt = (int)(F - f0 < RC_CHUNK ? F - f0 : RC_CHUNK);
    for(int j = 0; j < cnt; j++)
    {
      float t;
      const int side = ray_face(r, tri[j], t_min, t_max, facing, t);
      if(side)
      {
        const unsigned long long cand = (unsigned long long)__float_as_uint(t) << 32 | (unsigned long long)(uint32_t)(f0 + j);
        best = cand < best ? cand : best;
        nfront += side == RAY_FRONT, nback += side == RAY_BACK;
      }
    }
    __syncthreads();
  }
  if(!live) return;
  const int64_t i = frame * K + k;
  if(best != RAY_NONE) atomicMin(key + i, best);
  if(hits && nfront) atomicAdd(hits + i * 2, nfront);
  if(hits && nback) atomicAdd(hits + i * 2 + 1, nback);
}

__global__ __launch_bounds__(256) void rc_finish_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                        const float * __restrict__ origin, const float * __restrict__ dir,
                                                        const unsigned long long * __restrict__ key, int64_t * __restrict__ face,
                                                        float * __restrict__ t, float * __restrict__ bary, int64_t V, int64_t K, int64_t nk,
                                                        int shared)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nk) return;
  const unsigned long long best = key[i];
  const bool hit = best != RAY_NONE;
  const int64_t f = hit ? (int64_t)(best & 0xffffffffull) : -1;
  const float tt = hit ? __uint_as_float((uint32_t)(best >> 32)) : 0.0f;
  face[i] = f;
  t[i] = tt;
  if(!bary) return;
  float beta[3] = {0.0f, 0.0f, 0.0f};
  if(hit)
  {
    const int64_t frame = i / K, q = shared ? i % K : i;
    const Ray r = ray_setup(origin + q * 3, dir + q * 3);
    float tri[9];
    rc_load_face(verts + frame * V * 3, faces + f * 3, tri);
    ray_bary(r, ray_plane(r, tri), tt, beta);
  }
  for(int x = 0; x < 3; x++) bary[i * 3 + x] = beta[x];
}

// go / gd: grad_origin / grad_dir (nullable) when the rays are per frame or n = 1 (stored, or added with accumulate), else the
// per-frame terms of the shared sum (always stored)
__global__ __launch_bounds__(256) void rc_record_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                        const float * __restrict__ origin, const float * __restrict__ dir,
                                                        const int64_t * __restrict__ face, const float * __restrict__ grad_t,
                                                        RcRecord * __restrict__ rec, float * go, float * gd, int64_t V, int64_t F, int64_t K,
                                                        int64_t nk, int shared, int accumulate)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nk) return;
  const int64_t frame = i / K, q = shared ? i % K : i;
  const int64_t f = face[i];
  const float g = grad_t[i];
  RcRecord R;
  R.u[0] = R.u[1] = R.u[2] = R.u[3] = -1;
  for(int x = 0; x < 3; x++) R.w[x] = 0.0f, R.vec[x] = 0.0f;
  R.pad[0] = R.pad[1] = 0.0f;
  float to[3] = {0.0f, 0.0f, 0.0f}, td[3] = {0.0f, 0.0f, 0.0f};
  if(f >= 0 && f < F && g != 0.0f)
  {
    const Ray r = ray_setup(origin + q * 3, dir + q * 3);
    if(!r.dead)
    {
      // (the face is read as it is given: a cotangent on NaN data gives NaN)
      float tri[9];
      const int32_t * c = faces + f * 3;
      for(int v = 0; v < 3; v++)
        for(int x = 0; x < 3; x++) tri[v * 3 + x] = verts[(frame * V + c[v]) * 3 + x];
      const RayPlane p = ray_plane(r, tri);
      ray_bary(r, p, p.t, R.w);
      const float gn = g / p.nd;
      for(int x = 0; x < 3; x++)
      {
        R.vec[x] = gn * p.n[x];
        to[x] = -R.vec[x];
        td[x] = -(p.t * R.vec[x]);
      }
      R.u[0] = c[0], R.u[1] = c[1], R.u[2] = c[2];
    }
  }
  if(rec) rec[i] = R;
  for(int x = 0; x < 3; x++)
  {
    if(go) go[i * 3 + x] = accumulate ? go[i * 3 + x] + to[x] : to[x];
    if(gd) gd[i * 3 + x] = accumulate ? gd[i * 3 + x] + td[x] : td[x];
  }
}

// terms [n][K3] -> out [K3]: tiles of RC_FT frames, ascending within a tile from its first term, then across the tiles
__global__ __launch_bounds__(256) void rc_frames_kernel(const float * __restrict__ terms, float * __restrict__ out, int64_t n, int64_t K3,
                                                        int accumulate)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(e >= K3) return;
  float tile = 0.0f, tot = 0.0f;
  for(int64_t f = 0; f < n; f++)
  {
    const float term = terms[f * K3 + e];
    tile = f % RC_FT == 0 ? term : tile + term;
    if(f % RC_FT == RC_FT - 1 || f == n - 1) tot = f < RC_FT ? tile : tot + tile;
  }
  out[e] = accumulate ? out[e] + tot : tot;
}

static RayCastState * rc_state(smplpp_model * m)
{
  if(!m->rc) m->rc.reset(new RayCastState());
  return m->rc.get();
}
} // namespace smplpp_hip

using namespace smplpp_hip;

static int rc_check(const char * fn, smplpp_model * m, int64_t n, int64_t ray_frames, int64_t K, int space)
{
  const std::string name(fn);
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, name + ": the model has no faces");
  if(ray_frames != 1 && ray_frames != n) return fail(SMPLPP_ERR_INVALID, name + ": ray_frames must be 1 or n");
  // every [n,K], [n,V] and [n,F] index and every grid stays in int32
  if(n > 0x7fffffffLL || K > 0x7fffffffLL || n * K > 0x7fffffffLL || n * m->V > 0x7fffffffLL || n * m->F > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, name + ": n * K, n * V or n * F beyond int32 indexing");
  return check_space(space, fn);
}

extern "C" int smplpp_ray_cast(smplpp_model * m, int64_t n, const float * verts, int64_t ray_frames, int64_t K, const float * origin,
                               const float * dir, float t_min, float t_max, int facing, int64_t * face, float * t, float * bary, int32_t * hits,
                               int space, void * stream)
{
  const char * fn = "smplpp_ray_cast";
  if(!m || n <= 0 || K < 1 || !verts || !origin || !dir || !face || !t) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(!(std::isfinite(t_min) && t_min >= 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": t_min must be finite and >= 0");
  if(!(t_max > t_min)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": t_max must be above t_min"); // (a NaN fails; +inf passes)
  if(facing < 1 || facing > 3) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": facing must be 1 (front), 2 (back) or 3 (both)");
  int rc = rc_check(fn, m, n, ray_frames, K, space);
  if(rc) return rc;
  const int64_t F = m->F, chunks = (F + RC_CHUNK - 1) / RC_CHUNK;
  const int64_t T = rc_threads(K), kblocks = (K + T - 1) / T;
  const int64_t per = rc_per_slice(m, n, K, chunks), slices = (chunks + per - 1) / per;
  if(n * kblocks * slices > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grid beyond int32");
  Frame fr(m->device, &m->arena, space, stream, "ray cast");
  RayCastState * s = rc_state(m);
  const int shared = ray_frames == 1 && n > 1;
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * o = fr.in(origin, (size_t)ray_frames * K * 3);
  const float * d = fr.in(dir, (size_t)ray_frames * K * 3);
  int64_t * fo = fr.out(face, (size_t)n * K);
  float * to = fr.out(t, (size_t)n * K);
  float * bo = fr.out(bary, (size_t)n * K * 3);
  int32_t * ho = fr.out(hits, (size_t)n * K * 2);
  return fr.run([&]() -> int {
    const int64_t nk = n * K;
    HIP_TRY(s->key.reserve(sizeof(unsigned long long) * (size_t)nk));
    unsigned long long * key = s->key.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(key, 0xff, sizeof(unsigned long long) * (size_t)nk, fr.st));
    if(ho) HIP_TRY(hipMemsetAsync(ho, 0, sizeof(int32_t) * (size_t)nk * 2, fr.st));
    rc_scan_kernel<<<dim3((unsigned)(n * kblocks * slices)), dim3((unsigned)T), 0, fr.st>>>(v, m->faces.get(), o, d, key, ho, m->V, F, K, kblocks,
                                                                                          slices, per, shared, t_min, t_max, facing);
    HIP_TRY(hipGetLastError());
    rc_finish_kernel<<<dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, fr.st>>>(v, m->faces.get(), o, d, key, fo, to, bo, m->V, K, nk, shared);
    HIP_TRY(hipGetLastError());
    return SMPLPP_OK;
  });
}

extern "C" int smplpp_ray_cast_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t ray_frames, int64_t K, const float * origin,
                                   const float * dir, const int64_t * face, const float * grad_t, float * grad_verts, float * grad_origin,
                                   float * grad_dir, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_ray_cast_vjp";
  if(!m || n <= 0 || K < 1 || !verts || !origin || !dir || !face || !grad_t || (!grad_verts && !grad_origin && !grad_dir))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = rc_check(fn, m, n, ray_frames, K, space);
  if(rc) return rc;
  if(n * ((m->V + GATHER_T - 1) / GATHER_T) > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grid beyond int32");
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * K, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "ray cast VJP");
  RayCastState * s = rc_state(m);
  const int shared = ray_frames == 1 && n > 1;
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * o = fr.in(origin, (size_t)ray_frames * K * 3);
  const float * d = fr.in(dir, (size_t)ray_frames * K * 3);
  const int64_t * id = fr.in(face, (size_t)n * K);
  const float * g = fr.in(grad_t, (size_t)n * K);
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  float * go = fr.out(grad_origin, (size_t)ray_frames * K * 3, accumulate);
  float * gd = fr.out(grad_dir, (size_t)ray_frames * K * 3, accumulate);
  return fr.run([&]() -> int {
    const int64_t nk = n * K, K3 = K * 3;
    RcRecord * rec = nullptr;
    if(gv)
    {
      HIP_TRY(s->rec.reserve(sizeof(RcRecord) * (size_t)nk));
      rec = s->rec.as<RcRecord>();
    }
    float *po = go, *pd = gd; // where the record kernel puts the rays' own terms
    if(shared && (go || gd))
    {
      HIP_TRY(s->terms.reserve(sizeof(float) * 2 * (size_t)nk * 3));
      po = go ? s->terms.as<float>() : nullptr;
      pd = gd ? s->terms.as<float>() + nk * 3 : nullptr;
    }
    rc_record_kernel<<<dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, fr.st>>>(v, m->faces.get(), o, d, id, g, rec, po, pd, m->V, m->F, K, nk,
                                                                                shared, shared ? 0 : accumulate);
    HIP_TRY(hipGetLastError());
    if(shared)
      for(int which = 0; which < 2; which++)
        if(float * out = which ? gd : go)
        {
          rc_frames_kernel<<<dim3((unsigned)((K3 + 255) / 256)), dim3(256), 0, fr.st>>>(which ? pd : po, out, n, K3, accumulate);
          HIP_TRY(hipGetLastError());
        }
    if(gv) return record_gather<RcRecord>(rec, gv, accumulate, n, K, m->V, fr.st);
    return (int)SMPLPP_OK;
  });
}
