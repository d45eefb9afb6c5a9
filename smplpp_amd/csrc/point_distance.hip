// Point-to-mesh distance for many query points per frame (fitting to an unlabelled point cloud or scan) and its vector-Jacobian
// product to the posed vertices and the points.  The forward returns the bits of smplpp_closest_points (mesh.hip, the re-projection
// igl::point_mesh_squared_distance does at node/node.cpp:970-1001) plus the closest point's vertex weights.
//
// Forward, two forms (dispatch by the call's query count n K, or SMPLPP_POINT_DISTANCE_FORM read at model creation):
//  pd_query_kernel       one 256-thread workgroup per query over closest_point_block (mesh_device.h), then the weights of the
//                        chosen face: the form for few queries per call (n K < PD_TILED_MIN_NK).
//  pd_tri_image_kernel   per call: the triangle image [n][F][3] float4 = (a, r) (b, 0) (c, 0), r = the cull radius of
//                        tri_culled_v, so a workgroup reads every triangle once, coalesced.
//  pd_sort_kernel        one workgroup per frame: a counting sort of the frame's queries by 12-bit Morton cell of their bounding box,
//                        so the 64 lanes of a wavefront hold nearby queries and cull together.  (The order within a cell is not
//                        fixed; no result depends on it.)
//  pd_tiled_kernel       64 queries per workgroup, one per lane and in registers; its 16 wavefronts split every face and seed
//                        vertex range, and the triangles pass through LDS 1024 at a time:
//                          seed   the squared distance to the nearest vertex that has a face: an upper bound of the surface distance;
//                          pass 1 the minimum mn over the faces the cull (against min(seed, running minimum)) keeps;
//                          pass 2 the lowest face id with d <= mn (1 + 1e-6) + 1e-12, the cull against that band.
//                        Both culls are tri_culled_v's conservative sphere test, so the minimum and every face of the band are
//                        evaluated; a minimum over fp32 values and the lowest id of a band do not depend on the scan order, and
//                        every distance comes from the one noinline tri_sqdist_vals, so the bits are smplpp_closest_points'.
// Compatible, distance-capped forward (smplpp_point_mesh_distance_compatible): pdc_query_kernel / pdc_tri_image_kernel /
//  pdc_tiled_kernel<NORMALS> beside the kernels above, which stay as they are: the same two passes over the faces that pass the
//  normal test of scan_compat.h and lie within max_sq, no seed, unmatched queries written as (-1, +0).
// Backward (no search: the forward's face is an input):
//  pd_vjp_record_kernel  per query: c and w recomputed with the forward's evaluation, r = p - c; grad_points = 2 g r and the record
//                        (the face's three vertex ids, -2 g w_j r for j = 0..2).  A zero cotangent or an out-of-range face gives no
//                        record (ids -1) and a zero grad_points.
//  record_gather_kernel<PdRecord>  (distance_vjp.h) grad_verts: one fixed-order sum per vertex, ascending record index, then corner.
#include "mesh_device.h"
#include "point_distance.h"
#include "scan_compat.h"

#include <cmath>

namespace smplpp_hip
{
void StateDelete::operator()(PointDistState * s) const
{
  delete s;
}

constexpr int64_t PD_TILED_MIN_NK = 8192; // the tiled form from this many queries per call (n K) on (measured crossover)
constexpr int PD_WAVES = 16;                  // wavefronts per workgroup of the tiled form, all on the same 64 queries
constexpr int PD_THREADS = 64 * PD_WAVES;
constexpr int PD_TILE = 64 * PD_WAVES;        // faces per LDS tile (64 per wavefront)
constexpr int PD_VTILE = 3 * PD_TILE;         // seed vertices per LDS tile (the same 48 KiB)
constexpr int PD_MORTON_BITS = 4;  // per axis: 4096 cells

struct PdRecord
{
  int32_t u[4];   // the face's vertex ids (-1: no record), pad
  float g[3][3];  // -2 g w_j r per corner j
  float pad[3];

  // record_gather_kernel's pieces: the ids and the nine shares staged apart (no padding in LDS)
  struct Tile
  {
    int4 u[GATHER_TILE];
    float g[GATHER_TILE][9];
  };
  __device__ static bool touches(const int4 & U, int lo, int hi)
  {
    return (U.x >= lo && U.x < hi) || (U.y >= lo && U.y < hi) || (U.z >= lo && U.z < hi);
  }
  __device__ static void stage(Tile & t, int pos, const int4 & U, const PdRecord & r)
  {
    t.u[pos] = U;
    for(int e = 0; e < 9; e++) t.g[pos][e] = r.g[0][e];
  }
  __device__ static void add(float * acc, const Tile & t, int h, int u)
  {
    const int4 U = t.u[h];
    if(U.x == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][x];
    if(U.y == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][3 + x];
    if(U.z == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][6 + x];
  }
};
static_assert(sizeof(PdRecord) == 64, "PdRecord: four 16-byte loads");

// weights of the branch that produced closest_on_triangle_dev's point (values in, values out, like tri_sqdist_vals)
__device__ inline void tri_weights_vals(float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2, float p0,
                                        float p1, float p2, float * w)
{
  const float a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2}, cc[3] = {c0, c1, c2}, p[3] = {p0, p1, p2};
  float c[3];
  closest_on_triangle_t<true>(p, a, b, cc, c, w);
}

// tri_culled_v with the radius r = sqrt(max(|b - a|^2, |c - a|^2)) precomputed in the triangle image
__device__ inline bool pd_culled(const float4 & A, float p0, float p1, float p2, float sqrt_lim)
{
  const float d0 = (p0 - A.x) * (p0 - A.x) + (p1 - A.y) * (p1 - A.y) + (p2 - A.z) * (p2 - A.z);
  const float reach = (sqrt_lim + A.w) * 1.00001f + 1e-7f;
  return d0 > reach * reach;
}

// ---- per-query form
__global__ __launch_bounds__(256) void pd_query_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                       const float * __restrict__ points, int64_t * __restrict__ face_out,
                                                       float * __restrict__ w_out, float * __restrict__ closest_out,
                                                       float * __restrict__ sq_out, int64_t V, int64_t F, int64_t K)
{
  __shared__ int64_t s_face;
  __shared__ float s_c[3], s_sq;
  const int64_t i = blockIdx.x;
  const float * vf = verts + (i / K) * V * 3;
  closest_point_block(vf, faces, F, points + i * 3, &s_face, s_c, &s_sq);
  if(threadIdx.x != 0) return;
  const int64_t b = s_face;
  face_out[i] = b;
  sq_out[i] = s_sq;
  if(closest_out)
  {
    closest_out[i * 3] = s_c[0];
    closest_out[i * 3 + 1] = s_c[1];
    closest_out[i * 3 + 2] = s_c[2];
  }
  if(w_out)
  {
    const float * a = vf + 3 * faces[b * 3];
    const float * bb = vf + 3 * faces[b * 3 + 1];
    const float * c = vf + 3 * faces[b * 3 + 2];
    const float * p = points + i * 3;
    float w[3];
    tri_weights_vals(a[0], a[1], a[2], bb[0], bb[1], bb[2], c[0], c[1], c[2], p[0], p[1], p[2], w);
    w_out[i * 3] = w[0];
    w_out[i * 3 + 1] = w[1];
    w_out[i * 3 + 2] = w[2];
  }
}

// ---- tiled form
__global__ __launch_bounds__(256) void pd_tri_image_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                           float4 * __restrict__ img, int64_t V, int64_t F, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n * F) return;
  const int64_t f = i % F;
  const float * vf = verts + (i / F) * V * 3;
  const float * a = vf + 3 * faces[f * 3];
  const float * b = vf + 3 * faces[f * 3 + 1];
  const float * c = vf + 3 * faces[f * 3 + 2];
  const float e1 = (b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2]);
  const float e2 = (c[0] - a[0]) * (c[0] - a[0]) + (c[1] - a[1]) * (c[1] - a[1]) + (c[2] - a[2]) * (c[2] - a[2]);
  img[i * 3] = make_float4(a[0], a[1], a[2], sqrtf(fmaxf(e1, e2)));
  img[i * 3 + 1] = make_float4(b[0], b[1], b[2], 0.0f);
  img[i * 3 + 2] = make_float4(c[0], c[1], c[2], 0.0f);
}

__device__ inline uint32_t pd_spread4(uint32_t x) // 4 bits -> every third bit
{
  return (x & 1u) | ((x & 2u) << 2) | ((x & 4u) << 4) | ((x & 8u) << 6);
}

__global__ __launch_bounds__(1024) void pd_sort_kernel(const float * __restrict__ points, int32_t * __restrict__ perm, int64_t K)
{
  constexpr int CELLS = 1 << (3 * PD_MORTON_BITS);
  __shared__ int s_hist[CELLS];
  __shared__ int s_scan[1024];
  __shared__ float s_box[6][16];
  const float * pf = points + (int64_t)blockIdx.x * K * 3;
  int32_t * out = perm + (int64_t)blockIdx.x * K;
  const int t = threadIdx.x;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for(int64_t k = t; k < K; k += 1024)
  {
    const float x = pf[k * 3], y = pf[k * 3 + 1], z = pf[k * 3 + 2];
    if(!(fabsf(x) <= 3.0e38f && fabsf(y) <= 3.0e38f && fabsf(z) <= 3.0e38f)) continue; // non-finite: the last cell
    mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
  }
  for(int x = 0; x < 3; x++)
    for(int off = 32; off > 0; off >>= 1)
    {
      mn[x] = fminf(mn[x], __shfl_down(mn[x], off, 64));
      mx[x] = fmaxf(mx[x], __shfl_down(mx[x], off, 64));
    }
  if((t & 63) == 0)
    for(int x = 0; x < 3; x++)
    {
      s_box[x][t >> 6] = mn[x];
      s_box[3 + x][t >> 6] = mx[x];
    }
  for(int c = t; c < CELLS; c += 1024) s_hist[c] = 0;
  __syncthreads();
  float lo[3], scale[3];
  for(int x = 0; x < 3; x++)
  {
    float a = s_box[x][0], b = s_box[3 + x][0];
    for(int w = 1; w < 16; w++)
    {
      a = fminf(a, s_box[x][w]);
      b = fmaxf(b, s_box[3 + x][w]);
    }
    lo[x] = a;
    scale[x] = b > a ? (float)(1 << PD_MORTON_BITS) / (b - a) : 0.0f;
  }
  auto cell = [&](int64_t k) -> int {
    const float x = pf[k * 3], y = pf[k * 3 + 1], z = pf[k * 3 + 2];
    if(!(fabsf(x) <= 3.0e38f && fabsf(y) <= 3.0e38f && fabsf(z) <= 3.0e38f)) return CELLS - 1;
    const int m = (1 << PD_MORTON_BITS) - 1;
    const int ix = min(m, max(0, (int)((x - lo[0]) * scale[0])));
    const int iy = min(m, max(0, (int)((y - lo[1]) * scale[1])));
    const int iz = min(m, max(0, (int)((z - lo[2]) * scale[2])));
    return (int)(pd_spread4(ix) | (pd_spread4(iy) << 1) | (pd_spread4(iz) << 2));
  };
  for(int64_t k = t; k < K; k += 1024) atomicAdd(&s_hist[cell(k)], 1);
  __syncthreads();
  // exclusive scan: 4 cells per thread, then a scan of the 1024 partial sums
  constexpr int PER = CELLS / 1024;
  int loc = 0;
  for(int j = 0; j < PER; j++) loc += s_hist[t * PER + j];
  s_scan[t] = loc;
  __syncthreads();
  for(int d = 1; d < 1024; d <<= 1)
  {
    const int v = t >= d ? s_scan[t - d] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  int run = s_scan[t] - loc;
  for(int j = 0; j < PER; j++)
  {
    const int h = s_hist[t * PER + j];
    s_hist[t * PER + j] = run;
    run += h;
  }
  __syncthreads();
  for(int64_t k = t; k < K; k += 1024) out[atomicAdd(&s_hist[cell(k)], 1)] = (int32_t)k;
}

__global__ __launch_bounds__(PD_THREADS) void pd_tiled_kernel(const float * __restrict__ verts, const float4 * __restrict__ img,
                                                       const int32_t * __restrict__ seedv, int64_t nseed,
                                                       const float * __restrict__ points, const int32_t * __restrict__ perm,
                                                       int64_t * __restrict__ face_out, float * __restrict__ w_out,
                                                       float * __restrict__ closest_out, float * __restrict__ sq_out, int64_t V,
                                                       int64_t F, int64_t K, int64_t blocks_per_frame)
{
  __shared__ float4 s_tri[PD_TILE * 3];
  __shared__ float s_d[PD_WAVES][64];
  __shared__ int s_f[PD_WAVES][64];
  const int64_t frame = blockIdx.x / blocks_per_frame;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (blockIdx.x % blocks_per_frame) * 64 + lane;
  const bool live = q < K;
  const int64_t k = perm[frame * K + (live ? q : K - 1)]; // lanes past K repeat the last query: they cull like it
  const int64_t qi = frame * K + k;
  const float p0 = points[qi * 3], p1 = points[qi * 3 + 1], p2 = points[qi * 3 + 2];
  const float * vf = verts + frame * V * 3;
  const float4 * tf = img + frame * F * 3;

  // seed: nearest vertex that has a face
  float seed = INFINITY;
  for(int64_t base = 0; base < nseed; base += PD_VTILE)
  {
    __syncthreads();
    for(int j = threadIdx.x; j < PD_VTILE; j += PD_THREADS)
      if(base + j < nseed)
      {
        const float * v = vf + 3 * (int64_t)seedv[base + j];
        s_tri[j] = make_float4(v[0], v[1], v[2], 0.0f);
      }
    __syncthreads();
    const int cnt = (int)(nseed - base < PD_VTILE ? nseed - base : PD_VTILE);
    const int j1 = min(cnt, (wave + 1) * (PD_VTILE / PD_WAVES));
    for(int j = wave * (PD_VTILE / PD_WAVES); j < j1; j++)
    {
      const float4 v = s_tri[j];
      const float dx = p0 - v.x, dy = p1 - v.y, dz = p2 - v.z;
      seed = fminf(seed, dx * dx + dy * dy + dz * dz);
    }
  }
  s_d[wave][lane] = seed;
  __syncthreads();
  for(int w = 0; w < PD_WAVES; w++) seed = fminf(seed, s_d[w][lane]);

  // pass 1: minimum squared distance (and its face, the fallback if the band comes up empty)
  float best = INFINITY, lim = seed;
  int bf = 0;
  float sq = sqrtf(lim);
  for(int64_t fb = 0; fb < F; fb += PD_TILE)
  {
    __syncthreads();
    for(int j = threadIdx.x; j < PD_TILE * 3; j += PD_THREADS)
      if(fb * 3 + j < F * 3) s_tri[j] = tf[fb * 3 + j];
    __syncthreads();
    const int cnt = (int)(F - fb < PD_TILE ? F - fb : PD_TILE);
    const int j1 = min(cnt, (wave + 1) * 64);
    for(int j = wave * 64; j < j1; j++)
    {
      const float4 A = s_tri[j * 3];
      if(lim < INFINITY && pd_culled(A, p0, p1, p2, sq)) continue;
      const float4 B = s_tri[j * 3 + 1], C = s_tri[j * 3 + 2];
      const float d = tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2).x;
      const int f = (int)fb + j;
      if(d < best || (d == best && f < bf))
      {
        best = d;
        bf = f;
        if(d < lim)
        {
          lim = d;
          sq = sqrtf(lim);
        }
      }
    }
  }
  __syncthreads();
  s_d[wave][lane] = best;
  s_f[wave][lane] = bf;
  __syncthreads();
  float mn = s_d[0][lane];
  int amin = s_f[0][lane];
  for(int w = 1; w < PD_WAVES; w++)
    if(s_d[w][lane] < mn || (s_d[w][lane] == mn && s_f[w][lane] < amin))
    {
      mn = s_d[w][lane];
      amin = s_f[w][lane];
    }

  // pass 2: lowest face id within the tie band (ids ascend within a lane)
  const float thr = mn * (1.0f + 1e-6f) + 1e-12f;
  const float sq_thr = sqrtf(thr);
  int cf = 0x7fffffff;
  for(int64_t fb = 0; fb < F; fb += PD_TILE)
  {
    if(__syncthreads_and(cf < (int)fb + wave * 64)) break; // every lane of every wavefront holds a lower id than it would see next
    for(int j = threadIdx.x; j < PD_TILE * 3; j += PD_THREADS)
      if(fb * 3 + j < F * 3) s_tri[j] = tf[fb * 3 + j];
    __syncthreads();
    const int cnt = (int)(F - fb < PD_TILE ? F - fb : PD_TILE);
    const int j1 = min(cnt, (wave + 1) * 64);
    for(int j = wave * 64; j < j1; j++)
    {
      const int f = (int)fb + j;
      if(f >= cf) break;
      const float4 A = s_tri[j * 3];
      if(thr < INFINITY && pd_culled(A, p0, p1, p2, sq_thr)) continue;
      const float4 B = s_tri[j * 3 + 1], C = s_tri[j * 3 + 2];
      if(tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2).x <= thr) cf = f;
    }
  }
  __syncthreads();
  s_f[wave][lane] = cf;
  __syncthreads();
  if(wave != 0 || !live) return;
  int b = s_f[0][lane];
  for(int w = 1; w < PD_WAVES; w++) b = min(b, s_f[w][lane]);
  if(b < 0 || (int64_t)b >= F) b = amin; // empty band: never index out of range
  const float4 A = tf[(int64_t)b * 3], B = tf[(int64_t)b * 3 + 1], C = tf[(int64_t)b * 3 + 2];
  const float4 r = tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2);
  face_out[qi] = b;
  sq_out[qi] = r.x;
  if(closest_out)
  {
    closest_out[qi * 3] = r.y;
    closest_out[qi * 3 + 1] = r.z;
    closest_out[qi * 3 + 2] = r.w;
  }
  if(w_out)
  {
    float w[3];
    tri_weights_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2, w);
    w_out[qi * 3] = w[0];
    w_out[qi * 3 + 1] = w[1];
    w_out[qi * 3 + 2] = w[2];
  }
}

// ---- compatible, distance-capped search (smplpp_point_mesh_distance_compatible): new kernels beside the ones above, over the same
// device headers.  A face is a candidate iff its unfused normal m passes compat_normals (scan_compat.h) against the query's normal
// (NORMALS) and its distance d, from tri_sqdist_vals, has d <= max_sq.  Over the candidates: the minimum mn, then the lowest id
// with d <= mn (1 + 1e-6) + 1e-12.  There is no nearest-vertex seed (a near vertex may belong to ineligible faces only): the cull
// radius starts at max_sq.  A query without a candidate, or with a non-finite coordinate or normal, gets face -1 and +0 elsewhere.
__device__ inline void pdc_write_unmatched(int64_t i, int64_t * face_out, float * w_out, float * closest_out, float * sq_out)
{
  face_out[i] = -1;
  sq_out[i] = 0.0f;
  for(int x = 0; x < 3; x++)
  {
    if(closest_out) closest_out[i * 3 + x] = 0.0f;
    if(w_out) w_out[i * 3 + x] = 0.0f;
  }
}

// per-query form: one 256-thread workgroup per query, closest_point_block's two passes restricted to the candidates
template<bool NORMALS>
__global__ __launch_bounds__(256) void pdc_query_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                        const float * __restrict__ points, const float * __restrict__ pnormals, float c2,
                                                        float max_sq, int64_t * __restrict__ face_out, float * __restrict__ w_out,
                                                        float * __restrict__ closest_out, float * __restrict__ sq_out, int64_t V, int64_t F,
                                                        int64_t K)
{
  __shared__ float s_d[4], s_min;
  __shared__ int s_f[4], s_argmin;
  __shared__ int64_t s_face;
  __shared__ float s_c[3], s_sq;
  const int64_t i = blockIdx.x;
  const float * vf = verts + (i / K) * V * 3;
  const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  bool ok = compat_finite3(p[0], p[1], p[2]); // (the same on every thread)
  if constexpr(NORMALS)
  {
    q.x = pnormals[i * 3];
    q.y = pnormals[i * 3 + 1];
    q.z = pnormals[i * 3 + 2];
    q.w = compat_dot(q.x, q.y, q.z, q.x, q.y, q.z);
    ok = ok && compat_finite3(q.x, q.y, q.z);
  }
  if(!ok)
  {
    if(threadIdx.x == 0) pdc_write_unmatched(i, face_out, w_out, closest_out, sq_out);
    return;
  }
  const int wave = threadIdx.x >> 6;
  // pass 1: the minimum over the candidates
  float best = INFINITY, lim = max_sq;
  int bf = 0x7fffffff;
  float sq = sqrtf(lim);
  for(int64_t base = threadIdx.x; base < F; base += 256 * CP_BATCH)
  {
    TriBatch t;
    load_tri_batch(vf, faces, F, base, 256, t);
#pragma unroll
    for(int b = 0; b < CP_BATCH; b++)
    {
      if(!t.valid[b]) continue;
      const float * a = t.v[b];
      if constexpr(NORMALS)
        if(!compat_normals(compat_face_normal(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]), q, c2)) continue;
      if(lim < INFINITY && tri_culled_v(a, a + 3, a + 6, p, sq)) continue;
      const float d = tri_sqdist_vals(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], p[0], p[1], p[2]).x;
      if(!(d <= max_sq)) continue;
      const int f = (int)(base + (int64_t)b * 256);
      if(d < best || (d == best && f < bf))
      {
        best = d;
        bf = f;
        if(d < lim)
        {
          lim = d;
          sq = sqrtf(lim);
        }
      }
    }
  }
  for(int off = 32; off > 0; off >>= 1)
  {
    const float od = __shfl_down(best, off, 64);
    const int of = __shfl_down(bf, off, 64);
    if(od < best || (od == best && of < bf))
    {
      best = od;
      bf = of;
    }
  }
  if((threadIdx.x & 63) == 0)
  {
    s_d[wave] = best;
    s_f[wave] = bf;
  }
  __syncthreads();
  if(threadIdx.x == 0)
  {
    int w = 0;
    for(int j = 1; j < 4; j++)
      if(s_d[j] < s_d[w] || (s_d[j] == s_d[w] && s_f[j] < s_f[w])) w = j;
    s_min = s_d[w];
    s_argmin = s_f[w];
  }
  __syncthreads();
  const int amin = s_argmin;
  if(amin == 0x7fffffff) // no candidate
  {
    if(threadIdx.x == 0) pdc_write_unmatched(i, face_out, w_out, closest_out, sq_out);
    return;
  }
  // pass 2: the lowest candidate id within the tie band
  const float thr = s_min * (1.0f + 1e-6f) + 1e-12f;
  const float sq_thr = sqrtf(thr);
  int cf = 0x7fffffff;
  for(int64_t base = threadIdx.x; base < F && (int)base < cf; base += 256 * CP_BATCH)
  {
    TriBatch t;
    load_tri_batch(vf, faces, F, base, 256, t);
#pragma unroll
    for(int b = 0; b < CP_BATCH; b++)
    {
      const int f = (int)(base + (int64_t)b * 256);
      if(!t.valid[b] || f >= cf) continue; // ids ascend within a thread
      const float * a = t.v[b];
      if constexpr(NORMALS)
        if(!compat_normals(compat_face_normal(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]), q, c2)) continue;
      if(thr < INFINITY && tri_culled_v(a, a + 3, a + 6, p, sq_thr)) continue;
      const float d = tri_sqdist_vals(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], p[0], p[1], p[2]).x;
      if(d <= thr && d <= max_sq) cf = f;
    }
  }
  for(int off = 32; off > 0; off >>= 1)
  {
    const int of = __shfl_down(cf, off, 64);
    cf = of < cf ? of : cf;
  }
  __syncthreads(); // s_f is reused
  if((threadIdx.x & 63) == 0) s_f[wave] = cf;
  __syncthreads();
  // (from here on written as closest_point_block ends and pd_query_kernel writes: the weights' evaluation is inlined, and how
  // the compiler fuses its products follows the code around it)
  if(threadIdx.x == 0)
  {
    int b = s_f[0];
    for(int j = 1; j < 4; j++) b = s_f[j] < b ? s_f[j] : b;
    if(b < 0 || (int64_t)b >= F) b = amin; // empty band: never index out of range
    float c[3];
    const float d = tri_sqdist_dev(vf, faces, b, p, c);
    s_face = b;
    s_c[0] = c[0]; s_c[1] = c[1]; s_c[2] = c[2];
    s_sq = d;
  }
  __syncthreads();
  if(threadIdx.x != 0) return;
  const int64_t b = s_face;
  face_out[i] = b;
  sq_out[i] = s_sq;
  if(closest_out)
  {
    closest_out[i * 3] = s_c[0];
    closest_out[i * 3 + 1] = s_c[1];
    closest_out[i * 3 + 2] = s_c[2];
  }
  if(w_out)
  {
    const float * a = vf + 3 * faces[b * 3];
    const float * bb = vf + 3 * faces[b * 3 + 1];
    const float * c = vf + 3 * faces[b * 3 + 2];
    const float * p = points + i * 3;
    float w[3];
    tri_weights_vals(a[0], a[1], a[2], bb[0], bb[1], bb[2], c[0], c[1], c[2], p[0], p[1], p[2], w);
    w_out[i * 3] = w[0];
    w_out[i * 3 + 1] = w[1];
    w_out[i * 3 + 2] = w[2];
  }
}

// tiled form: pd_tri_image_kernel's image with, under NORMALS, a fourth float4 per face: (m.x, m.y, m.z, mm)
template<bool NORMALS>
__global__ __launch_bounds__(256) void pdc_tri_image_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                            float4 * __restrict__ img, int64_t V, int64_t F, int64_t n)
{
  constexpr int S = NORMALS ? 4 : 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n * F) return;
  const int64_t f = i % F;
  const float * vf = verts + (i / F) * V * 3;
  const float * a = vf + 3 * faces[f * 3];
  const float * b = vf + 3 * faces[f * 3 + 1];
  const float * c = vf + 3 * faces[f * 3 + 2];
  const float e1 = (b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2]);
  const float e2 = (c[0] - a[0]) * (c[0] - a[0]) + (c[1] - a[1]) * (c[1] - a[1]) + (c[2] - a[2]) * (c[2] - a[2]);
  img[i * S] = make_float4(a[0], a[1], a[2], sqrtf(fmaxf(e1, e2)));
  img[i * S + 1] = make_float4(b[0], b[1], b[2], 0.0f);
  img[i * S + 2] = make_float4(c[0], c[1], c[2], 0.0f);
  if constexpr(NORMALS) img[i * S + 3] = compat_face_normal(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
}

// pd_tiled_kernel without the seed: 64 queries per workgroup, its 16 wavefronts split every tile of faces (1024 faces of three
// float4, or 768 of four under NORMALS: the same 48 KiB).  The compatibility test reads the face's fourth float4 alone and comes
// first; pass 1 culls against min(max_sq, running minimum over candidates), pass 2 against the band.
template<bool NORMALS>
__global__ __launch_bounds__(PD_THREADS) void pdc_tiled_kernel(const float4 * __restrict__ img, const float * __restrict__ points,
                                                               const float * __restrict__ pnormals, float c2, float max_sq,
                                                               const int32_t * __restrict__ perm, int64_t * __restrict__ face_out,
                                                               float * __restrict__ w_out, float * __restrict__ closest_out,
                                                               float * __restrict__ sq_out, int64_t F, int64_t K, int64_t blocks_per_frame)
{
  constexpr int S = NORMALS ? 4 : 3;
  constexpr int TILE = PD_TILE * 3 / S, CH = TILE / PD_WAVES; // faces per tile, and per wavefront of a tile
  __shared__ float4 s_tri[TILE * S];
  __shared__ float s_d[PD_WAVES][64];
  __shared__ int s_f[PD_WAVES][64];
  const int64_t frame = blockIdx.x / blocks_per_frame;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qn = (blockIdx.x % blocks_per_frame) * 64 + lane;
  const bool live = qn < K;
  const int64_t k = perm[frame * K + (live ? qn : K - 1)]; // lanes past K repeat the last query: they cull like it
  const int64_t qi = frame * K + k;
  const float p0 = points[qi * 3], p1 = points[qi * 3 + 1], p2 = points[qi * 3 + 2];
  float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  bool ok = compat_finite3(p0, p1, p2);
  if constexpr(NORMALS)
  {
    q.x = pnormals[qi * 3];
    q.y = pnormals[qi * 3 + 1];
    q.z = pnormals[qi * 3 + 2];
    q.w = compat_dot(q.x, q.y, q.z, q.x, q.y, q.z);
    ok = ok && compat_finite3(q.x, q.y, q.z);
  }
  const float4 * tf = img + frame * F * S;

  // pass 1: the minimum over the candidates
  float best = INFINITY, lim = max_sq;
  int bf = 0x7fffffff;
  float sq = sqrtf(lim);
  for(int64_t fb = 0; fb < F; fb += TILE)
  {
    __syncthreads();
    for(int j = threadIdx.x; j < TILE * S; j += PD_THREADS)
      if(fb * S + j < F * S) s_tri[j] = tf[fb * S + j];
    __syncthreads();
    const int cnt = (int)(F - fb < TILE ? F - fb : TILE);
    const int j1 = ok ? min(cnt, (wave + 1) * CH) : 0; // (a query that cannot match scans nothing)
    for(int j = wave * CH; j < j1; j++)
    {
      if constexpr(NORMALS)
        if(!compat_normals(s_tri[j * S + 3], q, c2)) continue;
      const float4 A = s_tri[j * S];
      if(lim < INFINITY && pd_culled(A, p0, p1, p2, sq)) continue;
      const float4 B = s_tri[j * S + 1], C = s_tri[j * S + 2];
      const float d = tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2).x;
      if(!(d <= max_sq)) continue;
      const int f = (int)fb + j;
      if(d < best || (d == best && f < bf))
      {
        best = d;
        bf = f;
        if(d < lim)
        {
          lim = d;
          sq = sqrtf(lim);
        }
      }
    }
  }
  __syncthreads();
  s_d[wave][lane] = best;
  s_f[wave][lane] = bf;
  __syncthreads();
  float mn = s_d[0][lane];
  int amin = s_f[0][lane];
  for(int w = 1; w < PD_WAVES; w++)
    if(s_d[w][lane] < mn || (s_d[w][lane] == mn && s_f[w][lane] < amin))
    {
      mn = s_d[w][lane];
      amin = s_f[w][lane];
    }
  const bool none = amin == 0x7fffffff; // no candidate (the same in every wavefront's copy of the lane)

  // pass 2: the lowest candidate id within the tie band (ids ascend within a lane)
  const float thr = mn * (1.0f + 1e-6f) + 1e-12f;
  const float sq_thr = sqrtf(thr);
  int cf = 0x7fffffff;
  for(int64_t fb = 0; fb < F; fb += TILE)
  {
    if(__syncthreads_and(none || cf < (int)fb + wave * CH)) break; // every lane is done, or holds a lower id than it would see next
    for(int j = threadIdx.x; j < TILE * S; j += PD_THREADS)
      if(fb * S + j < F * S) s_tri[j] = tf[fb * S + j];
    __syncthreads();
    const int cnt = (int)(F - fb < TILE ? F - fb : TILE);
    const int j1 = none ? 0 : min(cnt, (wave + 1) * CH);
    for(int j = wave * CH; j < j1; j++)
    {
      const int f = (int)fb + j;
      if(f >= cf) break;
      if constexpr(NORMALS)
        if(!compat_normals(s_tri[j * S + 3], q, c2)) continue;
      const float4 A = s_tri[j * S];
      if(thr < INFINITY && pd_culled(A, p0, p1, p2, sq_thr)) continue;
      const float4 B = s_tri[j * S + 1], C = s_tri[j * S + 2];
      const float d = tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2).x;
      if(d <= thr && d <= max_sq) cf = f;
    }
  }
  __syncthreads();
  s_f[wave][lane] = cf;
  __syncthreads();
  if(wave != 0 || !live) return;
  if(none)
  {
    pdc_write_unmatched(qi, face_out, w_out, closest_out, sq_out);
    return;
  }
  int b = s_f[0][lane];
  for(int w = 1; w < PD_WAVES; w++) b = min(b, s_f[w][lane]);
  if(b < 0 || (int64_t)b >= F) b = amin; // empty band: never index out of range
  // (written as pd_tiled_kernel writes: the weights' evaluation is inlined, and its rounding follows the code around it)
  const float4 A = tf[(int64_t)b * S], B = tf[(int64_t)b * S + 1], C = tf[(int64_t)b * S + 2];
  const float4 r = tri_sqdist_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2);
  face_out[qi] = b;
  sq_out[qi] = r.x;
  if(closest_out)
  {
    closest_out[qi * 3] = r.y;
    closest_out[qi * 3 + 1] = r.z;
    closest_out[qi * 3 + 2] = r.w;
  }
  if(w_out)
  {
    float w[3];
    tri_weights_vals(A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z, p0, p1, p2, w);
    w_out[qi * 3] = w[0];
    w_out[qi * 3 + 1] = w[1];
    w_out[qi * 3 + 2] = w[2];
  }
}

// ---- backward
__global__ __launch_bounds__(256) void pd_vjp_record_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                            const float * __restrict__ points, const int64_t * __restrict__ face,
                                                            const float * __restrict__ gsq, PdRecord * __restrict__ rec,
                                                            float * __restrict__ gp, int accumulate, int64_t V, int64_t F, int64_t K,
                                                            int64_t nk)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nk) return;
  const float g = gsq[i];
  const int64_t f = face[i];
  PdRecord r;
  r.u[0] = r.u[1] = r.u[2] = -1;
  r.u[3] = 0;
  float gpt[3] = {0.0f, 0.0f, 0.0f};
  for(int j = 0; j < 3; j++) r.g[j][0] = r.g[j][1] = r.g[j][2] = 0.0f;
  r.pad[0] = r.pad[1] = r.pad[2] = 0.0f;
  if(g != 0.0f && f >= 0 && f < F)
  {
    const float * vf = verts + (i / K) * V * 3;
    const int u0 = faces[f * 3], u1 = faces[f * 3 + 1], u2 = faces[f * 3 + 2];
    const float * a = vf + 3 * u0;
    const float * b = vf + 3 * u1;
    const float * c = vf + 3 * u2;
    const float p0 = points[i * 3], p1 = points[i * 3 + 1], p2 = points[i * 3 + 2];
    const float4 t = tri_sqdist_vals(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], p0, p1, p2);
    float w[3];
    tri_weights_vals(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], p0, p1, p2, w);
    const float rr[3] = {p0 - t.y, p1 - t.z, p2 - t.w};
    const float s = 2.0f * g, sn = -2.0f * g;
    r.u[0] = u0;
    r.u[1] = u1;
    r.u[2] = u2;
    for(int x = 0; x < 3; x++) gpt[x] = s * rr[x];
    for(int j = 0; j < 3; j++)
    {
      const float sw = sn * w[j];
      for(int x = 0; x < 3; x++) r.g[j][x] = sw * rr[x];
    }
  }
  if(rec) rec[i] = r;
  if(gp)
    for(int x = 0; x < 3; x++) gp[i * 3 + x] = accumulate ? gp[i * 3 + x] + gpt[x] : gpt[x];
}

static PointDistState * pd_state(smplpp_model * m)
{
  if(!m->pd) m->pd.reset(new PointDistState());
  return m->pd.get();
}

static int pd_seed_setup(smplpp_model * m, PointDistState * s)
{
  if(s->nseed >= 0) return SMPLPP_OK;
  std::vector<int32_t> ids;
  for(int64_t v = 0; v < m->V; v++)
    if(m->h_adjOff[v + 1] > m->h_adjOff[v]) ids.push_back((int32_t)v);
  HIP_TRY(s->seedv.reserve(sizeof(int32_t) * (ids.size() + 1)));
  if(!ids.empty()) HIP_TRY(hipMemcpy(s->seedv.as<int32_t>(), ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice));
  s->nseed = (int64_t)ids.size();
  return SMPLPP_OK;
}

// all pointers on the device
int pd_forward_device(smplpp_model * m, PointDistState * s, int64_t n, const float * verts, int64_t K, const float * points,
                      int64_t * face, float * weights, float * closest, float * sqdist, hipStream_t st)
{
  const bool tiled = m->pd_form == 't' || (m->pd_form != 'q' && n * K >= PD_TILED_MIN_NK);
  const int64_t V = m->V, F = m->F;
  if(!tiled)
  {
    pd_query_kernel<<<dim3((unsigned)(n * K)), dim3(256), 0, st>>>(verts, m->faces.get(), points, face, weights, closest, sqdist, V, F, K);
    HIP_TRY(hipGetLastError());
    return SMPLPP_OK;
  }
  int rc = pd_seed_setup(m, s);
  if(rc) return rc;
  HIP_TRY(s->tri.reserve(sizeof(float4) * (size_t)n * F * 3));
  HIP_TRY(s->perm.reserve(sizeof(int32_t) * (size_t)n * K));
  pd_tri_image_kernel<<<dim3((unsigned)((n * F + 255) / 256)), dim3(256), 0, st>>>(verts, m->faces.get(), s->tri.as<float4>(), V, F, n);
  HIP_TRY(hipGetLastError());
  pd_sort_kernel<<<dim3((unsigned)n), dim3(1024), 0, st>>>(points, s->perm.as<int32_t>(), K);
  HIP_TRY(hipGetLastError());
  const int64_t bpf = (K + 63) / 64;
  pd_tiled_kernel<<<dim3((unsigned)(n * bpf)), dim3(PD_THREADS), 0, st>>>(verts, s->tri.as<float4>(), s->seedv.as<int32_t>(), s->nseed, points,
                                                                   s->perm.as<int32_t>(), face, weights, closest, sqdist, V, F, K, bpf);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// smplpp_point_mesh_distance_compatible, all pointers on the device (pnormals may be null); the forms are chosen as above
template<bool NORMALS>
static int pdc_forward_device(smplpp_model * m, PointDistState * s, int64_t n, const float * verts, int64_t K, const float * points,
                              const float * pnormals, float c2, float max_sq, int64_t * face, float * weights, float * closest,
                              float * sqdist, hipStream_t st)
{
  constexpr int S = NORMALS ? 4 : 3;
  const bool tiled = m->pd_form == 't' || (m->pd_form != 'q' && n * K >= PD_TILED_MIN_NK);
  const int64_t V = m->V, F = m->F;
  if(!tiled)
  {
    pdc_query_kernel<NORMALS><<<dim3((unsigned)(n * K)), dim3(256), 0, st>>>(verts, m->faces.get(), points, pnormals, c2, max_sq, face, weights,
                                                                             closest, sqdist, V, F, K);
    HIP_TRY(hipGetLastError());
    return SMPLPP_OK;
  }
  HIP_TRY(s->tri.reserve(sizeof(float4) * (size_t)n * F * S));
  HIP_TRY(s->perm.reserve(sizeof(int32_t) * (size_t)n * K));
  pdc_tri_image_kernel<NORMALS><<<dim3((unsigned)((n * F + 255) / 256)), dim3(256), 0, st>>>(verts, m->faces.get(), s->tri.as<float4>(), V, F, n);
  HIP_TRY(hipGetLastError());
  pd_sort_kernel<<<dim3((unsigned)n), dim3(1024), 0, st>>>(points, s->perm.as<int32_t>(), K);
  HIP_TRY(hipGetLastError());
  const int64_t bpf = (K + 63) / 64;
  pdc_tiled_kernel<NORMALS><<<dim3((unsigned)(n * bpf)), dim3(PD_THREADS), 0, st>>>(s->tri.as<float4>(), points, pnormals, c2, max_sq,
                                                                                    s->perm.as<int32_t>(), face, weights, closest, sqdist, F,
                                                                                    K, bpf);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

int pd_vjp_device(smplpp_model * m, PointDistState * s, int64_t n, const float * verts, int64_t K, const float * points,
                  const int64_t * face, const float * gsq, float * gv, float * gp, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, nk = n * K;
  PdRecord * rec = nullptr;
  if(gv)
  {
    HIP_TRY(s->rec.reserve(sizeof(PdRecord) * (size_t)nk));
    rec = s->rec.as<PdRecord>();
  }
  pd_vjp_record_kernel<<<dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st>>>(verts, m->faces.get(), points, face, gsq, rec, gp, accumulate, V,
                                                                                 m->F, K, nk);
  HIP_TRY(hipGetLastError());
  return gv ? record_gather(rec, gv, accumulate, n, K, V, st) : SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

static int pd_check(const char * fn, smplpp_model * m, int64_t n, int64_t K, int space)
{
  const std::string name(fn);
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, name + ": model has no faces");
  // every [n,K] index and every grid below stays in int32 (the tiled form's grid is n * ceil(K / 64), the gather's n * ceil(V / 256))
  if(n > 0x7fffffffLL || K > 0x7fffffffLL || n * K > 0x7fffffffLL || n * ((m->V + GATHER_T - 1) / GATHER_T) > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, name + ": n * K beyond int32 indexing");
  return check_space(space, fn);
}

extern "C" int smplpp_point_mesh_distance(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points, int64_t * face,
                                          float * weights, float * closest, float * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_distance";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !face || !sqdist) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = pd_check(fn, m, n, K, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "point-mesh distance");
  PointDistState * s = pd_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  int64_t * fo = fr.out(face, (size_t)n * K);
  float * wo = fr.out(weights, (size_t)n * K * 3);
  float * co = fr.out(closest, (size_t)n * K * 3);
  float * so = fr.out(sqdist, (size_t)n * K);
  return fr.run([&] { return pd_forward_device(m, s, n, v, K, p, fo, wo, co, so, fr.st); });
}

extern "C" int smplpp_point_mesh_distance_compatible(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                                     const float * point_normals, float cos_min, float max_sqdist, int64_t * face,
                                                     float * weights, float * closest, float * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_distance_compatible";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !face || !sqdist) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = compat_args(fn, cos_min, max_sqdist);
  if(rc) return rc;
  if((rc = pd_check(fn, m, n, K, space))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "point-mesh distance (compatible)");
  PointDistState * s = pd_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  const float * pn = fr.in(point_normals, (size_t)n * K * 3);
  int64_t * fo = fr.out(face, (size_t)n * K);
  float * wo = fr.out(weights, (size_t)n * K * 3);
  float * co = fr.out(closest, (size_t)n * K * 3);
  float * so = fr.out(sqdist, (size_t)n * K);
  const float c2 = cos_min * cos_min;
  return fr.run([&] {
    return point_normals ? pdc_forward_device<true>(m, s, n, v, K, p, pn, c2, max_sqdist, fo, wo, co, so, fr.st)
                         : pdc_forward_device<false>(m, s, n, v, K, p, nullptr, c2, max_sqdist, fo, wo, co, so, fr.st);
  });
}

extern "C" int smplpp_point_mesh_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                              const int64_t * face, const float * grad_sqdist, float * grad_verts, float * grad_points,
                                              int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_distance_vjp";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !face || !grad_sqdist || (!grad_verts && !grad_points))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = pd_check(fn, m, n, K, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * K, 0, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "point-mesh distance VJP");
  return distance_vjp(fr, pd_vjp_device, m, pd_state(m), n, verts, K, points, face, n * K, grad_sqdist, grad_verts, grad_points, accumulate);
}
