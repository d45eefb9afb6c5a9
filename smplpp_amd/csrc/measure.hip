// Body measurements: surface area and enclosed volume of regions of the posed mesh, the length of a region's section
// by a plane (a girth), and their vector-Jacobian product to the vertices and to the planes.  The rules are in include/smplpp_hip.h;
// every fp32 operation below is rounded on its own (no contraction to FMA), every output element is one fixed-order sum, and there
// are no floating-point atomics.
//
//  ms_forward_kernel<NQ>    a workgroup per (frame, region) of the regions whose list length frame_sum_split gives the form NQ: it
//                           walks the list once for area, volume and MS_SEC of the region's sections (again for every MS_SEC more),
//                           slot k in partial k mod 1024, and the partials meet by sum1024 (fixed_sum.h).
//  ms_vjp_verts_kernel      per (frame, vertex): the vertex's faces from the adjacency table, each face's regions from the transposed
//                           lists (measure_tables.h), each region's area, volume and section terms, summed in that order.
//  ms_vjp_planes_kernel     a workgroup per (frame, section): the four entries of the plane's gradient, each a sum1024 over the list.
//  ms_frames_kernel         planes shared by the frames: the frames' terms in the two-level tile order of smplpp_vertex_offsets_vjp.
#include "fixed_sum.h"
#include "measure_tables.h"
#include "staging.h"

#pragma clang fp contract(off)

struct smplpp_measure
{
  int device = 0;
  int64_t V = 0, F = 0, R = 0, S = 0, nnz = 0;
  smplpp_hip::DevBuf faces, adjOff, adjFace;           // the model's faces [F][3] and adjacency, copied: the handle may outlive the model
  smplpp_hip::DevBuf regionPtr, regionFace;            // measure_tables.h
  smplpp_hip::DevBuf facePtr, faceRegion;              // (the slots of the pairs stay on the host: no kernel asks where a face sits)
  smplpp_hip::DevBuf secPtr, secId, secRegion;
  smplpp_hip::DevBuf formRegion;                       // [R] the regions grouped by the form of their sum: nq = 0, then 4, then 1
  int64_t formOff[4] = {0, 0, 0, 0};
  smplpp_hip::DevBuf terms;                            // [n][S][4] the frames' terms of a shared plane's gradient in flight
  smplpp_hip::Arena arena;                             // staging of the host-space calls on this handle
};

namespace smplpp_hip
{
using Measure = struct ::smplpp_measure; // (the bare name is the measuring call)
constexpr int MS_T = 256;                // threads of the two backward kernels and of the frames kernel
constexpr int MS_SEC = 4;                // sections a pass of the forward kernel carries beside area and volume
constexpr int MS_FT = SMPLPP_VERTEX_OFFSETS_TILE;

__device__ inline bool ms_finite(float x)
{
  return fabsf(x) <= 3.402823466e+38f; // (false for NaN)
}
// entry i of a three-entry register array without indexing it by a variable
__device__ inline float ms_pick(float a0, float a1, float a2, int i)
{
  return i == 0 ? a0 : (i == 1 ? a1 : a2);
}

// A face of one frame: the raw corners v (the sections read them) and p = v - center (area and volume)
struct MsFace
{
  float v[3][3], p[3][3];
};
// false for a face with a corner that is not finite
__device__ inline bool ms_load_face(const float * __restrict__ X, const int32_t * __restrict__ ids, const float (&c)[3], MsFace & f)
{
  bool live = true;
#pragma unroll
  for(int i = 0; i < 3; i++)
#pragma unroll
    for(int x = 0; x < 3; x++)
    {
      const float a = X[(int64_t)ids[i] * 3 + x];
      live = live && ms_finite(a);
      f.v[i][x] = a;
      f.p[i][x] = a - c[x];
    }
  return live;
}

__device__ inline void ms_cross(const float (&a)[3], const float (&b)[3], float (&o)[3])
{
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// area_f, with cr = (p1 - p0) x (p2 - p0) and |cr| for the backward
struct MsArea
{
  float a[3], b[3], cr[3], nrm;
};
__device__ inline float ms_area(const MsFace & f, MsArea & o)
{
#pragma unroll
  for(int x = 0; x < 3; x++) o.a[x] = f.p[1][x] - f.p[0][x], o.b[x] = f.p[2][x] - f.p[0][x];
  ms_cross(o.a, o.b, o.cr);
  o.nrm = sqrtf((o.cr[0] * o.cr[0] + o.cr[1] * o.cr[1]) + o.cr[2] * o.cr[2]);
  return 0.5f * o.nrm;
}
__device__ inline float ms_volume(const MsFace & f)
{
  float w[3];
  ms_cross(f.p[1], f.p[2], w);
  return ((f.p[0][0] * w[0] + f.p[0][1] * w[1]) + f.p[0][2] * w[2]) / 6.0f;
}
// g d area_f / d corner c; false where |cr| = 0
__device__ inline bool ms_area_grad(const MsFace & f, float g, int c, float (&G)[3])
{
  MsArea A;
  ms_area(f, A);
  if(A.nrm == 0.0f) return false;
  const float k = (g * 0.5f) / A.nrm;
  float gc[3], ga[3], gb[3];
#pragma unroll
  for(int x = 0; x < 3; x++) gc[x] = k * A.cr[x];
  ms_cross(A.b, gc, ga);
  ms_cross(gc, A.a, gb);
#pragma unroll
  for(int x = 0; x < 3; x++) G[x] = ms_pick(-(ga[x] + gb[x]), ga[x], gb[x], c);
  return true;
}
// g d vol_f / d corner c
__device__ inline void ms_volume_grad(const MsFace & f, float g, int c, float (&G)[3])
{
  const float k = g / 6.0f;
  float w0[3], w1[3], w2[3];
  ms_cross(f.p[1], f.p[2], w0);
  ms_cross(f.p[2], f.p[0], w1);
  ms_cross(f.p[0], f.p[1], w2);
#pragma unroll
  for(int x = 0; x < 3; x++) G[x] = k * ms_pick(w0[x], w1[x], w2[x], c);
}

// A plane (nx, ny, nz, d) as given; dead with an entry that is not finite or a zero normal (and where there is none)
struct MsPlane
{
  float n[3], d;
  bool live;
};
__device__ inline MsPlane ms_plane(const float * __restrict__ p)
{
  MsPlane o;
  o.live = p != nullptr;
#pragma unroll
  for(int x = 0; x < 3; x++) o.n[x] = p ? p[x] : 0.0f;
  o.d = p ? p[3] : 0.0f;
  o.live = o.live && ms_finite(o.n[0]) && ms_finite(o.n[1]) && ms_finite(o.n[2]) && ms_finite(o.d) &&
           !(o.n[0] == 0.0f && o.n[1] == 0.0f && o.n[2] == 0.0f);
  return o;
}

// The segment a plane cuts from a face.  The corners are taken in the order L, M, N (x[0], x[1], x[2]): L alone on its side, then the
// cyclic order.  Edge j = 1, 2 joins L to x[j]; a is its end below the plane, b the end above.
struct MsEdge
{
  float a[3], b[3], ba[3], sa, sb, den, t, q[3];
};
struct MsSeg
{
  int L;       // the face's corner that is x[0]
  bool Labove; // L is the above end of both edges
  MsEdge e[3]; // (e[0] unused)
  float d[3], len; // q2 - q1 and its length
};
__device__ inline bool ms_segment(const MsFace & f, const MsPlane & pl, MsSeg & o)
{
  float s[3];
  int above = 0;
#pragma unroll
  for(int i = 0; i < 3; i++)
  {
    s[i] = ((pl.n[0] * f.v[i][0] + pl.n[1] * f.v[i][1]) + pl.n[2] * f.v[i][2]) - pl.d;
    above += s[i] >= 0.0f ? 1 : 0;
  }
  if(above == 0 || above == 3) return false;
  o.Labove = above == 1;
  o.L = ((s[0] >= 0.0f) == o.Labove) ? 0 : (((s[1] >= 0.0f) == o.Labove) ? 1 : 2);
  float x[3][3], sx[3];
#pragma unroll
  for(int j = 0; j < 3; j++)
  {
    const int i = (o.L + j) % 3;
    sx[j] = ms_pick(s[0], s[1], s[2], i);
#pragma unroll
    for(int k = 0; k < 3; k++) x[j][k] = ms_pick(f.v[0][k], f.v[1][k], f.v[2][k], i);
  }
#pragma unroll
  for(int j = 1; j < 3; j++)
  {
    MsEdge & e = o.e[j];
    e.sa = o.Labove ? sx[j] : sx[0];
    e.sb = o.Labove ? sx[0] : sx[j];
    e.den = e.sa - e.sb;
    e.t = e.sa / e.den;
#pragma unroll
    for(int k = 0; k < 3; k++)
    {
      e.a[k] = o.Labove ? x[j][k] : x[0][k];
      e.b[k] = o.Labove ? x[0][k] : x[j][k];
      e.ba[k] = e.b[k] - e.a[k];
      e.q[k] = e.a[k] + e.t * e.ba[k];
    }
  }
#pragma unroll
  for(int k = 0; k < 3; k++) o.d[k] = o.e[2].q[k] - o.e[1].q[k];
  o.len = sqrtf((o.d[0] * o.d[0] + o.d[1] * o.d[1]) + o.d[2] * o.d[2]);
  return true;
}
// g d len: to the corners L, M, N (GL, GM, GN) and to the plane's four entries (P); len != 0
__device__ inline void ms_segment_grad(const MsSeg & sg, const MsPlane & pl, float g, float (&GL)[3], float (&GM)[3], float (&GN)[3],
                                       float (&P)[4])
{
  float gu[3];
#pragma unroll
  for(int k = 0; k < 3; k++) gu[k] = g * (sg.d[k] / sg.len);
  float cl[3][3], co[3][3], pn[3][4]; // per edge: to L, to the other end, to the plane
#pragma unroll
  for(int j = 1; j < 3; j++)
  {
    const MsEdge & e = sg.e[j];
    float gq[3];
#pragma unroll
    for(int k = 0; k < 3; k++) gq[k] = j == 1 ? -gu[k] : gu[k];
    const float gt = (gq[0] * e.ba[0] + gq[1] * e.ba[1]) + gq[2] * e.ba[2];
    const float r = gt / e.den;
    const float gsa = -(r * (e.sb / e.den)), gsb = r * e.t, omt = 1.0f - e.t;
#pragma unroll
    for(int k = 0; k < 3; k++)
    {
      const float ca = omt * gq[k] + gsa * pl.n[k], cb = e.t * gq[k] + gsb * pl.n[k];
      cl[j][k] = sg.Labove ? cb : ca;
      co[j][k] = sg.Labove ? ca : cb;
      pn[j][k] = gsa * e.a[k] + gsb * e.b[k];
    }
    pn[j][3] = (-gsa) - gsb;
  }
#pragma unroll
  for(int k = 0; k < 3; k++) GL[k] = cl[1][k] + cl[2][k], GM[k] = co[1][k], GN[k] = co[2][k];
#pragma unroll
  for(int k = 0; k < 4; k++) P[k] = pn[1][k] + pn[2][k];
}

// grid: n * nform workgroups; formRegion: the nform regions of this form.  pstride: S (planes per frame) or 0 (shared)
template<int NQ>
__global__ __launch_bounds__(NQ == 0 ? 64 : 1024 / NQ) void ms_forward_kernel(
    const int32_t * __restrict__ faces, const int32_t * __restrict__ regionPtr, const int32_t * __restrict__ regionFace,
    const int32_t * __restrict__ secPtr, const int32_t * __restrict__ secId, const int32_t * __restrict__ formRegion, int nform,
    const float * __restrict__ verts, const float * __restrict__ center, const float * __restrict__ planes, int pstride,
    float * __restrict__ area, float * __restrict__ volume, float * __restrict__ section, int32_t * __restrict__ crossings, int V, int R, int S)
{
  constexpr int T = NQ == 0 ? 64 : 1024 / NQ, Q = NQ == 0 ? 1 : NQ, WAVES = T / 64;
  __shared__ float cross[2 + MS_SEC][WAVES];
  __shared__ int crossN[MS_SEC][WAVES];
  const int frame = blockIdx.x / nform, r = formRegion[blockIdx.x % nform], tid = threadIdx.x;
  const float * X = verts + (int64_t)frame * V * 3;
  float c[3] = {0.0f, 0.0f, 0.0f};
  if(center)
    for(int x = 0; x < 3; x++) c[x] = center[(int64_t)frame * 3 + x];
  const int k0 = regionPtr[r], K = regionPtr[r + 1] - k0, s0 = secPtr[r];
  const int ns = (section || crossings) ? secPtr[r + 1] - s0 : 0;
  const bool whole = area || volume;
  for(int pass = 0; pass == 0 || pass * MS_SEC < ns; pass++)
  {
    float acc[2 + MS_SEC][Q];
    int cnt[MS_SEC];
    MsPlane pl[MS_SEC];
#pragma unroll
    for(int j = 0; j < 2 + MS_SEC; j++)
#pragma unroll
      for(int q = 0; q < Q; q++) acc[j][q] = 0.0f;
#pragma unroll
    for(int j = 0; j < MS_SEC; j++)
    {
      const int si = pass * MS_SEC + j;
      cnt[j] = 0;
      pl[j] = ms_plane(si < ns ? planes + ((int64_t)frame * pstride + secId[s0 + si]) * 4 : nullptr);
    }
    for(int kb = 0; kb < K; kb += 1024)
#pragma unroll
      for(int q = 0; q < Q; q++)
      {
        const int k = kb + q * T + tid; // partial k mod 1024 = q T + tid
        if(k >= K) continue;
        MsFace f;
        if(!ms_load_face(X, faces + (int64_t)regionFace[k0 + k] * 3, c, f)) continue;
        if(pass == 0 && whole)
        {
          MsArea A;
          acc[0][q] = acc[0][q] + ms_area(f, A);
          acc[1][q] = acc[1][q] + ms_volume(f);
        }
#pragma unroll
        for(int j = 0; j < MS_SEC; j++)
          if(pl[j].live)
          {
            MsSeg sg;
            if(ms_segment(f, pl[j], sg))
            {
              acc[2 + j][q] = acc[2 + j][q] + sg.len;
              cnt[j]++;
            }
          }
      }
    // the crossed faces are counted in integers: any order
#pragma unroll
    for(int j = 0; j < MS_SEC; j++)
    {
      for(int s = 32; s >= 1; s >>= 1) cnt[j] += __shfl_xor(cnt[j], s);
      if(WAVES > 1 && (tid & 63) == 0) crossN[j][tid >> 6] = cnt[j];
    }
    float tot[2 + MS_SEC];
#pragma unroll
    for(int j = 0; j < 2 + MS_SEC; j++)
    {
      if constexpr(NQ == 0) tot[j] = sum64_meet(acc[j][0]);
      else
        tot[j] = sum1024_meet<Q>(acc[j], cross[j]); // (its barrier also publishes crossN)
    }
    if(tid == 0)
    {
      if(pass == 0 && area) area[(int64_t)frame * R + r] = tot[0];
      if(pass == 0 && volume) volume[(int64_t)frame * R + r] = tot[1];
#pragma unroll
      for(int j = 0; j < MS_SEC; j++)
      {
        const int si = pass * MS_SEC + j;
        if(si >= ns) continue;
        const int64_t o = (int64_t)frame * S + secId[s0 + si];
        if(section) section[o] = tot[2 + j];
        if(crossings)
        {
          int all = cnt[j];
          if(WAVES > 1)
          {
            all = 0;
            for(int w = 0; w < WAVES; w++) all += crossN[j][w];
          }
          crossings[o] = all;
        }
      }
    }
    if(WAVES > 1) __syncthreads(); // the next pass writes cross and crossN again
  }
}

// grid: ceil(n V / MS_T)
__global__ __launch_bounds__(MS_T) void ms_vjp_verts_kernel(
    const int32_t * __restrict__ faces, const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
    const int32_t * __restrict__ facePtr, const int32_t * __restrict__ faceRegion, const int32_t * __restrict__ secPtr,
    const int32_t * __restrict__ secId, const float * __restrict__ verts, const float * __restrict__ center,
    const float * __restrict__ planes, int pstride, const float * __restrict__ ga, const float * __restrict__ gvol,
    const float * __restrict__ gs, float * gv, int V, int R, int S, int64_t total, int accumulate)
{
  const int64_t gid = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  if(gid >= total) return;
  const int frame = (int)(gid / V), v = (int)(gid % V);
  const float * X = verts + (int64_t)frame * V * 3;
  float c[3] = {0.0f, 0.0f, 0.0f};
  if(center)
    for(int x = 0; x < 3; x++) c[x] = center[(int64_t)frame * 3 + x];
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for(int a = adjOff[v]; a < adjOff[v + 1]; a++)
  {
    const int fid = adjFace[a];
    const int e0 = facePtr[fid], e1 = facePtr[fid + 1];
    if(e0 == e1) continue; // in no region
    const int32_t * ids = faces + (int64_t)fid * 3;
    MsFace f;
    if(!ms_load_face(X, ids, c, f)) continue;
    for(int cn = 0; cn < 3; cn++)
    {
      if(ids[cn] != v) continue;
      for(int e = e0; e < e1; e++)
      {
        const int r = faceRegion[e];
        float G[3];
        float g = ga ? ga[(int64_t)frame * R + r] : 0.0f;
        if(g != 0.0f && ms_area_grad(f, g, cn, G))
          for(int x = 0; x < 3; x++) acc[x] = acc[x] + G[x];
        g = gvol ? gvol[(int64_t)frame * R + r] : 0.0f;
        if(g != 0.0f)
        {
          ms_volume_grad(f, g, cn, G);
          for(int x = 0; x < 3; x++) acc[x] = acc[x] + G[x];
        }
        if(!gs) continue;
        for(int si = secPtr[r]; si < secPtr[r + 1]; si++)
        {
          const int s = secId[si];
          g = gs[(int64_t)frame * S + s];
          if(g == 0.0f) continue;
          const MsPlane pl = ms_plane(planes + ((int64_t)frame * pstride + s) * 4);
          MsSeg sg;
          if(!pl.live || !ms_segment(f, pl, sg) || sg.len == 0.0f) continue;
          float GL[3], GM[3], GN[3], P[4];
          ms_segment_grad(sg, pl, g, GL, GM, GN, P);
          const int j = (cn - sg.L + 3) % 3; // the corner's place in (L, M, N)
          for(int x = 0; x < 3; x++) acc[x] = acc[x] + ms_pick(GL[x], GM[x], GN[x], j);
        }
      }
    }
  }
  float * o = gv + gid * 3;
  for(int x = 0; x < 3; x++) o[x] = accumulate ? o[x] + acc[x] : acc[x];
}

// grid: n S workgroups of MS_T threads, four partials of each of the four sums a thread.  out: grad_planes [n,S,4], or the frames' terms
__global__ __launch_bounds__(MS_T) void ms_vjp_planes_kernel(const int32_t * __restrict__ faces, const int32_t * __restrict__ regionPtr,
                                                             const int32_t * __restrict__ regionFace, const int32_t * __restrict__ secRegion,
                                                             const float * __restrict__ verts, const float * __restrict__ planes, int pstride,
                                                             const float * __restrict__ gs, float * out, int V, int S, int accumulate)
{
  constexpr int Q = 1024 / MS_T;
  __shared__ float cross[4][MS_T / 64];
  const int frame = blockIdx.x / S, s = blockIdx.x % S, tid = threadIdx.x;
  const int r = secRegion[s], k0 = regionPtr[r], K = regionPtr[r + 1] - k0;
  const float * X = verts + (int64_t)frame * V * 3;
  const float g = gs ? gs[(int64_t)frame * S + s] : 0.0f;
  const MsPlane pl = ms_plane(planes + ((int64_t)frame * pstride + s) * 4);
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  float acc[4][Q];
#pragma unroll
  for(int j = 0; j < 4; j++)
#pragma unroll
    for(int q = 0; q < Q; q++) acc[j][q] = 0.0f;
  if(g != 0.0f && pl.live)
    for(int kb = 0; kb < K; kb += 1024)
#pragma unroll
      for(int q = 0; q < Q; q++)
      {
        const int k = kb + q * MS_T + tid;
        if(k >= K) continue;
        MsFace f;
        MsSeg sg;
        if(!ms_load_face(X, faces + (int64_t)regionFace[k0 + k] * 3, zero, f) || !ms_segment(f, pl, sg) || sg.len == 0.0f) continue;
        float GL[3], GM[3], GN[3], P[4];
        ms_segment_grad(sg, pl, g, GL, GM, GN, P);
#pragma unroll
        for(int j = 0; j < 4; j++) acc[j][q] = acc[j][q] + P[j];
      }
  float tot[4];
#pragma unroll
  for(int j = 0; j < 4; j++) tot[j] = sum1024_meet<Q>(acc[j], cross[j]);
  if(tid < 4)
  {
    float * o = out + ((int64_t)frame * S + s) * 4 + tid;
    const float mine = tid == 3 ? tot[3] : ms_pick(tot[0], tot[1], tot[2], tid);
    *o = accumulate ? *o + mine : mine;
  }
}

// terms [n][S4] -> out [S4]: tiles of MS_FT frames, ascending within a tile from its first term, then across the tiles
__global__ __launch_bounds__(MS_T) void ms_frames_kernel(const float * __restrict__ terms, float * __restrict__ out, int n, int S4, int accumulate)
{
  const int e = blockIdx.x * MS_T + threadIdx.x;
  if(e >= S4) return;
  float tile = 0.0f, tot = 0.0f;
  for(int f = 0; f < n; f++)
  {
    const float term = terms[(int64_t)f * S4 + e];
    tile = f % MS_FT == 0 ? term : tile + term;
    if(f % MS_FT == MS_FT - 1 || f == n - 1) tot = f < MS_FT ? tile : tot + tile;
  }
  out[e] = accumulate ? out[e] + tot : tot;
}

static hipError_t ms_upload(DevBuf & b, const std::vector<int32_t> & v)
{
  hipError_t e = b.reserve(v.empty() ? 4 : sizeof(int32_t) * v.size());
  if(e == hipSuccess && !v.empty()) e = hipMemcpy(b.p.get(), v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice);
  return e;
}

static int ms_check(const char * fn, Measure * ms, int64_t n, const float * verts, const float * planes, int64_t plane_frames, int space)
{
  const std::string name(fn);
  if(!ms) return fail(SMPLPP_ERR_INVALID, name + ": no handle");
  if(n <= 0) return fail(SMPLPP_ERR_INVALID, name + ": n must be positive");
  if(!verts) return fail(SMPLPP_ERR_INVALID, name + ": verts is NULL");
  if(plane_frames != 1 && plane_frames != n) return fail(SMPLPP_ERR_INVALID, name + ": plane_frames must be 1 or n");
  if(ms->S > 0 && !planes) return fail(SMPLPP_ERR_INVALID, name + ": planes is NULL with S > 0");
  if(n > MS_INT32_MAX || n * ms->V * 3 > MS_INT32_MAX || n * ms->R > MS_INT32_MAX || n * ms->S * 4 > MS_INT32_MAX)
    return fail(SMPLPP_ERR_INVALID, name + ": n * V * 3, n * R or n * S * 4 beyond int32 indexing");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// Validate and build the host tables (measure_tables.h), then upload them with the model's faces and adjacency.
extern "C" int smplpp_measure_create(smplpp_model * m, int64_t R, const int64_t * region_ptr, const int64_t * region_face, int64_t S,
                                     const int64_t * section_region, struct smplpp_measure ** out)
{
  const char * fn = "smplpp_measure_create";
  if(out) *out = nullptr;
  if(!m || !out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no model or no out");
  const MeasureTables t = measure_tables(m->F, R, region_ptr, region_face, S, section_region);
  if(t.refusal) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + t.refusal);
  HIP_TRY(hipSetDevice(m->device));
  std::unique_ptr<Measure> ms(new Measure());
  ms->device = m->device, ms->V = m->V, ms->F = m->F, ms->R = t.R, ms->S = t.S, ms->nnz = t.nnz;
  std::vector<int32_t> form[3];
  for(int64_t r = 0; r < t.R; r++)
  {
    const int nq = frame_sum_split(t.regionPtr[(size_t)r + 1] - t.regionPtr[(size_t)r]).nq;
    form[nq == 0 ? 0 : (nq == 4 ? 1 : 2)].push_back((int32_t)r);
  }
  std::vector<int32_t> formRegion;
  for(int k = 0; k < 3; k++)
  {
    formRegion.insert(formRegion.end(), form[k].begin(), form[k].end());
    ms->formOff[k + 1] = (int64_t)formRegion.size();
  }
  HIP_TRY(ms_upload(ms->faces, m->h_faces));
  HIP_TRY(ms_upload(ms->adjOff, m->h_adjOff));
  HIP_TRY(ms_upload(ms->adjFace, m->h_adjFace));
  HIP_TRY(ms_upload(ms->regionPtr, t.regionPtr));
  HIP_TRY(ms_upload(ms->regionFace, t.regionFace));
  HIP_TRY(ms_upload(ms->facePtr, t.facePtr));
  HIP_TRY(ms_upload(ms->faceRegion, t.faceRegion));
  HIP_TRY(ms_upload(ms->secPtr, t.secPtr));
  HIP_TRY(ms_upload(ms->secId, t.secId));
  HIP_TRY(ms_upload(ms->secRegion, t.secRegion));
  HIP_TRY(ms_upload(ms->formRegion, formRegion));
  *out = ms.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_measure_destroy(struct smplpp_measure * ms)
{
  if(!ms) return SMPLPP_OK;
  (void)hipSetDevice(ms->device);
  delete ms;
  return SMPLPP_OK;
}

extern "C" int smplpp_measure_info(const struct smplpp_measure * ms, int64_t * R, int64_t * nnz, int64_t * S)
{
  if(!ms) return fail(SMPLPP_ERR_INVALID, "smplpp_measure_info: no handle");
  if(R) *R = ms->R;
  if(nnz) *nnz = ms->nnz;
  if(S) *S = ms->S;
  return SMPLPP_OK;
}

extern "C" int smplpp_measure(struct smplpp_measure * ms, int64_t n, const float * verts, const float * center, const float * planes,
                              int64_t plane_frames, float * area, float * volume, float * section, int32_t * crossings, int space,
                              void * stream)
{
  const char * fn = "smplpp_measure";
  if(int rc = ms_check(fn, ms, n, verts, planes, plane_frames, space)) return rc;
  if(!area && !volume && !(ms->S > 0 && (section || crossings)))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no output is asked for");
  Frame fr(ms->device, &ms->arena, space, stream, "measure");
  const float * v = fr.in(verts, (size_t)n * ms->V * 3);
  const float * c = fr.in(center, (size_t)n * 3);
  const float * p = fr.in(planes, (size_t)plane_frames * ms->S * 4);
  float * oa = fr.out(area, (size_t)n * ms->R);
  float * ov = fr.out(volume, (size_t)n * ms->R);
  float * os = fr.out(section, (size_t)n * ms->S);
  int32_t * oc = fr.out(crossings, (size_t)n * ms->S);
  return fr.run([&]() -> int {
    const int pstride = plane_frames == n ? (int)ms->S : 0;
    for(int k = 0; k < 3; k++)
    {
      const int nform = (int)(ms->formOff[k + 1] - ms->formOff[k]);
      if(!nform) continue;
      const int32_t * fr_regions = ms->formRegion.as<int32_t>() + ms->formOff[k];
      const dim3 G((unsigned)(n * nform));
#define MS_GO(NQ, T)                                                                                                                     \
  ms_forward_kernel<NQ><<<G, dim3(T), 0, fr.st>>>(ms->faces.as<int32_t>(), ms->regionPtr.as<int32_t>(), ms->regionFace.as<int32_t>(),    \
                                                  ms->secPtr.as<int32_t>(), ms->secId.as<int32_t>(), fr_regions, nform, v, c, p, pstride, \
                                                  oa, ov, os, oc, (int)ms->V, (int)ms->R, (int)ms->S)
      if(k == 0) MS_GO(0, 64);
      else if(k == 1) MS_GO(4, 256);
      else MS_GO(1, 1024);
#undef MS_GO
      HIP_TRY(hipGetLastError());
    }
    return SMPLPP_OK;
  });
}

extern "C" int smplpp_measure_vjp(struct smplpp_measure * ms, int64_t n, const float * verts, const float * center, const float * planes,
                                  int64_t plane_frames, const float * grad_area, const float * grad_volume, const float * grad_section,
                                  float * grad_verts, float * grad_planes, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_measure_vjp";
  if(int rc = ms_check(fn, ms, n, verts, planes, plane_frames, space)) return rc;
  if(!grad_verts && !(ms->S > 0 && grad_planes)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no output is asked for");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  Frame fr(ms->device, &ms->arena, space, stream, "measure VJP");
  const float * v = fr.in(verts, (size_t)n * ms->V * 3);
  const float * c = fr.in(center, (size_t)n * 3);
  const float * p = fr.in(planes, (size_t)plane_frames * ms->S * 4);
  const float * ga = fr.in(grad_area, (size_t)n * ms->R);
  const float * gvol = fr.in(grad_volume, (size_t)n * ms->R);
  const float * gs = fr.in(grad_section, (size_t)n * ms->S);
  float * gv = fr.out(grad_verts, (size_t)n * ms->V * 3, accumulate);
  float * gp = fr.out(grad_planes, (size_t)plane_frames * ms->S * 4, accumulate);
  return fr.run([&]() -> int {
    const int pstride = plane_frames == n ? (int)ms->S : 0;
    if(gv)
    {
      const int64_t total = n * ms->V;
      ms_vjp_verts_kernel<<<dim3((unsigned)((total + MS_T - 1) / MS_T)), dim3(MS_T), 0, fr.st>>>(
          ms->faces.as<int32_t>(), ms->adjOff.as<int32_t>(), ms->adjFace.as<int32_t>(), ms->facePtr.as<int32_t>(), ms->faceRegion.as<int32_t>(),
          ms->secPtr.as<int32_t>(), ms->secId.as<int32_t>(), v, c, p, pstride, ga, gvol, gs, gv, (int)ms->V, (int)ms->R, (int)ms->S, total,
          accumulate);
      HIP_TRY(hipGetLastError());
    }
    if(gp)
    {
      const bool shared = plane_frames == 1 && n > 1;
      float * dst = gp;
      if(shared)
      {
        HIP_TRY(ms->terms.reserve(sizeof(float) * (size_t)n * ms->S * 4));
        dst = ms->terms.as<float>();
      }
      ms_vjp_planes_kernel<<<dim3((unsigned)(n * ms->S)), dim3(MS_T), 0, fr.st>>>(ms->faces.as<int32_t>(), ms->regionPtr.as<int32_t>(),
                                                                                ms->regionFace.as<int32_t>(), ms->secRegion.as<int32_t>(), v, p,
                                                                                pstride, gs, dst, (int)ms->V, (int)ms->S, shared ? 0 : accumulate);
      HIP_TRY(hipGetLastError());
      if(shared)
      {
        const int S4 = (int)ms->S * 4;
        ms_frames_kernel<<<dim3((unsigned)((S4 + MS_T - 1) / MS_T)), dim3(MS_T), 0, fr.st>>>(dst, gp, (int)n, S4, accumulate);
        HIP_TRY(hipGetLastError());
      }
    }
    return SMPLPP_OK;
  });
}
