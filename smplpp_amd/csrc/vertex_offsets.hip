// SMPL+D: per-vertex rest-pose offsets carried through linear blend skinning, their vector-Jacobian product, and the
// mesh Laplacian that regularises them.  The rules are in include/smplpp_hip.h; every fp32 operation below is rounded on its own (no
// contraction to FMA), every output element is one fixed-order sum, and there are no floating-point atomics.
//
//  vo_kernel<MAXW, MODE>  over (tile of `ft` frames x chunk of 256 elements of a [V,3] row).  The tile's 24 x 9 rotation entries
//                      per frame go to LDS once (ft x 864 bytes, sized at launch).  A lane owns one ELEMENT (v, x) of the row and
//                      walks the tile's frames in order: consecutive lanes move consecutive floats of every [.,V,3] array (4-byte accesses: no alignment is
//                      asked of the caller), and a lane blends only the row (forward) or the column (backward) of M it needs, three
//                      entries from the vertex's sparse weight and joint tables, so no entry of M is computed twice.
//                        VO_FWD     verts_out = verts + M d / wSum, rest_displaced = rest + d
//                        VO_BWD     grad_offsets[f] = M^T (g / wSum)              (per-frame offsets)
//                        VO_SHARED  part[tile] = the tile's frames summed in ascending order from the first term (ft = VO_FT)
//  vo_tiles_kernel     per element: the tiles' partial sums in ascending tile order, then the store or the one addition of accumulate.
//  vo_laplacian_kernel per (frame, vertex, channel): the vertex's faces in ascending face id from the adjacency of the normals' backward
//                      pass; consecutive lanes store consecutive floats for every C.
// ft only shapes the launch (more workgroups for a small batch); no bit depends on it, and SMPLPP_VERTEX_OFFSETS_FRAMES (read at model
// creation) fixes it so that tests can hold every tile size to the same bits.
#include "common.h"
#include "staging.h"
#include "trace.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int VO_T = 256;            // threads of every kernel here
constexpr int VO_FT = SMPLPP_VERTEX_OFFSETS_TILE; // frames per tile of the shared sum (and the most of any tile)
constexpr int VO_R = NJ * 9;         // floats of a frame's rotations in LDS
constexpr int VO_U = 8;              // frames whose loads a lane issues before it computes
constexpr int64_t VO_MAX_C = 32;
enum { VO_FWD = 0, VO_BWD = 1, VO_SHARED = 2 };

struct VertexOffsetsState
{
  DevBuf part; // [tiles][V][3] partial sums of the shared backward in flight
};
void StateDelete::operator()(VertexOffsetsState * s) const
{
  delete s;
}

// entry i of the three of M the element needs (forward: M[x][i]; backward: M[i][x]), over the non-zero weights in ascending joint
template<int MAXW, bool TRANSPOSE>
__device__ inline void vo_blend(const float * __restrict__ sRf, const uint8_t * __restrict__ wi, const float * __restrict__ wv, int x,
                                float & m0, float & m1, float & m2)
{
  m0 = m1 = m2 = 0.0f;
  constexpr int UNR = MAXW > 8 ? 4 : MAXW;
#pragma unroll UNR
  for(int q = 0; q < MAXW; q++)
  {
    const float w = wv[q];
    if(w == 0.0f) continue;
    const float * R = sRf + (int)wi[q] * 9 + (TRANSPOSE ? x : 3 * x);
    m0 = m0 + w * R[0];
    m1 = m1 + w * R[TRANSPOSE ? 3 : 1];
    m2 = m2 + w * R[TRANSPOSE ? 6 : 2];
  }
}

// grid: ceil(n / ft) tiles x ceil(3 V / 256) chunks; dynamic LDS: ft VO_R floats.  a: verts (FWD) or grad_verts; d: offsets (FWD); o: verts_out, grad_offsets
// or part.  a and o, rest and rest_out may be the same array (an element is read, then written, by its own lane).
template<int MAXW, int MODE>
__global__ __launch_bounds__(VO_T) void vo_kernel(const float * __restrict__ xforms, const float * a, const float * __restrict__ d,
                                                  const float * rest, float * rest_out, float * o, const uint8_t * __restrict__ wIdx,
                                                  const float * __restrict__ wVal, const float * __restrict__ wSum, int n, int V3, int ft,
                                                  int ntile, int shared, int accumulate)
{
  extern __shared__ float sR[]; // [ft][VO_R]
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % ntile, chunk = blockIdx.x / ntile;
  const int f0 = tile * ft, nf = min(ft, n - f0);
  for(int i = tid; i < nf * VO_R; i += VO_T)
  {
    const int fl = i / VO_R, e = i - fl * VO_R, j = e / 9, q = e - j * 9;
    sR[i] = xforms[((int64_t)(f0 + fl) * NJ + j) * 16 + (q / 3) * 4 + q % 3];
  }
  __syncthreads();
  const int e = chunk * VO_T + tid;
  if(e >= V3) return;
  const int v = e / 3, x = e - v * 3;
  const uint8_t * wi = wIdx + (int64_t)v * MAXW;
  const float * wv = wVal + (int64_t)v * MAXW;
  const float ws = wSum[v];
  if(MODE == VO_FWD)
  {
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    if(shared) d0 = d[v * 3], d1 = d[v * 3 + 1], d2 = d[v * 3 + 2];
    for(int fb = 0; fb < nf; fb += VO_U)
    {
      float av[VO_U], rv[VO_U], dv[VO_U][3];
#pragma unroll
      for(int u = 0; u < VO_U; u++) // the batch's loads first: VO_U requests in flight per lane
      {
        const int64_t row = (int64_t)(f0 + min(fb + u, nf - 1)) * V3;
        av[u] = a[row + e];
        rv[u] = rest_out ? rest[row + e] : 0.0f;
        dv[u][0] = shared ? d0 : d[row + v * 3], dv[u][1] = shared ? d1 : d[row + v * 3 + 1], dv[u][2] = shared ? d2 : d[row + v * 3 + 2];
      }
#pragma unroll
      for(int u = 0; u < VO_U; u++)
      {
        if(fb + u >= nf) break;
        const int64_t row = (int64_t)(f0 + fb + u) * V3;
        float m0, m1, m2;
        vo_blend<MAXW, false>(sR + (fb + u) * VO_R, wi, wv, x, m0, m1, m2);
        const float delta = ((m0 * dv[u][0] + m1 * dv[u][1]) + m2 * dv[u][2]) / ws;
        o[row + e] = av[u] + delta;
        if(rest_out) rest_out[row + e] = rv[u] + (x == 0 ? dv[u][0] : (x == 1 ? dv[u][1] : dv[u][2]));
      }
    }
  }
  else
  {
    float s = 0.0f;
    for(int fb = 0; fb < nf; fb += VO_U)
    {
      float gv[VO_U][3], ov[VO_U];
#pragma unroll
      for(int u = 0; u < VO_U; u++)
      {
        const int64_t row = (int64_t)(f0 + min(fb + u, nf - 1)) * V3;
        gv[u][0] = a[row + v * 3], gv[u][1] = a[row + v * 3 + 1], gv[u][2] = a[row + v * 3 + 2];
        ov[u] = (MODE == VO_BWD && accumulate) ? o[row + e] : 0.0f;
      }
#pragma unroll
      for(int u = 0; u < VO_U; u++)
      {
        if(fb + u >= nf) break;
        const float g0 = gv[u][0] / ws, g1 = gv[u][1] / ws, g2 = gv[u][2] / ws;
        float m0, m1, m2;
        vo_blend<MAXW, true>(sR + (fb + u) * VO_R, wi, wv, x, m0, m1, m2);
        const float t = (m0 * g0 + m1 * g1) + m2 * g2;
        if(MODE == VO_BWD) o[(int64_t)(f0 + fb + u) * V3 + e] = accumulate ? ov[u] + t : t;
        else s = fb + u == 0 ? t : s + t;
      }
    }
    if(MODE == VO_SHARED) o[(int64_t)tile * V3 + e] = s;
  }
}

__global__ __launch_bounds__(VO_T) void vo_tiles_kernel(const float * __restrict__ part, float * __restrict__ out, int ntile, int V3,
                                                        int accumulate)
{
  const int e = blockIdx.x * VO_T + threadIdx.x;
  if(e >= V3) return;
  float s = part[e];
  for(int t = 1; t < ntile; t++) s = s + part[(int64_t)t * V3 + e];
  out[e] = accumulate ? out[e] + s : s;
}

__global__ __launch_bounds__(VO_T) void vo_laplacian_kernel(const float * __restrict__ x, const int32_t * __restrict__ faces,
                                                            const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
                                                            float * __restrict__ out, int C, int V, int total, int accumulate)
{
  const int64_t gid = (int64_t)blockIdx.x * VO_T + threadIdx.x;
  if(gid >= total) return;
  const int idx = (int)gid, fv = idx / C, k = idx - fv * C, frame = fv / V, v = fv - frame * V;
  const float * X = x + (int64_t)frame * V * C + k;
  const float xv = X[(int64_t)v * C];
  float s = 0.0f;
  for(int32_t q = adjOff[v]; q < adjOff[v + 1]; q++)
  {
    const int32_t * t = faces + (int64_t)adjFace[q] * 3;
    for(int c = 0; c < 3; c++)
      if(t[c] == v)
      {
        const float xa = X[(int64_t)t[(c + 1) % 3] * C], xb = X[(int64_t)t[(c + 2) % 3] * C];
        s = s + ((xv - xa) + (xv - xb));
      }
  }
  out[idx] = accumulate ? out[idx] + s : s;
}

// the launch shape: the tile is halved until the grid holds eight workgroups per compute unit (a count of workgroups to spread, not
// of resident ones: at ft = 32 the 27 KB of LDS let five stay on a compute unit), or is what the model's environment fixed
static int vo_frames(smplpp_model * m, int64_t n)
{
  if(m->vo_frames > 0) return m->vo_frames;
  const int64_t chunks = (m->V * 3 + VO_T - 1) / VO_T, want = 8 * (int64_t)device_cus(m->device);
  int ft = VO_FT;
  while(ft > 1 && ((n + ft - 1) / ft) * chunks < want) ft /= 2;
  return ft;
}

template<int MODE>
static int vo_launch(smplpp_model * m, int64_t n, int ft, const float * xf, const float * a, const float * d, const float * rest,
                     float * rest_out, float * o, int shared, int accumulate, hipStream_t st)
{
  const int V3 = (int)(m->V * 3), ntile = (int)((n + ft - 1) / ft), nchunk = (V3 + VO_T - 1) / VO_T;
  const dim3 G((unsigned)ntile * (unsigned)nchunk), T(VO_T);
  const size_t lds = sizeof(float) * VO_R * (size_t)ft;
#define VO_GO(MAXW) \
  vo_kernel<MAXW, MODE><<<G, T, lds, st>>>(xf, a, d, rest, rest_out, o, m->wIdx.get(), m->wVal.get(), m->wSum.get(), (int)n, V3, ft, ntile, shared, accumulate)
  if(m->maxw == 4) VO_GO(4);
  else if(m->maxw == 8) VO_GO(8);
  else VO_GO(NJ);
#undef VO_GO
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int vo_check(const char * fn, smplpp_model * m, int64_t n, int64_t per_vertex, int space)
{
  if(!m) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no model");
  if(n <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n must be positive");
  if(n > 0x7fffffffLL || n * m->V * per_vertex > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * V * " + std::to_string(per_vertex) + " beyond int32 indexing");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_vertex_offsets(smplpp_model * m, int64_t n, const float * verts, const float * xforms, const float * offsets,
                                     int64_t offset_frames, const float * rest, float * rest_displaced, float * verts_out, int space,
                                     void * stream)
{
  const char * fn = "smplpp_vertex_offsets";
  int rc = vo_check(fn, m, n, 3, space);
  if(rc) return rc;
  if(!verts || !xforms || !offsets || !verts_out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": verts, xforms, offsets or verts_out is NULL");
  if(offset_frames != 1 && offset_frames != n) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": offset_frames must be 1 or n");
  if(rest_displaced && !rest) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": rest_displaced needs rest");
  const size_t nv3 = (size_t)n * m->V * 3;
  Frame fr(m->device, &m->arena, space, stream, "vertex offsets");
  const float * v = fr.in(verts, nv3);
  const float * xf = fr.in(xforms, (size_t)n * NJ * 16);
  const float * d = fr.in(offsets, (size_t)offset_frames * m->V * 3);
  const float * r = rest_displaced ? fr.in(rest, nv3) : nullptr;
  float * rd = fr.out(rest_displaced, nv3);
  float * o = fr.out(verts_out, nv3);
  return fr.run([&] {
    return vo_launch<VO_FWD>(m, n, vo_frames(m, n), xf, v, d, r, rd, o, offset_frames == 1 ? 1 : 0, 0, fr.st);
  });
}

extern "C" int smplpp_vertex_offsets_vjp(smplpp_model * m, int64_t n, const float * xforms, const float * grad_verts, int64_t offset_frames,
                                         float * grad_offsets, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_vertex_offsets_vjp";
  int rc = vo_check(fn, m, n, 3, space);
  if(rc) return rc;
  if(!xforms || !grad_verts || !grad_offsets) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": xforms, grad_verts or grad_offsets is NULL");
  if(offset_frames != 1 && offset_frames != n) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": offset_frames must be 1 or n");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  if(grad_offsets == grad_verts) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_offsets must not be grad_verts");
  Frame fr(m->device, &m->arena, space, stream, "vertex offsets VJP");
  const float * xf = fr.in(xforms, (size_t)n * NJ * 16);
  const float * g = fr.in(grad_verts, (size_t)n * m->V * 3);
  float * o = fr.out(grad_offsets, (size_t)offset_frames * m->V * 3, accumulate);
  return fr.run([&] {
    if(offset_frames == n) // (n = 1: the shared sum is its single term, the same bits)
      return vo_launch<VO_BWD>(m, n, vo_frames(m, n), xf, g, nullptr, nullptr, nullptr, o, 0, accumulate, fr.st);
    // one field for all frames: the tile is the rule's
    if(!m->vo) m->vo.reset(new VertexOffsetsState());
    VertexOffsetsState * s = m->vo.get();
    const int ntile = (int)((n + VO_FT - 1) / VO_FT), V3 = (int)(m->V * 3);
    HIP_TRY(s->part.reserve(sizeof(float) * (size_t)ntile * V3));
    if(int rc2 = vo_launch<VO_SHARED>(m, n, VO_FT, xf, g, nullptr, nullptr, nullptr, s->part.as<float>(), 1, 0, fr.st)) return rc2;
    vo_tiles_kernel<<<dim3((unsigned)((V3 + VO_T - 1) / VO_T)), dim3(VO_T), 0, fr.st>>>(s->part.as<float>(), o, ntile, V3, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_mesh_laplacian(smplpp_model * m, int64_t n, const float * x, int64_t C, float * out, int accumulate, int space,
                                     void * stream)
{
  const char * fn = "smplpp_mesh_laplacian";
  if(C < 1 || C > VO_MAX_C) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": C must be in [1, 32]");
  int rc = vo_check(fn, m, n, C, space);
  if(rc) return rc;
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": the model has no faces");
  if(!x || !out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": x or out is NULL");
  if(x == out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": out must not be x");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  const int64_t total = n * m->V * C;
  Frame fr(m->device, &m->arena, space, stream, "mesh laplacian");
  const float * xi = fr.in(x, (size_t)total);
  float * o = fr.out(out, (size_t)total, accumulate);
  return fr.run([&] {
    vo_laplacian_kernel<<<dim3((unsigned)((total + VO_T - 1) / VO_T)), dim3(VO_T), 0, fr.st>>>(xi, m->faces.get(), m->adjOff.get(),
                                                                                              m->adjFace.get(), o, (int)C, (int)m->V,
                                                                                              (int)total, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
