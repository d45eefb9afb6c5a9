// Raster attribute interpolation: a per-vertex quantity carried into the rasteriser's image through its face ids and
// barycentrics, and the vector-Jacobian product to the attributes and, through the barycentrics, to the vertices.  The rule is in
// include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA).
//
// Forward:
//  ri_forward_kernel   per (pixel, channel): consecutive lanes take consecutive elements of image, so the store is coalesced for
//                      every C; the lanes of one pixel read the same face id and barycentrics (one request), and the three corner
//                      rows of attr come through L2.
// Backward (face and bary are inputs and held fixed; the walk is smplpp_depth_raster_vjp's):
//  ri_vertex_kernel    per (frame, vertex): camera-space position and snapped projection, as the rasteriser's vertex pass.
//  ri_verts_face_kernel per (frame, face), DR_SPLIT lanes: the face's clipped box in row-major order, lane l taking entries l,
//                      l + DR_SPLIT, ...; a pixel that names the face adds beta_i h to corner i's sum (nine sums); the lanes' sums
//                      meet in a fixed xor tree (4, 2, 1) and lane 0 stores them.
//  ri_attr_face_kernel the same walk for up to RI_CHUNK channels: corner i, channel k takes beta_i g[k] (3 RI_CHUNK sums).  A C
//                      above RI_CHUNK is walked once per chunk of channels, so no sum ever leaves its register.
//  ri_gather_kernel    per (frame, vertex): its faces' values in ascending face id (the adjacency of the normals' backward pass),
//                      then R^T once (grad_verts) or the plain store (grad_attr).  One fixed-order sum per element, no
//                      floating-point atomics.
#include "depth_raster_device.h"
#include "trace.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int RI_T = 256;      // threads of every kernel here
constexpr int RI_SPLIT = 8;    // lanes per face in the backward walk
constexpr int RI_CHUNK = 4;    // channels per walk of ri_attr_face_kernel
constexpr int RI_ROW = 12;     // floats per (frame, face) of the workspace: 3 corners x 4 (9 used by grad_verts)
constexpr int64_t RI_MAX_C = 32;

struct RasterInterpState
{
  DevBuf cam, snap; // [n][V] float4 camera-space vertex, int2 snapped projection
  DevBuf fsum;      // [n][F][RI_ROW] per-face corner sums of the walk in flight
};
void StateDelete::operator()(RasterInterpState * s) const
{
  delete s;
}

__global__ __launch_bounds__(RI_T) void ri_forward_kernel(const float * __restrict__ attr, const int32_t * __restrict__ faces,
                                                          const int64_t * __restrict__ face, const float * __restrict__ bary,
                                                          float * __restrict__ image, int C, int HW, int V, int F, int total)
{
  const int64_t gid = (int64_t)blockIdx.x * RI_T + threadIdx.x;
  if(gid >= total) return;
  const int idx = (int)gid, pix = idx / C, k = idx - pix * C;
  const int64_t f = face[pix];
  float v = 0.0f;
  if(f >= 0 && f < F)
  {
    const float * A = attr + (int64_t)(pix / HW) * V * C + k;
    const float * b = bary + (int64_t)pix * 3;
    const int32_t c0 = faces[f * 3], c1 = faces[f * 3 + 1], c2 = faces[f * 3 + 2];
    v = (b[0] * A[(int64_t)c0 * C] + b[1] * A[(int64_t)c1 * C]) + b[2] * A[(int64_t)c2 * C];
  }
  image[idx] = v;
}

__global__ __launch_bounds__(RI_T) void ri_vertex_kernel(const float * __restrict__ verts, const float * __restrict__ camera,
                                                         float4 * __restrict__ cam, int2 * __restrict__ snap, float near, int64_t V,
                                                         int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * RI_T + threadIdx.x;
  if(idx >= nv) return;
  const DrCamera c = dr_camera(camera, idx / V);
  float xc[3], u, v, su, sv;
  const bool ok = dr_project(c, verts[idx * 3], verts[idx * 3 + 1], verts[idx * 3 + 2], near, xc, u, v, su, sv);
  cam[idx] = make_float4(xc[0], xc[1], xc[2], 0.0f);
  snap[idx] = ok ? make_int2((int)su, (int)sv) : make_int2(DR_BAD, DR_BAD);
}

// the lanes' partial sums of one face meet in lane 0: ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7))
template<int N>
__device__ inline void ri_tree(float * s)
{
  for(int m = RI_SPLIT / 2; m >= 1; m >>= 1)
#pragma unroll
    for(int k = 0; k < N; k++) s[k] = s[k] + __shfl_xor(s[k], m);
}

__global__ __launch_bounds__(RI_T) void ri_verts_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                             const int32_t * __restrict__ faces, const float * __restrict__ camera,
                                                             const float * __restrict__ attr, const int64_t * __restrict__ face,
                                                             const float * __restrict__ bary, const float * __restrict__ gi,
                                                             float * __restrict__ fsum, int C, int64_t H, int64_t W, int64_t V,
                                                             int64_t F, int64_t nf)
{
  const int64_t tid = (int64_t)blockIdx.x * RI_T + threadIdx.x;
  const int64_t idx = tid / RI_SPLIT;
  const int part = (int)(tid % RI_SPLIT);
  const bool in = idx < nf;
  const int64_t frame = in ? idx / F : 0, f = in ? idx % F : 0;
  DrFace t;
  const bool live = in && dr_face_setup(t, cam, snap, faces, frame, f, V, H, W) == DR_FACE_OK;
  float s[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if(live)
  {
    const DrCamera c = dr_camera(camera, frame);
    const int64_t * ff = face + frame * H * W;
    const float * bf = bary + frame * H * W * 3;
    const float * gf = gi + frame * H * W * C;
    const float * A0 = attr + (frame * V + faces[f * 3]) * C;
    const float * A1 = attr + (frame * V + faces[f * 3 + 1]) * C;
    const float * A2 = attr + (frame * V + faces[f * 3 + 2]) * C;
    const float nn = (t.nx * t.nx + t.ny * t.ny) + t.nz * t.nz;
    const float c1[3] = {t.e2[1] * t.nz - t.e2[2] * t.ny, t.e2[2] * t.nx - t.e2[0] * t.nz, t.e2[0] * t.ny - t.e2[1] * t.nx}; // e2 x n
    const float c2[3] = {t.ny * t.e1[2] - t.nz * t.e1[1], t.nz * t.e1[0] - t.nx * t.e1[2], t.nx * t.e1[1] - t.ny * t.e1[0]}; // n x e1
    const float nrm[3] = {t.nx, t.ny, t.nz};
    const int w = t.i1 - t.i0 + 1;
    const int64_t area = (int64_t)w * (t.j1 - t.j0 + 1);
    for(int64_t r = part; r < area; r += RI_SPLIT)
    {
      const int i = t.i0 + (int)(r % w), j = t.j0 + (int)(r / w);
      const int64_t pix = (int64_t)j * W + i;
      if(ff[pix] != f) continue;
      const float * g = gf + pix * C;
      float ga = 0.0f, gb = 0.0f, gc = 0.0f;
      bool any = false;
      for(int k = 0; k < C; k++)
      {
        const float gk = g[k];
        if(gk == 0.0f) continue;
        any = true;
        ga = ga + gk * A0[k], gb = gb + gk * A1[k], gc = gc + gk * A2[k];
      }
      if(!any) continue;
      float dx, dy;
      dr_ray(c, i, j, dx, dy);
      const float nd = (t.nx * dx + t.ny * dy) + t.nz;
      const float u1 = gb - ga, u2 = gc - ga;
      float q[3];
      for(int x = 0; x < 3; x++) q[x] = (u1 * c1[x] + u2 * c2[x]) / nn;
      const float sc = ((q[0] * dx + q[1] * dy) + q[2]) / nd;
      const float * b = bf + pix * 3;
      const float b0 = b[0], b1 = b[1], b2 = b[2];
      for(int x = 0; x < 3; x++)
      {
        const float h = nrm[x] * sc - q[x];
        s[x] = s[x] + b0 * h, s[3 + x] = s[3 + x] + b1 * h, s[6 + x] = s[6 + x] + b2 * h;
      }
    }
  }
  ri_tree<9>(s);
  if(!in || part != 0) return;
  float * o = fsum + idx * RI_ROW;
  for(int k = 0; k < 9; k++) o[k] = s[k]; // (a face that is not live: zeros)
}

// channels [c0, c0 + NC) of grad_attr's per-face sums: fsum[idx][corner][NC]
template<int NC>
__global__ __launch_bounds__(RI_T) void ri_attr_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                            const int32_t * __restrict__ faces, const int64_t * __restrict__ face,
                                                            const float * __restrict__ bary, const float * __restrict__ gi,
                                                            float * __restrict__ fsum, int C, int c0, int64_t H, int64_t W, int64_t V,
                                                            int64_t F, int64_t nf)
{
  const int64_t tid = (int64_t)blockIdx.x * RI_T + threadIdx.x;
  const int64_t idx = tid / RI_SPLIT;
  const int part = (int)(tid % RI_SPLIT);
  const bool in = idx < nf;
  const int64_t frame = in ? idx / F : 0, f = in ? idx % F : 0;
  DrFace t;
  const bool live = in && dr_face_setup(t, cam, snap, faces, frame, f, V, H, W) == DR_FACE_OK;
  float s[3 * NC];
#pragma unroll
  for(int k = 0; k < 3 * NC; k++) s[k] = 0.0f;
  if(live)
  {
    const int64_t * ff = face + frame * H * W;
    const float * bf = bary + frame * H * W * 3;
    const float * gf = gi + frame * H * W * C + c0;
    const int w = t.i1 - t.i0 + 1;
    const int64_t area = (int64_t)w * (t.j1 - t.j0 + 1);
    for(int64_t r = part; r < area; r += RI_SPLIT)
    {
      const int i = t.i0 + (int)(r % w), j = t.j0 + (int)(r / w);
      const int64_t pix = (int64_t)j * W + i;
      if(ff[pix] != f) continue;
      float g[NC];
      bool any = false;
#pragma unroll
      for(int k = 0; k < NC; k++) g[k] = gf[pix * C + k], any = any || g[k] != 0.0f;
      if(!any) continue;
      const float * b = bf + pix * 3;
      const float bb[3] = {b[0], b[1], b[2]};
#pragma unroll
      for(int k = 0; k < NC; k++)
        if(g[k] != 0.0f)
#pragma unroll
          for(int e = 0; e < 3; e++) s[e * NC + k] = s[e * NC + k] + bb[e] * g[k];
    }
  }
  ri_tree<3 * NC>(s);
  if(!in || part != 0) return;
  float * o = fsum + idx * RI_ROW;
#pragma unroll
  for(int k = 0; k < 3 * NC; k++) o[k] = s[k];
}

// out[(frame V + v) stride + off + x], x < width: the vertex's faces' fsum[face][corner][width] in ascending face id; ROT: R^T first
template<bool ROT>
__global__ __launch_bounds__(RI_T) void ri_gather_kernel(const float * __restrict__ fsum, const int32_t * __restrict__ faces,
                                                         const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
                                                         const float * __restrict__ camera, float * __restrict__ out, int width,
                                                         int stride, int off, int accumulate, int64_t V, int64_t F, int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * RI_T + threadIdx.x;
  if(idx >= nv) return;
  const int64_t frame = idx / V;
  const int32_t v = (int32_t)(idx % V);
  float g[RI_CHUNK] = {0.0f, 0.0f, 0.0f, 0.0f};
  for(int32_t q = adjOff[v]; q < adjOff[v + 1]; q++)
  {
    const int64_t f = adjFace[q];
    for(int k = 0; k < 3; k++)
      if(faces[f * 3 + k] == v)
      {
        const float * p = fsum + (frame * F + f) * RI_ROW + k * width;
#pragma unroll
        for(int x = 0; x < RI_CHUNK; x++)
          if(x < width) g[x] = g[x] + p[x];
      }
  }
  float * o = out + idx * stride + off;
  if(ROT)
  {
    const float * R = camera + frame * 16;
    for(int x = 0; x < 3; x++)
    {
      const float w = (R[x] * g[0] + R[3 + x] * g[1]) + R[6 + x] * g[2];
      o[x] = accumulate ? o[x] + w : w;
    }
    return;
  }
#pragma unroll
  for(int x = 0; x < RI_CHUNK; x++)
    if(x < width) o[x] = accumulate ? o[x] + g[x] : g[x];
}

static unsigned ri_grid(int64_t items)
{
  return (unsigned)((items + RI_T - 1) / RI_T);
}

static int ri_check(const char * fn, smplpp_model * m, int64_t n, int64_t C, int64_t H, int64_t W, int space)
{
  if(C < 1 || C > RI_MAX_C) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": C must be in [1, 32]");
  int rc = dr_check(fn, m, n, H, W, space);
  if(rc) return rc;
  if(n * H * W * C > 0x7fffffffLL || n * m->V * C > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * H * W * C or n * V * C beyond int32 indexing");
  return SMPLPP_OK;
}

// all pointers on the device
static int ri_vjp_device(smplpp_model * m, RasterInterpState * s, int64_t n, const float * attr, int C, const float * verts,
                         const float * camera, int64_t H, int64_t W, float near, const int64_t * face, const float * bary,
                         const float * gi, float * ga, float * gv, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, F = m->F, nf = n * F, nv = n * V;
  HIP_TRY(s->cam.reserve(sizeof(float4) * (size_t)nv));
  HIP_TRY(s->snap.reserve(sizeof(int2) * (size_t)nv));
  HIP_TRY(s->fsum.reserve(sizeof(float) * RI_ROW * (size_t)nf));
  float4 * cam = s->cam.as<float4>();
  int2 * snap = s->snap.as<int2>();
  float * fsum = s->fsum.as<float>();
  const dim3 T(RI_T), walk(ri_grid(nf * RI_SPLIT)), pv(ri_grid(nv));
  ri_vertex_kernel<<<pv, T, 0, st>>>(verts, camera, cam, snap, near, V, nv);
  HIP_TRY(hipGetLastError());
  if(gv)
  {
    ri_verts_face_kernel<<<walk, T, 0, st>>>(cam, snap, m->faces.get(), camera, attr, face, bary, gi, fsum, C, H, W, V, F, nf);
    HIP_TRY(hipGetLastError());
    ri_gather_kernel<true><<<pv, T, 0, st>>>(fsum, m->faces.get(), m->adjOff.get(), m->adjFace.get(), camera, gv, 3, 3, 0, accumulate, V,
                                             F, nv);
    HIP_TRY(hipGetLastError());
  }
  for(int c0 = 0; ga && c0 < C; c0 += RI_CHUNK)
  {
    const int nc = std::min(RI_CHUNK, C - c0);
#define RI_WALK(NC) ri_attr_face_kernel<NC><<<walk, T, 0, st>>>(cam, snap, m->faces.get(), face, bary, gi, fsum, C, c0, H, W, V, F, nf)
    if(nc == 1) RI_WALK(1);
    else if(nc == 2) RI_WALK(2);
    else if(nc == 3) RI_WALK(3);
    else RI_WALK(4);
#undef RI_WALK
    HIP_TRY(hipGetLastError());
    ri_gather_kernel<false><<<pv, T, 0, st>>>(fsum, m->faces.get(), m->adjOff.get(), m->adjFace.get(), camera, ga, nc, C, c0, accumulate,
                                              V, F, nv);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_raster_interpolate(smplpp_model * m, int64_t n, const float * attr, int64_t C, int64_t H, int64_t W,
                                         const int64_t * face, const float * bary, float * image, int space, void * stream)
{
  const char * fn = "smplpp_raster_interpolate";
  if(!m || n <= 0 || !attr || !face || !bary || !image) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = ri_check(fn, m, n, C, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "raster interpolate");
  const float * a = fr.in(attr, (size_t)(n * m->V * C));
  const int64_t * f = fr.in(face, (size_t)(n * H * W));
  const float * b = fr.in(bary, (size_t)(n * H * W * 3));
  float * o = fr.out(image, (size_t)(n * H * W * C));
  return fr.run([&] {
    const int64_t total = n * H * W * C;
    ri_forward_kernel<<<dim3(ri_grid(total)), dim3(RI_T), 0, fr.st>>>(a, m->faces.get(), f, b, o, (int)C, (int)(H * W), (int)m->V,
                                                                      (int)m->F, (int)total);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_raster_interpolate_vjp(smplpp_model * m, int64_t n, const float * attr, int64_t C, const float * verts,
                                             const float * camera, int64_t H, int64_t W, float near, const int64_t * face,
                                             const float * bary, const float * grad_image, float * grad_attr, float * grad_verts,
                                             int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_raster_interpolate_vjp";
  if(!m || n <= 0 || !attr || !verts || !camera || !face || !bary || !grad_image)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(!grad_attr && !grad_verts) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_attr and grad_verts are both NULL");
  if(!(std::isfinite(near) && near > 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": near must be finite and > 0");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = ri_check(fn, m, n, C, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "raster interpolate VJP");
  if(!m->ri) m->ri.reset(new RasterInterpState());
  RasterInterpState * s = m->ri.get();
  const float * a = fr.in(attr, (size_t)(n * m->V * C));
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const int64_t * f = fr.in(face, (size_t)(n * H * W));
  const float * b = fr.in(bary, (size_t)(n * H * W * 3));
  const float * g = fr.in(grad_image, (size_t)(n * H * W * C));
  float * ga = fr.out(grad_attr, (size_t)(n * m->V * C), accumulate);
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  return fr.run([&] { return ri_vjp_device(m, s, n, a, (int)C, v, c, H, W, near, f, b, g, ga, gv, accumulate, fr.st); });
}
