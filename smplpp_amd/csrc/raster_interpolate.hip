// Raster attribute interpolation: a per-vertex quantity carried into the rasteriser's image through its face ids and
// barycentrics, and the vector-Jacobian product to the attributes and, through the barycentrics, to the vertices.  The rule is in
// include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA).
//
// Forward:
//  ri_forward_kernel   per (pixel, channel): consecutive lanes take consecutive elements of image, so the store is coalesced for
//                      every C; the lanes of one pixel read the same face id and barycentrics (one request), and the three corner
//                      rows of attr come through L2.
// Backward (face and bary are inputs and held fixed).  The vertex pass, the walk (DR_SPLIT lanes per (frame, face), a fixed xor tree)
// and the gather of the per-face sums to the vertices are smplpp_depth_raster_vjp's, from raster_walk.h, on the rasteriser's state;
// defined here are the two bodies of the walk:
//  ri_verts_face_kernel a pixel that names the face adds beta_i h to corner i's sum (nine sums); lane 0 stores them.
//  ri_attr_face_kernel the same walk for up to RI_CHUNK channels: corner i, channel k takes beta_i g[k] (3 RI_CHUNK sums).  A C
//                      above RI_CHUNK is walked once per chunk of channels, so no sum ever leaves its register.
#include "raster_walk.h"
#include "trace.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int RI_CHUNK = 4;    // channels per walk of ri_attr_face_kernel (the widest dr_gather takes)
constexpr int RI_ROW = 12;     // floats per (frame, face) of the workspace: 3 corners x 4 (9 used by grad_verts)
constexpr int64_t RI_MAX_C = 32;

__global__ __launch_bounds__(DR_T) void ri_forward_kernel(const float * __restrict__ attr, const int32_t * __restrict__ faces,
                                                          const int64_t * __restrict__ face, const float * __restrict__ bary,
                                                          float * __restrict__ image, int C, int HW, int V, int F, int total)
{
  const int64_t gid = (int64_t)blockIdx.x * DR_T + threadIdx.x;
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

// grad_verts' share of a pixel: beta_i h to corner i, h from the pixel's C cotangents and the face's three attribute rows
struct RiVertsBody
{
  const float * camera, * attr, * bary, * gi;
  const int32_t * faces;
  int C;
  int64_t HW, V;
  DrCamera c;
  const float * bf, * gf, * A0, * A1, * A2;
  float nn, c1[3], c2[3], nrm[3];
  __device__ void face(const DrFace & t, int64_t frame, int64_t f)
  {
    c = dr_camera(camera, frame);
    bf = bary + frame * HW * 3;
    gf = gi + frame * HW * C;
    A0 = attr + (frame * V + faces[f * 3]) * C;
    A1 = attr + (frame * V + faces[f * 3 + 1]) * C;
    A2 = attr + (frame * V + faces[f * 3 + 2]) * C;
    nn = (t.nx * t.nx + t.ny * t.ny) + t.nz * t.nz;
    c1[0] = t.e2[1] * t.nz - t.e2[2] * t.ny, c1[1] = t.e2[2] * t.nx - t.e2[0] * t.nz, c1[2] = t.e2[0] * t.ny - t.e2[1] * t.nx; // e2 x n
    c2[0] = t.ny * t.e1[2] - t.nz * t.e1[1], c2[1] = t.nz * t.e1[0] - t.nx * t.e1[2], c2[2] = t.nx * t.e1[1] - t.ny * t.e1[0]; // n x e1
    nrm[0] = t.nx, nrm[1] = t.ny, nrm[2] = t.nz;
  }
  __device__ void pixel(const DrFace & t, int i, int j, int64_t pix, float * s) const
  {
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
    if(!any) return;
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
};

__global__ __launch_bounds__(DR_T) void ri_verts_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                             const int32_t * __restrict__ faces, const float * __restrict__ camera,
                                                             const float * __restrict__ attr, const int64_t * __restrict__ face,
                                                             const float * __restrict__ bary, const float * __restrict__ gi,
                                                             float * __restrict__ fsum, int C, int64_t H, int64_t W, int64_t V,
                                                             int64_t F, int64_t nf)
{
  float s[9];
  RiVertsBody body{camera, attr, bary, gi, faces, C, H * W, V};
  const DrWalk w = dr_walk(cam, snap, faces, face, H, W, V, F, nf, s, body);
  if(!w.in || w.part != 0) return;
  float * o = fsum + w.idx * RI_ROW;
  for(int k = 0; k < 9; k++) o[k] = s[k]; // (a face that is not live: zeros)
}

// grad_attr's share of a pixel, channels [c0, c0 + NC): beta_i g[k] to corner i, channel k
template<int NC>
struct RiAttrBody
{
  const float * bary, * gi;
  int C;
  int64_t HW;
  const float * bf, * gf;
  __device__ void face(const DrFace &, int64_t frame, int64_t)
  {
    bf = bary + frame * HW * 3;
    gf = gi + frame * HW * C;
  }
  __device__ void pixel(const DrFace &, int, int, int64_t pix, float * s) const
  {
    float g[NC];
    bool any = false;
#pragma unroll
    for(int k = 0; k < NC; k++) g[k] = gf[pix * C + k], any = any || g[k] != 0.0f;
    if(!any) return;
    const float * b = bf + pix * 3;
    const float bb[3] = {b[0], b[1], b[2]};
#pragma unroll
    for(int k = 0; k < NC; k++)
      if(g[k] != 0.0f)
#pragma unroll
        for(int e = 0; e < 3; e++) s[e * NC + k] = s[e * NC + k] + bb[e] * g[k];
  }
};

// fsum[idx][corner][NC]; gi points at channel c0
template<int NC>
__global__ __launch_bounds__(DR_T) void ri_attr_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                            const int32_t * __restrict__ faces, const int64_t * __restrict__ face,
                                                            const float * __restrict__ bary, const float * __restrict__ gi,
                                                            float * __restrict__ fsum, int C, int64_t H, int64_t W, int64_t V,
                                                            int64_t F, int64_t nf)
{
  float s[3 * NC];
  RiAttrBody<NC> body{bary, gi, C, H * W};
  const DrWalk w = dr_walk(cam, snap, faces, face, H, W, V, F, nf, s, body);
  if(!w.in || w.part != 0) return;
  float * o = fsum + w.idx * RI_ROW;
#pragma unroll
  for(int k = 0; k < 3 * NC; k++) o[k] = s[k];
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
static int ri_vjp_device(smplpp_model * m, DepthRasterState * s, int64_t n, const float * attr, int C, const float * verts,
                         const float * camera, int64_t H, int64_t W, float near, const int64_t * face, const float * bary,
                         const float * gi, float * ga, float * gv, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, F = m->F, nf = n * F;
  int rc = dr_vertex_pass(m, s, n, verts, camera, near, st);
  if(rc) return rc;
  HIP_TRY(s->fsum.reserve(sizeof(float) * RI_ROW * (size_t)nf));
  const float4 * cam = s->cam.as<float4>();
  const int2 * snap = s->snap.as<int2>();
  float * fsum = s->fsum.as<float>();
  const dim3 T(DR_T), walk(dr_grid(nf * DR_SPLIT));
  if(gv)
  {
    ri_verts_face_kernel<<<walk, T, 0, st>>>(cam, snap, m->faces.get(), camera, attr, face, bary, gi, fsum, C, H, W, V, F, nf);
    HIP_TRY(hipGetLastError());
    if((rc = dr_gather(m, n, fsum, RI_ROW, 3, true, camera, gv, 3, 0, accumulate, st))) return rc;
  }
  for(int c0 = 0; ga && c0 < C; c0 += RI_CHUNK)
  {
    const int nc = std::min(RI_CHUNK, C - c0);
#define RI_WALK(NC) ri_attr_face_kernel<NC><<<walk, T, 0, st>>>(cam, snap, m->faces.get(), face, bary, gi + c0, fsum, C, H, W, V, F, nf)
    if(nc == 1) RI_WALK(1);
    else if(nc == 2) RI_WALK(2);
    else if(nc == 3) RI_WALK(3);
    else RI_WALK(4);
#undef RI_WALK
    HIP_TRY(hipGetLastError());
    if((rc = dr_gather(m, n, fsum, RI_ROW, nc, false, camera, ga, C, c0, accumulate, st))) return rc;
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
    ri_forward_kernel<<<dim3(dr_grid(total)), dim3(DR_T), 0, fr.st>>>(a, m->faces.get(), f, b, o, (int)C, (int)(H * W), (int)m->V,
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
  if(int rc = dr_check_near(fn, near)) return rc;
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = ri_check(fn, m, n, C, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "raster interpolate VJP");
  DepthRasterState * s = dr_state(m);
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
