// Depth rasteriser: each frame's posed mesh through a pinhole camera into a face-id + depth image, with vertex visibility, and the
// vector-Jacobian product of the depth image to the vertices.  The rule is in include/smplpp_hip.h; every fp32
// operation below is rounded on its own (no contraction to FMA), and coverage is decided in integers, so a numpy restatement
// reproduces every bit.
//
// Forward:
//  dr_vertex_kernel   per (frame, vertex): camera-space position (float4, w unused) and the snapped projection (int2; x = DR_BAD
//                     for a vertex the rule refuses).
//  dr_face_kernel     per (frame, face): skipped faces counted (integer atomics), the snapped bounding box clipped to the image; a
//                     box of at most `inline` pixels is walked by the face's own thread, a larger one is queued (an integer
//                     atomic takes the slot; the order of the queue cannot matter, see below).
//  dr_large_kernel    a fixed grid of wavefronts takes the queued faces in turn, 64 lanes striding one box: no lane ever owns a
//                     large face's whole box.
//                     Both apply the integer edge functions at the pixel centre, the ray-plane depth, and a 64-bit unsigned
//                     minimum on the pixel's key, depth bits << 32 | face id (depths are positive, so their bits order like their
//                     values): a minimum over a set does not depend on the order the set is met in.  A plain load of the key
//                     first skips the atomic for a candidate that has already lost (keys only fall).
//  dr_resolve_kernel  per pixel: key -> face, depth, the 3-D barycentrics of the hit point, and a plain byte store of 1 into
//                     `visible` for the three corners (every writer stores the same value).
// Backward (the face image is an input and held fixed):
//  dr_vjp_face_kernel   the walk of raster_walk.h (DR_SPLIT lanes per (frame, face), a fixed xor tree): a pixel that names the face
//                       and has a nonzero cotangent adds beta_i * (g / (n.d)) to corner i's sum; lane 0 stores n times each.
//  dr_gather_kernel     per (frame, vertex): its faces' values in ascending face id (the adjacency of the normals' backward pass),
//                       then R^T once (ROT) or the plain store.  One fixed-order sum per element, no floating-point atomics.
// dr_vertex_kernel and dr_gather_kernel also serve raster_interpolate.hip, through dr_vertex_pass and dr_gather of raster_walk.h,
// with the handle's one DepthRasterState.
#include "raster_walk.h"
#include "trace.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int DR_INLINE_DEFAULT = 16;       // box pixels a face's own thread walks (SMPLPP_DEPTH_RASTER_INLINE)
constexpr int DR_INLINE_MAX = 4096;
constexpr unsigned DR_LARGE_BLOCKS = 2048;  // grid of dr_large_kernel: 8192 wavefronts
constexpr unsigned long long DR_EMPTY = ~0ull;

void StateDelete::operator()(DepthRasterState * s) const
{
  delete s;
}

__global__ __launch_bounds__(DR_T) void dr_vertex_kernel(const float * __restrict__ verts, const float * __restrict__ camera,
                                                         float4 * __restrict__ cam, int2 * __restrict__ snap, float near, int64_t V,
                                                         int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * DR_T + threadIdx.x;
  if(idx >= nv) return;
  const DrCamera c = dr_camera(camera, idx / V);
  float xc[3], u, v, su, sv;
  const bool ok = dr_project(c, verts[idx * 3], verts[idx * 3 + 1], verts[idx * 3 + 2], near, xc, u, v, su, sv);
  cam[idx] = make_float4(xc[0], xc[1], xc[2], 0.0f);
  snap[idx] = ok ? make_int2((int)su, (int)sv) : make_int2(DR_BAD, DR_BAD);
}

// coverage of pixel (row j, column i) by the face, its depth, the depth test
__device__ inline void dr_pixel(const DrFace & t, const DrCamera & c, float near, int i, int j, unsigned f,
                                unsigned long long * __restrict__ keys, int64_t W)
{
  const int64_t px = 256 * (int64_t)i + 128, py = 256 * (int64_t)j + 128;
#pragma unroll
  for(int e = 0; e < 3; e++)
  {
    const int p = (e + 1) % 3, q = (e + 2) % 3;
    const int64_t ex = t.sgn * (t.x[q] - t.x[p]), ey = t.sgn * (t.y[q] - t.y[p]);
    const int64_t E = ex * (py - t.y[p]) - ey * (px - t.x[p]);
    if(!(E > 0 || (E == 0 && (ey < 0 || (ey == 0 && ex > 0))))) return;
  }
  float dx, dy;
  dr_ray(c, i, j, dx, dy);
  const float nd = (t.nx * dx + t.ny * dy) + t.nz;
  const float depth = t.na / nd;
  if(!(depth > near && depth < INFINITY)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | f;
  unsigned long long * k = keys + (int64_t)j * W + i;
  if(key < __atomic_load_n(k, __ATOMIC_RELAXED)) atomicMin(k, key);
}

__global__ __launch_bounds__(DR_T) void dr_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                       const int32_t * __restrict__ faces, const float * __restrict__ camera,
                                                       unsigned long long * __restrict__ keys, int32_t * __restrict__ queue,
                                                       int32_t * __restrict__ qn, unsigned long long * __restrict__ culled, float near,
                                                       int64_t H, int64_t W, int64_t V, int64_t F, int64_t nf, int inline_px)
{
  const int64_t idx = (int64_t)blockIdx.x * DR_T + threadIdx.x;
  if(idx >= nf) return;
  const int64_t frame = idx / F, f = idx % F;
  DrFace t;
  const int rc = dr_face_setup(t, cam, snap, faces, frame, f, V, H, W);
  if(rc == DR_FACE_SKIPPED && culled) atomicAdd(culled + frame, 1ull);
  if(rc != DR_FACE_OK) return;
  const int w = t.i1 - t.i0 + 1, h = t.j1 - t.j0 + 1;
  if((int64_t)w * h > inline_px)
  {
    queue[atomicAdd(qn, 1)] = (int32_t)idx;
    return;
  }
  const DrCamera c = dr_camera(camera, frame);
  unsigned long long * kf = keys + frame * H * W;
  for(int j = t.j0; j <= t.j1; j++)
    for(int i = t.i0; i <= t.i1; i++) dr_pixel(t, c, near, i, j, (unsigned)f, kf, W);
}

__global__ __launch_bounds__(DR_T) void dr_large_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                        const int32_t * __restrict__ faces, const float * __restrict__ camera,
                                                        unsigned long long * __restrict__ keys, const int32_t * __restrict__ queue,
                                                        const int32_t * __restrict__ qn, float near, int64_t H, int64_t W, int64_t V,
                                                        int64_t F)
{
  const int lane = threadIdx.x & 63;
  const int count = *qn;
  const int waves = (int)gridDim.x * (DR_T / 64);
  for(int e = (int)blockIdx.x * (DR_T / 64) + (int)(threadIdx.x >> 6); e < count; e += waves)
  {
    const int64_t idx = queue[e], frame = idx / F, f = idx % F;
    DrFace t;
    if(dr_face_setup(t, cam, snap, faces, frame, f, V, H, W) != DR_FACE_OK) continue; // (queued faces are OK)
    const DrCamera c = dr_camera(camera, frame);
    unsigned long long * kf = keys + frame * H * W;
    const int w = t.i1 - t.i0 + 1;
    const int64_t area = (int64_t)w * (t.j1 - t.j0 + 1);
    for(int64_t r = lane; r < area; r += 64) dr_pixel(t, c, near, t.i0 + (int)(r % w), t.j0 + (int)(r / w), (unsigned)f, kf, W);
  }
}

__global__ __launch_bounds__(DR_T) void dr_resolve_kernel(const float4 * __restrict__ cam, const int32_t * __restrict__ faces,
                                                          const float * __restrict__ camera,
                                                          const unsigned long long * __restrict__ keys, int64_t * __restrict__ face,
                                                          float * __restrict__ depth, float * __restrict__ bary,
                                                          uint8_t * __restrict__ visible, int64_t H, int64_t W, int64_t V, int64_t np)
{
  const int64_t idx = (int64_t)blockIdx.x * DR_T + threadIdx.x;
  if(idx >= np) return;
  const unsigned long long key = keys[idx];
  if(key == DR_EMPTY)
  {
    face[idx] = -1;
    depth[idx] = 0.0f;
    if(bary) bary[idx * 3] = 0.0f, bary[idx * 3 + 1] = 0.0f, bary[idx * 3 + 2] = 0.0f;
    return;
  }
  const int64_t frame = idx / (H * W), pix = idx % (H * W);
  const int64_t f = (int64_t)(key & 0xffffffffull);
  const float z = __uint_as_float((unsigned)(key >> 32));
  face[idx] = f;
  depth[idx] = z;
  const int32_t c0 = faces[f * 3], c1 = faces[f * 3 + 1], c2 = faces[f * 3 + 2];
  if(visible) visible[frame * V + c0] = 1, visible[frame * V + c1] = 1, visible[frame * V + c2] = 1;
  if(!bary) return;
  const DrCamera c = dr_camera(camera, frame);
  const float4 a = cam[frame * V + c0], b = cam[frame * V + c1], cc = cam[frame * V + c2];
  DrFace t;
  dr_plane(t, &a.x, &b.x, &cc.x);
  float dx, dy, ba, bb, bc;
  dr_ray(c, (int)(pix % W), (int)(pix / W), dx, dy);
  dr_bary(t, z, dx, dy, ba, bb, bc);
  bary[idx * 3] = ba, bary[idx * 3 + 1] = bb, bary[idx * 3 + 2] = bc;
}

// the depth term's share of a pixel: beta_i * (g / (n.d)) to corner i
struct DrDepthBody
{
  const float * camera, * gd;
  int64_t HW;
  DrCamera c;
  const float * gf;
  __device__ void face(const DrFace &, int64_t frame, int64_t)
  {
    c = dr_camera(camera, frame);
    gf = gd + frame * HW;
  }
  __device__ void pixel(const DrFace & t, int i, int j, int64_t pix, float * s) const
  {
    const float g = gf[pix];
    if(g == 0.0f) return;
    float dx, dy, b[3];
    dr_ray(c, i, j, dx, dy);
    const float nd = (t.nx * dx + t.ny * dy) + t.nz;
    const float depth = t.na / nd;
    dr_bary(t, depth, dx, dy, b[0], b[1], b[2]);
    const float coef = g / nd;
    for(int k = 0; k < 3; k++) s[k] = s[k] + b[k] * coef;
  }
};

__global__ __launch_bounds__(DR_T) void dr_vjp_face_kernel(const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                                           const int32_t * __restrict__ faces, const float * __restrict__ camera,
                                                           const int64_t * __restrict__ face, const float * __restrict__ gd,
                                                           float * __restrict__ fsum, int64_t H, int64_t W, int64_t V, int64_t F,
                                                           int64_t nf)
{
  float s[3];
  DrDepthBody body{camera, gd, H * W};
  const DrWalk w = dr_walk(cam, snap, faces, face, H, W, V, F, nf, s, body);
  if(!w.in || w.part != 0) return;
  float * o = fsum + w.idx * 9;
  for(int k = 0; k < 3; k++)
  {
    o[3 * k] = w.live ? s[k] * w.t.nx : 0.0f;
    o[3 * k + 1] = w.live ? s[k] * w.t.ny : 0.0f;
    o[3 * k + 2] = w.live ? s[k] * w.t.nz : 0.0f;
  }
}

// see dr_gather (raster_walk.h); instantiated on the width, so that a corner's values come in one load
template<int WIDTH, bool ROT>
__global__ __launch_bounds__(DR_T) void dr_gather_kernel(const float * __restrict__ fsum, const int32_t * __restrict__ faces,
                                                         const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
                                                         const float * __restrict__ camera, float * __restrict__ out, int row,
                                                         int stride, int off, int accumulate, int64_t V, int64_t F, int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * DR_T + threadIdx.x;
  if(idx >= nv) return;
  const int64_t frame = idx / V;
  const int32_t v = (int32_t)(idx % V);
  float g[WIDTH];
  for(int x = 0; x < WIDTH; x++) g[x] = 0.0f;
  for(int32_t q = adjOff[v]; q < adjOff[v + 1]; q++)
  {
    const int64_t f = adjFace[q];
    for(int k = 0; k < 3; k++)
      if(faces[f * 3 + k] == v)
      {
        const float * p = fsum + (frame * F + f) * row + k * WIDTH;
        for(int x = 0; x < WIDTH; x++) g[x] = g[x] + p[x];
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
  for(int x = 0; x < WIDTH; x++) o[x] = accumulate ? o[x] + g[x] : g[x];
}

DepthRasterState * dr_state(smplpp_model * m)
{
  if(!m->dr)
  {
    m->dr.reset(new DepthRasterState());
    m->dr->inline_px = m->dr_inline < 0 ? DR_INLINE_DEFAULT : m->dr_inline > DR_INLINE_MAX ? DR_INLINE_MAX : m->dr_inline;
  }
  return m->dr.get();
}

int dr_vertex_pass(smplpp_model * m, DepthRasterState * s, int64_t n, const float * verts, const float * camera, float near, hipStream_t st)
{
  const int64_t nv = n * m->V;
  HIP_TRY(s->cam.reserve(sizeof(float4) * (size_t)nv));
  HIP_TRY(s->snap.reserve(sizeof(int2) * (size_t)nv));
  dr_vertex_kernel<<<dim3(dr_grid(nv)), dim3(DR_T), 0, st>>>(verts, camera, s->cam.as<float4>(), s->snap.as<int2>(), near, m->V, nv);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

int dr_gather(smplpp_model * m, int64_t n, const float * fsum, int row, int width, bool rot, const float * camera, float * out,
              int stride, int off, int accumulate, hipStream_t st)
{
  const int64_t nv = n * m->V;
#define DR_GATHER(WIDTH, ROT)                                                                                                         \
  dr_gather_kernel<WIDTH, ROT><<<dim3(dr_grid(nv)), dim3(DR_T), 0, st>>>(fsum, m->faces.get(), m->adjOff.get(), m->adjFace.get(), camera, \
                                                                         out, row, stride, off, accumulate, m->V, m->F, nv)
  if(rot) DR_GATHER(3, true);
  else if(width == 1) DR_GATHER(1, false);
  else if(width == 2) DR_GATHER(2, false);
  else if(width == 3) DR_GATHER(3, false);
  else DR_GATHER(4, false);
#undef DR_GATHER
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// all pointers on the device
static int dr_forward_device(smplpp_model * m, DepthRasterState * s, int64_t n, const float * verts, const float * camera, int64_t H,
                             int64_t W, float near, int64_t * face, float * depth, float * bary, uint8_t * visible, int64_t * culled,
                             hipStream_t st)
{
  const int64_t V = m->V, F = m->F, nf = n * F, np = n * H * W;
  int rc = dr_vertex_pass(m, s, n, verts, camera, near, st);
  if(rc) return rc;
  HIP_TRY(s->keys.reserve(sizeof(unsigned long long) * (size_t)np));
  HIP_TRY(s->queue.reserve(sizeof(int32_t) * (size_t)nf));
  HIP_TRY(s->qn.reserve(sizeof(int32_t)));
  unsigned long long * keys = s->keys.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)np, st));
  HIP_TRY(hipMemsetAsync(s->qn.as<int32_t>(), 0, sizeof(int32_t), st));
  if(culled) HIP_TRY(hipMemsetAsync(culled, 0, sizeof(int64_t) * (size_t)n, st));
  if(visible) HIP_TRY(hipMemsetAsync(visible, 0, (size_t)(n * V), st));
  dr_face_kernel<<<dim3(dr_grid(nf)), dim3(DR_T), 0, st>>>(s->cam.as<float4>(), s->snap.as<int2>(), m->faces.get(), camera, keys,
                                                           s->queue.as<int32_t>(), s->qn.as<int32_t>(),
                                                           reinterpret_cast<unsigned long long *>(culled), near, H, W, V, F, nf,
                                                           s->inline_px);
  HIP_TRY(hipGetLastError());
  const unsigned blocks = (unsigned)std::min<int64_t>(DR_LARGE_BLOCKS, (nf + DR_T / 64 - 1) / (DR_T / 64));
  dr_large_kernel<<<dim3(blocks), dim3(DR_T), 0, st>>>(s->cam.as<float4>(), s->snap.as<int2>(), m->faces.get(), camera, keys,
                                                       s->queue.as<int32_t>(), s->qn.as<int32_t>(), near, H, W, V, F);
  HIP_TRY(hipGetLastError());
  dr_resolve_kernel<<<dim3(dr_grid(np)), dim3(DR_T), 0, st>>>(s->cam.as<float4>(), m->faces.get(), camera, keys, face, depth, bary,
                                                              visible, H, W, V, np);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int dr_vjp_device(smplpp_model * m, DepthRasterState * s, int64_t n, const float * verts, const float * camera, int64_t H,
                         int64_t W, const int64_t * face, const float * gd, float * gv, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, F = m->F, nf = n * F;
  // no near plane here: the face image names the faces; a vertex is refused for a non-finite or out-of-band projection only
  int rc = dr_vertex_pass(m, s, n, verts, camera, -INFINITY, st);
  if(rc) return rc;
  HIP_TRY(s->fsum.reserve(sizeof(float) * 9 * (size_t)nf));
  dr_vjp_face_kernel<<<dim3(dr_grid(nf * DR_SPLIT)), dim3(DR_T), 0, st>>>(s->cam.as<float4>(), s->snap.as<int2>(), m->faces.get(), camera,
                                                                          face, gd, s->fsum.as<float>(), H, W, V, F, nf);
  HIP_TRY(hipGetLastError());
  return dr_gather(m, n, s->fsum.as<float>(), 9, 3, true, camera, gv, 3, 0, accumulate, st);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_depth_raster(smplpp_model * m, int64_t n, const float * verts, const float * camera, int64_t H, int64_t W,
                                   float near, int64_t * face, float * depth, float * bary, uint8_t * visible, int64_t * culled,
                                   int space, void * stream)
{
  const char * fn = "smplpp_depth_raster";
  if(!m || n <= 0 || !verts || !camera || !face || !depth) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(int rc = dr_check_near(fn, near)) return rc;
  int rc = dr_check(fn, m, n, H, W, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "depth raster");
  DepthRasterState * s = dr_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  int64_t * fo = fr.out(face, (size_t)(n * H * W));
  float * zo = fr.out(depth, (size_t)(n * H * W));
  float * bo = fr.out(bary, (size_t)(n * H * W * 3));
  uint8_t * vo = fr.out(visible, (size_t)(n * m->V));
  int64_t * co = fr.out(culled, (size_t)n);
  return fr.run([&] { return dr_forward_device(m, s, n, v, c, H, W, near, fo, zo, bo, vo, co, fr.st); });
}

extern "C" int smplpp_depth_raster_vjp(smplpp_model * m, int64_t n, const float * verts, const float * camera, int64_t H, int64_t W,
                                       const int64_t * face, const float * grad_depth, float * grad_verts, int accumulate, int space,
                                       void * stream)
{
  const char * fn = "smplpp_depth_raster_vjp";
  if(!m || n <= 0 || !verts || !camera || !face || !grad_depth || !grad_verts)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = dr_check(fn, m, n, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "depth raster VJP");
  DepthRasterState * s = dr_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const int64_t * f = fr.in(face, (size_t)(n * H * W));
  const float * g = fr.in(grad_depth, (size_t)(n * H * W));
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  return fr.run([&] { return dr_vjp_device(m, s, n, v, c, H, W, f, g, gv, accumulate, fr.st); });
}
