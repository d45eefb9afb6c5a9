// The pieces of the depth rasteriser's rule that other image-space terms restate: the camera row, the vertex
// projection with its refusal, the pixel-centre ray, the plane of a face in camera space and the 3-D barycentrics of a hit point.
// raster_walk.h builds the backward passes' shared walk on them.
// Every fp32 operation is rounded on its own (no contraction to FMA), as include/smplpp_hip.h states the rule.
#pragma once
#include "staging.h"

#include <cmath>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int DR_BAD = INT32_MIN;           // snapped x of a refused vertex
constexpr float DR_GUARD = 8388608.0f;      // guard band in snapped units (1/256 px): 32768 px; |edge function| < 2^51
constexpr int64_t DR_MAX_SIDE = 8192;       // largest H or W

struct DrCamera
{
  float R[9], t[3], fx, fy, cx, cy;
};
__device__ inline DrCamera dr_camera(const float * __restrict__ camera, int64_t frame)
{
  DrCamera c;
  const float * p = camera + frame * 16;
  for(int k = 0; k < 9; k++) c.R[k] = p[k];
  for(int k = 0; k < 3; k++) c.t[k] = p[9 + k];
  c.fx = p[12], c.fy = p[13], c.cx = p[14], c.cy = p[15];
  return c;
}

// camera-space position of a world-space vertex
__device__ inline void dr_to_camera(const DrCamera & c, float x, float y, float z, float * xc)
{
  for(int k = 0; k < 3; k++) xc[k] = ((c.R[3 * k] * x + c.R[3 * k + 1] * y) + c.R[3 * k + 2] * z) + c.t[k];
}

// the vertex rule: camera-space position, the unsnapped projection (u, v), the snapped one (su, sv); false for a refused vertex
__device__ inline bool dr_project(const DrCamera & c, float x, float y, float z, float near, float * xc, float & u, float & v, float & su,
                                  float & sv)
{
  dr_to_camera(c, x, y, z, xc);
  u = (c.fx * xc[0]) / xc[2] + c.cx;
  v = (c.fy * xc[1]) / xc[2] + c.cy;
  su = rintf(u * 256.0f), sv = rintf(v * 256.0f);
  return fabsf(xc[0]) < INFINITY && fabsf(xc[1]) < INFINITY && fabsf(xc[2]) < INFINITY && xc[2] > near && fabsf(su) <= DR_GUARD &&
         fabsf(sv) <= DR_GUARD; // (a NaN fails every comparison)
}

// one (frame, face) ready to be walked: snapped corners, the clipped box, the plane
struct DrFace
{
  int64_t x[3], y[3];
  int sgn;
  int i0, i1, j0, j1;
  float ax, ay, az, nx, ny, nz, na;
  float e1[3], e2[3];
};

// the plane members of t (a, e1, e2, n, na) from the camera-space corners
__device__ inline void dr_plane(DrFace & t, const float * a, const float * b, const float * c)
{
  t.ax = a[0], t.ay = a[1], t.az = a[2];
  t.e1[0] = b[0] - a[0], t.e1[1] = b[1] - a[1], t.e1[2] = b[2] - a[2];
  t.e2[0] = c[0] - a[0], t.e2[1] = c[1] - a[1], t.e2[2] = c[2] - a[2];
  t.nx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
  t.ny = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
  t.nz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
  t.na = (t.nx * t.ax + t.ny * t.ay) + t.nz * t.az;
}

__host__ __device__ inline int64_t dr_min(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t dr_max(int64_t a, int64_t b) { return a > b ? a : b; }

// a (frame, face) made ready from the vertex pass (cam, snap): its status, and on DR_FACE_OK the snapped corners, the clipped box and the plane
enum
{
  DR_FACE_OK = 0,
  DR_FACE_SKIPPED = 1, // a refused corner
  DR_FACE_EMPTY = 2    // zero snapped area, or a box that holds no pixel centre of the image
};
__device__ inline int dr_face_setup(DrFace & t, const float4 * __restrict__ cam, const int2 * __restrict__ snap,
                                    const int32_t * __restrict__ faces, int64_t frame, int64_t f, int64_t V, int64_t H, int64_t W)
{
  int32_t c[3];
  int2 s[3];
  for(int k = 0; k < 3; k++)
  {
    c[k] = faces[f * 3 + k];
    s[k] = snap[frame * V + c[k]];
  }
  if(s[0].x == DR_BAD || s[1].x == DR_BAD || s[2].x == DR_BAD) return DR_FACE_SKIPPED;
  for(int k = 0; k < 3; k++) t.x[k] = s[k].x, t.y[k] = s[k].y;
  const int64_t A2 = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
  if(A2 == 0) return DR_FACE_EMPTY;
  t.sgn = A2 > 0 ? 1 : -1;
  const int64_t xmin = dr_min(t.x[0], dr_min(t.x[1], t.x[2])), xmax = dr_max(t.x[0], dr_max(t.x[1], t.x[2]));
  const int64_t ymin = dr_min(t.y[0], dr_min(t.y[1], t.y[2])), ymax = dr_max(t.y[0], dr_max(t.y[1], t.y[2]));
  // pixel centres 256 i + 128 inside [min, max]
  t.i0 = (int)dr_max(0, (xmin + 127) >> 8), t.i1 = (int)dr_min(W - 1, (xmax - 128) >> 8);
  t.j0 = (int)dr_max(0, (ymin + 127) >> 8), t.j1 = (int)dr_min(H - 1, (ymax - 128) >> 8);
  if(t.i0 > t.i1 || t.j0 > t.j1) return DR_FACE_EMPTY;
  const float4 a = cam[frame * V + c[0]], b = cam[frame * V + c[1]], cc = cam[frame * V + c[2]];
  dr_plane(t, &a.x, &b.x, &cc.x);
  return DR_FACE_OK;
}

// the pixel-centre ray's x and y (z = 1)
__device__ inline void dr_ray(const DrCamera & c, int i, int j, float & dx, float & dy)
{
  dx = (((float)i + 0.5f) - c.cx) / c.fx;
  dy = (((float)j + 0.5f) - c.cy) / c.fy;
}

// barycentrics of p = depth * d in (a, a + e1, a + e2) with normal n
__device__ inline void dr_bary(const DrFace & t, float depth, float dx, float dy, float & ba, float & bb, float & bc)
{
  const float wx = depth * dx - t.ax, wy = depth * dy - t.ay, wz = depth - t.az;
  const float nn = (t.nx * t.nx + t.ny * t.ny) + t.nz * t.nz;
  const float px = wy * t.e2[2] - wz * t.e2[1], py = wz * t.e2[0] - wx * t.e2[2], pz = wx * t.e2[1] - wy * t.e2[0]; // w x e2
  const float qx = t.e1[1] * wz - t.e1[2] * wy, qy = t.e1[2] * wx - t.e1[0] * wz, qz = t.e1[0] * wy - t.e1[1] * wx; // e1 x w
  bb = ((px * t.nx + py * t.ny) + pz * t.nz) / nn;
  bc = ((qx * t.nx + qy * t.ny) + qz * t.nz) / nn;
  ba = (1.0f - bb) - bc;
}

// the call rules every image-space entry shares; dr_check_near for the entries that take a near plane
inline int dr_check_near(const char * fn, float near)
{
  if(!(std::isfinite(near) && near > 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": near must be finite and > 0");
  return SMPLPP_OK;
}
inline int dr_check(const char * fn, smplpp_model * m, int64_t n, int64_t H, int64_t W, int space)
{
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": the model has no faces");
  if(H < 1 || W < 1 || H > DR_MAX_SIDE || W > DR_MAX_SIDE) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": H and W must be in [1, 8192]");
  // every [n,H,W], [n,V] and [n,F] index stays in int32 (and the 8 lanes per face of the backward walk in its grid)
  if(n > 0x7fffffffLL || n * H * W > 0x7fffffffLL || n * m->V > 0x7fffffffLL || n * m->F > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * H * W, n * V or n * F beyond int32 indexing");
  return check_space(space, fn);
}
} // namespace smplpp_hip
