// The derivatives of mesh_device.h's normal queries (SMPL::calcNormal / calcVertexNormal, src/SMPL.cpp:518-535), used by
// the normals' backward pass (mesh_vjp.hip).  mesh_device.h's forward helpers are left as they are, so the forward kernels
// compile to the same code.
#pragma once

#include "mesh_device.h"

namespace smplpp_hip
{
// vector-Jacobian product of normalize3 (torch's normalize: x / max(|x|, 1e-12)) at x for the cotangent g.  Above the clamp
// this is (g - y (y . g)) / |x| with y = x / |x|; below it the denominator is the constant 1e-12 and the product is g / 1e-12,
// torch's gradient of that branch (finite, not NaN).
__device__ inline void normalize3_vjp(const float * x, const float * g, float * out)
{
  const float nrm = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if(nrm >= 1e-12f)
  {
    const float y[3] = {x[0] / nrm, x[1] / nrm, x[2] / nrm};
    const float d = y[0] * g[0] + y[1] * g[1] + y[2] * g[2];
    out[0] = (g[0] - y[0] * d) / nrm;
    out[1] = (g[1] - y[1] * d) / nrm;
    out[2] = (g[2] - y[2] * d) / nrm;
  }
  else
  {
    out[0] = g[0] / 1e-12f;
    out[1] = g[1] / 1e-12f;
    out[2] = g[2] / 1e-12f;
  }
}

// The weighted sum s and the weight 1/deg of vertex_normal_dev (the same operations, so the same bits), before normalisation.
__device__ inline void vertex_normal_sum_dev(const float * verts, const int32_t * faces, const int32_t * adjOff, const int32_t * adjFace,
                                             int vertex, float * acc, float & w)
{
  const int b = adjOff[vertex], e = adjOff[vertex + 1];
  float sum = 0.0f;
  for(int q = b; q < e; q++) sum += 1.0f;
  w = 1.0f / sum;
  acc[0] = acc[1] = acc[2] = 0.f;
  for(int q = b; q < e; q++)
  {
    float fn[3];
    face_normal_dev<true>(verts, faces, adjFace[q], fn);
    acc[0] += w * fn[0];
    acc[1] += w * fn[1];
    acc[2] += w * fn[2];
  }
}

// Cotangent of every unit face normal that enters vertex `vertex`'s weighted sum: (1/deg) N'(s)^T g_n.  Zero for a vertex
// without faces.
__device__ inline void vertex_normal_vjp_dev(const float * verts, const int32_t * faces, const int32_t * adjOff, const int32_t * adjFace,
                                             int vertex, const float * gn, float * G)
{
  if(adjOff[vertex + 1] <= adjOff[vertex])
  {
    G[0] = G[1] = G[2] = 0.f;
    return;
  }
  float s[3], w, gs[3];
  vertex_normal_sum_dev(verts, faces, adjOff, adjFace, vertex, s, w);
  normalize3_vjp(s, gn, gs);
  G[0] = w * gs[0];
  G[1] = w * gs[1];
  G[2] = w * gs[2];
}

// Corner cotangents of face_normal_pts for the cotangent gchat of the unit normal: c = a x b with a = v1 - v0, b = v2 - v0,
// g_c = N'(c)^T gchat, g_a = b x g_c, g_b = g_c x a; corner 1 gets g_a, corner 2 g_b, corner 0 -(g_a + g_b).
__device__ inline void face_normal_vjp_pts(const float * v0, const float * v1, const float * v2, const float * gchat, float * ga, float * gb)
{
  const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
  const float b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  float c[3], gc[3];
  cross3(a, b, c);
  normalize3_vjp(c, gchat, gc);
  cross3(b, gc, ga);
  cross3(gc, a, gb);
}
__device__ inline void face_normal_vjp_dev(const float * verts, const int32_t * faces, int face, const float * gchat, float * ga, float * gb)
{
  face_normal_vjp_pts(verts + 3 * faces[face * 3 + 0], verts + 3 * faces[face * 3 + 1], verts + 3 * faces[face * 3 + 2], gchat, ga, gb);
}
} // namespace smplpp_hip
