// The one device copy of the normal-compatibility rule of smplpp_point_mesh_distance_compatible and
// smplpp_mesh_point_distance_compatible (include/smplpp_hip.h states it; the tests restate it in numpy float32).
// Every operation is rounded on its own: no contraction to FMA anywhere in this header.
#pragma once
#include "common.h"

namespace smplpp_hip
{
// the filter's arguments: cos_min in [0, 1]; max_sqdist >= 0, +inf allowed; a NaN fails either comparison
inline int compat_args(const char * fn, float cos_min, float max_sqdist)
{
  if(!(cos_min >= 0.0f && cos_min <= 1.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": cos_min must lie in [0, 1]");
  if(!(max_sqdist >= 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": max_sqdist must be >= 0 (+inf: no cap)");
  return SMPLPP_OK;
}

// (x x' + y y') + z z'
__device__ inline float compat_dot(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}

// m = (b - a) x (c - a), each component (e1y e2z) - (e1z e2y) and so on; .w = mm = (m.x m.x + m.y m.y) + m.z m.z
__device__ inline float4 compat_face_normal(float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2)
{
#pragma clang fp contract(off)
  const float e1x = b0 - a0, e1y = b1 - a1, e1z = b2 - a2;
  const float e2x = c0 - a0, e2y = c1 - a1, e2z = c2 - a2;
  const float mx = (e1y * e2z) - (e1z * e2y);
  const float my = (e1z * e2x) - (e1x * e2z);
  const float mz = (e1x * e2y) - (e1y * e2x);
  return make_float4(mx, my, mz, (mx * mx + my * my) + mz * mz);
}

// m, q: the two normals with their squared lengths in .w; c2 = cos_min * cos_min (rounded once, on the host).
// A NaN anywhere fails a comparison, so the pair is incompatible; a zero normal has mm qq = 0.
__device__ inline bool compat_normals(const float4 & m, const float4 & q, float c2)
{
#pragma clang fp contract(off)
  const float s = (m.x * q.x + m.y * q.y) + m.z * q.z;
  const float l = m.w * q.w;
  return s >= 0.0f && l > 0.0f && s * s >= c2 * l;
}

__device__ inline bool compat_finite3(float x, float y, float z)
{
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}
} // namespace smplpp_hip
