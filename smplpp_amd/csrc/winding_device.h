// The generalized winding number's per-face term, shared by the sweep grid (winding_kernel, mesh.hip) and the
// batched point query (winding.hip), so that both give the same bits at the same fp32 position by construction:
//   w(p) = sum_f Omega_f(p) / (4 pi), Omega_f = 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
// with a, b, c = the face's vertices minus p (igl::winding_number as called at node/node.cpp:1052).  fp32 terms summed in ascending
// face order within a chunk of 256 faces, the chunks' fp32 partials summed in fp64 in ascending chunk order from 0.0, then (float)(acc / (2 pi)).
#pragma once
#include <hip/hip_runtime.h>

namespace smplpp_hip
{
// one face's term atan2(det, den) at (px, py, pz); t = the face's a, b, c
__device__ __forceinline__ float winding_term(const float * t, float px, float py, float pz)
{
  const float ax = t[0] - px, ay = t[1] - py, az = t[2] - pz;
  const float bx = t[3] - px, by = t[4] - py, bz = t[5] - pz;
  const float cx = t[6] - px, cy = t[7] - py, cz = t[8] - pz;
  const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  const float den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb;
  return atan2f(det, den);
}
} // namespace smplpp_hip
