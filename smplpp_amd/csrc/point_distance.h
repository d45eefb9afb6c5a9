// The point-to-mesh distance's workspace and device paths (point_distance.hip), for the signed distance (winding.hip) that builds on
// them with a workspace of its own.
#pragma once
#include "distance_vjp.h"

namespace smplpp_hip
{
struct PointDistState
{
  DevBuf tri;          // [n][F][3] float4 triangle image of the tiled form
  DevBuf perm;         // [n][K] int32 query order of the tiled form
  DevBuf rec;          // [n][K] PdRecord of the backward pass
  DevBuf seedv;        // [nseed] int32 vertices that have a face (model constant, set up by the first call)
  int64_t nseed = -1;
};
// smplpp_point_mesh_distance's forward and smplpp_point_mesh_distance_vjp's product, all pointers on the device
int pd_forward_device(smplpp_model * m, PointDistState * s, int64_t n, const float * verts, int64_t K, const float * points, int64_t * face,
                      float * weights, float * closest, float * sqdist, hipStream_t st);
int pd_vjp_device(smplpp_model * m, PointDistState * s, int64_t n, const float * verts, int64_t K, const float * points, const int64_t * face,
                  const float * gsq, float * gv, float * gp, int accumulate, hipStream_t st);
} // namespace smplpp_hip
