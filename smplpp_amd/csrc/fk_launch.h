// The batch loop of the fused kernels' launchers (skin_e.hip, skin_h.hip, skin_b.hip): a long batch goes in launches of
// skin_batch_frames (fk_plan.h) frames, and each launch sees the workspace and the caller's arrays from its first frame on.
#pragma once

#include "common.h"
#include "fk_plan.h"

namespace smplpp_hip
{
// one launch: frames [f_off, f_off + n) of the batch, f_off a multiple of 64
struct SkinBatch
{
  int64_t n, f_off;
  const float * theta;
  float * verts, * rest;
  // a workspace array of whole 64-frame tiles (bytes_per_tile each), from this launch's first tile on
  template<class T>
  const T * tiles(const DevBuf & buf, int64_t bytes_per_tile) const
  {
    return reinterpret_cast<const T *>(buf.as<uint8_t>() + (f_off / 64) * bytes_per_tile);
  }
};

// launch(SkinBatch) for every launch of the batch; g_tile_bytes: the form's relative transforms of one frame tile
template<class F>
hipError_t for_each_skin_batch(int64_t V, int64_t n, int64_t g_tile_bytes, const float * theta, float * verts, float * rest, F && launch)
{
  const int64_t per = skin_batch_frames(V, g_tile_bytes);
  if(per < 64) return hipErrorInvalidValue;
  for(int64_t off = 0; off < n; off += per)
  {
    const SkinBatch b{(n - off < per) ? n - off : per, off, theta + off * ((NJ + 1) * 3), verts ? verts + off * V * 3 : nullptr,
                      rest ? rest + off * V * 3 : nullptr};
    hipError_t e = launch(b);
    if(e != hipSuccess) return e;
  }
  return hipSuccess;
}
} // namespace smplpp_hip
