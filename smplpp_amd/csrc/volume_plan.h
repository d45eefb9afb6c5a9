// The host plan of a signed-distance volume (smplpp_volume_create, scene.hip): what is refused, how many floats each storage
// layout takes, where node (i, j, k) of a point's cell lives in it, and which layout a handle uses.  Plain C++17, no HIP: a CPU test runs it
// as a stand-alone program (tests/cpp/volume_plan_dump.cpp).  The size and index functions are constexpr, so the kernels of scene.hip
// call the very same functions on the device.
//
// Node (i, j, k), i < Gx, j < Gy, k < Gz, holds values[(k Gy + j) Gx + i].  A cell (i, j, k), i < Gx-1, j < Gy-1, k < Gz-1, has the eight
// nodes (i + dx, j + dy, k + dz); its corner number is dx + 2 dy + 4 dz.
//   linear: the array as given.  The two x-neighbours of a corner pair are adjacent: a cell is four 8-byte reads.
//   cells:  one record of eight floats (32 bytes) per cell, in corner order, cells in the order of their first node: a cell is one
//           32-byte read, for 8 x the memory.  Available while the records fit VOL_CELLS_BYTES_MAX.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

namespace smplpp_hip
{
constexpr int64_t VOL_G_MIN = 2, VOL_G_MAX = 1024;
constexpr int64_t VOL_NODES_MAX = (int64_t)1 << 27;       // Gx Gy Gz: 512 MiB of floats as given
constexpr int64_t VOL_CELLS_BYTES_MAX = (int64_t)1 << 30; // the records of the cells layout: 1 GiB (a 256^3 grid takes 0.53 GB of them)
constexpr int VOL_LINEAR = 0, VOL_CELLS = 1;
constexpr int VOL_LAYOUT_DEFAULT = VOL_CELLS; // the faster of the two at body-fitting sizes (profiles/scene_bench.json)

// why a volume is refused, or null.  space: SMPLPP_HOST = 0 or SMPLPP_DEVICE = 1.  world_to_volume may be null (identity)
inline const char * volume_refusal(int64_t Gx, int64_t Gy, int64_t Gz, const float * origin, const float * spacing, const float * world_to_volume,
                                   int space, bool has_out)
{
  if(!has_out) return "no out";
  const int64_t G[3] = {Gx, Gy, Gz};
  for(int a = 0; a < 3; a++)
    if(G[a] < VOL_G_MIN || G[a] > VOL_G_MAX) return "Gx, Gy and Gz must be in [2, 1024]";
  if(Gx * Gy * Gz > VOL_NODES_MAX) return "Gx Gy Gz must not exceed 2^27";
  if(!origin || !spacing) return "origin or spacing is NULL";
  for(int a = 0; a < 3; a++)
    if(!(spacing[a] > 0.0f && std::isfinite(spacing[a]))) return "a spacing is not finite and positive";
  for(int a = 0; a < 3; a++)
    if(!std::isfinite(origin[a])) return "an origin entry is not finite";
  if(world_to_volume)
    for(int a = 0; a < 12; a++)
      if(!std::isfinite(world_to_volume[a])) return "a world_to_volume entry is not finite";
  if(space != 0 && space != 1) return "bad memory space";
  return nullptr;
}

constexpr int64_t volume_linear_floats(int64_t Gx, int64_t Gy, int64_t Gz)
{
  return Gx * Gy * Gz;
}
// node (i, j, k)
constexpr int64_t volume_linear_index(int64_t Gx, int64_t Gy, int64_t i, int64_t j, int64_t k)
{
  return (k * Gy + j) * Gx + i;
}
constexpr int64_t volume_cells_floats(int64_t Gx, int64_t Gy, int64_t Gz)
{
  return (Gx - 1) * (Gy - 1) * (Gz - 1) * 8;
}
// corner `corner` = dx + 2 dy + 4 dz of cell (i, j, k)
constexpr int64_t volume_cells_index(int64_t Gx, int64_t Gy, int64_t i, int64_t j, int64_t k, int corner)
{
  return ((k * (Gy - 1) + j) * (Gx - 1) + i) * 8 + corner;
}
constexpr bool volume_cells_available(int64_t Gx, int64_t Gy, int64_t Gz)
{
  return volume_cells_floats(Gx, Gy, Gz) * 4 <= VOL_CELLS_BYTES_MAX;
}
constexpr int64_t volume_floats(int layout, int64_t Gx, int64_t Gy, int64_t Gz)
{
  return layout == VOL_CELLS ? volume_cells_floats(Gx, Gy, Gz) : volume_linear_floats(Gx, Gy, Gz);
}

// The layout of a handle: `env` is the value of SMPLPP_VOLUME_LAYOUT (null or empty: the default).  "cells" above its bound is linear.
// An unknown value: -1.
inline int volume_layout(int64_t Gx, int64_t Gy, int64_t Gz, const char * env)
{
  int want = VOL_LAYOUT_DEFAULT;
  if(env && *env)
  {
    if(std::strcmp(env, "linear") == 0) want = VOL_LINEAR;
    else if(std::strcmp(env, "cells") == 0)
      want = VOL_CELLS;
    else
      return -1;
  }
  return want == VOL_CELLS && !volume_cells_available(Gx, Gy, Gz) ? VOL_LINEAR : want;
}
} // namespace smplpp_hip
