// Runs the plan of smplpp_amd/csrc/volume_plan.h on a description file and writes what it decides (tests/test_scene_cpu.py builds it with
// the address and undefined-behaviour sanitizers).  Host code only.
//   in : int64 Gx, Gy, Gz, space, has out, has origin and spacing, has transform, env (0: unset, 1: "linear", 2: "cells", 3: "bricks",
//        4: "") | float origin[3], spacing[3], world_to_volume[12]
//   out: records { char name[16]; int64 element size, count; the elements }.  A refusal is the file's only record, "refusal".  Else
//        "dims" = layout, linear floats, cells floats, cells available; and for grids of at most 4096 nodes "linear_index" (the index of
//        every node in k, j, i order) and "cells_index" (of every corner of every cell in k, j, i, corner order).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../smplpp_amd/csrc/volume_plan.h"

using namespace smplpp_hip;

static FILE * g_out;

template<class T>
static void put(const char * name, const T * data, size_t count)
{
  char nm[16] = {};
  strncpy(nm, name, 15);
  const int64_t es = sizeof(T), n = (int64_t)count;
  fwrite(nm, 1, 16, g_out);
  fwrite(&es, 8, 1, g_out);
  fwrite(&n, 8, 1, g_out);
  if(count) fwrite(data, sizeof(T), count, g_out);
}

int main(int argc, char ** argv)
{
  if(argc != 3)
  {
    fprintf(stderr, "usage: volume_plan_dump DESCRIPTION PLAN\n");
    return 2;
  }
  FILE * f = fopen(argv[1], "rb");
  if(!f) return 2;
  int64_t hdr[8];
  float fl[18];
  if(fread(hdr, 8, 8, f) != 8 || fread(fl, 4, 18, f) != 18)
  {
    fprintf(stderr, "volume_plan_dump: short read\n");
    return 2;
  }
  fclose(f);
  g_out = fopen(argv[2], "wb");
  if(!g_out) return 2;
  const int64_t Gx = hdr[0], Gy = hdr[1], Gz = hdr[2];
  static const char * envs[5] = {nullptr, "linear", "cells", "bricks", ""};
  const char * why = volume_refusal(Gx, Gy, Gz, hdr[5] ? fl : nullptr, hdr[5] ? fl + 3 : nullptr, hdr[6] ? fl + 6 : nullptr, (int)hdr[3], hdr[4] != 0);
  const int layout = why ? 0 : volume_layout(Gx, Gy, Gz, envs[hdr[7]]);
  if(!why && layout < 0) why = "SMPLPP_VOLUME_LAYOUT must be linear or cells";
  if(why) put("refusal", why, strlen(why));
  else
  {
    const int64_t dims[4] = {layout, volume_linear_floats(Gx, Gy, Gz), volume_cells_floats(Gx, Gy, Gz), volume_cells_available(Gx, Gy, Gz) ? 1 : 0};
    put("dims", dims, 4);
    if(dims[1] != volume_floats(VOL_LINEAR, Gx, Gy, Gz) || dims[2] != volume_floats(VOL_CELLS, Gx, Gy, Gz)) return 3;
    if(Gx * Gy * Gz <= 4096)
    {
      std::vector<int64_t> lin, cel;
      for(int64_t k = 0; k < Gz; k++)
        for(int64_t j = 0; j < Gy; j++)
          for(int64_t i = 0; i < Gx; i++) lin.push_back(volume_linear_index(Gx, Gy, i, j, k));
      for(int64_t k = 0; k + 1 < Gz; k++)
        for(int64_t j = 0; j + 1 < Gy; j++)
          for(int64_t i = 0; i + 1 < Gx; i++)
            for(int c = 0; c < 8; c++) cel.push_back(volume_cells_index(Gx, Gy, i, j, k, c));
      put("linear_index", lin.data(), lin.size());
      put("cells_index", cel.data(), cel.size());
    }
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
