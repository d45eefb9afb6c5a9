// The host decisions of a grouped L-BFGS handle (smplpp_amd/csrc/lbfgs_wide_plan.h) as a stand-alone program; driven by
// tests/test_lbfgs_groups_cpu.py, which builds it with the address and undefined-behaviour sanitizers and compares every answer with a
// Python restatement.
// usage: lbfgs_wide_plan_dump <queries.txt> <answers.txt>; one answer line per query line:
//   groups n D m P r_0 .. r_P  -> the refusal (of the shape, then of the groups), or "ok grid threads lds_vector lds_bytes ints floats sy vec
//                                 hist rows" and per problem " | x0 g0 d ring y_of_slot_0 last_slot_of_y" (offsets in floats)
//   nogroups n D m P           -> the same with a NULL row_start
//   walk D ld t steps          -> "k:at" of thread t's first element and after each of `steps` advances
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../smplpp_amd/csrc/lbfgs_wide_plan.h"

using namespace smplpp_hip;

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  std::FILE * in = std::fopen(argv[1], "r");
  std::FILE * out = std::fopen(argv[2], "w");
  if(!in || !out) return 2;
  static char line[1 << 16];
  while(std::fgets(line, sizeof line, in))
  {
    char * tok = std::strtok(line, " \n");
    if(!tok) continue;
    const std::string kind = tok;
    std::vector<long long> v;
    while((tok = std::strtok(nullptr, " \n"))) v.push_back(std::atoll(tok));
    if(kind == "groups" || kind == "nogroups")
    {
      if(v.size() < 4) return 3;
      const int64_t n = v[0], D = v[1], m = v[2], P = v[3];
      const bool null = kind == "nogroups";
      if(!null && P > 0 && (int64_t)v.size() != 4 + P + 1) return 3;
      const std::vector<int64_t> start(v.begin() + 4, v.end());
      const char * why = lbfgs_shape_refusal(n, D, m);
      if(!why) why = lbfgs_groups_refusal(n, P, null ? nullptr : start.data());
      if(why)
      {
        std::fprintf(out, "%s\n", why);
        continue;
      }
      const LbfgsLaunch L = lbfgs_wide_launch(D, P, start.data());
      const LbfgsWideSizes z = lbfgs_wide_sizes(n, D, m, P);
      std::fprintf(out, "ok %u %d %d %zu %zu %zu %zu %zu %zu %zu", L.grid, L.threads, (int)L.lds_vector, L.lds_bytes, z.ints, z.floats, z.sy, z.vec, z.hist,
                   z.rows);
      for(int64_t p = 0; p < P; p++)
      {
        const int64_t N = (start[(size_t)p + 1] - start[(size_t)p]) * D, r0 = start[(size_t)p];
        std::fprintf(out, " | %lld %lld %lld %lld %lld %lld", (long long)lbfgs_wide_vec_offset(LBFGS_X0, n, D, r0),
                     (long long)lbfgs_wide_vec_offset(LBFGS_G0, n, D, r0), (long long)lbfgs_wide_vec_offset(LBFGS_DIR, n, D, r0),
                     (long long)lbfgs_wide_hist_offset(D, m, r0), (long long)lbfgs_wide_slot_offset(N, m, 1, 0),
                     (long long)lbfgs_wide_slot_offset(N, m, 1, (int)m - 1));
      }
      std::fprintf(out, "\n");
    }
    else if(kind == "walk")
    {
      if(v.size() != 4) return 3;
      const int D = (int)v[0], t = (int)v[2];
      const int64_t ld = v[1];
      const LbfgsWideStride s = lbfgs_wide_stride(D, ld);
      LbfgsWideCursor c = lbfgs_wide_first(t, D, ld);
      std::fprintf(out, "%d:%lld", c.k, (long long)c.at);
      for(long long i = 0; i < v[3]; i++)
      {
        lbfgs_wide_advance(c, s, D);
        std::fprintf(out, " %d:%lld", c.k, (long long)c.at);
      }
      std::fprintf(out, "\n");
    }
    else
      return 3;
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
