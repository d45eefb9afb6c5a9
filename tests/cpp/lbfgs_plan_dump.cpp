// The host decisions of the batched L-BFGS (smplpp_amd/csrc/lbfgs_plan.h) as a stand-alone program; driven by tests/test_lbfgs_cpu.py,
// which builds it with the address and undefined-behaviour sanitizers and compares every answer with a Python restatement.
// usage: lbfgs_plan_dump <queries.txt> <answers.txt>; one answer line per query line:
//   plan n D m          -> the refusal, or "ok grid threads lds_vector lds_bytes ints floats sy vec hist"
//   rows n D ld         -> the refusal, or "ok"
//   opts c1 tol_grad tol_f max_ls curv_eps -> the refusal, or "ok"
//   ring m ops          -> ops is a string of p (push) and d (drop): after each op "slot|-:head:count:slots newest to oldest,"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../smplpp_amd/csrc/lbfgs_plan.h"

using namespace smplpp_hip;

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  std::FILE * in = std::fopen(argv[1], "r");
  std::FILE * out = std::fopen(argv[2], "w");
  if(!in || !out) return 2;
  char line[4096], kind[16];
  while(std::fgets(line, sizeof line, in))
  {
    long long a = 0, b = 0, c = 0;
    if(std::sscanf(line, "%15s", kind) != 1) continue;
    const char * rest = line + std::strlen(kind);
    if(!std::strcmp(kind, "plan") && std::sscanf(rest, "%lld %lld %lld", &a, &b, &c) == 3)
    {
      if(const char * why = lbfgs_shape_refusal(a, b, c))
        std::fprintf(out, "%s\n", why);
      else
      {
        const LbfgsLaunch L = lbfgs_launch(a, b);
        const LbfgsSizes z = lbfgs_sizes(a, b, c);
        std::fprintf(out, "ok %u %d %d %zu %zu %zu %zu %zu %zu\n", L.grid, L.threads, (int)L.lds_vector, L.lds_bytes, z.ints, z.floats, z.sy, z.vec, z.hist);
      }
    }
    else if(!std::strcmp(kind, "rows") && std::sscanf(rest, "%lld %lld %lld", &a, &b, &c) == 3)
    {
      const char * why = lbfgs_rows_refusal(a, b, c);
      std::fprintf(out, "%s\n", why ? why : "ok");
    }
    else if(!std::strcmp(kind, "opts"))
    {
      char t[5][64];
      if(std::sscanf(rest, "%63s %63s %63s %63s %63s", t[0], t[1], t[2], t[3], t[4]) != 5) return 3;
      const LbfgsOptions o{std::strtof(t[0], nullptr), std::strtof(t[1], nullptr), std::strtof(t[2], nullptr), std::atoi(t[3]), std::strtof(t[4], nullptr)};
      const char * why = lbfgs_options_refusal(o);
      std::fprintf(out, "%s\n", why ? why : "ok");
    }
    else if(!std::strcmp(kind, "ring"))
    {
      int m = 0;
      char ops[2048];
      if(std::sscanf(rest, "%d %2047s", &m, ops) != 2) return 3;
      int head = 0, count = 0;
      for(const char * p = ops; *p; p++)
      {
        if(*p == 'p')
          std::fprintf(out, "%d", lbfgs_ring_push(head, count, m));
        else
          lbfgs_ring_drop(head, count), std::fprintf(out, "-");
        std::fprintf(out, ":%d:%d:", head, count);
        for(int i = 0; i < count; i++) std::fprintf(out, "%d ", lbfgs_ring_slot(head, count, m, i));
        std::fprintf(out, ",");
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
