// Sweeps the host plans of smplpp_amd/csrc/ik_plan.h and prints one row of integers per input (tests/test_ik_plan_cpu.py builds it
// with the address and undefined-behaviour sanitizers, compares the solve rows with tests/solve_ref.py and hashes the others against
// tests/golden/ik_plan.json).  Host code only.
//   ik_plan_dump solve              K td bd locked live qp primal | D rows m_dim qp_k ntr dual_only chunk_rows shmem refusal
//   ik_plan_dump scan               n K F form blocks | chunks kpr nbt frame_split default_blocks    (blocks: the default first, then 1, 1536, 1e6)
//   ik_plan_dump side               overlap_ok phi_free use_flags latent_split opt_beta another | beside go ahead join_flag
//   ik_plan_dump iter               optimize_beta_from it | opt_beta phi_live
//   ik_plan_dump roles FILE NT      FILE: int32 parent[24]; one word per line, or "refusal: ..." alone
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../smplpp_amd/csrc/ik_plan.h"

using namespace smplpp_hip;

static void solve()
{
  for(int K = 1; K <= 64; K++)
    for(int td : {TD44, TD75})
      for(int bd : {0, NB})
        for(int mask = 0; mask < 16; mask++)
        {
          const bool locked = mask & 1, live = mask & 2, qp = mask & 4, primal = mask & 8;
          const SolvePlan p = solve_plan(K, td, bd, live && !locked, qp, primal);
          printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d\n", K, td, bd, (int)locked, (int)live, (int)qp, (int)primal, p.D, p.rows,
                 p.m_dim, p.qp_k, p.ntr, (int)p.dual_only, p.chunk_rows, p.shmem, p.refusal);
        }
}

static void scan()
{
  const long long ns[] = {1, 2, 3, 4, 8, 64, 128, 255, 256, 257, 511, 512, 513, 1024};
  const long long Fs[] = {1, 20, 767, 768, 769, 2304, 2305, 13776, 24576, 24577, 100000};
  for(long long n : ns)
    for(int K = 1; K <= 48; K++)
      for(long long F : Fs)
        for(int form = -1; form <= 1; form++)
        {
          const long long def = default_scan_blocks(n, K, F);
          for(long long blocks : {def, 1LL, 1536LL, 1000000LL})
          {
            const ScanPlan p = scan_plan(n, K, F, blocks, form);
            printf("%lld %d %lld %d %lld %d %d %d %d %lld\n", n, K, F, form, blocks, p.chunks, p.kpr, p.nbt3 ? 3 : 6, frame_split(n, K), def);
          }
        }
}

static void side()
{
  for(int x = 0; x < 64; x++)
  {
    const bool o = x & 1, f = x & 2, u = x & 4, l = x & 8, b = x & 16, a = x & 32;
    const SidePlan p = side_plan(o, f, u, l, b, a);
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)o, (int)f, (int)u, (int)l, (int)b, (int)a, (int)p.beside, (int)p.go, (int)p.ahead, (int)p.join_flag);
  }
}

static void iter()
{
  for(int from : {-1, 0, 1, 2, 25, 1000})
    for(int it = 0; it <= 30; it++)
    {
      const IterFlags f = iter_flags(from, it);
      printf("%d %d %d %d\n", from, it, f.opt_beta, f.phi_live);
    }
}

static int roles(const char * path, int nt)
{
  std::vector<int32_t> parent(NJ), words;
  FILE * f = fopen(path, "rb");
  if(!f || fread(parent.data(), sizeof(int32_t), NJ, f) != (size_t)NJ) return 2;
  fclose(f);
  if(const char * why = eval_roles(parent, nt, words))
  {
    printf("refusal: %s\n", why);
    return 0;
  }
  for(int32_t w : words) printf("%d\n", w);
  return 0;
}

int main(int argc, char ** argv)
{
  const char * mode = argc > 1 ? argv[1] : "";
  if(!strcmp(mode, "solve")) solve();
  else if(!strcmp(mode, "scan")) scan();
  else if(!strcmp(mode, "side")) side();
  else if(!strcmp(mode, "iter")) iter();
  else if(!strcmp(mode, "roles") && argc == 4) return roles(argv[2], atoi(argv[3]));
  else
  {
    fprintf(stderr, "usage: ik_plan_dump solve | scan | side | iter | roles FILE NT\n");
    return 2;
  }
  return 0;
}
