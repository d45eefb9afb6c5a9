// Sweeps the plans of smplpp_amd/csrc/fk_plan.h and prints one row of integers per input (tests/test_fk_plan_cpu.py builds it with
// the address and undefined-behaviour sanitizers, checks the rows against what defines them and hashes them against
// tests/golden/fk_plan.json).  Host code only.  cus, nvg, nft run over the sweep of the test's docstring.
//   fk_plan_dump grid               cus nvg nft | nbx of e, of h (levelled), of b
//   fk_plan_dump split [LEVEL=1]    cus nvg nft block | vg0 vg1 nvx i0 i1                  every workgroup of skin_grid(.., LEVEL)
//   fk_plan_dump walk LEVEL         cus nvg nft block | k ft vg next                       every item the run loop of e / h visits
//   fk_plan_dump items              cus nvg nft block | t vg ft next                       every item of b's interleaved lists
//   fk_plan_dump cut e|h|b          form V | frames per launch (0: refused)
//   fk_plan_dump ws                 form n rot_in | Gp A2h G2h A3 AT root ldA gp_pad_off gp_pad_bytes at_pad
//   fk_plan_dump vplan              n VGn | FT nft nq grid shmem
//   fk_plan_dump form               form form_ik range_slot override | form run
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../smplpp_amd/csrc/fk_plan.h"

using namespace smplpp_hip;

static const int CUS[] = {8, 64, 104, 256, 304};
static const int NVG[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 107, 108, 109, 512};
static const int NFT[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 40};
static const long long NS[] = {255, 256, 257, 1023, 1024, 1025, 65536, 1864128, 3000000};

template<class F>
static void for_grids(F f)
{
  for(int cus : CUS)
    for(int nvg : NVG)
      for(int nft : NFT) f(cus, nvg, nft);
}

static void grid()
{
  for_grids([](int cus, int nvg, int nft) {
    printf("%d %d %d %d %d %d\n", cus, nvg, nft, skin_grid(cus, nvg, nft, true), skin_grid(cus, nvg, nft, true), skin_grid(cus, nvg, nft, false));
  });
}

static void split(bool level)
{
  for_grids([&](int cus, int nvg, int nft) {
    const unsigned blocks = (unsigned)skin_grid(cus, nvg, nft, level) * 8;
    for(unsigned b = 0; b < blocks; b++)
    {
      const XcdRun r = xcd_run(blocks, b, nvg, nft);
      printf("%d %d %d %u %d %d %d %d %d\n", cus, nvg, nft, b, r.vg0, r.vg1, r.nvx, r.i0, r.i1);
    }
  });
}

// the run loop of skin_kernel_e / skin_kernel_h, stepped on the host: the same functions, the same ft / iend / vgk stepping
static void walk(bool level)
{
  for_grids([&](int cus, int nvg, int nft) {
    const unsigned blocks = (unsigned)skin_grid(cus, nvg, nft, level) * 8;
    for(unsigned b = 0; b < blocks; b++)
    {
      const XcdRun r = xcd_run(blocks, b, nvg, nft);
      if(r.i0 >= r.i1) continue;
      for(int i = r.i0; i < r.i1;)
      {
        const int ft = i / r.nvx;
        const int iend = (ft + 1) * r.nvx < r.i1 ? (ft + 1) * r.nvx : r.i1;
        int vgk = r.vg0 + (i - ft * r.nvx);
        printf("%d %d %d %u %d %d %d %d\n", cus, nvg, nft, b, i, ft, vgk, xcd_next_vg(r, i, vgk));
        for(int k = i + 1; k < iend; k++)
        {
          vgk++;
          printf("%d %d %d %u %d %d %d %d\n", cus, nvg, nft, b, k, ft, vgk, xcd_next_vg(r, k, vgk));
        }
        i = iend;
      }
    }
  });
}

// skin_kernel_b's loop over its list
static void items()
{
  for_grids([](int cus, int nvg, int nft) {
    const unsigned blocks = (unsigned)skin_grid(cus, nvg, nft, false) * 8;
    for(unsigned b = 0; b < blocks; b++)
    {
      const XcdItems l = xcd_items(blocks, b, nvg, nft);
      if(l.first >= l.cnt) continue;
      for(int t = l.first; t < l.cnt; t += l.stride)
      {
        const ItemTile it = xcd_item_tile(l, t, nft);
        printf("%d %d %d %u %d %d %d %d\n", cus, nvg, nft, b, t, it.vg, it.ft, xcd_items_next(l, t));
      }
    }
  });
}

// G' bytes of one frame tile as each form's kernel holds them: E_G_BYTES (skin_e.hip), HB_G_BYTES, B_LDS_G (skin_b.hip)
static long long g_tile_bytes(char form)
{
  return form == 'e' ? 64 * NJ * 48 : form == 'h' ? HB_G_BYTES : 64 * NJ * 12 * 4;
}
static void cut(char form)
{
  auto row = [&](long long V) { printf("%c %lld %lld\n", form, V, (long long)skin_batch_frames(V, g_tile_bytes(form))); };
  long long V = 1;
  for(; V <= 8192; V++) row(V);
  for(; V < 2796000; V += V / 64) row(V);
  for(V = 2796190; V <= 2796215; V++) row(V); // (the refusal begins at 2796203)
}

static void ws()
{
  auto row = [](char form, long long n, bool rot_in) {
    const FkWorkspacePlan p = fk_workspace_plan(form, n, rot_in);
    printf("%c %lld %d %zu %zu %zu %zu %zu %zu %lld %lld %zu %lld\n", form, n, (int)rot_in, p.Gp, p.A2h, p.G2h, p.A3, p.AT, p.root, (long long)p.ldA,
           (long long)p.gp_pad_off, p.gp_pad_bytes, (long long)p.at_pad);
  };
  for(char form : {'e', 'h', 'b', 'v'})
    for(int rot = 0; rot < 2; rot++)
    {
      for(long long n = 1; n <= 200; n++) row(form, n, rot);
      for(long long n : NS) row(form, n, rot);
    }
}

static void vplan()
{
  auto row = [](long long n, long long VGn) {
    const SkinVPlan p = skin_v_plan(n, VGn);
    printf("%lld %lld %d %d %d %d %zu\n", n, VGn, p.FT, p.nft, p.nq, p.grid, p.shmem);
  };
  for(long long VGn : {1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 216, 217, 1000})
  {
    for(long long n = 1; n <= 200; n++) row(n, VGn);
    for(long long n : NS) row(n, VGn);
  }
}

static void form()
{
  for(char f : {'e', 'h', 'b', 'v'})
    for(char fi : {'h', f})
      for(int slot : {RANGE_DEVICE, RANGE_HOST, RANGE_INTERNAL})
        for(char o : {'\0', 'e', 'h', 'b', 'v'}) printf("%d %d %d %d %d\n", f, fi, slot, o, launch_form(f, fi, slot, o));
}

int main(int argc, char ** argv)
{
  const char * mode = argc > 1 ? argv[1] : "";
  if(!strcmp(mode, "grid")) grid();
  else if(!strcmp(mode, "split")) split(argc < 3 || argv[2][0] != '0');
  else if(!strcmp(mode, "walk") && argc == 3) walk(argv[2][0] != '0');
  else if(!strcmp(mode, "items")) items();
  else if(!strcmp(mode, "cut") && argc == 3) cut(argv[2][0]);
  else if(!strcmp(mode, "ws")) ws();
  else if(!strcmp(mode, "vplan")) vplan();
  else if(!strcmp(mode, "form")) form();
  else
  {
    fprintf(stderr, "usage: fk_plan_dump grid | split [0|1] | walk 0|1 | items | cut e|h|b | ws | vplan | form\n");
    return 2;
  }
  return 0;
}
