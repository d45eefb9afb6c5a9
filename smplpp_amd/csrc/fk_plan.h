// What the forward pass decides in integers around its fused kernels (fk.hip, skin_e.hip, skin_h.hip, skin_b.hip): which workgroup
// computes which (frame tile, vertex group) items, how many workgroups a launch has, where a long batch is cut so that the kernels'
// 32-bit buffer offsets stay in range, which form a launch runs and how much workspace it reserves.  Plain C++, no HIP: the
// kernels call the functions marked FK_PLAN_HD, and tests/test_fk_plan_cpu.py sweeps all of them without a GPU
// (tests/cpp/fk_plan_dump.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "layout.h"

#ifdef __HIPCC__
#define FK_PLAN_HD __host__ __device__
#else
#define FK_PLAN_HD
#endif

namespace smplpp_hip
{
// ---- skin_kernel_e / skin_kernel_h: contiguous runs.  Workgroup b runs on XCD b & 7 (round-robin dispatch; a wrong guess costs
// speed only).  XCD x owns vertex groups [vg0, vg1), an eighth of the basis; its nvx * nft items, frame tile major (item i = frame
// tile i / nvx, group vg0 + i % nvx), are cut into contiguous runs [i0, i1), one per workgroup of the XCD: a run stays inside one
// frame tile as long as possible.  i0 >= i1: the workgroup has nothing to do (also every workgroup of an XCD that owns no group).
struct XcdRun
{
  int vg0, vg1, nvx, i0, i1;
};
FK_PLAN_HD inline XcdRun xcd_run(unsigned blocks, unsigned block, int nvg, int nft)
{
  const int nbx = (int)(blocks >> 3), xcd = (int)(block & 7), jb = (int)(block >> 3);
  const int vg0 = (xcd * nvg) >> 3, vg1 = ((xcd + 1) * nvg) >> 3, nvx = vg1 - vg0;
  const int cnt = nvx * nft;
  const int i0 = (int)(((unsigned)jb * (unsigned)cnt) / (unsigned)nbx), i1 = (int)(((unsigned)(jb + 1) * (unsigned)cnt) / (unsigned)nbx); // cnt < 2^26
  return {vg0, vg1, nvx, i0, i1};
}
// the group whose basis item k (group vgc) prefetches behind its own: the next group, the XCD's first one when the frame tile ends
// there, the same one when the run ends there (its prefetches land in images nobody reads)
FK_PLAN_HD inline int xcd_next_vg(const XcdRun & r, int k, int vgc)
{
  return k + 1 < r.i1 ? (vgc + 1 < r.vg1 ? vgc + 1 : r.vg0) : vgc;
}

// ---- skin_kernel_b: interleaved lists.  The same eighths; an XCD's cnt items, vertex group major (item i = group vg0 + i / nft,
// frame tile i % nft), go to its workgroups interleaved: workgroup j takes items j, j + stride, j + 2 stride, ...  first >= cnt:
// the workgroup has nothing to do.
struct XcdItems
{
  int vg0, cnt, first, stride;
};
FK_PLAN_HD inline XcdItems xcd_items(unsigned blocks, unsigned block, int nvg, int nft)
{
  const int nbx = (int)(blocks >> 3), xcd = (int)(block & 7), jb = (int)(block >> 3);
  const int vg0 = (xcd * nvg) >> 3, vg1 = ((xcd + 1) * nvg) >> 3;
  return {vg0, (vg1 - vg0) * nft, jb, nbx};
}
// the item whose operands item t prefetches: the list's next one, or t again (a harmless extra prefetch)
FK_PLAN_HD inline int xcd_items_next(const XcdItems & l, int t)
{
  return (t + l.stride < l.cnt) ? t + l.stride : t;
}
struct ItemTile
{
  int vg, ft;
};
FK_PLAN_HD inline ItemTile xcd_item_tile(const XcdItems & l, int i, int nft)
{
  return {l.vg0 + i / nft, i % nft};
}

// ---- workgroups per XCD of a launch (the grid is 8 times that): no more than the ceil(nvg / 8) * nft items an XCD has at most, no
// more than its CUs, at least one.  level_rounds (e, h): and no more than the longest run needs — 56 items per XCD (256 frames) are
// two rounds on 32 workgroups and on 28; the four CUs per XCD left alone are where the IK loops' side stream (face scan, finish
// kernel) runs beside this kernel, whose workgroups share a CU with nothing (1024 frames: 224 items, seven rounds on 32: unchanged)
inline int skin_grid(int cus, int nvg, int nft, bool level_rounds)
{
  const int per_xcd_items = ((nvg + 7) / 8) * nft;
  int nbx = cus / 8;
  if(nbx > per_xcd_items) nbx = per_xcd_items;
  if(nbx < 1) nbx = 1;
  if(level_rounds)
  {
    const int rounds = (per_xcd_items + nbx - 1) / nbx;
    nbx = (per_xcd_items + rounds - 1) / rounds;
  }
  return nbx;
}

// ---- frames per launch of a long batch (a multiple of 64), 0: not even one frame tile fits.  The kernels address their outputs
// with 32-bit buffer offsets: a launch writes at most 2 GiB of vertices, and has few enough frame tiles that the offsets into the
// relative transforms (g_tile_bytes per tile) stay below 2^31 too (small meshes).
constexpr int64_t SKIN_MAX_OFFSET = 0x7fffff00LL;
inline int64_t skin_batch_frames(int64_t V, int64_t g_tile_bytes)
{
  int64_t per = (SKIN_MAX_OFFSET / (V * 12)) & ~63LL;
  const int64_t per_g = (SKIN_MAX_OFFSET / g_tile_bytes) * 64;
  if(per > per_g) per = per_g;
  return per < 64 ? 0 : per;
}

// ---- the first form (fk.hip, skin_kernel<FT, MAXW>): a workgroup is 32 FT frames x 4 groups of 32 vertices
struct SkinVPlan
{
  int FT, nft, nq, grid;
  size_t shmem;
};
inline SkinVPlan skin_v_plan(int64_t n, int64_t VGn)
{
  SkinVPlan p;
  p.FT = n <= 32 ? 1 : 2;
  p.nft = (int)((n + 32 * p.FT - 1) / (32 * p.FT));
  p.nq = (int)((VGn + 3) / 4);
  p.grid = 8 * ((p.nq + 7) / 8) * p.nft;
  p.shmem = sizeof(float) * (size_t)(32 * p.FT) * (NJ * 12 + 3);
  return p;
}

// ---- form of the fused kernel a launch runs (decided once per launch, for both halves of the forward pass).  form (from
// SMPLPP_SKIN at model creation; default e) is what smplpp_fk runs: e (skin_e.hip) carries every fp32 operand exactly (bf16x3
// pieces, six MFMA products per fp32 product, fp32 VALU skinning) — the reference's arithmetic; h (skin_h.hip): fp16x2 pieces,
// 22-bit operands, skinning on the matrix pipe too; b (skin_b.hip): round 1's bf16x3 kernel; v: the first form (fp32 MFMA).
// The IK / VPoser loops' internal launches (range_slot RANGE_INTERNAL: intermediate iterates whose mesh feeds the residual's few
// vertices and the re-projection's face scan) run form_ik: h unless SMPLPP_SKIN chose a form for everything.
// form_override (0: none): the form the caller chose for this launch (an IK solver in exact-arithmetic mode runs the model's form).
inline char launch_form(char form, char form_ik, int range_slot, char form_override)
{
  return form_override ? form_override : range_slot == RANGE_INTERNAL ? form_ik : form;
}

// ---- bytes each workspace buffer of a launch of `form` must hold (0: the form does not use it).  Every form's pose step writes
// whole 64-frame tiles of its operand images (e / b stage whole tiles of G'; padding content is irrelevant there, the rows it feeds
// are never stored); the fp32 form reads its padding, so the launch zeroes it: gp_pad_bytes at float gp_pad_off of Gp, and rows
// [n, ldA) of each of AT's KP columns (at_pad floats in all).
struct FkWorkspacePlan
{
  size_t Gp, A2h, G2h, A3, AT, root;
  int64_t ldA;     // v: leading dimension of AT; other forms: 0
  int64_t gp_pad_off;
  size_t gp_pad_bytes;
  int64_t at_pad;
};
inline FkWorkspacePlan fk_workspace_plan(char form, int64_t n, bool rot_in)
{
  FkWorkspacePlan p{};
  const int64_t n64 = ((n + 63) / 64) * 64;
  if(rot_in) p.root = sizeof(float) * (size_t)n * (NJ + 1) * 3;
  p.Gp = sizeof(float) * (size_t)n64 * NJ * 12;
  if(form == 'h')
  {
    p.A2h = (size_t)(n64 / 64) * HB_KS * HB_A_BYTES;
    p.G2h = (size_t)(n64 / 64) * HB_G_BYTES;
  }
  else if(form == 'e' || form == 'b')
    p.A3 = (size_t)(n64 / 64) * BB_KS * BB_A_BYTES;
  else
  {
    p.ldA = n64;
    p.AT = sizeof(float) * (size_t)KP * p.ldA;
    if(n64 > n)
    {
      p.gp_pad_off = n * NJ * 12;
      p.gp_pad_bytes = sizeof(float) * (size_t)(n64 - n) * NJ * 12;
      p.at_pad = (int64_t)KP * (p.ldA - n);
    }
  }
  return p;
}
} // namespace smplpp_hip
