// What the host decides for the IK loop (ik.hip) before it launches anything: which instantiation of each kernel, how much LDS,
// how many workgroups, and which of the two streams does what.  Plain functions of integers and bools — plain C++, no HIP — so
// that tests/test_ik_plan_cpu.py can sweep them without a GPU (tests/cpp/ik_plan_dump.cpp); tests/solve_ref.py::solve_plan is the
// independent restatement of solve_plan below.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "layout.h"

namespace smplpp_hip
{
constexpr int TD75 = SMPLPP_THETA_DIM;        // 75
constexpr int TD44 = SMPLPP_LATENT_POSE_DIM;  // 44
constexpr int IK_MAXK = 48;                   // tasks per frame supported (the reference uses at most 41: MocapBody markers)
constexpr size_t SOLVE_LDS_MAX = 160 * 1024 - 1536; // dynamic LDS the solve kernels may ask for (160 KiB per CU, minus their static LDS: 1.2 KB)
constexpr int MAXD = TD75 + 2 * IK_MAXK + NB;  // 181: unknowns per frame supported by the in-LDS solver (every task count up to IK_MAXK, beta included)

// ---- one iteration's switches (node.cpp:655, :693-700)
struct IterFlags
{
  int opt_beta, phi_live;
};
inline IterFlags iter_flags(int optimize_beta_from, int it)
{
  const int on = (optimize_beta_from >= 0 && it >= optimize_beta_from) ? 1 : 0;
  return {on, optimize_beta_from >= 0 ? on : 1};
}

// ---- the solve: instantiation of ik_solve_kernel and its LDS plan
// phi_free: some task's surface coordinates can move (phi is live this iteration and not every limit is <= 0)
constexpr const char * SOLVE_TOO_LARGE = "smplpp_ik_iterate: system too large for the in-LDS solver";
struct SolvePlan
{
  int D, rows;     // unknowns theta_dim + 2K + beta_dim, residual rows 4K
  int m_dim, qp_k; // unknowns that can be free; the box QP (1) or the kernel's LLT exit (0)
  int ntr;         // register tiles of the instantiation (dual_only: ik_solve_kernel<true>, which carries the default, 6)
  bool dual_only;
  int chunk_rows;  // rows of J staged through LDS at a time
  size_t shmem;
  int refusal;     // 0, or which of the two "too large" conditions (SOLVE_TOO_LARGE): 1 fewer than 4 rows fit, 2 a dual shape whose rows do not all fit
};
inline SolvePlan solve_plan(int K, int theta_dim, int beta_dim, bool phi_free, bool enable_qp, bool primal_only)
{
  SolvePlan p{};
  // LDS plan: packed system + vectors, the rest (up to a 150 KB total) for the J row chunk
  p.D = theta_dim + 2 * K + beta_dim;
  p.rows = 4 * K;
  // the packed system is sized for the unknowns that CAN be free: a pinned phi (zero limit, node.cpp:567,699) never is,
  // which leaves 75 of the 157 unknowns of a 41-marker motion solve and room for its 164 Jacobian rows in two chunks
  p.m_dim = p.D - (phi_free ? 0 : 2 * K);
  // the box of node.cpp:911-929 bounds phi and d beta only: with every phi pinned and beta fixed (each motion-stage solve) no
  // variable has a finite bound, the QP's optimum IS the LLT solution (x = 0 + 1.0 (x_llt - 0): the same bits), and the kernel
  // takes its LLT exit instead of a ratio test and a bound check that cannot find anything (six barriers)
  p.qp_k = (enable_qp && (phi_free || beta_dim != 0)) ? 1 : 0;
  // tiles of 16 the register-tiled factorisation covers (176 < m_dim + 1: all-LDS path).  5 (round 4): the motion solve of a capture
  // fit has 75 unknowns that can be free (+ the rhs row = 76 <= 80): 15 register tiles per thread instead of 21 in every rank-4
  // update of its 19 column steps, its own instantiation like 11 (one tile count per instantiation: DESIGN.md §3.3)
  // (and the same fit in the 44-d latent layout has 44 + 1 <= 48: 6 register tiles per thread in its 11 steps)
  const int m1 = p.m_dim + 1;
  const int ntr_primal = (m1 <= 48) ? 3 : (m1 <= 80) ? 5 : ((m1 <= 96 || m1 > 176) ? 6 : 11);
  // theta is never bound, so the free set keeps at least theta_dim unknowns: with fewer residual rows than that every pass
  // (also every active-set pass of the QP) takes the dual form.  (Decided up here because the kernel's LDS plan depends on the
  // instantiation's tile count: ik_solve_kernel<true> carries the default, 6.)
  const bool dual_shape = p.rows < theta_dim && p.rows <= 63 && p.D <= 192 && !primal_only;
  p.ntr = dual_shape ? 6 : ntr_primal;
  const int64_t D = p.D, m_dim = p.m_dim;
  const int64_t fixed = 8 * ((m_dim + 1) * (m_dim + 2) / 2 + 7 * D + 2 * p.rows + 128 * p.ntr + 4) + 4 * 2 * D;
  // (signed: a system whose fixed part alone exceeds the budget refuses instead of wrapping around)
  const int64_t fit = ((int64_t)SOLVE_LDS_MAX - fixed) / (8 * D);
  p.chunk_rows = (int)(fit > p.rows ? p.rows : fit);
  if(p.chunk_rows < 4)
  {
    p.refusal = 1;
    return p;
  }
  p.shmem = (size_t)(fixed + 8 * p.chunk_rows * D);
  p.dual_only = dual_shape && p.chunk_rows >= p.rows;
  if(dual_shape && !p.dual_only) p.refusal = 2;
  return p;
}

// ---- the re-projection
// workgroups of the face scan.  Few frames: 1536 in all (a capture fit's 64 chains: 24 chunks of 574 faces per frame, measured
// against 9 / 18 / 36 chunks).  256 frames: TWO chunks per frame — the scan then runs beside kernels that fill the chip
// themselves (solve, pose, FK: one workgroup per frame or per CU), and fewer, longer scan workgroups take less from them than
// many short ones: configs[2] 89.2 -> 85.0 us per iteration in three alternating pairs on one box (6 chunks before); 512 frames
// keep their three (2 and 3 measured level).  SMPLPP_SCAN_BLOCKS overrides (ik.hip).
inline int64_t default_scan_blocks(int64_t n, int64_t K, int64_t F)
{
  if(n >= 512 && K <= 8 && (F + 767) / 768 <= 32) return n * ((F + 767) / 768); // (chunks of at most 768 faces: the 80-register instantiation, below)
  return (n >= 256 && n < 512) ? 2 * n : 1536;
}

struct ScanPlan
{
  int chunks;  // workgroups per frame
  int kpr;     // proj_scan_kernel<kpr, nbt3 ? 3 : CP_BATCH>: 2 / 4 queries in registers, 0 queries from LDS
  bool nbt3;
};
inline ScanPlan scan_plan(int64_t n, int K, int64_t F, int64_t scan_blocks, int scan_form)
{
  int chunks = (int)(scan_blocks / n);
  chunks = chunks < 1 ? 1 : (chunks > 32 ? 32 : chunks);
  const bool small_chunk = (F + chunks - 1) / chunks <= 3 * 256; // (a thread then meets at most three faces)
  // K <= 8 with 512 frames and more (configs[4]): the K > 8 instantiation on chunks of at most 768 faces — 80 registers, six
  // wavefronts per SIMD instead of three — is the faster one beside the decoder, whose workgroups wait for the scan's to drain
  // (44.8 against 51.6 us, the latent loop -4 %); at 256 frames the queries-in-registers form stays ahead (81.5 against 84.2 us)
  // (scan_form: the development switch SMPLPP_SCAN_FORM, 0 forces the K > 8 instantiations)
  const bool many = scan_form < 0 ? (n >= 512 && small_chunk) : scan_form == 0;
  const int kpr = (K > 8 || many) ? 0 : (K <= 4 ? 2 : 4);
  return {chunks, kpr, kpr == 0 && small_chunk};
}

// workgroups per frame of a kernel that deals a frame's K tasks to several (the evaluation, the finish kernel): with few frames,
// one round of workgroups (one per CU)
inline int frame_split(int64_t n, int K)
{
  const int split = n < 256 ? (int)(256 / n) : 1;
  return std::max(1, std::min(split, K));
}

// ---- the side stream (decisions only: the tick counters and the launches are ik.hip's)
struct SidePlan
{
  // x_phi = 0 for every task (no task's surface coordinates can move): the query points are the actual positions the
  // evaluation wrote, so scan + finish run on the side stream beside the solve and the next iteration's pose / FK
  bool beside;
  bool go;        // the side stream's fork is a flag, raised by the solve kernel once all its workgroups run
  bool ahead;     // latent_split: the NEXT iteration's decoder Jacobian on the side stream, behind this solve's "configuration final" flag
  bool join_flag; // the finish kernel raises the join flag (ahead: the Jacobian kernel behind it does)
};
inline SidePlan side_plan(bool overlap_ok, bool phi_free, bool use_flags, bool latent_split, bool opt_beta, bool another_follows)
{
  SidePlan p;
  p.beside = overlap_ok && !phi_free;
  p.go = p.beside && use_flags;
  p.ahead = latent_split && p.go && !opt_beta && another_follows;
  p.join_flag = p.go && !p.ahead;
  return p;
}

// ---- the evaluation's per-thread entries
// ik_eval_kernel advances the chain derivatives one tree level per step with one thread per (joint of the level, ancestor depth,
// axis, row).  roles [TREE_DMAX][eval_nt]: every (joint i, ancestor depth da <= depth(i), axis, row) once, dealt to the threads
// ROUND-ROBIN: entry e goes to thread e % eval_nt as its e / eval_nt-th (SMPL: 1.2 k entries, two per thread at most); -1 = none.
// (Rounds 1-3 filled row L with the entries of the joints at tree level L, the order their level-by-level recurrence needed; the
// closed form has no order, and with that filling the first wavefronts held nine entries each while the last held none.)
// Word: joint | (parent & 31) << 5 | (3 da + axis) << 10 | row << 16 | (da == depth) << 18.  Joints at depth >= TREE_DMAX get no
// entry (smplpp_ik_create refuses such a tree).  Returns the refusal, or null.
inline const char * eval_roles(const std::vector<int32_t> & parent, int eval_nt, std::vector<int32_t> & roles)
{
  roles.assign((size_t)TREE_DMAX * eval_nt, -1);
  std::vector<int> depth(NJ, 0);
  std::vector<std::vector<int>> at(NJ + 1);
  for(int i = 0; i < NJ; i++)
  {
    depth[i] = i ? depth[parent[i]] + 1 : 0;
    at[depth[i]].push_back(i);
  }
  size_t e = 0;
  for(int L = 0; L < TREE_DMAX; L++)
  {
    const int per = 9 * (L + 1);
    for(int t = 0; t < (int)at[L].size() * per; t++, e++)
    {
      if(e >= roles.size()) return "smplpp_ik_create: kinematic tree too wide for the evaluation kernel";
      const int ji = t / per, rem = t % per, da = rem / 9, a9 = rem % 9, i = at[L][ji];
      roles[e] = i | ((parent[i] & 31) << 5) | ((3 * da + a9 / 3) << 10) | ((a9 % 3) << 16) | ((da == L ? 1 : 0) << 18);
    }
  }
  return nullptr;
}
} // namespace smplpp_hip
