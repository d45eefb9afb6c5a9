// smplpp_skeleton / smplpp_skeleton_rotmat and their vector-Jacobian products: the kinematic chain alone.  World joint transforms
// [A_j | g_j + trans], the posed joints g_j + trans and the rest joints J, from the functions the pose step is written in
// (pose_math.h), and the gradient of any loss on them to beta, theta (or trans and rot), without touching a vertex.
//
// Forward, per frame:  R_j = rodrigues9(theta[1 + j]) (rotmat entry: rot[j] as given);  J = J0 + JS.beta (joint_coord);
//   A_0 = R_0, g_0 = J_0;  A_j = A_p R_j, g_j = A_p (J_j - J_p) + g_p (chain_entry, the operand order of pose_body.h, one tree level
//   at a time);  posed_j = g_j + trans (one fp32 add);  world_j = [A_j | posed_j], 3x4 row-major.
// So world[..., :3] has the bits of the 3x3 block of smplpp_fk's xforms, and joints the bits of its joints.
//
// Backward, per frame (the forward is recomputed; nothing is saved between the two calls; every operation outside the shared
// functions is rounded on its own):
//   seeds  dA_j = grad_world[j][:, :3], dg_j = grad_world[j][:, 3] + grad_posed[j], dJ_j = grad_joints[j]   (NULL reads as +0)
//   grad_trans = sum of the 24 seed dg_j, ascending j, from +0
//   levels from the deepest to 1, joint j with parent p:
//     dR_j = A_p^T dA_j;  cA_j = dA_j R_j^T + dg_j (J_j - J_p)^T;  cJ_j = A_p^T dg_j;  dJ_j += cJ_j
//     then the parent gathers its children in ascending joint order: dA_p += cA_i, dg_p += dg_i, dJ_p -= cJ_i
//   root   dR_0 = dA_0, dJ_0 += dg_0
//   grad_beta[k] = sum_i JS[i][k] dJ[i], i = 0..71 ascending from +0
//   grad_theta[1 + j][m] = sum_q dR_j[q] rodrigues_grad_dev(theta_j, m)[q], ascending q from +0; row 0 = grad_trans
//   rotmat entry: grad_rot = dR, nine independent entries per joint (the convention of smplpp_fk_rotmat_vjp)
// This is vjp_chain_kernel's recurrence (fk_vjp.hip) with other seeds.
//
// Kernel shape: ONE WAVEFRONT PER FRAME, SK_T = 4 frames per 256-thread workgroup, one launch per call.  The chain is a string of
// dependent latencies with at most 60 independent entries per level on SMPL's tree, so a frame fits one wavefront, and a
// wavefront's LDS traffic executes in order: the phases are separated by wave_sync() (pose_body.h) alone.  The four wavefronts of a
// workgroup never meet: there is no s_barrier in either kernel, each wavefront has its own LDS block, and a wavefront whose frame
// is past n leaves at once.  No atomics, no scratch, no workspace: a device-space call touches nothing in the handle.  A frame's
// arithmetic depends on that frame's inputs and the model only, so its bits do not depend on n, on its place in the batch, on the
// memory space or on which outputs or cotangents are asked for.  Any tree smplpp_model_create accepts runs through the same loops
// (levels from the model's level table; a level wider than a wavefront's lanes takes more than one pass).
// The kernels are chains of LDS turn-arounds, so each step makes as few as it can: the tree comes from one packed word per slot of
// the level order and a mask of children (SkelFwd), the level offsets from a register, and a lane picks its operands by word offset
// with selects instead of branching on the kind of entry it owns (SkelAll); the backward fetches its cotangents, its column of JS and
// its axis-angles in front of the chain.  Measurements: DESIGN.md 3.26.
#include "common.h"
#include "pose_body.h"
#include "rodrigues_grad.h"
#include "staging.h"
#include "trace.h"

namespace smplpp_hip
{
constexpr int SK_T = 4; // frames (wavefronts) per workgroup

struct SkelArgs
{
  const float * beta;  // [n][10] (nullable: zeros)
  const float * pose;  // theta [n][25][3]; rotmat entries: rot [n][24][9]
  const float * trans; // rotmat entries: [n][3] (nullable: zeros)
  const float * JSp;   // [72][12] folded regressor rows [JS (10) | J0 | 0]
  const float * JS;    // [72][10]
  const int32_t *parent, *lvl_off, *lvl_joint;
  int nlev;
  int64_t n;
  float *world, *posed, *joints;           // forward outputs (nullable)
  const float *gworld, *gposed, *gjoints;  // backward cotangents (nullable: +0)
  float *gbeta, *gpose0, *grot;            // backward outputs (nullable): gpose0 = grad_theta [n][25][3], or grad_trans [n][3] beside grad_rot
  int accumulate;
};

// the forward state of one frame, one block per wavefront
struct SkelFwd
{
  float R[NJ][9], J[NJ][3];
  __attribute__((aligned(16))) float G[NJ][12]; // [A | g], 3x4 row-major
  float tr[4], zero[4];
  // the tree in level order (slot k of the model's joints-by-level list): lj = joint | parent << 8 (root: parent byte 0xff), cm = the
  // joint's children as a bit mask.  One look-up per step instead of a chain of them; the children of a joint all lie one level down,
  // and ascending bits are ascending joints.
  int lj[NJ], cm[NJ];
};
struct SkelBwd
{
  float dA[NJ][9], dg[NJ][3], dJ[NJ][3], dR[NJ][9], cA[NJ][9], cJ[NJ][3];
};
// forward and backward state of a frame in one block: the steps of the chain address it by WORD OFFSET from its start, so that a lane
// picks its operands with selects, fetches them in one batch and runs the same instructions as its neighbours whatever entry it
// owns (a branch per kind of entry would run the kinds one after the other, each with its own LDS turn-around)
struct SkelAll
{
  SkelFwd f;
  SkelBwd b;
};
constexpr int SK_R = offsetof(SkelFwd, R) / 4, SK_J = offsetof(SkelFwd, J) / 4, SK_G = offsetof(SkelFwd, G) / 4,
              SK_ZERO = offsetof(SkelFwd, zero) / 4, SK_B = offsetof(SkelAll, b) / 4, SK_DA = SK_B + offsetof(SkelBwd, dA) / 4,
              SK_DG = SK_B + offsetof(SkelBwd, dg) / 4, SK_DJ = SK_B + offsetof(SkelBwd, dJ) / 4, SK_DR = SK_B + offsetof(SkelBwd, dR) / 4,
              SK_CA = SK_B + offsetof(SkelBwd, cA) / 4, SK_CJ = SK_B + offsetof(SkelBwd, cJ) / 4;

// offset of level L in the level-ordered list (lane L of `offv` holds it: a register look-up, no LDS turn-around per level)
__device__ __forceinline__ int skel_level(int offv, int L)
{
  return __builtin_amdgcn_readlane(offv, L);
}

// rotations, joints and the chain of frame f into s, by the wavefront's 64 lanes; returns the level offsets, one per lane
template<bool ROT_IN>
__device__ __forceinline__ int skel_forward(const SkelArgs & a, const int64_t f, const int lane, SkelFwd & s)
{
  const int offv = lane <= a.nlev ? a.lvl_off[lane] : 0;
  if(lane >= 32 && lane < 32 + NJ)
  {
    const int i = a.lvl_joint[lane - 32], p = a.parent[i];
    int cm = 0;
#pragma unroll
    for(int c = 1; c < NJ; c++) cm |= (a.parent[c] == i ? 1 : 0) << c; // (uniform addresses: scalar loads)
    s.lj[lane - 32] = i | ((p & 0xff) << 8);
    s.cm[lane - 32] = cm;
  }
  if(lane >= 60 && lane < 63)
  {
    if constexpr(ROT_IN)
      s.tr[lane - 60] = a.trans ? a.trans[f * 3 + (lane - 60)] : 0.0f;
    else
      s.tr[lane - 60] = a.pose[f * ((NJ + 1) * 3) + (lane - 60)];
  }
  float be[NB];
#pragma unroll
  for(int k = 0; k < NB; k++) be[k] = a.beta ? a.beta[f * NB + k] : 0.0f;
  for(int t = lane; t < NJ * 3; t += 64) // joints (src/JointRegression.cpp:588-590 through the folded regressor)
  {
    const float4 * row = reinterpret_cast<const float4 *>(a.JSp + t * 12);
    const float4 u = row[0], v = row[1], w = row[2];
    const float js[NB] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w, w.x, w.y};
    s.J[t / 3][t % 3] = joint_coord(w.z, js, be);
  }
  if(lane < NJ)
  {
    float R[9];
    if constexpr(ROT_IN)
    {
#pragma unroll
      for(int q = 0; q < 9; q++) R[q] = a.pose[(f * NJ + lane) * 9 + q];
    }
    else
    {
      const float * th = a.pose + (f * (NJ + 1) + 1 + lane) * 3;
      rodrigues9(th[0], th[1], th[2], R);
    }
#pragma unroll
    for(int q = 0; q < 9; q++) s.R[lane][q] = R[q];
  }
  if(lane >= 56 && lane < 60) s.zero[lane - 56] = 0.0f;
  wave_sync();
  // chain: G_0 = [R_0 | J_0] (level 0 is joint 0 alone: parent(i) < i), G_i = G_p . [R_i | J_i - J_p], level by level; lane = (joint
  // of the level, entry of its 3x4).  The operand is a - b with (a, b) = (column c of R_i, the zero words) or (J_i, J_p), as in
  // pose_body.h's chain: a - 0 is a, to the bit.
  const float * fb = reinterpret_cast<const float *>(&s);
  if(lane < 12) s.G[0][lane] = (lane % 4 < 3) ? s.R[0][(lane / 4) * 3 + lane % 4] : s.J[0][lane / 4];
  wave_sync();
  for(int L = 1; L < a.nlev; L++)
  {
    const int lo = skel_level(offv, L) * 12, hi = skel_level(offv, L + 1) * 12;
    for(int e = lo + lane; e < hi; e += 64)
    {
      const int w = s.lj[e / 12], i = w & 0xff, p = w >> 8, q = e % 12, r = q / 4, c = q % 4;
      const bool t = c == 3;
      const int xa = t ? SK_J + i * 3 : SK_R + i * 9 + c, xs = t ? 1 : 3;
      const int ba = t ? SK_J + p * 3 : SK_ZERO, bs = t ? 1 : 0;
      const float * g = fb + SK_G + p * 12 + r * 4;
      const float a0 = fb[xa], a1 = fb[xa + xs], a2 = fb[xa + 2 * xs], b0 = fb[ba], b1 = fb[ba + bs], b2 = fb[ba + 2 * bs];
      const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
      s.G[i][q] = chain_entry(g0, g1, g2, g3, a0 - b0, a1 - b1, a2 - b2, t);
    }
    wave_sync();
  }
  return offv;
}

template<bool ROT_IN>
__global__ __launch_bounds__(64 * SK_T) void skeleton_kernel(SkelArgs a)
{
  __shared__ SkelFwd sF[SK_T];
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * SK_T + w;
  if(f >= a.n) return; // (wavefront-uniform; the kernel has no workgroup barrier)
  SkelFwd & s = sF[w];
  skel_forward<ROT_IN>(a, f, lane, s);
  for(int e = lane; e < NJ * 12; e += 64)
  {
    const int i = e / 12, q = e % 12, r = q / 4, c = q % 4;
    float v = s.G[i][q];
    if(c == 3)
    {
      v = v + s.tr[r];
      if(a.posed) a.posed[(f * NJ + i) * 3 + r] = v;
    }
    if(a.world) a.world[f * (NJ * 12) + e] = v;
  }
  if(a.joints)
    for(int t = lane; t < NJ * 3; t += 64) a.joints[f * (NJ * 3) + t] = s.J[t / 3][t % 3];
}

__device__ __forceinline__ void skel_store(float * p, float v, int accumulate)
{
  *p = accumulate ? *p + v : v;
}

template<bool ROT_IN>
__global__ __launch_bounds__(64 * SK_T) void skeleton_vjp_kernel(SkelArgs a)
{
#pragma clang fp contract(off)
  __shared__ SkelAll sA[SK_T];
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * SK_T + w;
  if(f >= a.n) return;
  SkelFwd & s = sA[w].f;
  SkelBwd & b = sA[w].b;
  float * const fb = reinterpret_cast<float *>(&sA[w]); // the block by word offset (SK_*)
  // what does not depend on the chain is fetched in front of it, so that its latency runs beside the forward: the cotangents (six
  // seed entries per lane), this lane's column of JS for grad_beta, and the axis-angles of its grad_theta entries
  float seed[6];
#pragma unroll
  for(int t = 0; t < 6; t++)
  {
    const int e = lane + 64 * t, j = e / 15, q = e % 15;
    float v = 0.0f;
    if(e < NJ * 15)
    {
      if(q < 9)
        v = a.gworld ? a.gworld[(f * NJ + j) * 12 + (q / 3) * 4 + q % 3] : 0.0f;
      else if(q < 12)
      {
        const float gw = a.gworld ? a.gworld[(f * NJ + j) * 12 + (q - 9) * 4 + 3] : 0.0f;
        const float gp = a.gposed ? a.gposed[(f * NJ + j) * 3 + (q - 9)] : 0.0f;
        v = gw + gp;
      }
      else
        v = a.gjoints ? a.gjoints[(f * NJ + j) * 3 + (q - 12)] : 0.0f;
    }
    seed[t] = v;
  }
  const bool beta_lane = a.gbeta && lane >= 32 && lane < 32 + NB;
  float js[NJ * 3];
#pragma unroll
  for(int i = 0; i < NJ * 3; i++) js[i] = beta_lane ? a.JS[i * NB + (lane - 32)] : 0.0f;
  float th[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  if constexpr(!ROT_IN)
  {
#pragma unroll
    for(int u = 0; u < 2; u++)
      if(a.gpose0 && lane + 64 * u < NJ * 3)
#pragma unroll
        for(int c = 0; c < 3; c++) th[u][c] = a.pose[(f * (NJ + 1) + 1 + (lane + 64 * u) / 3) * 3 + c];
  }
  const int offv = skel_forward<ROT_IN>(a, f, lane, s);
  // ---- seeds
#pragma unroll
  for(int t = 0; t < 6; t++)
  {
    const int e = lane + 64 * t, j = e / 15, q = e % 15;
    if(e < NJ * 15) *(q < 9 ? &b.dA[j][q] : (q < 12 ? &b.dg[j][q - 9] : &b.dJ[j][q - 12])) = seed[t];
  }
  wave_sync();
  float gt = 0.0f; // lanes 0..2: grad_trans, the seed dg in ascending joint order
  if(lane < 3)
#pragma unroll
    for(int j = 0; j < NJ; j++) gt = gt + b.dg[j][lane];
  // ---- the chain backwards
  for(int L = a.nlev - 1; L >= 1; L--)
  {
    const int lo = skel_level(offv, L), hi = skel_level(offv, L + 1), plo = skel_level(offv, L - 1);
    // lane = (joint of level L, one of the 21 entries of dR | cA | cJ)
    for(int e = lane; e < (hi - lo) * 21; e += 64)
    {
      // kind 0, q < 9:  dR_j[c0][c1] = sum_k A_p[k][c0] dA_j[k][c1]
      // kind 1, q < 18: cA_j[c0][c1] = sum_k dA_j[c0][k] R_j[c1][k] + dg_j[c0] (J_j - J_p)[c1]
      // kind 2:         cJ_j[c1]     = sum_k A_p[k][c1] dg_j[k], and dJ_j[c1] += cJ_j[c1]
      // each (x0 y0 + x1 y1) + x2 y2 over operands at (xa + k xs, ya + k ys)
      const int w2 = s.lj[lo + e / 21], j = w2 & 0xff, p = w2 >> 8, q = e % 21;
      const int kind = q < 9 ? 0 : (q < 18 ? 1 : 2), u = q - (kind == 0 ? 0 : (kind == 1 ? 9 : 18)), c0 = u / 3, c1 = u % 3;
      const int xa = kind == 1 ? SK_DA + j * 9 + 3 * c0 : SK_G + p * 12 + (kind == 0 ? c0 : c1), xs = kind == 1 ? 1 : 4;
      const int ya = kind == 0 ? SK_DA + j * 9 + c1 : (kind == 1 ? SK_R + j * 9 + 3 * c1 : SK_DG + j * 3), ys = kind == 0 ? 3 : 1;
      const int dst = kind == 0 ? SK_DR + j * 9 + u : (kind == 1 ? SK_CA + j * 9 + u : SK_CJ + j * 3 + u);
      const float x0 = fb[xa], x1 = fb[xa + xs], x2 = fb[xa + 2 * xs], y0 = fb[ya], y1 = fb[ya + ys], y2 = fb[ya + 2 * ys];
      const float dgr = b.dg[j][c0], jj = s.J[j][c1], jp = s.J[p][c1], dJold = b.dJ[j][c1]; // (in range for every kind)
      float v = (x0 * y0 + x1 * y1) + x2 * y2;
      const float ex = dgr * (jj - jp);
      v = kind == 1 ? v + ex : v;
      fb[dst] = v;
      if(kind == 2) b.dJ[j][c1] = dJold + v;
    }
    wave_sync();
    // lane = (joint of level L - 1, one of the 15 entries of dA | dg | dJ): its children from the mask, ascending
    for(int e = lane; e < (lo - plo) * 15; e += 64)
    {
      const int k = plo + e / 15, p = s.lj[k] & 0xff, q = e % 15;
      int cm = s.cm[k];
      const int kind = q < 9 ? 0 : (q < 12 ? 1 : 2), u = q - (kind == 0 ? 0 : (kind == 1 ? 9 : 12));
      const int dst = kind == 0 ? SK_DA + p * 9 + u : (kind == 1 ? SK_DG : SK_DJ) + p * 3 + u;
      const int src = (kind == 0 ? SK_CA : (kind == 1 ? SK_DG : SK_CJ)) + u, stride = kind == 0 ? 9 : 3;
      float v = fb[dst];
      while(cm)
      {
        const int i = __builtin_ctz(cm);
        cm &= cm - 1;
        const float x = fb[src + i * stride];
        v = kind == 2 ? v - x : v + x;
      }
      fb[dst] = v;
    }
    wave_sync();
  }
  // ---- root: A_0 = R_0, g_0 = J_0
  if(lane < 9) b.dR[0][lane] = b.dA[0][lane];
  if(lane >= 9 && lane < 12) b.dJ[0][lane - 9] = b.dJ[0][lane - 9] + b.dg[0][lane - 9];
  wave_sync();
  // ---- J = J0 + JS.beta
  if(beta_lane)
  {
    float sum = 0.0f;
#pragma unroll
    for(int i = 0; i < NJ * 3; i++) sum = sum + js[i] * b.dJ[i / 3][i % 3];
    skel_store(a.gbeta + f * NB + (lane - 32), sum, a.accumulate);
  }
  if constexpr(ROT_IN)
  {
    if(a.grot)
      for(int t = lane; t < NJ * 9; t += 64) skel_store(a.grot + f * (NJ * 9) + t, b.dR[t / 9][t % 9], a.accumulate);
    if(a.gpose0 && lane < 3) skel_store(a.gpose0 + f * 3 + lane, gt, a.accumulate);
  }
  else if(a.gpose0)
  {
#pragma unroll
    for(int u = 0; u < 2; u++)
    {
      const int t = lane + 64 * u, j = t / 3, m = t % 3;
      if(t >= NJ * 3) break;
      float dRdt[9];
      rodrigues_grad_dev(th[u], m, dRdt);
      float sum = 0.0f;
#pragma unroll
      for(int q = 0; q < 9; q++) sum = sum + b.dR[j][q] * dRdt[q];
      skel_store(a.gpose0 + (f * (NJ + 1) + 1 + j) * 3 + m, sum, a.accumulate);
    }
    if(lane < 3) skel_store(a.gpose0 + f * ((NJ + 1) * 3) + lane, gt, a.accumulate);
  }
}

static SkelArgs skel_args(const smplpp_model * m, int64_t n, const float * beta, const float * pose, const float * trans)
{
  SkelArgs a = {};
  a.beta = beta;
  a.pose = pose;
  a.trans = trans;
  a.JSp = m->JSp.get();
  a.JS = m->JS.get();
  a.parent = m->parent.get();
  a.lvl_off = m->lvl.get();
  a.lvl_joint = m->lvl.get() + NJ + 1;
  a.nlev = m->nlev;
  a.n = n;
  return a;
}

static int skel_launch(const SkelArgs & a, bool rot_in, bool backward, hipStream_t st)
{
  const dim3 grid((unsigned)((a.n + SK_T - 1) / SK_T)), block(64 * SK_T);
  if(backward)
  {
    if(rot_in)
      skeleton_vjp_kernel<true><<<grid, block, 0, st>>>(a);
    else
      skeleton_vjp_kernel<false><<<grid, block, 0, st>>>(a);
  }
  else
  {
    if(rot_in)
      skeleton_kernel<true><<<grid, block, 0, st>>>(a);
    else
      skeleton_kernel<false><<<grid, block, 0, st>>>(a);
  }
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int skel_forward_call(const char * fn, smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * pose, bool rot_in,
                             float * world, float * posed, float * joints, int space, void * stream)
{
  const std::string name(fn);
  if(!m) return fail(SMPLPP_ERR_INVALID, name + ": null model");
  if(n <= 0 || !pose) return fail(SMPLPP_ERR_INVALID, name + (rot_in ? ": needs n > 0 and rot" : ": needs n > 0 and theta"));
  if(!world && !posed && !joints) return fail(SMPLPP_ERR_INVALID, name + ": at least one output must be asked for");
  if(int rc = check_space(space, fn)) return rc;
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, name + ": too many frames");
  Frame fr(m->device, &m->arena, space, stream, "skeleton");
  SkelArgs a = skel_args(m, n, nullptr, nullptr, nullptr);
  a.beta = fr.in(beta, (size_t)n * NB);
  a.trans = rot_in ? fr.in(trans, (size_t)n * 3) : nullptr;
  a.pose = fr.in(pose, (size_t)n * (rot_in ? NJ * 9 : (NJ + 1) * 3));
  a.world = fr.out(world, (size_t)n * NJ * 12);
  a.posed = fr.out(posed, (size_t)n * NJ * 3);
  a.joints = fr.out(joints, (size_t)n * NJ * 3);
  return fr.run([&] { return skel_launch(a, rot_in, false, fr.st); });
}

static int skel_backward_call(const char * fn, smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * pose, bool rot_in,
                              const float * grad_world, const float * grad_posed, const float * grad_joints, float * grad_beta, float * grad_pose0,
                              float * grad_rot, int accumulate, int space, void * stream)
{
  const std::string name(fn);
  if(!m) return fail(SMPLPP_ERR_INVALID, name + ": null model");
  if(n <= 0 || !pose) return fail(SMPLPP_ERR_INVALID, name + (rot_in ? ": needs n > 0 and rot" : ": needs n > 0 and theta"));
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, name + ": accumulate must be 0 or 1");
  if(!grad_world && !grad_posed && !grad_joints) return fail(SMPLPP_ERR_INVALID, name + ": at least one cotangent must be given");
  if(!grad_beta && !grad_pose0 && !grad_rot) return fail(SMPLPP_ERR_INVALID, name + ": at least one output must be asked for");
  if(int rc = check_space(space, fn)) return rc;
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, name + ": too many frames");
  Frame fr(m->device, &m->arena, space, stream, "backward skeleton");
  SkelArgs a = skel_args(m, n, nullptr, nullptr, nullptr);
  a.beta = fr.in(beta, (size_t)n * NB);
  // (the rotmat backward does not read trans: no output depends on it)
  a.pose = fr.in(pose, (size_t)n * (rot_in ? NJ * 9 : (NJ + 1) * 3));
  a.gworld = fr.in(grad_world, (size_t)n * NJ * 12);
  a.gposed = fr.in(grad_posed, (size_t)n * NJ * 3);
  a.gjoints = fr.in(grad_joints, (size_t)n * NJ * 3);
  a.gbeta = fr.out(grad_beta, (size_t)n * NB, accumulate != 0);
  a.gpose0 = fr.out(grad_pose0, (size_t)n * (rot_in ? 3 : (NJ + 1) * 3), accumulate != 0);
  a.grot = rot_in ? fr.out(grad_rot, (size_t)n * NJ * 9, accumulate != 0) : nullptr;
  a.accumulate = accumulate;
  (void)trans;
  return fr.run([&] { return skel_launch(a, rot_in, true, fr.st); });
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_skeleton(smplpp_model * m, int64_t n, const float * beta, const float * theta, float * world, float * posed, float * joints,
                               int space, void * stream)
{
  return skel_forward_call("smplpp_skeleton", m, n, beta, nullptr, theta, false, world, posed, joints, space, stream);
}

extern "C" int smplpp_skeleton_rotmat(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot, float * world,
                                      float * posed, float * joints, int space, void * stream)
{
  return skel_forward_call("smplpp_skeleton_rotmat", m, n, beta, trans, rot, true, world, posed, joints, space, stream);
}

extern "C" int smplpp_skeleton_vjp(smplpp_model * m, int64_t n, const float * beta, const float * theta, const float * grad_world,
                                   const float * grad_posed, const float * grad_joints, float * grad_beta, float * grad_theta, int accumulate,
                                   int space, void * stream)
{
  return skel_backward_call("smplpp_skeleton_vjp", m, n, beta, nullptr, theta, false, grad_world, grad_posed, grad_joints, grad_beta, grad_theta,
                            nullptr, accumulate, space, stream);
}

extern "C" int smplpp_skeleton_rotmat_vjp(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot,
                                          const float * grad_world, const float * grad_posed, const float * grad_joints, float * grad_beta,
                                          float * grad_trans, float * grad_rot, int accumulate, int space, void * stream)
{
  return skel_backward_call("smplpp_skeleton_rotmat_vjp", m, n, beta, trans, rot, true, grad_world, grad_posed, grad_joints, grad_beta, grad_trans,
                            grad_rot, accumulate, space, stream);
}
