// smplpp_fk_jvp / smplpp_fk_rotmat_jvp: the Jacobian-vector product (forward mode) of smplpp_fk / smplpp_fk_rotmat and of the skeleton
// calls as gfx950 kernels.  Given tangents (dbeta, dtheta) or (dbeta, dtrans, drot) it returns the tangents of the vertices, of the
// rest joints and of the world joint frames.  No reference counterpart (the reference differentiates in reverse mode only).
//
// Per column = (frame, tangent), with R, J, A, g, G'_j = [A_j | t_j = g_j - A_j J_j], rest and wSum_v = sum_j w_vj as smplpp_fk has them:
//   dR_j    = sum_m dtheta[1+j][m] dRodrigues(theta_j)/dtheta_m  (rodrigues_grad.h; rotmat entry: drot[j] as given)
//   dJ      = JS dbeta                                           (the folded regressor; `djoints`)
//   drest_v = S_v dbeta + P_v vec(dR_j, j >= 1)                  (a row of the operand image BT against [vec dR | dbeta | 0])
//   dA_0 = dR_0, dg_0 = dJ_0;  level by level, joint j with parent p:
//     dA_j = dA_p R_j + A_p dR_j;   dg_j = dA_p (J_j - J_p) + A_p (dJ_j - dJ_p) + dg_p
//   dt_j    = dg_j - dA_j J_j - A_j dJ_j
//   dverts_v = ((sum_j w_vj dA_j) rest_v + sum_j w_vj dt_j + (sum_j w_vj A_j) drest_v) / wSum_v + dtrans
//   dworld_j = [dA_j | dg_j + dtrans]
//
// Kernels (on the caller's stream):
//  jvp_chain_kernel  ONE WAVEFRONT PER COLUMN, four columns per workgroup, no workgroup barrier (skeleton.hip's shape).  It runs the
//                    frame's forward chain itself from the functions the pose step is written in (pose_math.h: the same operations
//                    in the same order, so A, g and J have the forward's bits) beside its tangent, and writes djoints, dworld and,
//                    for the vertex pass, the column's coefficient row and its record [G' | dG' | dtrans].  A call without dverts is
//                    this kernel alone: one launch, no workspace, any tree smplpp_model_create accepts (levels wider than a
//                    wavefront take more passes).  The forward is recomputed per column instead of once per frame by a pose step
//                    of its own: it is a few hundred FMAs, and it keeps the chain-only call to one launch.
//  jvp_skin_kernel   the hot kernel, over (tile of 32 columns x chunk of vertex groups), a wavefront per group of 32 vertices:
//                    drest [32 vertices x 3][32 columns] = BT rows x coefficient rows on v_mfma_f32_32x32x2_f32 (fp32 operands
//                    carried exactly, fp32 accumulate, 336 MFMAs per group), then per (vertex, column) the blend of dG' and A from
//                    the sparse weight tables out of LDS and the three outputs, in fp32 VALU.
// No atomics and no sum across vertices, columns or workgroups: every output element is produced by one lane from its own column's
// record, so the bits of a column depend on its frame's inputs and its tangent only - not on n, T, its slot, `shared`, the
// memory space, the chunking or which outputs are asked for - and a column of NaNs stays in its column.
//
// The MFMA's contraction index is laid out for 16-byte loads: step (m, i) of 28 x 4 contracts k = 8 m + 4 h + i in lane half h, so a
// lane fetches four consecutive floats of its BT row and four of its coefficient row per four MFMAs.  The coefficient rows are
// written by jvp_chain_kernel in that order: coef [column tile][m 28][h 2][column 32][i 4].
#include "common.h"
#include "fk_vjp_state.h"
#include "pose_body.h"
#include "rodrigues_grad.h"
#include "staging.h"
#include "trace.h"

#include <algorithm>

namespace smplpp_hip
{
constexpr int JV_T = 4;                     // columns (wavefronts) per workgroup of jvp_chain_kernel
constexpr int JV_CT = 32;                   // columns per tile of jvp_skin_kernel (the MFMA's columns)
constexpr int JV_G = NJ * 12;               // a column's G' (and dG'), 3x4 row-major per joint
constexpr int JV_REC = 2 * JV_G + 4;        // record of a column: [G' | dG' | dtrans 3 | 0]
constexpr int JV_RS = JV_REC + 1;           // its LDS stride (odd: the 32 columns of a wavefront hit 32 banks)
constexpr int JV_TILE = VJ_KN * JV_CT;      // floats of a tile's coefficient rows
constexpr int JV_LDS = JV_CT * JV_RS * (int)sizeof(float);
constexpr int JV_PF = 4;                    // k-steps of eight whose operands jvp_skin_kernel keeps in flight

typedef float jv_f32x16 __attribute__((ext_vector_type(16)));

struct JvpArgs
{
  const float *beta, *pose;             // [n][10] (nullable: zeros), theta [n][25][3] or rot [n][24][9]
  const float *dbeta, *dpose, *dtrans;  // [tf][T][10], dtheta [tf][T][25][3] or drot [tf][T][24][9], rotmat entry: dtrans [tf][T][3] (nullable: zeros)
  const float * JSp;                    // [72][12] folded regressor rows [JS (10) | J0 | 0]
  const int32_t *parent, *lvl_off, *lvl_joint;
  int nlev, shared;
  int64_t ncol, T;
  float *djoints, *dworld;              // [ncol][24][3], [ncol][24][3][4] (nullable)
  float *coef, *rec;                    // the vertex pass's operands (nullable)
};

// the state of one column, one block per wavefront
struct JvpCol
{
  float R[NJ][9], J[NJ][3], dR[NJ][9], dJ[NJ][3];
  float G[NJ][12], dG[NJ][12]; // [A | g] and its tangent, 3x4 row-major
  float dtr[4];
};

template<bool ROT_IN>
__global__ __launch_bounds__(64 * JV_T) void jvp_chain_kernel(JvpArgs a)
{
#pragma clang fp contract(off)
  __shared__ JvpCol sC[JV_T];
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * JV_T + w;
  if(c >= a.ncol) return; // (wavefront-uniform; the kernel has no workgroup barrier)
  JvpCol & s = sC[w];
  const int64_t f = c / a.T, ti = a.shared ? c % a.T : c;
  // ---- rotations, joints and their tangents
  if(lane < NJ)
  {
    float R[9], dR[9];
#pragma unroll
    for(int q = 0; q < 9; q++) dR[q] = 0.0f;
    if constexpr(ROT_IN)
    {
#pragma unroll
      for(int q = 0; q < 9; q++) R[q] = a.pose[(f * NJ + lane) * 9 + q];
      if(a.dpose)
#pragma unroll
        for(int q = 0; q < 9; q++) dR[q] = a.dpose[(ti * NJ + lane) * 9 + q];
    }
    else
    {
      const float * th = a.pose + (f * (NJ + 1) + 1 + lane) * 3;
      rodrigues9(th[0], th[1], th[2], R);
      if(a.dpose)
      {
        const float * d = a.dpose + (ti * (NJ + 1) + 1 + lane) * 3;
        const float thl[3] = {th[0], th[1], th[2]};
        float g0[9], g1[9], g2[9];
        rodrigues_grad_dev(thl, 0, g0);
        rodrigues_grad_dev(thl, 1, g1);
        rodrigues_grad_dev(thl, 2, g2);
        const float d0 = d[0], d1 = d[1], d2 = d[2];
#pragma unroll
        for(int q = 0; q < 9; q++) dR[q] = __builtin_fmaf(d2, g2[q], __builtin_fmaf(d1, g1[q], d0 * g0[q]));
      }
    }
#pragma unroll
    for(int q = 0; q < 9; q++)
    {
      s.R[lane][q] = R[q];
      s.dR[lane][q] = dR[q];
    }
  }
  if(lane >= 24 && lane < 28)
  {
    const int x = lane - 24;
    float v = 0.0f;
    if(x < 3)
    {
      if constexpr(ROT_IN)
        v = a.dtrans ? a.dtrans[ti * 3 + x] : 0.0f;
      else
        v = a.dpose ? a.dpose[ti * ((NJ + 1) * 3) + x] : 0.0f;
    }
    s.dtr[x] = v;
  }
  {
    float be[NB], db[NB];
#pragma unroll
    for(int k = 0; k < NB; k++)
    {
      be[k] = a.beta ? a.beta[f * NB + k] : 0.0f;
      db[k] = a.dbeta ? a.dbeta[ti * NB + k] : 0.0f;
    }
    for(int t = lane; t < NJ * 3; t += 64)
    {
      const float4 * row = reinterpret_cast<const float4 *>(a.JSp + t * 12);
      const float4 u = row[0], v = row[1], x = row[2];
      const float js[NB] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w, x.x, x.y};
      s.J[t / 3][t % 3] = joint_coord(x.z, js, be);
      s.dJ[t / 3][t % 3] = joint_coord(0.0f, js, db);
    }
  }
  wave_sync();
  // ---- the chain and its tangent, one tree level at a time; lane = (joint of the level, entry of its 3x4)
  for(int L = 0; L < a.nlev; L++)
  {
    const int lo = a.lvl_off[L] * 12, hi = a.lvl_off[L + 1] * 12;
    for(int e = lo + lane; e < hi; e += 64)
    {
      const int i = a.lvl_joint[e / 12], p = a.parent[i], q = e % 12, r = q / 4, cc = q % 4;
      float v, dv;
      if(p < 0)
      {
        v = cc < 3 ? s.R[i][r * 3 + cc] : s.J[i][r];
        dv = cc < 3 ? s.dR[i][r * 3 + cc] : s.dJ[i][r];
      }
      else
      {
        float x[3], dx[3];
#pragma unroll
        for(int k = 0; k < 3; k++)
        {
          x[k] = cc < 3 ? s.R[i][k * 3 + cc] : s.J[i][k] - s.J[p][k];
          dx[k] = cc < 3 ? s.dR[i][k * 3 + cc] : s.dJ[i][k] - s.dJ[p][k];
        }
        const float * g = &s.G[p][r * 4];
        const float * dg = &s.dG[p][r * 4];
        v = chain_entry(g[0], g[1], g[2], g[3], x[0], x[1], x[2], cc == 3);
        dv = __builtin_fmaf(dg[2], x[2], __builtin_fmaf(dg[1], x[1], dg[0] * x[0])) +
             __builtin_fmaf(g[2], dx[2], __builtin_fmaf(g[1], dx[1], g[0] * dx[0]));
        if(cc == 3) dv = dv + dg[3];
      }
      s.G[i][q] = v;
      s.dG[i][q] = dv;
    }
    wave_sync();
  }
  // ---- outputs
  if(a.djoints)
    for(int t = lane; t < NJ * 3; t += 64) a.djoints[c * (NJ * 3) + t] = s.dJ[t / 3][t % 3];
  for(int e = lane; e < JV_G; e += 64)
  {
    const int i = e / 12, q = e % 12, r = q / 4, cc = q % 4;
    float v = s.G[i][q], dv = s.dG[i][q];
    if(a.dworld) a.dworld[c * JV_G + e] = cc == 3 ? dv + s.dtr[r] : dv;
    if(a.rec)
    {
      if(cc == 3) // relative transform: t = g - A J, dt = dg - dA J - A dJ
      {
        const float * A = &s.G[i][r * 4];
        const float * dA = &s.dG[i][r * 4];
        v = relative_t(v, A[0], A[1], A[2], s.J[i][0], s.J[i][1], s.J[i][2]);
        dv = dv - (__builtin_fmaf(dA[2], s.J[i][2], __builtin_fmaf(dA[1], s.J[i][1], dA[0] * s.J[i][0])) +
                   __builtin_fmaf(A[2], s.dJ[i][2], __builtin_fmaf(A[1], s.dJ[i][1], A[0] * s.dJ[i][0])));
      }
      a.rec[c * JV_REC + e] = v;
      a.rec[c * JV_REC + JV_G + e] = dv;
    }
  }
  if(a.rec && lane < 4) a.rec[c * JV_REC + 2 * JV_G + lane] = s.dtr[lane];
  if(a.coef)
  {
    float * out = a.coef + (c / JV_CT) * JV_TILE + (c % JV_CT) * 4;
    for(int k = lane; k < VJ_KN; k += 64)
    {
      float v = 0.0f;
      if(k < NP)
        v = s.dR[1 + k / 9][k % 9];
      else if(k < NP + NB)
        v = a.dbeta ? a.dbeta[ti * NB + (k - NP)] : 0.0f;
      out[(k / 4) * (JV_CT * 4) + k % 4] = v; // [m = k / 8][h = k / 4 % 2][column][i = k % 4]
    }
  }
}

// grid: nct column tiles x nch chunks of `gpc` vertex groups; the four wavefronts of a workgroup take one group each per round.
// Lane l = 32 h + r of a wavefront: column c0 + r; as the MFMA's A operand the BT rows of vertex r of the group, afterwards the
// vertices (i & 3) + 8 (i >> 2) + 4 h, i = 0..15, of that column.
template<int MAXW>
__global__ __launch_bounds__(256) void jvp_skin_kernel(const float * __restrict__ BT, const float * __restrict__ coef,
                                                    const float * __restrict__ rec, const float * __restrict__ rest,
                                                    const uint8_t * __restrict__ wIdx, const float * __restrict__ wVal,
                                                    const float * __restrict__ wSum, float * __restrict__ dverts, int64_t ncol, int64_t T,
                                                    int64_t V, int VGn, int gpc, int64_t nct)
{
#pragma clang fp contract(off)
  extern __shared__ float sRec[]; // [JV_CT][JV_RS]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int64_t ct = (int64_t)blockIdx.x % nct;
  const int chunk = (int)((int64_t)blockIdx.x / nct);
  const int64_t c0 = ct * JV_CT, c = c0 + r;
  const bool cok = c < ncol;
  for(int i = tid; i < JV_CT * JV_REC; i += 256)
  {
    const int cl = i / JV_REC, e = i % JV_REC;
    sRec[cl * JV_RS + e] = c0 + cl < ncol ? rec[(c0 + cl) * JV_REC + e] : 0.0f;
  }
  __syncthreads();
  const float * cq = coef + ct * JV_TILE + (h * JV_CT + r) * 4;
  const float * my = sRec + r * JV_RS;
  const int64_t f = cok ? c / T : 0;
  const float dt0 = my[2 * JV_G], dt1 = my[2 * JV_G + 1], dt2 = my[2 * JV_G + 2];
  const int g_end = min((chunk + 1) * gpc, VGn);
  for(int g = chunk * gpc + w; g < g_end; g += 4)
  {
    jv_f32x16 acc[3];
#pragma unroll
    for(int x = 0; x < 3; x++)
#pragma unroll
      for(int i = 0; i < 16; i++) acc[x][i] = 0.0f;
    // ---- drest of the group's 32 vertices x 32 columns: rows (v, x) of BT against the coefficient rows
    const float * ap = BT + ((int64_t)g * VG + r) * (3 * VJ_KN) + 4 * h;
    // The operands of step m + JV_PF are fetched while step m's twelve MFMAs run: BT comes from beyond L2 and a wavefront has the
    // SIMD to itself, so without the ring every step would wait out a memory latency.  (The barrier keeps the compiler from sinking
    // the loads to their use or hoisting all 112 of them.)
    float4 av[JV_PF][3], bv[JV_PF];
#pragma unroll
    for(int m = 0; m < JV_PF; m++)
    {
      bv[m] = cok ? *reinterpret_cast<const float4 *>(cq + m * (2 * JV_CT * 4)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for(int x = 0; x < 3; x++) av[m][x] = *reinterpret_cast<const float4 *>(ap + x * VJ_KN + 8 * m);
    }
#pragma unroll
    for(int m = 0; m < VJ_KN / 8; m++)
    {
      const int sl = m % JV_PF;
#pragma unroll
      for(int x = 0; x < 3; x++)
      {
        acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][x].x, bv[sl].x, acc[x], 0, 0, 0);
        acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][x].y, bv[sl].y, acc[x], 0, 0, 0);
        acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][x].z, bv[sl].z, acc[x], 0, 0, 0);
        acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][x].w, bv[sl].w, acc[x], 0, 0, 0);
      }
      if(m + JV_PF < VJ_KN / 8)
      {
        const int mn = m + JV_PF;
        bv[sl] = cok ? *reinterpret_cast<const float4 *>(cq + mn * (2 * JV_CT * 4)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for(int x = 0; x < 3; x++) av[sl][x] = *reinterpret_cast<const float4 *>(ap + x * VJ_KN + 8 * mn);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- per (vertex, column): blend A, dA and dt from the sparse weights, then the three outputs
    if(cok)
    {
#pragma unroll
      for(int i = 0; i < 16; i++)
      {
        const int64_t v = (int64_t)g * VG + (i & 3) + 8 * (i >> 2) + 4 * h;
        if(v >= V) continue;
        const float * q = rest + (f * V + v) * 3;
        const float rx = q[0], ry = q[1], rz = q[2];
        float M[9], dM[9], dT[3];
#pragma unroll
        for(int e = 0; e < 9; e++) M[e] = dM[e] = 0.0f;
        dT[0] = dT[1] = dT[2] = 0.0f;
        constexpr int WUNR = MAXW > 8 ? 2 : MAXW;
#pragma unroll WUNR
        for(int k = 0; k < MAXW; k++)
        {
          const float ww = wVal[v * MAXW + k];
          const float * G = my + (int)wIdx[v * MAXW + k] * 12;
          const float * dG = G + JV_G;
#pragma unroll
          for(int e = 0; e < 9; e++)
          {
            M[e] = __builtin_fmaf(ww, G[(e / 3) * 4 + e % 3], M[e]);
            dM[e] = __builtin_fmaf(ww, dG[(e / 3) * 4 + e % 3], dM[e]);
          }
#pragma unroll
          for(int e = 0; e < 3; e++) dT[e] = __builtin_fmaf(ww, dG[e * 4 + 3], dT[e]);
        }
        const float ws = wSum[v], d0 = acc[0][i], d1 = acc[1][i], d2 = acc[2][i];
        float * o = dverts + (c * V + v) * 3;
        const float tr[3] = {dt0, dt1, dt2};
#pragma unroll
        for(int e = 0; e < 3; e++)
        {
          const float s = (__builtin_fmaf(dM[e * 3 + 2], rz, __builtin_fmaf(dM[e * 3 + 1], ry, dM[e * 3] * rx)) + dT[e]) +
                          __builtin_fmaf(M[e * 3 + 2], d2, __builtin_fmaf(M[e * 3 + 1], d1, M[e * 3] * d0));
          o[e] = s / ws + tr[e];
        }
      }
    }
  }
}

template<int MAXW>
static hipError_t launch_jvp_skin(const smplpp_model * m, const float * BT, const float * coef, const float * rec, const float * rest,
                                  float * dverts, int64_t ncol, int64_t T, int64_t nct, int nch, int gpc, hipStream_t st)
{
  static PerDeviceOnce once;
  if(hipError_t e = lds_opt_in(once, m->device, reinterpret_cast<const void *>(&jvp_skin_kernel<MAXW>), JV_LDS)) return e;
  jvp_skin_kernel<MAXW><<<dim3((unsigned)(nct * nch)), dim3(256), JV_LDS, st>>>(BT, coef, rec, rest, m->wIdx.get(), m->wVal.get(), m->wSum.get(),
                                                                                 dverts, ncol, T, m->V, (int)m->VGn, gpc, nct);
  return hipGetLastError();
}

// rot_in (smplpp_fk_rotmat_jvp): pose = rot [n][24][9], dpose = drot, dtrans its own array; else pose = theta, dpose = dtheta
static int jvp_device(smplpp_model * m, int64_t n, int64_t T, const float * beta, const float * pose, const float * rest, const float * dbeta,
                      const float * dpose, const float * dtrans, int shared, bool rot_in, float * dverts, float * djoints, float * dworld,
                      hipStream_t st)
{
  const int64_t ncol = n * T, nct = (ncol + JV_CT - 1) / JV_CT;
  JvpArgs a = {};
  a.beta = beta;
  a.pose = pose;
  a.dbeta = dbeta;
  a.dpose = dpose;
  a.dtrans = dtrans;
  a.JSp = m->JSp.get();
  a.parent = m->parent.get();
  a.lvl_off = m->lvl.get();
  a.lvl_joint = m->lvl.get() + NJ + 1;
  a.nlev = m->nlev;
  a.shared = shared;
  a.ncol = ncol;
  a.T = T;
  a.djoints = djoints;
  a.dworld = dworld;
  const float * BT = nullptr;
  int nch = 0, gpc = 0;
  if(dverts)
  {
    VjpState * s = m->vjp.get();
    if(int rc = fk_vjp_image(m, st, &BT)) return rc;
    if(!rest)
      if(int rc = fk_vjp_rest(m, n, beta, pose, nullptr, rot_in, st, &rest)) return rc;
    HIP_TRY(s->jcoef.reserve(sizeof(float) * (size_t)nct * JV_TILE));
    HIP_TRY(s->jrec.reserve(sizeof(float) * (size_t)ncol * JV_REC));
    a.coef = s->jcoef.as<float>();
    a.rec = s->jrec.as<float>();
    // chunks of the vertex groups: about two workgroups per CU, a multiple of four groups each (the bits do not depend on it)
    const int64_t want = std::max<int64_t>(1, 2 * (int64_t)device_cus(m->device) / nct);
    gpc = (int)((m->VGn + want - 1) / want);
    gpc = std::max(4, (gpc + 3) / 4 * 4);
    nch = (int)((m->VGn + gpc - 1) / gpc);
  }
  const dim3 grid((unsigned)((ncol + JV_T - 1) / JV_T)), block(64 * JV_T);
  if(rot_in)
    jvp_chain_kernel<true><<<grid, block, 0, st>>>(a);
  else
    jvp_chain_kernel<false><<<grid, block, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  if(dverts)
  {
    switch(m->maxw)
    {
      case 4: HIP_TRY(launch_jvp_skin<4>(m, BT, a.coef, a.rec, rest, dverts, ncol, T, nct, nch, gpc, st)); break;
      case 8: HIP_TRY(launch_jvp_skin<8>(m, BT, a.coef, a.rec, rest, dverts, ncol, T, nct, nch, gpc, st)); break;
      default: HIP_TRY(launch_jvp_skin<NJ>(m, BT, a.coef, a.rec, rest, dverts, ncol, T, nct, nch, gpc, st)); break;
    }
  }
  return SMPLPP_OK;
}

static int jvp_call(const char * fn, smplpp_model * m, int64_t n, int64_t T, const float * beta, const float * pose, bool rot_in,
                    const float * rest, const float * dbeta, const float * dpose, const float * dtrans, int shared, float * dverts,
                    float * djoints, float * dworld, int space, void * stream)
{
  const std::string name(fn);
  if(!m) return fail(SMPLPP_ERR_INVALID, name + ": null model");
  if(n <= 0 || T <= 0) return fail(SMPLPP_ERR_INVALID, name + ": needs n > 0 and T > 0");
  if(!pose || (!rot_in && !beta)) return fail(SMPLPP_ERR_INVALID, name + (rot_in ? ": needs rot" : ": needs beta and theta"));
  if(!dbeta && !dpose && !dtrans) return fail(SMPLPP_ERR_INVALID, name + ": at least one tangent must be given");
  if(!dverts && !djoints && !dworld) return fail(SMPLPP_ERR_INVALID, name + ": at least one output must be asked for");
  if(shared != 0 && shared != 1) return fail(SMPLPP_ERR_INVALID, name + ": shared must be 0 or 1");
  if(int rc = check_space(space, fn)) return rc;
  if(n > 0x7fffffffLL || T > 0x7fffffffLL || n * T > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, name + ": too many columns (n T)");
  const int64_t ncol = n * T;
  if(dverts && (ncol + JV_CT - 1) / JV_CT * ((m->VGn + 3) / 4) > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, name + ": too many columns (n T)");
  Frame fr(m->device, &m->arena, space, stream, "tangent SMPL");
  if(!fr.ok()) return fr.finish();
  if(dverts)
    if(int rc = fk_vjp_state(m)) return rc;
  const size_t tc = (size_t)(shared ? T : ncol);
  const float * b = fr.in(beta, (size_t)n * NB);
  const float * p = fr.in(pose, (size_t)n * (rot_in ? NJ * 9 : (NJ + 1) * 3));
  const float * r = dverts ? fr.in(rest, (size_t)n * m->V * 3) : nullptr;
  const float * db = fr.in(dbeta, tc * NB);
  const float * dp = fr.in(dpose, tc * (rot_in ? NJ * 9 : (NJ + 1) * 3));
  const float * dt = fr.in(dtrans, tc * 3);
  float * dv = fr.out(dverts, (size_t)ncol * m->V * 3);
  float * dj = fr.out(djoints, (size_t)ncol * NJ * 3);
  float * dw = fr.out(dworld, (size_t)ncol * JV_G);
  return fr.run([&] { return jvp_device(m, n, T, b, p, r, db, dp, dt, shared, rot_in, dv, dj, dw, fr.st); });
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_fk_jvp(smplpp_model * m, int64_t n, int64_t T, const float * beta, const float * theta, const float * rest,
                             const float * dbeta, const float * dtheta, int shared, float * dverts, float * djoints, float * dworld, int space,
                             void * stream)
{
  return jvp_call("smplpp_fk_jvp", m, n, T, beta, theta, false, rest, dbeta, dtheta, nullptr, shared, dverts, djoints, dworld, space, stream);
}

extern "C" int smplpp_fk_rotmat_jvp(smplpp_model * m, int64_t n, int64_t T, const float * beta, const float * trans, const float * rot,
                                    const float * rest, const float * dbeta, const float * dtrans, const float * drot, int shared,
                                    float * dverts, float * djoints, float * dworld, int space, void * stream)
{
  (void)trans; // (no tangent depends on the root translation)
  return jvp_call("smplpp_fk_rotmat_jvp", m, n, T, beta, rot, true, rest, dbeta, drot, dtrans, shared, dverts, djoints, dworld, space, stream);
}
