// smplpp_fk_vjp: the vector-Jacobian product of smplpp_fk (the backward pass of SMPL::launch, src/SMPL.cpp:671-737, that the
// reference gets from libtorch autograd, e.g. node/node.cpp:823-869) as gfx950 kernels.
//
// Per frame, with g = dL/dverts, G' the relative transforms, R' their 3x3 part, w the skinning weights of vertex v and
// wSum_v = sum_j w_vj (the homogeneous divide of src/LinearBlendSkinning.cpp:545-550, constant per vertex on this path):
//   g~_v     = g_v / wSum_v
//   g_rest_v = sum_j w_vj R'_j^T g~_v                      dG'_j = sum_v w_vj g~_v [rest_v; 1]^T          g_root = sum_v g_v
//   g_c[k]   = sum_{v,x} basis[k](v,x) g_rest[v,x]         k < 207: pose coefficients (R_j - I, j = 1..23), 207..216: beta
// then dG' back through G'_j = [A_j | g_j - A_j J_j], A_j = A_p [R_j | J_j - J_p] (leaf to root), J = J0 + JS.beta, Rodrigues.
//
// Kernels (all on the caller's stream):
//  vjp_pose_kernel    the pose step of pose_body.h (the same instructions as pose_kernel, so the same bits), writing the frame's
//                     rotations, joints and G' into the backward's own workspace.
//  vjp_skin_kernel    the hot kernel, over (32-frame tile x chunk of vertex groups): per vertex the skinning backward in fp32 VALU
//                     from the sparse weight tables; g_rest goes straight into the matrix pipe as the A operand of the transposed
//                     blend GEMM [frames x 3V] x [3V x 224] against the operand image BT; dG' and g_root are reduced over the chunk's
//                     vertices in LDS / registers in a fixed order; one partial slab per (chunk, frame) goes to HBM.  No atomics.
//  vjp_chain_kernel   one workgroup per frame: sums the slabs in chunk order, runs the chain, joint-regression and Rodrigues
//                     backward (rodrigues_grad.h: the reference's ||theta + 1e-8|| form) and writes dL/dbeta, dL/dtheta.
//
// Arithmetic: the transposed GEMM runs on v_mfma_f32_32x32x2_f32 — fp32 operands carried exactly, fp32 accumulate.  (The bf16x3
// pieces of skin_e.hip would cut the matrix floor from ~58 to ~22 us at n = 1024 but add a three-way split of g_rest per (frame,
// vertex) in the VALU; the kernel is latency-bound, not matrix-bound: DESIGN.md 3.4.)  Everything else is fp32 VALU.  Same inputs -> same bits: every sum has a
// fixed order.
//
// Operand image BT [VGn*32*3][224] fp32, row (v, x) = [posedirs P[v][x][0..207) | shapedirs S[v][x][0..10) | 0 x 7]: the basis with
// the vertex coordinates along K.  Built from the vertex-major bases the model keeps (Pvm / Svm; the K-major Bm is freed by the
// default forms) on the first call on a model, owned by the model's backward state.
#include "common.h"
#include "fk_vjp_state.h"
#include "pose_body.h"
#include "rodrigues_grad.h"
#include "staging.h"
#include "trace.h"

#include <algorithm>

namespace smplpp_hip
{
int fk_device(smplpp_model * m, int64_t n, const float * beta, const float * theta, float * verts, float * joints, float * xforms44,
              float * rest, float * poserot, hipStream_t st, int range_slot, int * range_word, char form_override = 0);
PoseArgs fk_pose_args(smplpp_model * m, int64_t n, const float * beta, const float * theta, float * joints, float * poserot, float * xforms44,
                      bool with_ops);
int fk_rotmat_device(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot, float * verts, float * joints,
                     float * xforms44, float * rest, hipStream_t st, int range_slot, int * range_word);

constexpr int VJ_FT = 32;              // frames per workgroup of the hot kernel (the MFMA rows)
constexpr int VJ_NT = VJ_KN / 32;      // N tiles of the transposed GEMM
constexpr int VJ_RS = NJ * 9 + 1;      // LDS stride of a frame's 24 rotations (odd: the 32 frames of a wave hit 32 banks)
constexpr int VJ_RED = VJ_KN + 4;      // LDS row of the cross-wave reduction of the GEMM result
// partial slab of one (chunk, frame): [g_c 224 | dG' 24 x 3x4 | g_root 3 high parts | g_root 3 low parts | pad]
constexpr int VJ_DG = VJ_KN, VJ_ROOT = VJ_KN + NJ * 12, VJ_SLAB = VJ_ROOT + 8;

void StateDelete::operator()(VjpState * s) const
{
  delete s;
}

typedef float vj_f32x16 __attribute__((ext_vector_type(16)));

__global__ void vjp_image_kernel(const float * __restrict__ Pvm, const float * __restrict__ Svm, float * __restrict__ BT, int64_t V, int64_t rows)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= rows * VJ_KN) return;
  const int64_t row = i / VJ_KN; // v * 3 + x
  const int k = (int)(i % VJ_KN);
  float val = 0.0f;
  if(row < V * 3)
  {
    if(k < NP)
      val = Pvm[row * NP + k];
    else if(k < NP + NB)
      val = Svm[row * NB + (k - NP)];
  }
  BT[i] = val;
}

__global__ __launch_bounds__(256) void vjp_pose_kernel(PoseArgs a)
{
  const int64_t f = blockIdx.x;
  if(f >= a.n) return;
  pose_body(a, f, (int)threadIdx.x, a.theta + f * ((NJ + 1) * 3));
}

// smplpp_fk_rotmat_vjp's pose step: the rotation-input instantiation (a.theta = rot [n][24][9])
__global__ __launch_bounds__(256) void vjp_pose_kernel_rot(PoseArgs a)
{
  const int64_t f = blockIdx.x;
  if(f >= a.n) return;
  pose_body<true>(a, f, (int)threadIdx.x, a.theta + f * (NJ * 9));
}

// grid: nft frame tiles x nch chunks of `gpc` vertex groups (gpc a multiple of 4: the four wavefronts take one group each per round).
// Lane l = 32 h + r of a wavefront: frame f0 + r; in the skinning phase the vertices 2i + h of the half group, in the dG' phase the
// entries b = 2h, 2h + 1 of [rest; 1].
template<int MAXW>
__global__ __launch_bounds__(256, 2) void vjp_skin_kernel(const float * __restrict__ BT, const float * __restrict__ Gp,
                                                       const float * __restrict__ rest, const float * __restrict__ gv,
                                                       const uint8_t * __restrict__ wIdx, const float * __restrict__ wVal,
                                                       const float * __restrict__ wSum, const float * __restrict__ Wdense,
                                                       float * __restrict__ slab, int64_t n, int64_t V, int VGn, int gpc, int nft)
{
  __shared__ float sR[VJ_FT * VJ_RS];             // R' of the tile's frames
  __shared__ __align__(16) float sT[4][16][6][VJ_FT]; // per wavefront, the half group's g~ (3) and rest (3) for the dG' phase
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int ftile = blockIdx.x % nft, chunk = blockIdx.x / nft;
  const int64_t f0 = (int64_t)ftile * VJ_FT, f = f0 + r;
  const bool fok = f < n;
  for(int i = tid; i < VJ_FT * NJ * 9; i += 256)
  {
    const int fl = i / (NJ * 9), e = i % (NJ * 9), j = e / 9, q = e % 9;
    const int64_t ff = f0 + fl;
    sR[fl * VJ_RS + e] = ff < n ? Gp[(ff * NJ + j) * 12 + (q / 3) * 4 + q % 3] : 0.0f;
  }
  __syncthreads();

  vj_f32x16 acc[VJ_NT];
#pragma unroll
  for(int t = 0; t < VJ_NT; t++)
#pragma unroll
    for(int i = 0; i < 16; i++) acc[t][i] = 0.0f;
  float dg[6][3][2];
#pragma unroll
  for(int jj = 0; jj < 6; jj++)
#pragma unroll
    for(int a = 0; a < 3; a++) dg[jj][a][0] = dg[jj][a][1] = 0.0f;
  float gr0 = 0.0f, gr1 = 0.0f, gr2 = 0.0f;
  const float * sRf = sR + r * VJ_RS;
  const int g_begin = chunk * gpc, g_end = min(g_begin + gpc, VGn);

  for(int g0 = g_begin; g0 < g_end; g0 += 4)
  {
    const int g = g0 + w;
    const bool gok = g < g_end;
    for(int hf = 0; hf < 2; hf++)
    {
      // ---- skinning backward, one vertex per (lane, i)
      float grest[8][3];
#pragma unroll
      for(int i = 0; i < 8; i++)
      {
        const int vl = 2 * i + h;
        const int64_t v = (int64_t)g * VG + 16 * hf + vl;
        const bool vok = gok && v < V;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f;
        if(vok && fok)
        {
          const float * p = gv + (f * V + v) * 3;
          const float * q = rest + (f * V + v) * 3;
          gx = p[0]; gy = p[1]; gz = p[2];
          rx = q[0]; ry = q[1]; rz = q[2];
        }
        const float wi = vok ? 1.0f / wSum[v] : 0.0f;
        const float tx = gx * wi, ty = gy * wi, tz = gz * wi;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        if(vok)
        {
          constexpr int WUNR = MAXW > 8 ? 2 : MAXW; // (dense weights: a full unroll spills beside the accumulators)
#pragma unroll WUNR
          for(int q = 0; q < MAXW; q++)
          {
            const float ww = wVal[v * MAXW + q];
            const float * R = sRf + (int)wIdx[v * MAXW + q] * 9;
            a0 += ww * ((R[0] * tx + R[3] * ty) + R[6] * tz);
            a1 += ww * ((R[1] * tx + R[4] * ty) + R[7] * tz);
            a2 += ww * ((R[2] * tx + R[5] * ty) + R[8] * tz);
          }
        }
        grest[i][0] = a0;
        grest[i][1] = a1;
        grest[i][2] = a2;
        gr0 += gx;
        gr1 += gy;
        gr2 += gz;
        float * st = &sT[w][vl][0][r];
        st[0 * VJ_FT] = tx; st[1 * VJ_FT] = ty; st[2 * VJ_FT] = tz;
        st[3 * VJ_FT] = rx; st[4 * VJ_FT] = ry; st[5 * VJ_FT] = rz;
      }
      // ---- transposed blend GEMM: A[frame r][k = h] = g_rest of vertex 2i + h, B[k = h][col r] = BT row of that vertex
      if(gok)
      {
        const float * Bp = BT + ((int64_t)g * VG + 16 * hf + h) * 3 * VJ_KN + r;
#pragma unroll
        for(int i = 0; i < 8; i++)
        {
          __builtin_amdgcn_sched_barrier(0); // (keeps the compiler from hoisting all 168 basis loads of the half group: registers)
#pragma unroll
          for(int x = 0; x < 3; x++)
          {
            const float * b = Bp + (int64_t)(2 * i * 3 + x) * VJ_KN;
            float bv[VJ_NT];
#pragma unroll
            for(int t = 0; t < VJ_NT; t++) bv[t] = b[32 * t];
#pragma unroll
            for(int t = 0; t < VJ_NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(grest[i][x], bv[t], acc[t], 0, 0, 0);
          }
        }
      }
      __syncthreads(); // sT of all four wavefronts complete
      // ---- dG': wavefront w owns joints 6w .. 6w+5 over the round's vertices (weight tests are wavefront-uniform)
      for(int ww = 0; ww < 4; ww++)
      {
        const int gg = g0 + ww;
        if(gg >= g_end) break;
        for(int vi = 0; vi < 16; vi++)
        {
          const int64_t v = (int64_t)gg * VG + 16 * hf + vi;
          if(v >= V) break;
          const float * Wr = Wdense + v * NJ + 6 * w;
          const float * st = &sT[ww][vi][0][r];
#pragma unroll
          for(int jj = 0; jj < 6; jj++)
          {
            const float wt = Wr[jj];
            if(wt != 0.0f)
            {
              const float t0 = st[0], t1 = st[VJ_FT], t2 = st[2 * VJ_FT];
              const float rb0 = st[(3 + 2 * h) * VJ_FT], rb1 = h ? 1.0f : st[4 * VJ_FT];
              const float w0 = wt * t0, w1 = wt * t1, w2 = wt * t2;
              dg[jj][0][0] += w0 * rb0; dg[jj][0][1] += w0 * rb1;
              dg[jj][1][0] += w1 * rb0; dg[jj][1][1] += w1 * rb1;
              dg[jj][2][0] += w2 * rb0; dg[jj][2][1] += w2 * rb1;
            }
          }
        }
      }
      __syncthreads(); // sT free for the next round
    }
  }

  // ---- the workgroup's partial slab
  float * red = &sT[0][0][0][0]; // [32 frames][VJ_RED]
  // g_root = sum_v g_v cancels (dense cotangents: |sum| ~ sum|g| / 66).  A lane's own sum stays fp32 (at most 64 terms); from here on
  // the partial sums are large beside the result, so the eight lanes of a frame, and the chunks in vjp_chain_kernel, are added in double.
  double * sRoot = reinterpret_cast<double *>(red + VJ_FT * VJ_RED); // [4 wavefronts][2 parities][32 frames][3], behind `red` in sT
  static_assert((VJ_FT * VJ_RED) % 4 == 0 && sizeof(float) * VJ_FT * VJ_RED + sizeof(double) * 8 * VJ_FT * 3 <= sizeof(sT), "sT holds both");
  sRoot[((w * 2 + h) * VJ_FT + r) * 3 + 0] = (double)gr0;
  sRoot[((w * 2 + h) * VJ_FT + r) * 3 + 1] = (double)gr1;
  sRoot[((w * 2 + h) * VJ_FT + r) * 3 + 2] = (double)gr2;
  for(int ww = 0; ww < 4; ww++)  // wavefront order: fixed
  {
    if(w == ww)
#pragma unroll
      for(int t = 0; t < VJ_NT; t++)
#pragma unroll
        for(int i = 0; i < 16; i++)
        {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * h, idx = row * VJ_RED + 32 * t + r;
          red[idx] = ww == 0 ? acc[t][i] : red[idx] + acc[t][i];
        }
    __syncthreads();
  }
  float * out = slab + ((int64_t)chunk * n + f0) * VJ_SLAB;
  for(int e = tid; e < VJ_FT * VJ_KN; e += 256)
  {
    const int fl = e / VJ_KN, c = e % VJ_KN;
    if(f0 + fl < n) out[(int64_t)fl * VJ_SLAB + c] = red[fl * VJ_RED + c];
  }
  if(tid < VJ_FT * 3)
  {
    const int fl = tid / 3, x = tid % 3;
    double s = 0.0;
    for(int ww = 0; ww < 4; ww++) s = (s + sRoot[((ww * 2 + 0) * VJ_FT + fl) * 3 + x]) + sRoot[((ww * 2 + 1) * VJ_FT + fl) * 3 + x];
    if(f0 + fl < n) // the chunk's sum as an fp32 pair (48 bits)
    {
      const float hi = (float)s;
      out[(int64_t)fl * VJ_SLAB + VJ_ROOT + x] = hi;
      out[(int64_t)fl * VJ_SLAB + VJ_ROOT + 3 + x] = (float)(s - (double)hi);
    }
  }
  if(fok)
  {
    float * o = out + (int64_t)r * VJ_SLAB + VJ_DG;
#pragma unroll
    for(int jj = 0; jj < 6; jj++)
#pragma unroll
      for(int a = 0; a < 3; a++)
      {
        o[(6 * w + jj) * 12 + a * 4 + 2 * h] = dg[jj][a][0];
        o[(6 * w + jj) * 12 + a * 4 + 2 * h + 1] = dg[jj][a][1];
      }
  }
}

// one workgroup per frame.  nch = 0: no vertex gradient (the slabs are not read).
// ROT_OUT (smplpp_fk_rotmat_vjp): `rot` is the caller's rot [n][24][9], `theta` unused; instead of contracting dL/dR with the Rodrigues
// derivative the kernel writes it, nine independent entries per joint, to gtheta = grad_rot [n][24][9], and the root sum to gtrans [n][3]
// (either may be null).  Everything up to there is the same code in the same order: the same bits.
template<bool ROT_OUT>
__global__ __launch_bounds__(256) void vjp_chain_kernel(const float * __restrict__ slab, int nch, const float * __restrict__ Gp,
                                                     const float * __restrict__ joints, const float * __restrict__ rot,
                                                     const float * __restrict__ theta, const float * __restrict__ gj,
                                                     const float * __restrict__ JS, const int32_t * __restrict__ parent,
                                                     float * __restrict__ gbeta, float * __restrict__ gtheta,
                                                     float * __restrict__ gtrans, int64_t n)
{
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ float sS[VJ_SLAB];
  __shared__ float sG[NJ][12], sJ[NJ][3], sRot[NJ][9];
  __shared__ float dA[NJ][9], dgt[NJ][3], dJ[NJ][3], dR[NJ][9], cA[NJ][9], cJ[NJ][3];
  __shared__ int sPar[NJ], sDep[NJ], sMaxDep;
  for(int t = tid; t < VJ_ROOT; t += 256)
  {
    float s = 0.0f;
    for(int c = 0; c < nch; c++) s += slab[((int64_t)c * n + f) * VJ_SLAB + t];
    sS[t] = s;
  }
  if(tid >= 256 - 3) // g_root: the chunks' pairs summed in double in chunk order, rounded once
  {
    const int t = VJ_ROOT + tid - (256 - 3);
    double s = 0.0;
    for(int c = 0; c < nch; c++)
    {
      const float * p = slab + ((int64_t)c * n + f) * VJ_SLAB + t;
      s += (double)p[0] + (double)p[3];
    }
    sS[t] = (float)s;
  }
  for(int t = tid; t < NJ * 12; t += 256) sG[t / 12][t % 12] = Gp[f * NJ * 12 + t];
  for(int t = tid; t < NJ * 9; t += 256) sRot[t / 9][t % 9] = rot[f * NJ * 9 + t];
  if(tid < NJ * 3) sJ[tid / 3][tid % 3] = joints[f * NJ * 3 + tid];
  if(tid < NJ) sPar[tid] = parent[tid];
  __syncthreads();
  if(tid == 0) // depths (parents precede their children: smplpp_model_create)
  {
    int md = 0;
    for(int i = 0; i < NJ; i++)
    {
      const int p = sPar[i];
      sDep[i] = p < 0 ? 0 : sDep[p] + 1;
      md = max(md, sDep[i]);
    }
    sMaxDep = md;
  }
  const int j = tid;
  if(j < NJ)
  {
    // G'_j = [A | g - A J]: dA = dA' - dt J^T, dg = dt, dJ = -A^T dt (+ the caller's dL/djoints)
    const float * d = sS + VJ_DG + j * 12;
    const float dt0 = d[3], dt1 = d[7], dt2 = d[11];
#pragma unroll
    for(int a = 0; a < 3; a++)
#pragma unroll
      for(int c = 0; c < 3; c++) dA[j][a * 3 + c] = d[a * 4 + c] - d[a * 4 + 3] * sJ[j][c];
    dgt[j][0] = dt0; dgt[j][1] = dt1; dgt[j][2] = dt2;
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      const float s = -((sG[j][c] * dt0 + sG[j][4 + c] * dt1) + sG[j][8 + c] * dt2);
      dJ[j][c] = gj ? s + gj[(f * NJ + j) * 3 + c] : s;
    }
#pragma unroll
    for(int q = 0; q < 9; q++) dR[j][q] = j >= 1 ? sS[9 * (j - 1) + q] : 0.0f; // pose coefficients: R_j - I, j >= 1
  }
  __syncthreads();
  for(int L = sMaxDep; L >= 1; L--)
  {
    // A_j = A_p R_j, g_j = A_p (J_j - J_p) + g_p
    if(j < NJ && sDep[j] == L)
    {
      const int p = sPar[j];
      float Ap[9], dj[3];
#pragma unroll
      for(int a = 0; a < 3; a++)
#pragma unroll
        for(int c = 0; c < 3; c++) Ap[a * 3 + c] = sG[p][a * 4 + c];
#pragma unroll
      for(int c = 0; c < 3; c++) dj[c] = sJ[j][c] - sJ[p][c];
#pragma unroll
      for(int c = 0; c < 3; c++)
#pragma unroll
        for(int e = 0; e < 3; e++) dR[j][c * 3 + e] += (Ap[c] * dA[j][e] + Ap[3 + c] * dA[j][3 + e]) + Ap[6 + c] * dA[j][6 + e];
#pragma unroll
      for(int a = 0; a < 3; a++)
#pragma unroll
        for(int c = 0; c < 3; c++)
          cA[j][a * 3 + c] = ((dA[j][a * 3] * sRot[j][c * 3] + dA[j][a * 3 + 1] * sRot[j][c * 3 + 1]) + dA[j][a * 3 + 2] * sRot[j][c * 3 + 2]) +
                             dgt[j][a] * dj[c];
#pragma unroll
      for(int c = 0; c < 3; c++)
      {
        cJ[j][c] = (Ap[c] * dgt[j][0] + Ap[3 + c] * dgt[j][1]) + Ap[6 + c] * dgt[j][2];
        dJ[j][c] += cJ[j][c];
      }
    }
    __syncthreads();
    if(j < NJ && sDep[j] == L - 1) // children in ascending joint order
      for(int i = 0; i < NJ; i++)
        if(sPar[i] == j)
        {
#pragma unroll
          for(int q = 0; q < 9; q++) dA[j][q] += cA[i][q];
#pragma unroll
          for(int c = 0; c < 3; c++)
          {
            dgt[j][c] += dgt[i][c];
            dJ[j][c] -= cJ[i][c];
          }
        }
    __syncthreads();
  }
  if(j < NJ && sDep[j] == 0) // root: A = R, g = J
  {
#pragma unroll
    for(int q = 0; q < 9; q++) dR[j][q] += dA[j][q];
#pragma unroll
    for(int c = 0; c < 3; c++) dJ[j][c] += dgt[j][c];
  }
  __syncthreads();
  if(gbeta && tid < NB) // J = J0 + JS beta; the shape coefficients of the blend GEMM
  {
    float s = sS[K_BETA + tid];
    for(int i = 0; i < NJ * 3; i++) s += JS[i * NB + tid] * dJ[i / 3][i % 3];
    gbeta[f * NB + tid] = s;
  }
  if constexpr(ROT_OUT)
  {
    if(gtheta && tid < NJ * 9) gtheta[f * (NJ * 9) + tid] = dR[tid / 9][tid % 9];
    if(gtrans && tid >= 224 && tid < 227) gtrans[f * 3 + (tid - 224)] = sS[VJ_ROOT + tid - 224];
    return;
  }
  if(gtheta && tid >= 64 && tid < 64 + NJ * 3)
  {
    const int t = tid - 64, jj = t / 3, m = t % 3;
    float th[3], dRdt[9];
    for(int c = 0; c < 3; c++) th[c] = theta[(f * (NJ + 1) + 1 + jj) * 3 + c];
    rodrigues_grad_dev(th, m, dRdt);
    float s = 0.0f;
    for(int q = 0; q < 9; q++) s += dR[jj][q] * dRdt[q];
    gtheta[(f * (NJ + 1) + 1 + jj) * 3 + m] = s;
  }
  if(gtheta && tid >= 160 && tid < 163) gtheta[f * (NJ + 1) * 3 + (tid - 160)] = sS[VJ_ROOT + tid - 160];
}

template<int MAXW>
static hipError_t launch_vjp_skin(const smplpp_model * m, const VjpState * s, int64_t n, const float * rest, const float * gv, float * slab,
                                  int nft, int nch, int gpc, hipStream_t st)
{
  vjp_skin_kernel<MAXW><<<dim3((unsigned)(nft * nch)), dim3(256), 0, st>>>(s->BT.get(), s->Gp.as<float>(), rest, gv, m->wIdx.get(), m->wVal.get(),
                                                                            m->wSum.get(), m->Wdense.get(), slab, n, m->V, (int)m->VGn, gpc, nft);
  return hipGetLastError();
}

// chunking of the vertex groups: about two workgroups per CU, chunks of a multiple of four groups
static void vjp_chunks(const smplpp_model * m, int64_t n, int & nft, int & nch, int & gpc)
{
  nft = (int)((n + VJ_FT - 1) / VJ_FT);
  const int want = std::max(1, 2 * device_cus(m->device) / nft);
  gpc = (int)((m->VGn + want - 1) / want);
  gpc = std::max(4, (gpc + 3) / 4 * 4);
  nch = (int)((m->VGn + gpc - 1) / gpc);
}

// rot_in (smplpp_fk_rotmat_vjp): `theta` is rot [n][24][9], `trans` [n][3] (nullable) the root translation, gtheta = grad_rot
// [n][24][9] and gtrans = grad_trans [n][3]
int fk_vjp_image(smplpp_model * m, hipStream_t st, const float ** BT)
{
  VjpState * s = m->vjp.get();
  if(!s->BT)
  {
    const int64_t rows = m->VGn * VG * 3;
    HIP_TRY(dev_alloc(s->BT, (size_t)rows * VJ_KN));
    vjp_image_kernel<<<dim3((unsigned)((rows * VJ_KN + 255) / 256)), dim3(256), 0, st>>>(m->Pvm.get(), m->Svm.get(), s->BT.get(), m->V, rows);
    HIP_TRY(hipGetLastError());
  }
  *BT = s->BT.get();
  return SMPLPP_OK;
}

int fk_vjp_rest(smplpp_model * m, int64_t n, const float * beta, const float * pose, const float * trans, bool rot_in, hipStream_t st,
                const float ** rest)
{
  // the model's forward form into the backward's own workspace: smplpp_fk's workspace, range words and profiling record stay as they were
  VjpState * s = m->vjp.get();
  HIP_TRY(s->rest.reserve(sizeof(float) * (size_t)n * m->V * 3));
  std::swap(m->ws, s->fws);
  const bool prof = m->profiling;
  m->profiling = false;
  int rc = rot_in ? fk_rotmat_device(m, n, beta, trans, pose, nullptr, nullptr, nullptr, s->rest.as<float>(), st, RANGE_DEVICE,
                                     s->range_word.get())
                  : fk_device(m, n, beta, pose, nullptr, nullptr, nullptr, s->rest.as<float>(), nullptr, st, RANGE_DEVICE, s->range_word.get());
  m->profiling = prof;
  std::swap(m->ws, s->fws);
  if(rc) return rc;
  *rest = s->rest.as<float>();
  return SMPLPP_OK;
}

static int vjp_device(smplpp_model * m, int64_t n, const float * beta, const float * theta, const float * rest, const float * gv,
                      const float * gj, float * gbeta, float * gtheta, hipStream_t st, bool rot_in = false, const float * trans = nullptr,
                      float * gtrans = nullptr)
{
  VjpState * s = m->vjp.get();
  const float * BT = nullptr; // (launch_vjp_skin reads it from the state)
  if(int rc = fk_vjp_image(m, st, &BT)) return rc;
  if(gv && !rest)
    if(int rc = fk_vjp_rest(m, n, beta, theta, trans, rot_in, st, &rest)) return rc;
  HIP_TRY(s->Gp.reserve(sizeof(float) * (size_t)n * NJ * 12));
  HIP_TRY(s->joints.reserve(sizeof(float) * (size_t)n * NJ * 3));
  if(!rot_in) HIP_TRY(s->rot.reserve(sizeof(float) * (size_t)n * NJ * 9));
  // (rotation input: the chain kernel reads the caller's matrices, no copy)
  PoseArgs pa = fk_pose_args(m, n, beta, theta, s->joints.as<float>(), rot_in ? nullptr : s->rot.as<float>(), nullptr, false);
  pa.Gp = s->Gp.as<float>();
  pa.A3 = nullptr;
  pa.AT = nullptr;
  pa.gscale = 1.0f;
  pa.range_flag = nullptr;
  if(rot_in)
    vjp_pose_kernel_rot<<<dim3((unsigned)n), dim3(256), 0, st>>>(pa);
  else
    vjp_pose_kernel<<<dim3((unsigned)n), dim3(256), 0, st>>>(pa);
  HIP_TRY(hipGetLastError());
  int nft = 0, nch = 0, gpc = 0;
  if(gv)
  {
    vjp_chunks(m, n, nft, nch, gpc);
    HIP_TRY(s->slab.reserve(sizeof(float) * (size_t)nch * n * VJ_SLAB));
    float * slab = s->slab.as<float>();
    switch(m->maxw)
    {
      case 4: HIP_TRY(launch_vjp_skin<4>(m, s, n, rest, gv, slab, nft, nch, gpc, st)); break;
      case 8: HIP_TRY(launch_vjp_skin<8>(m, s, n, rest, gv, slab, nft, nch, gpc, st)); break;
      default: HIP_TRY(launch_vjp_skin<NJ>(m, s, n, rest, gv, slab, nft, nch, gpc, st)); break;
    }
  }
  if(rot_in)
    vjp_chain_kernel<true><<<dim3((unsigned)n), dim3(256), 0, st>>>(gv ? s->slab.as<float>() : nullptr, gv ? nch : 0, s->Gp.as<float>(),
                                                                   s->joints.as<float>(), theta, nullptr, gj, m->JS.get(), m->parent.get(),
                                                                   gbeta, gtheta, gtrans, n);
  else
    vjp_chain_kernel<false><<<dim3((unsigned)n), dim3(256), 0, st>>>(gv ? s->slab.as<float>() : nullptr, gv ? nch : 0, s->Gp.as<float>(),
                                                                    s->joints.as<float>(), s->rot.as<float>(), theta, gj, m->JS.get(),
                                                                    m->parent.get(), gbeta, gtheta, nullptr, n);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}
// the backward state of a model, created by the first backward call on it
int fk_vjp_state(smplpp_model * m)
{
  if(!m->vjp)
  {
    StatePtr<VjpState> s(new VjpState());
    HIP_TRY(dev_alloc(s->range_word, 1));
    HIP_TRY(hipMemset(s->range_word.get(), 0, sizeof(int)));
    m->vjp = std::move(s);
  }
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_fk_vjp(smplpp_model * m, int64_t n, const float * beta, const float * theta, const float * rest, const float * grad_verts,
                             const float * grad_joints, float * grad_beta, float * grad_theta, int space, void * stream)
{
  if(!m) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_vjp: null model");
  if(n <= 0 || !beta || !theta) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_vjp: needs n > 0, beta and theta");
  if(int rc = check_space(space, "smplpp_fk_vjp")) return rc;
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_vjp: too many frames");
  Frame fr(m->device, &m->arena, space, stream, "backward SMPL");
  if(!fr.ok()) return fr.finish();
  if(int rc = fk_vjp_state(m)) return rc;
  if(!grad_beta && !grad_theta) return SMPLPP_OK;
  if(space == SMPLPP_DEVICE)
    return fr.run([&] { return vjp_device(m, n, beta, theta, rest, grad_verts, grad_joints, grad_beta, grad_theta, fr.st); });

  const size_t nb = (size_t)n * NB, nt = (size_t)n * (NJ + 1) * 3, nv = (size_t)n * m->V * 3;
  const float * b = fr.in(beta, nb);
  const float * t = fr.in(theta, nt);
  const float * r = grad_verts ? fr.in(rest, nv) : nullptr;
  const float * gv = fr.in(grad_verts, nv);
  const float * gj = fr.in(grad_joints, (size_t)n * NJ * 3);
  float * gb = fr.out(grad_beta, nb);
  float * gt = fr.out(grad_theta, nt);
  return fr.run([&] { return vjp_device(m, n, b, t, r, gv, gj, gb, gt, fr.st); });
}

extern "C" int smplpp_fk_rotmat_vjp(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot, const float * rest,
                                    const float * grad_verts, const float * grad_joints, float * grad_beta, float * grad_trans,
                                    float * grad_rot, int space, void * stream)
{
  if(!m) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_rotmat_vjp: null model");
  if(n <= 0 || !rot) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_rotmat_vjp: needs n > 0 and rot");
  if(int rc = check_space(space, "smplpp_fk_rotmat_vjp")) return rc;
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, "smplpp_fk_rotmat_vjp: too many frames");
  Frame fr(m->device, &m->arena, space, stream, "backward SMPL");
  if(!fr.ok()) return fr.finish();
  if(int rc = fk_vjp_state(m)) return rc;
  if(!grad_beta && !grad_trans && !grad_rot) return SMPLPP_OK;
  // `trans` is not read: neither the rest shape nor any of the three gradients depends on it (and the call stages eight arguments)
  (void)trans;
  if(space == SMPLPP_DEVICE)
    return fr.run(
        [&] { return vjp_device(m, n, beta, rot, rest, grad_verts, grad_joints, grad_beta, grad_rot, fr.st, true, nullptr, grad_trans); });

  const size_t nb = (size_t)n * NB, nr = (size_t)n * NJ * 9, nv = (size_t)n * m->V * 3;
  const float * b = fr.in(beta, nb);
  const float * ro = fr.in(rot, nr);
  const float * r = grad_verts ? fr.in(rest, nv) : nullptr;
  const float * gv = fr.in(grad_verts, nv);
  const float * gj = fr.in(grad_joints, (size_t)n * NJ * 3);
  float * gb = fr.out(grad_beta, nb);
  float * gt = fr.out(grad_trans, (size_t)n * 3);
  float * gr = fr.out(grad_rot, nr);
  return fr.run([&] { return vjp_device(m, n, b, ro, r, gv, gj, gb, gr, fr.st, true, nullptr, gt); });
}
