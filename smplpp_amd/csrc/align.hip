// Rigid and similarity alignment of point sets: per frame the weighted least-squares R, t, s with s (R x) + t ~ y, in
// closed form (Horn's quaternion method: the top eigenvector of a symmetric 4 x 4 matrix by cyclic Jacobi), and its vector-Jacobian
// product to both point sets, also in closed form.  The rules are in include/smplpp_hip.h; every fp32 operation below is rounded on its
// own (no contraction to FMA), every sum over a frame's points is sum1024 of fixed_sum.h (whose two facts about +0 let the work split
// follow K), divisions and square roots are the correctly rounded ones, and there are no floating-point atomics.  The calls take no
// handle.
//
//  aln_forward_kernel<NQ>   three passes over the frame's points: centroids (7 sums), moments (10 sums), outputs (1 sum).
//  aln_backward_kernel<NQ>  the same first two passes by the same device functions, so the bits match; then the twelve sums of the
//                           cotangents, the closed form once per frame, and a last pass that writes both gradients.
// NQ = 0: K <= 64, a wavefront per frame, lane k owns point k.  NQ = 4 or 1: a workgroup per frame of 256 or 1024 threads by
// frame_sum_split, thread t owns the partials t + T q.  Between the passes every thread solves the frame's 4 x 4 problem alike, in
// registers (the Jacobi rotations are unrolled, every matrix index a constant): no divergence inside a frame, no broadcast.
#include "fixed_sum.h"
#include "staging.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int ALN_T = 256;        // threads of the wavefront-per-frame form: four frames a workgroup
constexpr int ALN_SWEEPS = 7;     // Jacobi sweeps: a constant of the rule (DESIGN §3.25 has the measurement behind it)
constexpr int ALN_MOMENT_SUMS = 17, ALN_FWD_SUMS = ALN_MOMENT_SUMS + 1, ALN_BWD_SUMS = ALN_MOMENT_SUMS + 12;
constexpr int64_t ALN_INT32_MAX = 0x7fffffffLL;
// floats of LDS of a kernel with `sums` sums in the form nq (AlnLds)
constexpr int aln_lds_floats(int nq, int sums)
{
  return nq == 0 ? 1 : nq == 1 ? 2 * 3 * 16 : sums * (1024 / nq / 64);
}

struct AlnArgs
{
  const float *x, *y, *w;
  int K;
  int y_per_frame, w_per_frame; // 0: shared by all frames (Tn, Wn = 1)
  int with_scale;
  float min_gap;
};
struct AlnOut
{
  float *transform, *aligned, *energy, *point_error, *gap;
  int32_t * status;
};
// the cotangents of transform [n,13], aligned [n,K,3] and energy [n]; each may be null
struct AlnCot
{
  const float *gtr, *gal, *ge;
};

struct AlnPoint
{
  float x[3], y[3], w;
  bool live, moved; // moved: the three source coordinates are finite
};

// what a frame's threads all hold after the first two passes and the solve
struct AlnFrame
{
  float W, cx[3], cy[3], S[9], vx; // S[3 a + b] = sum w x~_a y~_b
  float lam[4], V[4][4], q[4];     // every eigenpair (column i of V belongs to lam[i]); q: the normalised top eigenvector
  int top;
  float R[9], t[3], s, gap;
  int status;
};

__device__ inline bool aln_finite(float v)
{
  return fabsf(v) < INFINITY;
}

__device__ inline AlnPoint aln_point(const AlnArgs & a, int f, int k)
{
  AlnPoint r;
  const int p = f * a.K + k;
  const float * xs = a.x + 3 * p;
  const float * ys = a.y + 3 * (a.y_per_frame ? p : k);
#pragma unroll
  for(int c = 0; c < 3; c++) r.x[c] = xs[c], r.y[c] = ys[c];
  r.w = a.w ? a.w[a.w_per_frame ? p : k] : 1.0f;
  r.moved = aln_finite(r.x[0]) && aln_finite(r.x[1]) && aln_finite(r.x[2]);
  r.live = r.w > 0.0f && r.w < INFINITY && r.moved && aln_finite(r.y[0]) && aln_finite(r.y[1]) && aln_finite(r.y[2]);
  return r;
}

// fn(k) for every point k < K that thread t of the frame's team owns
template<int NQ, class Fn>
__device__ inline void aln_each(int K, int t, Fn fn)
{
  if constexpr(NQ == 0)
  {
    if(t < K) fn(t);
  }
  else
  {
    constexpr int T = 1024 / NQ;
    for(int k0 = 0; k0 < K; k0 += 1024)
#pragma unroll
      for(int q = 0; q < NQ; q++)
      {
        const int k = k0 + T * q + t;
        if(k < K) fn(k);
      }
  }
}

// The LDS of a frame's sums.  NQ = 4: a row of T / 64 floats for every sum of the kernel, taken in turn, so that one barrier per sum is
// enough.  NQ = 1: the two banks of sum1024_meet_many, three sums a meeting.  The wavefront form uses none.
struct AlnLds
{
  float * base;
  int row, turn;
};

// sum1024_meet_many over p[E0 ...], three at a time
template<int NS, int E0>
__device__ inline void aln_meet_chunks(float (&p)[NS], AlnLds & lds)
{
  if constexpr(E0 < NS)
  {
    constexpr int C = NS - E0 < 3 ? NS - E0 : 3;
    float v[C];
#pragma unroll
    for(int e = 0; e < C; e++) v[e] = p[E0 + e];
    sum1024_meet_many<C, 0u>(v, reinterpret_cast<float(*)[3][SUM1024_WAVES]>(lds.base), lds.turn);
#pragma unroll
    for(int e = 0; e < C; e++) p[E0 + e] = v[e];
    aln_meet_chunks<NS, E0 + 3>(p, lds);
  }
}

// NS sums at once over the frame's points by sum1024: term(k, v) gives point k's NS terms.  Every thread ends with the same bits.
template<int NQ, int NS, class Term>
__device__ inline void aln_sums(int K, int t, float (&out)[NS], AlnLds & lds, Term term)
{
  if constexpr(NQ == 0)
  {
    float v[NS];
#pragma unroll
    for(int e = 0; e < NS; e++) v[e] = 0.0f;
    if(t < K) term(t, v);
#pragma unroll
    for(int e = 0; e < NS; e++) out[e] = 0.0f + v[e]; // partial k; the partials past 63 are +0 and left out
    sum64_meet(out);
  }
  else
  {
    constexpr int T = 1024 / NQ;
    float part[NS][NQ];
#pragma unroll
    for(int e = 0; e < NS; e++)
#pragma unroll
      for(int q = 0; q < NQ; q++) part[e][q] = 0.0f;
    for(int k0 = 0; k0 < K; k0 += 1024)
#pragma unroll
      for(int q = 0; q < NQ; q++)
      {
        const int k = k0 + T * q + t;
        if(k < K)
        {
          float v[NS];
          term(k, v);
#pragma unroll
          for(int e = 0; e < NS; e++) part[e][q] = part[e][q] + v[e];
        }
      }
    if constexpr(NQ == 1)
    {
#pragma unroll
      for(int e = 0; e < NS; e++) out[e] = part[e][0];
      aln_meet_chunks<NS, 0>(out, lds);
    }
    else
    {
#pragma unroll
      for(int e = 0; e < NS; e++) out[e] = sum1024_meet<NQ>(part[e], lds.base + (lds.row + e) * (T / 64));
      lds.row += NS;
    }
  }
}

// passes one and two: W, the centroids, the nine moments and vx
template<int NQ>
__device__ inline void aln_moments(const AlnArgs & a, int f, int t, AlnFrame & F, AlnLds & lds)
{
  float m[7];
  aln_sums<NQ, 7>(a.K, t, m, lds, [&](int k, float(&v)[7]) {
    const AlnPoint p = aln_point(a, f, k);
    v[0] = p.live ? p.w : 0.0f;
#pragma unroll
    for(int c = 0; c < 3; c++) v[1 + c] = p.live ? p.w * p.x[c] : 0.0f, v[4 + c] = p.live ? p.w * p.y[c] : 0.0f;
  });
  F.W = m[0];
#pragma unroll
  for(int c = 0; c < 3; c++) F.cx[c] = m[1 + c] / F.W, F.cy[c] = m[4 + c] / F.W;
  float s[10];
  aln_sums<NQ, 10>(a.K, t, s, lds, [&](int k, float(&v)[10]) {
    const AlnPoint p = aln_point(a, f, k);
    float xt[3], yt[3];
#pragma unroll
    for(int c = 0; c < 3; c++) xt[c] = p.x[c] - F.cx[c], yt[c] = p.y[c] - F.cy[c];
#pragma unroll
    for(int i = 0; i < 3; i++)
#pragma unroll
      for(int j = 0; j < 3; j++) v[3 * i + j] = p.live ? (p.w * xt[i]) * yt[j] : 0.0f;
    v[9] = p.live ? p.w * ((xt[0] * xt[0] + xt[1] * xt[1]) + xt[2] * xt[2]) : 0.0f;
  });
#pragma unroll
  for(int e = 0; e < 9; e++) F.S[e] = s[e];
  F.vx = s[9];
}

// one Jacobi rotation on the pair (P, Q) of the symmetric A (kept whole), accumulated into the columns of V
template<int P, int Q>
__device__ inline void aln_rotate(float (&A)[4][4], float (&V)[4][4])
{
  const float apq = A[P][Q];
  if(apq == 0.0f) return;
  const float theta = (A[Q][Q] - A[P][P]) / (2.0f * apq);
  const float t = (theta < 0.0f ? -1.0f : 1.0f) / (fabsf(theta) + sqrtf(theta * theta + 1.0f)); // theta^2 = inf: t = 0
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  const float h = t * apq;
  A[P][P] = A[P][P] - h, A[Q][Q] = A[Q][Q] + h;
  A[P][Q] = 0.0f, A[Q][P] = 0.0f;
#pragma unroll
  for(int r = 0; r < 4; r++)
    if(r != P && r != Q)
    {
      const float arp = A[r][P], arq = A[r][Q];
      const float np = c * arp - s * arq, nq = s * arp + c * arq;
      A[r][P] = np, A[P][r] = np, A[r][Q] = nq, A[Q][r] = nq;
    }
#pragma unroll
  for(int r = 0; r < 4; r++)
  {
    const float vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = c * vrp - s * vrq, V[r][Q] = s * vrp + c * vrq;
  }
}

// R (x) for a row-major R
__device__ inline void aln_rot(const float (&R)[9], const float (&x)[3], float (&o)[3])
{
#pragma unroll
  for(int a = 0; a < 3; a++) o[a] = (R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2];
}

// aligned = s (R x) + t
__device__ inline void aln_apply(const AlnFrame & F, const float (&x)[3], float (&o)[3])
{
  float r[3];
  aln_rot(F.R, x, r);
#pragma unroll
  for(int a = 0; a < 3; a++) o[a] = F.s * r[a] + F.t[a];
}

// steps 4 to 7 and 9 of the forward rule, done by every thread of the frame alike
__device__ inline void aln_solve(const AlnArgs & a, AlnFrame & F)
{
#pragma unroll
  for(int i = 0; i < 9; i++) F.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
  F.t[0] = 0.0f, F.t[1] = 0.0f, F.t[2] = 0.0f, F.s = 1.0f, F.gap = 0.0f, F.top = 0;
#pragma unroll
  for(int i = 0; i < 4; i++)
  {
    F.lam[i] = 0.0f, F.q[i] = i ? 0.0f : 1.0f;
#pragma unroll
    for(int j = 0; j < 4; j++) F.V[i][j] = i == j ? 1.0f : 0.0f;
  }
  if(!(F.W > 0.0f && F.W < INFINITY))
  {
    F.status = 1;
    return;
  }
  const float Sxx = F.S[0], Sxy = F.S[1], Sxz = F.S[2], Syx = F.S[3], Syy = F.S[4], Syz = F.S[5], Szx = F.S[6], Szy = F.S[7], Szz = F.S[8];
  float A[4][4];
  A[0][0] = (Sxx + Syy) + Szz, A[1][1] = (Sxx - Syy) - Szz, A[2][2] = ((-Sxx) + Syy) - Szz, A[3][3] = ((-Sxx) - Syy) + Szz;
  A[0][1] = A[1][0] = Syz - Szy, A[0][2] = A[2][0] = Szx - Sxz, A[0][3] = A[3][0] = Sxy - Syx;
  A[1][2] = A[2][1] = Sxy + Syx, A[1][3] = A[3][1] = Szx + Sxz, A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
  for(int sweep = 0; sweep < ALN_SWEEPS; sweep++)
  {
    aln_rotate<0, 1>(A, F.V), aln_rotate<0, 2>(A, F.V), aln_rotate<0, 3>(A, F.V);
    aln_rotate<1, 2>(A, F.V), aln_rotate<1, 3>(A, F.V), aln_rotate<2, 3>(A, F.V);
  }
#pragma unroll
  for(int i = 0; i < 4; i++) F.lam[i] = A[i][i];
  float l1 = F.lam[0], l4 = F.lam[0];
#pragma unroll
  for(int i = 1; i < 4; i++)
  {
    if(F.lam[i] > l1) l1 = F.lam[i], F.top = i;
    if(F.lam[i] < l4) l4 = F.lam[i];
  }
  float l2 = -INFINITY;
#pragma unroll
  for(int i = 0; i < 4; i++)
    if(i != F.top && F.lam[i] > l2) l2 = F.lam[i];
  const float spread = l1 - l4;
  F.gap = spread > 0.0f ? (l1 - l2) / spread : 0.0f;
  F.status = (F.vx == 0.0f ? 2 : 0) | (F.gap <= a.min_gap ? 4 : 0);
  float e[4];
#pragma unroll
  for(int r = 0; r < 4; r++) e[r] = F.top == 0 ? F.V[r][0] : F.top == 1 ? F.V[r][1] : F.top == 2 ? F.V[r][2] : F.V[r][3];
  const float len = sqrtf(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);
#pragma unroll
  for(int r = 0; r < 4; r++) F.q[r] = e[r] / len;
  if(F.vx != 0.0f)
  {
    const float w = F.q[0], x = F.q[1], y = F.q[2], z = F.q[3];
    const float ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    F.R[0] = ((ww + xx) - yy) - zz, F.R[1] = 2.0f * (xy - wz), F.R[2] = 2.0f * (xz + wy);
    F.R[3] = 2.0f * (xy + wz), F.R[4] = ((ww - xx) + yy) - zz, F.R[5] = 2.0f * (yz - wx);
    F.R[6] = 2.0f * (xz - wy), F.R[7] = 2.0f * (yz + wx), F.R[8] = ((ww - xx) - yy) + zz;
    if(a.with_scale)
    {
      float acc = F.R[0] * F.S[0];
#pragma unroll
      for(int i = 1; i < 9; i++) acc = acc + F.R[i] * F.S[3 * (i % 3) + i / 3];
      F.s = acc / F.vx;
    }
  }
  float rc[3];
  aln_rot(F.R, F.cx, rc);
#pragma unroll
  for(int c = 0; c < 3; c++) F.t[c] = F.cy[c] - F.s * rc[c];
}

// what the backward's last pass needs of the closed form
struct AlnPull
{
  float Gt[3], GM[9], g2, cs[3]; // GM row-major; g2 = 2 g_vx; cs = -(s R^T G_t)
};

// the closed form of the backward for a frame with status 0.  gtr: the frame's 13 cotangents of the transform, or null.
// sums: sum ga [3], then sum ga x^T [9] row-major
__device__ inline void aln_pull(const AlnArgs & a, const AlnFrame & F, const float * gtr, const float (&sums)[12], AlnPull & B)
{
  float gR[9], gt[3], gs;
#pragma unroll
  for(int i = 0; i < 9; i++) gR[i] = gtr ? gtr[i] : 0.0f;
#pragma unroll
  for(int i = 0; i < 3; i++) gt[i] = gtr ? gtr[9 + i] : 0.0f;
  gs = gtr ? gtr[12] : 0.0f;
  const float * P = sums + 3;
#pragma unroll
  for(int c = 0; c < 3; c++) B.Gt[c] = gt[c] + sums[c];
  float rc[3];
  aln_rot(F.R, F.cx, rc);
  float Gs = 0.0f;
  if(a.with_scale)
  {
    float rp = F.R[0] * P[0];
#pragma unroll
    for(int i = 1; i < 9; i++) rp = rp + F.R[i] * P[i];
    Gs = (gs + rp) - ((B.Gt[0] * rc[0] + B.Gt[1] * rc[1]) + B.Gt[2] * rc[2]);
  }
  float GR[9];
#pragma unroll
  for(int i = 0; i < 3; i++)
#pragma unroll
    for(int j = 0; j < 3; j++) GR[3 * i + j] = ((gR[3 * i + j] + F.s * P[3 * i + j]) - (F.s * B.Gt[i]) * F.cx[j]) + (Gs * F.S[3 * j + i]) / F.vx;
  B.g2 = 2.0f * ((-(Gs * F.s)) / F.vx);
  // through R(q)
  const float w = F.q[0], x = F.q[1], y = F.q[2], z = F.q[3];
  const float d0 = (GR[0] + GR[4]) + GR[8], d1 = (GR[0] - GR[4]) - GR[8], d2 = ((-GR[0]) + GR[4]) - GR[8], d3 = ((-GR[0]) - GR[4]) + GR[8];
  const float a01 = GR[7] - GR[5], a02 = GR[2] - GR[6], a03 = GR[3] - GR[1]; // the matrix of step 4, built from G_R^T in S's place
  const float a12 = GR[1] + GR[3], a13 = GR[2] + GR[6], a23 = GR[5] + GR[7];
  float gq[4];
  gq[0] = 2.0f * (((d0 * w + a01 * x) + a02 * y) + a03 * z);
  gq[1] = 2.0f * (((a01 * w + d1 * x) + a12 * y) + a13 * z);
  gq[2] = 2.0f * (((a02 * w + a12 * x) + d2 * y) + a23 * z);
  gq[3] = 2.0f * (((a03 * w + a13 * x) + a23 * y) + d3 * z);
  // through the eigenvector
  const float l1 = F.top == 0 ? F.lam[0] : F.top == 1 ? F.lam[1] : F.top == 2 ? F.lam[2] : F.lam[3];
  float co[4];
#pragma unroll
  for(int i = 0; i < 4; i++)
  {
    const float dot = ((F.V[0][i] * gq[0] + F.V[1][i] * gq[1]) + F.V[2][i] * gq[2]) + F.V[3][i] * gq[3];
    co[i] = i == F.top ? 0.0f : dot / (l1 - F.lam[i]);
  }
  float u[4];
#pragma unroll
  for(int r = 0; r < 4; r++) u[r] = ((F.V[r][0] * co[0] + F.V[r][1] * co[1]) + F.V[r][2] * co[2]) + F.V[r][3] * co[3];
  // G_N = u q^T through the linear map S -> N
  const float D0 = u[0] * F.q[0], D1 = u[1] * F.q[1], D2 = u[2] * F.q[2], D3 = u[3] * F.q[3];
  const float H01 = u[0] * F.q[1] + u[1] * F.q[0], H02 = u[0] * F.q[2] + u[2] * F.q[0], H03 = u[0] * F.q[3] + u[3] * F.q[0];
  const float H12 = u[1] * F.q[2] + u[2] * F.q[1], H13 = u[1] * F.q[3] + u[3] * F.q[1], H23 = u[2] * F.q[3] + u[3] * F.q[2];
  float GS[9];
  GS[0] = ((D0 + D1) - D2) - D3, GS[4] = ((D0 - D1) + D2) - D3, GS[8] = ((D0 - D1) - D2) + D3;
  GS[5] = H23 + H01, GS[7] = H23 - H01; // yz, zy
  GS[6] = H13 + H02, GS[2] = H13 - H02; // zx, xz
  GS[1] = H12 + H03, GS[3] = H12 - H03; // xy, yx
#pragma unroll
  for(int i = 0; i < 3; i++)
#pragma unroll
    for(int j = 0; j < 3; j++) B.GM[3 * i + j] = (Gs * F.R[3 * i + j]) / F.vx + GS[3 * j + i];
#pragma unroll
  for(int c = 0; c < 3; c++) B.cs[c] = -(F.s * ((F.R[c] * B.Gt[0] + F.R[3 + c] * B.Gt[1]) + F.R[6 + c] * B.Gt[2]));
}

template<int NQ>
__device__ inline bool aln_team(int n, int & f, int & t)
{
  if constexpr(NQ == 0)
  {
    f = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ALN_T / 64) + (threadIdx.x >> 6))), t = threadIdx.x & 63;
    return f < n;
  }
  else
  {
    f = blockIdx.x, t = threadIdx.x;
    return true;
  }
}

// NQ = 0: grid ceil(n / 4), ALN_T threads; else grid n, 1024 / NQ threads
template<int NQ>
__global__ __launch_bounds__(NQ ? 1024 / NQ : ALN_T) void aln_forward_kernel(AlnArgs a, AlnOut o, int n)
{
  __shared__ float cross[aln_lds_floats(NQ, ALN_FWD_SUMS)];
  int f, t;
  if(!aln_team<NQ>(n, f, t)) return;
  AlnLds lds{cross, 0, 0};
  AlnFrame F;
  aln_moments<NQ>(a, f, t, F, lds);
  aln_solve(a, F);
  if(t == 0)
  {
    if(o.transform)
    {
      float * tr = o.transform + (int64_t)13 * f; // (n may pass 2^31 / 13: only n K 3 is held to int32)
#pragma unroll
      for(int i = 0; i < 9; i++) tr[i] = F.R[i];
      tr[9] = F.t[0], tr[10] = F.t[1], tr[11] = F.t[2], tr[12] = F.s;
    }
    if(o.gap) o.gap[f] = F.gap;
    if(o.status) o.status[f] = F.status;
  }
  if(!o.aligned && !o.point_error && !o.energy) return;
  float e[1];
  aln_sums<NQ, 1>(a.K, t, e, lds, [&](int k, float(&v)[1]) {
    const AlnPoint p = aln_point(a, f, k);
    const int at = f * a.K + k;
    float al[3];
    aln_apply(F, p.x, al);
    if(o.aligned) o.aligned[3 * at] = al[0], o.aligned[3 * at + 1] = al[1], o.aligned[3 * at + 2] = al[2];
    const float d0 = al[0] - p.y[0], d1 = al[1] - p.y[1], d2 = al[2] - p.y[2];
    const float pe = p.live ? (d0 * d0 + d1 * d1) + d2 * d2 : 0.0f;
    if(o.point_error) o.point_error[at] = pe;
    v[0] = p.live ? p.w * pe : 0.0f;
  });
  if(t == 0 && o.energy) o.energy[f] = (F.status & 1) ? 0.0f : e[0];
}

template<int NQ>
__global__ __launch_bounds__(NQ ? 1024 / NQ : ALN_T) void aln_backward_kernel(AlnArgs a, AlnCot g, float * gsrc, float * gtgt, int accumulate, int n)
{
  __shared__ float cross[aln_lds_floats(NQ, ALN_BWD_SUMS)];
  int f, t;
  if(!aln_team<NQ>(n, f, t)) return;
  AlnLds lds{cross, 0, 0};
  AlnFrame F;
  aln_moments<NQ>(a, f, t, F, lds);
  aln_solve(a, F);
  const float ge2 = 2.0f * (g.ge ? g.ge[f] : 0.0f);
  // ga = grad_aligned + (2 ge w) (aligned - y), the second term for live points; d = aligned - y; c2 = 2 ge w
  auto cot = [&](const AlnPoint & p, int at, float(&ga)[3], float(&d)[3], float & c2) {
    float al[3];
    aln_apply(F, p.x, al);
    c2 = ge2 * p.w;
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      d[c] = al[c] - p.y[c];
      ga[c] = (g.gal ? g.gal[3 * at + c] : 0.0f) + (p.live ? c2 * d[c] : 0.0f);
    }
  };
  float sums[12];
  aln_sums<NQ, 12>(a.K, t, sums, lds, [&](int k, float(&v)[12]) {
    const AlnPoint p = aln_point(a, f, k);
    float ga[3], d[3], c2;
    cot(p, f * a.K + k, ga, d, c2);
#pragma unroll
    for(int i = 0; i < 3; i++)
    {
      v[i] = p.moved ? ga[i] : 0.0f;
#pragma unroll
      for(int j = 0; j < 3; j++) v[3 + 3 * i + j] = p.moved ? ga[i] * p.x[j] : 0.0f;
    }
  });
  AlnPull B;
  const bool whole = F.status == 0;
  if(whole) aln_pull(a, F, g.gtr ? g.gtr + (int64_t)13 * f : nullptr, sums, B);
  aln_each<NQ>(a.K, t, [&](int k) {
    const AlnPoint p = aln_point(a, f, k);
    const int at = f * a.K + k;
    float ga[3], d[3], c2;
    cot(p, at, ga, d, c2);
    float gx[3], gy[3];
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      gx[c] = F.s * ((F.R[c] * ga[0] + F.R[3 + c] * ga[1]) + F.R[6 + c] * ga[2]);
      gy[c] = p.live ? 0.0f - c2 * d[c] : 0.0f;
    }
    if(whole && p.live)
    {
      float xt[3], yt[3];
#pragma unroll
      for(int c = 0; c < 3; c++) xt[c] = p.x[c] - F.cx[c], yt[c] = p.y[c] - F.cy[c];
      const float share = p.w / F.W;
#pragma unroll
      for(int c = 0; c < 3; c++)
      {
        const float my = (B.GM[c] * yt[0] + B.GM[3 + c] * yt[1]) + B.GM[6 + c] * yt[2];
        const float mx = (B.GM[3 * c] * xt[0] + B.GM[3 * c + 1] * xt[1]) + B.GM[3 * c + 2] * xt[2];
        gx[c] = (gx[c] + p.w * (my + B.g2 * xt[c])) + share * B.cs[c];
        gy[c] = (gy[c] + p.w * mx) + share * B.Gt[c];
      }
    }
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      if(gsrc) gsrc[3 * at + c] = accumulate ? gsrc[3 * at + c] + gx[c] : gx[c];
      if(gtgt) gtgt[3 * at + c] = accumulate ? gtgt[3 * at + c] + gy[c] : gy[c];
    }
  });
}

static int aln_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

// what the two calls refuse alike
static int aln_check(const char * fn, int64_t n, int64_t K, const float * source, const float * target, int64_t Tn, int64_t Wn, int with_scale,
                     float min_gap, int space)
{
  if(!source || !target) return aln_refuse(fn, "source or target is NULL");
  if(n <= 0 || K <= 0) return aln_refuse(fn, "n and K must be positive");
  if(Tn != 1 && Tn != n) return aln_refuse(fn, "Tn must be 1 or n");
  if(Wn != 1 && Wn != n) return aln_refuse(fn, "Wn must be 1 or n");
  if(with_scale != 0 && with_scale != 1) return aln_refuse(fn, "with_scale must be 0 or 1");
  if(!(min_gap >= 0.0f && min_gap < INFINITY)) return aln_refuse(fn, "min_gap must be finite and not negative");
  if(n > ALN_INT32_MAX || K > ALN_INT32_MAX || n * K > ALN_INT32_MAX / 3) return aln_refuse(fn, "n K 3 beyond int32 indexing");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// one launch per form of frame_sum_split
#define ALN_LAUNCH(KERNEL, n, K, st, ...)                                                               \
  do                                                                                                    \
  {                                                                                                     \
    const FrameSumSplit sp = frame_sum_split(K);                                                        \
    if(sp.nq == 0) KERNEL<0><<<dim3((unsigned)((n + ALN_T / 64 - 1) / (ALN_T / 64))), dim3(ALN_T), 0, st>>>(__VA_ARGS__); \
    else if(sp.nq == 4)                                                                                 \
      KERNEL<4><<<dim3((unsigned)n), dim3(sp.threads), 0, st>>>(__VA_ARGS__);                           \
    else                                                                                                \
      KERNEL<1><<<dim3((unsigned)n), dim3(sp.threads), 0, st>>>(__VA_ARGS__);                           \
    HIP_TRY(hipGetLastError());                                                                         \
  } while(0)

extern "C" int smplpp_align(int device, int64_t n, int64_t K, const float * source, const float * target, int64_t Tn, const float * weight, int64_t Wn,
                            int with_scale, float min_gap, float * transform, float * aligned, float * energy, float * point_error, float * gap,
                            int32_t * status, int space, void * stream)
{
  const char * fn = "smplpp_align";
  if(int rc = aln_check(fn, n, K, source, target, Tn, Wn, with_scale, min_gap, space)) return rc;
  if(!transform && !aligned && !energy && !point_error && !gap && !status) return aln_refuse(fn, "every output is NULL");
  const int64_t total = n * K;
  Frame fr(device, nullptr, space, stream, "align");
  AlnArgs a{fr.in(source, (size_t)(total * 3)), fr.in(target, (size_t)(Tn * K * 3)), nullptr, (int)K, Tn != 1, weight && Wn != 1, with_scale, min_gap};
  a.w = fr.in(weight, (size_t)(Wn * K));
  AlnOut o{fr.out(transform, (size_t)(n * 13)), fr.out(aligned, (size_t)(total * 3)), fr.out(energy, (size_t)n), fr.out(point_error, (size_t)total),
           fr.out(gap, (size_t)n), fr.out(status, (size_t)n)};
  return fr.run([&] {
    ALN_LAUNCH(aln_forward_kernel, n, K, fr.st, a, o, (int)n);
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_align_vjp(int device, int64_t n, int64_t K, const float * source, const float * target, int64_t Tn, const float * weight,
                                int64_t Wn, int with_scale, float min_gap, const float * grad_transform, const float * grad_aligned,
                                const float * grad_energy, float * grad_source, float * grad_target, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_align_vjp";
  if(int rc = aln_check(fn, n, K, source, target, Tn, Wn, with_scale, min_gap, space)) return rc;
  if(!grad_transform && !grad_aligned && !grad_energy) return aln_refuse(fn, "every cotangent is NULL");
  if(!grad_source && !grad_target) return aln_refuse(fn, "grad_source and grad_target are both NULL");
  if(accumulate != 0 && accumulate != 1) return aln_refuse(fn, "accumulate must be 0 or 1");
  const int64_t total = n * K;
  Frame fr(device, nullptr, space, stream, "align VJP");
  AlnArgs a{fr.in(source, (size_t)(total * 3)), fr.in(target, (size_t)(Tn * K * 3)), nullptr, (int)K, Tn != 1, weight && Wn != 1, with_scale, min_gap};
  a.w = fr.in(weight, (size_t)(Wn * K));
  const AlnCot g{fr.in(grad_transform, (size_t)(n * 13)), fr.in(grad_aligned, (size_t)(total * 3)), fr.in(grad_energy, (size_t)n)};
  float * gs = fr.out(grad_source, (size_t)(total * 3), accumulate != 0);
  float * gt = fr.out(grad_target, (size_t)(total * 3), accumulate != 0);
  return fr.run([&] {
    ALN_LAUNCH(aln_backward_kernel, n, K, fr.st, a, g, gs, gt, accumulate, (int)n);
    return (int)SMPLPP_OK;
  });
}
