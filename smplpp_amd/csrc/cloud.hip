// Scan preparation: the k nearest cloud points of every query, normals and surface variation from the neighbour lists, and
// farthest-point sampling.  The rules are in include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to
// FMA), divisions and square roots are the correctly rounded ones, every sum is sequential in a stated order, every choice is the
// minimum or maximum of a total order, and there are no floating-point atomics.  The calls take no handle and no workspace.
//
//  cld_knn_kernel<C>      a wavefront of 64 queries of one frame, the frame's cloud streamed through LDS CLD_TILE points at a time as
//                         float4 (every lane reads the same point: a broadcast).  A lane keeps its C best (d, j) sorted in registers;
//                         a candidate that beats the list's worst entry replaces it and is carried up by an unrolled chain of
//                         compare-and-swaps, every list index a constant.  Candidates come in ascending j, and the chain swaps on a
//                         strict d < only, so equal distances stay in ascending j: the order (d, j).  C = 8, 16 or 32 by k.
//  cld_normals_kernel     a lane per point: the gather of its k neighbours, the 3 x 3 covariance, four sweeps of cyclic Jacobi in
//                         registers (the rotations unrolled, every matrix index a constant), the normal's sign, curvature and status.
//  cld_fps_kernel<PPT>    a workgroup of 1024 per frame and M dependent rounds: the update of dmin against the last pick, then the
//                         workgroup's argmax of (dmin, -j) (a wavefront reduction, then 16 partials through LDS, two banks taken in
//                         turn so that a round has one barrier).  PPT = 1, 4 or 16 points of a thread live in registers with their
//                         dmin (K <= 1024 PPT); PPT = 0 reads the points from memory and keeps dmin in min_sqdist.  A chosen point
//                         and a point that is not finite hold dmin = -1 while the kernel runs (never a candidate), and +0 at the end.
#include "staging.h"

#include <cmath>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int CLD_KNN_T = 64;     // queries per workgroup: (1, 16384) still gives each of the 256 CUs a workgroup
constexpr int CLD_TILE = 1024;    // points per LDS tile (float4: 16 KiB)
constexpr int CLD_K_MAX = 32;     // the largest list
constexpr int CLD_NRM_T = 256;    // points per workgroup of the normals kernel
constexpr int CLD_SWEEPS = 4;     // Jacobi sweeps: a constant of the rule (DESIGN §3.32 has the measurement behind it)
constexpr int CLD_FPS_T = 1024;   // threads of a frame's workgroup in farthest-point sampling
constexpr int CLD_FPS_WAVES = CLD_FPS_T / 64;
constexpr int CLD_FPS_PPT = 16;   // the most points a thread keeps in registers: above 1024 * 16 points dmin lives in min_sqdist
constexpr int64_t CLD_INT32_MAX = 0x7fffffffLL;

__device__ inline bool cld_finite(float v)
{
  return fabsf(v) < INFINITY;
}

// the contract's distance: ((dx dx + dy dy) + dz dz)
__device__ inline float cld_sqdist(float ax, float ay, float az, float bx, float by, float bz)
{
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ---- k nearest neighbours
// grid n * qblocks, CLD_KNN_T threads; self: the cloud queries itself (queries is not read, Q = K) and candidate j = q is left out
template<int C>
__global__ __launch_bounds__(CLD_KNN_T) void cld_knn_kernel(const float * __restrict__ points, const float * __restrict__ queries, int K, int Q,
                                                            int qblocks, int k, float cap, int self, int32_t * __restrict__ index,
                                                            float * __restrict__ sqdist, int32_t * __restrict__ count)
{
  __shared__ float4 s_p[CLD_TILE];
  const int f = blockIdx.x / (uint32_t)qblocks, qb = blockIdx.x % (uint32_t)qblocks;
  const int t = threadIdx.x;
  const int q = qb * CLD_KNN_T + t;
  const int qc = q < Q ? q : Q - 1; // lanes past Q repeat the last query and write nothing
  const float * pf = points + (int64_t)f * K * 3;
  const float * qp = (self ? points : queries) + ((int64_t)f * Q + qc) * 3;
  const float qx = qp[0], qy = qp[1], qz = qp[2];
  float bd[C];
  int bj[C];
#pragma unroll
  for(int i = 0; i < C; i++) bd[i] = INFINITY, bj[i] = -1;
  for(int base = 0; base < K; base += CLD_TILE)
  {
    const int cnt = K - base < CLD_TILE ? K - base : CLD_TILE;
    __syncthreads();
    for(int j = t; j < cnt; j += CLD_KNN_T)
    {
      const float * p = pf + (int64_t)(base + j) * 3;
      s_p[j] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    __syncthreads();
#pragma unroll 4
    for(int j = 0; j < cnt; j++)
    {
      const float4 p = s_p[j];
      const int kk = base + j;
      const float d = cld_sqdist(qx, qy, qz, p.x, p.y, p.z);
      // (a NaN d fails both tests, an infinite one the second: the list's worst entry is at most +inf)
      if(d <= cap && d < bd[C - 1] && !(self && kk == q))
      {
        bd[C - 1] = d, bj[C - 1] = kk;
#pragma unroll
        for(int i = C - 1; i > 0; i--)
        {
          const bool up = bd[i] < bd[i - 1];
          const float d0 = bd[i - 1], d1 = bd[i];
          const int j0 = bj[i - 1], j1 = bj[i];
          bd[i - 1] = up ? d1 : d0, bd[i] = up ? d0 : d1;
          bj[i - 1] = up ? j1 : j0, bj[i] = up ? j0 : j1;
        }
      }
    }
  }
  if(q >= Q) return;
  const int64_t row = ((int64_t)f * Q + q) * k;
  int found = 0;
#pragma unroll
  for(int r = 0; r < C; r++)
    if(r < k)
    {
      const bool have = bj[r] >= 0;
      found += have ? 1 : 0;
      if(index) index[row + r] = bj[r];
      if(sqdist) sqdist[row + r] = have ? bd[r] : 0.0f;
    }
  if(count) count[(int64_t)f * Q + q] = found;
}

// ---- normals
// one Jacobi rotation on the pair (P, R) of the symmetric A (kept whole), accumulated into the columns of V
template<int P, int R>
__device__ inline void cld_rotate(float (&A)[3][3], float (&V)[3][3])
{
  const float apq = A[P][R];
  if(apq == 0.0f) return;
  const float tau = (A[R][R] - A[P][P]) / (2.0f * apq);
  const float t = (tau < 0.0f ? -1.0f : 1.0f) / (fabsf(tau) + sqrtf(tau * tau + 1.0f)); // tau^2 = inf: t = 0
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  const float h = t * apq;
  A[P][P] = A[P][P] - h, A[R][R] = A[R][R] + h;
  A[P][R] = 0.0f, A[R][P] = 0.0f;
  constexpr int O = 3 - P - R; // the third index
  {
    const float arp = A[O][P], arq = A[O][R];
    const float np = c * arp - s * arq, nq = s * arp + c * arq;
    A[O][P] = np, A[P][O] = np, A[O][R] = nq, A[R][O] = nq;
  }
#pragma unroll
  for(int r = 0; r < 3; r++)
  {
    const float vrp = V[r][P], vrq = V[r][R];
    V[r][P] = c * vrp - s * vrq, V[r][R] = s * vrp + c * vrq;
  }
}

// swap the pair (a, b) of the order when lam[b] < lam[a]; three of these in the order (0,1), (1,2), (0,1) sort by (value, column)
__device__ inline void cld_order(float & la, float & lb, int & ia, int & ib)
{
  if(lb < la)
  {
    const float l = la;
    la = lb, lb = l;
    const int i = ia;
    ia = ib, ib = i;
  }
}

// grid ceil(n K / CLD_NRM_T); view_per_frame: 0 one viewpoint for all frames, 1 one per frame (viewpoint null: none)
__global__ __launch_bounds__(CLD_NRM_T) void cld_normals_kernel(const float * __restrict__ points, const int32_t * __restrict__ index,
                                                                const float * __restrict__ viewpoint, int view_per_frame, int total, int K,
                                                                int k, float min_gap, float * __restrict__ normal,
                                                                float * __restrict__ curvature, int32_t * __restrict__ status)
{
  const int g = blockIdx.x * CLD_NRM_T + threadIdx.x;
  if(g >= total) return;
  const int f = g / K;
  const float * pf = points + (int64_t)f * K * 3;
  const float px = points[(int64_t)g * 3], py = points[(int64_t)g * 3 + 1], pz = points[(int64_t)g * 3 + 2];
  const int32_t * row = index + (int64_t)g * k;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, xx = 0.0f, xy = 0.0f, xz = 0.0f, yy = 0.0f, yz = 0.0f, zz = 0.0f;
  int m = 1;
  for(int r = 0; r < k; r++)
  {
    const int j = row[r];
    if(j < 0 || j >= K) continue;
    const float e0 = pf[(int64_t)j * 3] - px, e1 = pf[(int64_t)j * 3 + 1] - py, e2 = pf[(int64_t)j * 3 + 2] - pz;
    if(!(cld_finite(e0) && cld_finite(e1) && cld_finite(e2))) continue;
    m++;
    s0 = s0 + e0, s1 = s1 + e1, s2 = s2 + e2;
    xx = xx + e0 * e0, xy = xy + e0 * e1, xz = xz + e0 * e2, yy = yy + e1 * e1, yz = yz + e1 * e2, zz = zz + e2 * e2;
  }
  float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, curv = 0.0f;
  int st = 1;
  if(m >= 3 && cld_finite(px) && cld_finite(py) && cld_finite(pz))
  {
    const float mf = (float)m;
    const float m0 = s0 / mf, m1 = s1 / mf, m2 = s2 / mf;
    float A[3][3], V[3][3];
    A[0][0] = xx - mf * (m0 * m0), A[1][1] = yy - mf * (m1 * m1), A[2][2] = zz - mf * (m2 * m2);
    A[0][1] = A[1][0] = xy - mf * (m0 * m1), A[0][2] = A[2][0] = xz - mf * (m0 * m2), A[1][2] = A[2][1] = yz - mf * (m1 * m2);
#pragma unroll
    for(int i = 0; i < 3; i++)
#pragma unroll
      for(int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0f : 0.0f;
#pragma unroll
    for(int sweep = 0; sweep < CLD_SWEEPS; sweep++) cld_rotate<0, 1>(A, V), cld_rotate<0, 2>(A, V), cld_rotate<1, 2>(A, V);
    float l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
    int i0 = 0, i1 = 1, i2 = 2;
    cld_order(l0, l1, i0, i1), cld_order(l1, l2, i1, i2), cld_order(l0, l1, i0, i1);
    const float v0 = i0 == 0 ? V[0][0] : i0 == 1 ? V[0][1] : V[0][2];
    const float v1 = i0 == 0 ? V[1][0] : i0 == 1 ? V[1][1] : V[1][2];
    const float v2 = i0 == 0 ? V[2][0] : i0 == 1 ? V[2][1] : V[2][2];
    const float len = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
    n0 = v0 / len, n1 = v1 / len, n2 = v2 / len;
    bool flip;
    if(viewpoint)
    {
      const float * c = viewpoint + (view_per_frame ? (int64_t)f * 3 : 0);
      flip = ((n0 * (c[0] - px) + n1 * (c[1] - py)) + n2 * (c[2] - pz)) < 0.0f;
    }
    else
    {
      float big = n0, mag = fabsf(n0);
      if(fabsf(n1) > mag) big = n1, mag = fabsf(n1);
      if(fabsf(n2) > mag) big = n2;
      flip = big < 0.0f;
    }
    if(flip) n0 = -n0, n1 = -n1, n2 = -n2;
    const float sum = (l0 + l1) + l2;
    curv = sum > 0.0f ? l0 / sum : 0.0f;
    st = (l2 <= 0.0f || (l1 - l0) < min_gap * l2) ? 2 : 0;
  }
  if(normal) normal[(int64_t)g * 3] = n0, normal[(int64_t)g * 3 + 1] = n1, normal[(int64_t)g * 3 + 2] = n2;
  if(curvature) curvature[g] = curv;
  if(status) status[g] = st;
}

// ---- farthest points
// (d, j) is ahead of (bd, bj) in the order (dmin, -j); "none" is (-1, -1), behind every candidate (their dmin is >= 0)
__device__ inline bool cld_ahead(float d, int j, float bd, int bj)
{
  return d > bd || (d == bd && j < bj);
}

// the workgroup's best (d, j), the same in every thread; bank: this round's 16 partials
__device__ inline void cld_argmax(float & d, int & j, float * sd, int * sj)
{
#pragma unroll
  for(int off = 32; off > 0; off >>= 1)
  {
    const float od = __shfl_xor(d, off, 64);
    const int oj = __shfl_xor(j, off, 64);
    if(cld_ahead(od, oj, d, j)) d = od, j = oj;
  }
  if((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = d, sj[threadIdx.x >> 6] = j;
  __syncthreads();
  d = sd[0], j = sj[0];
#pragma unroll
  for(int w = 1; w < CLD_FPS_WAVES; w++)
    if(cld_ahead(sd[w], sj[w], d, j)) d = sd[w], j = sj[w];
}

// grid n, CLD_FPS_T threads; PPT > 0: K <= CLD_FPS_T * PPT
template<int PPT>
__global__ __launch_bounds__(CLD_FPS_T) void cld_fps_kernel(const float * __restrict__ points, const int32_t * __restrict__ start, int K, int M,
                                                            int32_t * __restrict__ index, float * __restrict__ radius_sq,
                                                            float * __restrict__ min_sqdist)
{
  __shared__ float s_d[2][CLD_FPS_WAVES];
  __shared__ int s_j[2][CLD_FPS_WAVES];
  constexpr int R = PPT > 0 ? PPT : 1;
  const int f = blockIdx.x, t = threadIdx.x;
  const float * pf = points + (int64_t)f * K * 3;
  float * dm = min_sqdist + (int64_t)f * K;
  float x[R], y[R], z[R], dmin[R];
  int turn = 0;
  // dmin = +inf for the finite points, and the lowest finite index as the workgroup's first argmax
  float bd = -1.0f;
  int bj = -1;
  if constexpr(PPT > 0)
  {
#pragma unroll
    for(int i = 0; i < PPT; i++)
    {
      const int j = i * CLD_FPS_T + t;
      const int jc = j < K ? j : K - 1;
      x[i] = pf[(int64_t)jc * 3], y[i] = pf[(int64_t)jc * 3 + 1], z[i] = pf[(int64_t)jc * 3 + 2];
      dmin[i] = j < K && cld_finite(x[i]) && cld_finite(y[i]) && cld_finite(z[i]) ? INFINITY : -1.0f;
      if(cld_ahead(dmin[i], j, bd, bj)) bd = dmin[i], bj = j;
    }
  }
  else
  {
    for(int j = t; j < K; j += CLD_FPS_T)
    {
      const float d = cld_finite(pf[(int64_t)j * 3]) && cld_finite(pf[(int64_t)j * 3 + 1]) && cld_finite(pf[(int64_t)j * 3 + 2]) ? INFINITY : -1.0f;
      dm[j] = d;
      if(cld_ahead(d, j, bd, bj)) bd = d, bj = j;
    }
  }
  cld_argmax(bd, bj, s_d[turn], s_j[turn]), turn ^= 1;
  const int s = start ? start[f] : 0;
  if(bj >= 0 && s >= 0 && s < K && cld_finite(pf[(int64_t)s * 3]) && cld_finite(pf[(int64_t)s * 3 + 1]) && cld_finite(pf[(int64_t)s * 3 + 2])) bj = s;
  int cur = __builtin_amdgcn_readfirstlane(bj);
  float curd = INFINITY;
  int32_t * idx = index ? index + (int64_t)f * M : nullptr;
  float * rad = radius_sq ? radius_sq + (int64_t)f * M : nullptr;
  for(int i = 0; i < M; i++)
  {
    if(cur < 0) // no unchosen finite point is left
    {
      for(int r = i + t; r < M; r += CLD_FPS_T)
      {
        if(idx) idx[r] = -1;
        if(rad) rad[r] = 0.0f;
      }
      break;
    }
    if(t == 0)
    {
      if(idx) idx[i] = cur;
      if(rad) rad[i] = curd;
    }
    const float cx = pf[(int64_t)cur * 3], cy = pf[(int64_t)cur * 3 + 1], cz = pf[(int64_t)cur * 3 + 2];
    bd = -1.0f, bj = -1;
    if constexpr(PPT > 0)
    {
#pragma unroll
      for(int q = 0; q < PPT; q++)
      {
        const int j = q * CLD_FPS_T + t;
        const float d = cld_sqdist(x[q], y[q], z[q], cx, cy, cz);
        float v = dmin[q];
        if(v >= 0.0f) v = d < v ? d : v;
        if(j == cur) v = -1.0f;
        dmin[q] = v;
        if(cld_ahead(v, j, bd, bj)) bd = v, bj = j;
      }
    }
    else
    {
      for(int j = t; j < K; j += CLD_FPS_T)
      {
        const float d = cld_sqdist(pf[(int64_t)j * 3], pf[(int64_t)j * 3 + 1], pf[(int64_t)j * 3 + 2], cx, cy, cz);
        float v = dm[j];
        if(v >= 0.0f) v = d < v ? d : v;
        if(j == cur) v = -1.0f;
        dm[j] = v;
        if(cld_ahead(v, j, bd, bj)) bd = v, bj = j;
      }
    }
    if(i + 1 == M) break;
    cld_argmax(bd, bj, s_d[turn], s_j[turn]), turn ^= 1;
    cur = __builtin_amdgcn_readfirstlane(bj), curd = bd;
  }
  // the final dmin: +0 for the chosen points and the ones that are not finite
  if constexpr(PPT > 0)
  {
#pragma unroll
    for(int q = 0; q < PPT; q++)
    {
      const int j = q * CLD_FPS_T + t;
      if(j < K) dm[j] = dmin[q] < 0.0f ? 0.0f : dmin[q];
    }
  }
  else
  {
    for(int j = t; j < K; j += CLD_FPS_T)
      if(dm[j] < 0.0f) dm[j] = 0.0f;
  }
}

static int cld_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_cloud_knn(int device, int64_t n, int64_t K, const float * points, int64_t Q, const float * queries, int k, float max_sqdist,
                                int32_t * index, float * sqdist, int32_t * count, int space, void * stream)
{
  const char * fn = "smplpp_cloud_knn";
  if(k < 1 || k > CLD_K_MAX) return cld_refuse(fn, "k must be in 1..32");
  if(n < 0 || K < 0 || Q < 0) return cld_refuse(fn, "n, K and Q must not be negative");
  if(max_sqdist != max_sqdist) return cld_refuse(fn, "max_sqdist is NaN");
  if(!index && !sqdist && !count) return cld_refuse(fn, "every output is NULL");
  const bool self = queries == nullptr;
  if(self) Q = K;
  if(n > CLD_INT32_MAX || K > CLD_INT32_MAX || Q > CLD_INT32_MAX || n * K > CLD_INT32_MAX / 3 || n * Q > CLD_INT32_MAX / 3 ||
     n * Q * k > CLD_INT32_MAX)
    return cld_refuse(fn, "n Q k or n K 3 beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(n == 0 || Q == 0) return SMPLPP_OK;
  if(!points && K > 0) return cld_refuse(fn, "points is NULL");
  Frame fr(device, nullptr, space, stream, "cloud knn");
  const float * p = fr.in(points, (size_t)(n * K * 3));
  const float * q = self ? nullptr : fr.in(queries, (size_t)(n * Q * 3));
  int32_t * oi = fr.out(index, (size_t)(n * Q * k));
  float * od = fr.out(sqdist, (size_t)(n * Q * k));
  int32_t * oc = fr.out(count, (size_t)(n * Q));
  return fr.run([&] {
    const int qblocks = (int)((Q + CLD_KNN_T - 1) / CLD_KNN_T);
    const dim3 grid((unsigned)(n * qblocks)), block(CLD_KNN_T);
    if(k <= 8) cld_knn_kernel<8><<<grid, block, 0, fr.st>>>(p, q, (int)K, (int)Q, qblocks, k, max_sqdist, self, oi, od, oc);
    else if(k <= 16)
      cld_knn_kernel<16><<<grid, block, 0, fr.st>>>(p, q, (int)K, (int)Q, qblocks, k, max_sqdist, self, oi, od, oc);
    else
      cld_knn_kernel<32><<<grid, block, 0, fr.st>>>(p, q, (int)K, (int)Q, qblocks, k, max_sqdist, self, oi, od, oc);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_cloud_normals(int device, int64_t n, int64_t K, const float * points, int k, const int32_t * index, const float * viewpoint,
                                    int64_t Vn, float min_gap, float * normal, float * curvature, int32_t * status, int space, void * stream)
{
  const char * fn = "smplpp_cloud_normals";
  if(k < 1) return cld_refuse(fn, "k must be positive");
  if(n < 0 || K < 0) return cld_refuse(fn, "n and K must not be negative");
  if(Vn != 0 && Vn != 1 && Vn != n) return cld_refuse(fn, "Vn must be 0, 1 or n");
  if(Vn != 0 && !viewpoint) return cld_refuse(fn, "viewpoint is NULL");
  if(!(min_gap >= 0.0f && min_gap < INFINITY)) return cld_refuse(fn, "min_gap must be finite and not negative");
  if(!normal && !curvature && !status) return cld_refuse(fn, "every output is NULL");
  if(n > CLD_INT32_MAX || K > CLD_INT32_MAX || n * K > CLD_INT32_MAX / 3 || n * K * k > CLD_INT32_MAX)
    return cld_refuse(fn, "n K k or n K 3 beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(n == 0 || K == 0) return SMPLPP_OK;
  if(!points || !index) return cld_refuse(fn, "points or index is NULL");
  if(space == SMPLPP_HOST)
    for(int64_t i = 0; i < n * K * k; i++)
      if(index[i] >= K) return cld_refuse(fn, "index out of range");
  Frame fr(device, nullptr, space, stream, "cloud normals");
  const float * p = fr.in(points, (size_t)(n * K * 3));
  const int32_t * ix = fr.in(index, (size_t)(n * K * k));
  const float * vp = Vn ? fr.in(viewpoint, (size_t)(Vn * 3)) : nullptr;
  float * on = fr.out(normal, (size_t)(n * K * 3));
  float * oc = fr.out(curvature, (size_t)(n * K));
  int32_t * os = fr.out(status, (size_t)(n * K));
  return fr.run([&] {
    const int total = (int)(n * K);
    cld_normals_kernel<<<dim3((unsigned)((total + CLD_NRM_T - 1) / CLD_NRM_T)), dim3(CLD_NRM_T), 0, fr.st>>>(p, ix, vp, Vn == n && n != 1, total,
                                                                                                           (int)K, k, min_gap, on, oc, os);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_cloud_farthest_points(int device, int64_t n, int64_t K, const float * points, int64_t M, const int32_t * start, int32_t * index,
                                            float * radius_sq, float * min_sqdist, int space, void * stream)
{
  const char * fn = "smplpp_cloud_farthest_points";
  if(n < 0 || K < 0 || M < 0) return cld_refuse(fn, "n, K and M must not be negative");
  if(M < 1 || M > K) return cld_refuse(fn, "M must be in 1..K");
  if(!min_sqdist) return cld_refuse(fn, "min_sqdist is NULL");
  if(n > CLD_INT32_MAX || K > CLD_INT32_MAX || n * K > CLD_INT32_MAX / 3) return cld_refuse(fn, "n K 3 beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(n == 0) return SMPLPP_OK;
  if(!points) return cld_refuse(fn, "points is NULL");
  if(space == SMPLPP_HOST && start)
    for(int64_t f = 0; f < n; f++)
      if(start[f] < 0 || start[f] >= K) return cld_refuse(fn, "start out of range");
  Frame fr(device, nullptr, space, stream, "cloud farthest points");
  const float * p = fr.in(points, (size_t)(n * K * 3));
  const int32_t * s = fr.in(start, (size_t)n);
  int32_t * oi = fr.out(index, (size_t)(n * M));
  float * orad = fr.out(radius_sq, (size_t)(n * M));
  float * od = fr.out(min_sqdist, (size_t)(n * K));
  return fr.run([&] {
    const dim3 grid((unsigned)n), block(CLD_FPS_T);
    if(K <= CLD_FPS_T) cld_fps_kernel<1><<<grid, block, 0, fr.st>>>(p, s, (int)K, (int)M, oi, orad, od);
    else if(K <= CLD_FPS_T * 4)
      cld_fps_kernel<4><<<grid, block, 0, fr.st>>>(p, s, (int)K, (int)M, oi, orad, od);
    else if(K <= CLD_FPS_T * CLD_FPS_PPT)
      cld_fps_kernel<CLD_FPS_PPT><<<grid, block, 0, fr.st>>>(p, s, (int)K, (int)M, oi, orad, od);
    else
      cld_fps_kernel<0><<<grid, block, 0, fr.st>>>(p, s, (int)K, (int)M, oi, orad, od);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
