// The ray casting rule (include/smplpp_hip.h states it in full), shared by the forward scan and the record kernel of
// the backward pass (ray_cast.hip).  fp32, every operation rounded on its own (no contraction to FMA), divisions correctly rounded.
//
// Per ray: kz = the axis of the largest |dir| (lowest on a tie), kx = kz + 1, ky = kz + 2 (mod 3), Sx = dir[kx] / dir[kz],
// Sy = dir[ky] / dir[kz]; dead when a coordinate of origin or dir is not finite or dir[kz] == 0 (then Sx = Sy = NaN, which covers
// nothing).  Per (ray, vertex): P = x - origin, X = P[kx] - Sx P[kz], Y = P[ky] - Sy P[kz]: the vertex in the ray's sheared plane,
// two fp32 numbers that no face enters.  Per edge p -> q of a face, in stored corner order: e = the sign of the EXACT
// X_p Y_q - Y_p X_q, decided on the two rounded fp32 products where they differ (rounding is monotone) and in fp64, where the
// products are exact, where they are equal; a zero takes the sign of Y_p - Y_q, else of X_q - X_p: the sign the edge function has
// when the ray is shifted by (eps, eps^2) in its plane, so that a ray through a shared edge or a vertex of a closed mesh is inside
// exactly the faces a generic ray next to it is inside.  A face is covered with sign s when its three edges have e = s.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int RAY_FRONT = 1, RAY_BACK = 2;
constexpr unsigned long long RAY_NONE = ~0ull; // the key of a ray that nothing has hit

struct Ray
{
  float o[3], d[3];
  float Sx, Sy;
  int kz;
  bool neg;  // dir[kz] < 0
  bool dead;
};

__device__ __forceinline__ float ray_pick(int k, float a0, float a1, float a2)
{
  return k == 0 ? a0 : (k == 1 ? a1 : a2);
}

__device__ __forceinline__ Ray ray_setup(const float * __restrict__ o, const float * __restrict__ d)
{
  Ray r;
  for(int x = 0; x < 3; x++) r.o[x] = o[x], r.d[x] = d[x];
  const float a0 = fabsf(r.d[0]), a1 = fabsf(r.d[1]), a2 = fabsf(r.d[2]);
  r.kz = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
  const float dz = ray_pick(r.kz, r.d[0], r.d[1], r.d[2]);
  const float dx = ray_pick(r.kz, r.d[1], r.d[2], r.d[0]), dy = ray_pick(r.kz, r.d[2], r.d[0], r.d[1]);
  bool fin = true;
  for(int x = 0; x < 3; x++) fin = fin && fabsf(r.o[x]) < INFINITY && fabsf(r.d[x]) < INFINITY; // (a NaN fails)
  r.dead = !fin || dz == 0.0f;
  r.neg = dz < 0.0f;
  r.Sx = r.dead ? NAN : dx / dz;
  r.Sy = r.dead ? NAN : dy / dz;
  return r;
}

// the sign of an edge whose rounded products are equal (rare: the ray within an ulp of the edge's line): +1, -1, or 0 for a
// projected edge of no length
__device__ __forceinline__ int ray_edge_tie(float Xp, float Yp, float Xq, float Yq)
{
  const double p1 = (double)Xp * (double)Yq, p2 = (double)Yp * (double)Xq; // exact
  if(p1 != p2) return p1 > p2 ? 1 : -1;
  if(Yp != Yq) return Yp > Yq ? 1 : -1;
  if(Xq != Xp) return Xq > Xp ? 1 : -1;
  return 0;
}

// the range of the ray on the plane of the face tri = (a, b, c): n = (b - a) x (c - a), na = n . (a - origin), nd = n . dir
struct RayPlane
{
  float A[3], e1[3], e2[3], n[3], na, nd, t;
};
__device__ __forceinline__ RayPlane ray_plane(const Ray & r, const float * tri)
{
  RayPlane p;
  for(int x = 0; x < 3; x++) p.A[x] = tri[x] - r.o[x], p.e1[x] = tri[3 + x] - tri[x], p.e2[x] = tri[6 + x] - tri[x];
  p.n[0] = p.e1[1] * p.e2[2] - p.e1[2] * p.e2[1];
  p.n[1] = p.e1[2] * p.e2[0] - p.e1[0] * p.e2[2];
  p.n[2] = p.e1[0] * p.e2[1] - p.e1[1] * p.e2[0];
  p.na = (p.n[0] * p.A[0] + p.n[1] * p.A[1]) + p.n[2] * p.A[2];
  p.nd = (p.n[0] * r.d[0] + p.n[1] * r.d[1]) + p.n[2] * r.d[2];
  p.t = p.na / p.nd;
  return p;
}

// barycentrics (of a, b, c) of the point t dir on the plane, as the depth rasteriser forms them (dr_bary)
__device__ __forceinline__ void ray_bary(const Ray & r, const RayPlane & p, float t, float * beta)
{
  const float wx = t * r.d[0] - p.A[0], wy = t * r.d[1] - p.A[1], wz = t * r.d[2] - p.A[2];
  const float nn = (p.n[0] * p.n[0] + p.n[1] * p.n[1]) + p.n[2] * p.n[2];
  const float px = wy * p.e2[2] - wz * p.e2[1], py = wz * p.e2[0] - wx * p.e2[2], pz = wx * p.e2[1] - wy * p.e2[0]; // w x e2
  const float qx = p.e1[1] * wz - p.e1[2] * wy, qy = p.e1[2] * wx - p.e1[0] * wz, qz = p.e1[0] * wy - p.e1[1] * wx; // e1 x w
  beta[1] = ((px * p.n[0] + py * p.n[1]) + pz * p.n[2]) / nn;
  beta[2] = ((qx * p.n[0] + qy * p.n[1]) + qz * p.n[2]) / nn;
  beta[0] = (1.0f - beta[1]) - beta[2];
}

// One (ray, face): 0 when the face is not covered, under `facing`, or out of (t_min, t_max]; else RAY_FRONT or RAY_BACK with its
// range in t.  tri holds a, b, c (all NaN for a face with a corner that is not finite: it covers nothing).
__device__ __forceinline__ int ray_face(const Ray & r, const float * tri, float t_min, float t_max, int facing, float & t)
{
  float X[3], Y[3];
#pragma unroll
  for(int v = 0; v < 3; v++)
  {
    const float p0 = tri[3 * v] - r.o[0], p1 = tri[3 * v + 1] - r.o[1], p2 = tri[3 * v + 2] - r.o[2];
    const float pz = ray_pick(r.kz, p0, p1, p2);
    X[v] = ray_pick(r.kz, p1, p2, p0) - r.Sx * pz;
    Y[v] = ray_pick(r.kz, p2, p0, p1) - r.Sy * pz;
  }
  bool ge = true, le = true, tie = false; // no edge yet says -, no edge yet says +, some edge's products are equal
  float m1[3], m2[3];
#pragma unroll
  for(int e = 0; e < 3; e++)
  {
    const int p = e, q = e == 2 ? 0 : e + 1;
    m1[e] = X[p] * Y[q], m2[e] = Y[p] * X[q];
    ge = ge && m1[e] >= m2[e]; // (a NaN fails both)
    le = le && m1[e] <= m2[e];
    tie = tie || m1[e] == m2[e];
  }
  if(!(ge || le)) return 0;
  int s = ge ? 1 : -1;
  if(tie) // rare: the exact signs
  {
    int sg[3];
#pragma unroll
    for(int e = 0; e < 3; e++)
    {
      const int p = e, q = e == 2 ? 0 : e + 1;
      sg[e] = m1[e] > m2[e] ? 1 : (m1[e] < m2[e] ? -1 : ray_edge_tie(X[p], Y[p], X[q], Y[q]));
    }
    if(sg[0] == 0 || sg[0] != sg[1] || sg[1] != sg[2]) return 0;
    s = sg[0];
  }
  const int side = ((s > 0) != r.neg) ? RAY_BACK : RAY_FRONT; // front: s sign(dir[kz]) < 0
  if(!(facing & side)) return 0;
  const RayPlane p = ray_plane(r, tri);
  if(!(fabsf(p.t) < INFINITY && p.t > t_min && p.t <= t_max)) return 0;
  t = p.t;
  return side;
}
} // namespace smplpp_hip
