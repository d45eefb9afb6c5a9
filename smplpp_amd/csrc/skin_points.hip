// Skinning of bound points and its inverse: points that are not the model's vertices, carried by the blend of the world
// joint transforms of smplpp_skeleton, brought back to the rest pose by the inverse of that blend, and the vector-Jacobian products
// of both to the points, the transforms, the rest joints and a dense weight binding.  The rules are in include/smplpp_hip.h; every
// fp32 operation below is rounded on its own (no contraction to FMA), '/' is the correctly rounded one, every output element is one
// fixed-order sum, and there are no floating-point atomics and no workspace.
//
//  sp_point_kernel<MODE>   over (chunk of 256 points x range of frames).  A workgroup puts `ft` frames' 24 x 12 floats of [A_j | c_j]
//                          into LDS at a time (ft x 1152 bytes, sized at launch); a lane owns a POINT, since it needs all three rows
//                          of the blend, and walks the frames in ascending order.  Per-frame outputs are stored as they are made;
//                          an output shared by the frames (point_frames = 1 or bind_frames = 1 in a backward) is summed in the
//                          lane's registers by the two-level tile rule of smplpp_vertex_offsets_vjp, and then the workgroup's range
//                          is all n frames.  ft only shapes the launch: no bit depends on it.
//                            SP_SKIN, SP_UNSKIN          out, blend, valid
//                            SP_SKIN_VJP, SP_UNSKIN_VJP  grad_points, grad_weights
//  sp_joint_kernel<UNSKIN, NQ>  the sums over the points, a team per (frame, joint) by frame_sum_split(K): NQ = 0 a wavefront, lane k
//                          owns point k; NQ = 4 or 1 a workgroup of 256 or 1024, thread t owns the partials t + T q of sum1024 for the
//                          three entries of dc and the nine of dR.  A point whose weight on the joint is 0 is passed over before
//                          anything else of it is read; the others recompute their forward by sp_point, as sp_point_kernel does, so
//                          the bits of a value do not depend on which outputs are asked for.  Thread 0 writes the joint's rows of
//                          grad_world and grad_joints.
#include "common.h"
#include "fixed_sum.h"
#include "staging.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int SP_T = 256;                         // threads of sp_point_kernel
constexpr int SP_FT = SMPLPP_VERTEX_OFFSETS_TILE; // frames per tile of the shared sums (and the most a workgroup holds in LDS)
constexpr int SP_X = NJ * 12;                     // floats of a frame's [A_j | c_j] in LDS
enum { SP_SKIN = 0, SP_UNSKIN = 1, SP_SKIN_VJP = 2, SP_UNSKIN_VJP = 3 };

struct SpArgs
{
  const float * world;   // [n][24][3][4]
  const float * joints;  // [n][24][3]
  const float * points;  // [point_frames][K][3]
  const int64_t * face;  // [bind_frames][K]      face binding ...
  const float * bary;    // [bind_frames][K][3]
  const float * weights; // [bind_frames][K][24]  ... or weight binding
  const uint8_t * wIdx;  // the model's kept weights (face binding)
  const float * wVal;
  const int32_t * faces;
  int n, K, F, maxw;
  int p_per_frame, b_per_frame; // 0: shared by all frames
};

// one point of one frame after the forward's operations
struct SpPoint
{
  float s, M[9], t[3]; // the blend: M[3 a + b]
  float x[3];          // the point as given
  float o[3];          // the forward's output
  float C[9], det;     // unskin: the cofactors and the determinant
  bool live;
};

__device__ inline bool sp_finite(float v)
{
  return fabsf(v) < INFINITY;
}

__device__ inline void sp_store(float * p, float v, int accumulate)
{
  *p = accumulate ? *p + v : v;
}

// a frame's [A_j | c_j] into LDS: c_j[a] = p_j[a] - ((A_j[a][0] J_j[0] + A_j[a][1] J_j[1]) + A_j[a][2] J_j[2])
__device__ inline void sp_stage(float * __restrict__ sX, const SpArgs & a, int f0, int nf, int tid, int T)
{
  for(int i = tid; i < nf * NJ * 3; i += T)
  {
    const int fl = i / (NJ * 3), e = i - fl * (NJ * 3), j = e / 3, r = e - j * 3;
    const float * w = a.world + ((f0 + fl) * NJ + j) * 12 + r * 4;
    const float * J = a.joints + ((f0 + fl) * NJ + j) * 3;
    float * d = sX + fl * SP_X + j * 12 + r * 4;
    const float A0 = w[0], A1 = w[1], A2 = w[2];
    d[0] = A0, d[1] = A1, d[2] = A2;
    d[3] = w[3] - ((A0 * J[0] + A1 * J[1]) + A2 * J[2]);
  }
}

// the face binding's weight of one joint: (bary0 W[v0][j] + bary1 W[v1][j]) + bary2 W[v2][j], W = 0 where the model keeps none
__device__ inline float sp_face_weight(const SpArgs & a, const int32_t * __restrict__ tri, const float (&b)[3], int j)
{
  float w[3];
#pragma unroll
  for(int c = 0; c < 3; c++)
  {
    const uint8_t * wi = a.wIdx + (int64_t)tri[c] * a.maxw;
    const float * wv = a.wVal + (int64_t)tri[c] * a.maxw;
    w[c] = 0.0f;
    for(int q = 0; q < a.maxw; q++)
      if((int)wi[q] == j && wv[q] != 0.0f) w[c] = wv[q];
  }
  return (b[0] * w[0] + b[1] * w[1]) + b[2] * w[2];
}

// fn(j, w) for the joints with w != 0 in ascending j; false when the binding makes the point dead (a face id out of range, through
// which nothing is read, or a bary or weight that is not finite: then fn may have seen values that are not finite)
template<class Fn>
__device__ inline bool sp_weights(const SpArgs & a, int f, int k, Fn fn)
{
  const int row = (a.b_per_frame ? f * a.K : 0) + k;
  bool fin = true;
  if(a.weights)
  {
    const float * wr = a.weights + (int64_t)row * NJ;
#pragma unroll 4
    for(int j = 0; j < NJ; j++)
    {
      const float w = wr[j];
      fin = fin && sp_finite(w);
      if(w != 0.0f) fn(j, w);
    }
    return fin;
  }
  const int64_t t = a.face[row];
  if(t < 0 || t >= a.F) return false;
  const float b[3] = {a.bary[(int64_t)row * 3], a.bary[(int64_t)row * 3 + 1], a.bary[(int64_t)row * 3 + 2]};
  if(!(sp_finite(b[0]) && sp_finite(b[1]) && sp_finite(b[2]))) return false;
  const int32_t * tri = a.faces + t * 3;
  const uint8_t * wi[3];
  const float * wv[3];
  int q[3];
#pragma unroll
  for(int c = 0; c < 3; c++) wi[c] = a.wIdx + (int64_t)tri[c] * a.maxw, wv[c] = a.wVal + (int64_t)tri[c] * a.maxw, q[c] = 0;
  for(;;) // a three-way merge of the corners' ascending joint lists (entries of value 0 are padding)
  {
    int jc[3], j = NJ;
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      while(q[c] < a.maxw && wv[c][q[c]] == 0.0f) q[c]++;
      jc[c] = q[c] < a.maxw ? (int)wi[c][q[c]] : NJ;
      j = jc[c] < j ? jc[c] : j;
    }
    if(j >= NJ) break;
    float w[3];
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      w[c] = jc[c] == j ? wv[c][q[c]] : 0.0f;
      if(jc[c] == j) q[c]++;
    }
    const float om = (b[0] * w[0] + b[1] * w[1]) + b[2] * w[2];
    if(om != 0.0f) fn(j, om);
  }
  return true;
}

// the point's weight on joint j alone, 0 for a face id out of range (the same bits as sp_weights hands to fn)
__device__ inline float sp_weight_of(const SpArgs & a, int f, int k, int j)
{
  const int row = (a.b_per_frame ? f * a.K : 0) + k;
  if(a.weights) return a.weights[(int64_t)row * NJ + j];
  const int64_t t = a.face[row];
  if(t < 0 || t >= a.F) return 0.0f;
  const float b[3] = {a.bary[(int64_t)row * 3], a.bary[(int64_t)row * 3 + 1], a.bary[(int64_t)row * 3 + 2]};
  return sp_face_weight(a, a.faces + t * 3, b, j);
}

// sX: the frame's [A_j | c_j]
template<bool UNSKIN>
__device__ inline void sp_point(const SpArgs & a, const float * __restrict__ sX, int f, int k, SpPoint & z)
{
  const float * p = a.points + (int64_t)((a.p_per_frame ? f * a.K : 0) + k) * 3;
  z.x[0] = p[0], z.x[1] = p[1], z.x[2] = p[2];
  float s = 0.0f, M[9], t[3];
#pragma unroll
  for(int e = 0; e < 9; e++) M[e] = 0.0f;
  t[0] = t[1] = t[2] = 0.0f;
  bool live = sp_weights(a, f, k, [&](int j, float w) {
    const float * X = sX + j * 12;
    s = s + w;
#pragma unroll
    for(int r = 0; r < 3; r++)
    {
#pragma unroll
      for(int b = 0; b < 3; b++) M[3 * r + b] = M[3 * r + b] + w * X[4 * r + b];
      t[r] = t[r] + w * X[4 * r + 3];
    }
  });
  live = live && sp_finite(z.x[0]) && sp_finite(z.x[1]) && sp_finite(z.x[2]) && s > 0.0f;
  z.s = s;
#pragma unroll
  for(int e = 0; e < 9; e++) z.M[e] = M[e];
#pragma unroll
  for(int r = 0; r < 3; r++) z.t[r] = t[r];
  z.det = 0.0f;
  if constexpr(!UNSKIN)
  {
#pragma unroll
    for(int r = 0; r < 3; r++)
    {
      const float h = ((M[3 * r] * z.x[0] + M[3 * r + 1] * z.x[1]) + M[3 * r + 2] * z.x[2]) + t[r];
      z.o[r] = h / s;
    }
  }
  else
  {
    float q[3];
#pragma unroll
    for(int r = 0; r < 3; r++) q[r] = s * z.x[r] - t[r];
#pragma unroll
    for(int r = 0; r < 3; r++)
#pragma unroll
      for(int b = 0; b < 3; b++)
      {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        z.C[3 * r + b] = M[3 * r1 + b1] * M[3 * r2 + b2] - M[3 * r1 + b2] * M[3 * r2 + b1];
      }
    const float det = (M[0] * z.C[0] + M[1] * z.C[1]) + M[2] * z.C[2];
    z.det = det;
    live = live && fabsf(det) > ((SMPLPP_UNSKIN_MIN_DET * s) * s) * s;
#pragma unroll
    for(int b = 0; b < 3; b++) z.o[b] = ((z.C[b] * q[0] + z.C[3 + b] * q[1]) + z.C[6 + b] * q[2]) / det;
  }
  z.live = live;
}

// what the backward passes pull to the blend: gt (skin: g / s; unskin: -u, with u = (C g) / det)
template<bool UNSKIN>
__device__ inline void sp_pull(const SpPoint & z, const float (&g)[3], float (&gt)[3], float (&u)[3])
{
#pragma unroll
  for(int r = 0; r < 3; r++)
  {
    if constexpr(UNSKIN)
    {
      u[r] = ((z.C[3 * r] * g[0] + z.C[3 * r + 1] * g[1]) + z.C[3 * r + 2] * g[2]) / z.det;
      gt[r] = -u[r];
    }
    else
    {
      gt[r] = g[r] / z.s;
      u[r] = gt[r];
    }
  }
}

// a sum over the frames by the two-level tile rule: tiles of SP_FT frames, ascending within a tile from its first term, then across
// the tiles from the first tile's sum (the caller walks f = 0 .. n - 1 in order)
struct SpTileSum
{
  float tile, tot;
  __device__ inline void add(int f, int n, float term)
  {
    tile = f % SP_FT == 0 ? term : tile + term;
    if(f % SP_FT == SP_FT - 1 || f == n - 1) tot = f < SP_FT ? tile : tot + tile;
  }
};

struct SpOut
{
  float *out, *blend; // forward: [n][K][3], [n][K][3][4]
  uint8_t * valid;    // [n][K]
  const float * g;    // backward: grad_out [n][K][3]
  float *gpoints, *gweights;
  int gp_shared, gw_shared, accumulate;
};

// grid: chunks of SP_T points x groups of `fpg` frames (fpg = ft, or n when an output is shared); dynamic LDS: ft SP_X floats
template<int MODE>
__global__ __launch_bounds__(SP_T) void sp_point_kernel(SpArgs a, SpOut o, int ft, int fpg, int nchunk)
{
  constexpr bool UNSKIN = MODE == SP_UNSKIN || MODE == SP_UNSKIN_VJP;
  extern __shared__ float sX[]; // [ft][SP_X]
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % nchunk, group = blockIdx.x / nchunk;
  const int g0 = group * fpg, g1 = min(a.n, g0 + fpg);
  const int k = chunk * SP_T + tid;
  const bool own = k < a.K;
  SpTileSum sp[3] = {}, sw[(MODE == SP_SKIN_VJP || MODE == SP_UNSKIN_VJP) ? NJ : 1] = {};
  for(int fb = g0; fb < g1; fb += ft)
  {
    const int nf = min(ft, g1 - fb);
    __syncthreads();
    sp_stage(sX, a, fb, nf, tid, SP_T);
    __syncthreads();
    if(!own) continue;
    for(int fl = 0; fl < nf; fl++)
    {
      const int f = fb + fl, at = f * a.K + k;
      const float * X = sX + fl * SP_X;
      SpPoint z;
      sp_point<UNSKIN>(a, X, f, k, z);
      if constexpr(MODE == SP_SKIN || MODE == SP_UNSKIN)
      {
#pragma unroll
        for(int r = 0; r < 3; r++) o.out[at * 3 + r] = z.live ? z.o[r] : 0.0f;
        if(o.blend)
#pragma unroll
          for(int r = 0; r < 3; r++)
          {
#pragma unroll
            for(int b = 0; b < 3; b++) o.blend[at * 12 + 4 * r + b] = z.live ? z.M[3 * r + b] / z.s : 0.0f;
            o.blend[at * 12 + 4 * r + 3] = z.live ? z.t[r] / z.s : 0.0f;
          }
        if(o.valid) o.valid[at] = z.live ? 1 : 0;
      }
      else
      {
        const float g[3] = {o.g[at * 3], o.g[at * 3 + 1], o.g[at * 3 + 2]};
        float gt[3], u[3];
        sp_pull<UNSKIN>(z, g, gt, u);
        if(o.gpoints)
#pragma unroll
          for(int b = 0; b < 3; b++)
          {
            float v = 0.0f;
            if(z.live) v = UNSKIN ? z.s * u[b] : (z.M[b] * gt[0] + z.M[3 + b] * gt[1]) + z.M[6 + b] * gt[2];
            if(o.gp_shared) sp[b].add(f, a.n, v);
            else sp_store(o.gpoints + at * 3 + b, v, o.accumulate);
          }
        if(o.gweights)
        {
          // skin: the rest point x goes through joint j and is compared with the output; unskin: the recomputed rest point
          // goes through joint j and is compared with the posed point given
          const float * xr = UNSKIN ? z.o : z.x;
          const float * cmp = UNSKIN ? z.x : z.o;
#pragma unroll
          for(int j = 0; j < NJ; j++)
          {
            float v = 0.0f;
            if(z.live)
            {
              float d[3];
#pragma unroll
              for(int r = 0; r < 3; r++)
              {
                const float rj = ((X[j * 12 + 4 * r] * xr[0] + X[j * 12 + 4 * r + 1] * xr[1]) + X[j * 12 + 4 * r + 2] * xr[2]) + X[j * 12 + 4 * r + 3];
                d[r] = UNSKIN ? cmp[r] - rj : rj - cmp[r];
              }
              v = (u[0] * d[0] + u[1] * d[1]) + u[2] * d[2];
            }
            if(o.gw_shared) sw[j].add(f, a.n, v);
            else sp_store(o.gweights + at * NJ + j, v, o.accumulate);
          }
        }
      }
    }
  }
  if constexpr(MODE == SP_SKIN_VJP || MODE == SP_UNSKIN_VJP)
  {
    if(!own) return;
    if(o.gpoints && o.gp_shared)
#pragma unroll
      for(int b = 0; b < 3; b++) sp_store(o.gpoints + k * 3 + b, sp[b].tot, o.accumulate);
    if(o.gweights && o.gw_shared)
#pragma unroll
      for(int j = 0; j < NJ; j++) sp_store(o.gweights + k * NJ + j, sw[j].tot, o.accumulate);
  }
}

// grid: n x 24 (frame, joint) items; NQ = 0: 64 threads, else 1024 / NQ
template<bool UNSKIN, int NQ>
__global__ __launch_bounds__(NQ ? 1024 / NQ : 64) void sp_joint_kernel(SpArgs a, const float * __restrict__ gout, float * gworld, float * gjoints,
                                                                       int accumulate)
{
  constexpr int T = NQ ? 1024 / NQ : 64, NP = NQ ? NQ : 1;
  __shared__ float sX[SP_X];
  __shared__ float cross[2][3][SUM1024_WAVES];
  const int t = (int)threadIdx.x, f = (int)blockIdx.x / NJ, j = (int)blockIdx.x % NJ;
  sp_stage(sX, a, f, 1, t, T);
  __syncthreads();
  float part[12][NP]; // dc[0..2], dR[3 a + b] at 3 + 3 a + b
#pragma unroll
  for(int e = 0; e < 12; e++)
#pragma unroll
    for(int q = 0; q < NP; q++) part[e][q] = 0.0f;
  for(int k0 = 0; k0 < a.K; k0 += 1024)
#pragma unroll
    for(int q = 0; q < NP; q++)
    {
      const int k = k0 + T * q + t;
      if(k >= a.K) continue;
      const float om = sp_weight_of(a, f, k, j);
      if(om == 0.0f) continue;
      SpPoint z;
      sp_point<UNSKIN>(a, sX, f, k, z);
      if(!z.live) continue;
      const int at = f * a.K + k;
      const float g[3] = {gout[at * 3], gout[at * 3 + 1], gout[at * 3 + 2]};
      float gt[3], u[3];
      sp_pull<UNSKIN>(z, g, gt, u);
      const float * x = UNSKIN ? z.o : z.x;
#pragma unroll
      for(int r = 0; r < 3; r++)
      {
        const float wg = om * gt[r];
        part[r][q] = part[r][q] + wg;
#pragma unroll
        for(int b = 0; b < 3; b++) part[3 + 3 * r + b][q] = part[3 + 3 * r + b][q] + wg * x[b];
      }
    }
  float sum[12];
  if constexpr(NQ == 0)
  {
    // K <= 64: the partials past 63 are +0 and their meetings are left out
#pragma unroll
    for(int e = 0; e < 12; e++) sum[e] = part[e][0];
    sum64_meet(sum);
  }
  else if constexpr(NQ == 1)
  {
    int turn = 0;
#pragma unroll
    for(int e = 0; e < 12; e += 3) // three sums a meeting (every thread of the workgroup calls)
    {
      float v[3] = {part[e][0], part[e + 1][0], part[e + 2][0]};
      sum1024_meet_many<3, 0u>(v, cross, turn);
      sum[e] = v[0], sum[e + 1] = v[1], sum[e + 2] = v[2];
    }
  }
  else
  {
#pragma unroll
    for(int e = 0; e < 12; e++)
    {
      sum[e] = sum1024_meet<NQ>(part[e], &cross[0][0][0]);
      __syncthreads(); // `cross` is written again by the next sum
    }
  }
  if(t != 0) return;
  const float * A = sX + j * 12;
  const float * J = a.joints + (f * NJ + j) * 3;
  if(gworld)
#pragma unroll
    for(int r = 0; r < 3; r++)
    {
#pragma unroll
      for(int b = 0; b < 3; b++) sp_store(gworld + (f * NJ + j) * 12 + 4 * r + b, sum[3 + 3 * r + b] - sum[r] * J[b], accumulate);
      sp_store(gworld + (f * NJ + j) * 12 + 4 * r + 3, sum[r], accumulate);
    }
  if(gjoints)
#pragma unroll
    for(int b = 0; b < 3; b++) sp_store(gjoints + (f * NJ + j) * 3 + b, -((A[b] * sum[0] + A[4 + b] * sum[1]) + A[8 + b] * sum[2]), accumulate);
}

static int sp_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

// what the four calls refuse alike (the host-space face ids are looked at last)
static int sp_check(const char * fn, smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                    int64_t point_frames, const int64_t * face, const float * bary, const float * weights, int64_t bind_frames, int space)
{
  if(!m) return sp_refuse(fn, "no model");
  if(n <= 0 || K <= 0) return sp_refuse(fn, "n and K must be positive");
  if(!world || !joints || !points) return sp_refuse(fn, "world, joints or points is NULL");
  if(weights ? (face || bary) : !(face && bary)) return sp_refuse(fn, "give face and bary, or weights, not both");
  if(face && m->F <= 0) return sp_refuse(fn, "a face binding needs a model with faces");
  if(point_frames != 1 && point_frames != n) return sp_refuse(fn, "point_frames must be 1 or n");
  if(bind_frames != 1 && bind_frames != n) return sp_refuse(fn, "bind_frames must be 1 or n");
  if(n > 0x7fffffffLL || K > 0x7fffffffLL || n * K > 0x7fffffffLL / NJ || n > 0x7fffffffLL / (NJ * 12))
    return sp_refuse(fn, "n * K * 24 or n * 288 beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(face && space == SMPLPP_HOST) return ids_in(fn, "face id", face, bind_frames * K, 0, m->F);
  return SMPLPP_OK;
}

static SpArgs sp_args(Frame & fr, smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                      int64_t point_frames, const int64_t * face, const float * bary, const float * weights, int64_t bind_frames)
{
  SpArgs a = {};
  a.world = fr.in(world, (size_t)(n * NJ * 12));
  a.joints = fr.in(joints, (size_t)(n * NJ * 3));
  a.points = fr.in(points, (size_t)(point_frames * K * 3));
  a.face = fr.in(face, (size_t)(bind_frames * K));
  a.bary = fr.in(bary, (size_t)(bind_frames * K * 3));
  a.weights = fr.in(weights, (size_t)(bind_frames * K * NJ));
  a.wIdx = m->wIdx.get(), a.wVal = m->wVal.get(), a.faces = m->faces.get();
  a.n = (int)n, a.K = (int)K, a.F = (int)m->F, a.maxw = m->maxw;
  a.p_per_frame = point_frames != 1, a.b_per_frame = bind_frames != 1;
  return a;
}

// frames a workgroup holds in LDS: halved until the grid has eight workgroups per compute unit, or what the model's environment fixed
static int sp_frames(smplpp_model * m, int64_t n, int64_t K)
{
  if(m->sp_frames > 0) return m->sp_frames;
  const int64_t chunks = (K + SP_T - 1) / SP_T, want = 8 * (int64_t)device_cus(m->device);
  int ft = SP_FT;
  while(ft > 1 && ((n + ft - 1) / ft) * chunks < want) ft /= 2;
  return ft;
}

template<int MODE>
static int sp_launch_points(smplpp_model * m, const SpArgs & a, const SpOut & o, hipStream_t st)
{
  const bool shared = (o.gpoints && o.gp_shared) || (o.gweights && o.gw_shared);
  const int ft = sp_frames(m, a.n, a.K), fpg = shared ? a.n : ft;
  const int nchunk = (a.K + SP_T - 1) / SP_T, ngroup = (a.n + fpg - 1) / fpg;
  sp_point_kernel<MODE><<<dim3((unsigned)nchunk * (unsigned)ngroup), dim3(SP_T), sizeof(float) * SP_X * (size_t)ft, st>>>(a, o, ft, fpg, nchunk);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

template<bool UNSKIN>
static int sp_launch_joints(smplpp_model * m, const SpArgs & a, const float * g, float * gworld, float * gjoints, int accumulate, hipStream_t st)
{
  int nq = frame_sum_split(a.K).nq;
  if(m->sp_split == 1 || m->sp_split == 4) nq = m->sp_split; // (the wavefront form holds 64 points: it cannot be forced above that)
  const dim3 G((unsigned)a.n * NJ);
  if(nq == 0) sp_joint_kernel<UNSKIN, 0><<<G, dim3(64), 0, st>>>(a, g, gworld, gjoints, accumulate);
  else if(nq == 4) sp_joint_kernel<UNSKIN, 4><<<G, dim3(256), 0, st>>>(a, g, gworld, gjoints, accumulate);
  else sp_joint_kernel<UNSKIN, 1><<<G, dim3(1024), 0, st>>>(a, g, gworld, gjoints, accumulate);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

template<bool UNSKIN>
static int sp_forward(const char * fn, const char * trace, smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K,
                      const float * points, int64_t point_frames, const int64_t * face, const float * bary, const float * weights,
                      int64_t bind_frames, float * out, float * blend, uint8_t * valid, int space, void * stream)
{
  if(int rc = sp_check(fn, m, n, world, joints, K, points, point_frames, face, bary, weights, bind_frames, space)) return rc;
  if(!out) return sp_refuse(fn, "out is NULL");
  Frame fr(m->device, &m->arena, space, stream, trace);
  const SpArgs a = sp_args(fr, m, n, world, joints, K, points, point_frames, face, bary, weights, bind_frames);
  SpOut o = {};
  o.out = fr.out(out, (size_t)(n * K * 3));
  o.blend = fr.out(blend, (size_t)(n * K * 12));
  o.valid = fr.out(valid, (size_t)(n * K));
  return fr.run([&] { return sp_launch_points<UNSKIN ? SP_UNSKIN : SP_SKIN>(m, a, o, fr.st); });
}

template<bool UNSKIN>
static int sp_backward(const char * fn, const char * trace, smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K,
                       const float * points, int64_t point_frames, const int64_t * face, const float * bary, const float * weights,
                       int64_t bind_frames, const float * grad_out, float * grad_points, float * grad_world, float * grad_joints,
                       float * grad_weights, int accumulate, int space, void * stream)
{
  if(int rc = sp_check(fn, m, n, world, joints, K, points, point_frames, face, bary, weights, bind_frames, space)) return rc;
  if(!grad_out) return sp_refuse(fn, "grad_out is NULL");
  if(!grad_points && !grad_world && !grad_joints && !grad_weights) return sp_refuse(fn, "every gradient is NULL");
  if(grad_weights && !weights) return sp_refuse(fn, "grad_weights needs a weight binding");
  if(accumulate != 0 && accumulate != 1) return sp_refuse(fn, "accumulate must be 0 or 1");
  Frame fr(m->device, &m->arena, space, stream, trace);
  const SpArgs a = sp_args(fr, m, n, world, joints, K, points, point_frames, face, bary, weights, bind_frames);
  SpOut o = {};
  o.g = fr.in(grad_out, (size_t)(n * K * 3));
  o.gpoints = fr.out(grad_points, (size_t)(point_frames * K * 3), accumulate != 0);
  float * gw = fr.out(grad_world, (size_t)(n * NJ * 12), accumulate != 0);
  float * gj = fr.out(grad_joints, (size_t)(n * NJ * 3), accumulate != 0);
  o.gweights = fr.out(grad_weights, (size_t)(bind_frames * K * NJ), accumulate != 0);
  o.gp_shared = point_frames == 1 && n > 1, o.gw_shared = bind_frames == 1 && n > 1, o.accumulate = accumulate;
  return fr.run([&] {
    if(o.gpoints || o.gweights)
      if(int rc = sp_launch_points<UNSKIN ? SP_UNSKIN_VJP : SP_SKIN_VJP>(m, a, o, fr.st)) return rc;
    if(gw || gj)
      if(int rc = sp_launch_joints<UNSKIN>(m, a, o.g, gw, gj, accumulate, fr.st)) return rc;
    return (int)SMPLPP_OK;
  });
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_skin_points(smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                                  int64_t point_frames, const int64_t * face, const float * bary, const float * weights, int64_t bind_frames,
                                  float * out, float * blend, uint8_t * valid, int space, void * stream)
{
  return sp_forward<false>("smplpp_skin_points", "skin points", m, n, world, joints, K, points, point_frames, face, bary, weights, bind_frames,
                           out, blend, valid, space, stream);
}

extern "C" int smplpp_unskin_points(smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                                    int64_t point_frames, const int64_t * face, const float * bary, const float * weights, int64_t bind_frames,
                                    float * out, float * blend, uint8_t * valid, int space, void * stream)
{
  return sp_forward<true>("smplpp_unskin_points", "unskin points", m, n, world, joints, K, points, point_frames, face, bary, weights,
                          bind_frames, out, blend, valid, space, stream);
}

extern "C" int smplpp_skin_points_vjp(smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                                      int64_t point_frames, const int64_t * face, const float * bary, const float * weights,
                                      int64_t bind_frames, const float * grad_out, float * grad_points, float * grad_world, float * grad_joints,
                                      float * grad_weights, int accumulate, int space, void * stream)
{
  return sp_backward<false>("smplpp_skin_points_vjp", "skin points VJP", m, n, world, joints, K, points, point_frames, face, bary, weights,
                            bind_frames, grad_out, grad_points, grad_world, grad_joints, grad_weights, accumulate, space, stream);
}

extern "C" int smplpp_unskin_points_vjp(smplpp_model * m, int64_t n, const float * world, const float * joints, int64_t K, const float * points,
                                        int64_t point_frames, const int64_t * face, const float * bary, const float * weights,
                                        int64_t bind_frames, const float * grad_out, float * grad_points, float * grad_world,
                                        float * grad_joints, float * grad_weights, int accumulate, int space, void * stream)
{
  return sp_backward<true>("smplpp_unskin_points_vjp", "unskin points VJP", m, n, world, joints, K, points, point_frames, face, bary, weights,
                           bind_frames, grad_out, grad_points, grad_world, grad_joints, grad_weights, accumulate, space, stream);
}
