// The orientation term on world joint frames and the vector-Jacobian product of smplpp_axis_angle_to_rotmat.
//
// smplpp_orientation_term: per frame f and sensor s, the 3 x C residual E = A O - T of joint joint[s]'s 3 x 3 block A (read in place
// from [n,J,3,row_stride]: smplpp_skeleton's `world` at row_stride 4, a stack of matrices at 3) against a target, a plain or
// Geman-McClure energy of it, and the frame's energy by sum1024.  smplpp_orientation_term_vjp: the gradients to the frames (a gather
// over the sensors of a joint), to the target and to the bone-to-sensor offsets (sum1024 over the frames).  The rules are in
// include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA), '/' is the correctly rounded one,
// and there are no atomics, no workspace and no handle.
//
//  ori_forward_kernel<NQ>   a team per frame by frame_sum_split(S): NQ = 0 a wavefront (four frames a workgroup), lane s owns sensor
//                           s; NQ = 4 or 1 a workgroup of 256 or 1024, thread t owns the partials t + T q.
//  ori_gather_kernel        the backward's per-frame outputs: a thread per (frame, sensor) writes grad_target = -G (Tn = n) and leaves
//                           G O^T in LDS, then a thread per (frame, joint) adds its joint's sensors in ascending s.  A gather:
//                           several sensors may share a joint.
//  ori_across_kernel        the sums across the frames: a workgroup of 1024 per sensor, thread t holding partial t of sum1024 for
//                           every entry of A^T G (grad_offset) and of -G (a shared target).
// Every kernel recomputes the sensor's forward by ori_sensor, so the bits of a value do not depend on which outputs are asked for.
//  rodrigues_vjp_kernel     a thread per (row, m): the contraction of skeleton.hip and fk_vjp.hip with rodrigues_grad_dev.
#include "common.h"
#include "rodrigues_grad.h"

#include "fixed_sum.h"
#include "staging.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int ORI_T = 256;
constexpr int64_t ORI_INT32_MAX = 0x7fffffffLL;

struct OriArgs
{
  const float * frames;  // [n][J][3][rs]
  const int64_t * joint; // [S]
  const float * offset;  // [S][3][C] (nullable: the first C columns of the identity)
  const float * target;  // [Tn][S][3][C]
  const float * weight;  // [Wn][S] (nullable: 1)
  int n, J, rs, S, C;
  int t_per_frame, w_per_frame; // 0: shared by all frames
  float rho;
};
struct OriCot
{
  const float *ge, *gse, *gr; // [n], [n][S], [n][S][3][C]; each may be null (+0)
};

// one sensor of one frame after the forward's operations
struct OriSensor
{
  float A[9], O[9], E[9]; // O, E: entry (r, c) at 3 r + c, c < C
  float w, q;
  int j;
  bool live;
};

__device__ inline bool ori_finite(float v)
{
  return fabsf(v) < INFINITY;
}

__device__ inline void ori_sensor(const OriArgs & a, int f, int s, OriSensor & z)
{
  const int C = a.C;
  z.w = a.weight ? a.weight[(a.w_per_frame ? f * a.S : 0) + s] : 1.0f;
  const int64_t j = a.joint[s];
  z.j = (int)j;
  z.q = 0.0f;
  z.live = z.w != 0.0f && ori_finite(z.w) && j >= 0 && j < a.J;
#pragma unroll
  for(int e = 0; e < 9; e++) z.A[e] = 0.0f, z.O[e] = 0.0f, z.E[e] = 0.0f;
  if(!z.live) return; // (nothing is read through a joint out of range)
  const float * Af = a.frames + (f * a.J + z.j) * (3 * a.rs);
  const float * Tf = a.target + ((a.t_per_frame ? f * a.S : 0) + s) * (3 * C);
  float T[9];
  bool fin = true;
#pragma unroll
  for(int r = 0; r < 3; r++)
#pragma unroll
    for(int c = 0; c < 3; c++)
    {
      z.A[3 * r + c] = Af[r * a.rs + c];
      fin = fin && ori_finite(z.A[3 * r + c]);
      if(c < C)
      {
        z.O[3 * r + c] = a.offset ? a.offset[(s * 3 + r) * C + c] : (r == c ? 1.0f : 0.0f);
        T[3 * r + c] = Tf[r * C + c];
        fin = fin && ori_finite(z.O[3 * r + c]) && ori_finite(T[3 * r + c]);
      }
    }
  z.live = fin;
  if(!fin) return;
#pragma unroll
  for(int r = 0; r < 3; r++)
#pragma unroll
    for(int c = 0; c < 3; c++)
      if(c < C)
      {
        const float m = (z.A[3 * r] * z.O[c] + z.A[3 * r + 1] * z.O[3 + c]) + z.A[3 * r + 2] * z.O[6 + c];
        const float e = m - T[3 * r + c];
        z.E[3 * r + c] = e;
        z.q = z.q + e * e;
      }
}

// sensor_energy of a live sensor
__device__ inline float ori_energy(const OriArgs & a, const OriSensor & z)
{
  if(a.rho == 0.0f) return z.w * z.q;
  const float p2 = a.rho * a.rho;
  return z.w * ((p2 * z.q) / (p2 + z.q));
}

// G = ((2 g) m) E + grad_residual of a live sensor
__device__ inline void ori_pull(const OriArgs & a, const OriCot & g, int f, int s, const OriSensor & z, float (&G)[9])
{
  const int at = f * a.S + s;
  const float gg = (g.ge ? g.ge[f] : 0.0f) + (g.gse ? g.gse[at] : 0.0f);
  float m = z.w;
  if(a.rho != 0.0f)
  {
    const float p2 = a.rho * a.rho;
    const float d = p2 / (p2 + z.q);
    m = z.w * (d * d);
  }
  const float k = (2.0f * gg) * m;
#pragma unroll
  for(int r = 0; r < 3; r++)
#pragma unroll
    for(int c = 0; c < 3; c++)
      G[3 * r + c] = c < a.C ? k * z.E[3 * r + c] + (g.gr ? g.gr[(at * 3 + r) * a.C + c] : 0.0f) : 0.0f;
}

struct OriOut
{
  float *energy, *sensor_energy, *residual;
};

// the sensor's outputs; returns its energy
__device__ inline float ori_emit(const OriArgs & a, const OriOut & o, int f, int s)
{
  OriSensor z;
  ori_sensor(a, f, s, z);
  const float se = z.live ? ori_energy(a, z) : 0.0f;
  const int at = f * a.S + s;
  if(o.sensor_energy) o.sensor_energy[at] = se;
  if(o.residual)
#pragma unroll
    for(int r = 0; r < 3; r++)
#pragma unroll
      for(int c = 0; c < 3; c++)
        if(c < a.C) o.residual[(at * 3 + r) * a.C + c] = z.E[3 * r + c];
  return se;
}

// NQ = 0: grid ceil(n / 4), ORI_T threads; else grid n, 1024 / NQ threads
template<int NQ>
__global__ __launch_bounds__(NQ ? 1024 / NQ : ORI_T) void ori_forward_kernel(OriArgs a, OriOut o)
{
  if constexpr(NQ == 0)
  {
    const int f = (int)(blockIdx.x * (ORI_T / 64) + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if(f >= a.n) return; // (wavefront-uniform; no workgroup barrier in this form)
    float p = 0.0f;
    if(lane < a.S) p = 0.0f + ori_emit(a, o, f, lane); // partial s; the partials past 63 are +0 and left out
    p = sum64_meet(p);
    if(lane == 0 && o.energy) o.energy[f] = p;
  }
  else
  {
    constexpr int T = 1024 / NQ;
    __shared__ float cross[T / 64];
    const int f = blockIdx.x, t = threadIdx.x;
    float part[NQ];
#pragma unroll
    for(int q = 0; q < NQ; q++) part[q] = 0.0f;
    for(int s0 = 0; s0 < a.S; s0 += 1024)
#pragma unroll
      for(int q = 0; q < NQ; q++)
      {
        const int s = s0 + T * q + t;
        if(s < a.S) part[q] = part[q] + ori_emit(a, o, f, s);
      }
    const float e = sum1024_meet<NQ>(part, cross);
    if(t == 0 && o.energy) o.energy[f] = e;
  }
}

// without `energy`: a thread per (frame, sensor)
__global__ __launch_bounds__(ORI_T) void ori_sensors_kernel(OriArgs a, OriOut o)
{
  const int i = (int)(blockIdx.x * ORI_T + threadIdx.x);
  if(i >= a.n * a.S) return;
  ori_emit(a, o, i / a.S, i % a.S);
}

__device__ inline void ori_store(float * p, float v, int accumulate)
{
  *p = accumulate ? *p + v : v;
}

// The backward's per-frame outputs in one launch.  A workgroup takes FT frames and walks the sensors in chunks of SC, FT SC <= ORI_T:
//  step 1  thread (frame, sensor of the chunk) recomputes the sensor, writes grad_target[f][s] = -G (+0 for a dead sensor; Tn = n
//          only) and leaves its share of grad_frames, (G O^T)_rk = sum_c G_rc O_kc (ascending c from the first product), with its
//          joint (-1 when dead) in LDS;
//  step 2  thread (frame, joint) adds the shares of its joint's sensors in ascending s from +0: a gather, several sensors may share
//          a joint, and a joint without a live sensor is stored as +0 (left alone under accumulate).
// The order of the additions does not depend on FT or SC, which follow n and J (a joint count above ORI_T takes the joints in batches,
// step 1 again for each).  Column 3 of a row_stride 4 buffer is never touched.
__global__ __launch_bounds__(ORI_T) void ori_gather_kernel(OriArgs a, OriCot g, float * gframes, float * gtarget, int accumulate, int FT, int SC)
{
  __shared__ float share[ORI_T][9]; // (stride 9: the lanes of step 1 write to distinct banks)
  __shared__ int joint_of[ORI_T];
  const int t = (int)threadIdx.x, f0 = (int)blockIdx.x * FT;
  const int nf = a.n - f0 < FT ? a.n - f0 : FT;
  const int items = gframes ? nf * a.J : 0;
  const int pf = t / SC, pl = t % SC; // step 1: this thread's frame of the tile and sensor of the chunk
  for(int base = 0; base == 0 || base < items; base += ORI_T)
  {
    const int item = base + t;
    const bool own = item < items;
    const int fl = own ? item / a.J : 0, j = own ? item % a.J : -2;
    float acc[9];
#pragma unroll
    for(int e = 0; e < 9; e++) acc[e] = 0.0f;
    bool any = false;
    for(int s0 = 0; s0 < a.S; s0 += SC)
    {
      const int ps = s0 + pl;
      int jn = -1;
      if(pf < nf && ps < a.S)
      {
        const int f = f0 + pf;
        OriSensor z;
        ori_sensor(a, f, ps, z);
        float G[9];
#pragma unroll
        for(int e = 0; e < 9; e++) G[e] = 0.0f;
        if(z.live)
        {
          ori_pull(a, g, f, ps, z, G);
          jn = z.j;
#pragma unroll
          for(int r = 0; r < 3; r++)
#pragma unroll
            for(int k = 0; k < 3; k++)
            {
              float v = G[3 * r] * z.O[3 * k];
#pragma unroll
              for(int c = 1; c < 3; c++)
                if(c < a.C) v = v + G[3 * r + c] * z.O[3 * k + c];
              share[t][3 * r + k] = v;
            }
        }
        if(gtarget && base == 0)
#pragma unroll
          for(int r = 0; r < 3; r++)
#pragma unroll
            for(int c = 0; c < 3; c++)
              if(c < a.C) ori_store(gtarget + ((f * a.S + ps) * 3 + r) * a.C + c, z.live ? -G[3 * r + c] : 0.0f, accumulate);
      }
      joint_of[t] = jn;
      __syncthreads();
      const int lim = a.S - s0 < SC ? a.S - s0 : SC; // the chunk's sensors
      if(own)
        for(int sl = 0; sl < lim; sl++)
        {
          const int slot = fl * SC + sl;
          if(joint_of[slot] != j) continue;
          any = true;
#pragma unroll
          for(int e = 0; e < 9; e++) acc[e] = acc[e] + share[slot][e];
        }
      __syncthreads();
    }
    if(own && !(accumulate && !any))
    {
      float * dst = gframes + ((f0 + fl) * a.J + j) * (3 * a.rs);
#pragma unroll
      for(int r = 0; r < 3; r++)
#pragma unroll
        for(int k = 0; k < 3; k++) ori_store(dst + r * a.rs + k, acc[3 * r + k], accumulate);
    }
  }
}

// The sums across the frames, a workgroup of 1024 per sensor: thread t holds partial t of sum1024 for every entry of grad_offset[s],
// (A^T G)_kc = (A_0k G_0c + A_1k G_1c) + A_2k G_2c, and of the shared grad_target[0][s], -G_kc, over the frames t, t + 1024, ...
// ascending; a dead sensor adds +0.  The partials meet three sums at a time (sum1024_meet_many).
__global__ __launch_bounds__(1024) void ori_across_kernel(OriArgs a, OriCot g, float * goffset, float * gtarget, int accumulate)
{
  __shared__ float cross[2][3][SUM1024_WAVES];
  const int s = (int)blockIdx.x, t = (int)threadIdx.x;
  float po[9], pt[9];
#pragma unroll
  for(int e = 0; e < 9; e++) po[e] = 0.0f, pt[e] = 0.0f;
  for(int f = t; f < a.n; f += 1024)
  {
    OriSensor z;
    ori_sensor(a, f, s, z);
    if(!z.live) continue;
    float G[9];
    ori_pull(a, g, f, s, z, G);
#pragma unroll
    for(int k = 0; k < 3; k++)
#pragma unroll
      for(int c = 0; c < 3; c++)
        if(c < a.C)
        {
          po[3 * k + c] = po[3 * k + c] + ((z.A[k] * G[c] + z.A[3 + k] * G[3 + c]) + z.A[6 + k] * G[6 + c]);
          pt[3 * k + c] = pt[3 * k + c] + (-G[3 * k + c]);
        }
  }
  int turn = 0;
#pragma unroll
  for(int k = 0; k < 3; k++) // row k of both blocks: three sums a meeting (every thread of the workgroup calls)
  {
    float v[3];
    if(goffset)
    {
#pragma unroll
      for(int c = 0; c < 3; c++) v[c] = po[3 * k + c];
      sum1024_meet_many<3, 0u>(v, cross, turn);
#pragma unroll
      for(int c = 0; c < 3; c++) po[3 * k + c] = v[c];
    }
    if(gtarget)
    {
#pragma unroll
      for(int c = 0; c < 3; c++) v[c] = pt[3 * k + c];
      sum1024_meet_many<3, 0u>(v, cross, turn);
#pragma unroll
      for(int c = 0; c < 3; c++) pt[3 * k + c] = v[c];
    }
  }
  if(t == 0)
#pragma unroll
    for(int k = 0; k < 3; k++)
#pragma unroll
      for(int c = 0; c < 3; c++)
        if(c < a.C)
        {
          if(goffset) ori_store(goffset + (s * 3 + k) * a.C + c, po[3 * k + c], accumulate);
          if(gtarget) ori_store(gtarget + (s * 3 + k) * a.C + c, pt[3 * k + c], accumulate);
        }
}

// grad_aa[i][m] = sum_q grad_rot[i][q] rodrigues_grad_dev(aa_i, m)[q], ascending q from +0
__global__ __launch_bounds__(ORI_T) void rodrigues_vjp_kernel(int64_t n, const float * aa, const float * grot, float * gaa, int accumulate)
{
  const int64_t i = (int64_t)blockIdx.x * ORI_T + threadIdx.x;
  if(i >= n * 3) return;
  const int64_t row = i / 3;
  const int m = (int)(i % 3);
  const float th[3] = {aa[row * 3], aa[row * 3 + 1], aa[row * 3 + 2]};
  float dRdt[9];
  rodrigues_grad_dev(th, m, dRdt);
  float sum = 0.0f;
#pragma unroll
  for(int q = 0; q < 9; q++) sum = sum + grot[row * 9 + q] * dRdt[q];
  ori_store(gaa + i, sum, accumulate);
}

static int ori_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

// what the two calls refuse alike
static int ori_check(const char * fn, int64_t n, int64_t J, int64_t row_stride, const float * frames, int64_t S, int64_t C, const int64_t * joint,
                     const float * target, int64_t Tn, int64_t Wn, float rho, int space)
{
  if(!frames || !joint || !target) return ori_refuse(fn, "frames, joint or target is NULL");
  if(n <= 0 || J <= 0 || S <= 0) return ori_refuse(fn, "n, J and S must be positive");
  if(C < 1 || C > 3) return ori_refuse(fn, "C must be 1, 2 or 3");
  if(row_stride != 3 && row_stride != 4) return ori_refuse(fn, "row_stride must be 3 or 4");
  if(Tn != 1 && Tn != n) return ori_refuse(fn, "Tn must be 1 or n");
  if(Wn != 1 && Wn != n) return ori_refuse(fn, "Wn must be 1 or n");
  if(!(rho >= 0.0f && rho < INFINITY)) return ori_refuse(fn, "rho must be finite and not negative");
  if(n > ORI_INT32_MAX || J > ORI_INT32_MAX || S > ORI_INT32_MAX || n * J > ORI_INT32_MAX / 12 || n * S > ORI_INT32_MAX / 9)
    return ori_refuse(fn, "n J 12 or n S 9 beyond int32 indexing");
  return check_space(space, fn);
}

static OriArgs ori_args(Frame & fr, int64_t n, int64_t J, int64_t rs, const float * frames, int64_t S, int64_t C, const int64_t * joint,
                        const float * offset, const float * target, int64_t Tn, const float * weight, int64_t Wn, float rho)
{
  OriArgs a = {};
  a.frames = fr.in(frames, (size_t)(n * J * 3 * rs));
  a.joint = fr.in(joint, (size_t)S);
  a.offset = fr.in(offset, (size_t)(S * 3 * C));
  a.target = fr.in(target, (size_t)(Tn * S * 3 * C));
  a.weight = fr.in(weight, (size_t)(Wn * S));
  a.n = (int)n, a.J = (int)J, a.rs = (int)rs, a.S = (int)S, a.C = (int)C;
  a.t_per_frame = Tn != 1, a.w_per_frame = weight && Wn != 1;
  a.rho = rho;
  return a;
}

static unsigned ori_blocks(int64_t items, int per)
{
  return (unsigned)((items + per - 1) / per);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_orientation_term(int device, int64_t n, int64_t J, int64_t row_stride, const float * frames, int64_t S, int64_t C,
                                       const int64_t * joint, const float * offset, const float * target, int64_t Tn, const float * weight,
                                       int64_t Wn, float rho, float * energy, float * sensor_energy, float * residual, int space, void * stream)
{
  const char * fn = "smplpp_orientation_term";
  if(int rc = ori_check(fn, n, J, row_stride, frames, S, C, joint, target, Tn, Wn, rho, space)) return rc;
  if(!energy && !sensor_energy && !residual) return ori_refuse(fn, "every output is NULL");
  Frame fr(device, nullptr, space, stream, "orientation term");
  const OriArgs a = ori_args(fr, n, J, row_stride, frames, S, C, joint, offset, target, Tn, weight, Wn, rho);
  const OriOut o{fr.out(energy, (size_t)n), fr.out(sensor_energy, (size_t)(n * S)), fr.out(residual, (size_t)(n * S * 3 * C))};
  return fr.run([&] {
    const FrameSumSplit sp = frame_sum_split(S);
    if(!o.energy)
      ori_sensors_kernel<<<dim3(ori_blocks(n * S, ORI_T)), dim3(ORI_T), 0, fr.st>>>(a, o);
    else if(sp.nq == 0)
      ori_forward_kernel<0><<<dim3(ori_blocks(n, ORI_T / 64)), dim3(ORI_T), 0, fr.st>>>(a, o);
    else if(sp.nq == 4)
      ori_forward_kernel<4><<<dim3((unsigned)n), dim3(sp.threads), 0, fr.st>>>(a, o);
    else
      ori_forward_kernel<1><<<dim3((unsigned)n), dim3(sp.threads), 0, fr.st>>>(a, o);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_orientation_term_vjp(int device, int64_t n, int64_t J, int64_t row_stride, const float * frames, int64_t S, int64_t C,
                                           const int64_t * joint, const float * offset, const float * target, int64_t Tn, const float * weight,
                                           int64_t Wn, float rho, const float * grad_energy, const float * grad_sensor_energy,
                                           const float * grad_residual, float * grad_frames, float * grad_offset, float * grad_target,
                                           int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_orientation_term_vjp";
  if(int rc = ori_check(fn, n, J, row_stride, frames, S, C, joint, target, Tn, Wn, rho, space)) return rc;
  if(!grad_energy && !grad_sensor_energy && !grad_residual) return ori_refuse(fn, "every cotangent is NULL");
  if(!grad_frames && !grad_offset && !grad_target) return ori_refuse(fn, "grad_frames, grad_offset and grad_target are all NULL");
  if(accumulate != 0 && accumulate != 1) return ori_refuse(fn, "accumulate must be 0 or 1");
  Frame fr(device, nullptr, space, stream, "orientation term VJP");
  const OriArgs a = ori_args(fr, n, J, row_stride, frames, S, C, joint, offset, target, Tn, weight, Wn, rho);
  const OriCot g{fr.in(grad_energy, (size_t)n), fr.in(grad_sensor_energy, (size_t)(n * S)), fr.in(grad_residual, (size_t)(n * S * 3 * C))};
  // (a host-space grad_frames is loaded whole in either mode: column 3 of a row_stride 4 buffer goes back as it came)
  float * gf = fr.out(grad_frames, (size_t)(n * J * 3 * row_stride), accumulate != 0 || row_stride == 4);
  float * go = fr.out(grad_offset, (size_t)(S * 3 * C), accumulate != 0);
  float * gt = fr.out(grad_target, (size_t)(Tn * S * 3 * C), accumulate != 0);
  return fr.run([&] {
    float * frame_target = Tn != 1 ? gt : nullptr;
    if(gf || frame_target)
    {
      // frames per workgroup and sensors per chunk: every joint of the tile's frames has a thread while J allows it
      const int64_t fit = J <= ORI_T ? ORI_T / J : 1;
      const int FT = (int)(fit < n ? fit : n), SC = ORI_T / FT;
      ori_gather_kernel<<<dim3(ori_blocks(n, FT)), dim3(ORI_T), 0, fr.st>>>(a, g, gf, frame_target, accumulate, FT, SC);
      HIP_TRY(hipGetLastError());
    }
    float * shared_target = Tn == 1 ? gt : nullptr;
    if(go || shared_target)
    {
      ori_across_kernel<<<dim3((unsigned)S), dim3(1024), 0, fr.st>>>(a, g, go, shared_target, accumulate);
      HIP_TRY(hipGetLastError());
    }
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_axis_angle_to_rotmat_vjp(int device, int64_t n, const float * aa, const float * grad_rot, float * grad_aa, int accumulate,
                                               int space, void * stream)
{
  const char * fn = "smplpp_axis_angle_to_rotmat_vjp";
  if(n <= 0 || !aa || !grad_rot || !grad_aa) return ori_refuse(fn, "needs n > 0, aa, grad_rot and grad_aa");
  if(accumulate != 0 && accumulate != 1) return ori_refuse(fn, "accumulate must be 0 or 1");
  if(n > ORI_INT32_MAX * (int64_t)(ORI_T / 3)) return ori_refuse(fn, "too many rows");
  if(int rc = check_space(space, fn)) return rc;
  Frame fr(device, nullptr, space, stream, "axis-angle to rotmat VJP");
  const float * a = fr.in(aa, (size_t)(n * 3));
  const float * g = fr.in(grad_rot, (size_t)(n * 9));
  float * o = fr.out(grad_aa, (size_t)(n * 3), accumulate != 0);
  return fr.run([&] {
    rodrigues_vjp_kernel<<<dim3(ori_blocks(n * 3, ORI_T)), dim3(ORI_T), 0, fr.st>>>(n, a, g, o, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
