// The scene term: a static signed-distance volume sampled at the body's points by trilinear interpolation, the
// penetration and contact energies on the sample, and their vector-Jacobian product to the points.  A volume handle keeps the grid on the
// device in one of two storage layouts (volume_plan.h); smplpp_volume_set refreshes it with one kernel.  The rules are in
// include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA), the frame energy is one fixed-order
// sum (sum1024 of fixed_sum.h, whose two facts about +0 let the work split follow K), and there are no floating-point atomics.  No
// output bit depends on the layout: both hand the same eight floats to vol_sample.
//
//  vol_set_kernel<L>          a thread per stored unit: a node (linear: a copy) or a cell record (cells: eight reads, two 16-byte writes).
//  scene_sample_kernel<L>     a thread per point: value, gradient, valid.
//  scene_points_kernel<L>     the term without the frame energy: a thread per point.
//  scene_small_kernel<L>      K <= 64: a wavefront per frame, lane k owns point k (partial k; the partials past 63 are +0).
//  scene_wide_kernel<L, NQ>   K > 64: a workgroup per frame, of 256 or 1024 threads by frame_sum_split: thread t owns the partials t + T q.
//  scene_vjp_kernel<L>        a thread per point: it samples again by the forward's device function, so the bits match; no sums.
// A point's three coordinates are three dword reads per lane (rows of 3 floats are not 16-byte aligned; a wavefront's three reads cover
// the same 768 contiguous bytes).  The gather of the grid is the cost: 64 lanes in up to 64 different rows of it.
#include <cstdlib>

#include "fixed_sum.h"
#include "staging.h"
#include "volume_plan.h"

#pragma clang fp contract(off)

struct smplpp_volume
{
  int device = 0;
  int64_t G[3] = {0, 0, 0};
  float origin[3] = {0, 0, 0}, spacing[3] = {1, 1, 1};
  float xf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; // row-major [R|t]
  bool has_xf = false;
  int layout = smplpp_hip::VOL_LINEAR;
  smplpp_hip::DevBuf data;  // volume_floats(layout, G) floats
  smplpp_hip::Arena arena;  // staging of the host-space calls on this volume
};

namespace smplpp_hip
{
using Volume = struct ::smplpp_volume;
constexpr int SCN_T = 256; // threads of every kernel here (the wide forward above K = 1024 takes 1024)
constexpr int SCN_WAVES = SCN_T / 64;
constexpr int64_t SCN_INT32_MAX = 0x7fffffffLL;

// the device image of a volume
struct VolView
{
  const float * data;
  int Gx, Gy, Gz;
  float o[3], h[3], R[9], t[3];
  int has_xf;
};

// two adjacent floats at any 4-byte-aligned address, read as one 8-byte access
struct __attribute__((packed, aligned(4))) VolPair
{
  float x, y;
};

// the eight nodes of cell (i, j, k) in corner order dx + 2 dy + 4 dz
template<int L>
__device__ inline void vol_cell(const VolView & v, int i, int j, int k, float (&c)[8])
{
  if constexpr(L == VOL_CELLS)
  {
    const float4 * r = reinterpret_cast<const float4 *>(v.data + volume_cells_index(v.Gx, v.Gy, i, j, k, 0));
    const float4 a = r[0], b = r[1];
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
  }
  else
  {
#pragma unroll
    for(int d = 0; d < 4; d++)
    {
      const VolPair p = *reinterpret_cast<const VolPair *>(v.data + volume_linear_index(v.Gx, v.Gy, i, j + (d & 1), k + (d >> 1)));
      c[2 * d] = p.x, c[2 * d + 1] = p.y;
    }
  }
}

struct VolSample
{
  float s, gx, gy, gz; // the value and its gradient to the WORLD point; all +0 when not valid
  bool valid;
};

// The sampling rule of include/smplpp_hip.h at the world point (px, py, pz).  GRAD = false leaves the gradient out (+0).
template<int L, bool GRAD>
__device__ inline VolSample vol_sample(const VolView & v, float px, float py, float pz)
{
  VolSample r{0.0f, 0.0f, 0.0f, 0.0f, false};
  float q[3] = {px, py, pz};
  if(v.has_xf)
#pragma unroll
    for(int a = 0; a < 3; a++) q[a] = ((v.R[3 * a] * px + v.R[3 * a + 1] * py) + v.R[3 * a + 2] * pz) + v.t[a];
  const float gx = (q[0] - v.o[0]) / v.h[0], gy = (q[1] - v.o[1]) / v.h[1], gz = (q[2] - v.o[2]) / v.h[2];
  // (a NaN fails every comparison, an infinity the upper one)
  const bool inside = gx >= 0.0f && gx <= (float)(v.Gx - 1) && gy >= 0.0f && gy <= (float)(v.Gy - 1) && gz >= 0.0f && gz <= (float)(v.Gz - 1);
  if(!inside) return r;
  const int i = min((int)floorf(gx), v.Gx - 2), j = min((int)floorf(gy), v.Gy - 2), k = min((int)floorf(gz), v.Gz - 2);
  const float fx = gx - (float)i, fy = gy - (float)j, fz = gz - (float)k;
  float c[8];
  vol_cell<L>(v, i, j, k, c);
  // x differences d[y][z] and x lerps c[y][z]
  const float d00 = c[1] - c[0], d10 = c[3] - c[2], d01 = c[5] - c[4], d11 = c[7] - c[6];
  const float c00 = c[0] + fx * d00, c10 = c[2] + fx * d10, c01 = c[4] + fx * d01, c11 = c[6] + fx * d11;
  const float e0 = c10 - c00, e1 = c11 - c01; // y differences at z = 0, 1
  const float c0 = c00 + fy * e0, c1 = c01 + fy * e1;
  const float ez = c1 - c0;
  const float s = c0 + fz * ez;
  if(!(fabsf(s) < INFINITY)) return r;
  r.s = s, r.valid = true;
  if constexpr(GRAD)
  {
    const float x0 = d00 + fy * (d10 - d00), x1 = d01 + fy * (d11 - d01);
    const float vx = (x0 + fz * (x1 - x0)) / v.h[0];
    const float vy = (e0 + fz * (e1 - e0)) / v.h[1];
    const float vz = ez / v.h[2];
    if(v.has_xf)
    {
      r.gx = (v.R[0] * vx + v.R[3] * vy) + v.R[6] * vz;
      r.gy = (v.R[1] * vx + v.R[4] * vy) + v.R[7] * vz;
      r.gz = (v.R[2] * vx + v.R[5] * vy) + v.R[8] * vz;
    }
    else
      r.gx = vx, r.gy = vy, r.gz = vz;
  }
  return r;
}

// the term's arguments
struct TermArgs
{
  const float * points;
  int K;
  const float *w_pen, *w_con;
  float rho;
  float *point_energy, *value;
  uint8_t * valid;
};

// e of a valid sample s under the weights (wp, wc)
__device__ inline float scene_energy(float s, float wp, float wc, float rho)
{
  const float q = s * s;
  const float e_pen = s < 0.0f ? wp * q : 0.0f;
  float e_con;
  if(rho == 0.0f) e_con = wc * q;
  else
  {
    const float p2 = rho * rho;
    e_con = wc * ((p2 * q) / (p2 + q));
  }
  return e_pen + e_con;
}

// point i = f K + k of the term: writes its per-point outputs, returns its energy
template<int L>
__device__ inline float scene_point(const VolView & v, const TermArgs & a, int i, int k)
{
  const float wp = a.w_pen ? a.w_pen[k] : 1.0f, wc = a.w_con ? a.w_con[k] : 0.0f;
  const bool live = wp != 0.0f || wc != 0.0f;
  float e = 0.0f;
  if(live || a.value || a.valid)
  {
    const float * p = a.points + 3 * i;
    const VolSample r = vol_sample<L, false>(v, p[0], p[1], p[2]);
    if(a.value) a.value[i] = r.s;
    if(a.valid) a.valid[i] = r.valid ? 1 : 0;
    if(live && r.valid) e = scene_energy(r.s, wp, wc, a.rho);
  }
  if(a.point_energy) a.point_energy[i] = e;
  return e;
}

// grid: ceil(units / SCN_T).  dst and src never overlap: src is the caller's array (or its staged copy)
template<int L>
__global__ __launch_bounds__(SCN_T) void vol_set_kernel(float * __restrict__ dst, const float * __restrict__ src, int Gx, int Gy, int Gz)
{
  const int64_t u = (int64_t)blockIdx.x * SCN_T + threadIdx.x;
  if constexpr(L == VOL_LINEAR)
  {
    if(u < volume_linear_floats(Gx, Gy, Gz)) dst[u] = src[u];
  }
  else
  {
    const int cx = Gx - 1, cy = Gy - 1;
    if(u >= (int64_t)cx * cy * (Gz - 1)) return;
    const int i = (int)(u % cx), j = (int)((u / cx) % cy), k = (int)(u / ((int64_t)cx * cy));
    float c[8];
#pragma unroll
    for(int d = 0; d < 8; d++) c[d] = src[volume_linear_index(Gx, Gy, i + (d & 1), j + ((d >> 1) & 1), k + (d >> 2))];
    float4 * r = reinterpret_cast<float4 *>(dst + volume_cells_index(Gx, Gy, i, j, k, 0));
    r[0] = make_float4(c[0], c[1], c[2], c[3]);
    r[1] = make_float4(c[4], c[5], c[6], c[7]);
  }
}

// grid: ceil(n K / SCN_T)
template<int L>
__global__ __launch_bounds__(SCN_T) void scene_sample_kernel(VolView v, int total, const float * __restrict__ points, float * __restrict__ value,
                                                             float * __restrict__ gradient, uint8_t * __restrict__ valid)
{
  const int i = blockIdx.x * SCN_T + threadIdx.x;
  if(i >= total) return;
  const float * p = points + 3 * i;
  const VolSample r = gradient ? vol_sample<L, true>(v, p[0], p[1], p[2]) : vol_sample<L, false>(v, p[0], p[1], p[2]);
  if(value) value[i] = r.s;
  if(valid) valid[i] = r.valid ? 1 : 0;
  if(gradient) gradient[3 * i] = r.gx, gradient[3 * i + 1] = r.gy, gradient[3 * i + 2] = r.gz;
}

// grid: ceil(n K / SCN_T)
template<int L>
__global__ __launch_bounds__(SCN_T) void scene_points_kernel(VolView v, TermArgs a, int total)
{
  const int i = blockIdx.x * SCN_T + threadIdx.x;
  if(i < total) scene_point<L>(v, a, i, i % a.K);
}

// K <= 64.  grid: ceil(n / SCN_WAVES): wavefront f, lane k
template<int L>
__global__ __launch_bounds__(SCN_T) void scene_small_kernel(VolView v, TermArgs a, int n, float * __restrict__ energy)
{
  const int f = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SCN_WAVES + (threadIdx.x >> 6))), k = threadIdx.x & 63;
  if(f >= n) return;
  float e = 0.0f;
  if(k < a.K) e = scene_point<L>(v, a, f * a.K + k, k);
  const float s = sum64_meet(0.0f + e); // fixed_sum.h: partial k, the partials past 63 left out
  if(k == 0) energy[f] = s;
}

// K > 64.  grid: n; a workgroup of 1024 / NQ threads, thread t owns the partials t + (1024 / NQ) q, q < NQ
template<int L, int NQ>
__global__ __launch_bounds__(1024 / NQ) void scene_wide_kernel(VolView v, TermArgs a, float * __restrict__ energy)
{
  constexpr int T = 1024 / NQ;
  __shared__ float cross[T / 64];
  const int f = blockIdx.x, t = threadIdx.x;
  float s[NQ];
#pragma unroll
  for(int q = 0; q < NQ; q++) s[q] = 0.0f;
  for(int k0 = 0; k0 < a.K; k0 += 1024)
#pragma unroll
    for(int q = 0; q < NQ; q++)
    {
      const int k = k0 + T * q + t;
      if(k < a.K) s[q] = s[q] + scene_point<L>(v, a, f * a.K + k, k);
    }
  const float sum = sum1024_meet<NQ>(s, cross);
  if(t == 0) energy[f] = sum;
}

// grid: ceil(n K / SCN_T): thread (f, k).  ge, gpe, gv: the cotangents of energy, point_energy and value, each may be null
template<int L>
__global__ __launch_bounds__(SCN_T) void scene_vjp_kernel(VolView v, TermArgs a, int total, const float * __restrict__ ge, const float * __restrict__ gpe,
                                                          const float * __restrict__ gv, float * gp, int accumulate)
{
  const int i = blockIdx.x * SCN_T + threadIdx.x;
  if(i >= total) return;
  const int f = i / a.K, k = i % a.K;
  const float wp = a.w_pen ? a.w_pen[k] : 1.0f, wc = a.w_con ? a.w_con[k] : 0.0f;
  const bool live = wp != 0.0f || wc != 0.0f;
  float el[3] = {0.0f, 0.0f, 0.0f};
  if(live || gv)
  {
    const float * p = a.points + 3 * i;
    const VolSample r = vol_sample<L, true>(v, p[0], p[1], p[2]);
    if(r.valid)
    {
      float term = 0.0f;
      if(live)
      {
        const float g = (ge ? ge[f] : 0.0f) + (gpe ? gpe[i] : 0.0f);
        const float s = r.s, pen = s < 0.0f ? (2.0f * wp) * s : 0.0f;
        float con;
        if(a.rho == 0.0f) con = (2.0f * wc) * s;
        else
        {
          const float p2 = a.rho * a.rho, d = p2 / (p2 + s * s);
          con = ((2.0f * wc) * (d * d)) * s;
        }
        term = g * (pen + con);
      }
      const float kk = (gv ? gv[i] : 0.0f) + term;
      el[0] = kk * r.gx, el[1] = kk * r.gy, el[2] = kk * r.gz;
    }
  }
  float * o = gp + 3 * i;
#pragma unroll
  for(int c = 0; c < 3; c++) o[c] = accumulate ? o[c] + el[c] : el[c];
}

static VolView vol_view(const Volume * q)
{
  VolView v;
  v.data = q->data.as<float>();
  v.Gx = (int)q->G[0], v.Gy = (int)q->G[1], v.Gz = (int)q->G[2];
  for(int a = 0; a < 3; a++) v.o[a] = q->origin[a], v.h[a] = q->spacing[a], v.t[a] = q->xf[4 * a + 3];
  for(int a = 0; a < 9; a++) v.R[a] = q->xf[4 * (a / 3) + a % 3];
  v.has_xf = q->has_xf ? 1 : 0;
  return v;
}

static unsigned scn_blocks(int64_t items, int per)
{
  return (unsigned)((items + per - 1) / per);
}

static int scn_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

// what the three calls on points refuse alike
static int scn_points_check(const char * fn, const Volume * q, int64_t n, int64_t K, const float * points, int space)
{
  if(!q) return scn_refuse(fn, "no volume");
  if(!points) return scn_refuse(fn, "points is NULL");
  if(n <= 0 || K <= 0) return scn_refuse(fn, "n and K must be positive");
  if(n > SCN_INT32_MAX || K > SCN_INT32_MAX || n * K > SCN_INT32_MAX / 3) return scn_refuse(fn, "n K 3 beyond int32 indexing");
  return check_space(space, fn);
}

// the device copy of `values` (device pointer d) into the layout of q, on st
static int vol_fill(Volume * q, const float * d, hipStream_t st)
{
  const int Gx = (int)q->G[0], Gy = (int)q->G[1], Gz = (int)q->G[2];
  if(q->layout == VOL_CELLS)
    vol_set_kernel<VOL_CELLS><<<dim3(scn_blocks(volume_cells_floats(Gx, Gy, Gz) / 8, SCN_T)), dim3(SCN_T), 0, st>>>(q->data.as<float>(), d, Gx, Gy, Gz);
  else
    vol_set_kernel<VOL_LINEAR><<<dim3(scn_blocks(volume_linear_floats(Gx, Gy, Gz), SCN_T)), dim3(SCN_T), 0, st>>>(q->data.as<float>(), d, Gx, Gy, Gz);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// one launch per layout: KERNEL<VOL_LINEAR ...> or KERNEL<VOL_CELLS ...>
#define SCN_LAUNCH(q, KERNEL, grid, block, st, ...)                                              \
  do                                                                                             \
  {                                                                                              \
    if((q)->layout == VOL_CELLS) KERNEL(VOL_CELLS)<<<grid, block, 0, st>>>(__VA_ARGS__);         \
    else                                                                                         \
      KERNEL(VOL_LINEAR)<<<grid, block, 0, st>>>(__VA_ARGS__);                                   \
    HIP_TRY(hipGetLastError());                                                                  \
  } while(0)
#define SCN_SAMPLE(L) scene_sample_kernel<L>
#define SCN_POINTS(L) scene_points_kernel<L>
#define SCN_SMALL(L) scene_small_kernel<L>
#define SCN_WIDE4(L) scene_wide_kernel<L, 4>
#define SCN_WIDE1(L) scene_wide_kernel<L, 1>
#define SCN_VJP(L) scene_vjp_kernel<L>

extern "C" int smplpp_volume_set(struct smplpp_volume * q, const float * values, int space, void * stream)
{
  const char * fn = "smplpp_volume_set";
  if(!q) return scn_refuse(fn, "no volume");
  if(!values) return scn_refuse(fn, "values is NULL");
  if(int rc = check_space(space, fn)) return rc;
  Frame fr(q->device, &q->arena, space, stream, "volume set");
  const float * d = fr.in(values, (size_t)volume_linear_floats(q->G[0], q->G[1], q->G[2]));
  return fr.run([&] { return vol_fill(q, d, fr.st); });
}

// Validate (volume_plan.h), choose the layout, allocate, fill.
extern "C" int smplpp_volume_create(int device, int64_t Gx, int64_t Gy, int64_t Gz, const float * origin, const float * spacing,
                                    const float * world_to_volume, const float * values, int space, struct smplpp_volume ** out)
{
  const char * fn = "smplpp_volume_create";
  if(out) *out = nullptr;
  if(const char * why = volume_refusal(Gx, Gy, Gz, origin, spacing, world_to_volume, space, out != nullptr)) return scn_refuse(fn, why);
  const int layout = volume_layout(Gx, Gy, Gz, getenv("SMPLPP_VOLUME_LAYOUT"));
  if(layout < 0) return scn_refuse(fn, "SMPLPP_VOLUME_LAYOUT must be linear or cells");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<Volume> q(new Volume());
  q->device = device, q->layout = layout;
  q->G[0] = Gx, q->G[1] = Gy, q->G[2] = Gz;
  for(int a = 0; a < 3; a++) q->origin[a] = origin[a], q->spacing[a] = spacing[a];
  if(world_to_volume)
  {
    q->has_xf = true;
    for(int a = 0; a < 12; a++) q->xf[a] = world_to_volume[a];
  }
  const size_t bytes = sizeof(float) * (size_t)volume_floats(layout, Gx, Gy, Gz);
  HIP_TRY(q->data.reserve(bytes));
  if(values)
  {
    if(int rc = smplpp_volume_set(q.get(), values, space, nullptr)) return rc;
  }
  else
    HIP_TRY(hipMemset(q->data.p.get(), 0, bytes));
  HIP_TRY(hipDeviceSynchronize());
  *out = q.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_volume_destroy(struct smplpp_volume * q)
{
  if(!q) return SMPLPP_OK;
  (void)hipSetDevice(q->device);
  delete q;
  return SMPLPP_OK;
}

extern "C" int smplpp_volume_info(const struct smplpp_volume * q, int64_t * G, float * origin, float * spacing, float * world_to_volume, int * layout)
{
  if(!q) return scn_refuse("smplpp_volume_info", "no volume");
  for(int a = 0; a < 3; a++)
  {
    if(G) G[a] = q->G[a];
    if(origin) origin[a] = q->origin[a];
    if(spacing) spacing[a] = q->spacing[a];
  }
  if(world_to_volume)
    for(int a = 0; a < 12; a++) world_to_volume[a] = q->xf[a];
  if(layout) *layout = q->layout;
  return SMPLPP_OK;
}

extern "C" int smplpp_volume_sample(struct smplpp_volume * q, int64_t n, int64_t K, const float * points, float * value, float * gradient,
                                    uint8_t * valid, int space, void * stream)
{
  const char * fn = "smplpp_volume_sample";
  if(int rc = scn_points_check(fn, q, n, K, points, space)) return rc;
  if(!value && !gradient && !valid) return scn_refuse(fn, "every output is NULL");
  const int64_t total = n * K;
  Frame fr(q->device, &q->arena, space, stream, "volume sample");
  const float * p = fr.in(points, (size_t)(total * 3));
  float * o_v = fr.out(value, (size_t)total);
  float * o_g = fr.out(gradient, (size_t)(total * 3));
  uint8_t * o_ok = fr.out(valid, (size_t)total);
  return fr.run([&] {
    SCN_LAUNCH(q, SCN_SAMPLE, dim3(scn_blocks(total, SCN_T)), dim3(SCN_T), fr.st, vol_view(q), (int)total, p, o_v, o_g, o_ok);
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_scene_term(struct smplpp_volume * q, int64_t n, int64_t K, const float * points, const float * w_pen, const float * w_con,
                                 float rho, float * energy, float * point_energy, float * value, uint8_t * valid, int space, void * stream)
{
  const char * fn = "smplpp_scene_term";
  if(int rc = scn_points_check(fn, q, n, K, points, space)) return rc;
  if(!(rho >= 0.0f && rho < INFINITY)) return scn_refuse(fn, "rho must be finite and not negative");
  if(!energy && !point_energy && !value && !valid) return scn_refuse(fn, "every output is NULL");
  const int64_t total = n * K;
  Frame fr(q->device, &q->arena, space, stream, "scene term");
  TermArgs a{fr.in(points, (size_t)(total * 3)), (int)K, fr.in(w_pen, (size_t)K), fr.in(w_con, (size_t)K), rho, nullptr, nullptr, nullptr};
  float * e = fr.out(energy, (size_t)n);
  a.point_energy = fr.out(point_energy, (size_t)total);
  a.value = fr.out(value, (size_t)total);
  a.valid = fr.out(valid, (size_t)total);
  return fr.run([&] {
    const FrameSumSplit sp = frame_sum_split(K); // fixed_sum.h
    if(!e) SCN_LAUNCH(q, SCN_POINTS, dim3(scn_blocks(total, SCN_T)), dim3(SCN_T), fr.st, vol_view(q), a, (int)total);
    else if(sp.nq == 0)
      SCN_LAUNCH(q, SCN_SMALL, dim3(scn_blocks(n, SCN_WAVES)), dim3(SCN_T), fr.st, vol_view(q), a, (int)n, e);
    else if(sp.nq == 4)
      SCN_LAUNCH(q, SCN_WIDE4, dim3((unsigned)n), dim3(sp.threads), fr.st, vol_view(q), a, e);
    else
      SCN_LAUNCH(q, SCN_WIDE1, dim3((unsigned)n), dim3(sp.threads), fr.st, vol_view(q), a, e);
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_scene_term_vjp(struct smplpp_volume * q, int64_t n, int64_t K, const float * points, const float * w_pen,
                                     const float * w_con, float rho, const float * grad_energy, const float * grad_point_energy,
                                     const float * grad_value, float * grad_points, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_scene_term_vjp";
  if(int rc = scn_points_check(fn, q, n, K, points, space)) return rc;
  if(!(rho >= 0.0f && rho < INFINITY)) return scn_refuse(fn, "rho must be finite and not negative");
  if(!grad_energy && !grad_point_energy && !grad_value) return scn_refuse(fn, "every cotangent is NULL");
  if(!grad_points) return scn_refuse(fn, "grad_points is NULL");
  if(accumulate != 0 && accumulate != 1) return scn_refuse(fn, "accumulate must be 0 or 1");
  const int64_t total = n * K;
  Frame fr(q->device, &q->arena, space, stream, "scene term VJP");
  const TermArgs a{fr.in(points, (size_t)(total * 3)), (int)K, fr.in(w_pen, (size_t)K), fr.in(w_con, (size_t)K), rho, nullptr, nullptr, nullptr};
  const float * ge = fr.in(grad_energy, (size_t)n);
  const float * gpe = fr.in(grad_point_energy, (size_t)total);
  const float * gv = fr.in(grad_value, (size_t)total);
  float * gp = fr.out(grad_points, (size_t)(total * 3), accumulate != 0);
  return fr.run([&] {
    SCN_LAUNCH(q, SCN_VJP, dim3(scn_blocks(total, SCN_T)), dim3(SCN_T), fr.st, vol_view(q), a, (int)total, ge, gpe, gv, gp, accumulate);
    return (int)SMPLPP_OK;
  });
}
