// Keypoints: a sparse landmark regressor over [verts; joints] with its vector-Jacobian product, and the projection of
// any points through the rasteriser's camera with a 2-D keypoint energy and its vector-Jacobian product to the points and to the
// camera.  The rules are in include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA), every
// output element is one fixed-order sum, and there are no floating-point atomics.
//
//  lm_forward_kernel   LM_SPLIT = 8 consecutive lanes per (frame, landmark): lane p takes the row's entries of rank p, p + 8, ...; the
//                      eight partial sums meet in the xor tree of raster_walk.h, ((s0+s4)+(s2+s6)) + ((s1+s5)+(s3+s7)).
//  lm_vjp_kernel       per (frame, source, component): the source's entries in ascending e from the transposed lists built at creation
//                      (landmark_tables.h); consecutive lanes store consecutive floats.
//  pp_forward_kernel   per (frame, point): dr_project, then the energy.
//  pp_vjp_points_kernel per (frame, point), when no gradient to the camera is asked for.
//  pp_vjp_frame_kernel one wavefront per frame: lane p takes the points p, p + 64, ... in ascending order, stores their gradients and
//                      keeps the 16 partial sums of the camera row, which meet by sum64 (fixed_sum.h).
#include "depth_raster_device.h"
#include "fixed_sum.h"
#include "landmark_tables.h"

#pragma clang fp contract(off)

struct smplpp_landmarks
{
  int device = 0;
  int64_t V = 0, L = 0, nnz = 0;
  smplpp_hip::DevBuf rowPtr, col, val; // the CSR: [L+1] int32, [nnz] int32, [nnz] float
  smplpp_hip::DevBuf srcPtr, srcRow, srcVal; // its transpose: [V+24+1] int32, [nnz] int32 landmark, [nnz] float
  smplpp_hip::Arena arena;             // staging of the host-space calls on this regressor
};

namespace smplpp_hip
{
using Landmarks = struct ::smplpp_landmarks; // (the bare name is the regression call)
constexpr int LM_T = 256;   // threads of the landmark kernels and of the per-point projection kernels
constexpr int LM_SPLIT = 8; // lanes per (frame, landmark)
constexpr int PP_W = 64;    // one wavefront per frame in pp_vjp_frame_kernel

// grid: ceil(total LM_SPLIT / LM_T), total = n L
__global__ __launch_bounds__(LM_T) void lm_forward_kernel(const int32_t * __restrict__ rowPtr, const int32_t * __restrict__ col,
                                                          const float * __restrict__ val, const float * __restrict__ verts,
                                                          const float * __restrict__ joints, float * __restrict__ points, int L, int V,
                                                          int64_t total)
{
  const int64_t tid = (int64_t)blockIdx.x * LM_T + threadIdx.x;
  const int64_t idx = tid / LM_SPLIT;
  const int part = (int)(tid % LM_SPLIT);
  const bool in = idx < total;
  float s[3] = {0.0f, 0.0f, 0.0f};
  if(in)
  {
    const int64_t frame = idx / L;
    const int l = (int)(idx % L);
    const float * xv = verts + frame * V * 3;
    const float * xj = joints + frame * NJ * 3;
    const int64_t end = rowPtr[l + 1];
    for(int64_t e = (int64_t)rowPtr[l] + part; e < end; e += LM_SPLIT)
    {
      const int c = col[e];
      const float w = val[e];
      const float * x = c < V ? xv + (int64_t)c * 3 : xj + (int64_t)(c - V) * 3;
      for(int k = 0; k < 3; k++) s[k] = s[k] + w * x[k];
    }
  }
  for(int m = LM_SPLIT / 2; m >= 1; m >>= 1) // (every thread of the grid: lanes past the end carry zeros)
#pragma unroll
    for(int k = 0; k < 3; k++) s[k] = s[k] + __shfl_xor(s[k], m);
  if(in && part == 0)
    for(int k = 0; k < 3; k++) points[idx * 3 + k] = s[k];
}

// sources [lo, lo + cnt3 / 3) of every frame; grid: ceil(n cnt3 / LM_T).  gv or gj may be null when its sources are not in the range
__global__ __launch_bounds__(LM_T) void lm_vjp_kernel(const int32_t * __restrict__ srcPtr, const int32_t * __restrict__ srcRow,
                                                      const float * __restrict__ srcVal, const float * __restrict__ g, float * gv, float * gj,
                                                      int L, int V, int lo, int64_t cnt3, int64_t total, int accumulate)
{
  const int64_t gid = (int64_t)blockIdx.x * LM_T + threadIdx.x;
  if(gid >= total) return;
  const int64_t frame = gid / cnt3, r = gid % cnt3;
  const int src = lo + (int)(r / 3), k = (int)(r % 3);
  const float * gf = g + frame * L * 3 + k;
  float acc = 0.0f;
  const int64_t end = srcPtr[src + 1];
  for(int64_t q = srcPtr[src]; q < end; q++) acc = acc + srcVal[q] * gf[(int64_t)srcRow[q] * 3];
  float * o = src < V ? gv + (frame * V + src) * 3 + k : gj + (frame * NJ + (src - V)) * 3 + k;
  *o = accumulate ? *o + acc : acc;
}

// the energy of a projected point against its target row (tu, tv, c), with the residual r and w = d energy / d q the backward needs;
// false (and energy 0) when the confidence is 0: nothing else of the row is read
__device__ inline bool pp_energy(const float * __restrict__ t, float u, float v, float rho, float & e, float & rx, float & ry, float & w)
{
  const float c = t[2];
  e = 0.0f;
  if(c == 0.0f) return false;
  rx = u - t[0], ry = v - t[1];
  const float q = rx * rx + ry * ry, cc = c * c;
  if(rho == 0.0f)
  {
    w = cc;
    e = cc * q;
    return true;
  }
  const float r2 = rho * rho, den = r2 + q, d = r2 / den;
  w = cc * (d * d);
  e = cc * ((r2 * q) / den);
  return true;
}

__global__ __launch_bounds__(LM_T) void pp_forward_kernel(const float * __restrict__ points, const float * __restrict__ camera, float near,
                                                          const float * __restrict__ target, float rho, float * __restrict__ uv,
                                                          float * __restrict__ energy, uint8_t * __restrict__ valid, int K, int64_t total)
{
  const int64_t idx = (int64_t)blockIdx.x * LM_T + threadIdx.x;
  if(idx >= total) return;
  const DrCamera c = dr_camera(camera, idx / K);
  const float * p = points + idx * 3;
  float xc[3], u, v, su, sv;
  const bool ok = dr_project(c, p[0], p[1], p[2], near, xc, u, v, su, sv);
  if(uv) uv[idx * 2] = ok ? u : 0.0f, uv[idx * 2 + 1] = ok ? v : 0.0f;
  if(valid) valid[idx] = ok ? 1 : 0;
  if(energy)
  {
    float e = 0.0f, rx, ry, w;
    if(ok) pp_energy(target + idx * 3, u, v, rho, e, rx, ry, w);
    energy[idx] = e;
  }
}

// one point of the backward: false for a refused point; else the cotangent k on (u, v), the camera-space cotangent j, the world
// point x, xc, and the world-space gradient gp
struct PpPull
{
  float x[3], xc[3], kx, ky, j[3], gp[3];
};
__device__ inline bool pp_pull(const DrCamera & c, const float * __restrict__ points, float near, const float * __restrict__ target, float rho,
                               const float * __restrict__ grad_uv, const float * __restrict__ grad_energy, int64_t idx, PpPull & o)
{
  for(int a = 0; a < 3; a++) o.x[a] = points[idx * 3 + a];
  float u, v, su, sv;
  if(!dr_project(c, o.x[0], o.x[1], o.x[2], near, o.xc, u, v, su, sv)) return false;
  o.kx = grad_uv ? grad_uv[idx * 2] : 0.0f;
  o.ky = grad_uv ? grad_uv[idx * 2 + 1] : 0.0f;
  const float g = grad_energy ? grad_energy[idx] : 0.0f;
  if(g != 0.0f)
  {
    float e, rx, ry, w;
    if(pp_energy(target + idx * 3, u, v, rho, e, rx, ry, w))
    {
      const float gw = (2.0f * g) * w;
      o.kx = o.kx + gw * rx;
      o.ky = o.ky + gw * ry;
    }
  }
  const float z = o.xc[2];
  o.j[0] = (c.fx * o.kx) / z;
  o.j[1] = (c.fy * o.ky) / z;
  o.j[2] = -((o.j[0] * o.xc[0] + o.j[1] * o.xc[1]) / z);
  for(int a = 0; a < 3; a++) o.gp[a] = (c.R[a] * o.j[0] + c.R[3 + a] * o.j[1]) + c.R[6 + a] * o.j[2];
  return true;
}

__global__ __launch_bounds__(LM_T) void pp_vjp_points_kernel(const float * __restrict__ points, const float * __restrict__ camera, float near,
                                                             const float * __restrict__ target, float rho, const float * __restrict__ grad_uv,
                                                             const float * __restrict__ grad_energy, float * __restrict__ grad_points, int K,
                                                             int64_t total, int accumulate)
{
  const int64_t idx = (int64_t)blockIdx.x * LM_T + threadIdx.x;
  if(idx >= total) return;
  const DrCamera c = dr_camera(camera, idx / K);
  PpPull o;
  const bool live = pp_pull(c, points, near, target, rho, grad_uv, grad_energy, idx, o);
  for(int a = 0; a < 3; a++)
  {
    const float w = live ? o.gp[a] : 0.0f;
    grad_points[idx * 3 + a] = accumulate ? grad_points[idx * 3 + a] + w : w;
  }
}

// grid: n blocks of one wavefront; grad_points may be null
__global__ __launch_bounds__(PP_W) void pp_vjp_frame_kernel(const float * __restrict__ points, const float * __restrict__ camera, float near,
                                                            const float * __restrict__ target, float rho, const float * __restrict__ grad_uv,
                                                            const float * __restrict__ grad_energy, float * __restrict__ grad_points,
                                                            float * __restrict__ grad_camera, int K, int accumulate)
{
  const int64_t frame = blockIdx.x;
  const int lane = threadIdx.x;
  const DrCamera c = dr_camera(camera, frame);
  float s[16];
#pragma unroll
  for(int e = 0; e < 16; e++) s[e] = 0.0f;
  for(int k = lane; k < K; k += PP_W)
  {
    const int64_t idx = frame * K + k;
    PpPull o;
    const bool live = pp_pull(c, points, near, target, rho, grad_uv, grad_energy, idx, o);
    if(grad_points)
      for(int a = 0; a < 3; a++)
      {
        const float w = live ? o.gp[a] : 0.0f;
        grad_points[idx * 3 + a] = accumulate ? grad_points[idx * 3 + a] + w : w;
      }
    if(!live) continue;
#pragma unroll
    for(int a = 0; a < 3; a++)
    {
#pragma unroll
      for(int b = 0; b < 3; b++) s[3 * a + b] = s[3 * a + b] + o.j[a] * o.x[b];
      s[9 + a] = s[9 + a] + o.j[a];
    }
    s[12] = s[12] + o.kx * (o.xc[0] / o.xc[2]);
    s[13] = s[13] + o.ky * (o.xc[1] / o.xc[2]);
    s[14] = s[14] + o.kx;
    s[15] = s[15] + o.ky;
  }
  sum64_meet(s); // fixed_sum.h
  float mine = 0.0f; // lane e < 16 stores entry e
#pragma unroll
  for(int e = 0; e < 16; e++)
    if(lane == e) mine = s[e];
  if(lane < 16)
  {
    float * o = grad_camera + frame * 16 + lane;
    *o = accumulate ? *o + mine : mine;
  }
}

static hipError_t lm_upload(DevBuf & b, const void * src, size_t bytes)
{
  hipError_t e = b.reserve(bytes ? bytes : 4);
  if(e == hipSuccess && bytes) e = hipMemcpy(b.p.get(), src, bytes, hipMemcpyHostToDevice);
  return e;
}

static int lm_check(const char * fn, Landmarks * lm, int64_t n, int space)
{
  if(!lm) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no regressor");
  if(n <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n must be positive");
  if(n > LM_INT32_MAX || n * (lm->V + NJ) > LM_INT32_MAX || n * lm->L * 3 > LM_INT32_MAX)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * (V + 24) or n * L * 3 beyond int32 indexing");
  return check_space(space, fn);
}

static int pp_check(const char * fn, int64_t n, int64_t K, float near, float rho, int space)
{
  if(n <= 0 || K <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n and K must be positive");
  if(n > LM_INT32_MAX || K > LM_INT32_MAX || n * K * 3 > LM_INT32_MAX)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * K * 3 beyond int32 indexing");
  if(int rc = dr_check_near(fn, near)) return rc;
  if(!(std::isfinite(rho) && rho >= 0.0f)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": rho must be finite and >= 0");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// Validate and build the host tables (landmark_tables.h), then upload them.
extern "C" int smplpp_landmarks_create(smplpp_model * m, int64_t L, const int64_t * row_ptr, const int64_t * col, const float * val,
                                       struct smplpp_landmarks ** out)
{
  const char * fn = "smplpp_landmarks_create";
  if(!m || !out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no model or no out");
  *out = nullptr;
  const LandmarkTables t = landmark_tables(L, m->V + NJ, row_ptr, col, val);
  if(t.refusal) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + t.refusal);
  HIP_TRY(hipSetDevice(m->device));
  std::unique_ptr<Landmarks> lm(new Landmarks());
  lm->device = m->device, lm->V = m->V, lm->L = t.L, lm->nnz = t.nnz;
  HIP_TRY(lm_upload(lm->rowPtr, t.rowPtr.data(), sizeof(int32_t) * t.rowPtr.size()));
  HIP_TRY(lm_upload(lm->col, t.col.data(), sizeof(int32_t) * t.col.size()));
  HIP_TRY(lm_upload(lm->val, t.val.data(), sizeof(float) * t.val.size()));
  HIP_TRY(lm_upload(lm->srcPtr, t.srcPtr.data(), sizeof(int32_t) * t.srcPtr.size()));
  HIP_TRY(lm_upload(lm->srcRow, t.srcRow.data(), sizeof(int32_t) * t.srcRow.size()));
  HIP_TRY(lm_upload(lm->srcVal, t.srcVal.data(), sizeof(float) * t.srcVal.size()));
  *out = lm.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_landmarks_destroy(struct smplpp_landmarks * lm)
{
  if(!lm) return SMPLPP_OK;
  (void)hipSetDevice(lm->device);
  delete lm;
  return SMPLPP_OK;
}

extern "C" int smplpp_landmarks_info(const struct smplpp_landmarks * lm, int64_t * L, int64_t * nnz)
{
  if(!lm) return fail(SMPLPP_ERR_INVALID, "smplpp_landmarks_info: no regressor");
  if(L) *L = lm->L;
  if(nnz) *nnz = lm->nnz;
  return SMPLPP_OK;
}

extern "C" int smplpp_landmarks(struct smplpp_landmarks * lm, int64_t n, const float * verts, const float * joints, float * points, int space,
                                void * stream)
{
  const char * fn = "smplpp_landmarks";
  if(int rc = lm_check(fn, lm, n, space)) return rc;
  if(!verts || !joints || !points) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": verts, joints or points is NULL");
  Frame fr(lm->device, &lm->arena, space, stream, "landmarks");
  const float * v = fr.in(verts, (size_t)n * lm->V * 3);
  const float * j = fr.in(joints, (size_t)n * NJ * 3);
  float * p = fr.out(points, (size_t)n * lm->L * 3);
  return fr.run([&] {
    const int64_t total = n * lm->L;
    lm_forward_kernel<<<dim3((unsigned)((total * LM_SPLIT + LM_T - 1) / LM_T)), dim3(LM_T), 0, fr.st>>>(
        lm->rowPtr.as<int32_t>(), lm->col.as<int32_t>(), lm->val.as<float>(), v, j, p, (int)lm->L, (int)lm->V, total);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_landmarks_vjp(struct smplpp_landmarks * lm, int64_t n, const float * grad_points, float * grad_verts, float * grad_joints,
                                    int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_landmarks_vjp";
  if(int rc = lm_check(fn, lm, n, space)) return rc;
  if(!grad_points) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_points is NULL");
  if(!grad_verts && !grad_joints) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_verts and grad_joints are both NULL");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  Frame fr(lm->device, &lm->arena, space, stream, "landmarks VJP");
  const float * g = fr.in(grad_points, (size_t)n * lm->L * 3);
  float * gv = fr.out(grad_verts, (size_t)n * lm->V * 3, accumulate);
  float * gj = fr.out(grad_joints, (size_t)n * NJ * 3, accumulate);
  return fr.run([&] {
    const int64_t lo = grad_verts ? 0 : lm->V, hi = grad_joints ? lm->V + NJ : lm->V;
    const int64_t cnt3 = (hi - lo) * 3, total = n * cnt3;
    lm_vjp_kernel<<<dim3((unsigned)((total + LM_T - 1) / LM_T)), dim3(LM_T), 0, fr.st>>>(
        lm->srcPtr.as<int32_t>(), lm->srcRow.as<int32_t>(), lm->srcVal.as<float>(), g, gv, gj, (int)lm->L, (int)lm->V, (int)lo, cnt3, total,
        accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_project_points(int device, int64_t n, int64_t K, const float * points, const float * camera, float near,
                                     const float * target, float rho, float * uv, float * energy, uint8_t * valid, int space, void * stream)
{
  const char * fn = "smplpp_project_points";
  if(int rc = pp_check(fn, n, K, near, rho, space)) return rc;
  if(!points || !camera) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": points or camera is NULL");
  if(!uv && !energy && !valid) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": uv, energy and valid are all NULL");
  if(energy && !target) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": energy needs target");
  const size_t nk = (size_t)n * K;
  Frame fr(device, nullptr, space, stream, "project points");
  const float * p = fr.in(points, nk * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const float * t = energy ? fr.in(target, nk * 3) : nullptr;
  float * o_uv = fr.out(uv, nk * 2);
  float * o_e = fr.out(energy, nk);
  uint8_t * o_v = fr.out(valid, nk);
  return fr.run([&] {
    pp_forward_kernel<<<dim3((unsigned)((nk + LM_T - 1) / LM_T)), dim3(LM_T), 0, fr.st>>>(p, c, near, t, rho, o_uv, o_e, o_v, (int)K,
                                                                                        (int64_t)nk);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_project_points_vjp(int device, int64_t n, int64_t K, const float * points, const float * camera, float near,
                                         const float * target, float rho, const float * grad_uv, const float * grad_energy,
                                         float * grad_points, float * grad_camera, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_project_points_vjp";
  if(int rc = pp_check(fn, n, K, near, rho, space)) return rc;
  if(!points || !camera) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": points or camera is NULL");
  if(!grad_uv && !grad_energy) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_uv and grad_energy are both NULL");
  if(grad_energy && !target) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_energy needs target");
  if(!grad_points && !grad_camera) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_points and grad_camera are both NULL");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  const size_t nk = (size_t)n * K;
  Frame fr(device, nullptr, space, stream, "project points VJP");
  const float * p = fr.in(points, nk * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const float * t = grad_energy ? fr.in(target, nk * 3) : nullptr;
  const float * guv = fr.in(grad_uv, nk * 2);
  const float * ge = fr.in(grad_energy, nk);
  float * gp = fr.out(grad_points, nk * 3, accumulate);
  float * gc = fr.out(grad_camera, (size_t)n * 16, accumulate);
  return fr.run([&] {
    if(gc) pp_vjp_frame_kernel<<<dim3((unsigned)n), dim3(PP_W), 0, fr.st>>>(p, c, near, t, rho, guv, ge, gp, gc, (int)K, accumulate);
    else
      pp_vjp_points_kernel<<<dim3((unsigned)((nk + LM_T - 1) / LM_T)), dim3(LM_T), 0, fr.st>>>(p, c, near, t, rho, guv, ge, gp, (int)K,
                                                                                             (int64_t)nk, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
