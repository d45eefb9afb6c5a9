// Generalized winding numbers of each frame's posed mesh at K query points per frame (which points lie inside the body), and the
// signed point-to-mesh distance built on them, with its vector-Jacobian product (penetration terms, one-sided scan terms).
//
// Winding numbers (smplpp_point_mesh_winding): the bits of the sweep grid's winding_kernel (mesh.hip) at the same fp32 position, by
// construction: the same per-face term (winding_device.h), summed in fp32 in ascending face order within each 256-face chunk, the
// chunk partials summed in fp64 in ascending chunk order from 0.0, then (float)(acc / (2 pi)).
//  wn_scan_kernel    one point per lane, in registers (64..256 lanes per workgroup, from K), the frame's faces streamed through LDS one
//                    chunk at a time (every lane reads the same face: broadcasts).  With few (frame, point block) workgroups the call
//                    splits the chunks over `slices` workgroups at chunk boundaries (chosen from n and K alone) and each writes its
//                    chunks' fp32 partials; unsplit, the workgroup sums its partials in fp64 itself.
//  wn_reduce_kernel  a split call's partials: one thread per (frame, point), the fp64 sum in ascending chunk order.
//                    Either way the same fp32 partials are summed in the same order: the bits do not depend on n, slot or split.
// Signed distance (smplpp_point_mesh_signed_distance): smplpp_point_mesh_distance's forward (pd_forward_device, in a workspace of
// its own), then the winding numbers, whose last step negates sqdist in place where the point is inside (w > 0.5).
// Backward: sigma = inside ? -1 : 1 is piecewise constant, so the product is smplpp_point_mesh_distance_vjp's at the cotangent
// sigma g: wn_sign_kernel writes sigma g (a negation: exact) into this workspace, then pd_vjp_device.
#include "point_distance.h"
#include "winding_device.h"

namespace smplpp_hip
{
struct WindingState
{
  StatePtr<PointDistState> pd; // the signed distance's point-to-mesh workspace
  DevBuf part;                 // [n][chunks][K] fp32 chunk partials of a split call
  DevBuf gs;                   // [n][K] sigma g of the backward pass
};
void StateDelete::operator()(WindingState * s) const
{
  delete s;
}

constexpr int WN_CHUNK = 256;                // faces per chunk: the sweep grid's LDS tile, so the partials are its partials
constexpr int64_t WN_TARGET_WAVES = 8192;    // below this many wavefronts (256 CUs x 32) the call splits the chunks

static int64_t wn_threads(int64_t K) // lanes per workgroup: 256, or K rounded up to whole wavefronts
{
  return K >= 256 ? 256 : (K + 63) / 64 * 64;
}

// chunks per slice: from (n, K) alone, so the same call always splits the same way
static int64_t wn_per_slice(int64_t n, int64_t K, int64_t chunks)
{
  const int64_t T = wn_threads(K);
  const int64_t waves = n * ((K + T - 1) / T) * (T / 64);
  if(waves >= WN_TARGET_WAVES) return chunks;
  int64_t s = (WN_TARGET_WAVES + waves - 1) / waves;
  if(s > chunks) s = chunks;
  return (chunks + s - 1) / s;
}

// winding_kernel's epilogue, plus the sign of the signed distance
__device__ inline void wn_store(int64_t i, double acc, float * __restrict__ winding, uint8_t * __restrict__ inside, float * __restrict__ sq)
{
  const float w = (float)(acc / (2.0 * 3.14159265358979323846));
  const bool in = w > 0.5f; // (false for NaN)
  if(winding) winding[i] = w;
  if(inside) inside[i] = in ? 1 : 0;
  if(sq && in) sq[i] = -sq[i];
}

__global__ __launch_bounds__(256) void wn_scan_kernel(const float * __restrict__ verts, const int32_t * __restrict__ faces,
                                                      const float * __restrict__ points, float * __restrict__ part,
                                                      float * __restrict__ winding, uint8_t * __restrict__ inside, float * __restrict__ sq,
                                                      int64_t V, int64_t F, int64_t K, int64_t kblocks, int64_t slices, int64_t per_slice)
{
  __shared__ float tri[WN_CHUNK][9];
  const uint32_t b = blockIdx.x; // (the grid is below 2^31)
  const int64_t kb = b % (uint32_t)kblocks, fs = b / (uint32_t)kblocks;
  const int64_t s = (uint32_t)fs % (uint32_t)slices, frame = (uint32_t)fs / (uint32_t)slices;
  const int64_t k = kb * blockDim.x + threadIdx.x;
  const bool live = k < K;
  const int64_t q = frame * K + (live ? k : K - 1); // lanes past K repeat the last point and write nothing
  const float px = points[q * 3], py = points[q * 3 + 1], pz = points[q * 3 + 2];
  const float * vf = verts + frame * V * 3;
  const int64_t chunks = (F + WN_CHUNK - 1) / WN_CHUNK;
  const int64_t c0 = s * per_slice, c1 = c0 + per_slice < chunks ? c0 + per_slice : chunks;
  double acc = 0.0;
  for(int64_t c = c0; c < c1; c++)
  {
    const int64_t f0 = c * WN_CHUNK;
    for(int j = threadIdx.x; j < WN_CHUNK; j += blockDim.x)
      if(f0 + j < F)
#pragma unroll
        for(int v = 0; v < 3; v++)
        {
          const float * x = vf + 3 * (int64_t)faces[(f0 + j) * 3 + v];
          tri[j][v * 3 + 0] = x[0];
          tri[j][v * 3 + 1] = x[1];
          tri[j][v * 3 + 2] = x[2];
        }
    __syncthreads();
    const int cnt = (int)(F - f0 < WN_CHUNK ? F - f0 : WN_CHUNK);
    float p = 0.0f;
    for(int t = 0; t < cnt; t++) p += winding_term(tri[t], px, py, pz);
    if(slices == 1) acc += (double)p;
    else if(live) part[(frame * chunks + c) * K + k] = p;
    __syncthreads();
  }
  if(slices == 1 && live) wn_store(frame * K + k, acc, winding, inside, sq);
}

__global__ __launch_bounds__(256) void wn_reduce_kernel(const float * __restrict__ part, float * __restrict__ winding,
                                                        uint8_t * __restrict__ inside, float * __restrict__ sq, int64_t K, int64_t chunks,
                                                        int64_t nk)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nk) return;
  const float * pf = part + (i / K) * chunks * K + i % K;
  double acc = 0.0;
#pragma unroll 8
  for(int64_t c = 0; c < chunks; c++) acc += (double)pf[c * K]; // (unrolled: the loads are independent; the adds keep their order)
  wn_store(i, acc, winding, inside, sq);
}

__global__ __launch_bounds__(256) void wn_sign_kernel(const float * __restrict__ g, const uint8_t * __restrict__ inside, float * __restrict__ gs,
                                                      int64_t nk)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nk) return;
  gs[i] = inside[i] ? -g[i] : g[i];
}

static WindingState * wn_state(smplpp_model * m)
{
  if(!m->wn)
  {
    m->wn.reset(new WindingState());
    m->wn->pd.reset(new PointDistState());
  }
  return m->wn.get();
}

// all pointers on the device; sq (nullable) is negated where inside
static int wn_forward_device(smplpp_model * m, WindingState * s, int64_t n, const float * verts, int64_t K, const float * points,
                             float * winding, uint8_t * inside, float * sq, hipStream_t st)
{
  const int64_t F = m->F, chunks = (F + WN_CHUNK - 1) / WN_CHUNK;
  const int64_t T = wn_threads(K), kblocks = (K + T - 1) / T;
  const int64_t per = wn_per_slice(n, K, chunks), slices = (chunks + per - 1) / per;
  if(n * kblocks * slices > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, "smplpp_point_mesh_winding: grid beyond int32");
  float * part = nullptr;
  if(slices > 1)
  {
    HIP_TRY(s->part.reserve(sizeof(float) * (size_t)(n * chunks * K)));
    part = s->part.as<float>();
  }
  wn_scan_kernel<<<dim3((unsigned)(n * kblocks * slices)), dim3((unsigned)T), 0, st>>>(verts, m->faces.get(), points, part, winding, inside, sq,
                                                                                       m->V, F, K, kblocks, slices, per);
  HIP_TRY(hipGetLastError());
  if(slices > 1)
  {
    wn_reduce_kernel<<<dim3((unsigned)((n * K + 255) / 256)), dim3(256), 0, st>>>(part, winding, inside, sq, K, chunks, n * K);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

static int wn_check(const char * fn, smplpp_model * m, int64_t n, int64_t K, int space)
{
  const std::string name(fn);
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, name + ": model has no faces");
  // every [n,K] index and every grid stays in int32 (the backward's gather grid is n * ceil(V / 256))
  if(n > 0x7fffffffLL || K > 0x7fffffffLL || n * K > 0x7fffffffLL || n * ((m->V + GATHER_T - 1) / GATHER_T) > 0x7fffffffLL)
    return fail(SMPLPP_ERR_INVALID, name + ": n * K beyond int32 indexing");
  return check_space(space, fn);
}

extern "C" int smplpp_point_mesh_winding(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points, float * winding,
                                         uint8_t * inside, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_winding";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !winding) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = wn_check(fn, m, n, K, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "point-mesh winding");
  WindingState * s = wn_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  float * wo = fr.out(winding, (size_t)n * K);
  uint8_t * io = fr.out(inside, (size_t)n * K);
  return fr.run([&] { return wn_forward_device(m, s, n, v, K, p, wo, io, nullptr, fr.st); });
}

extern "C" int smplpp_point_mesh_signed_distance(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                                 int64_t * face, float * weights, float * closest, float * winding, uint8_t * inside,
                                                 float * signed_sqdist, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_signed_distance";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !face || !inside || !signed_sqdist)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  int rc = wn_check(fn, m, n, K, space);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "signed point-mesh distance");
  WindingState * s = wn_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * p = fr.in(points, (size_t)n * K * 3);
  int64_t * fo = fr.out(face, (size_t)n * K);
  float * wo = fr.out(weights, (size_t)n * K * 3);
  float * co = fr.out(closest, (size_t)n * K * 3);
  float * wno = fr.out(winding, (size_t)n * K);
  uint8_t * io = fr.out(inside, (size_t)n * K);
  float * so = fr.out(signed_sqdist, (size_t)n * K);
  return fr.run([&]() -> int {
    int rc = pd_forward_device(m, s->pd.get(), n, v, K, p, fo, wo, co, so, fr.st);
    return rc ? rc : wn_forward_device(m, s, n, v, K, p, wno, io, so, fr.st);
  });
}

extern "C" int smplpp_point_mesh_signed_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                                     const int64_t * face, const uint8_t * inside, const float * grad_signed_sqdist,
                                                     float * grad_verts, float * grad_points, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_point_mesh_signed_distance_vjp";
  if(!m || n <= 0 || K <= 0 || !verts || !points || !face || !inside || !grad_signed_sqdist || (!grad_verts && !grad_points))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = wn_check(fn, m, n, K, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * K, 0, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "signed point-mesh distance VJP");
  WindingState * s = wn_state(m);
  const uint8_t * ind = fr.in(inside, (size_t)n * K);
  auto device = [s, ind](smplpp_model * m, PointDistState * pd, int64_t n, const float * v, int64_t K, const float * p, const int64_t * id,
                         const float * g, float * gv, float * gp, int acc, hipStream_t st) -> int {
    HIP_TRY(s->gs.reserve(sizeof(float) * (size_t)(n * K)));
    float * gs = s->gs.as<float>();
    wn_sign_kernel<<<dim3((unsigned)((n * K + 255) / 256)), dim3(256), 0, st>>>(g, ind, gs, n * K);
    HIP_TRY(hipGetLastError());
    return pd_vjp_device(m, pd, n, v, K, p, id, gs, gv, gp, acc, st);
  };
  return distance_vjp(fr, device, m, s->pd.get(), n, verts, K, points, face, n * K, grad_signed_sqdist, grad_verts, grad_points, accumulate);
}
