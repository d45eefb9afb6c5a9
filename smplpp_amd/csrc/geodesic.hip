// Surface geodesics on the mesh graph and the geodesic-filtered self-contact search.  The rules are in
// include/smplpp_hip.h and edge_tables.h; every fp32 operation below is rounded on its own (no contraction to FMA), every choice is
// the minimum of a total order, and there are no floating-point atomics.
//
//  geo_weight_kernel    a thread per (frame, directed edge): the edge's length into the workspace [n][nnz], +inf for a length that is
//                       not finite.  Both directions of an edge compute d = x_hi - x_lo, so they hold the same bits.
//  geo_relax_kernel     a workgroup per (frame, source set), the field in LDS (V floats, dynamic, and no static LDS beside it; above
//                       64 KiB by opt-in).  Pull form: thread t owns vertices t, t + 1024, ...; it reads its neighbours' values and
//                       writes only its own, so there are no write conflicts and no atomics.  A read may see a neighbour's value of
//                       this sweep or of the last one: both are sums along realised paths, which is all the rule asks
//                       (edge_tables.h).  The exit is workgroup-uniform: a changed flag that every thread reads after the sweep's
//                       barrier, and the loop ends at V sweeps regardless.
//  sc_upper_kernel      handle creation: from a batch of single-source fields on the rest mesh, the bits far(v, u) for u > v
//                       (source v = the lower index, read at u), a thread per (row, word).
//  sc_mirror_kernel     the full rows: bit u < v of row v is bit v of row u.  It also counts the far pairs (an integer atomic).
//  sc_scan_kernel       mesh_point_distance.hip's vertex scan with the frame's own vertices as candidates: SC_VPL query vertices per
//                       lane in registers, the candidates through LDS SC_TILE at a time, and per query one word of its mask row for
//                       every 32 candidates (the next group's words are loaded while this group's are used).  The same chunking of
//                       the candidates, partial (d, u) pairs and lexicographic reduction as the scan it copies: a minimum over a
//                       total order does not depend on the split.
//  smplpp_self_contact_vjp  no kernel of its own: smplpp_mesh_point_distance_vjp twice, on a private model handle that holds only V
//                       and the device.
#include "edge_tables.h"
#include "scan_compat.h"
#include "staging.h"

#include <cmath>

namespace smplpp_hip
{
// the device copy of an edge table and the edge lengths of the frames of the call in flight
struct GeoTables
{
  int64_t V = 0, nnz = 0;
  DevBuf off, adj, src; // edge_tables.h
  DevBuf w;             // [n][nnz]
};
struct GeodesicState
{
  bool ready = false;
  GeoTables t;
};
void StateDelete::operator()(GeodesicState * s) const
{
  delete s;
}
} // namespace smplpp_hip

struct smplpp_self_contact
{
  int device = 0;
  int64_t V = 0, W = 0, far_pairs = 0;
  float geo_min = 0.0f;
  smplpp_hip::DevBuf mask;                 // [V][W] the far relation
  smplpp_hip::DevBuf part_d, part_k;       // [n][chunks][V] partial (d, u) of a split search
  std::unique_ptr<smplpp_model> shadow;    // V and the device: what smplpp_mesh_point_distance_vjp reads of a model, and its workspace
  smplpp_hip::Arena arena;                 // staging of the host-space calls on this handle
};

namespace smplpp_hip
{
using SelfContact = struct ::smplpp_self_contact; // (the bare name is the search)

constexpr int SC_THREADS = 256;
constexpr int SC_VPL = 4;                          // query vertices per lane
constexpr int SC_VBLOCK = SC_THREADS * SC_VPL;     // query vertices per workgroup
constexpr int SC_TILE = 1024;                      // candidates per LDS tile (float4: 16 KiB, twice with normals)
constexpr int SC_GROUP = 32;                       // candidates per mask word: every chunk starts at a multiple of it
constexpr int64_t SC_TARGET_WG = 2048;             // below this many (frame, query block) workgroups the call splits the candidates ...
constexpr int64_t SC_MIN_CHUNK = 256;              // ... into chunks of at least this many
constexpr int64_t SC_FIELD_BYTES = 32ll << 20;     // handle creation: bytes of fields in flight per batch of sources

template<class T>
static hipError_t geo_upload(DevBuf & dst, const std::vector<T> & src)
{
  hipError_t e = dst.reserve(sizeof(T) * (src.size() ? src.size() : 1));
  if(e == hipSuccess && !src.empty()) e = hipMemcpy(dst.p.get(), src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
  return e;
}
static hipError_t geo_upload_tables(GeoTables & g, const EdgeTable & t)
{
  g.V = t.V, g.nnz = t.nnz;
  hipError_t e = geo_upload(g.off, t.off);
  if(e == hipSuccess) e = geo_upload(g.adj, t.adj);
  if(e == hipSuccess) e = geo_upload(g.src, t.src);
  return e;
}

// ---- geodesics
__global__ __launch_bounds__(256) void geo_weight_kernel(const float * __restrict__ verts, const int32_t * __restrict__ src,
                                                         const int32_t * __restrict__ adj, float * __restrict__ w, int64_t V, int64_t nnz,
                                                         int64_t total)
{
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= total) return;
  const int64_t frame = i / nnz, e = i % nnz;
  const int a = src[e], b = adj[e];
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const float * X = verts + frame * V * 3;
  const float dx = X[hi * 3] - X[lo * 3], dy = X[hi * 3 + 1] - X[lo * 3 + 1], dz = X[hi * 3 + 2] - X[lo * 3 + 2];
  const float l = sqrtf((dx * dx + dy * dy) + dz * dz); // (the correctly rounded one: the library is built without fast-math)
  w[i] = fabsf(l) < INFINITY ? l : INFINITY; // (a NaN fails the comparison)
}

__global__ __launch_bounds__(GEO_THREADS) void geo_relax_kernel(const int32_t * __restrict__ off, const int32_t * __restrict__ adj,
                                                                const float * __restrict__ w, const int64_t * __restrict__ source_ptr,
                                                                const int64_t * __restrict__ source_vertex, float max_dist,
                                                                float * __restrict__ dist, int V, int64_t nnz, int S, int max_sweeps)
{
  extern __shared__ float s_d[];                      // [V] the field, then GEO_LDS_FLAGS bytes (edge_tables.h, geodesic_plan)
  int * s_flag = reinterpret_cast<int *>(s_d + V);    // [3] flag k mod 3: sweep k changed a value
  const int t = threadIdx.x;
  const int64_t frame = blockIdx.x / (uint32_t)S, s = blockIdx.x % (uint32_t)S;
  const float * wf = w + frame * nnz;
  for(int v = t; v < V; v += GEO_THREADS) s_d[v] = INFINITY;
  if(t < 3) s_flag[t] = 0;
  __syncthreads();
  for(int64_t e = source_ptr[s] + t; e < source_ptr[s + 1]; e += GEO_THREADS)
  {
    const int64_t q = source_vertex[e];
    if(q >= 0 && q < V) s_d[q] = 0.0f; // (a repeated source stores the same +0)
  }
  __syncthreads();
  for(int sweep = 0; sweep < max_sweeps; sweep++)
  {
    bool changed = false;
    for(int v = t; v < V; v += GEO_THREADS)
    {
      const float old = s_d[v];
      float cur = old;
      const int e1 = off[v + 1];
      for(int e = off[v]; e < e1; e++)
      {
        const float cand = s_d[adj[e]] + wf[e];
        if(cand < cur && cand <= max_dist) cur = cand;
      }
      if(cur < old)
      {
        s_d[v] = cur;
        changed = true;
      }
    }
    const int k = sweep % 3;
    if(changed) s_flag[k] = 1;
    __syncthreads();
    const int any = s_flag[k];
    if(t == 0) s_flag[(k + 2) % 3] = 0; // read last before this sweep's barrier, set next after the next one
    if(!any) break;
  }
  float * out = dist + (frame * S + s) * (int64_t)V;
  for(int v = t; v < V; v += GEO_THREADS) out[v] = s_d[v]; // (every finite value is <= max_dist: no candidate above it was kept)
}

static int geo_weights(GeoTables & g, int64_t n, const float * verts, hipStream_t st)
{
  if(g.nnz == 0) return SMPLPP_OK;
  HIP_TRY(g.w.reserve(sizeof(float) * (size_t)(n * g.nnz)));
  const int64_t total = n * g.nnz;
  geo_weight_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(verts, g.src.as<int32_t>(), g.adj.as<int32_t>(), g.w.as<float>(),
                                                                                g.V, g.nnz, total);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// the fields of n frames and S source sets from the lengths geo_weights left in g.w; all pointers on the device
static int geo_relax(GeoTables & g, int device, int64_t n, int64_t S, const int64_t * source_ptr, const int64_t * source_vertex, float max_dist,
                     float * dist, hipStream_t st)
{
  static PerDeviceOnce once;
  const GeodesicPlan p = geodesic_plan(g.V);
  if(p.opt_in) // (one opt-in per device serves every V: it asks for the largest field)
    HIP_TRY(lds_opt_in(once, device, reinterpret_cast<const void *>(geo_relax_kernel), (int)geodesic_plan(GEO_MAX_V).lds_bytes));
  geo_relax_kernel<<<dim3((unsigned)(n * S)), dim3(GEO_THREADS), (size_t)p.lds_bytes, st>>>(g.off.as<int32_t>(), g.adj.as<int32_t>(), g.w.as<float>(),
                                                                                          source_ptr, source_vertex, max_dist, dist, (int)g.V, g.nnz,
                                                                                          (int)S, (int)p.max_sweeps);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// ---- the far mask
// dist [rows][V]: the field of source s0 + r in row r
__global__ __launch_bounds__(256) void sc_upper_kernel(const float * __restrict__ dist, uint32_t * __restrict__ upper, float geo_min, int s0,
                                                       int rows, int V, int W)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= (int64_t)rows * W) return;
  const int r = (int)(i / W), wd = (int)(i % W), v = s0 + r;
  const float * d = dist + (int64_t)r * V;
  uint32_t bits = 0;
  for(int b = 0; b < 32; b++)
  {
    const int u = wd * 32 + b;
    if(u > v && u < V && d[u] > geo_min) bits |= 1u << b;
  }
  upper[(int64_t)v * W + wd] = bits;
}

__global__ __launch_bounds__(256) void sc_mirror_kernel(const uint32_t * __restrict__ upper, uint32_t * __restrict__ mask,
                                                        unsigned long long * __restrict__ pairs, int V, int W)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= (int64_t)V * W) return;
  const int v = (int)(i / W), wd = (int)(i % W);
  uint32_t bits = upper[i];
  if(bits) atomicAdd(pairs, (unsigned long long)__popc(bits));
  if(wd <= v >> 5)
    for(int b = 0; b < 32; b++)
    {
      const int u = wd * 32 + b;
      if(u < v) bits |= ((upper[(int64_t)u * W + (v >> 5)] >> (v & 31)) & 1u) << b;
    }
  mask[i] = bits;
}

// ---- the search
__device__ inline float sc_sqdist(float vx, float vy, float vz, float px, float py, float pz)
{
#pragma clang fp contract(off)
  const float dx = vx - px, dy = vy - py, dz = vz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// candidate chunks of one call: from (n, V) alone, a multiple of SC_GROUP
static int64_t sc_chunk_len(int64_t n, int64_t V)
{
  const int64_t wg = n * ((V + SC_VBLOCK - 1) / SC_VBLOCK);
  if(wg >= SC_TARGET_WG || V < 2 * SC_MIN_CHUNK) return (V + SC_GROUP - 1) / SC_GROUP * SC_GROUP;
  int64_t s = (SC_TARGET_WG + wg - 1) / wg;
  if(s > V / SC_MIN_CHUNK) s = V / SC_MIN_CHUNK;
  return ((V + s - 1) / s + SC_GROUP - 1) / SC_GROUP * SC_GROUP;
}

template<bool NORMALS>
__global__ __launch_bounds__(SC_THREADS) void sc_scan_kernel(const float * __restrict__ verts, const float * __restrict__ vnormals,
                                                             const uint32_t * __restrict__ mask, float c2, float max_sq,
                                                             int64_t * __restrict__ index_out, float * __restrict__ sq_out,
                                                             float * __restrict__ part_d, int32_t * __restrict__ part_k, int V, int W,
                                                             int vblocks, int chunks, int chunk)
{
  __shared__ float4 s_p[SC_TILE];
  __shared__ float4 s_q[NORMALS ? SC_TILE : 1];
  const uint32_t blk = blockIdx.x; // (the grid is below 2^31: 32-bit index arithmetic)
  const int vb = (int)(blk % (uint32_t)vblocks);
  const int64_t fc = blk / (uint32_t)vblocks; // frame * chunks + c
  const int c = (int)((uint32_t)fc % (uint32_t)chunks);
  const int64_t frame = (uint32_t)fc / (uint32_t)chunks;
  const int k0 = c * chunk, k1 = k0 + chunk < V ? k0 + chunk : V; // (k0 is a multiple of SC_GROUP)
  const int t = threadIdx.x;
  const float * vf = verts + frame * V * 3;
  float vx[SC_VPL], vy[SC_VPL], vz[SC_VPL], bd[SC_VPL];
  float4 vm[SC_VPL];
  const uint32_t * row[SC_VPL];
  int bk[SC_VPL];
#pragma unroll
  for(int i = 0; i < SC_VPL; i++)
  {
    int v = vb * SC_VBLOCK + i * SC_THREADS + t;
    if(v >= V) v = V - 1; // lanes past V repeat the last vertex and write nothing
    vx[i] = vf[v * 3];
    vy[i] = vf[v * 3 + 1];
    vz[i] = vf[v * 3 + 2];
    vm[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr(NORMALS)
    {
      const float * nf = vnormals + (frame * V + v) * 3;
      const float nx = nf[0], ny = nf[1], nz = nf[2];
      vm[i] = compat_finite3(nx, ny, nz) ? make_float4(nx, ny, nz, compat_dot(nx, ny, nz, nx, ny, nz)) : make_float4(NAN, NAN, NAN, NAN);
    }
    row[i] = mask + (int64_t)v * W;
    bd[i] = INFINITY;
    bk[i] = -1;
  }
  for(int base = k0; base < k1; base += SC_TILE)
  {
    const int cnt = k1 - base < SC_TILE ? k1 - base : SC_TILE;
    __syncthreads();
    for(int j = t; j < cnt; j += SC_THREADS)
    {
      const float * p = vf + (base + j) * 3;
      s_p[j] = make_float4(p[0], p[1], p[2], 0.0f);
      if constexpr(NORMALS)
      {
        // the candidate's normal negated: compat_normals(m, -q) is  s <= 0 && mm qq > 0 && s s >= c2 (mm qq)  on s = m . q, bit for bit
        const float * qf = vnormals + (frame * V + base + j) * 3;
        const float qx = qf[0], qy = qf[1], qz = qf[2];
        s_q[j] = compat_finite3(qx, qy, qz) ? make_float4(-qx, -qy, -qz, compat_dot(qx, qy, qz, qx, qy, qz)) : make_float4(NAN, NAN, NAN, NAN);
      }
    }
    __syncthreads();
    const int w0 = base / SC_GROUP, groups = (cnt + SC_GROUP - 1) / SC_GROUP; // (w0 + groups <= W: base + cnt <= V)
    uint32_t mw[SC_VPL], nx[SC_VPL];
#pragma unroll
    for(int i = 0; i < SC_VPL; i++) mw[i] = row[i][w0];
    for(int g = 0; g < groups; g++)
    {
#pragma unroll
      for(int i = 0; i < SC_VPL; i++) nx[i] = g + 1 < groups ? row[i][w0 + g + 1] : 0u;
      const int j0 = g * SC_GROUP, jn = cnt - j0 < SC_GROUP ? cnt - j0 : SC_GROUP;
#pragma unroll 4
      for(int b = 0; b < jn; b++)
      {
        const float4 p = s_p[j0 + b];
        const int k = base + j0 + b;
#pragma unroll
        for(int i = 0; i < SC_VPL; i++)
        {
          const float d = sc_sqdist(vx[i], vy[i], vz[i], p.x, p.y, p.z);
          if(((mw[i] >> b) & 1u) && d < bd[i] && d <= max_sq)
          {
            bool take = true;
            if constexpr(NORMALS) take = compat_normals(vm[i], s_q[j0 + b], c2);
            if(take)
            {
              bd[i] = d;
              bk[i] = k;
            }
          }
        }
      }
#pragma unroll
      for(int i = 0; i < SC_VPL; i++) mw[i] = nx[i];
    }
  }
#pragma unroll
  for(int i = 0; i < SC_VPL; i++)
  {
    const int v = vb * SC_VBLOCK + i * SC_THREADS + t;
    if(v >= V) continue;
    if(chunks == 1)
    {
      index_out[frame * V + v] = bk[i];
      sq_out[frame * V + v] = bk[i] < 0 ? 0.0f : bd[i];
    }
    else
    {
      part_d[fc * V + v] = bd[i];
      part_k[fc * V + v] = bk[i];
    }
  }
}

// the lexicographic (d, u) minimum over a vertex's chunks
__global__ __launch_bounds__(256) void sc_reduce_kernel(const float * __restrict__ part_d, const int32_t * __restrict__ part_k,
                                                        int64_t * __restrict__ index_out, float * __restrict__ sq_out, int64_t V,
                                                        int64_t chunks, int64_t nv)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nv) return;
  const int64_t frame = i / V, v = i % V;
  float bd = INFINITY;
  int bk = -1;
#pragma unroll 8
  for(int64_t c = 0; c < chunks; c++)
  {
    const int64_t j = (frame * chunks + c) * V + v;
    const int k = part_k[j];
    const float d = part_d[j];
    if(k >= 0 && (bk < 0 || d < bd || (d == bd && k < bk)))
    {
      bd = d;
      bk = k;
    }
  }
  index_out[i] = bk;
  sq_out[i] = bk < 0 ? 0.0f : bd;
}

// all pointers on the device
template<bool NORMALS>
static int sc_forward_device(SelfContact * sc, int64_t n, const float * verts, const float * vnormals, float c2, float max_sq, int64_t * index,
                             float * sqdist, hipStream_t st)
{
  const int64_t V = sc->V;
  const int64_t vblocks = (V + SC_VBLOCK - 1) / SC_VBLOCK;
  const int64_t chunk = sc_chunk_len(n, V);
  const int64_t chunks = (V + chunk - 1) / chunk;
  float * pd = nullptr;
  int32_t * pk = nullptr;
  if(chunks > 1)
  {
    HIP_TRY(sc->part_d.reserve(sizeof(float) * (size_t)(n * chunks * V)));
    HIP_TRY(sc->part_k.reserve(sizeof(int32_t) * (size_t)(n * chunks * V)));
    pd = sc->part_d.as<float>();
    pk = sc->part_k.as<int32_t>();
  }
  sc_scan_kernel<NORMALS><<<dim3((unsigned)(n * chunks * vblocks)), dim3(SC_THREADS), 0, st>>>(verts, vnormals, sc->mask.as<uint32_t>(), c2, max_sq,
                                                                                             index, sqdist, pd, pk, (int)V, (int)sc->W, (int)vblocks,
                                                                                             (int)chunks, (int)chunk);
  HIP_TRY(hipGetLastError());
  if(chunks > 1)
  {
    sc_reduce_kernel<<<dim3((unsigned)((n * V + 255) / 256)), dim3(256), 0, st>>>(pd, pk, index, sqdist, V, chunks, n * V);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}

static int sc_check(const char * fn, const SelfContact * sc, int64_t n, int space)
{
  if(!sc) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no handle");
  if(n <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n must be positive");
  // every [n,V,3] index, every partial [n][chunks][V] index and every grid stays in int32
  if(n > GEO_INT32_MAX / 3 || n * sc->V * 3 > GEO_INT32_MAX)
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * V * 3 beyond int32 indexing");
  const int64_t chunk = sc_chunk_len(n, sc->V), chunks = (sc->V + chunk - 1) / chunk;
  if(n * chunks * sc->V > GEO_INT32_MAX) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * chunks * V beyond int32 indexing");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_mesh_geodesic(smplpp_model * m, int64_t n, const float * verts, int64_t S, const int64_t * source_ptr,
                                    const int64_t * source_vertex, float max_dist, float * dist, int space, void * stream)
{
  const std::string fn = "smplpp_mesh_geodesic";
  if(!m || n <= 0 || S <= 0 || !verts || !source_ptr || !dist) return fail(SMPLPP_ERR_INVALID, fn + ": bad argument");
  if(!(max_dist >= 0.0f)) return fail(SMPLPP_ERR_INVALID, fn + ": max_dist must be >= 0 (+inf: no cap)");
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, fn + ": the model has no faces");
  const GeodesicPlan plan = geodesic_plan(m->V);
  if(plan.refusal) return fail(SMPLPP_ERR_INVALID, fn + ": " + plan.refusal);
  if(n > GEO_INT32_MAX || S > GEO_INT32_MAX || n * S > GEO_INT32_MAX || n * S * m->V > GEO_INT32_MAX || n * m->V * 3 > GEO_INT32_MAX)
    return fail(SMPLPP_ERR_INVALID, fn + ": n * S * V beyond int32 indexing");
  if(int rc = check_space(space, fn.c_str())) return rc;
  // the source lists: checked on the host in either space (a device-space source_ptr is read back; the ids stay on the device)
  std::vector<int64_t> ptr_host;
  const int64_t * ptr = source_ptr;
  if(space == SMPLPP_DEVICE)
  {
    ptr_host.resize((size_t)S + 1);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(ptr_host.data(), source_ptr, sizeof(int64_t) * ((size_t)S + 1), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    ptr = ptr_host.data();
  }
  if(const char * why = geodesic_sources_refusal(m->V, S, ptr, nullptr)) return fail(SMPLPP_ERR_INVALID, fn + ": " + why);
  const int64_t ns = ptr[S];
  if(ns > 0 && !source_vertex) return fail(SMPLPP_ERR_INVALID, fn + ": source_vertex is NULL");
  if(space == SMPLPP_HOST)
    if(const char * why = geodesic_sources_refusal(m->V, S, ptr, source_vertex)) return fail(SMPLPP_ERR_INVALID, fn + ": " + why);
  if(!m->geo) m->geo.reset(new GeodesicState());
  GeodesicState * gs = m->geo.get();
  if(!gs->ready)
  {
    const EdgeTable t = edge_table(m->V, m->F, m->h_faces.data());
    if(t.refusal) return fail(SMPLPP_ERR_INVALID, fn + ": " + t.refusal);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(geo_upload_tables(gs->t, t));
    gs->ready = true;
  }
  if(n * gs->t.nnz > GEO_INT32_MAX * 256) return fail(SMPLPP_ERR_INVALID, fn + ": n * edges beyond the grid");
  Frame fr(m->device, &m->arena, space, stream, "mesh geodesic");
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const int64_t * sp = fr.in(source_ptr, (size_t)S + 1);
  const int64_t * sv = fr.in(source_vertex, (size_t)ns);
  float * d = fr.out(dist, (size_t)n * S * m->V);
  return fr.run([&]() -> int {
    if(int rc = geo_weights(gs->t, n, v, fr.st)) return rc;
    return geo_relax(gs->t, m->device, n, S, sp, sv, max_dist, d, fr.st);
  });
}

// The far mask of the rest mesh: a single-source field from every vertex, in batches through a bounded workspace; nothing of it but
// the mask stays on the handle.
extern "C" int smplpp_self_contact_create(smplpp_model * m, const float * rest, float geo_min, struct smplpp_self_contact ** out)
{
  const std::string fn = "smplpp_self_contact_create";
  if(out) *out = nullptr;
  if(!m || !out) return fail(SMPLPP_ERR_INVALID, fn + ": no model or no out");
  if(!rest) return fail(SMPLPP_ERR_INVALID, fn + ": rest is NULL");
  if(!(geo_min >= 0.0f && geo_min < INFINITY)) return fail(SMPLPP_ERR_INVALID, fn + ": geo_min must be finite and >= 0");
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, fn + ": the model has no faces");
  const GeodesicPlan plan = geodesic_plan(m->V);
  if(plan.refusal) return fail(SMPLPP_ERR_INVALID, fn + ": " + plan.refusal);
  const int64_t V = m->V, W = contact_mask_words(V);
  for(int64_t i = 0; i < V * 3; i++)
    if(!(std::fabs(rest[i]) < INFINITY)) return fail(SMPLPP_ERR_INVALID, fn + ": a rest coordinate is not finite");
  const EdgeTable t = edge_table(V, m->F, m->h_faces.data());
  if(t.refusal) return fail(SMPLPP_ERR_INVALID, fn + ": " + t.refusal);
  HIP_TRY(hipSetDevice(m->device));
  std::unique_ptr<SelfContact> sc(new SelfContact());
  sc->device = m->device, sc->V = V, sc->W = W, sc->geo_min = geo_min;
  sc->shadow.reset(new smplpp_model());
  sc->shadow->device = m->device, sc->shadow->V = V;
  GeoTables g;
  HIP_TRY(geo_upload_tables(g, t));
  const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(V, SC_FIELD_BYTES / (V * (int64_t)sizeof(float))));
  std::vector<int64_t> iota((size_t)V + 1);
  for(int64_t i = 0; i <= V; i++) iota[(size_t)i] = i; // source_ptr of single-source sets, and the sources themselves
  DevBuf d_rest, d_iota, d_dist, d_upper, d_pairs;
  HIP_TRY(d_rest.reserve(sizeof(float) * (size_t)V * 3));
  HIP_TRY(hipMemcpy(d_rest.p.get(), rest, sizeof(float) * (size_t)V * 3, hipMemcpyHostToDevice));
  HIP_TRY(geo_upload(d_iota, iota));
  HIP_TRY(d_dist.reserve(sizeof(float) * (size_t)(batch * V)));
  HIP_TRY(d_upper.reserve(sizeof(uint32_t) * (size_t)(V * W)));
  HIP_TRY(sc->mask.reserve(sizeof(uint32_t) * (size_t)(V * W)));
  HIP_TRY(d_pairs.reserve(sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(d_pairs.p.get(), 0, sizeof(unsigned long long), nullptr));
  if(int rc = geo_weights(g, 1, d_rest.as<float>(), nullptr)) return rc;
  for(int64_t s0 = 0; s0 < V; s0 += batch)
  {
    const int64_t rows = std::min(batch, V - s0);
    // capped at geo_min: a value above it is reported as +inf, which is still above it
    if(int rc = geo_relax(g, m->device, 1, rows, d_iota.as<int64_t>(), d_iota.as<int64_t>() + s0, geo_min, d_dist.as<float>(), nullptr)) return rc;
    sc_upper_kernel<<<dim3((unsigned)((rows * W + 255) / 256)), dim3(256), 0, nullptr>>>(d_dist.as<float>(), d_upper.as<uint32_t>(), geo_min, (int)s0,
                                                                                       (int)rows, (int)V, (int)W);
    HIP_TRY(hipGetLastError());
  }
  sc_mirror_kernel<<<dim3((unsigned)((V * W + 255) / 256)), dim3(256), 0, nullptr>>>(d_upper.as<uint32_t>(), sc->mask.as<uint32_t>(),
                                                                                   d_pairs.as<unsigned long long>(), (int)V, (int)W);
  HIP_TRY(hipGetLastError());
  unsigned long long pairs = 0;
  HIP_TRY(hipMemcpy(&pairs, d_pairs.p.get(), sizeof(pairs), hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(nullptr));
  sc->far_pairs = (int64_t)pairs;
  *out = sc.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_self_contact_destroy(struct smplpp_self_contact * sc)
{
  if(!sc) return SMPLPP_OK;
  (void)hipSetDevice(sc->device);
  delete sc;
  return SMPLPP_OK;
}

extern "C" int smplpp_self_contact_info(const struct smplpp_self_contact * sc, int64_t * V, int64_t * words_per_row, float * geo_min,
                                        int64_t * far_pairs)
{
  if(!sc) return fail(SMPLPP_ERR_INVALID, "smplpp_self_contact_info: no handle");
  if(V) *V = sc->V;
  if(words_per_row) *words_per_row = sc->W;
  if(geo_min) *geo_min = sc->geo_min;
  if(far_pairs) *far_pairs = sc->far_pairs;
  return SMPLPP_OK;
}

extern "C" int smplpp_self_contact_mask(const struct smplpp_self_contact * sc, uint32_t * mask, int space, void * stream)
{
  const char * fn = "smplpp_self_contact_mask";
  if(!sc || !mask) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no handle or no mask");
  if(int rc = check_space(space, fn)) return rc;
  Frame fr(sc->device, nullptr, space, stream, "self-contact mask");
  fr.fetch(mask, sc->mask.as<uint32_t>(), (size_t)(sc->V * sc->W));
  return fr.finish();
}

extern "C" int smplpp_self_contact(struct smplpp_self_contact * sc, int64_t n, const float * verts, const float * vert_normals, float cos_min,
                                   float max_sqdist, int64_t * index, float * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_self_contact";
  if(int rc = sc_check(fn, sc, n, space)) return rc;
  if(!verts || !index || !sqdist) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(int rc = compat_args(fn, cos_min, max_sqdist)) return rc;
  Frame fr(sc->device, &sc->arena, space, stream, "self-contact search");
  const float * v = fr.in(verts, (size_t)n * sc->V * 3);
  const float * vn = fr.in(vert_normals, (size_t)n * sc->V * 3);
  int64_t * io = fr.out(index, (size_t)n * sc->V);
  float * so = fr.out(sqdist, (size_t)n * sc->V);
  const float c2 = cos_min * cos_min;
  return fr.run([&] {
    return vert_normals ? sc_forward_device<true>(sc, n, v, vn, c2, max_sqdist, io, so, fr.st)
                        : sc_forward_device<false>(sc, n, v, nullptr, c2, max_sqdist, io, so, fr.st);
  });
}

extern "C" int smplpp_self_contact_vjp(struct smplpp_self_contact * sc, int64_t n, const float * verts, const int64_t * index,
                                       const float * grad_sqdist, float * grad_verts, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_self_contact_vjp";
  if(int rc = sc_check(fn, sc, n, space)) return rc;
  if(!verts || !index || !grad_sqdist || !grad_verts) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  if(space == SMPLPP_HOST)
    if(int rc = ids_in(fn, "partner index", index, n * sc->V, -1, sc->V)) return rc;
  Frame fr(sc->device, &sc->arena, space, stream, "self-contact VJP");
  const float * v = fr.in(verts, (size_t)n * sc->V * 3);
  const int64_t * id = fr.in(index, (size_t)n * sc->V);
  const float * g = fr.in(grad_sqdist, (size_t)n * sc->V);
  float * gv = fr.out(grad_verts, (size_t)n * sc->V * 3, accumulate);
  return fr.run([&]() -> int {
    // each vertex's own 2 g r, then one add of the ascending-v sum of -2 g r over the vertices that chose it
    smplpp_model * sm = sc->shadow.get();
    if(int rc = smplpp_mesh_point_distance_vjp(sm, n, v, sc->V, v, id, g, gv, nullptr, accumulate, SMPLPP_DEVICE, fr.st)) return rc;
    return smplpp_mesh_point_distance_vjp(sm, n, v, sc->V, v, id, g, nullptr, gv, 1, SMPLPP_DEVICE, fr.st);
  });
}
