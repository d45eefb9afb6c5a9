// Vector-Jacobian products of the three normal queries (smplpp_face_normals, smplpp_vertex_normals, smplpp_mesh_vertex_normals):
// the backward pass of SMPL::calcNormal / calcVertexNormal (src/SMPL.cpp:518-535) that the reference takes from libtorch autograd
// when its IK residual differentiates the mesh normals (src/IkTask.cpp:58-86, node/node.cpp:803-869).
//
// Per frame, with s_u the weighted sum of vertex u, c_f = a x b the cross product of face f and N torch's normalize:
//   1. per vertex  G_u = (1/deg_u) N'(s_u)^T g_n_u                    (the cotangent of every unit face normal in s_u)
//   2. per face    g_chat_f = sum over the face's DISTINCT corners u of G_u   (a face enters s_u once, as the reference's emplace)
//   3. per face    g_c_f = N'(c_f)^T g_chat_f, g_a = b x g_c, g_b = g_c x a
//   4. per vertex  the corner cotangents of its adjacent faces, gathered in ascending face id, corners in order.
// There are no floating-point atomics: every output element is one fixed-order sum, so a frame's bits do not depend on n or on
// its position in the batch.
//
// Kernels:
//  mesh_vjp_lds_kernel      whole mesh, one workgroup per frame: step 1 into LDS (V x 12 bytes: 82.7 KB at V = 6890), then steps
//                           2-4 per vertex, recomputing each adjacent face from the frame's vertices (L2-resident).
//  mesh_vjp_g_kernel /      the staged form for meshes whose G does not fit in LDS (or SMPLPP_NORMALS_VJP_STAGED=1): step 1 to a
//  mesh_vjp_gather_kernel   workspace [n][V][3], then steps 2-4 over (frame, vertex).
//  list_pairs_kernel,       list forms, set up once per call (an id list is the same for every frame): the (id, face) pairs in
//  list_rank_kernel,        list order and the records (pair, corner) -> target vertex, ranked by (target, record) without float
//  list_order_kernel        arithmetic (integer atomics only count), so each target's records are a contiguous run in record order.
//  list_vjp_lds_kernel /    one workgroup per frame: G per id (vertex lists), (g_a, g_b) per pair, then one sum per target vertex
//  list_vjp_ws_kernel       over its run, in LDS or (long lists) a workspace.  Only the target vertices are touched: the cost does
//                           not grow with V.
#include "mesh_grad.h"
#include "staging.h"
#include "trace.h"

#include <algorithm>
#include <cstdlib>

namespace smplpp_hip
{
struct NormalsVjpState
{
  DevBuf G;         // staged whole-mesh form: [n][V][3]
  DevBuf setup;     // list set-up: int32 hdr[4] | pairId[Pmax] | pairFace[Pmax] | tgt[Rmax] | pos[Rmax] | order[Rmax] | stgt[Rmax]
  DevBuf lbuf;      // list form whose per-frame buffer exceeds LDS: [n][buffer]
  int maxdeg = -1;  // largest vertex valence of the model (host, measured on the first call)
};
void StateDelete::operator()(NormalsVjpState * s) const
{
  delete s;
}

constexpr int LIST_LDS_BYTES = 64 * 1024;   // per-frame buffer of the list form kept in LDS up to this size (no opt-in needed)
constexpr int MESH_LDS_MAX = 160 * 1024;    // LDS of one workgroup on gfx950

// ---- whole mesh
__device__ inline void mesh_vertex_gather(const float * __restrict__ vf, const float * G, const int32_t * __restrict__ faces,
                                          const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace, int u, float * acc)
{
  acc[0] = acc[1] = acc[2] = 0.f;
  const int b = adjOff[u], e = adjOff[u + 1];
  for(int q = b; q < e; q++)
  {
    const int f = adjFace[q];
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    float gch[3] = {G[i0 * 3], G[i0 * 3 + 1], G[i0 * 3 + 2]};
    if(i1 != i0)
      for(int x = 0; x < 3; x++) gch[x] += G[i1 * 3 + x];
    if(i2 != i0 && i2 != i1)
      for(int x = 0; x < 3; x++) gch[x] += G[i2 * 3 + x];
    float ga[3], gb[3];
    face_normal_vjp_pts(vf + 3 * i0, vf + 3 * i1, vf + 3 * i2, gch, ga, gb);
    if(i0 == u)
      for(int x = 0; x < 3; x++) acc[x] += -(ga[x] + gb[x]);
    if(i1 == u)
      for(int x = 0; x < 3; x++) acc[x] += ga[x];
    if(i2 == u)
      for(int x = 0; x < 3; x++) acc[x] += gb[x];
  }
}

__global__ __launch_bounds__(1024) void mesh_vjp_lds_kernel(const float * __restrict__ verts, const float * __restrict__ gn,
                                                            float * __restrict__ gv, const int32_t * __restrict__ faces,
                                                            const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
                                                            int64_t V, int accumulate)
{
  extern __shared__ float sG[]; // [V][3]
  const int64_t fo = (int64_t)blockIdx.x * V * 3;
  const float * vf = verts + fo;
  for(int u = threadIdx.x; u < (int)V; u += blockDim.x)
  {
    float G[3];
    vertex_normal_vjp_dev(vf, faces, adjOff, adjFace, u, gn + fo + (int64_t)u * 3, G);
    sG[u * 3] = G[0];
    sG[u * 3 + 1] = G[1];
    sG[u * 3 + 2] = G[2];
  }
  __syncthreads();
  for(int u = threadIdx.x; u < (int)V; u += blockDim.x)
  {
    float acc[3];
    mesh_vertex_gather(vf, sG, faces, adjOff, adjFace, u, acc);
    float * o = gv + fo + (int64_t)u * 3;
    if(accumulate)
    {
      acc[0] = o[0] + acc[0];
      acc[1] = o[1] + acc[1];
      acc[2] = o[2] + acc[2];
    }
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
  }
}

__global__ __launch_bounds__(256) void mesh_vjp_g_kernel(const float * __restrict__ verts, const float * __restrict__ gn, float * __restrict__ G,
                                                         const int32_t * __restrict__ faces, const int32_t * __restrict__ adjOff,
                                                         const int32_t * __restrict__ adjFace, int64_t V, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n * V) return;
  const int64_t f = i / V;
  vertex_normal_vjp_dev(verts + f * V * 3, faces, adjOff, adjFace, (int)(i % V), gn + i * 3, G + i * 3);
}

__global__ __launch_bounds__(256) void mesh_vjp_gather_kernel(const float * __restrict__ verts, const float * __restrict__ G,
                                                              float * __restrict__ gv, const int32_t * __restrict__ faces,
                                                              const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace,
                                                              int64_t V, int64_t n, int accumulate)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n * V) return;
  const int64_t f = i / V;
  float acc[3];
  mesh_vertex_gather(verts + f * V * 3, G + f * V * 3, faces, adjOff, adjFace, (int)(i % V), acc);
  float * o = gv + i * 3;
  if(accumulate)
  {
    acc[0] = o[0] + acc[0];
    acc[1] = o[1] + acc[1];
    acc[2] = o[2] + acc[2];
  }
  o[0] = acc[0];
  o[1] = acc[1];
  o[2] = acc[2];
}

// ---- list forms: set-up (frame-independent)
struct ListSetup
{
  int32_t * hdr;      // [0] = pairs P (records R = 3 P)
  int32_t * pairId;   // [Pmax] index of the pair's id in the list
  int32_t * pairFace; // [Pmax] the pair's face
  int32_t * tgt;      // [Rmax] record r = 3 p + corner -> target vertex
  int32_t * pos;      // [Rmax] rank of (tgt[r], r) among all records
  int32_t * order;    // [Rmax] records by (target, record)
  int32_t * stgt;     // [Rmax] target of order[j]
};

// One workgroup: the pairs in list order (vertex list: an id's adjacent faces in ascending face id; face list: the id itself).
// An id out of range (possible only for device-space lists, which are not read on the host) has no pairs.
__global__ __launch_bounds__(256) void list_pairs_kernel(const int64_t * __restrict__ ids, int64_t count, int vertex,
                                                         const int32_t * __restrict__ faces, const int32_t * __restrict__ adjOff,
                                                         const int32_t * __restrict__ adjFace, int64_t V, int64_t F, ListSetup s)
{
  __shared__ int32_t sc[256];
  int32_t carry = 0;
  for(int64_t base = 0; base < count; base += 256)
  {
    const int64_t i = base + threadIdx.x;
    int32_t d = 0;
    int64_t id = -1;
    if(i < count)
    {
      id = ids[i];
      if(vertex) d = (id >= 0 && id < V) ? adjOff[id + 1] - adjOff[id] : 0;
      else d = (id >= 0 && id < F) ? 1 : 0;
    }
    sc[threadIdx.x] = d;
    __syncthreads();
    for(int off = 1; off < 256; off <<= 1)
    {
      const int32_t t = threadIdx.x >= off ? sc[threadIdx.x - off] : 0;
      __syncthreads();
      sc[threadIdx.x] += t;
      __syncthreads();
    }
    const int32_t p0 = carry + sc[threadIdx.x] - d;
    for(int32_t q = 0; q < d; q++)
    {
      const int32_t f = vertex ? adjFace[adjOff[id] + q] : (int32_t)id;
      s.pairId[p0 + q] = (int32_t)i;
      s.pairFace[p0 + q] = f;
      for(int k = 0; k < 3; k++)
      {
        s.tgt[3 * (p0 + q) + k] = faces[f * 3 + k];
        s.pos[3 * (p0 + q) + k] = 0;
      }
    }
    carry += sc[255];
    __syncthreads();
  }
  if(threadIdx.x == 0) s.hdr[0] = carry;
}

// pos[r] = #{q : (tgt[q], q) < (tgt[r], r)}, over a 2-D grid of (record tile, comparison tile); integer sums, so the result
// does not depend on the order the tiles land in.
__global__ __launch_bounds__(256) void list_rank_kernel(ListSetup s)
{
  __shared__ int32_t st[256];
  const int32_t R = 3 * s.hdr[0];
  const int32_t r0 = blockIdx.x * 256, q0 = blockIdx.y * 256;
  if(r0 >= R || q0 >= R) return;
  const int32_t q = q0 + threadIdx.x;
  st[threadIdx.x] = q < R ? s.tgt[q] : 0x7fffffff;
  __syncthreads();
  const int32_t r = r0 + threadIdx.x;
  if(r >= R) return;
  const int32_t t = s.tgt[r];
  const int32_t m = R - q0 < 256 ? R - q0 : 256;
  int32_t c = 0;
  for(int j = 0; j < m; j++)
  {
    const int32_t tq = st[j];
    c += (tq < t || (tq == t && q0 + j < r)) ? 1 : 0;
  }
  if(c) atomicAdd(&s.pos[r], c);
}

__global__ __launch_bounds__(256) void list_order_kernel(ListSetup s, int32_t Rmax)
{
  const int32_t R = 3 * s.hdr[0];
  const int32_t r = blockIdx.x * 256 + threadIdx.x;
  if(r >= R || r >= Rmax) return;
  const int32_t p = s.pos[r];
  if(p < 0 || p >= R) return;
  s.order[p] = r;
  s.stgt[p] = s.tgt[r];
}

// ---- list forms: one workgroup per frame.  buf: G [count][3] (vertex lists) | (g_a, g_b) [Pmax][6] | order [Rmax] | stgt [Rmax]
// (the last two copied from the set-up, so that the per-target runs are walked in LDS rather than by dependent global loads)
__device__ inline void list_vjp_body(float * buf, const float * __restrict__ vf, const float * __restrict__ gnf, float * __restrict__ gvf,
                                     const int64_t * __restrict__ ids, int64_t count, int vertex, const int32_t * __restrict__ faces,
                                     const int32_t * __restrict__ adjOff, const int32_t * __restrict__ adjFace, int64_t V,
                                     const ListSetup & s, int64_t Pmax, int accumulate)
{
  const int32_t P = s.hdr[0], R = 3 * P;
  float * pb = buf + (vertex ? 3 * count : 0);
  int32_t * order = reinterpret_cast<int32_t *>(pb + 6 * Pmax);
  int32_t * stgt = order + 3 * Pmax;
  for(int32_t j = threadIdx.x; j < R; j += blockDim.x)
  {
    order[j] = s.order[j];
    stgt[j] = s.stgt[j];
  }
  if(vertex)
  {
    for(int64_t i = threadIdx.x; i < count; i += blockDim.x)
    {
      const int64_t id = ids[i];
      float G[3] = {0.f, 0.f, 0.f};
      if(id >= 0 && id < V) vertex_normal_vjp_dev(vf, faces, adjOff, adjFace, (int)id, gnf + i * 3, G);
      buf[i * 3] = G[0];
      buf[i * 3 + 1] = G[1];
      buf[i * 3 + 2] = G[2];
    }
    __syncthreads();
  }
  for(int32_t p = threadIdx.x; p < P; p += blockDim.x)
  {
    const int32_t i = s.pairId[p], f = s.pairFace[p];
    float gch[3];
    const float * src = vertex ? buf + (int64_t)i * 3 : gnf + (int64_t)i * 3;
    gch[0] = src[0];
    gch[1] = src[1];
    gch[2] = src[2];
    float ga[3], gb[3];
    face_normal_vjp_dev(vf, faces, f, gch, ga, gb);
    for(int x = 0; x < 3; x++)
    {
      pb[p * 6 + x] = ga[x];
      pb[p * 6 + 3 + x] = gb[x];
    }
  }
  __syncthreads();
  for(int32_t j = threadIdx.x; j < R; j += blockDim.x)
  {
    const int32_t t = stgt[j];
    if(j > 0 && stgt[j - 1] == t) continue; // not the first record of its target
    if(t < 0 || t >= V) continue;
    float acc[3] = {0.f, 0.f, 0.f};
    for(int32_t jj = j; jj < R && stgt[jj] == t; jj++)
    {
      const int32_t r = order[jj], p = r / 3, k = r - 3 * p;
      const float * g = pb + p * 6;
      for(int x = 0; x < 3; x++) acc[x] += k == 0 ? -(g[x] + g[3 + x]) : (k == 1 ? g[x] : g[3 + x]);
    }
    float * o = gvf + (int64_t)t * 3;
    if(accumulate)
    {
      acc[0] = o[0] + acc[0];
      acc[1] = o[1] + acc[1];
      acc[2] = o[2] + acc[2];
    }
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
  }
}

__global__ __launch_bounds__(256) void list_vjp_lds_kernel(const float * __restrict__ verts, const float * __restrict__ gn, float * __restrict__ gv,
                                                           const int64_t * __restrict__ ids, int64_t count, int vertex,
                                                           const int32_t * __restrict__ faces, const int32_t * __restrict__ adjOff,
                                                           const int32_t * __restrict__ adjFace, int64_t V, ListSetup s, int64_t Pmax,
                                                           int accumulate)
{
  extern __shared__ float sbuf[];
  const int64_t f = blockIdx.x;
  list_vjp_body(sbuf, verts + f * V * 3, gn + f * count * 3, gv + f * V * 3, ids, count, vertex, faces, adjOff, adjFace, V, s, Pmax,
                accumulate);
}

__global__ __launch_bounds__(256) void list_vjp_ws_kernel(const float * __restrict__ verts, const float * __restrict__ gn, float * __restrict__ gv,
                                                          const int64_t * __restrict__ ids, int64_t count, int vertex,
                                                          const int32_t * __restrict__ faces, const int32_t * __restrict__ adjOff,
                                                          const int32_t * __restrict__ adjFace, int64_t V, ListSetup s, int64_t Pmax,
                                                          int accumulate, float * ws, int64_t ws_floats)
{
  const int64_t f = blockIdx.x;
  list_vjp_body(ws + f * ws_floats, verts + f * V * 3, gn + f * count * 3, gv + f * V * 3, ids, count, vertex, faces, adjOff, adjFace, V, s,
                Pmax, accumulate);
}

static bool staged_forced()
{
  const char * e = getenv("SMPLPP_NORMALS_VJP_STAGED");
  return e && e[0] == '1';
}

static NormalsVjpState * nvjp_state(smplpp_model * m)
{
  if(!m->nvjp)
  {
    NormalsVjpState * s = new NormalsVjpState();
    int md = 0;
    for(int64_t v = 0; v < m->V; v++) md = std::max<int>(md, m->h_adjOff[v + 1] - m->h_adjOff[v]);
    s->maxdeg = md;
    m->nvjp.reset(s);
  }
  return m->nvjp.get();
}

// all pointers on the device; gv already zeroed or holding what is accumulated into
static int mesh_vjp_device(smplpp_model * m, NormalsVjpState * s, int64_t n, const float * verts, const float * gn, float * gv, int accumulate,
                           hipStream_t st)
{
  static PerDeviceOnce once;
  const int64_t V = m->V;
  const int lds = (int)(V * 3 * sizeof(float));
  bool onchip = !staged_forced() && V * 3 * (int64_t)sizeof(float) <= MESH_LDS_MAX && n <= 0x7fffffffLL;
  if(onchip && lds > 64 * 1024 && lds_opt_in(once, m->device, (const void *)mesh_vjp_lds_kernel, lds) != hipSuccess) onchip = false;
  if(onchip)
  {
    mesh_vjp_lds_kernel<<<dim3((unsigned)n), dim3(1024), lds, st>>>(verts, gn, gv, m->faces.get(), m->adjOff.get(), m->adjFace.get(), V,
                                                                     accumulate);
    HIP_TRY(hipGetLastError());
    return SMPLPP_OK;
  }
  HIP_TRY(s->G.reserve(sizeof(float) * (size_t)n * V * 3));
  const unsigned grid = (unsigned)((n * V + 255) / 256);
  mesh_vjp_g_kernel<<<dim3(grid), dim3(256), 0, st>>>(verts, gn, s->G.as<float>(), m->faces.get(), m->adjOff.get(), m->adjFace.get(), V, n);
  HIP_TRY(hipGetLastError());
  mesh_vjp_gather_kernel<<<dim3(grid), dim3(256), 0, st>>>(verts, s->G.as<float>(), gv, m->faces.get(), m->adjOff.get(), m->adjFace.get(), V, n,
                                                           accumulate);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int list_vjp_device(smplpp_model * m, NormalsVjpState * s, int64_t n, const float * verts, int64_t count, const int64_t * ids,
                           const float * gn, float * gv, int accumulate, bool vertex, hipStream_t st)
{
  const int64_t Pmax = vertex ? count * (int64_t)s->maxdeg : count;
  const int64_t Rmax = 3 * Pmax;
  if(Rmax >= 0x7fffffffLL / 4 || (Rmax + 255) / 256 > 65535) return fail(SMPLPP_ERR_INVALID, "normals VJP: id list too long");
  const size_t words = 4 + 2 * (size_t)Pmax + 4 * (size_t)Rmax;
  HIP_TRY(s->setup.reserve(sizeof(int32_t) * words));
  int32_t * w = s->setup.as<int32_t>();
  ListSetup ls{w, w + 4, w + 4 + Pmax, w + 4 + 2 * Pmax, w + 4 + 2 * Pmax + Rmax, w + 4 + 2 * Pmax + 2 * Rmax, w + 4 + 2 * Pmax + 3 * Rmax};
  list_pairs_kernel<<<dim3(1), dim3(256), 0, st>>>(ids, count, vertex ? 1 : 0, m->faces.get(), m->adjOff.get(), m->adjFace.get(), m->V, m->F, ls);
  HIP_TRY(hipGetLastError());
  if(Rmax > 0)
  {
    const unsigned tiles = (unsigned)((Rmax + 255) / 256);
    list_rank_kernel<<<dim3(tiles, tiles), dim3(256), 0, st>>>(ls);
    HIP_TRY(hipGetLastError());
    list_order_kernel<<<dim3(tiles), dim3(256), 0, st>>>(ls, (int32_t)Rmax);
    HIP_TRY(hipGetLastError());
  }
  const int64_t buf_floats = (vertex ? 3 * count : 0) + 6 * Pmax + 2 * Rmax;
  const int64_t bytes = buf_floats * (int64_t)sizeof(float);
  if(bytes <= LIST_LDS_BYTES && !staged_forced())
    list_vjp_lds_kernel<<<dim3((unsigned)n), dim3(256), (unsigned)bytes, st>>>(verts, gn, gv, ids, count, vertex ? 1 : 0, m->faces.get(),
                                                                               m->adjOff.get(), m->adjFace.get(), m->V, ls, Pmax, accumulate);
  else
  {
    HIP_TRY(s->lbuf.reserve(sizeof(float) * (size_t)n * (size_t)buf_floats + 16));
    list_vjp_ws_kernel<<<dim3((unsigned)n), dim3(256), 0, st>>>(verts, gn, gv, ids, count, vertex ? 1 : 0, m->faces.get(), m->adjOff.get(),
                                                                m->adjFace.get(), m->V, ls, Pmax, accumulate, s->lbuf.as<float>(), buf_floats);
  }
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// kind: 0 = face list, 1 = vertex list, 2 = whole mesh
static int normals_vjp_common(const char * fn, smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * ids,
                              const float * grad_normals, float * grad_verts, int accumulate, int space, void * stream, int kind)
{
  const std::string name(fn);
  if(!m || n <= 0 || !verts || !grad_normals || !grad_verts) return fail(SMPLPP_ERR_INVALID, name + ": bad argument");
  if(kind != 2 && (count <= 0 || !ids)) return fail(SMPLPP_ERR_INVALID, name + ": bad argument");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, name + ": accumulate must be 0 or 1");
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, name + ": model has no faces");
  if(n > 0x7fffffffLL || count > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, name + ": too many frames or ids");
  int rc = check_space(space, fn);
  if(rc) return rc;
  if(kind != 2 && space == SMPLPP_HOST && (rc = ids_in(fn, "id", ids, count, 0, kind == 1 ? m->V : m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "normals VJP");
  NormalsVjpState * s = nvjp_state(m);
  const int64_t V = m->V, rows = kind == 2 ? V : count;
  const size_t nv = (size_t)n * V * 3;
  const float * v = fr.in(verts, nv);
  const float * g = fr.in(grad_normals, (size_t)n * rows * 3);
  float * gv = fr.out(grad_verts, nv, accumulate);
  const int64_t * id = fr.in(ids, (size_t)count);
  return fr.run([&]() -> int {
    // a list form writes only the vertices it touches: without accumulate the rest is zeroed first
    if(kind != 2 && !accumulate) HIP_TRY(hipMemsetAsync(gv, 0, sizeof(float) * nv, fr.st));
    return kind == 2 ? mesh_vjp_device(m, s, n, v, g, gv, accumulate, fr.st)
                     : list_vjp_device(m, s, n, v, count, id, g, gv, accumulate, kind == 1, fr.st);
  });
}

extern "C" int smplpp_face_normals_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * face_ids,
                                       const float * grad_normals, float * grad_verts, int accumulate, int space, void * stream)
{
  return normals_vjp_common("smplpp_face_normals_vjp", m, n, verts, count, face_ids, grad_normals, grad_verts, accumulate, space, stream, 0);
}

extern "C" int smplpp_vertex_normals_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * vertex_ids,
                                         const float * grad_normals, float * grad_verts, int accumulate, int space, void * stream)
{
  return normals_vjp_common("smplpp_vertex_normals_vjp", m, n, verts, count, vertex_ids, grad_normals, grad_verts, accumulate, space, stream, 1);
}

extern "C" int smplpp_mesh_vertex_normals_vjp(smplpp_model * m, int64_t n, const float * verts, const float * grad_normals, float * grad_verts,
                                              int accumulate, int space, void * stream)
{
  return normals_vjp_common("smplpp_mesh_vertex_normals_vjp", m, n, verts, 0, nullptr, grad_normals, grad_verts, accumulate, space, stream, 2);
}
