// Silhouette term: the exact Euclidean feature transform of binary images, the two residual sets built on it (model ->
// mask per vertex, mask -> model per pixel) and their vector-Jacobian product to the vertices.  The rule is in include/smplpp_hip.h;
// the transform is all integers, every fp32 operation below is rounded on its own (no contraction to FMA).
//
// Transform (separable; a pixel's candidates are the nearest set pixel of every column, the upper one on a tie):
//  sil_bits_kernel      per (frame, segment of 32 rows, column): the segment's set pixels as one 32-bit word.
//  sil_column_kernel    per (frame, segment, column): the nearest set row above and below the segment from the other segments' words,
//                       then each of its rows from the word's bits (clz / ctz): col [n][H][W] int16, -1 for an empty column.
//  sil_scan             per pixel: the minimum of the key d^2 << 32 | linear index over its row's candidates, walked outwards from the
//                       pixel's own column, both sides at once, until dx^2 exceeds the best d^2 so far (every candidate that can
//                       tie with the minimum is met before that).
//  sil_transform_kernel the public transform: a workgroup stages its rows of `col` in LDS and scans every pixel.
// Residuals: only the pixels that need a nearest feature are scanned, from `col` in global memory: the pixel under each vertex
// (sil_vertex_kernel) and the uncovered mask pixels (sil_pixel_kernel).  The bits are those of the full transform.
// Backward:
//  sil_count_kernel / sil_offsets_kernel / sil_record_kernel   the live pixel records (a cotangent, a source, a face under it)
//                       compacted per frame in pixel order: counts per 256 pixels, the frame's exclusive prefix, the write.
//  record_gather        (distance_vjp.h) each vertex sums its shares in ascending record, then corner.
//  sil_vjp_vertex_kernel per (frame, vertex): that sum, then the vertex's own term added last, then the store.
#include "depth_raster_device.h"
#include "distance_vjp.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int SIL_T = 256;   // threads of every kernel here
constexpr int SIL_SEG = 32;  // rows per segment of the column pass: one bit each
constexpr unsigned long long SIL_NONE = ~0ull;

struct SilRecord
{
  int32_t u[4];   // the source face's vertex ids (-1: no record), pad
  float g[3][3];  // beta_i R^T J^T (2 g r) per corner i
  float pad[3];

  struct Tile
  {
    int4 u[GATHER_TILE];
    float g[GATHER_TILE][9];
  };
  __device__ static bool touches(const int4 & U, int lo, int hi)
  {
    return (U.x >= lo && U.x < hi) || (U.y >= lo && U.y < hi) || (U.z >= lo && U.z < hi);
  }
  __device__ static void stage(Tile & t, int pos, const int4 & U, const SilRecord & r)
  {
    t.u[pos] = U;
    for(int e = 0; e < 9; e++) t.g[pos][e] = r.g[0][e];
  }
  __device__ static void add(float * acc, const Tile & t, int h, int u)
  {
    const int4 U = t.u[h];
    if(U.x == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][x];
    if(U.y == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][3 + x];
    if(U.z == u)
      for(int x = 0; x < 3; x++) acc[x] += t.g[h][6 + x];
  }
};
static_assert(sizeof(SilRecord) == 64, "SilRecord: four 16-byte loads");

struct SilhouetteState
{
  DevBuf bits;            // [n][segments][W] uint32: the set rows of a segment of one column
  DevBuf colm, colc;      // [n][H][W] int16: the column pass of the mask and of the coverage
  DevBuf cnt, off, nvalid; // [n][blocks] int32 live records per 256 pixels, their exclusive prefix; [n] int64 records per frame
  DevBuf rec;             // [n][H W] SilRecord, the first nvalid[frame] of a frame live
  DevBuf gpix;            // [n][V][3] the pixel term's sums
};
void StateDelete::operator()(SilhouetteState * s) const
{
  delete s;
}

template<class T>
__device__ inline bool sil_set(T v);
template<>
__device__ inline bool sil_set<uint8_t>(uint8_t v)
{
  return v != 0;
}
template<>
__device__ inline bool sil_set<int64_t>(int64_t v) // a face image: coverage
{
  return v >= 0;
}

// idx = (frame * nseg + seg) * W + column
template<class T>
__global__ __launch_bounds__(SIL_T) void sil_bits_kernel(const T * __restrict__ img, uint32_t * __restrict__ bits, int64_t H, int64_t W,
                                                         int64_t nseg, int64_t total)
{
  const int64_t idx = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if(idx >= total) return;
  const int64_t i = idx % W, seg = (idx / W) % nseg, frame = idx / (W * nseg);
  const int64_t j0 = seg * SIL_SEG;
  const int rows = (int)(H - j0 < SIL_SEG ? H - j0 : SIL_SEG);
  const T * p = img + (frame * H + j0) * W + i;
  uint32_t b = 0;
#pragma unroll 8
  for(int k = 0; k < rows; k++) b |= sil_set<T>(p[(int64_t)k * W]) ? 1u << k : 0u;
  bits[idx] = b;
}

__global__ __launch_bounds__(SIL_T) void sil_column_kernel(const uint32_t * __restrict__ bits, int16_t * __restrict__ col, int64_t H,
                                                           int64_t W, int64_t nseg, int64_t total)
{
  const int64_t idx = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if(idx >= total) return;
  const int64_t i = idx % W, seg = (idx / W) % nseg, frame = idx / (W * nseg);
  const uint32_t * bf = bits + frame * nseg * W + i;
  int up_in = -1, dn_in = -1; // the nearest set row above and below the segment
  for(int64_t s = seg - 1; s >= 0; s--)
  {
    const uint32_t b = bf[s * W];
    if(b)
    {
      up_in = (int)(s * SIL_SEG) + 31 - __clz((int)b);
      break;
    }
  }
  for(int64_t s = seg + 1; s < nseg; s++)
  {
    const uint32_t b = bf[s * W];
    if(b)
    {
      dn_in = (int)(s * SIL_SEG) + __ffs((int)b) - 1;
      break;
    }
  }
  const uint32_t b = bf[seg * W];
  const int j0 = (int)(seg * SIL_SEG);
  const int rows = (int)(H - j0 < SIL_SEG ? H - j0 : SIL_SEG);
  int16_t * c = col + (frame * H + j0) * W + i;
  for(int k = 0; k < rows; k++)
  {
    const int j = j0 + k;
    const uint32_t lo = b & ((2u << k) - 1u), hi = b >> k; // rows <= j, rows >= j of the segment
    const int up = lo ? j0 + 31 - __clz((int)lo) : up_in;
    const int dn = hi ? j + __ffs((int)hi) - 1 : dn_in;
    // the nearer of the two, the upper one on a tie
    c[(int64_t)k * W] = (int16_t)(up < 0 ? dn : (dn >= 0 && dn - j < j - up) ? dn : up);
  }
}

// the minimum key of pixel (row j, column i) over its row's candidates: row[i'] = the candidate's row in column i', -1 = none
__device__ inline unsigned long long sil_scan(const int16_t * row, int W, int j, int i)
{
  unsigned long long best = SIL_NONE;
  auto candidate = [&](int ii) {
    const int r = row[ii];
    if(r < 0) return;
    const int dy = j - r, dx = i - ii;
    const unsigned long long key = ((unsigned long long)(unsigned)(dx * dx + dy * dy) << 32) | (unsigned)(r * W + ii);
    best = key < best ? key : best;
  };
  candidate(i);
  for(int dx = 1;; dx++)
  {
    const bool left = i - dx >= 0, right = i + dx < W;
    if(!left && !right) break;
    if((unsigned long long)(dx * dx) > (best >> 32)) break; // (no candidate yet: 2^32 - 1, above every dx^2 of an image)
    if(left) candidate(i - dx);
    if(right) candidate(i + dx);
  }
  return best;
}

// a workgroup takes `rpb` rows of one frame (rpb W <= max(W, SIL_T)); bpf workgroups per frame
__global__ __launch_bounds__(SIL_T) void sil_transform_kernel(const int16_t * __restrict__ col, int64_t * __restrict__ nearest,
                                                              int32_t * __restrict__ sqdist, int64_t H, int64_t W, int rpb, int64_t bpf)
{
  __shared__ int16_t s_row[DR_MAX_SIDE];
  const int64_t frame = blockIdx.x / bpf, jb = (blockIdx.x % bpf) * rpb;
  const int rows = (int)(H - jb < rpb ? H - jb : rpb);
  const int cnt = rows * (int)W;
  const int16_t * src = col + (frame * H + jb) * W;
  for(int e = threadIdx.x; e < cnt; e += SIL_T) s_row[e] = src[e];
  __syncthreads();
  for(int e = threadIdx.x; e < cnt; e += SIL_T)
  {
    const int r = e / (int)W, i = e % (int)W;
    const unsigned long long key = sil_scan(s_row + r * (int)W, (int)W, (int)jb + r, i);
    const int64_t o = (frame * H + jb) * W + e;
    if(nearest) nearest[o] = key == SIL_NONE ? -1 : (int64_t)(key & 0xffffffffull);
    if(sqdist) sqdist[o] = key == SIL_NONE ? 0 : (int32_t)(key >> 32);
  }
}

__global__ __launch_bounds__(SIL_T) void sil_vertex_kernel(const float * __restrict__ verts, const float * __restrict__ camera,
                                                           const uint8_t * __restrict__ mask, const int16_t * __restrict__ colm,
                                                           int64_t * __restrict__ vt, float * __restrict__ vsq, float near, int64_t H,
                                                           int64_t W, int64_t V, int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if(idx >= nv) return;
  const int64_t frame = idx / V;
  const DrCamera c = dr_camera(camera, frame);
  float xc[3], u, v, su, sv;
  int64_t target = -1;
  float sq = 0.0f;
  if(dr_project(c, verts[idx * 3], verts[idx * 3 + 1], verts[idx * 3 + 2], near, xc, u, v, su, sv))
  {
    // (|u|, |v| <= 32768 + 1/512 here: the casts are exact)
    int i = (int)floorf(u), j = (int)floorf(v);
    i = i < 0 ? 0 : i > (int)W - 1 ? (int)W - 1 : i;
    j = j < 0 ? 0 : j > (int)H - 1 ? (int)H - 1 : j;
    const int64_t row = (frame * H + j) * W;
    if(mask[row + i] == 0)
    {
      const unsigned long long key = sil_scan(colm + row, (int)W, j, i);
      if(key != SIL_NONE)
      {
        target = (int64_t)(key & 0xffffffffull);
        const float rx = u - ((float)(int)(target % W) + 0.5f), ry = v - ((float)(int)(target / W) + 0.5f);
        sq = rx * rx + ry * ry;
      }
    }
  }
  if(vt) vt[idx] = target;
  if(vsq) vsq[idx] = sq;
}

__global__ __launch_bounds__(SIL_T) void sil_pixel_kernel(const uint8_t * __restrict__ mask, const int64_t * __restrict__ face,
                                                          const int16_t * __restrict__ colc, int64_t * __restrict__ ps,
                                                          float * __restrict__ psq, int64_t H, int64_t W, int64_t np)
{
  const int64_t idx = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if(idx >= np) return;
  int64_t source = -1;
  float sq = 0.0f;
  if(mask[idx] != 0 && face[idx] < 0)
  {
    const int64_t pix = idx % (H * W);
    const int j = (int)(pix / W), i = (int)(pix % W);
    const unsigned long long key = sil_scan(colc + (idx - i), (int)W, j, i);
    if(key != SIL_NONE)
    {
      source = (int64_t)(key & 0xffffffffull);
      sq = (float)(int32_t)(key >> 32);
    }
  }
  if(ps) ps[idx] = source;
  if(psq) psq[idx] = sq;
}

// ---- backward
// J^T k for the projection (fx x / z + cx, fy y / z + cy) at the camera-space point x, then R^T: the world-space vector
__device__ inline void sil_pull(const DrCamera & c, const float * x, float kx, float ky, float * w)
{
  const float jx = (c.fx * kx) / x[2], jy = (c.fy * ky) / x[2];
  const float jz = -((jx * x[0] + jy * x[1]) / x[2]);
  for(int a = 0; a < 3; a++) w[a] = (c.R[a] * jx + c.R[3 + a] * jy) + c.R[6 + a] * jz;
}

// pixel q of the frame carries a record: a nonzero cotangent, a source s inside the image, a face of the model under s
__device__ inline bool sil_live(const int64_t * __restrict__ ps, const float * __restrict__ gps, const int64_t * __restrict__ face,
                                int64_t frame, int64_t q, int64_t HW, int64_t F, int64_t & s, int64_t & f)
{
  if(q >= HW) return false;
  const int64_t idx = frame * HW + q;
  if(gps[idx] == 0.0f) return false;
  s = ps[idx];
  if(s < 0 || s >= HW) return false;
  f = face[frame * HW + s];
  return f >= 0 && f < F;
}

// grid: n * nb workgroups, 256 pixels each
__global__ __launch_bounds__(SIL_T) void sil_count_kernel(const int64_t * __restrict__ ps, const float * __restrict__ gps,
                                                          const int64_t * __restrict__ face, int32_t * __restrict__ cnt, int64_t HW,
                                                          int64_t F, int64_t nb)
{
  __shared__ int s_c[SIL_T / 64];
  const int64_t frame = blockIdx.x / nb, q = (blockIdx.x % nb) * SIL_T + threadIdx.x;
  int64_t s, f;
  const uint64_t m = __ballot(sil_live(ps, gps, face, frame, q, HW, F, s, f));
  if((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = (int)__popcll(m);
  __syncthreads();
  if(threadIdx.x == 0)
  {
    int t = 0;
    for(int w = 0; w < SIL_T / 64; w++) t += s_c[w];
    cnt[blockIdx.x] = t;
  }
}

// per frame: off = exclusive prefix of cnt in pixel order, nvalid = the total
__global__ __launch_bounds__(SIL_T) void sil_offsets_kernel(const int32_t * __restrict__ cnt, int32_t * __restrict__ off,
                                                            int64_t * __restrict__ nvalid, int64_t nb)
{
  __shared__ int s_w[SIL_T / 64];
  const int64_t frame = blockIdx.x;
  const int32_t * c = cnt + frame * nb;
  int32_t * o = off + frame * nb;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t per = (nb + SIL_T - 1) / SIL_T;
  const int64_t b = t * per < nb ? t * per : nb, e = b + per < nb ? b + per : nb;
  int sum = 0;
  for(int64_t k = b; k < e; k++) sum += c[k];
  int inc = sum; // inclusive scan over the wavefront
  for(int d = 1; d < 64; d <<= 1)
  {
    const int y = __shfl_up(inc, d);
    if(lane >= d) inc += y;
  }
  if(lane == 63) s_w[wave] = inc;
  __syncthreads();
  int run = inc - sum;
  for(int w = 0; w < wave; w++) run += s_w[w];
  for(int64_t k = b; k < e; k++)
  {
    o[k] = run;
    run += c[k];
  }
  if(t == SIL_T - 1) nvalid[frame] = run;
}

__global__ __launch_bounds__(SIL_T) void sil_record_kernel(const float * __restrict__ verts, const float * __restrict__ camera,
                                                           const int32_t * __restrict__ faces, const int64_t * __restrict__ face,
                                                           const int64_t * __restrict__ ps, const float * __restrict__ gps,
                                                           const int32_t * __restrict__ off, SilRecord * __restrict__ rec, int64_t H,
                                                           int64_t W, int64_t V, int64_t F, int64_t nb)
{
  __shared__ int s_c[SIL_T / 64];
  const int64_t HW = H * W;
  const int64_t frame = blockIdx.x / nb, q = (blockIdx.x % nb) * SIL_T + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t s = 0, f = 0;
  const bool live = sil_live(ps, gps, face, frame, q, HW, F, s, f);
  const uint64_t m = __ballot(live);
  if(lane == 0) s_c[wave] = (int)__popcll(m);
  __syncthreads();
  if(!live) return;
  int pos = off[blockIdx.x] + (int)__popcll(m & ((1ull << lane) - 1ull));
  for(int w = 0; w < wave; w++) pos += s_c[w];
  const DrCamera c = dr_camera(camera, frame);
  SilRecord r;
  float x[3][3];
  for(int k = 0; k < 3; k++)
  {
    r.u[k] = faces[f * 3 + k];
    const float * p = verts + (frame * V + r.u[k]) * 3;
    dr_to_camera(c, p[0], p[1], p[2], x[k]);
  }
  r.u[3] = -1;
  DrFace t;
  dr_plane(t, x[0], x[1], x[2]);
  const int is = (int)(s % W), js = (int)(s / W), iq = (int)(q % W), jq = (int)(q / W);
  float dx, dy, beta[3], y[3], w[3];
  dr_ray(c, is, js, dx, dy);
  const float nd = (t.nx * dx + t.ny * dy) + t.nz;
  const float depth = t.na / nd;
  dr_bary(t, depth, dx, dy, beta[0], beta[1], beta[2]);
  y[0] = depth * dx, y[1] = depth * dy, y[2] = depth;
  const float g2 = 2.0f * gps[frame * HW + q];
  sil_pull(c, y, g2 * (float)(is - iq), g2 * (float)(js - jq), w);
  for(int k = 0; k < 3; k++)
    for(int a = 0; a < 3; a++) r.g[k][a] = beta[k] * w[a];
  r.pad[0] = r.pad[1] = r.pad[2] = 0.0f;
  rec[frame * HW + pos] = r;
}

__global__ __launch_bounds__(SIL_T) void sil_vjp_vertex_kernel(const float * __restrict__ verts, const float * __restrict__ camera,
                                                               const int64_t * __restrict__ vt, const float * __restrict__ gvs,
                                                               const float * __restrict__ gpix, float * __restrict__ gv, int accumulate,
                                                               float near, int64_t H, int64_t W, int64_t V, int64_t nv)
{
  const int64_t idx = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if(idx >= nv) return;
  float w[3] = {0.0f, 0.0f, 0.0f};
  if(gvs)
  {
    const float g = gvs[idx];
    const int64_t t = vt[idx];
    if(g != 0.0f && t >= 0 && t < H * W)
    {
      const DrCamera c = dr_camera(camera, idx / V);
      float xc[3], u, v, su, sv;
      if(dr_project(c, verts[idx * 3], verts[idx * 3 + 1], verts[idx * 3 + 2], near, xc, u, v, su, sv))
      {
        const float rx = u - ((float)(int)(t % W) + 0.5f), ry = v - ((float)(int)(t / W) + 0.5f);
        const float g2 = 2.0f * g;
        sil_pull(c, xc, g2 * rx, g2 * ry, w);
      }
    }
  }
  float * o = gv + idx * 3;
  for(int a = 0; a < 3; a++)
  {
    const float sum = gpix ? gpix[idx * 3 + a] + w[a] : w[a];
    o[a] = accumulate ? o[a] + sum : sum;
  }
}

static SilhouetteState * sil_state(smplpp_model * m)
{
  if(!m->sil) m->sil.reset(new SilhouetteState());
  return m->sil.get();
}

static unsigned sil_grid(int64_t items)
{
  return (unsigned)((items + SIL_T - 1) / SIL_T);
}

// the column pass of n images (set: a nonzero byte, or a face id >= 0) into col [n][H][W]
template<class T>
static int sil_columns(SilhouetteState * s, int64_t n, const T * img, int64_t H, int64_t W, DevBuf & col, hipStream_t st)
{
  const int64_t nseg = (H + SIL_SEG - 1) / SIL_SEG, total = n * nseg * W;
  HIP_TRY(s->bits.reserve(sizeof(uint32_t) * (size_t)total));
  HIP_TRY(col.reserve(sizeof(int16_t) * (size_t)(n * H * W)));
  sil_bits_kernel<T><<<dim3(sil_grid(total)), dim3(SIL_T), 0, st>>>(img, s->bits.as<uint32_t>(), H, W, nseg, total);
  HIP_TRY(hipGetLastError());
  sil_column_kernel<<<dim3(sil_grid(total)), dim3(SIL_T), 0, st>>>(s->bits.as<uint32_t>(), col.as<int16_t>(), H, W, nseg, total);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

// all pointers on the device
static int sil_transform_device(SilhouetteState * s, int64_t n, const uint8_t * mask, int64_t H, int64_t W, int64_t * nearest,
                                int32_t * sqdist, hipStream_t st)
{
  int rc = sil_columns(s, n, mask, H, W, s->colm, st);
  if(rc) return rc;
  const int rpb = W >= SIL_T ? 1 : (int)std::min<int64_t>(H, SIL_T / W);
  const int64_t bpf = (H + rpb - 1) / rpb;
  sil_transform_kernel<<<dim3((unsigned)(n * bpf)), dim3(SIL_T), 0, st>>>(s->colm.as<int16_t>(), nearest, sqdist, H, W, rpb, bpf);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

static int sil_forward_device(smplpp_model * m, SilhouetteState * s, int64_t n, const float * verts, const float * camera, int64_t H,
                              int64_t W, float near, const int64_t * face, const uint8_t * mask, int64_t * vt, float * vsq, int64_t * ps,
                              float * psq, hipStream_t st)
{
  if(vt || vsq)
  {
    int rc = sil_columns(s, n, mask, H, W, s->colm, st);
    if(rc) return rc;
    sil_vertex_kernel<<<dim3(sil_grid(n * m->V)), dim3(SIL_T), 0, st>>>(verts, camera, mask, s->colm.as<int16_t>(), vt, vsq, near, H, W, m->V,
                                                                        n * m->V);
    HIP_TRY(hipGetLastError());
  }
  if(ps || psq)
  {
    int rc = sil_columns(s, n, face, H, W, s->colc, st);
    if(rc) return rc;
    sil_pixel_kernel<<<dim3(sil_grid(n * H * W)), dim3(SIL_T), 0, st>>>(mask, face, s->colc.as<int16_t>(), ps, psq, H, W, n * H * W);
    HIP_TRY(hipGetLastError());
  }
  return SMPLPP_OK;
}

static int sil_vjp_device(smplpp_model * m, SilhouetteState * s, int64_t n, const float * verts, const float * camera, int64_t H,
                          int64_t W, float near, const int64_t * face, const int64_t * vt, const int64_t * ps, const float * gvs,
                          const float * gps, float * gv, int accumulate, hipStream_t st)
{
  const int64_t V = m->V, HW = H * W, nb = (HW + SIL_T - 1) / SIL_T;
  if(gps)
  {
    HIP_TRY(s->cnt.reserve(sizeof(int32_t) * (size_t)(n * nb)));
    HIP_TRY(s->off.reserve(sizeof(int32_t) * (size_t)(n * nb)));
    HIP_TRY(s->nvalid.reserve(sizeof(int64_t) * (size_t)n));
    HIP_TRY(s->rec.reserve(sizeof(SilRecord) * (size_t)(n * HW)));
    HIP_TRY(s->gpix.reserve(sizeof(float) * 3 * (size_t)(n * V)));
    sil_count_kernel<<<dim3((unsigned)(n * nb)), dim3(SIL_T), 0, st>>>(ps, gps, face, s->cnt.as<int32_t>(), HW, m->F, nb);
    HIP_TRY(hipGetLastError());
    sil_offsets_kernel<<<dim3((unsigned)n), dim3(SIL_T), 0, st>>>(s->cnt.as<int32_t>(), s->off.as<int32_t>(), s->nvalid.as<int64_t>(), nb);
    HIP_TRY(hipGetLastError());
    sil_record_kernel<<<dim3((unsigned)(n * nb)), dim3(SIL_T), 0, st>>>(verts, camera, m->faces.get(), face, ps, gps, s->off.as<int32_t>(),
                                                                        s->rec.as<SilRecord>(), H, W, V, m->F, nb);
    HIP_TRY(hipGetLastError());
    int rc = record_gather(s->rec.as<SilRecord>(), s->gpix.as<float>(), 0, n, HW, V, st, s->nvalid.as<int64_t>());
    if(rc) return rc;
  }
  sil_vjp_vertex_kernel<<<dim3(sil_grid(n * V)), dim3(SIL_T), 0, st>>>(verts, camera, vt, gvs, gps ? s->gpix.as<float>() : nullptr, gv,
                                                                      accumulate, near, H, W, V, n * V);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_mask_distance_transform(smplpp_model * m, int64_t n, const uint8_t * mask, int64_t H, int64_t W, int64_t * nearest,
                                              int32_t * sqdist, int space, void * stream)
{
  const char * fn = "smplpp_mask_distance_transform";
  if(!m || n <= 0 || !mask || (!nearest && !sqdist)) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(H < 1 || W < 1 || H > DR_MAX_SIDE || W > DR_MAX_SIDE) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": H and W must be in [1, 8192]");
  if(n > 0x7fffffffLL || n * H * W > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * H * W beyond int32 indexing");
  int rc = check_space(space, fn);
  if(rc) return rc;
  Frame fr(m->device, &m->arena, space, stream, "mask distance transform");
  SilhouetteState * s = sil_state(m);
  const uint8_t * mk = fr.in(mask, (size_t)(n * H * W));
  int64_t * no = fr.out(nearest, (size_t)(n * H * W));
  int32_t * so = fr.out(sqdist, (size_t)(n * H * W));
  return fr.run([&] { return sil_transform_device(s, n, mk, H, W, no, so, fr.st); });
}

extern "C" int smplpp_silhouette(smplpp_model * m, int64_t n, const float * verts, const float * camera, int64_t H, int64_t W, float near,
                                 const int64_t * face, const uint8_t * mask, int64_t * vert_target, float * vert_sq, int64_t * pix_source,
                                 float * pix_sq, int space, void * stream)
{
  const char * fn = "smplpp_silhouette";
  if(!m || n <= 0 || !verts || !camera || !face || !mask || (!vert_target && !vert_sq && !pix_source && !pix_sq))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(int rc = dr_check_near(fn, near)) return rc;
  int rc = dr_check(fn, m, n, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST && (rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
  Frame fr(m->device, &m->arena, space, stream, "silhouette");
  SilhouetteState * s = sil_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const int64_t * f = fr.in(face, (size_t)(n * H * W));
  const uint8_t * mk = fr.in(mask, (size_t)(n * H * W));
  int64_t * vt = fr.out(vert_target, (size_t)(n * m->V));
  float * vs = fr.out(vert_sq, (size_t)(n * m->V));
  int64_t * ps = fr.out(pix_source, (size_t)(n * H * W));
  float * pq = fr.out(pix_sq, (size_t)(n * H * W));
  return fr.run([&] { return sil_forward_device(m, s, n, v, c, H, W, near, f, mk, vt, vs, ps, pq, fr.st); });
}

extern "C" int smplpp_silhouette_vjp(smplpp_model * m, int64_t n, const float * verts, const float * camera, int64_t H, int64_t W,
                                     float near, const int64_t * face, const int64_t * vert_target, const int64_t * pix_source,
                                     const float * grad_vert_sq, const float * grad_pix_sq, float * grad_verts, int accumulate, int space,
                                     void * stream)
{
  const char * fn = "smplpp_silhouette_vjp";
  if(!m || n <= 0 || !verts || !camera || !face || !grad_verts || (!grad_vert_sq && !grad_pix_sq) || (grad_vert_sq && !vert_target) ||
     (grad_pix_sq && !pix_source))
    return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": bad argument");
  if(int rc = dr_check_near(fn, near)) return rc;
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  int rc = dr_check(fn, m, n, H, W, space);
  if(rc) return rc;
  if(space == SMPLPP_HOST)
  {
    if((rc = ids_in(fn, "face id", face, n * H * W, -1, m->F))) return rc;
    if(grad_vert_sq && (rc = ids_in(fn, "vert_target", vert_target, n * m->V, -1, H * W))) return rc;
    if(grad_pix_sq && (rc = ids_in(fn, "pix_source", pix_source, n * H * W, -1, H * W))) return rc;
  }
  Frame fr(m->device, &m->arena, space, stream, "silhouette VJP");
  SilhouetteState * s = sil_state(m);
  const float * v = fr.in(verts, (size_t)n * m->V * 3);
  const float * c = fr.in(camera, (size_t)n * 16);
  const int64_t * f = fr.in(face, (size_t)(n * H * W));
  // a term without its gradient is left out: its indices are not read
  const int64_t * vt = grad_vert_sq ? fr.in(vert_target, (size_t)(n * m->V)) : nullptr;
  const float * gs = fr.in(grad_vert_sq, (size_t)(n * m->V));
  const int64_t * ps = grad_pix_sq ? fr.in(pix_source, (size_t)(n * H * W)) : nullptr;
  const float * gp = fr.in(grad_pix_sq, (size_t)(n * H * W));
  float * gv = fr.out(grad_verts, (size_t)n * m->V * 3, accumulate);
  return fr.run([&] { return sil_vjp_device(m, s, n, v, c, H, W, near, f, vt, ps, gs, gp, gv, accumulate, fr.st); });
}
