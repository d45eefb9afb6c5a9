// The image term: a dense channels-last image [B,H,W,C] sampled at projected points uv [n,K,2] by bilinear interpolation,
// a robust squared residual against a target, and the vector-Jacobian product to the points AND to the image.  The rules are in
// include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to FMA), the frame energy is one fixed-order sum
// (sum1024 of fixed_sum.h, whose two facts about +0 let the work split follow K), and there are no floating-point atomics: grad_image
// is a gather, one fixed-order sum per image element in ascending point index.  The calls take no handle.
//
//  img_sample_kernel<V>     a thread per point: value, gradient, valid.
//  img_points_kernel<V>     the term without the frame energy: a thread per point.
//  img_small_kernel<V>      K <= 64: a wavefront per frame, lane k owns point k (partial k; the partials past 63 are +0).
//  img_wide_kernel<V, NQ>   K > 64: a workgroup per frame, of 256 or 1024 threads by frame_sum_split: thread t owns the partials t + T q.
//  img_vjp_uv_kernel<V>     a thread per point: it samples again by the forward's device function, so the bits match; no sums across points.
//  img_vjp_image_kernel<V>  a workgroup per (image, 16 x 16 pixel tile, 4 channels), a thread per pixel: the points that read the image
//                           pass through it in point order, IMG_LIST at a time, their uv read one pass ahead; those whose cell touches the tile are compacted in that
//                           order into LDS (__ballot / __popcll, then a prefix over rows and wavefronts, as record_gather_kernel of
//                           distance_vjp.h does) with their four cotangents, and every thread adds its pixel's share of each in list
//                           order.  The add is branch-free: +0 for another pixel's tap leaves the bits (the sum starts at +0, and a
//                           sum is -0 only if both terms are).  The cost grows with tiles x points.
// V is the number of channels a thread reads at once: 4 (16-byte reads) when C % 4 == 0, the image is 16-byte aligned and there is no
// `channel`, else 1.  A thread holds its point's channels in ascending order either way, so no bit depends on V.
#include "fixed_sum.h"
#include "staging.h"

#pragma clang fp contract(off)

namespace smplpp_hip
{
constexpr int IMG_T = 256; // threads of every kernel here (the wide forward above K = 1024 takes 1024)
constexpr int IMG_WAVES = IMG_T / 64;
constexpr int64_t IMG_INT32_MAX = 0x7fffffffLL;
constexpr int IMG_TILE = 16;              // grad_image: pixels a side of a workgroup's tile (IMG_TILE^2 == IMG_T)
constexpr int IMG_GC = 4;                 // grad_image: channels of a workgroup
constexpr int IMG_GR = 2;                 // grad_image: points per thread per pass
constexpr int IMG_LIST = IMG_T * IMG_GR;  // grad_image: points per pass
static_assert(IMG_TILE * IMG_TILE == IMG_T, "a thread per pixel of the tile");

// what the three calls read
struct ImgArgs
{
  const float *uv, *image;
  const int64_t * channel;
  const float *target, *weight;
  int K, H, W, C, Cs;
  int image_per_frame, target_per_frame, weight_per_frame; // 0: shared by all frames (B, Tn, Wn = 1)
  float rho;
};
// the term's per-point outputs
struct ImgOut
{
  float *point_energy, *value;
  uint8_t * valid;
};
// the cotangents of energy [n], point_energy [n,K] and value [n,K,Cs]; each may be null
struct ImgCot
{
  const float *ge, *gpe, *gv;
};

// two adjacent floats at any 4-byte-aligned address, read as one 8-byte access
struct __attribute__((packed, aligned(4))) ImgPair
{
  float x, y;
};

// where point (f, k) falls: its cell (i, j), the fractions, the first sampled channel c and the address p of pixel (j, i), channel c
struct ImgCell
{
  const float * p;
  int i, j, c;
  float fx, fy;
  bool inside;
};

// The coordinate, inside and cell steps of the sampling rule on (u, v) alone: c and p are not set
__device__ inline ImgCell img_cell_at(const ImgArgs & a, float u, float v)
{
  ImgCell r{nullptr, 0, 0, 0, 0.0f, 0.0f, false};
  const float gx = u - 0.5f, gy = v - 0.5f;
  // (a NaN fails every comparison, an infinity one of them)
  if(!(gx >= 0.0f && gx <= (float)(a.W - 1) && gy >= 0.0f && gy <= (float)(a.H - 1))) return r;
  r.i = min((int)floorf(gx), a.W - 2), r.j = min((int)floorf(gy), a.H - 2);
  r.fx = gx - (float)r.i, r.fy = gy - (float)r.j;
  r.inside = true;
  return r;
}

// The channel and the address of an inside cell of point (f, k).  A device-space channel outside [0, C) makes the point not inside.
__device__ inline void img_cell_bind(const ImgArgs & a, int f, int k, ImgCell & r)
{
  if(a.channel)
  {
    const int64_t ch = a.channel[k];
    r.inside = ch >= 0 && ch < a.C;
    r.c = r.inside ? (int)ch : 0;
  }
  r.p = a.image + ((((a.image_per_frame ? f : 0) * a.H + r.j) * a.W + r.i) * a.C + r.c);
}

__device__ inline ImgCell img_cell(const ImgArgs & a, int f, int k)
{
  const ImgPair t = *reinterpret_cast<const ImgPair *>(a.uv + 2 * (f * a.K + k));
  ImgCell r = img_cell_at(a, t.x, t.y);
  if(r.inside) img_cell_bind(a, f, k, r);
  return r;
}

// The value and gradient steps for the sampled channels [lo, hi) of a cell, in ascending order: fn(c, s, ds/du, ds/dv).  With V = 4,
// lo and hi are multiples of 4.
template<int V, class Fn>
__device__ inline void img_channels(const ImgArgs & a, const ImgCell & q, int lo, int hi, Fn fn)
{
  const int sx = a.C, sy = a.W * a.C;
  for(int c = lo; c < hi; c += V)
  {
    float v[4][V]; // the taps (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1)
    if constexpr(V == 4)
    {
#pragma unroll
      for(int u = 0; u < 4; u++)
      {
        const float4 x = *reinterpret_cast<const float4 *>(q.p + c + (u & 1) * sx + (u >> 1) * sy);
        v[u][0] = x.x, v[u][1] = x.y, v[u][2] = x.z, v[u][3] = x.w;
      }
    }
    else
    {
#pragma unroll
      for(int u = 0; u < 4; u++) v[u][0] = q.p[c + (u & 1) * sx + (u >> 1) * sy];
    }
#pragma unroll
    for(int e = 0; e < V; e++)
    {
      const float d0 = v[1][e] - v[0][e], d1 = v[3][e] - v[2][e];
      const float c0 = v[0][e] + q.fx * d0, c1 = v[2][e] + q.fx * d1;
      const float ey = c1 - c0;
      const float s = c0 + q.fy * ey;
      fn(c + e, s, d0 + q.fy * (d1 - d0), ey);
    }
  }
}

// the Geman-McClure form of smplpp_project_points on q = sum_c r_c r_c
__device__ inline float img_energy(float w, float q, float rho)
{
  if(rho == 0.0f) return w * q;
  const float p2 = rho * rho;
  return w * ((p2 * q) / (p2 + q));
}

// point (f, k) of the term: writes its per-point outputs, returns its energy
template<int V>
__device__ inline float img_point(const ImgArgs & a, const ImgOut & o, int f, int k)
{
  const int p = f * a.K + k;
  const float w = a.weight ? a.weight[a.weight_per_frame ? p : k] : 1.0f;
  const bool live = w != 0.0f;
  float e = 0.0f;
  if(live || o.value || o.valid)
  {
    const ImgCell q = img_cell(a, f, k);
    float * val = o.value ? o.value + p * a.Cs : nullptr;
    bool ok = q.inside;
    float qq = 0.0f;
    if(ok)
    {
      const float * t = live && a.target ? a.target + (a.target_per_frame ? p : k) * a.Cs : nullptr;
      img_channels<V>(a, q, 0, a.Cs, [&](int c, float s, float, float) {
        ok = ok && fabsf(s) < INFINITY;
        if(val) val[c] = s;
        if(live)
        {
          const float r = t ? s - t[c] : s;
          qq = qq + r * r;
        }
      });
    }
    if(!ok && val)
      for(int c = 0; c < a.Cs; c++) val[c] = 0.0f;
    if(o.valid) o.valid[p] = ok ? 1 : 0;
    if(live && ok) e = img_energy(w, qq, a.rho);
  }
  if(o.point_energy) o.point_energy[p] = e;
  return e;
}

// The backward rule at point (f, k), whose cell is q (inside): fn(c, gamma_c, ds_c/du, ds_c/dv) for the sampled channels [lo, hi) in
// ascending order.  false, and no call of fn, when the point contributes nothing: it is not valid, or its weight is 0 under a null
// grad_value (then it reads no image value).
template<int V, class Fn>
__device__ inline bool img_point_vjp(const ImgArgs & a, const ImgCot & g, int f, int k, const ImgCell & q, int lo, int hi, Fn fn)
{
  const int p = f * a.K + k;
  const float w = a.weight ? a.weight[a.weight_per_frame ? p : k] : 1.0f;
  const bool live = w != 0.0f;
  if(!live && !g.gv) return false;
  const float * t = live && a.target ? a.target + (a.target_per_frame ? p : k) * a.Cs : nullptr;
  bool ok = true;
  float qq = 0.0f;
  img_channels<V>(a, q, 0, a.Cs, [&](int c, float s, float, float) {
    ok = ok && fabsf(s) < INFINITY;
    if(live)
    {
      const float r = t ? s - t[c] : s;
      qq = qq + r * r;
    }
  });
  if(!ok) return false;
  float coef = 0.0f;
  if(live)
  {
    const float gg = (g.ge ? g.ge[f] : 0.0f) + (g.gpe ? g.gpe[p] : 0.0f);
    float m = w;
    if(a.rho != 0.0f)
    {
      const float p2 = a.rho * a.rho, d = p2 / (p2 + qq);
      m = w * (d * d);
    }
    coef = (2.0f * gg) * m;
  }
  const float * gv = g.gv ? g.gv + p * a.Cs : nullptr;
  img_channels<V>(a, q, lo, hi, [&](int c, float s, float du, float dv) {
    const float r = t ? s - t[c] : s;
    fn(c, (gv ? gv[c] : 0.0f) + (live ? coef * r : 0.0f), du, dv);
  });
  return true;
}

// grid: ceil(n K / IMG_T)
template<int V>
__global__ __launch_bounds__(IMG_T) void img_sample_kernel(ImgArgs a, int total, float * __restrict__ value, float * __restrict__ gradient,
                                                           uint8_t * __restrict__ valid)
{
  const int p = blockIdx.x * IMG_T + threadIdx.x;
  if(p >= total) return;
  const ImgCell q = img_cell(a, p / a.K, p % a.K);
  float * val = value ? value + p * a.Cs : nullptr;
  float * grd = gradient ? gradient + 2 * (p * a.Cs) : nullptr;
  bool ok = q.inside;
  if(ok)
    img_channels<V>(a, q, 0, a.Cs, [&](int c, float s, float du, float dv) {
      ok = ok && fabsf(s) < INFINITY;
      if(val) val[c] = s;
      if(grd) grd[2 * c] = du, grd[2 * c + 1] = dv;
    });
  if(!ok)
    for(int c = 0; c < a.Cs; c++)
    {
      if(val) val[c] = 0.0f;
      if(grd) grd[2 * c] = 0.0f, grd[2 * c + 1] = 0.0f;
    }
  if(valid) valid[p] = ok ? 1 : 0;
}

// grid: ceil(n K / IMG_T)
template<int V>
__global__ __launch_bounds__(IMG_T) void img_points_kernel(ImgArgs a, ImgOut o, int total)
{
  const int p = blockIdx.x * IMG_T + threadIdx.x;
  if(p < total) img_point<V>(a, o, p / a.K, p % a.K);
}

// K <= 64.  grid: ceil(n / IMG_WAVES): wavefront f, lane k
template<int V>
__global__ __launch_bounds__(IMG_T) void img_small_kernel(ImgArgs a, ImgOut o, int n, float * __restrict__ energy)
{
  const int f = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * IMG_WAVES + (threadIdx.x >> 6))), k = threadIdx.x & 63;
  if(f >= n) return;
  float e = 0.0f;
  if(k < a.K) e = img_point<V>(a, o, f, k);
  const float s = sum64_meet(0.0f + e); // fixed_sum.h: partial k, the partials past 63 left out
  if(k == 0) energy[f] = s;
}

// K > 64.  grid: n; a workgroup of 1024 / NQ threads, thread t owns the partials t + (1024 / NQ) q, q < NQ
template<int V, int NQ>
__global__ __launch_bounds__(1024 / NQ) void img_wide_kernel(ImgArgs a, ImgOut o, float * __restrict__ energy)
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
      if(k < a.K) s[q] = s[q] + img_point<V>(a, o, f, k);
    }
  const float sum = sum1024_meet<NQ>(s, cross);
  if(t == 0) energy[f] = sum;
}

// grid: ceil(n K / IMG_T): thread (f, k)
template<int V>
__global__ __launch_bounds__(IMG_T) void img_vjp_uv_kernel(ImgArgs a, ImgCot g, int total, float * guv, int accumulate)
{
  const int p = blockIdx.x * IMG_T + threadIdx.x;
  if(p >= total) return;
  const int f = p / a.K, k = p % a.K;
  float su = 0.0f, sv = 0.0f;
  const ImgCell q = img_cell(a, f, k);
  if(q.inside)
    img_point_vjp<V>(a, g, f, k, q, 0, a.Cs, [&](int, float gamma, float du, float dv) {
      su = su + gamma * du;
      sv = sv + gamma * dv;
    });
  float * o = guv + 2 * p;
  o[0] = accumulate ? o[0] + su : su;
  o[1] = accumulate ? o[1] + sv : sv;
}

// grid: B x chunks x tiles, tiles = tiles_x x ceil(H / IMG_TILE), chunks = ceil(C / IMG_GC); the tile index runs fastest.  n: the frames.
template<int V>
__global__ __launch_bounds__(IMG_T) void img_vjp_image_kernel(ImgArgs a, ImgCot g, int n, int tiles_x, int tiles, int chunks, float * gimg, int accumulate)
{
  __shared__ float4 s_g[IMG_LIST];                   // the cotangents gamma of the workgroup's channels (+0 where the point samples none)
  __shared__ float s_fx[IMG_LIST], s_fy[IMG_LIST];
  __shared__ int s_at[IMG_LIST];                     // the cell against the tile: (i - x0 + 1) | (j - y0 + 1) << 8
  __shared__ int s_cnt[IMG_GR][IMG_WAVES];
  const int tile = blockIdx.x % tiles, chunk = (blockIdx.x / tiles) % chunks, b = blockIdx.x / (tiles * chunks);
  const int x0 = (tile % tiles_x) * IMG_TILE, y0 = (tile / tiles_x) * IMG_TILE, c0 = chunk * IMG_GC;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int px = t % IMG_TILE, py = t / IMG_TILE;
  // the points that read image b, in ascending flat index
  const int p_lo = a.image_per_frame ? b * a.K : 0, p_hi = a.image_per_frame ? p_lo + a.K : n * a.K;
  float acc[IMG_GC] = {0.0f, 0.0f, 0.0f, 0.0f};
  // a pass's uv are read one pass ahead, so that the read is in flight behind the list of the pass before (past the end: outside)
  const ImgPair * uv2 = reinterpret_cast<const ImgPair *>(a.uv);
  ImgPair cur[IMG_GR], nxt[IMG_GR];
#pragma unroll
  for(int r = 0; r < IMG_GR; r++)
  {
    const int p = p_lo + r * IMG_T + t;
    cur[r] = p < p_hi ? uv2[p] : ImgPair{-1.0f, -1.0f};
  }
  for(int base = p_lo; base < p_hi; base += IMG_LIST)
  {
    bool hit[IMG_GR];
    int pos[IMG_GR], at[IMG_GR];
    float fx[IMG_GR], fy[IMG_GR];
    float4 gm[IMG_GR];
#pragma unroll
    for(int r = 0; r < IMG_GR; r++)
    {
      const int p = base + IMG_LIST + r * IMG_T + t;
      nxt[r] = p < p_hi ? uv2[p] : ImgPair{-1.0f, -1.0f};
    }
#pragma unroll
    for(int r = 0; r < IMG_GR; r++)
    {
      const int p = base + r * IMG_T + t;
      hit[r] = false;
      gm[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      ImgCell q = img_cell_at(a, cur[r].x, cur[r].y);
      const int lx = q.i - x0 + 1, ly = q.j - y0 + 1; // the cell's pixels are (i, i + 1) x (j, j + 1)
      if(q.inside && lx >= 0 && lx <= IMG_TILE && ly >= 0 && ly <= IMG_TILE)
      {
        const int f = a.image_per_frame ? b : p / a.K, k = p - f * a.K;
        img_cell_bind(a, f, k, q);
        if(q.inside && (!a.channel || q.c / IMG_GC == chunk))
        {
          const int lo = a.channel ? 0 : c0, hi = a.channel ? 1 : min(c0 + IMG_GC, a.C);
          float4 & m = gm[r];
          hit[r] = img_point_vjp<V>(a, g, f, k, q, lo, hi, [&](int c, float gamma, float, float) {
            const int e = (a.channel ? q.c : c) - c0;
            if(e == 0) m.x = gamma;
            else if(e == 1) m.y = gamma;
            else if(e == 2) m.z = gamma;
            else m.w = gamma;
          });
          at[r] = lx | ly << 8, fx[r] = q.fx, fy[r] = q.fy;
        }
      }
      const uint64_t mask = __ballot(hit[r]);
      pos[r] = (int)__popcll(mask & ((1ull << lane) - 1ull));
      if(lane == 0) s_cnt[r][wave] = (int)__popcll(mask);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for(int r = 0; r < IMG_GR; r++)
      for(int w = 0; w < IMG_WAVES; w++)
      {
        if(w == wave) pos[r] += total; // points before this one: earlier rows, then earlier wavefronts of this row
        total += s_cnt[r][w];
      }
#pragma unroll
    for(int r = 0; r < IMG_GR; r++)
      if(hit[r]) s_g[pos[r]] = gm[r], s_fx[pos[r]] = fx[r], s_fy[pos[r]] = fy[r], s_at[pos[r]] = at[r];
    __syncthreads();
#pragma unroll 4
    for(int h = 0; h < total; h++)
    {
      const int cell = s_at[h];
      const int dx = px - ((cell & 255) - 1), dy = py - ((cell >> 8) - 1); // 0 or 1: this pixel is a tap of the cell
      const bool on = (unsigned)dx < 2u && (unsigned)dy < 2u;
      const float hx = s_fx[h], hy = s_fy[h];
      const float wx = dx ? hx : 1.0f - hx, wy = dy ? hy : 1.0f - hy;
      const float w = wx * wy;
      const float4 m = s_g[h];
      acc[0] = acc[0] + (on ? w * m.x : 0.0f);
      acc[1] = acc[1] + (on ? w * m.y : 0.0f);
      acc[2] = acc[2] + (on ? w * m.z : 0.0f);
      acc[3] = acc[3] + (on ? w * m.w : 0.0f);
    }
    __syncthreads();
#pragma unroll
    for(int r = 0; r < IMG_GR; r++) cur[r] = nxt[r];
  }
  const int x = x0 + px, y = y0 + py;
  if(x >= a.W || y >= a.H) return;
  float * o = gimg + (((b * a.H + y) * a.W + x) * a.C + c0);
#pragma unroll
  for(int e = 0; e < IMG_GC; e++)
    if(c0 + e < a.C) o[e] = accumulate ? o[e] + acc[e] : acc[e];
}

static unsigned img_blocks(int64_t items, int per)
{
  return (unsigned)((items + per - 1) / per);
}

static int img_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

static bool img_one_or_n(int64_t v, int64_t n)
{
  return v == 1 || v == n;
}

// what the three calls refuse alike
static int img_check(const char * fn, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W, int64_t C,
                     const int64_t * channel, int space)
{
  if(!uv || !image) return img_refuse(fn, "uv or image is NULL");
  if(n <= 0 || K <= 0) return img_refuse(fn, "n and K must be positive");
  if(H < 2 || H > 8192 || W < 2 || W > 8192) return img_refuse(fn, "H and W must be in [2, 8192]");
  if(C < 1 || C > 32) return img_refuse(fn, "C must be in [1, 32]");
  if(!img_one_or_n(B, n)) return img_refuse(fn, "B must be 1 or n");
  const int64_t Cs = channel ? 1 : C;
  if(n > IMG_INT32_MAX || K > IMG_INT32_MAX || n * K > IMG_INT32_MAX / (2 * Cs)) return img_refuse(fn, "n K Cs 2 beyond int32 indexing");
  if(B * H * W * C > IMG_INT32_MAX) return img_refuse(fn, "B H W C beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(channel && space == SMPLPP_HOST) return ids_in(fn, "channel", channel, K, 0, C);
  return SMPLPP_OK;
}

// and the two calls of the term
static int img_term_check(const char * fn, int64_t n, const float * target, int64_t Tn, const float * weight, int64_t Wn, float rho)
{
  if(target && !img_one_or_n(Tn, n)) return img_refuse(fn, "Tn must be 1 or n");
  if(weight && !img_one_or_n(Wn, n)) return img_refuse(fn, "Wn must be 1 or n");
  if(!(rho >= 0.0f && rho < INFINITY)) return img_refuse(fn, "rho must be finite and not negative");
  return SMPLPP_OK;
}

// 16-byte reads: whole groups of four channels at 16-byte-aligned addresses
static bool img_wide_reads(const float * image, int64_t C, const int64_t * channel)
{
  return C % 4 == 0 && !channel && reinterpret_cast<uintptr_t>(image) % 16 == 0;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// one launch per read width: KERNEL(4) or KERNEL(1)
#define IMG_LAUNCH(wide, KERNEL, grid, block, st, ...)                   \
  do                                                                     \
  {                                                                      \
    if(wide) KERNEL(4)<<<grid, block, 0, st>>>(__VA_ARGS__);             \
    else                                                                 \
      KERNEL(1)<<<grid, block, 0, st>>>(__VA_ARGS__);                    \
    HIP_TRY(hipGetLastError());                                          \
  } while(0)
#define IMG_SAMPLE(V) img_sample_kernel<V>
#define IMG_POINTS(V) img_points_kernel<V>
#define IMG_SMALL(V) img_small_kernel<V>
#define IMG_WIDE4(V) img_wide_kernel<V, 4>
#define IMG_WIDE1(V) img_wide_kernel<V, 1>
#define IMG_VJP_UV(V) img_vjp_uv_kernel<V>
#define IMG_VJP_IMAGE(V) img_vjp_image_kernel<V>

extern "C" int smplpp_image_sample(int device, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W,
                                   int64_t C, const int64_t * channel, float * value, float * gradient, uint8_t * valid, int space, void * stream)
{
  const char * fn = "smplpp_image_sample";
  if(int rc = img_check(fn, n, K, uv, image, B, H, W, C, channel, space)) return rc;
  if(!value && !gradient && !valid) return img_refuse(fn, "every output is NULL");
  const int64_t total = n * K, Cs = channel ? 1 : C;
  Frame fr(device, nullptr, space, stream, "image sample");
  ImgArgs a{fr.in(uv, (size_t)(total * 2)), fr.in(image, (size_t)(B * H * W * C)), fr.in(channel, (size_t)K), nullptr, nullptr,
            (int)K, (int)H, (int)W, (int)C, (int)Cs, B != 1, 0, 0, 0.0f};
  float * o_v = fr.out(value, (size_t)(total * Cs));
  float * o_g = fr.out(gradient, (size_t)(total * Cs * 2));
  uint8_t * o_ok = fr.out(valid, (size_t)total);
  return fr.run([&] {
    IMG_LAUNCH(img_wide_reads(a.image, C, channel), IMG_SAMPLE, dim3(img_blocks(total, IMG_T)), dim3(IMG_T), fr.st, a, (int)total, o_v, o_g, o_ok);
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_image_term(int device, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W, int64_t C,
                                 const int64_t * channel, const float * target, int64_t Tn, const float * weight, int64_t Wn, float rho,
                                 float * energy, float * point_energy, float * value, uint8_t * valid, int space, void * stream)
{
  const char * fn = "smplpp_image_term";
  if(int rc = img_check(fn, n, K, uv, image, B, H, W, C, channel, space)) return rc;
  if(int rc = img_term_check(fn, n, target, Tn, weight, Wn, rho)) return rc;
  if(!energy && !point_energy && !value && !valid) return img_refuse(fn, "every output is NULL");
  const int64_t total = n * K, Cs = channel ? 1 : C;
  Frame fr(device, nullptr, space, stream, "image term");
  ImgArgs a{fr.in(uv, (size_t)(total * 2)), fr.in(image, (size_t)(B * H * W * C)), fr.in(channel, (size_t)K), nullptr, nullptr,
            (int)K, (int)H, (int)W, (int)C, (int)Cs, B != 1, target && Tn != 1, weight && Wn != 1, rho};
  a.target = fr.in(target, (size_t)(Tn * K * Cs));
  a.weight = fr.in(weight, (size_t)(Wn * K));
  float * e = fr.out(energy, (size_t)n);
  ImgOut o{fr.out(point_energy, (size_t)total), fr.out(value, (size_t)(total * Cs)), fr.out(valid, (size_t)total)};
  return fr.run([&] {
    const bool wide = img_wide_reads(a.image, C, channel);
    const FrameSumSplit sp = frame_sum_split(K); // fixed_sum.h
    if(!e) IMG_LAUNCH(wide, IMG_POINTS, dim3(img_blocks(total, IMG_T)), dim3(IMG_T), fr.st, a, o, (int)total);
    else if(sp.nq == 0)
      IMG_LAUNCH(wide, IMG_SMALL, dim3(img_blocks(n, IMG_WAVES)), dim3(IMG_T), fr.st, a, o, (int)n, e);
    else if(sp.nq == 4)
      IMG_LAUNCH(wide, IMG_WIDE4, dim3((unsigned)n), dim3(sp.threads), fr.st, a, o, e);
    else
      IMG_LAUNCH(wide, IMG_WIDE1, dim3((unsigned)n), dim3(sp.threads), fr.st, a, o, e);
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_image_term_vjp(int device, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W,
                                     int64_t C, const int64_t * channel, const float * target, int64_t Tn, const float * weight, int64_t Wn,
                                     float rho, const float * grad_energy, const float * grad_point_energy, const float * grad_value,
                                     float * grad_uv, float * grad_image, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_image_term_vjp";
  if(int rc = img_check(fn, n, K, uv, image, B, H, W, C, channel, space)) return rc;
  if(int rc = img_term_check(fn, n, target, Tn, weight, Wn, rho)) return rc;
  if(!grad_energy && !grad_point_energy && !grad_value) return img_refuse(fn, "every cotangent is NULL");
  if(!grad_uv && !grad_image) return img_refuse(fn, "grad_uv and grad_image are both NULL");
  if(accumulate != 0 && accumulate != 1) return img_refuse(fn, "accumulate must be 0 or 1");
  const int64_t total = n * K, Cs = channel ? 1 : C, pixels = B * H * W * C;
  Frame fr(device, nullptr, space, stream, "image term VJP");
  ImgArgs a{fr.in(uv, (size_t)(total * 2)), fr.in(image, (size_t)pixels), fr.in(channel, (size_t)K), nullptr, nullptr,
            (int)K, (int)H, (int)W, (int)C, (int)Cs, B != 1, target && Tn != 1, weight && Wn != 1, rho};
  a.target = fr.in(target, (size_t)(Tn * K * Cs));
  a.weight = fr.in(weight, (size_t)(Wn * K));
  const ImgCot g{fr.in(grad_energy, (size_t)n), fr.in(grad_point_energy, (size_t)total), fr.in(grad_value, (size_t)(total * Cs))};
  float * guv = fr.out(grad_uv, (size_t)(total * 2), accumulate != 0);
  float * gimg = fr.out(grad_image, (size_t)pixels, accumulate != 0);
  return fr.run([&] {
    const bool wide = img_wide_reads(a.image, C, channel);
    if(guv) IMG_LAUNCH(wide, IMG_VJP_UV, dim3(img_blocks(total, IMG_T)), dim3(IMG_T), fr.st, a, g, (int)total, guv, accumulate);
    if(gimg)
    {
      const int tiles_x = (int)((W + IMG_TILE - 1) / IMG_TILE), tiles = tiles_x * (int)((H + IMG_TILE - 1) / IMG_TILE);
      const int chunks = (int)((C + IMG_GC - 1) / IMG_GC);
      IMG_LAUNCH(wide, IMG_VJP_IMAGE, dim3((unsigned)(B * chunks * tiles)), dim3(IMG_T), fr.st, a, g, (int)n, tiles_x, tiles, chunks, gimg,
                 accumulate);
    }
    return (int)SMPLPP_OK;
  });
}
