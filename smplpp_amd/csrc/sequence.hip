// Sequence terms: what makes the frames of a grouped L-BFGS problem a sequence.  A layout handle maps the optimiser's rows
// to compact frames; split / merge move between the optimiser buffer and the per-frame arrays (merge sums a shared row's gradient over the
// problem's frames), sum folds frame values into problem values, and smoothness is the first- or second-difference term between
// consecutive frames of a problem with its vector-Jacobian product.  The rules are in include/smplpp_hip.h; every fp32 operation below is
// rounded on its own (no contraction to FMA), every output element is one fixed-order sum (sum1024 of fixed_sum.h, whose two facts about
// +0 let the work split follow the size), and there are no floating-point atomics.
//
//  seq_split_kernel         a thread per (frame, coordinate) of the two outputs together: one launch makes theta [F,C_f] and beta [F,C_s].
//  seq_merge_kernel         a thread per (row, coordinate < D): a frame row's slice of grad_frames or +0, a shared row's +0 past C_s.
//  seq_merge_shared_kernel  a wavefront per (problem, coordinate < C_s): lane l owns the partials l + 64 q, q < 16.
//  seq_sum_kernel           a wavefront per problem, the same ownership.
//  seq_smooth_small_kernel  K <= 64: a wavefront per frame, lane k owns point k (partial k; the partials past 63 are +0).
//  seq_smooth_wide_kernel   K > 64: a workgroup per frame, of 256 or 1024 threads by frame_sum_split: thread t owns the partials t + T q.
//  seq_smooth_vjp_kernel    a thread per (frame, point): it recomputes the at most three stencils that touch it (a gather).
#include <algorithm>

#include "fixed_sum.h"
#include "sequence_tables.h"
#include "staging.h"

#pragma clang fp contract(off)

struct smplpp_sequence
{
  int device = 0;
  int64_t P = 0, rows = 0, frames = 0;
  int shared_rows = 0;
  std::vector<int64_t> frame_start;                                    // [P+1], host
  smplpp_hip::DevBuf row_start, frame_start_d, problem_of, row_of, frame_of; // the tables of sequence_tables.h as int32
  smplpp_hip::Arena arena;                                              // staging of the host-space calls on this layout
};

namespace smplpp_hip
{
using Sequence = struct ::smplpp_sequence;
constexpr int SEQ_T = 256; // threads of every kernel here (the wide forward above K = 1024 takes 1024)
constexpr int SEQ_WAVES = SEQ_T / 64;

// the device images of a layout
struct SeqView
{
  const int *row_start, *frame_start, *problem_of, *row_of, *frame_of;
  int P, F, rows;
};

// grid: ceil(F W / SEQ_T), W = the widths of the outputs given
__global__ __launch_bounds__(SEQ_T) void seq_split_kernel(SeqView s, const float * __restrict__ rows, int64_t ld, int off_f, int C_f,
                                                          float * __restrict__ frames, int C_s, float * __restrict__ shared)
{
  const int wf = frames ? C_f : 0, W = wf + (shared ? C_s : 0);
  const int64_t i = (int64_t)blockIdx.x * SEQ_T + threadIdx.x;
  if(i >= (int64_t)s.F * W) return;
  const int f = (int)(i / W), c = (int)(i % W);
  if(c < wf) frames[(int64_t)f * C_f + c] = rows[s.row_of[f] * ld + off_f + c];
  else
    shared[(int64_t)f * C_s + (c - wf)] = rows[(s.row_start[s.problem_of[f] + 1] - 1) * ld + (c - wf)];
}

// grid: ceil(rows D / SEQ_T).  cs_sum: the coordinates of a shared row that seq_merge_shared_kernel writes (C_s, or 0 without grad_shared)
__global__ __launch_bounds__(SEQ_T) void seq_merge_kernel(SeqView s, const float * __restrict__ gf, int off_f, int C_f, int cs_sum, float * gr,
                                                          int64_t ld, int D, int accumulate)
{
  const int64_t i = (int64_t)blockIdx.x * SEQ_T + threadIdx.x;
  if(i >= (int64_t)s.rows * D) return;
  const int r = (int)(i / D), d = (int)(i % D), f = s.frame_of[r];
  float v = 0.0f;
  if(f < 0)
  {
    if(d < cs_sum) return;
  }
  else if(gf && d >= off_f && d < off_f + C_f)
    v = gf[(int64_t)f * C_f + (d - off_f)];
  float * o = gr + r * ld + d;
  *o = accumulate ? *o + v : v;
}

// grid: ceil(P C_s / SEQ_WAVES): wavefront (p, c) sums grad_shared[f][c] over the frames of problem p into its shared row
__global__ __launch_bounds__(SEQ_T) void seq_merge_shared_kernel(SeqView s, const float * __restrict__ gs, int C_s, float * gr, int64_t ld,
                                                                 int accumulate)
{
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SEQ_WAVES + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if(w >= s.P * C_s) return;
  const int p = w / C_s, c = w % C_s, f0 = s.frame_start[p], T = s.frame_start[p + 1] - f0;
  const float * col = gs + (int64_t)f0 * C_s + c;
  const float v = sum1024_wave(T, lane, [&](int j) { return col[(int64_t)j * C_s]; });
  if(lane == 0)
  {
    float * o = gr + (s.row_start[p + 1] - 1) * ld + c;
    *o = accumulate ? *o + v : v;
  }
}

// grid: ceil(P / SEQ_WAVES): wavefront p
__global__ __launch_bounds__(SEQ_T) void seq_sum_kernel(SeqView s, const float * __restrict__ fv, float scale, float * pv, int accumulate)
{
  const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SEQ_WAVES + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if(p >= s.P) return;
  const int f0 = s.frame_start[p], T = s.frame_start[p + 1] - f0;
  const float * col = fv + f0;
  const float v = scale * sum1024_wave(T, lane, [&](int j) { return col[j]; });
  if(lane == 0) pv[p] = accumulate ? pv[p] + v : v;
}

// the temporal term's arguments
struct SmoothArgs
{
  const float * x;
  int64_t ld;
  int K, C, order;
  const float * weight;
  float rho;
};

// is there a stencil at frame h of the problem whose frames are [lo, hi)?  (h itself in [lo, hi))
__device__ inline bool seq_stencil(int h, int lo, int hi, int order)
{
  return order == 1 ? h + 1 < hi : (h - 1 >= lo && h + 1 < hi);
}
// d_c of the stencil at the frame whose point starts at xp
__device__ inline float seq_d(const float * __restrict__ xp, int64_t ld, int c, int order)
{
  const float a = xp[ld + c] - xp[c];
  return order == 1 ? a : a - (xp[c] - xp[c - ld]);
}
__device__ inline float seq_q(const float * __restrict__ xp, int64_t ld, int C, int order)
{
  float q = 0.0f;
  for(int c = 0; c < C; c++)
  {
    const float d = seq_d(xp, ld, c, order);
    q = q + d * d;
  }
  return q;
}
// e of point k of frame f (stencil: there is one at f)
__device__ inline float seq_energy(const SmoothArgs & a, int f, int k, bool stencil)
{
  const float w = a.weight ? a.weight[k] : 1.0f;
  if(!stencil || w == 0.0f) return 0.0f;
  const float q = seq_q(a.x + f * a.ld + k * a.C, a.ld, a.C, a.order);
  if(a.rho == 0.0f) return w * q;
  const float p2 = a.rho * a.rho;
  return w * ((p2 * q) / (p2 + q));
}

// K <= 64.  grid: ceil(F / SEQ_WAVES): wavefront f, lane k
__global__ __launch_bounds__(SEQ_T) void seq_smooth_small_kernel(SeqView s, SmoothArgs a, float * __restrict__ frame_energy,
                                                                 float * __restrict__ point_energy)
{
  const int f = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SEQ_WAVES + (threadIdx.x >> 6))), k = threadIdx.x & 63;
  if(f >= s.F) return;
  const int p = s.problem_of[f];
  const bool stencil = seq_stencil(f, s.frame_start[p], s.frame_start[p + 1], a.order);
  float e = 0.0f;
  if(k < a.K)
  {
    e = seq_energy(a, f, k, stencil);
    if(point_energy) point_energy[(int64_t)f * a.K + k] = e;
  }
  if(!frame_energy) return;
  const float v = sum64_meet(0.0f + e); // fixed_sum.h: partial k, the partials past 63 left out
  if(k == 0) frame_energy[f] = v;
}

// K > 64.  grid: F; a workgroup of 1024 / NQ threads, thread t owns the partials t + (1024 / NQ) q, q < NQ
template<int NQ>
__global__ __launch_bounds__(1024 / NQ) void seq_smooth_wide_kernel(SeqView s, SmoothArgs a, float * __restrict__ frame_energy,
                                                                     float * __restrict__ point_energy)
{
  constexpr int T = 1024 / NQ;
  __shared__ float cross[T / 64];
  const int f = blockIdx.x, t = threadIdx.x, p = s.problem_of[f];
  const bool stencil = seq_stencil(f, s.frame_start[p], s.frame_start[p + 1], a.order);
  float v[NQ];
#pragma unroll
  for(int q = 0; q < NQ; q++) v[q] = 0.0f;
  for(int k0 = 0; k0 < a.K; k0 += 1024)
#pragma unroll
    for(int q = 0; q < NQ; q++)
    {
      const int k = k0 + T * q + t;
      if(k < a.K)
      {
        const float e = seq_energy(a, f, k, stencil);
        if(point_energy) point_energy[(int64_t)f * a.K + k] = e;
        v[q] = v[q] + e;
      }
    }
  if(!frame_energy) return;
  const float sum = sum1024_meet<NQ>(v, cross);
  if(t == 0) frame_energy[f] = sum;
}

// grid: ceil(F K / SEQ_T): thread (f, k).  gfe, gpe: the cotangents of frame_energy and point_energy, each may be null
__global__ __launch_bounds__(SEQ_T) void seq_smooth_vjp_kernel(SeqView s, SmoothArgs a, const float * __restrict__ gfe,
                                                               const float * __restrict__ gpe, float * gx, int accumulate)
{
  const int64_t i = (int64_t)blockIdx.x * SEQ_T + threadIdx.x;
  if(i >= (int64_t)s.F * a.K) return;
  const int f = (int)(i / a.K), k = (int)(i % a.K), p = s.problem_of[f], lo = s.frame_start[p], hi = s.frame_start[p + 1];
  const float w = a.weight ? a.weight[k] : 1.0f, p2 = a.rho * a.rho;
  // the stencils at f - 1, f and (order 2) f + 1: their scale s_n, and whether they contribute at all
  float sc[3] = {0.0f, 0.0f, 0.0f};
  bool live[3] = {false, false, false};
#pragma unroll
  for(int n = 0; n < 3; n++)
  {
    const int h = f - 1 + n;
    if(n > a.order || h < lo || h >= hi || !seq_stencil(h, lo, hi, a.order) || w == 0.0f) continue;
    float g = gfe ? gfe[h] : 0.0f;
    if(gpe) g = g + gpe[(int64_t)h * a.K + k];
    if(g == 0.0f) continue;
    live[n] = true;
    const float gw = (2.0f * g) * w;
    if(a.rho == 0.0f) sc[n] = gw;
    else
    {
      const float q = seq_q(a.x + h * a.ld + k * a.C, a.ld, a.C, a.order);
      const float t = p2 / (p2 + q);
      sc[n] = gw * (t * t);
    }
  }
  float * o = gx + f * a.ld + k * a.C;
  for(int c = 0; c < a.C; c++)
  {
    float v[3];
#pragma unroll
    for(int n = 0; n < 3; n++) v[n] = live[n] ? sc[n] * seq_d(a.x + (f - 1 + n) * a.ld + k * a.C, a.ld, c, a.order) : 0.0f;
    const float el = a.order == 1 ? v[0] - v[1] : (v[0] + v[2]) - (2.0f * v[1]);
    o[c] = accumulate ? o[c] + el : el;
  }
}

template<class T>
static hipError_t seq_upload(DevBuf & b, const std::vector<T> & v)
{
  hipError_t e = b.reserve(v.empty() ? 4 : sizeof(T) * v.size());
  if(e == hipSuccess && !v.empty()) e = hipMemcpy(b.p.get(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
  return e;
}

static SeqView seq_view(const Sequence * q)
{
  return SeqView{q->row_start.as<int>(), q->frame_start_d.as<int>(), q->problem_of.as<int>(), q->row_of.as<int>(), q->frame_of.as<int>(),
                 (int)q->P, (int)q->frames, (int)q->rows};
}

static unsigned seq_blocks(int64_t items, int per)
{
  return (unsigned)((items + per - 1) / per);
}

static int seq_refuse(const char * fn, const char * why)
{
  return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + why);
}

// what the two calls of the temporal term refuse alike
static int seq_smooth_check(const char * fn, Sequence * q, const float * x, int64_t ld, int64_t K, int64_t C, int order, const float * weight,
                            float rho, int space)
{
  if(!q) return seq_refuse(fn, "no layout");
  if(!x) return seq_refuse(fn, "x is NULL");
  if(K <= 0) return seq_refuse(fn, "K must be positive");
  if(C < 1 || C > 16) return seq_refuse(fn, "C must be in [1, 16]");
  if(K > SEQ_INT32_MAX / 16 || ld < K * C) return seq_refuse(fn, "ld must be at least K C");
  if(order != 1 && order != 2) return seq_refuse(fn, "order must be 1 or 2");
  if(!(rho >= 0.0f && rho < INFINITY)) return seq_refuse(fn, "rho must be finite and not negative");
  if(ld > SEQ_INT32_MAX || q->frames * ld > SEQ_INT32_MAX) return seq_refuse(fn, "F ld beyond int32 indexing");
  if(int rc = check_space(space, fn)) return rc;
  if(weight && space == SMPLPP_HOST)
    for(int64_t k = 0; k < K; k++)
      if(!(weight[k] >= 0.0f && weight[k] < INFINITY)) return seq_refuse(fn, "a weight is negative or not finite");
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// Validate and build the host tables (sequence_tables.h), then upload them.
extern "C" int smplpp_sequence_create(int device, int64_t P, const int64_t * row_start, int shared_rows, struct smplpp_sequence ** out)
{
  const char * fn = "smplpp_sequence_create";
  if(!out) return seq_refuse(fn, "no out");
  *out = nullptr;
  const SequenceTables t = sequence_tables(P, row_start, shared_rows);
  if(t.refusal) return seq_refuse(fn, t.refusal);
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<Sequence> q(new Sequence());
  q->device = device, q->P = t.P, q->rows = t.rows, q->frames = t.frames, q->shared_rows = t.shared_rows;
  q->frame_start = t.frame_start;
  HIP_TRY(seq_upload(q->row_start, std::vector<int>(t.row_start.begin(), t.row_start.end())));
  HIP_TRY(seq_upload(q->frame_start_d, std::vector<int>(t.frame_start.begin(), t.frame_start.end())));
  HIP_TRY(seq_upload(q->problem_of, t.problem_of));
  HIP_TRY(seq_upload(q->row_of, t.row_of));
  HIP_TRY(seq_upload(q->frame_of, t.frame_of));
  *out = q.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_sequence_destroy(struct smplpp_sequence * q)
{
  if(!q) return SMPLPP_OK;
  (void)hipSetDevice(q->device);
  delete q;
  return SMPLPP_OK;
}

extern "C" int smplpp_sequence_info(const struct smplpp_sequence * q, int64_t * P, int64_t * rows, int64_t * frames, int * shared_rows,
                                    int64_t * frame_start)
{
  if(!q) return seq_refuse("smplpp_sequence_info", "no layout");
  if(P) *P = q->P;
  if(rows) *rows = q->rows;
  if(frames) *frames = q->frames;
  if(shared_rows) *shared_rows = q->shared_rows;
  if(frame_start)
    for(int64_t p = 0; p <= q->P; p++) frame_start[p] = q->frame_start[(size_t)p];
  return SMPLPP_OK;
}

extern "C" int smplpp_sequence_split(struct smplpp_sequence * q, const float * rows, int64_t ld, int64_t off_f, int64_t C_f, float * frames,
                                     int64_t C_s, float * shared, int space, void * stream)
{
  const char * fn = "smplpp_sequence_split";
  if(!q) return seq_refuse(fn, "no layout");
  if(!rows) return seq_refuse(fn, "rows is NULL");
  if(!frames && !shared) return seq_refuse(fn, "every output is NULL");
  if(ld <= 0 || ld > SEQ_INT32_MAX || q->rows * ld > SEQ_INT32_MAX) return seq_refuse(fn, "ld must be positive and rows ld within int32 indexing");
  if(frames && (off_f < 0 || C_f < 1 || off_f > ld || off_f + C_f > ld)) return seq_refuse(fn, "off_f + C_f must lie within ld");
  if(shared && q->shared_rows == 0) return seq_refuse(fn, "this layout has no shared rows");
  if(shared && (C_s < 1 || C_s > ld)) return seq_refuse(fn, "C_s must lie within ld");
  if(int rc = check_space(space, fn)) return rc;
  const int64_t F = q->frames, W = (frames ? C_f : 0) + (shared ? C_s : 0);
  if(F * W > SEQ_INT32_MAX) return seq_refuse(fn, "the outputs are beyond int32 indexing");
  const int64_t need = std::max(frames ? off_f + C_f : 0, shared ? C_s : 0); // the floats of the last row that are read
  Frame fr(q->device, &q->arena, space, stream, "sequence split");
  const float * r = fr.in(rows, (size_t)((q->rows - 1) * ld + need));
  float * o_f = fr.out(frames, (size_t)(F * C_f));
  float * o_s = fr.out(shared, (size_t)(F * C_s));
  return fr.run([&] {
    seq_split_kernel<<<dim3(seq_blocks(F * W, SEQ_T)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), r, ld, (int)off_f, (int)C_f, o_f, (int)C_s, o_s);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_sequence_merge(struct smplpp_sequence * q, const float * grad_frames, int64_t off_f, int64_t C_f, const float * grad_shared,
                                     int64_t C_s, float * grad_rows, int64_t ld, int64_t D, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_sequence_merge";
  if(!q) return seq_refuse(fn, "no layout");
  if(!grad_rows) return seq_refuse(fn, "grad_rows is NULL");
  if(!grad_frames && !grad_shared) return seq_refuse(fn, "every input is NULL");
  if(D < 1 || D > ld || ld > SEQ_INT32_MAX || q->rows * ld > SEQ_INT32_MAX) return seq_refuse(fn, "D must be in [1, ld] and rows ld within int32 indexing");
  if(grad_frames && (off_f < 0 || C_f < 1 || off_f > D || off_f + C_f > D)) return seq_refuse(fn, "off_f + C_f must lie within D");
  if(grad_shared && q->shared_rows == 0) return seq_refuse(fn, "this layout has no shared rows");
  if(grad_shared && (C_s < 1 || C_s > D)) return seq_refuse(fn, "C_s must lie within D");
  if(accumulate != 0 && accumulate != 1) return seq_refuse(fn, "accumulate must be 0 or 1");
  if(int rc = check_space(space, fn)) return rc;
  const int64_t F = q->frames;
  if((grad_frames && F * C_f > SEQ_INT32_MAX) || (grad_shared && F * C_s > SEQ_INT32_MAX)) return seq_refuse(fn, "the inputs are beyond int32 indexing");
  Frame fr(q->device, &q->arena, space, stream, "sequence merge");
  const float * gf = fr.in(grad_frames, (size_t)(F * C_f));
  const float * gs = fr.in(grad_shared, (size_t)(F * C_s));
  // (a host-space row's floats past D travel with it: they are loaded so that the copy back leaves them as they were)
  float * gr = fr.out(grad_rows, (size_t)((q->rows - 1) * ld + D), accumulate || ld > D);
  return fr.run([&] {
    const int cs = gs ? (int)C_s : 0;
    seq_merge_kernel<<<dim3(seq_blocks(q->rows * D, SEQ_T)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), gf, (int)off_f, (int)C_f, cs, gr, ld, (int)D,
                                                                                      accumulate);
    HIP_TRY(hipGetLastError());
    if(gs)
    {
      seq_merge_shared_kernel<<<dim3(seq_blocks(q->P * C_s, SEQ_WAVES)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), gs, cs, gr, ld, accumulate);
      HIP_TRY(hipGetLastError());
    }
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_sequence_sum(struct smplpp_sequence * q, const float * frame_values, float scale, float * problem_values, int accumulate,
                                   int space, void * stream)
{
  const char * fn = "smplpp_sequence_sum";
  if(!q) return seq_refuse(fn, "no layout");
  if(!frame_values || !problem_values) return seq_refuse(fn, "frame_values or problem_values is NULL");
  if(accumulate != 0 && accumulate != 1) return seq_refuse(fn, "accumulate must be 0 or 1");
  if(int rc = check_space(space, fn)) return rc;
  Frame fr(q->device, &q->arena, space, stream, "sequence sum");
  const float * fv = fr.in(frame_values, (size_t)q->frames);
  float * pv = fr.out(problem_values, (size_t)q->P, accumulate != 0);
  return fr.run([&] {
    seq_sum_kernel<<<dim3(seq_blocks(q->P, SEQ_WAVES)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), fv, scale, pv, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_sequence_smoothness(struct smplpp_sequence * q, const float * x, int64_t ld, int64_t K, int64_t C, int order,
                                          const float * weight, float rho, float * frame_energy, float * point_energy, int space, void * stream)
{
  const char * fn = "smplpp_sequence_smoothness";
  if(int rc = seq_smooth_check(fn, q, x, ld, K, C, order, weight, rho, space)) return rc;
  if(!frame_energy && !point_energy) return seq_refuse(fn, "every output is NULL");
  const int64_t F = q->frames;
  Frame fr(q->device, &q->arena, space, stream, "sequence smoothness");
  const SmoothArgs a{fr.in(x, (size_t)((F - 1) * ld + K * C)), ld, (int)K, (int)C, order, fr.in(weight, (size_t)K), rho};
  float * fe = fr.out(frame_energy, (size_t)F);
  float * pe = fr.out(point_energy, (size_t)(F * K));
  return fr.run([&] {
    const FrameSumSplit sp = frame_sum_split(K); // fixed_sum.h
    if(sp.nq == 0) seq_smooth_small_kernel<<<dim3(seq_blocks(F, SEQ_WAVES)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), a, fe, pe);
    else if(sp.nq == 4)
      seq_smooth_wide_kernel<4><<<dim3((unsigned)F), dim3(sp.threads), 0, fr.st>>>(seq_view(q), a, fe, pe);
    else
      seq_smooth_wide_kernel<1><<<dim3((unsigned)F), dim3(sp.threads), 0, fr.st>>>(seq_view(q), a, fe, pe);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_sequence_smoothness_vjp(struct smplpp_sequence * q, const float * x, int64_t ld, int64_t K, int64_t C, int order,
                                              const float * weight, float rho, const float * grad_frame_energy, const float * grad_point_energy,
                                              float * grad_x, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_sequence_smoothness_vjp";
  if(int rc = seq_smooth_check(fn, q, x, ld, K, C, order, weight, rho, space)) return rc;
  if(!grad_frame_energy && !grad_point_energy) return seq_refuse(fn, "every cotangent is NULL");
  if(!grad_x) return seq_refuse(fn, "grad_x is NULL");
  if(accumulate != 0 && accumulate != 1) return seq_refuse(fn, "accumulate must be 0 or 1");
  const int64_t F = q->frames;
  const size_t span = (size_t)((F - 1) * ld + K * C);
  Frame fr(q->device, &q->arena, space, stream, "sequence smoothness VJP");
  const SmoothArgs a{fr.in(x, span), ld, (int)K, (int)C, order, fr.in(weight, (size_t)K), rho};
  const float * gfe = fr.in(grad_frame_energy, (size_t)F);
  const float * gpe = fr.in(grad_point_energy, (size_t)(F * K));
  // (a host-space row's floats past K C travel with it: they are loaded so that the copy back leaves them as they were)
  float * gx = fr.out(grad_x, span, accumulate || ld > K * C);
  return fr.run([&] {
    seq_smooth_vjp_kernel<<<dim3(seq_blocks(F * K, SEQ_T)), dim3(SEQ_T), 0, fr.st>>>(seq_view(q), a, gfe, gpe, gx, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
