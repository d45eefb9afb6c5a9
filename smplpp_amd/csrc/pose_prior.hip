// Pose priors: a max-mixture Gaussian prior over D pose coordinates and one-sided quadratic joint limits, with their
// vector-Jacobian product.  The rules are in include/smplpp_hip.h; every fp32 operation below is rounded on its own (no contraction to
// FMA), every output element is one fixed-order sum, and there are no floating-point atomics.
//
//  prior_forward_kernel  a workgroup of PR_WAVES wavefronts takes PR_FT consecutive frames.  Wave w takes the components w, w + 4, ...:
//                        it leaves d = pose - mean[m] of the tile in its own LDS rows, then lane j runs the 8 partial sums of y_j for
//                        the PR_FT frames at once from the transposed image, so that one load of a matrix element serves the whole
//                        tile.  The outputs 64 .. D-1 take a second round: a lane each when they are many, else eight lanes each, one
//                        per partial (pr_matvec_split), which shortens the round from D dependent steps to D / 8.  y goes to LDS
//                        (when the residual is asked for), y.y by sum64 (fixed_sum.h), e_m to LDS; after a barrier one
//                        thread per frame selects, and the workgroup copies the chosen y out.  Then wave f sums the limit term of
//                        frame f.
//  prior_vjp_kernel      the same tile.  Without a given component the workgroup first selects as the forward does.  Then wave f takes
//                        frame f: y of the chosen component by the same matrix-vector walk, v = (2 g) y + grad_residual in LDS, and
//                        t = mat^T v by that walk on the untransposed image (lane k owns coordinate k).
#include "fixed_sum.h"
#include "pose_prior_tables.h"
#include "staging.h"

#pragma clang fp contract(off)

struct smplpp_pose_prior
{
  int device = 0;
  int64_t M = 0, D = 0;
  bool limits = false;
  smplpp_hip::DevBuf mean, mat, matT, offset; // [M,D], [M,D,D] as given, [M,D,D] transposed, [M]
  smplpp_hip::DevBuf lo, hi, weight;          // [D] each, with limits
  smplpp_hip::Arena arena;                    // staging of the host-space calls on this prior
};

namespace smplpp_hip
{
using PosePrior = struct ::smplpp_pose_prior; // (the bare name is the evaluation call)
constexpr int PR_T = 256;               // threads of both kernels
constexpr int PR_WAVES = PR_T / 64;     // wavefronts of a workgroup
constexpr int PR_FT = 4;                // frames of a workgroup's tile (the backward gives one to each wave: PR_FT == PR_WAVES)
constexpr int64_t PR_INT32_MAX = 0x7fffffffLL;
static_assert(PR_FT == PR_WAVES && PR_FT >= 2, "the backward gives wave f frame f and keeps d and v in two of its PR_FT rows");

// the device images of a prior
struct PriorTables
{
  const float *mean, *mat, *matT, *offset, *lo, *hi, *weight;
  int M, D;
};

constexpr size_t pr_lds_floats(int64_t M, int64_t D, bool stash)
{
  return (size_t)(PR_WAVES * PR_FT * D + (stash ? M * PR_FT * D : 0) + PR_FT * M + PR_FT);
}
constexpr int PR_LDS_MAX = (int)(sizeof(float) * pr_lds_floats(PRIOR_MAX_M, PRIOR_MAX_D, true));

// FT consecutive floats of LDS (one 16-byte read for the forward's tile)
template<int FT>
__device__ inline void pr_row(const float * vec, int i, float (&x)[FT])
{
  if constexpr(FT == 4)
  {
    const float4 v = *reinterpret_cast<const float4 *>(vec + i * 4);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  }
  else
#pragma unroll
    for(int f = 0; f < FT; f++) x[f] = vec[i * FT + f];
}

// out[f] = sum_i img[i D + idx] vec[i FT + f] for the FT columns of vec (LDS, [D][FT]), idx < D: partial i mod 8 in ascending i from +0,
// then ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7)).  Consecutive lanes read consecutive idx; 16 loads are in flight at a time.
template<int FT>
__device__ inline void pr_matvec(const float * __restrict__ img, const float * vec, int D, int idx, float (&out)[FT])
{
  float s[FT][8];
#pragma unroll
  for(int f = 0; f < FT; f++)
#pragma unroll
    for(int p = 0; p < 8; p++) s[f][p] = 0.0f;
  const float * col = img + idx;
  int i0 = 0;
  for(; i0 + 16 <= D; i0 += 16)
  {
    float a[16];
#pragma unroll
    for(int q = 0; q < 16; q++) a[q] = col[(i0 + q) * D];
#pragma unroll
    for(int q = 0; q < 16; q++)
    {
      float x[FT];
      pr_row<FT>(vec, i0 + q, x);
#pragma unroll
      for(int f = 0; f < FT; f++) s[f][q & 7] = s[f][q & 7] + a[q] * x[f];
    }
  }
  float a[16];
#pragma unroll
  for(int q = 0; q < 16; q++) a[q] = i0 + q < D ? col[(i0 + q) * D] : 0.0f;
#pragma unroll
  for(int q = 0; q < 16; q++)
    if(i0 + q < D)
    {
      float x[FT];
      pr_row<FT>(vec, i0 + q, x);
#pragma unroll
      for(int f = 0; f < FT; f++) s[f][q & 7] = s[f][q & 7] + a[q] * x[f];
    }
#pragma unroll
  for(int f = 0; f < FT; f++) out[f] = ((s[f][0] + s[f][4]) + (s[f][2] + s[f][6])) + ((s[f][1] + s[f][5]) + (s[f][3] + s[f][7]));
}

// The same sums for the outputs 64 .. D-1 when they are few (D - 64 <= PR_SPLIT): eight lanes per output, lane p of a group running
// partial p alone (i = p, p + 8, ... in ascending order from +0), the eight met by the xor tree 4, 2, 1, which is the grouping above.
// Eight outputs per pass; the result of output 64 + o is handed to lane o, its owner in the lane-per-output form.  Whole wavefront.
constexpr int PR_SPLIT = 32;
template<int FT>
__device__ inline void pr_matvec_split(const float * __restrict__ img, const float * vec, int D, int lane, float (&out)[FT])
{
  const int group = lane >> 3, p = lane & 7;
  for(int pass = 0; 64 + pass * 8 < D; pass++)
  {
    const int idx = 64 + pass * 8 + group;
    float s[FT];
#pragma unroll
    for(int f = 0; f < FT; f++) s[f] = 0.0f;
    if(idx < D)
      for(int i = p; i < D; i += 8)
      {
        const float a = img[i * D + idx];
        float x[FT];
        pr_row<FT>(vec, i, x);
#pragma unroll
        for(int f = 0; f < FT; f++) s[f] = s[f] + a * x[f];
      }
#pragma unroll
    for(int f = 0; f < FT; f++)
    {
      for(int m = 4; m >= 1; m >>= 1) s[f] = s[f] + __shfl_xor(s[f], m);
      const float got = __shfl(s[f], (lane & 7) * 8); // output 64 + pass 8 + (lane & 7), from the first lane of its group
      if(group == pass) out[f] = got;
    }
  }
}

// y of the outputs this lane owns: out[0] for output `lane`, out[1] for output lane + 64 (each when below D).  Whole wavefront.
template<int FT>
__device__ inline void pr_wave_matvec(const float * __restrict__ img, const float * vec, int D, int lane, float (&out)[2][FT])
{
  if(lane < D) pr_matvec<FT>(img, vec, D, lane, out[0]);
  if(D <= 64) return;
  if(D - 64 <= PR_SPLIT) pr_matvec_split<FT>(img, vec, D, lane, out[1]);
  else if(lane + 64 < D)
    pr_matvec<FT>(img, vec, D, lane + 64, out[1]);
}

// By the whole workgroup (it holds barriers): e_m of the frames [frame0, frame0 + nf) into esh [PR_FT][M], and their y into
// ysh [M][PR_FT][D] when ysh is given.  dsh: [PR_WAVES][PR_FT][D].  Rows of the tile past nf read zeros.
__device__ inline void pr_mixture(const PriorTables & t, const float * __restrict__ pose, int64_t ld, int64_t frame0, int nf, float * dsh,
                                  float * ysh, float * esh)
{
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, M = t.M, D = t.D;
  float * dw = dsh + w * PR_FT * D;
  for(int mb = 0; mb < M; mb += PR_WAVES)
  {
    const int m = mb + w;
    if(m < M)
      for(int f = 0; f < PR_FT; f++)
        for(int k = lane; k < D; k += 64) dw[k * PR_FT + f] = f < nf ? pose[(frame0 + f) * ld + k] - t.mean[m * D + k] : 0.0f;
    __syncthreads();
    if(m < M)
    {
      float qp[PR_FT];
#pragma unroll
      for(int f = 0; f < PR_FT; f++) qp[f] = 0.0f;
      float y[2][PR_FT];
      pr_wave_matvec<PR_FT>(t.matT + (int64_t)m * D * D, dw, D, lane, y);
#pragma unroll
      for(int r = 0; r < 2; r++)
      {
        const int j = lane + 64 * r;
        if(j < D)
#pragma unroll
          for(int f = 0; f < PR_FT; f++)
          {
            if(ysh) ysh[(m * PR_FT + f) * D + j] = y[r][f];
            qp[f] = qp[f] + y[r][f] * y[r][f];
          }
      }
#pragma unroll
      for(int f = 0; f < PR_FT; f++)
      {
        const float q = sum64_meet(qp[f]);
        if(lane == 0) esh[f * M + m] = q + t.offset[m];
      }
    }
    __syncthreads();
  }
}

// component 0, replaced by m = 1 .. M-1 in order when e_m < e_best: a tie keeps the lower index, a NaN never replaces nor is replaced
__device__ inline int pr_select(const float * e, int M)
{
  int best = 0;
  float eb = e[0];
  for(int m = 1; m < M; m++)
    if(e[m] < eb) eb = e[m], best = m;
  return best;
}

// grid: ceil(n / PR_FT); dynamic LDS: pr_lds_floats(M, D, residual != null) floats.  A null output is not computed; the mixture runs
// when energy, component or residual is given, the limit term when limit_energy is
__global__ __launch_bounds__(PR_T) void prior_forward_kernel(PriorTables t, const float * __restrict__ pose, int64_t ld, int64_t n,
                                                             float * __restrict__ energy, int64_t * __restrict__ component,
                                                             float * __restrict__ residual, float * __restrict__ limit_energy)
{
  extern __shared__ __attribute__((aligned(16))) float pr_smem[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, M = t.M, D = t.D;
  const int64_t frame0 = (int64_t)blockIdx.x * PR_FT;
  const int nf = (int)(n - frame0 < PR_FT ? n - frame0 : PR_FT);
  if(energy || component || residual)
  {
    float * dsh = pr_smem;
    float * ysh = residual ? dsh + PR_WAVES * PR_FT * D : nullptr;
    float * esh = dsh + PR_WAVES * PR_FT * D + (residual ? M * PR_FT * D : 0);
    int * sel = reinterpret_cast<int *>(esh + PR_FT * M);
    pr_mixture(t, pose, ld, frame0, nf, dsh, ysh, esh);
    if((int)threadIdx.x < nf)
    {
      const int f = threadIdx.x, b = pr_select(esh + f * M, M);
      sel[f] = b;
      if(energy) energy[frame0 + f] = esh[f * M + b];
      if(component) component[frame0 + f] = b;
    }
    if(residual)
    {
      __syncthreads();
      for(int i = threadIdx.x; i < nf * D; i += PR_T)
      {
        const int f = i / D, j = i % D;
        residual[(frame0 + f) * D + j] = ysh[(sel[f] * PR_FT + f) * D + j];
      }
    }
  }
  if(limit_energy && w < nf)
  {
    const int64_t frame = frame0 + w;
    float p = 0.0f;
    for(int k = lane; k < D; k += 64)
    {
      const float x = pose[frame * ld + k], a = x - t.hi[k], b = t.lo[k] - x;
      const float v = a > 0.0f ? a : (b > 0.0f ? b : 0.0f);
      p = p + t.weight[k] * (v * v);
    }
    p = sum64_meet(p);
    if(lane == 0) limit_energy[frame] = p;
  }
}

// grid: ceil(n / PR_FT); dynamic LDS: pr_lds_floats(M, D, false) floats.  ge, gr: the mixture's cotangents, gl: the limit term's; each
// may be null.  component null: chosen as the forward does; outside [0, M): the mixture contributes nothing
__global__ __launch_bounds__(PR_T) void prior_vjp_kernel(PriorTables t, const float * __restrict__ pose, int64_t ld, int64_t n,
                                                         const int64_t * __restrict__ component, const float * __restrict__ ge,
                                                         const float * __restrict__ gr, const float * __restrict__ gl, float * gp,
                                                         int accumulate)
{
  extern __shared__ __attribute__((aligned(16))) float pr_smem[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, M = t.M, D = t.D;
  const int64_t frame0 = (int64_t)blockIdx.x * PR_FT;
  const int nf = (int)(n - frame0 < PR_FT ? n - frame0 : PR_FT);
  float * dsh = pr_smem;
  float * esh = dsh + PR_WAVES * PR_FT * D;
  int * sel = reinterpret_cast<int *>(esh + PR_FT * M);
  const bool mix = ge || gr;
  if(mix)
  {
    if(!component)
    {
      pr_mixture(t, pose, ld, frame0, nf, dsh, nullptr, esh);
      if((int)threadIdx.x < nf) sel[threadIdx.x] = pr_select(esh + threadIdx.x * M, M);
    }
    else if((int)threadIdx.x < nf)
    {
      const int64_t c = component[frame0 + threadIdx.x];
      sel[threadIdx.x] = c >= 0 && c < M ? (int)c : -1;
    }
    __syncthreads();
  }
  // wave w takes frame frame0 + w; every wave reaches the two barriers
  const bool live = w < nf;
  const int64_t frame = frame0 + w;
  const int m = live && mix ? sel[w] : -1;
  const float g = m >= 0 && ge ? ge[frame] : 0.0f;
  float * dw = dsh + w * PR_FT * D; // d of the frame
  float * vw = dw + D;              // v of the frame
  if(g != 0.0f)
    for(int k = lane; k < D; k += 64) dw[k] = pose[frame * ld + k] - t.mean[m * D + k];
  __syncthreads();
  if(m >= 0)
  {
    const float g2 = 2.0f * g;
    float y[2][1];
    if(g != 0.0f) pr_wave_matvec<1>(t.matT + (int64_t)m * D * D, dw, D, lane, y);
    for(int r = 0; r < 2; r++)
    {
      const int j = lane + 64 * r;
      if(j >= D) continue;
      float v = g != 0.0f ? g2 * y[r][0] : 0.0f;
      if(gr) v = v + gr[frame * D + j];
      vw[j] = v;
    }
  }
  __syncthreads();
  float tk[2][1] = {{0.0f}, {0.0f}};
  if(m >= 0) pr_wave_matvec<1>(t.mat + (int64_t)m * D * D, vw, D, lane, tk);
  if(!live) return;
  const float g_l = gl ? gl[frame] : 0.0f;
  for(int r = 0; r < 2; r++)
  {
    const int k = lane + 64 * r;
    if(k >= D) break;
    float el = tk[r][0];
    if(gl)
    {
      float u = 0.0f;
      if(g_l != 0.0f)
      {
        const float x = pose[frame * ld + k], a = x - t.hi[k], b = t.lo[k] - x, c = (2.0f * g_l) * t.weight[k];
        if(a > 0.0f) u = c * a;
        else if(b > 0.0f) u = -(c * b);
      }
      el = mix ? el + u : u;
    }
    float * o = gp + frame * ld + k;
    *o = accumulate ? *o + el : el;
  }
}

static hipError_t pr_upload(DevBuf & b, const std::vector<float> & v)
{
  hipError_t e = b.reserve(v.empty() ? 4 : sizeof(float) * v.size());
  if(e == hipSuccess && !v.empty()) e = hipMemcpy(b.p.get(), v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice);
  return e;
}

static PriorTables pr_tables(const PosePrior * pr)
{
  return PriorTables{pr->mean.as<float>(), pr->mat.as<float>(), pr->matT.as<float>(), pr->offset.as<float>(), pr->lo.as<float>(),
                     pr->hi.as<float>(), pr->weight.as<float>(), (int)pr->M, (int)pr->D};
}

// what both calls refuse alike; `mixture` / `limit`: an output or cotangent of that part is given
static int pr_check(const char * fn, PosePrior * pr, int64_t n, const float * pose, int64_t ld, bool mixture, bool limit, int space)
{
  if(!pr) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no prior");
  if(n <= 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n must be positive");
  if(ld < pr->D) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": ld must be at least D");
  if(n > PR_INT32_MAX || ld > PR_INT32_MAX || n * ld > PR_INT32_MAX) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": n * ld beyond int32 indexing");
  if(!pose) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": pose is NULL");
  if(mixture && pr->M == 0) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": this prior has no mixture");
  if(limit && !pr->limits) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": this prior has no limits");
  return check_space(space, fn);
}
} // namespace smplpp_hip

using namespace smplpp_hip;

// Validate and build the host tables (pose_prior_tables.h), then upload them.
extern "C" int smplpp_pose_prior_create(int device, int64_t M, int64_t D, const float * mean, const float * mat, const float * offset,
                                        const float * lo, const float * hi, const float * limit_weight, struct smplpp_pose_prior ** out)
{
  const char * fn = "smplpp_pose_prior_create";
  if(!out) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": no out");
  *out = nullptr;
  const PosePriorTables t = pose_prior_tables(M, D, mean, mat, offset, lo, hi, limit_weight);
  if(t.refusal) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": " + t.refusal);
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<PosePrior> pr(new PosePrior());
  pr->device = device, pr->M = t.M, pr->D = t.D, pr->limits = t.limits;
  HIP_TRY(pr_upload(pr->mean, t.mean));
  HIP_TRY(pr_upload(pr->mat, t.mat));
  HIP_TRY(pr_upload(pr->matT, t.matT));
  HIP_TRY(pr_upload(pr->offset, t.offset));
  HIP_TRY(pr_upload(pr->lo, t.lo));
  HIP_TRY(pr_upload(pr->hi, t.hi));
  HIP_TRY(pr_upload(pr->weight, t.weight));
  *out = pr.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_pose_prior_destroy(struct smplpp_pose_prior * pr)
{
  if(!pr) return SMPLPP_OK;
  (void)hipSetDevice(pr->device);
  delete pr;
  return SMPLPP_OK;
}

extern "C" int smplpp_pose_prior_info(const struct smplpp_pose_prior * pr, int64_t * M, int64_t * D, int * has_limits)
{
  if(!pr) return fail(SMPLPP_ERR_INVALID, "smplpp_pose_prior_info: no prior");
  if(M) *M = pr->M;
  if(D) *D = pr->D;
  if(has_limits) *has_limits = pr->limits ? 1 : 0;
  return SMPLPP_OK;
}

extern "C" int smplpp_pose_prior(struct smplpp_pose_prior * pr, int64_t n, const float * pose, int64_t ld, float * energy,
                                 int64_t * component, float * residual, float * limit_energy, int space, void * stream)
{
  const char * fn = "smplpp_pose_prior";
  const bool mixture = energy || component || residual;
  if(int rc = pr_check(fn, pr, n, pose, ld, mixture, limit_energy != nullptr, space)) return rc;
  if(!mixture && !limit_energy) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": every output is NULL");
  const size_t lds = sizeof(float) * pr_lds_floats(pr->M, pr->D, residual != nullptr);
  static PerDeviceOnce once;
  Frame fr(pr->device, &pr->arena, space, stream, "pose prior");
  const float * p = fr.in(pose, (size_t)((n - 1) * ld + pr->D));
  float * e = fr.out(energy, (size_t)n);
  int64_t * c = fr.out(component, (size_t)n);
  float * r = fr.out(residual, (size_t)(n * pr->D));
  float * l = fr.out(limit_energy, (size_t)n);
  return fr.run([&] {
    HIP_TRY(lds_opt_in(once, pr->device, reinterpret_cast<const void *>(&prior_forward_kernel), PR_LDS_MAX));
    prior_forward_kernel<<<dim3((unsigned)((n + PR_FT - 1) / PR_FT)), dim3(PR_T), lds, fr.st>>>(pr_tables(pr), p, ld, n, e, c, r, l);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}

extern "C" int smplpp_pose_prior_vjp(struct smplpp_pose_prior * pr, int64_t n, const float * pose, int64_t ld, const int64_t * component,
                                     const float * grad_energy, const float * grad_residual, const float * grad_limit_energy,
                                     float * grad_pose, int accumulate, int space, void * stream)
{
  const char * fn = "smplpp_pose_prior_vjp";
  const bool mixture = grad_energy || grad_residual;
  if(int rc = pr_check(fn, pr, n, pose, ld, mixture, grad_limit_energy != nullptr, space)) return rc;
  if(!mixture && !grad_limit_energy) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": every cotangent is NULL");
  if(!grad_pose) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": grad_pose is NULL");
  if(accumulate != 0 && accumulate != 1) return fail(SMPLPP_ERR_INVALID, std::string(fn) + ": accumulate must be 0 or 1");
  if(mixture && component && space == SMPLPP_HOST) // (without a mixture cotangent the array is not read, in either space)
    if(int rc = ids_in(fn, "component", component, n, 0, pr->M)) return rc;
  const size_t rows = (size_t)((n - 1) * ld + pr->D);
  Frame fr(pr->device, &pr->arena, space, stream, "pose prior VJP");
  const float * p = fr.in(pose, rows);
  const int64_t * c = mixture ? fr.in(component, (size_t)n) : nullptr;
  const float * ge = fr.in(grad_energy, (size_t)n);
  const float * gr = fr.in(grad_residual, (size_t)(n * pr->D));
  const float * gl = fr.in(grad_limit_energy, (size_t)n);
  // (a host-space row's floats past D travel with it: they are loaded so that the copy back leaves them as they were)
  float * gp = fr.out(grad_pose, rows, accumulate || ld > pr->D);
  return fr.run([&] {
    prior_vjp_kernel<<<dim3((unsigned)((n + PR_FT - 1) / PR_FT)), dim3(PR_T), sizeof(float) * pr_lds_floats(pr->M, pr->D, false), fr.st>>>(
        pr_tables(pr), p, ld, n, c, ge, gr, gl, gp, accumulate);
    HIP_TRY(hipGetLastError());
    return (int)SMPLPP_OK;
  });
}
