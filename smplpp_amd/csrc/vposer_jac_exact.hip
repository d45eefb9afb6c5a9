// smplpp_vposer_jacobian: d(out)/dz [n,63,32] of the VPoser decoder in exact fp32, what the reference gets from libtorch autograd
// through vposer->forward(latent) in its capture loop (node/node.cpp:761-772).
//
// Per frame, with s0, s1 the LeakyReLU slopes (1 or 0.01) of layers 0 and 1 and o6 the layer-2 output [126]:
//   T0 = diag(s0) W0            [512 x 32]
//   T1 = diag(s1) (W1 T0)       [512 x 32]   512 . 512 . 32 MACs per frame: the hot product
//   T2 = W2 T1                  [126 x 32]
//   jac[3j..3j+2, :] = (d aa_j / d o6_j) T2[6j..6j+5, :]   per joint, the dual numbers of vposer_tail.h at o6
//
// Kernels, all on the caller's stream:
//  vposer_kernel<true>        (vposer.hip) the value-only forward smplpp_vposer_forward runs when jac is NULL, storing s0, s1 and o6
//                             into the workspace: `out` is that call's bits, and the masks and branches are the ones a loss on it saw.
//  vposer_jx_layer1_kernel    T1 on v_mfma_f32_32x32x2_f32 (exact fp32 products, a k-ordered fmaf chain).  A workgroup is NF frames
//                             x 128 rows: each wave owns one 32-row tile of W1, streamed from L2 once for the NF frames; the B operand
//                             s0 (.) W0 is formed in registers from the one W0 stream and the frame's slopes (staged in LDS).
//  vposer_jx_tail_kernel      one frame per workgroup: T2 on the same instruction (a wave per 32-row tile), the rotation tail, the store.
// No atomics.  Every element of T1, T2 and jac is one chain over k in ascending order: a frame's bits do not depend on n,
// frame_base, NF or the workgroup it lands in.
#include "staging.h"

#pragma clang fp contract(on) // contraction decided by the source (vposer.hip)

#include "vposer_state.h"
#include "vposer_tail.h"

namespace smplpp_hip
{
typedef float jx_f32x16 __attribute__((ext_vector_type(16)));
constexpr int JX_ROWS = 128;          // layer-1 rows per workgroup of vposer_jx_layer1_kernel (4 waves x 32)
constexpr int JX_T1 = HID * LAT;      // floats of one frame's T1
constexpr int JX_PF = 16;             // k-steps whose operands are in flight

struct VPoserJxWork
{
  DevBuf ws; // [n][VW_FRAME] of vposer_kernel<true>
  DevBuf t1; // [n][512][32] T1
};

void StateDelete::operator()(VPoserJxWork * w) const
{
  delete w;
}

// grid (ceil(n / NF), HID / JX_ROWS), block 256.  Lane l of wave w: r = l & 31, h = l >> 5.  At k-step ks (k = 2 ks + h):
//   A[r][h] = W1[row][k]            row = 128 blockIdx.y + 32 w + r   (w1t [in][out]: lanes read consecutive rows)
//   B[h][r] = s0[f][k] * W0[k][r]                                     (w0r [512][32]: lanes read consecutive columns)
// C/D: column r, row (g & 3) + 8 (g >> 2) + 4 h of the tile in register g.
template<int NF>
__global__ __launch_bounds__(256) void vposer_jx_layer1_kernel(const float * __restrict__ ws, const float * __restrict__ w1t,
                                                               const float * __restrict__ w0r, float * __restrict__ t1, int64_t n)
{
  __shared__ __attribute__((aligned(16))) float sS0[HID * NF]; // [k][NF] the slopes of layer 0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t f0 = (int64_t)blockIdx.x * NF;
  for(int i = tid; i < HID * NF; i += 256)
  {
    const int q = i / HID, k = i % HID;
    sS0[k * NF + q] = f0 + q < n ? ws[(f0 + q) * VW_FRAME + VW_S0 + k] : 0.0f;
  }
  __syncthreads();
  const int row = blockIdx.y * JX_ROWS + wave * 32 + r;
  const float * ap = w1t + (size_t)h * HID + row;
  const float * bp = w0r + h * LAT + r;
  jx_f32x16 acc[NF];
#pragma unroll
  for(int q = 0; q < NF; q++)
#pragma unroll
    for(int g = 0; g < 16; g++) acc[q][g] = 0.0f;
  float a[JX_PF], b[JX_PF], an[JX_PF], bn[JX_PF];
#pragma unroll
  for(int u = 0; u < JX_PF; u++)
  {
    a[u] = ap[(size_t)(2 * u) * HID];
    b[u] = bp[(2 * u) * LAT];
  }
#pragma nounroll
  for(int ks0 = 0; ks0 < HID / 2; ks0 += JX_PF)
  {
    const int kn = ks0 + JX_PF < HID / 2 ? ks0 + JX_PF : ks0; // the last batch loads its own operands once more (in bounds)
#pragma unroll
    for(int u = 0; u < JX_PF; u++)
    {
      an[u] = ap[(size_t)(2 * (kn + u)) * HID];
      bn[u] = bp[(2 * (kn + u)) * LAT];
    }
#pragma unroll
    for(int u = 0; u < JX_PF; u++)
    {
      const float * sp = sS0 + (2 * (ks0 + u) + h) * NF;
      float s0[NF];
      if constexpr(NF >= 4)
      {
#pragma unroll
        for(int q4 = 0; q4 < NF; q4 += 4)
        {
          const float4 v4 = *reinterpret_cast<const float4 *>(sp + q4);
          s0[q4] = v4.x;
          s0[q4 + 1] = v4.y;
          s0[q4 + 2] = v4.z;
          s0[q4 + 3] = v4.w;
        }
      }
      else
      {
#pragma unroll
        for(int q = 0; q < NF; q++) s0[q] = sp[q];
      }
#pragma unroll
      for(int q = 0; q < NF; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], s0[q] * b[u], acc[q], 0, 0, 0);
    }
#pragma unroll
    for(int u = 0; u < JX_PF; u++)
    {
      a[u] = an[u];
      b[u] = bn[u];
    }
  }
  // times the slopes of layer 1, into T1 [f][512][32]
  const int tile0 = blockIdx.y * JX_ROWS + wave * 32;
#pragma unroll
  for(int q = 0; q < NF; q++)
  {
    const int64_t f = f0 + q;
    if(f >= n) break;
#pragma unroll
    for(int g = 0; g < 16; g++)
    {
      const int rr = tile0 + (g & 3) + 8 * (g >> 2) + 4 * h;
      t1[(f * HID + rr) * LAT + r] = acc[q][g] * ws[f * VW_FRAME + VW_S1 + rr];
    }
  }
}
static_assert(HID % JX_ROWS == 0 && (HID / 2) % JX_PF == 0, "vposer_jx_layer1_kernel tiles layer 1 exactly");

// grid n, block 256.  Wave w: T2 rows 32 w + r (A[r][h] = W2[row][k], zero for the padding rows 126, 127), B[h][r] = T1[f][k][r].
__global__ __launch_bounds__(256) void vposer_jx_tail_kernel(const float * __restrict__ ws, const float * __restrict__ t1,
                                                             const float * __restrict__ w2t, float * __restrict__ jac)
{
  __shared__ float sT[OUT6 * 33];  // T2 [126][32] (rows padded to 33)
  __shared__ float sJ[21 * 18];    // per joint d aa / d o6 [3][6]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t f = blockIdx.x;
  if(tid < 21) // the rotation tail's 3 x 6 Jacobian of joint tid at this frame's o6
  {
    float o6[6], aa[3], jc[18];
    for(int k = 0; k < 6; k++) o6[k] = ws[f * VW_FRAME + VW_O6 + tid * 6 + k];
    sixd_to_aa(o6, aa, jc);
    for(int i = 0; i < 18; i++) sJ[tid * 18 + i] = jc[i];
  }
  {
    const int row = wave * 32 + r;
    const bool live = row < OUT6;
    const float * ap = w2t + (size_t)h * OUT6 + (live ? row : 0);
    const float * bp = t1 + f * JX_T1 + h * LAT + r;
    jx_f32x16 acc;
#pragma unroll
    for(int g = 0; g < 16; g++) acc[g] = 0.0f;
    float a[JX_PF], b[JX_PF], an[JX_PF], bn[JX_PF];
#pragma unroll
    for(int u = 0; u < JX_PF; u++)
    {
      a[u] = live ? ap[(size_t)(2 * u) * OUT6] : 0.0f;
      b[u] = bp[(2 * u) * LAT];
    }
#pragma nounroll
    for(int ks0 = 0; ks0 < HID / 2; ks0 += JX_PF)
    {
      const int kn = ks0 + JX_PF < HID / 2 ? ks0 + JX_PF : ks0;
#pragma unroll
      for(int u = 0; u < JX_PF; u++)
      {
        an[u] = live ? ap[(size_t)(2 * (kn + u)) * OUT6] : 0.0f;
        bn[u] = bp[(2 * (kn + u)) * LAT];
      }
#pragma unroll
      for(int u = 0; u < JX_PF; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
#pragma unroll
      for(int u = 0; u < JX_PF; u++)
      {
        a[u] = an[u];
        b[u] = bn[u];
      }
    }
#pragma unroll
    for(int g = 0; g < 16; g++)
    {
      const int rr = wave * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
      if(rr < OUT6) sT[rr * 33 + r] = acc[g];
    }
  }
  __syncthreads();
  // one thread per (joint, latent column): the joint's six T2 entries of the column once for its three output rows
  for(int item = tid; item < 21 * LAT; item += 256)
  {
    const int j = item / LAT, c = item % LAT;
    float t6[6];
#pragma unroll
    for(int k = 0; k < 6; k++) t6[k] = sT[(j * 6 + k) * 33 + c];
#pragma unroll
    for(int i = 0; i < 3; i++)
    {
      float s = 0.f;
#pragma unroll
      for(int k = 0; k < 6; k++) s += sJ[j * 18 + i * 6 + k] * t6[k];
      jac[(f * 63 + j * 3 + i) * LAT + c] = s;
    }
  }
}
static_assert(OUT6 <= 4 * 32, "vposer_jx_tail_kernel: four 32-row tiles cover layer 2");

int vposer_jacobian_device(smplpp_vposer * v, StatePtr<VPoserJxWork> & work, int64_t n, const float * z, int64_t z_stride, float * out,
                           int64_t out_stride, float * jac, hipStream_t st)
{
  int rc = vposer_weight_rows(v, false);
  if(rc) return rc;
  if(!work) work.reset(new VPoserJxWork());
  VPoserJxWork * w = work.get();
  HIP_TRY(w->ws.reserve(sizeof(float) * (size_t)n * VW_FRAME));
  HIP_TRY(w->t1.reserve(sizeof(float) * (size_t)n * JX_T1));
  float * ws = w->ws.as<float>();
  float * t1 = w->t1.as<float>();
  rc = vposer_value_device(v, n, z, out, ws, st, z_stride, out_stride);
  if(rc) return rc;
  // frames per workgroup: as many as still give about four waves per SIMD (fewer frames: layer 1's rows spread over more CUs)
  const int64_t want = 16LL * device_cus(v->device);
  const int nf = n * 16 / 8 >= want ? 8 : n * 16 / 4 >= want ? 4 : n * 16 / 2 >= want ? 2 : 1;
  const unsigned groups = (unsigned)((n + nf - 1) / nf);
  const dim3 grid(groups, HID / JX_ROWS), block(256);
  if(nf == 8)
    vposer_jx_layer1_kernel<8><<<grid, block, 0, st>>>(ws, v->w1t.get(), v->w0r.get(), t1, n);
  else if(nf == 4)
    vposer_jx_layer1_kernel<4><<<grid, block, 0, st>>>(ws, v->w1t.get(), v->w0r.get(), t1, n);
  else if(nf == 2)
    vposer_jx_layer1_kernel<2><<<grid, block, 0, st>>>(ws, v->w1t.get(), v->w0r.get(), t1, n);
  else
    vposer_jx_layer1_kernel<1><<<grid, block, 0, st>>>(ws, v->w1t.get(), v->w0r.get(), t1, n);
  HIP_TRY(hipGetLastError());
  vposer_jx_tail_kernel<<<dim3((unsigned)n), block, 0, st>>>(ws, t1, v->w2t.get(), jac);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_vposer_jacobian(smplpp_vposer * v, int64_t n, int64_t frame_base, const float * z, float * out, float * jac,
                                      int space, void * stream)
{
  if(!v || n <= 0 || frame_base < 0 || !z || !jac) return fail(SMPLPP_ERR_INVALID, "smplpp_vposer_jacobian: bad argument");
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, "smplpp_vposer_jacobian: too many frames");
  int rc = check_space(space, "smplpp_vposer_jacobian");
  if(rc) return rc;
  Frame fr(v->device, &v->arena, space, stream, nullptr);
  const float * zi = fr.in(z, (size_t)n * LAT);
  float * jo = fr.out(jac, (size_t)n * 63 * LAT);
  float * oo = fr.out(out, (size_t)n * 63);
  return fr.run([&] { return vposer_jacobian_device(v, v->jx, n, zi, LAT, oo, 63, jo, fr.st); });
}
