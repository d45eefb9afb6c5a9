// smplpp_vposer_vjp: the vector-Jacobian product of the VPoser decoder (dL/dout [n,21,3] -> dL/dz [n,32]), what the reference gets
// from libtorch autograd through vposer->forward(latent) in its capture loop (node/node.cpp:761-772).
//
// Per frame, with s0, s1 the LeakyReLU slopes (1 or 0.01) of layers 0 and 1 and o the layer-2 output [126]:
//   g_o6[j] = (d aa_j / d o6_j)^T g_aa[j]      per joint, the dual numbers of vposer_tail.h (the Jacobian kernel's own code)
//   g2      = s1 (.) (W2^T g_o)                 126 -> 512
//   g1      = s0 (.) (W1^T g2)                  512 -> 512
//   g_z     = W0^T g1                           512 -> 32       (dropout is the identity: eval)
//
// Kernels, both on the caller's stream:
//  vposer_kernel<true>   (vposer.hip) the value-only forward smplpp_vposer_forward runs when jac is NULL, with the same arithmetic,
//                        also storing s0, s1 and o into the backward's workspace: the masks and the axis-angle branches are the
//                        ones the caller's loss saw, and `out` is that call's bits.
//  vposer_vjp_kernel     VV_NF frames per workgroup, exact fp32 on the VALU: every weight the workgroup streams from L2 serves
//                        VV_NF frames.  Weights are read from the decoder's copies in [out][in] layout (vposer_weight_rows, built
//                        by the first backward call that needs them), so that consecutive lanes read consecutive inputs.
// No atomics; every sum runs in a fixed order that does not depend on the frame's slot in its workgroup, on n or on frame_base:
// a frame's bits are the same in any batch or shard.
#include "staging.h"

#pragma clang fp contract(on) // contraction decided by the source (vposer.hip)

#include "vposer_state.h"
#include "vposer_tail.h"

namespace smplpp_hip
{
constexpr int VV_NF = 8; // frames per workgroup of vposer_vjp_kernel

// [in][out] -> [out][in]
__global__ void vposer_untranspose_kernel(const float * __restrict__ src, float * __restrict__ dst, int in, int out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= in * out) return;
  const int o = i / in, k = i % in;
  dst[i] = src[k * out + o];
}

// dst [out][in] from src [in][out] on the null stream (dst null: nothing to build)
static void untranspose(const float * src, float * dst, int in, int out)
{
  if(dst) vposer_untranspose_kernel<<<dim3((in * out + 255) / 256), dim3(256), 0, nullptr>>>(src, dst, in, out);
}

int vposer_weight_rows(smplpp_vposer * v, bool all3)
{
  if(v->w0r && (!all3 || (v->w1r && v->w2r))) return SMPLPP_OK;
  DevPtr<float> w0, w1, w2; // the missing copies, handed to the decoder once complete
  if(!v->w0r) HIP_TRY(dev_alloc(w0, (size_t)HID * LAT));
  if(all3 && !v->w1r) HIP_TRY(dev_alloc(w1, (size_t)HID * HID));
  if(all3 && !v->w2r) HIP_TRY(dev_alloc(w2, (size_t)OUT6 * HID));
  untranspose(v->w0t.get(), w0.get(), LAT, HID);
  untranspose(v->w1t.get(), w1.get(), HID, HID);
  untranspose(v->w2t.get(), w2.get(), HID, OUT6);
  // waited for once, here: a later call on any stream finds the copies complete
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  if(w0) v->w0r = std::move(w0);
  if(w1) v->w1r = std::move(w1);
  if(w2) v->w2r = std::move(w2);
  return SMPLPP_OK;
}

// grid: ceil(n / VV_NF) workgroups of 256.  LDS holds the gradients of the workgroup's frames as [row][VV_NF], so a weight's VV_NF
// products read one broadcast pair of 16-byte words.
__global__ __launch_bounds__(256) void vposer_vjp_kernel(const float * __restrict__ ws, const float * __restrict__ gout,
                                                         const float * __restrict__ w0, const float * __restrict__ w1,
                                                         const float * __restrict__ w2, float * __restrict__ gz, int64_t n)
{
  __shared__ __attribute__((aligned(16))) float sO[OUT6 * VV_NF]; // g_o
  __shared__ __attribute__((aligned(16))) float sG2[HID * VV_NF]; // g2 (times s1)
  __shared__ __attribute__((aligned(16))) float sG1[HID * VV_NF]; // g1 (times s0)
  const int tid = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * VV_NF;

  // rotation tail, one thread per (frame, joint): the 3 x 6 Jacobian of the joint's axis-angle, transposed onto its gradient
  if(tid < VV_NF * 21)
  {
    const int q = tid / 21, j = tid % 21;
    const int64_t f = f0 + q;
    float g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if(f < n)
    {
      float o6[6], aa[3], jac[18], ga[3];
      for(int k = 0; k < 6; k++) o6[k] = ws[f * VW_FRAME + VW_O6 + j * 6 + k];
      for(int i = 0; i < 3; i++) ga[i] = gout[f * 63 + j * 3 + i];
      sixd_to_aa(o6, aa, jac);
      for(int k = 0; k < 6; k++) g6[k] = (jac[k] * ga[0] + jac[6 + k] * ga[1]) + jac[12 + k] * ga[2];
    }
    for(int k = 0; k < 6; k++) sO[(j * 6 + k) * VV_NF + q] = g6[k];
  }
  __syncthreads();

  // One transposed layer: rows 2 tid, 2 tid + 1 of W^T (columns of W [K][512]) for the VV_NF frames, k in ascending order; the
  // next KU weight pairs are in flight while the current ones are used (KU x 2 VV_NF FMAs per wait: enough to cover an L2 trip).
  auto layerT = [&](const float * __restrict__ w, const float * __restrict__ sIn, int K, float (&acc)[2][VV_NF]) {
#pragma unroll
    for(int q = 0; q < VV_NF; q++) acc[0][q] = acc[1][q] = 0.0f;
    constexpr int KU = 32;
    float2 wv[KU], wn[KU];
#pragma unroll
    for(int u = 0; u < KU; u++) wv[u] = u < K ? *reinterpret_cast<const float2 *>(w + (size_t)u * HID + 2 * tid) : make_float2(0.f, 0.f);
#pragma nounroll
    for(int k0 = 0; k0 < K; k0 += KU)
    {
#pragma unroll
      for(int u = 0; u < KU; u++)
      {
        const int kn = k0 + KU + u;
        wn[u] = kn < K ? *reinterpret_cast<const float2 *>(w + (size_t)kn * HID + 2 * tid) : make_float2(0.f, 0.f);
      }
#pragma unroll
      for(int u = 0; u < KU; u++)
      {
        if(k0 + u < K)
        {
          const float4 ga = *reinterpret_cast<const float4 *>(sIn + (k0 + u) * VV_NF);
          const float4 gb = *reinterpret_cast<const float4 *>(sIn + (k0 + u) * VV_NF + 4);
          const float g[VV_NF] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
#pragma unroll
          for(int q = 0; q < VV_NF; q++)
          {
            acc[0][q] += wv[u].x * g[q];
            acc[1][q] += wv[u].y * g[q];
          }
        }
      }
#pragma unroll
      for(int u = 0; u < KU; u++) wv[u] = wn[u];
    }
  };
  // times the slopes of the layer below, into LDS as [row][VV_NF]
  auto store = [&](const float (&acc)[2][VV_NF], int slope_off, float * sOut) {
    float s[2][VV_NF];
#pragma unroll
    for(int q = 0; q < VV_NF; q++)
    {
      const int64_t f = f0 + q;
      const float2 sl = f < n ? *reinterpret_cast<const float2 *>(ws + f * VW_FRAME + slope_off + 2 * tid) : make_float2(0.f, 0.f);
      s[0][q] = acc[0][q] * sl.x;
      s[1][q] = acc[1][q] * sl.y;
    }
#pragma unroll
    for(int r = 0; r < 2; r++)
    {
      float4 * p = reinterpret_cast<float4 *>(sOut + (2 * tid + r) * VV_NF);
      p[0] = make_float4(s[r][0], s[r][1], s[r][2], s[r][3]);
      p[1] = make_float4(s[r][4], s[r][5], s[r][6], s[r][7]);
    }
  };
  {
    float acc[2][VV_NF];
    layerT(w2, sO, OUT6, acc); // W2 [126][512]
    store(acc, VW_S1, sG2);
  }
  __syncthreads();
  {
    float acc[2][VV_NF];
    layerT(w1, sG2, HID, acc); // W1 [512][512]
    store(acc, VW_S0, sG1);
  }
  __syncthreads();

  // layer 0: thread (slice ks of 64 rows, latent c) for all VV_NF frames, its 64 weights requested at once; the eight slices'
  // partial sums meet in LDS (sG2 is dead) and are added in a fixed tree order by thread (frame q, latent c)
  {
    const int c = tid & 31, ks = tid >> 5;
    float wk[HID / 8];
#pragma unroll
    for(int u = 0; u < HID / 8; u++) wk[u] = w0[(ks * (HID / 8) + u) * LAT + c];
    float a[VV_NF];
#pragma unroll
    for(int q = 0; q < VV_NF; q++) a[q] = 0.0f;
#pragma unroll
    for(int u = 0; u < HID / 8; u++)
    {
      const float * gk = sG1 + (ks * (HID / 8) + u) * VV_NF;
      const float4 ga = *reinterpret_cast<const float4 *>(gk), gb = *reinterpret_cast<const float4 *>(gk + 4);
      const float g[VV_NF] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
#pragma unroll
      for(int q = 0; q < VV_NF; q++) a[q] += wk[u] * g[q];
    }
    float * part = sG2; // [8 slices][VV_NF][32]
#pragma unroll
    for(int q = 0; q < VV_NF; q++) part[(ks * VV_NF + q) * LAT + c] = a[q];
    __syncthreads();
    const int q = tid >> 5;
    const float * p = sG2 + q * LAT + c;
    constexpr int SS = VV_NF * LAT; // stride between slices
    const float sum = ((p[0] + p[SS]) + (p[2 * SS] + p[3 * SS])) + ((p[4 * SS] + p[5 * SS]) + (p[6 * SS] + p[7 * SS]));
    const int64_t f = f0 + q;
    if(f < n) gz[f * LAT + c] = sum;
  }
}
static_assert(VV_NF * LAT == 256 && 8 * LAT == 256, "layer 0 of vposer_vjp_kernel maps one thread to each (slice, latent), then to each (frame, latent)");
static_assert(VV_NF * 21 <= 256, "the rotation tail of vposer_vjp_kernel maps one thread to each (frame, joint)");
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" int smplpp_vposer_vjp(smplpp_vposer * v, int64_t n, int64_t frame_base, const float * z, const float * grad_out,
                                 float * grad_z, float * out, int space, void * stream)
{
  if(!v || n <= 0 || frame_base < 0 || !z || !grad_out || !grad_z) return fail(SMPLPP_ERR_INVALID, "smplpp_vposer_vjp: bad argument");
  if(n > 0x7fffffffLL) return fail(SMPLPP_ERR_INVALID, "smplpp_vposer_vjp: too many frames");
  int rc = check_space(space, "smplpp_vposer_vjp");
  if(rc) return rc;
  Frame fr(v->device, &v->arena, space, stream, nullptr);
  if(!fr.ok()) return fr.finish();
  rc = vposer_weight_rows(v, true);
  if(rc) return rc;
  HIP_TRY(v->vjp_ws.reserve(sizeof(float) * (size_t)n * VW_FRAME));
  const float * zi = fr.in(z, (size_t)n * LAT);
  const float * gi = fr.in(grad_out, (size_t)n * 63);
  float * gzo = fr.out(grad_z, (size_t)n * LAT);
  float * oo = fr.out(out, (size_t)n * 63);
  return fr.run([&]() -> int {
    int rc = vposer_value_device(v, n, zi, oo, v->vjp_ws.as<float>(), fr.st);
    if(rc) return rc;
    vposer_vjp_kernel<<<dim3((unsigned)((n + VV_NF - 1) / VV_NF)), dim3(256), 0, fr.st>>>(v->vjp_ws.as<float>(), gi, v->w0r.get(), v->w1r.get(),
                                                                                         v->w2r.get(), gzo, n);
    HIP_TRY(hipGetLastError());
    return SMPLPP_OK;
  });
}
