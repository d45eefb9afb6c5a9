// The VPoser decoder handle (vposer.hip) and its shapes, shared by the forward (vposer.hip) and its backward (vposer_vjp.hip).
#pragma once
#include "common.h"

struct smplpp_vposer
{
  int device = 0;
  smplpp_hip::DevPtr<float> w0t, b0, w1t, b1, w2t, b2;
  // layers 1 and 2 once more as fp16x2 pieces in MFMA fragment order (the A operand of the tangent GEMMs, layout below)
  smplpp_hip::DevPtr<uint8_t> w1h, w2h;
  float sW1 = 1.f, sW2 = 1.f, sD1 = 1.f, sD2 = 1.f; // power-of-two scales: weights of layers 1 / 2, tangent blocks of layers 0 / 1
  // vposer_jac2_kernel (several frames per workgroup): W0 once more as the B operand of layer 1's tangent GEMM (fragment order,
  // scale sD1, no slopes) and the constant product C10 = W1 . W0 [512][32] (fp32, from an fp64 sum on the host)
  smplpp_hip::DevPtr<uint8_t> w0h;
  smplpp_hip::DevPtr<float> c10;
  // the backward calls (smplpp_vposer_vjp, smplpp_vposer_jacobian): W0 [512][32], W1 [512][512], W2 [126][512] once more in
  // torch::nn::Linear's [out][in] layout, each null until the first call that reads it (vposer_weight_rows)
  smplpp_hip::DevPtr<float> w0r, w1r, w2r;
  smplpp_hip::DevBuf vjp_ws; // smplpp_vposer_vjp's workspace: [n][VW_FRAME] of vposer_kernel<true>
  smplpp_hip::StatePtr<smplpp_hip::VPoserJxWork> jx; // smplpp_vposer_jacobian's workspace: null until its first call on the decoder
  smplpp_hip::Arena arena;   // staging of the host-space calls on this decoder
  ~smplpp_vposer(); // (vposer.hip)
};

namespace smplpp_hip
{
constexpr int LAT = SMPLPP_LATENT_DIM; // 32
constexpr int HID = 512;               // VPoser.h hiddenDim_
constexpr int OUT6 = 126;              // 6 * 21

// Value-only decoder (vposer_kernel, exact fp32): what smplpp_vposer_forward runs when jac is NULL.  ws (nullable) [n][VW_FRAME]:
// per frame the LeakyReLU slopes of layers 0 and 1 and the layer-2 output, as the backward reads them (vposer_vjp.hip).
constexpr int VW_S0 = 0, VW_S1 = HID, VW_O6 = 2 * HID, VW_FRAME = 2 * HID + 128;
// z_stride / out_stride: floats between frames of z and out (a splice into a wider layout, e.g. the IK solver's theta25)
int vposer_value_device(smplpp_vposer * v, int64_t n, const float * z, float * out, float * ws, hipStream_t st, int64_t z_stride = LAT,
                        int64_t out_stride = 63);

// Builds the decoder's missing [out][in] weight copies: w0r, and w1r and w2r too when all3 (vposer_vjp.hip); returns at once when
// they exist
int vposer_weight_rows(smplpp_vposer * v, bool all3);

// Exact-fp32 d(out)/dz [n][63][32] (vposer_jac_exact.hip) at the decode vposer_value_device gives, which it also writes to out
// (nullable).  work: the caller's workspace, created on first use (work null) and grown to n.
int vposer_jacobian_device(smplpp_vposer * v, StatePtr<VPoserJxWork> & work, int64_t n, const float * z, int64_t z_stride, float * out,
                           int64_t out_stride, float * jac, hipStream_t st);
} // namespace smplpp_hip
