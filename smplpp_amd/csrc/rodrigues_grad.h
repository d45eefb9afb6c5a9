// The derivative of the reference's Rodrigues form, shared by the IK evaluation (ik_eval.h) and the FK backward (fk_vjp.hip).
#pragma once

#include "common.h"

namespace smplpp_hip
{
// derivative of Rodrigues (src/BlendShape.cpp:813-841) wrt theta_m, including the ||theta + eps|| angle
__device__ inline void rodrigues_grad_dev(const float * th, int m, float * dR)
{
  const float eps = 1e-8f;
  const float ae0 = th[0] + eps, ae1 = th[1] + eps, ae2 = th[2] + eps;
  const float a = sqrtf(ae0 * ae0 + ae1 * ae1 + ae2 * ae2);
  const float s = sinf(a), c = cosf(a);
  const float k[3] = {th[0] / a, th[1] / a, th[2] / a};
  const float K[9] = {0.f, -k[2], k[1], k[2], 0.f, -k[0], -k[1], k[0], 0.f};
  const float aem = (m == 0) ? ae0 : (m == 1 ? ae1 : ae2);
  const float da = aem / a;
  float dk[3];
  for(int x = 0; x < 3; x++) dk[x] = ((x == m) ? 1.0f : 0.0f) / a - th[x] * da / (a * a);
  const float dK[9] = {0.f, -dk[2], dk[1], dk[2], 0.f, -dk[0], -dk[1], dk[0], 0.f};
  for(int r = 0; r < 3; r++)
    for(int cc = 0; cc < 3; cc++)
    {
      float kk = 0.f, d1 = 0.f, d2 = 0.f;
      for(int q = 0; q < 3; q++)
      {
        kk += K[r * 3 + q] * K[q * 3 + cc];
        d1 += dK[r * 3 + q] * K[q * 3 + cc];
        d2 += K[r * 3 + q] * dK[q * 3 + cc];
      }
      dR[r * 3 + cc] = dK[r * 3 + cc] * s + K[r * 3 + cc] * c * da + (d1 + d2) * (1.0f - c) + kk * s * da;
    }
}
} // namespace smplpp_hip
