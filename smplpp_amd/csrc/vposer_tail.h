// The rotation tail of the VPoser decoder (src/VPoser.cpp:25-141) as dual numbers: Gram-Schmidt of a joint's 6D output and
// convertRotMatToAxisAngle, value and derivative with the reference's branches.  Shared by the forward + Jacobian kernels
// (vposer.hip) and the vector-Jacobian product (vposer_vjp.hip), so both take the same branches with the same arithmetic.
#pragma once
#include <cfloat>
#include <cmath>

namespace smplpp_hip
{
// dual number: a value and ND directional derivatives (ND = 6: all six inputs of a joint at once; ND = 1: one direction per
// thread — the components never mix, so both give the same bits)
template<int ND>
struct DN
{
  float v;
  float d[ND];
};
typedef DN<6> D6;
template<int ND>
__device__ inline DN<ND> mk(float v)
{
  DN<ND> r;
  r.v = v;
  for(int i = 0; i < ND; i++) r.d[i] = 0.f;
  return r;
}
template<int ND>
__device__ inline DN<ND> operator+(const DN<ND> & a, const DN<ND> & b)
{
  DN<ND> r;
  r.v = a.v + b.v;
  for(int i = 0; i < ND; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template<int ND>
__device__ inline DN<ND> operator-(const DN<ND> & a, const DN<ND> & b)
{
  DN<ND> r;
  r.v = a.v - b.v;
  for(int i = 0; i < ND; i++) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template<int ND>
__device__ inline DN<ND> operator*(const DN<ND> & a, const DN<ND> & b)
{
  DN<ND> r;
  r.v = a.v * b.v;
  for(int i = 0; i < ND; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template<int ND>
__device__ inline DN<ND> operator/(const DN<ND> & a, const DN<ND> & b)
{
  DN<ND> r;
  r.v = a.v / b.v;
  for(int i = 0; i < ND; i++) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
  return r;
}
template<int ND>
__device__ inline DN<ND> operator*(float s, const DN<ND> & a)
{
  DN<ND> r;
  r.v = s * a.v;
  for(int i = 0; i < ND; i++) r.d[i] = s * a.d[i];
  return r;
}
template<int ND>
__device__ inline DN<ND> operator+(const DN<ND> & a, float s)
{
  DN<ND> r = a;
  r.v += s;
  return r;
}
template<int ND>
__device__ inline DN<ND> neg(const DN<ND> & a)
{
  return -1.0f * a;
}
template<int ND>
__device__ inline DN<ND> dsqrt(const DN<ND> & a)
{
  DN<ND> r;
  r.v = sqrtf(a.v);
  for(int i = 0; i < ND; i++) r.d[i] = a.d[i] / (2.0f * r.v);
  return r;
}
template<int ND>
__device__ inline DN<ND> dacos(const DN<ND> & a)
{
  DN<ND> r;
  r.v = acosf(a.v);
  const float g = -1.0f / sqrtf(1.0f - a.v * a.v);
  for(int i = 0; i < ND; i++) r.d[i] = g * a.d[i];
  return r;
}
template<int ND>
__device__ inline DN<ND> dsin(const DN<ND> & a)
{
  DN<ND> r;
  r.v = sinf(a.v);
  const float c = cosf(a.v);
  for(int i = 0; i < ND; i++) r.d[i] = c * a.d[i];
  return r;
}
// torch::nn::functional::normalize of a 3-vector: x / max(||x||, 1e-12) (clamp_min passes no gradient when active)
template<int ND>
__device__ inline void dnormalize3(const DN<ND> * x, DN<ND> * o)
{
  DN<ND> n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  DN<ND> n = dsqrt(n2);
  if(n.v < 1e-12f) n = mk<ND>(1e-12f);
  for(int i = 0; i < 3; i++) o[i] = x[i] / n;
}

// convertRotMatToAxisAngle (src/VPoser.cpp:25-120) on one matrix, value + derivative
template<int ND>
__device__ inline void rotmat_to_aa(const DN<ND> R[3][3], DN<ND> aa[3])
{
  const float eps = FLT_EPSILON;
  const float epsSqrt = sqrtf(eps);
  const float epsSqrt2 = sqrtf(epsSqrt);
  const float kPi = 3.14159265358979323846f;
  DN<ND> trace = R[0][0] + R[1][1] + R[2][2];
  DN<ND> theta = dacos((float)((1.0 - (double)eps) * 0.5) * (trace + (-1.0f))); // :41
  DN<ND> w[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};      // :43-49
  if(1.0f + trace.v < epsSqrt2) // near pi (:53-103)
  {
    DN<ND> tn2[3];
    DN<ND> one_m_tr = neg(trace) + 1.0f, three_m_tr = neg(trace) + 3.0f;
    for(int i = 0; i < 3; i++)
    {
      DN<ND> s = (2.0f * R[i][i] + one_m_tr) / three_m_tr; // :54-56
      tn2[i] = dsqrt(s + eps) * theta;                   // :60
    }
    if(theta.v > kPi - 1e-4f) // :62-94
    {
      if(tn2[0].v > 0.0f)
      {
        if(R[0][1].v + R[1][0].v < 0.0f) tn2[1] = neg(tn2[1]);
        if(R[0][2].v + R[2][0].v < 0.0f) tn2[2] = neg(tn2[2]);
      }
      else if(tn2[1].v > 0.0f)
      {
        if(R[1][2].v + R[2][1].v < 0.0f) tn2[2] = neg(tn2[2]);
      }
    }
    else // :96-99
    {
      for(int i = 0; i < 3; i++)
        if(!(w[i].v >= 0.0f)) tn2[i] = neg(tn2[i]);
    }
    for(int i = 0; i < 3; i++) aa[i] = tn2[i];
  }
  else if(fabsf(3.0f - trace.v) < epsSqrt) // near zero: Taylor (:105-111)
  {
    DN<ND> t2 = theta * theta;
    DN<ND> f = (1.0f / 6.0f) * t2 + (7.0f / 360.0f) * (t2 * t2) + 1.0f;
    for(int i = 0; i < 3; i++) aa[i] = 0.5f * (w[i] * f);
  }
  else // :112-116
  {
    DN<ND> f = theta / (2.0f * dsin(theta));
    for(int i = 0; i < 3; i++) aa[i] = w[i] * f;
  }
}

// ContinousRotReprDecoderImpl::forward (:129-141) on one joint's 6 numbers (view [3,2]) then -> axis-angle.  ND = 6: all six
// derivative directions (jac36 [3][6]); ND = 1: direction `dir` only (jac36 [3]: d aa / d o6[dir])
template<int ND>
__device__ inline void sixd_to_aa_dir(const float * o6, int dir, float * aa_out, float * jac)
{
  DN<ND> c1[3], c2[3];
  for(int r = 0; r < 3; r++)
  {
    c1[r] = mk<ND>(o6[2 * r]);
    c2[r] = mk<ND>(o6[2 * r + 1]);
    if(ND == 6)
    {
      c1[r].d[(2 * r) % ND] = 1.0f;
      c2[r].d[(2 * r + 1) % ND] = 1.0f;
    }
    else
    {
      c1[r].d[0] = (2 * r == dir) ? 1.0f : 0.0f;
      c2[r].d[0] = (2 * r + 1 == dir) ? 1.0f : 0.0f;
    }
  }
  DN<ND> a1[3], a2[3], t[3];
  dnormalize3(c1, a1);
  DN<ND> dot = a1[0] * c2[0] + a1[1] * c2[1] + a1[2] * c2[2];
  for(int r = 0; r < 3; r++) t[r] = c2[r] - dot * a1[r];
  dnormalize3(t, a2);
  DN<ND> a3[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
  DN<ND> R[3][3];
  for(int r = 0; r < 3; r++)
  {
    R[r][0] = a1[r];
    R[r][1] = a2[r];
    R[r][2] = a3[r];
  }
  DN<ND> aa[3];
  rotmat_to_aa(R, aa);
  for(int i = 0; i < 3; i++)
  {
    aa_out[i] = aa[i].v;
    if(jac)
      for(int q = 0; q < ND; q++) jac[i * ND + q] = aa[i].d[q];
  }
}
__device__ inline void sixd_to_aa(const float * o6, float * aa_out, float * jac36 /*[3][6]*/)
{
  sixd_to_aa_dir<6>(o6, 0, aa_out, jac36);
}
} // namespace smplpp_hip
