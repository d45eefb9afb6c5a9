// smplpp::imageSample / imageTerm / imageTermBackward over the C ABI — header-only C++ shim of the image term (smplpp_image_sample,
// smplpp_image_term, smplpp_image_term_vjp): a dense channels-last image [B,H,W,C] read at projected points uv [N,K,2] (the uv of
// projectPoints) by bilinear interpolation, a robust squared residual against a target, and the gradient to uv and to the image.
// B is 1 (shared by all frames) or N; with `channel` [K] kInt64, point k reads channel channel[k] alone (Cs = 1), else Cs = C.
// No reference counterpart: the reference has no images.
#ifndef SMPLPP_SHIM_IMAGE_H
#define SMPLPP_SHIM_IMAGE_H

#include "SMPL.h"

namespace smplpp
{
namespace detail
{
// the shapes the three calls share
struct ImageShape
{
  int64_t n, K, B, H, W, C, Cs;
  const int64_t * channel;
};
inline ImageShape imageShape(const Tensor & uv, const Tensor & image, const Tensor & channel, const char * what)
{
  if(uv.dtype != kFloat32 || uv.dim() != 3 || uv.size(2) != 2 || uv.numel() == 0 || image.dtype != kFloat32 || image.dim() != 4)
    throw Exception("Image", what);
  ImageShape s{uv.size(0), uv.size(1), image.size(0), image.size(1), image.size(2), image.size(3), image.size(3), nullptr};
  if(channel.defined())
  {
    if(channel.dtype != kInt64 || channel.numel() != s.K) throw Exception("Image", what);
    s.channel = channel.idata.data(), s.Cs = 1;
  }
  return s;
}
// target [1 or N,K,Cs] / weight [1 or N,K]: the leading count, from the element count
inline int64_t imageRows(const Tensor & t, int64_t n, int64_t per, const char * what)
{
  if(!t.defined()) return 1;
  if(t.dtype != kFloat32 || (t.numel() != per && t.numel() != n * per)) throw Exception("Image", what);
  return t.numel() == per ? 1 : n;
}
} // namespace detail

// The image at uv [N,K,2]: value [N,K,Cs], gradient [N,K,Cs,2] = (d value / du, d value / dv) in pixels, valid [N,K] kInt64 0 / 1
struct ImageSample
{
  Tensor value, gradient, valid;
};
inline ImageSample imageSample(const Tensor & uv, const Tensor & image, const Tensor & channel = Tensor(), int device = 0)
{
  const detail::ImageShape s = detail::imageShape(uv, image, channel, "Cannot sample the image!");
  ImageSample r{Tensor({s.n, s.K, s.Cs}), Tensor({s.n, s.K, s.Cs, 2}), Tensor({s.n, s.K}, kInt64)};
  std::vector<uint8_t> ok((size_t)(s.n * s.K));
  check(smplpp_image_sample(device, s.n, s.K, uv.ptr(), image.ptr(), s.B, s.H, s.W, s.C, s.channel, r.value.ptr(), r.gradient.ptr(), ok.data(),
                            SMPLPP_HOST, nullptr),
        "Image");
  r.valid.idata.assign(ok.begin(), ok.end());
  return r;
}

// The squared residual of the sample against target [1 or N,K,Cs] (undefined: zeros) under weight [1 or N,K] (undefined: ones; rho > 0
// for the Geman-McClure form): energy [N], pointEnergy [N,K], value [N,K,Cs], valid [N,K] kInt64 0 / 1
struct ImageTerm
{
  Tensor energy, pointEnergy, value, valid;
};
inline ImageTerm imageTerm(const Tensor & uv, const Tensor & image, const Tensor & target = Tensor(), const Tensor & weight = Tensor(),
                           float rho = 0.0f, const Tensor & channel = Tensor(), int device = 0)
{
  const char * what = "Cannot evaluate the image term!";
  const detail::ImageShape s = detail::imageShape(uv, image, channel, what);
  const int64_t Tn = detail::imageRows(target, s.n, s.K * s.Cs, what), Wn = detail::imageRows(weight, s.n, s.K, what);
  ImageTerm r{Tensor({s.n}), Tensor({s.n, s.K}), Tensor({s.n, s.K, s.Cs}), Tensor({s.n, s.K}, kInt64)};
  std::vector<uint8_t> ok((size_t)(s.n * s.K));
  check(smplpp_image_term(device, s.n, s.K, uv.ptr(), image.ptr(), s.B, s.H, s.W, s.C, s.channel, target.defined() ? target.ptr() : nullptr, Tn,
                          weight.defined() ? weight.ptr() : nullptr, Wn, rho, r.energy.ptr(), r.pointEnergy.ptr(), r.value.ptr(), ok.data(),
                          SMPLPP_HOST, nullptr),
        "Image");
  r.valid.idata.assign(ok.begin(), ok.end());
  return r;
}

// Its backward: dL/duv [N,K,2] and dL/dimage [B,H,W,C] for dL/denergy [N], dL/dpointEnergy [N,K] and dL/dvalue [N,K,Cs] (an undefined
// one is left out).  `accumulate` non-null: the products are added into its tensors (and it is returned).
struct ImageGradients
{
  Tensor uv, image;
};
inline ImageGradients imageTermBackward(const Tensor & uv, const Tensor & image, const Tensor & gradEnergy, const Tensor & gradPointEnergy,
                                        const Tensor & gradValue, const Tensor & target = Tensor(), const Tensor & weight = Tensor(),
                                        float rho = 0.0f, const Tensor & channel = Tensor(), ImageGradients * accumulate = nullptr, int device = 0)
{
  const char * what = "Cannot back-propagate through the image term!";
  const detail::ImageShape s = detail::imageShape(uv, image, channel, what);
  const int64_t Tn = detail::imageRows(target, s.n, s.K * s.Cs, what), Wn = detail::imageRows(weight, s.n, s.K, what);
  const bool ge = gradEnergy.defined(), gp = gradPointEnergy.defined(), gv = gradValue.defined();
  if((ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != s.n)) ||
     (gp && (gradPointEnergy.dtype != kFloat32 || gradPointEnergy.numel() != s.n * s.K)) ||
     (gv && (gradValue.dtype != kFloat32 || gradValue.numel() != s.n * s.K * s.Cs)))
    throw Exception("Image", what);
  ImageGradients local;
  ImageGradients & out = accumulate ? *accumulate : local;
  if(accumulate)
  {
    if(out.uv.dtype != kFloat32 || out.uv.numel() != s.n * s.K * 2 || out.image.dtype != kFloat32 || out.image.numel() != image.numel())
      throw Exception("Image", what);
  }
  else
    out = ImageGradients{Tensor({s.n, s.K, 2}), Tensor({s.B, s.H, s.W, s.C})};
  check(smplpp_image_term_vjp(device, s.n, s.K, uv.ptr(), image.ptr(), s.B, s.H, s.W, s.C, s.channel, target.defined() ? target.ptr() : nullptr, Tn,
                              weight.defined() ? weight.ptr() : nullptr, Wn, rho, ge ? gradEnergy.ptr() : nullptr,
                              gp ? gradPointEnergy.ptr() : nullptr, gv ? gradValue.ptr() : nullptr, out.uv.ptr(), out.image.ptr(), accumulate ? 1 : 0,
                              SMPLPP_HOST, nullptr),
        "Image");
  return out;
}
} // namespace smplpp
#endif
