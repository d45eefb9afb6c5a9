// smplpp::SelfContact over the C ABI — header-only C++ shim of the self-contact search (smplpp_self_contact_create / smplpp_self_contact
// / smplpp_self_contact_vjp): a vertex's contact partner is the nearest other vertex in space among those that are far along the
// surface.  "Far" is a static bit mask built once from the geodesic distances of a rest mesh (SMPL::meshGeodesic gives the fields
// themselves).  No reference counterpart: the reference has no notion of distance along the surface.
#ifndef SMPLPP_SHIM_CONTACT_H
#define SMPLPP_SHIM_CONTACT_H

#include "SMPL.h"

namespace smplpp
{
class SelfContact
{
public:
  // rest [V,3] (or [N,V,3]: its first frame): the mesh the geodesic distances are taken on, for instance a frame of
  // SMPL::getRestShape() at the subject's beta; far(v, u) iff the distance between v and u along its edges is above geoMin
  SelfContact(const SMPL & smpl, const Tensor & rest, float geoMin = 0.3f) : V_(smpl.vertexNum())
  {
    if(rest.dtype != kFloat32 || rest.numel() < V_ * 3 || rest.numel() % (V_ * 3) != 0) throw Exception("SelfContact", "Cannot build the far mask!");
    check(smplpp_self_contact_create(smpl.handle(), rest.ptr(), geoMin, &h_), "SelfContact");
    check(smplpp_self_contact_info(h_, nullptr, &W_, &geoMin_, &farPairs_), "SelfContact");
  }
  ~SelfContact() { smplpp_self_contact_destroy(h_); }
  SelfContact(const SelfContact &) = delete;
  SelfContact & operator=(const SelfContact &) = delete;

  int64_t vertexNum() const { return V_; }
  int64_t wordsPerRow() const { return W_; }
  float geoMin() const { return geoMin_; }
  int64_t farPairs() const { return farPairs_; } // unordered far pairs
  struct smplpp_self_contact * handle() const { return h_; }

  // the mask [V,W] as kInt64 words (each holds one uint32): bit (u & 31) of word (u >> 5) of row v is far(v, u)
  Tensor mask() const
  {
    std::vector<uint32_t> words((size_t)(V_ * W_));
    check(smplpp_self_contact_mask(h_, words.data(), SMPLPP_HOST, nullptr), "SelfContact");
    Tensor m({V_, W_}, kInt64);
    for(size_t i = 0; i < words.size(); i++) m.idata[i] = (int64_t)words[i];
    return m;
  }

  // index [N,V] kInt64 (-1: no partner), sqdist [N,V] of verts [N,V,3].  vertNormals [N,V,3] (undefined: no normal test) need not be
  // unit: a partner's normal opposes the vertex's by at least cosMin.  maxSqdist is the squared cap (+inf: none).
  struct Partners
  {
    Tensor index, sqdist;
  };
  Partners search(const Tensor & verts, const Tensor & vertNormals = Tensor(), float cosMin = 0.0f,
                  float maxSqdist = std::numeric_limits<float>::infinity()) const
  {
    const char * what = "Cannot search for self-contact!";
    const int64_t n = frames(verts, what);
    if(vertNormals.defined() && (vertNormals.dtype != kFloat32 || vertNormals.numel() != verts.numel())) throw Exception("SelfContact", what);
    Partners r{Tensor({n, V_}, kInt64), Tensor({n, V_})};
    check(smplpp_self_contact(h_, n, verts.ptr(), vertNormals.defined() ? vertNormals.ptr() : nullptr, cosMin, maxSqdist, r.index.idata.data(),
                              r.sqdist.ptr(), SMPLPP_HOST, nullptr),
          "SelfContact");
    return r;
  }
  // Its backward pass: dL/dverts [N,V,3] for dL/dsqdist = gradSqdist [N,V] at the partners `index` [N,V] search chose, to a vertex
  // both as a query and as a partner.  `accumulate` non-null: the product is added into it (and it is returned).
  Tensor searchBackward(const Tensor & verts, const Tensor & index, const Tensor & gradSqdist, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the self-contact search!";
    const int64_t n = frames(verts, what);
    if(index.dtype != kInt64 || index.numel() != n * V_ || gradSqdist.dtype != kFloat32 || gradSqdist.numel() != n * V_ ||
       (accumulate && (accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3)))
      throw Exception("SelfContact", what);
    Tensor local;
    if(!accumulate) local = Tensor({n, V_, 3});
    Tensor & out = accumulate ? *accumulate : local;
    check(smplpp_self_contact_vjp(h_, n, verts.ptr(), index.idata.data(), gradSqdist.ptr(), out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SelfContact");
    return out;
  }

private:
  int64_t frames(const Tensor & verts, const char * what) const
  {
    if(verts.dtype != kFloat32 || verts.numel() == 0 || verts.numel() % (V_ * 3) != 0) throw Exception("SelfContact", what);
    return verts.numel() / (V_ * 3);
  }
  int64_t V_, W_ = 0, farPairs_ = 0;
  float geoMin_ = 0.0f;
  struct smplpp_self_contact * h_ = nullptr;
};
} // namespace smplpp
#endif
