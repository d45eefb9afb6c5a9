// smplpp::Landmarks and smplpp::projectPoints over the C ABI — header-only C++ shim of the keypoint term (smplpp_landmarks_create /
// smplpp_landmarks / smplpp_landmarks_vjp, smplpp_project_points / smplpp_project_points_vjp).  No reference counterpart: the
// reference reads its correspondences from motion-capture markers (node/node.cpp:681-700), not from image keypoints.  A regressor is
// a CSR matrix of L rows over V + 24 sources: column c < V is vertex c, column V + j joint j of SMPL::getRestJoint.
#ifndef SMPLPP_SHIM_LANDMARKS_H
#define SMPLPP_SHIM_LANDMARKS_H

#include "SMPL.h"

namespace smplpp
{
class Landmarks
{
public:
  // rowPtr [L+1], col [nnz], val [nnz]; a column may repeat within a row, a row may be empty
  Landmarks(const SMPL & smpl, const std::vector<int64_t> & rowPtr, const std::vector<int64_t> & col, const std::vector<float> & val)
      : V_(smpl.vertexNum()), L_((int64_t)rowPtr.size() - 1)
  {
    if(rowPtr.size() < 2 || col.size() != val.size() || rowPtr.back() != (int64_t)col.size())
      throw Exception("Landmarks", "rowPtr [L+1] must end at the length of col and val");
    check(smplpp_landmarks_create(smpl.handle(), L_, rowPtr.data(), col.data(), val.data(), &h_), "Landmarks");
  }
  ~Landmarks() { smplpp_landmarks_destroy(h_); }
  Landmarks(const Landmarks &) = delete;
  Landmarks & operator=(const Landmarks &) = delete;

  int64_t landmarkNum() const { return L_; }
  struct smplpp_landmarks * handle() const { return h_; }

  // points [N,L,3] from verts [N,V,3] and joints [N,24,3] (SMPL::getVertex, SMPL::getRestJoint)
  Tensor regress(const Tensor & verts, const Tensor & joints) const
  {
    const int64_t n = frames(verts, V_ * 3, "Cannot regress the landmarks!");
    if(joints.dtype != kFloat32 || joints.numel() != n * JOINT_NUM * 3) throw Exception("Landmarks", "Cannot regress the landmarks!");
    Tensor points({n, L_, 3});
    check(smplpp_landmarks(h_, n, verts.ptr(), joints.ptr(), points.ptr(), SMPLPP_HOST, nullptr), "Landmarks");
    return points;
  }
  // Its backward pass: dL/dverts [N,V,3] and dL/djoints [N,24,3] for dL/dpoints = gradPoints [N,L,3], what SMPL::launchBackward takes.
  // `accumulate` non-null: the products are added into its tensors (and it is returned).
  struct Gradients
  {
    Tensor verts, joints;
  };
  Gradients regressBackward(const Tensor & gradPoints, Gradients * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the landmarks!";
    const int64_t n = frames(gradPoints, L_ * 3, what);
    Gradients local;
    Gradients & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(out.verts.dtype != kFloat32 || out.verts.numel() != n * V_ * 3 || out.joints.dtype != kFloat32 || out.joints.numel() != n * JOINT_NUM * 3)
        throw Exception("Landmarks", what);
    }
    else
      out = Gradients{Tensor({n, V_, 3}), Tensor({n, JOINT_NUM, 3})};
    check(smplpp_landmarks_vjp(h_, n, gradPoints.ptr(), out.verts.ptr(), out.joints.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr), "Landmarks");
    return out;
  }

private:
  static int64_t frames(const Tensor & t, int64_t row, const char * what)
  {
    if(t.dtype != kFloat32 || t.numel() == 0 || t.numel() % row != 0) throw Exception("Landmarks", what);
    return t.numel() / row;
  }
  int64_t V_, L_;
  struct smplpp_landmarks * h_ = nullptr;
};

namespace detail
{
// points [N,K,3] -> (N, K); camera [16] or [N,16] as N rows
inline std::vector<float> projectionRows(const Tensor & points, const Tensor & camera, int64_t & n, int64_t & K, const char * what)
{
  if(points.dtype != kFloat32 || points.dim() != 3 || points.size(2) != 3 || points.numel() == 0 || camera.dtype != kFloat32 ||
     (camera.numel() != 16 && camera.numel() != points.size(0) * 16))
    throw Exception("Landmarks", what);
  n = points.size(0), K = points.size(1);
  std::vector<float> cam((size_t)n * 16);
  for(size_t i = 0; i < cam.size(); i++) cam[i] = camera.data[camera.numel() == 16 ? i % 16 : i];
  return cam;
}
} // namespace detail

// Points [N,K,3] through the cameras ([16] or [N,16]: R row-major world -> camera, t, fx, fy, cx, cy) by the depth rasteriser's vertex
// rule, and their keypoint energy against target [N,K,3] = (u, v, confidence); an undefined (default-constructed) target: no energy.
// uv [N,K,2], energy [N,K], valid [N,K] kInt64 (1 = projected, 0 = refused: uv and energy 0).  smplpp_project_points.
struct Projection
{
  Tensor uv, energy, valid;
};
inline Projection projectPoints(const Tensor & points, const Tensor & camera, const Tensor & target = Tensor(), float rho = 0.0f,
                                float near = 0.05f, int device = 0)
{
  const char * what = "Cannot project the points!";
  int64_t n, K;
  const std::vector<float> cam = detail::projectionRows(points, camera, n, K, what);
  const bool tg = target.defined();
  if(tg && (target.dtype != kFloat32 || target.numel() != n * K * 3)) throw Exception("Landmarks", what);
  Projection r{Tensor({n, K, 2}), tg ? Tensor({n, K}) : Tensor(), Tensor({n, K}, kInt64)};
  std::vector<uint8_t> valid((size_t)(n * K));
  check(smplpp_project_points(device, n, K, points.ptr(), cam.data(), near, tg ? target.ptr() : nullptr, rho, r.uv.ptr(),
                              tg ? r.energy.ptr() : nullptr, valid.data(), SMPLPP_HOST, nullptr),
        "Landmarks");
  for(size_t i = 0; i < valid.size(); i++) r.valid.idata[i] = valid[i];
  return r;
}
// Its backward pass (smplpp_project_points_vjp): dL/dpoints [N,K,3] and dL/dcamera [N,16] (the layout of the camera rows, R as nine
// independent entries) for dL/duv = gradUv [N,K,2] and dL/denergy = gradEnergy [N,K]; an undefined cotangent is left out.
// `accumulate` non-null: the products are added into its tensors (and it is returned).
struct ProjectionGradients
{
  Tensor points, camera;
};
inline ProjectionGradients projectPointsBackward(const Tensor & points, const Tensor & camera, const Tensor & target, float rho,
                                                 const Tensor & gradUv, const Tensor & gradEnergy, float near = 0.05f,
                                                 ProjectionGradients * accumulate = nullptr, int device = 0)
{
  const char * what = "Cannot back-propagate through the projection!";
  int64_t n, K;
  const std::vector<float> cam = detail::projectionRows(points, camera, n, K, what);
  const bool tg = target.defined(), gu = gradUv.defined(), ge = gradEnergy.defined();
  if((tg && (target.dtype != kFloat32 || target.numel() != n * K * 3)) || (gu && (gradUv.dtype != kFloat32 || gradUv.numel() != n * K * 2)) ||
     (ge && (gradEnergy.dtype != kFloat32 || gradEnergy.numel() != n * K)))
    throw Exception("Landmarks", what);
  ProjectionGradients local;
  ProjectionGradients & out = accumulate ? *accumulate : local;
  if(accumulate)
  {
    if(out.points.dtype != kFloat32 || out.points.numel() != n * K * 3 || out.camera.dtype != kFloat32 || out.camera.numel() != n * 16)
      throw Exception("Landmarks", what);
  }
  else
    out = ProjectionGradients{Tensor({n, K, 3}), Tensor({n, 16})};
  check(smplpp_project_points_vjp(device, n, K, points.ptr(), cam.data(), near, tg ? target.ptr() : nullptr, rho, gu ? gradUv.ptr() : nullptr,
                                  ge ? gradEnergy.ptr() : nullptr, out.points.ptr(), out.camera.ptr(), accumulate ? 1 : 0, SMPLPP_HOST,
                                  nullptr),
        "Landmarks");
  return out;
}
} // namespace smplpp
#endif
