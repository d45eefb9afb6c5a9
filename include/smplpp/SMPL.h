// smplpp::SMPL / smplpp::IkTask over the C ABI of libsmplpp_hip.so — header-only C++ shim.
//
// Keeps the reference's class names, method names and argument meaning
// (/root/reference/include/smplpp/SMPL.h:241-269, include/smplpp/IkTask.h:20-84) so that node/node.cpp-style callers
// re-link against the MI355X engine.  `torch::Tensor` is replaced by the minimal owning host container `smplpp::Tensor`
// (Tensor.h: the methods node.cpp applies to these results, under torch's names); errors become `smplpp::Exception` like
// smpl_error (include/smplpp/toolbox/Exception.h:48-49).  Signatures follow the reference header line by line: the
// three-argument constructor, copy construction / assignment, setVertPath + out(index), getFaceIndex / getFaceIndexRaw as tensors
// of kInt32 (1-based), getVertexRaw(index tensor), getAdjacentFaces as a reference to an unordered_map.
// The one semantic change is the autograd seam: there is no backward(); use IkSolver::eval()/iterate().
#ifndef SMPLPP_SHIM_SMPL_H
#define SMPLPP_SHIM_SMPL_H

#include <array>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <unordered_map>
#include <vector>

#include "../smplpp_hip.h"
#include "Tensor.h"

namespace smplpp
{
constexpr int64_t JOINT_NUM = SMPLPP_JOINT_NUM;
constexpr int64_t SHAPE_BASIS_DIM = SMPLPP_SHAPE_BASIS_DIM;
constexpr int64_t POSE_BASIS_DIM = SMPLPP_POSE_BASIS_DIM;
constexpr int64_t LATENT_DIM = SMPLPP_LATENT_DIM;

inline void check(int rc, const char * module)
{
  if(rc != SMPLPP_OK) throw Exception(module, smplpp_last_error());
}
// the reference's name for its exception (include/smplpp/toolbox/Exception.h:48-49: smpl_error(module, message))
using smpl_error = Exception;

// An index list as a tensor of kInt64 (`getVertexRaw(faceVertexIdxs.to(torch::kInt64))`, node/node.cpp:186)
struct IndexTensor : Tensor
{
  IndexTensor() : Tensor({0}, kInt64) {}
  IndexTensor(std::initializer_list<int64_t> v) : Tensor({(int64_t)v.size()}, kInt64) { idata.assign(v.begin(), v.end()); }
  explicit IndexTensor(const std::vector<int64_t> & v) : Tensor({(int64_t)v.size()}, kInt64) { idata = v; }
};

namespace detail
{
// Just enough JSON for the model files scripts/preprocess.py writes: an object of (nested) numeric arrays.
struct JsonArrays
{
  std::map<std::string, std::vector<double>> values;
  std::map<std::string, std::vector<int64_t>> shapes;
  explicit JsonArrays(const std::string & path)
  {
    std::ifstream f(path, std::ios::binary);
    if(!f) throw Exception("SMPL", "Cannot initialize a SMPL model!"); // src/SMPL.cpp:616
    std::stringstream ss;
    ss << f.rdbuf();
    s_ = ss.str();
    skip();
    expect('{');
    for(;;)
    {
      skip();
      if(peek() == '}') break;
      std::string key = str();
      skip();
      expect(':');
      std::vector<int64_t> shape;
      std::vector<double> vals;
      array(vals, shape, 0);
      values[key] = std::move(vals);
      shapes[key] = std::move(shape);
      skip();
      if(peek() == ',') p_++;
    }
  }

private:
  std::string s_;
  size_t p_ = 0;
  char peek() const { return p_ < s_.size() ? s_[p_] : '\0'; }
  void skip()
  {
    while(p_ < s_.size() && std::isspace((unsigned char)s_[p_])) p_++;
  }
  void expect(char c)
  {
    if(peek() != c) throw Exception("SMPL", std::string("model json: expected '") + c + "'");
    p_++;
  }
  std::string str()
  {
    expect('"');
    size_t b = p_;
    while(p_ < s_.size() && s_[p_] != '"') p_++;
    std::string r = s_.substr(b, p_ - b);
    p_++;
    return r;
  }
  void array(std::vector<double> & vals, std::vector<int64_t> & shape, size_t depth)
  {
    skip();
    if(peek() != '[')
    {
      char * end = nullptr;
      vals.push_back(std::strtod(s_.c_str() + p_, &end));
      p_ = (size_t)(end - s_.c_str());
      return;
    }
    p_++;
    int64_t n = 0;
    for(;;)
    {
      skip();
      if(peek() == ']')
      {
        p_++;
        break;
      }
      array(vals, shape, depth + 1);
      n++;
      skip();
      if(peek() == ',') p_++;
    }
    if(shape.size() <= depth) shape.resize(depth + 1, 0);
    shape[depth] = n;
  }
};
} // namespace detail

class SMPL
{
public:
  // %% Constructor and Destructor %% (reference include/smplpp/SMPL.h:241-247, src/SMPL.cpp:100-262)
  SMPL() = default;
  SMPL(const std::string & modelPath, const std::string & vertPath, const Device & device) : vertPath_(vertPath)
  {
    setDevice(device);
    setModelPath(modelPath);
  }
  // A copy shares the engine's model (immutable once created) and takes a copy of the outputs of the last launch — the
  // reference deep-copies its tensors (src/SMPL.cpp:160-262); std::map<std::string, IkTask> and the node's globals need no more.
  SMPL(const SMPL &) = default;
  SMPL & operator=(const SMPL &) = default;
  ~SMPL() = default;

  // %% Setter and Getter %%
  void setDevice(const Device & device)
  {
    if(!device.has_index()) throw Exception("SMPL", "Failed to fetch device index!"); // src/SMPL.cpp:289-297
    if(device.type == "CPU" || device.type == "cpu") throw Exception("SMPL", "libsmplpp_hip has no CPU engine");
    device_ = device;
  }
  Device getDevice() const { return device_; }
  void setModelPath(const std::string & modelPath) { path_ = modelPath; }
  void setVertPath(const std::string & vertexPath) { vertPath_ = vertexPath; } // src/SMPL.cpp:361

  // SMPL::init (src/SMPL.cpp:560-643): parse the .json written by scripts/preprocess.py and create the engine model.
  void init()
  {
    detail::JsonArrays j(path_);
    auto f32 = [&](const char * k) {
      auto it = j.values.find(k);
      if(it == j.values.end()) throw Exception("SMPL", std::string("model json lacks ") + k);
      return std::vector<float>(it->second.begin(), it->second.end());
    };
    std::vector<float> vt = f32("vertices_template"), S = f32("shape_blend_shapes"), P = f32("pose_blend_shapes"),
                       Jr = f32("joint_regressor"), W = f32("weights");
    const auto & kv = j.values.at("kinematic_tree");
    const auto & fv = j.values.at("face_indices");
    std::vector<int64_t> kin(kv.begin(), kv.end());
    std::vector<int32_t> faces(fv.begin(), fv.end());
    initFromArrays((int64_t)vt.size() / 3, (int64_t)faces.size() / 3, vt.data(), S.data(), P.data(), Jr.data(), W.data(),
                   kin.data(), faces.data());
  }
  void initFromArrays(int64_t V, int64_t F, const float * vt, const float * S, const float * P, const float * Jreg,
                      const float * W, const int64_t * kintree, const int32_t * faces1)
  {
    smplpp_model * m = nullptr;
    check(smplpp_model_create(V, F, vt, S, P, Jreg, W, kintree, faces1, device_.index, &m), "SMPL");
    m_ = std::shared_ptr<smplpp_model>(m, [](smplpp_model * p) { smplpp_model_destroy(p); });
    V_ = V;
    F_ = F;
    faces1_ = Tensor({F, 3}, kInt32); // 1-based like the model file (scripts/preprocess.py:91)
    faces1_.idata.assign(faces1, faces1 + F * 3);
    // adjacent faces per vertex with uniform weights 1 / degree (src/SMPL.cpp:620-640), kept for getAdjacentFaces
    auto adj = std::make_shared<std::vector<std::unordered_map<int64_t, float>>>((size_t)V);
    std::vector<int64_t> fbuf(256);
    std::vector<float> wbuf(256);
    for(int64_t v = 0; v < V; v++)
    {
      int64_t cnt = 0;
      check(smplpp_adjacent_faces(m, v, (int64_t)fbuf.size(), fbuf.data(), wbuf.data(), &cnt), "SMPL");
      if(cnt > (int64_t)fbuf.size())
      {
        fbuf.resize((size_t)cnt);
        wbuf.resize((size_t)cnt);
        check(smplpp_adjacent_faces(m, v, cnt, fbuf.data(), wbuf.data(), &cnt), "SMPL");
      }
      for(int64_t i = 0; i < cnt; i++) (*adj)[(size_t)v][fbuf[(size_t)i]] = wbuf[(size_t)i];
    }
    adjacent_ = adj;
  }

  // SMPL::launch (src/SMPL.cpp:671-737): beta [N,10], theta [N,25,3] (row 0 = root translation)
  void launch(const Tensor & beta, const Tensor & theta)
  {
    if(!m_ || beta.shape.size() != 2 || beta.size(1) != SHAPE_BASIS_DIM || theta.shape.size() != 3
       || theta.size(0) != beta.size(0) || theta.size(1) != JOINT_NUM + 1 || theta.size(2) != 3 || beta.dtype != kFloat32 || theta.dtype != kFloat32)
      throw Exception("SMPL", "Cannot launch a SMPL model!");
    const int64_t n = beta.size(0);
    verts_ = Tensor({n, V_, 3});
    rest_ = Tensor({n, V_, 3});
    joints_ = Tensor({n, JOINT_NUM, 3});
    xforms_ = Tensor({n, JOINT_NUM, 4, 4});
    check(smplpp_fk(m_.get(), n, beta.ptr(), theta.ptr(), verts_.ptr(), joints_.ptr(), xforms_.ptr(), rest_.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    beta_ = beta;
    theta_ = theta;
    rot_ = Tensor(); // (the outputs are no longer launchRotmat's)
  }

  // What backward() through the last launch's graph gave the reference (e.g. node/node.cpp:823-869): for the beta / theta of the
  // last launch, dL/dbeta [N,10] and dL/dtheta [N,25,3] of a loss with dL/dverts = gradVert [N,V,3] and dL/djoints = gradJoint
  // [N,24,3] (an empty Tensor = zero).  smplpp_fk_vjp, reusing the launch's rest shape.
  std::pair<Tensor, Tensor> launchBackward(const Tensor & gradVert, const Tensor & gradJoint) const
  {
    const Tensor & rest = need(rest_);
    const int64_t n = beta_.size(0);
    const bool hv = !gradVert.data.empty(), hj = !gradJoint.data.empty();
    if((hv && (gradVert.numel() != n * V_ * 3 || gradVert.dtype != kFloat32)) ||
       (hj && (gradJoint.numel() != n * JOINT_NUM * 3 || gradJoint.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot back-propagate through a SMPL model!");
    Tensor gb({n, SHAPE_BASIS_DIM}), gt({n, JOINT_NUM + 1, 3});
    check(smplpp_fk_vjp(m_.get(), n, beta_.ptr(), theta_.ptr(), rest.ptr(), hv ? gradVert.ptr() : nullptr, hj ? gradJoint.ptr() : nullptr,
                        gb.ptr(), gt.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return {gb, gt};
  }

  // Axis-angles [..., 3] as rotation matrices [..., 3, 3], row-major, with the bits launch computes internally
  // (smplpp_axis_angle_to_rotmat): launchRotmat(beta, theta[:, 0], axisAngleToRotmat(theta[:, 1:])) gives the bits of launch.
  Tensor axisAngleToRotmat(const Tensor & aa) const
  {
    if(aa.shape.empty() || aa.shape.back() != 3 || aa.numel() == 0 || aa.dtype != kFloat32)
      throw Exception("SMPL", "axisAngleToRotmat: expected float32 axis-angles of shape [..., 3]");
    std::vector<int64_t> shape(aa.shape.begin(), aa.shape.end() - 1);
    shape.push_back(3);
    shape.push_back(3);
    Tensor rot(shape);
    check(smplpp_axis_angle_to_rotmat(device_.index, aa.numel() / 3, aa.ptr(), rot.ptr(), SMPLPP_HOST, nullptr), "SMPL");
    return rot;
  }

  // Its vector-Jacobian product (smplpp_axis_angle_to_rotmat_vjp): dL/daa [..., 3] for dL/drot = gradRot [..., 3, 3], nine independent
  // entries per matrix, by the derivative launchBackward and skeletonBackward contract with (finite at aa = 0 and at |aa| = pi).
  // `accumulate` non-null: the gradient is added into it (and it is returned).
  Tensor axisAngleToRotmatBackward(const Tensor & aa, const Tensor & gradRot, Tensor * accumulate = nullptr) const
  {
    if(aa.shape.empty() || aa.shape.back() != 3 || aa.numel() == 0 || aa.dtype != kFloat32 || gradRot.dtype != kFloat32 ||
       gradRot.numel() != aa.numel() * 3 || (accumulate && (accumulate->dtype != kFloat32 || accumulate->numel() != aa.numel())))
      throw Exception("SMPL", "axisAngleToRotmatBackward: expected float32 aa [..., 3] and gradRot [..., 3, 3]");
    Tensor local;
    if(!accumulate) local = Tensor(std::vector<int64_t>(aa.shape.begin(), aa.shape.end()));
    Tensor & out = accumulate ? *accumulate : local;
    check(smplpp_axis_angle_to_rotmat_vjp(device_.index, aa.numel() / 3, aa.ptr(), gradRot.ptr(), out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST,
                                          nullptr),
          "SMPL");
    return out;
  }

  // launch from rotation matrices (smplpp_fk_rotmat): beta [N,10], trans [N,3] (root translation), rot [N,24,3,3] row-major, joint 0
  // the root orientation, used as given.  An empty beta or trans = zero.  The getters return its outputs as they do launch's.
  void launchRotmat(const Tensor & beta, const Tensor & trans, const Tensor & rot)
  {
    const bool hb = !beta.data.empty(), ht = !trans.data.empty();
    if(!m_ || rot.shape.size() != 4 || rot.size(1) != JOINT_NUM || rot.size(2) != 3 || rot.size(3) != 3 || rot.dtype != kFloat32
       || (hb && (beta.numel() != rot.size(0) * SHAPE_BASIS_DIM || beta.dtype != kFloat32))
       || (ht && (trans.numel() != rot.size(0) * 3 || trans.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot launch a SMPL model!");
    const int64_t n = rot.size(0);
    verts_ = Tensor({n, V_, 3});
    rest_ = Tensor({n, V_, 3});
    joints_ = Tensor({n, JOINT_NUM, 3});
    xforms_ = Tensor({n, JOINT_NUM, 4, 4});
    check(smplpp_fk_rotmat(m_.get(), n, hb ? beta.ptr() : nullptr, ht ? trans.ptr() : nullptr, rot.ptr(), verts_.ptr(), joints_.ptr(),
                           xforms_.ptr(), rest_.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    betaR_ = beta;
    transR_ = trans;
    rot_ = rot;
    beta_ = theta_ = Tensor(); // (the outputs are no longer launch's: launchBackward refuses)
  }

  // The backward of the last launchRotmat (smplpp_fk_rotmat_vjp, reusing its rest shape): {dL/dbeta [N,10], dL/dtrans [N,3],
  // dL/drot [N,24,3,3]} for dL/dverts = gradVert and dL/djoints = gradJoint (an empty Tensor = zero).  dL/drot is the gradient to nine
  // independent entries per joint.
  std::tuple<Tensor, Tensor, Tensor> launchRotmatBackward(const Tensor & gradVert, const Tensor & gradJoint) const
  {
    const Tensor & rest = need(rest_);
    if(rot_.data.empty()) throw Exception("SMPL", "Cannot back-propagate through a SMPL model!");
    const int64_t n = rot_.size(0);
    const bool hv = !gradVert.data.empty(), hj = !gradJoint.data.empty();
    if((hv && (gradVert.numel() != n * V_ * 3 || gradVert.dtype != kFloat32)) ||
       (hj && (gradJoint.numel() != n * JOINT_NUM * 3 || gradJoint.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot back-propagate through a SMPL model!");
    Tensor gb({n, SHAPE_BASIS_DIM}), gt({n, 3}), gr({n, JOINT_NUM, 3, 3});
    check(smplpp_fk_rotmat_vjp(m_.get(), n, betaR_.data.empty() ? nullptr : betaR_.ptr(), transR_.data.empty() ? nullptr : transR_.ptr(),
                               rot_.ptr(), rest.ptr(), hv ? gradVert.ptr() : nullptr, hj ? gradJoint.ptr() : nullptr, gb.ptr(), gt.ptr(),
                               gr.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return {gb, gt, gr};
  }

  // Forward mode of the last launch (smplpp_fk_jvp, reusing its rest shape; no reference counterpart): for T tangents dBeta [N,T,10]
  // and dTheta [N,T,25,3] (an empty Tensor = zero, not both; row 0 of dTheta is the tangent of the root translation) the tangents
  // verts [N,T,V,3] of getVertex, joints [N,T,24,3] of getRestJoint and world [N,T,24,3,4] of skeleton().world.  shared: the tangents
  // are [T,10] / [T,25,3], one set applied to every frame (the one-hot basis of a Jacobian).  With dTheta = the pose rate these are
  // velocities.
  struct Tangent
  {
    Tensor verts, joints, world;
  };
  Tangent launchTangent(const Tensor & dBeta, const Tensor & dTheta, bool shared = false) const
  {
    const Tensor & rest = need(rest_);
    if(beta_.data.empty()) throw Exception("SMPL", "Cannot push a tangent through a SMPL model!");
    const int64_t n = beta_.size(0), tf = shared ? 1 : n;
    const int64_t T = tangentCount(tf, {&dBeta, &dTheta}, {SHAPE_BASIS_DIM, (JOINT_NUM + 1) * 3});
    Tangent t{Tensor({n, T, V_, 3}), Tensor({n, T, JOINT_NUM, 3}), Tensor({n, T, JOINT_NUM, 3, 4})};
    check(smplpp_fk_jvp(m_.get(), n, T, beta_.ptr(), theta_.ptr(), rest.ptr(), dBeta.data.empty() ? nullptr : dBeta.ptr(),
                        dTheta.data.empty() ? nullptr : dTheta.ptr(), shared ? 1 : 0, t.verts.ptr(), t.joints.ptr(), t.world.ptr(),
                        SMPLPP_HOST, nullptr),
          "SMPL");
    return t;
  }

  // The same for the last launchRotmat (smplpp_fk_rotmat_jvp): tangents dBeta [N,T,10], dTrans [N,T,3] and dRot [N,T,24,3,3] (nine
  // independent entries per joint, used as given; an empty Tensor = zero, not all three); shared drops their leading N.
  Tangent launchRotmatTangent(const Tensor & dBeta, const Tensor & dTrans, const Tensor & dRot, bool shared = false) const
  {
    const Tensor & rest = need(rest_);
    if(rot_.data.empty()) throw Exception("SMPL", "Cannot push a tangent through a SMPL model!");
    const int64_t n = rot_.size(0), tf = shared ? 1 : n;
    const int64_t T = tangentCount(tf, {&dBeta, &dTrans, &dRot}, {SHAPE_BASIS_DIM, 3, JOINT_NUM * 9});
    Tangent t{Tensor({n, T, V_, 3}), Tensor({n, T, JOINT_NUM, 3}), Tensor({n, T, JOINT_NUM, 3, 4})};
    check(smplpp_fk_rotmat_jvp(m_.get(), n, T, betaR_.data.empty() ? nullptr : betaR_.ptr(), transR_.data.empty() ? nullptr : transR_.ptr(),
                               rot_.ptr(), rest.ptr(), dBeta.data.empty() ? nullptr : dBeta.ptr(), dTrans.data.empty() ? nullptr : dTrans.ptr(),
                               dRot.data.empty() ? nullptr : dRot.ptr(), shared ? 1 : 0, t.verts.ptr(), t.joints.ptr(), t.world.ptr(),
                               SMPLPP_HOST, nullptr),
          "SMPL");
    return t;
  }

  // The skeleton alone (smplpp_skeleton; no reference counterpart): world [N,24,3,4] = [A_j | posed_j] row-major, the world orientation
  // and position of every joint; posed [N,24,3] the posed joints; joints [N,24,3] the rest joints of getRestJoint.  One kernel, no
  // vertex; nothing is kept for the getters or for a later backward: the backward calls below take beta and theta again.
  struct Skeleton
  {
    Tensor world, posed, joints;
  };
  Skeleton skeleton(const Tensor & beta, const Tensor & theta) const
  {
    const bool hb = !beta.data.empty();
    if(!m_ || theta.shape.size() != 3 || theta.size(1) != JOINT_NUM + 1 || theta.size(2) != 3 || theta.dtype != kFloat32
       || (hb && (beta.numel() != theta.size(0) * SHAPE_BASIS_DIM || beta.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot pose the skeleton of a SMPL model!");
    const int64_t n = theta.size(0);
    Skeleton s{Tensor({n, JOINT_NUM, 3, 4}), Tensor({n, JOINT_NUM, 3}), Tensor({n, JOINT_NUM, 3})};
    check(smplpp_skeleton(m_.get(), n, hb ? beta.ptr() : nullptr, theta.ptr(), s.world.ptr(), s.posed.ptr(), s.joints.ptr(), SMPLPP_HOST,
                          nullptr),
          "SMPL");
    return s;
  }

  // skeleton from rotation matrices (smplpp_skeleton_rotmat): rot [N,24,3,3] used as given; an empty beta or trans = zero.
  Skeleton skeletonRotmat(const Tensor & beta, const Tensor & trans, const Tensor & rot) const
  {
    checkSkeletonRotmat(beta, trans, rot);
    const int64_t n = rot.size(0);
    Skeleton s{Tensor({n, JOINT_NUM, 3, 4}), Tensor({n, JOINT_NUM, 3}), Tensor({n, JOINT_NUM, 3})};
    check(smplpp_skeleton_rotmat(m_.get(), n, beta.data.empty() ? nullptr : beta.ptr(), trans.data.empty() ? nullptr : trans.ptr(), rot.ptr(),
                                 s.world.ptr(), s.posed.ptr(), s.joints.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return s;
  }

  // {dL/dbeta [N,10], dL/dtheta [N,25,3]} of a loss on skeleton(beta, theta) with dL/dworld = gradWorld [N,24,3,4], dL/dposed =
  // gradPosed [N,24,3] and dL/djoints = gradJoints [N,24,3] (an empty Tensor = zero; at least one).  smplpp_skeleton_vjp.
  std::pair<Tensor, Tensor> skeletonBackward(const Tensor & beta, const Tensor & theta, const Tensor & gradWorld, const Tensor & gradPosed,
                                             const Tensor & gradJoints) const
  {
    const bool hb = !beta.data.empty();
    if(!m_ || theta.shape.size() != 3 || theta.size(1) != JOINT_NUM + 1 || theta.size(2) != 3 || theta.dtype != kFloat32
       || (hb && (beta.numel() != theta.size(0) * SHAPE_BASIS_DIM || beta.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot back-propagate through the skeleton of a SMPL model!");
    const int64_t n = theta.size(0);
    checkSkeletonGrads(n, gradWorld, gradPosed, gradJoints);
    Tensor gb({n, SHAPE_BASIS_DIM}), gt({n, JOINT_NUM + 1, 3});
    check(smplpp_skeleton_vjp(m_.get(), n, hb ? beta.ptr() : nullptr, theta.ptr(), optional(gradWorld), optional(gradPosed),
                              optional(gradJoints), gb.ptr(), gt.ptr(), 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return {gb, gt};
  }

  // {dL/dbeta [N,10], dL/dtrans [N,3], dL/drot [N,24,3,3]} of a loss on skeletonRotmat(beta, trans, rot); dL/drot is the gradient to
  // nine independent entries per joint, as launchRotmatBackward's.  smplpp_skeleton_rotmat_vjp.
  std::tuple<Tensor, Tensor, Tensor> skeletonRotmatBackward(const Tensor & beta, const Tensor & trans, const Tensor & rot,
                                                            const Tensor & gradWorld, const Tensor & gradPosed, const Tensor & gradJoints) const
  {
    checkSkeletonRotmat(beta, trans, rot);
    const int64_t n = rot.size(0);
    checkSkeletonGrads(n, gradWorld, gradPosed, gradJoints);
    Tensor gb({n, SHAPE_BASIS_DIM}), gt({n, 3}), gr({n, JOINT_NUM, 3, 3});
    check(smplpp_skeleton_rotmat_vjp(m_.get(), n, beta.data.empty() ? nullptr : beta.ptr(), trans.data.empty() ? nullptr : trans.ptr(),
                                     rot.ptr(), optional(gradWorld), optional(gradPosed), optional(gradJoints), gb.ptr(), gt.ptr(), gr.ptr(), 0,
                                     SMPLPP_HOST, nullptr),
          "SMPL");
    return {gb, gt, gr};
  }

  Tensor getVertex() const { return need(verts_); }       // [N,6890,3] copy (src/SMPL.cpp:492-506)
  Tensor getRestShape() const { return need(rest_); }
  Tensor getRestJoint() const { return need(joints_); }   // [N,24,3]
  Tensor getTransformation() const { return need(xforms_); }
  // batch 0 only, like src/LinearBlendSkinning.cpp:419-427
  Tensor getVertexRaw(int64_t idx) const
  {
    need(verts_);
    if(idx < 0 || idx >= V_) throw Exception("LinearBlendSknning", "vertex index out of range");
    Tensor t({3});
    for(int x = 0; x < 3; x++) t.data[x] = verts_.data[(size_t)idx * 3 + x];
    return t;
  }
  // index-tensor overload (include/smplpp/SMPL.h:257 of the reference; src/LinearBlendSkinning.cpp:424-427): rows of
  // batch 0 for a list of vertex ids -> [len, 3]
  Tensor getVertexRaw(const Tensor & idx) const
  {
    need(verts_);
    if(idx.dtype != kInt64 && idx.dtype != kInt32) throw Exception("LinearBlendSknning", "vertex indices must be an integer tensor");
    Tensor t({idx.numel(), 3});
    for(int64_t i = 0; i < idx.numel(); i++)
    {
      const int64_t v = idx.idata[(size_t)i];
      if(v < 0 || v >= V_) throw Exception("LinearBlendSknning", "vertex index out of range");
      for(int x = 0; x < 3; x++) t.data[(size_t)i * 3 + x] = verts_.data[(size_t)v * 3 + x];
    }
    return t;
  }
  Tensor getFaceIndex() const { return faces1_; } // [F,3] kInt32, 1-based (src/SMPL.cpp:418-433)
  Tensor getFaceIndexRaw(int64_t idx) const        // [3] kInt32, 1-based (:435-438)
  {
    if(idx < 0 || idx >= F_) throw Exception("SMPL", "face index out of range");
    return faces1_.index({idx});
  }
  Tensor calcNormal(int64_t faceIdx) const // src/SMPL.cpp:518-525 (batch 0)
  {
    need(verts_);
    Tensor t({3});
    check(smplpp_face_normals(m_.get(), 1, verts_.ptr(), 1, &faceIdx, t.ptr(), SMPLPP_HOST, nullptr), "SMPL");
    return t;
  }
  Tensor calcVertexNormal(int64_t idx) const // src/SMPL.cpp:527-535 (batch 0)
  {
    need(verts_);
    Tensor t({3});
    check(smplpp_vertex_normals(m_.get(), 1, verts_.ptr(), 1, &idx, t.ptr(), SMPLPP_HOST, nullptr), "SMPL");
    return t;
  }
  const std::unordered_map<int64_t, float> & getAdjacentFaces(int64_t idx) const // src/SMPL.cpp:537-540
  {
    if(!adjacent_ || idx < 0 || idx >= V_) throw Exception("SMPL", "Cannot get adjacent faces!");
    return (*adjacent_)[(size_t)idx];
  }
  // SMPL::calcVertexNormal for every vertex of every frame of the last launch: [N,V,3]
  Tensor calcMeshVertexNormals() const
  {
    need(verts_);
    Tensor t(verts_.shape);
    check(smplpp_mesh_vertex_normals(m_.get(), verts_.size(0), verts_.ptr(), t.ptr(), SMPLPP_HOST, nullptr), "SMPL");
    return t;
  }
  // What backward() through calcNormal / calcVertexNormal / calcMeshVertexNormals on the last launch's vertices gave the reference
  // (the normal terms of node/node.cpp:803-869): dL/dverts [N,V,3] for dL/dnormals = gradNormal ([N,count,3] for the id lists,
  // [N,V,3] for the whole mesh).  `accumulate` non-null: the product is added into it (and it is returned), so normal and position
  // terms share one buffer that goes straight to launchBackward.  smplpp_face_normals_vjp / smplpp_vertex_normals_vjp /
  // smplpp_mesh_vertex_normals_vjp.
  Tensor calcNormalBackward(const std::vector<int64_t> & faceIds, const Tensor & gradNormal, Tensor * accumulate = nullptr) const
  {
    return normalsBackward(0, faceIds, gradNormal, accumulate);
  }
  Tensor calcVertexNormalBackward(const std::vector<int64_t> & vertexIds, const Tensor & gradNormal, Tensor * accumulate = nullptr) const
  {
    return normalsBackward(1, vertexIds, gradNormal, accumulate);
  }
  Tensor calcMeshVertexNormalsBackward(const Tensor & gradNormal, Tensor * accumulate = nullptr) const
  {
    return normalsBackward(2, {}, gradNormal, accumulate);
  }
  // Point-to-mesh distance on the last launch's vertices (fitting to a point cloud or scan): for points [N,K,3], the closest face of
  // each frame's mesh (smplpp_point_mesh_distance).  face [N,K] kInt64, weights [N,K,3] (the closest point's vertex weights),
  // closest [N,K,3] and sqdist [N,K]; face / closest / sqdist have the bits of smplpp_closest_points.
  struct PointMeshDistance
  {
    Tensor face, weights, closest, sqdist;
  };
  PointMeshDistance pointMeshDistance(const Tensor & points) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    if(points.dtype != kFloat32 || points.dim() != 3 || points.size(0) != n || points.size(1) < 1 || points.size(2) != 3)
      throw Exception("SMPL", "Cannot compute the point-to-mesh distance!");
    const int64_t K = points.size(1);
    PointMeshDistance r{Tensor({n, K}, kInt64), Tensor({n, K, 3}), Tensor({n, K, 3}), Tensor({n, K})};
    check(smplpp_point_mesh_distance(m_.get(), n, verts_.ptr(), K, points.ptr(), r.face.idata.data(), r.weights.ptr(), r.closest.ptr(),
                                     r.sqdist.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Its backward pass (smplpp_point_mesh_distance_vjp): dL/dverts [N,V,3] for dL/dsqdist = gradSqdist [N,K] at the faces `face` [N,K]
  // pointMeshDistance chose.  `gradPoints` non-null receives dL/dpoints [N,K,3].  `accumulate` non-null: the vertex product is added
  // into it (and it is returned), as calcNormalBackward does, and the point product into *gradPoints, which must then hold [N,K,3].
  Tensor pointMeshDistanceBackward(const Tensor & points, const Tensor & face, const Tensor & gradSqdist, Tensor * gradPoints = nullptr,
                                   Tensor * accumulate = nullptr) const
  {
    return distanceBackward(smplpp_point_mesh_distance_vjp, false, points, face, gradSqdist, gradPoints, accumulate,
                            "Cannot back-propagate through the point-to-mesh distance!");
  }
  // Mesh-to-point distance on the last launch's vertices (the other direction of pointMeshDistance): for points [N,K,3], the nearest
  // point to each vertex of each frame's mesh (smplpp_mesh_point_distance).  index [N,V] kInt64 (-1: no finite distance), sqdist [N,V].
  struct MeshPointDistance
  {
    Tensor index, sqdist;
  };
  MeshPointDistance meshPointDistance(const Tensor & points) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    if(points.dtype != kFloat32 || points.dim() != 3 || points.size(0) != n || points.size(1) < 1 || points.size(2) != 3)
      throw Exception("SMPL", "Cannot compute the mesh-to-point distance!");
    const int64_t K = points.size(1);
    MeshPointDistance r{Tensor({n, V_}, kInt64), Tensor({n, V_})};
    check(smplpp_mesh_point_distance(m_.get(), n, verts_.ptr(), K, points.ptr(), r.index.idata.data(), r.sqdist.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Its backward pass (smplpp_mesh_point_distance_vjp): dL/dverts [N,V,3] for dL/dsqdist = gradSqdist [N,V] at the points `index` [N,V]
  // meshPointDistance chose.  `gradPoints` non-null receives dL/dpoints [N,K,3].  `accumulate` non-null: the vertex product is added
  // into it (and it is returned), and the point product into *gradPoints, which must then hold [N,K,3].
  Tensor meshPointDistanceBackward(const Tensor & points, const Tensor & index, const Tensor & gradSqdist, Tensor * gradPoints = nullptr,
                                   Tensor * accumulate = nullptr) const
  {
    return distanceBackward(smplpp_mesh_point_distance_vjp, true, points, index, gradSqdist, gradPoints, accumulate,
                            "Cannot back-propagate through the mesh-to-point distance!");
  }
  // Normal-compatible, distance-capped correspondences on the last launch's vertices (smplpp_point_mesh_distance_compatible /
  // smplpp_mesh_point_distance_compatible, which state the rule).  pointNormals [N,K,3] need not be unit; an undefined tensor (Tensor()): no
  // normal test.  maxSqdist is the squared cap (+inf: none).  An unmatched row has face / index -1 and zeros elsewhere.  The faces go to
  // pointMeshDistanceCompatibleBackward, the indices straight to meshPointDistanceBackward (which ignores -1).
  PointMeshDistance pointMeshDistanceCompatible(const Tensor & points, const Tensor & pointNormals, float cosMin = 0.5f,
                                                float maxSqdist = std::numeric_limits<float>::infinity()) const
  {
    const char * what = "Cannot compute the compatible point-to-mesh distance!";
    const int64_t n = pointsFor(points, what), K = points.size(1);
    const bool normals = pointNormals.defined();
    if(normals && (pointNormals.dtype != kFloat32 || pointNormals.shape != points.shape)) throw Exception("SMPL", what);
    PointMeshDistance r{Tensor({n, K}, kInt64), Tensor({n, K, 3}), Tensor({n, K, 3}), Tensor({n, K})};
    check(smplpp_point_mesh_distance_compatible(m_.get(), n, verts_.ptr(), K, points.ptr(), normals ? pointNormals.ptr() : nullptr, cosMin,
                                                maxSqdist, r.face.idata.data(), r.weights.ptr(), r.closest.ptr(), r.sqdist.ptr(), SMPLPP_HOST,
                                                nullptr),
          "SMPL");
    return r;
  }
  // pointMeshDistanceBackward at the faces pointMeshDistanceCompatible chose: an unmatched query (face -1) contributes nothing (it
  // goes to smplpp_point_mesh_distance_vjp, which refuses -1 in host space, as face 0 with a zero cotangent).
  Tensor pointMeshDistanceCompatibleBackward(const Tensor & points, const Tensor & face, const Tensor & gradSqdist,
                                             Tensor * gradPoints = nullptr, Tensor * accumulate = nullptr) const
  {
    Tensor f = face, g = gradSqdist;
    if(f.idata.size() == g.data.size())
      for(size_t i = 0; i < f.idata.size(); i++)
        if(f.idata[i] < 0)
        {
          f.idata[i] = 0;
          g.data[i] = 0.0f;
        }
    return pointMeshDistanceBackward(points, f, g, gradPoints, accumulate);
  }
  // vertNormals [N,V,3] null: the whole-mesh vertex normals of the last launch (calcMeshVertexNormals)
  MeshPointDistance meshPointDistanceCompatible(const Tensor & points, const Tensor & pointNormals, float cosMin = 0.5f,
                                                float maxSqdist = std::numeric_limits<float>::infinity(),
                                                const Tensor * vertNormals = nullptr) const
  {
    const char * what = "Cannot compute the compatible mesh-to-point distance!";
    const int64_t n = pointsFor(points, what), K = points.size(1);
    const bool normals = pointNormals.defined();
    if(normals && (pointNormals.dtype != kFloat32 || pointNormals.shape != points.shape)) throw Exception("SMPL", what);
    if(vertNormals && (vertNormals->dtype != kFloat32 || vertNormals->shape != verts_.shape)) throw Exception("SMPL", what);
    Tensor own;
    if(normals && !vertNormals) own = calcMeshVertexNormals();
    const float * vn = !normals ? nullptr : vertNormals ? vertNormals->ptr() : own.ptr();
    MeshPointDistance r{Tensor({n, V_}, kInt64), Tensor({n, V_})};
    check(smplpp_mesh_point_distance_compatible(m_.get(), n, verts_.ptr(), vn, K, points.ptr(), normals ? pointNormals.ptr() : nullptr,
                                                cosMin, maxSqdist, r.index.idata.data(), r.sqdist.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Distance along the mesh's edges on the last launch's vertices (smplpp_mesh_geodesic, which states the rule): dist [N,S,V] from S
  // source sets, lists of vertex indices that the frames share (a set may be empty: its field is +inf).  +inf where no path leads and
  // where dist > maxDist (+inf: no cap).  A graph distance: an upper bound of the surface's.  smplpp::SelfContact (Contact.h) builds
  // the self-contact search on it.
  Tensor meshGeodesic(const std::vector<std::vector<int64_t>> & sources, float maxDist = std::numeric_limits<float>::infinity()) const
  {
    need(verts_);
    const int64_t n = verts_.size(0), S = (int64_t)sources.size();
    if(S < 1) throw Exception("SMPL", "Cannot compute the geodesic distance!");
    std::vector<int64_t> ptr(1, 0), ids;
    for(const auto & s : sources)
    {
      ids.insert(ids.end(), s.begin(), s.end());
      ptr.push_back((int64_t)ids.size());
    }
    ids.push_back(0); // (never an empty array)
    Tensor dist({n, S, V_});
    check(smplpp_mesh_geodesic(m_.get(), n, verts_.ptr(), S, ptr.data(), ids.data(), maxDist, dist.ptr(), SMPLPP_HOST, nullptr), "SMPL");
    return dist;
  }
  // Generalized winding numbers of each frame's mesh at points [N,K,3] on the last launch's vertices (smplpp_point_mesh_winding):
  // winding [N,K] (the bits calcSweepGrid's cells have at the same position), inside [N,K] kInt64 0 / 1 (winding > 0.5).
  struct PointMeshWinding
  {
    Tensor winding, inside;
  };
  PointMeshWinding pointMeshWinding(const Tensor & points) const
  {
    const int64_t n = pointsFor(points, "Cannot compute the winding numbers!"), K = points.size(1);
    std::vector<uint8_t> in((size_t)(n * K));
    PointMeshWinding r{Tensor({n, K}), Tensor({n, K}, kInt64)};
    check(smplpp_point_mesh_winding(m_.get(), n, verts_.ptr(), K, points.ptr(), r.winding.ptr(), in.data(), SMPLPP_HOST, nullptr), "SMPL");
    for(size_t i = 0; i < in.size(); i++) r.inside.idata[i] = in[i];
    return r;
  }
  // Signed point-to-mesh distance on the last launch's vertices (smplpp_point_mesh_signed_distance): pointMeshDistance's face,
  // weights and closest, pointMeshWinding's winding and inside, and signedSqdist [N,K] = -sqdist where inside, else sqdist.
  struct PointMeshSignedDistance
  {
    Tensor face, weights, closest, winding, inside, signedSqdist;
  };
  PointMeshSignedDistance pointMeshSignedDistance(const Tensor & points) const
  {
    const int64_t n = pointsFor(points, "Cannot compute the signed point-to-mesh distance!"), K = points.size(1);
    std::vector<uint8_t> in((size_t)(n * K));
    PointMeshSignedDistance r{Tensor({n, K}, kInt64), Tensor({n, K, 3}), Tensor({n, K, 3}), Tensor({n, K}), Tensor({n, K}, kInt64), Tensor({n, K})};
    check(smplpp_point_mesh_signed_distance(m_.get(), n, verts_.ptr(), K, points.ptr(), r.face.idata.data(), r.weights.ptr(), r.closest.ptr(),
                                            r.winding.ptr(), in.data(), r.signedSqdist.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    for(size_t i = 0; i < in.size(); i++) r.inside.idata[i] = in[i];
    return r;
  }
  // Its backward pass (smplpp_point_mesh_signed_distance_vjp) at the faces `face` and flags `inside` [N,K] (nonzero = inside) it
  // gave: pointMeshDistanceBackward at the cotangent gradSignedSqdist * (inside ? -1 : 1), with the same gradPoints / accumulate rules.
  Tensor pointMeshSignedDistanceBackward(const Tensor & points, const Tensor & face, const Tensor & inside, const Tensor & gradSignedSqdist,
                                         Tensor * gradPoints = nullptr, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot back-propagate through the signed point-to-mesh distance!";
    if((inside.dtype != kInt64 && inside.dtype != kInt32) || inside.numel() != face.numel()) throw Exception("SMPL", what);
    std::vector<uint8_t> in((size_t)inside.numel());
    for(size_t i = 0; i < in.size(); i++) in[i] = inside.idata[i] != 0 ? 1 : 0;
    return distanceBackward(smplpp_point_mesh_distance_vjp, false, points, face, gradSignedSqdist, gradPoints, accumulate, what, in.data());
  }
  // Ray casting against the last launch's meshes (smplpp_ray_cast): origin and dir [1,K,3] (one set of rays for every frame) or
  // [N,K,3]; dir is used as given, t is in units of |dir|.  face [N,K] kInt64 (-1: no hit), t [N,K] (0 without a hit), bary [N,K,3],
  // hits [N,K,2] kInt64 (front, back faces met in (tMin, tMax]).  facing: 1 front, 2 back, 3 both.
  struct RayCast
  {
    Tensor face, t, bary, hits;
  };
  RayCast rayCast(const Tensor & origin, const Tensor & dir, float tMin = 0.0f, float tMax = std::numeric_limits<float>::infinity(),
                  int facing = 3) const
  {
    int64_t rf = 0;
    const int64_t n = raysFor(origin, dir, rf, "Cannot cast the rays!"), K = origin.size(1);
    std::vector<int32_t> h((size_t)(n * K * 2));
    RayCast r{Tensor({n, K}, kInt64), Tensor({n, K}), Tensor({n, K, 3}), Tensor({n, K, 2}, kInt64)};
    check(smplpp_ray_cast(m_.get(), n, verts_.ptr(), rf, K, origin.ptr(), dir.ptr(), tMin, tMax, facing, r.face.idata.data(), r.t.ptr(),
                          r.bary.ptr(), h.data(), SMPLPP_HOST, nullptr),
          "SMPL");
    for(size_t i = 0; i < h.size(); i++) r.hits.idata[i] = h[i];
    return r;
  }
  // Its backward pass (smplpp_ray_cast_vjp) at the faces `face` [N,K] it gave, for gradT = dL/dt [N,K]: verts [N,V,3], origin and
  // dir in the rays' shape ([1,K,3]: the frames' sum).
  struct RayCastGrad
  {
    Tensor verts, origin, dir;
  };
  RayCastGrad rayCastBackward(const Tensor & origin, const Tensor & dir, const Tensor & face, const Tensor & gradT) const
  {
    const char * what = "Cannot back-propagate through the ray cast!";
    int64_t rf = 0;
    const int64_t n = raysFor(origin, dir, rf, what), K = origin.size(1);
    if(face.dtype != kInt64 || face.numel() != n * K || gradT.dtype != kFloat32 || gradT.numel() != n * K) throw Exception("SMPL", what);
    RayCastGrad r{Tensor({n, V_, 3}), Tensor({rf, K, 3}), Tensor({rf, K, 3})};
    check(smplpp_ray_cast_vjp(m_.get(), n, verts_.ptr(), rf, K, origin.ptr(), dir.ptr(), face.idata.data(), gradT.ptr(), r.verts.ptr(),
                              r.origin.ptr(), r.dir.ptr(), 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Self-intersections of the last launch's meshes (smplpp_self_intersections): pairs [N,maxPairs,2] kInt64 in ascending (f, g),
  // -1 past count, and count [N] kInt64, the true totals (a frame with more than maxPairs pairs keeps the lowest maxPairs).
  struct SelfIntersections
  {
    Tensor pairs, count;
  };
  SelfIntersections selfIntersections(int64_t maxPairs = 32768) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    SelfIntersections r{Tensor({n, maxPairs, 2}, kInt64), Tensor({n}, kInt64)};
    check(smplpp_self_intersections(m_.get(), n, verts_.ptr(), maxPairs, r.pairs.idata.data(), r.count.idata.data(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // selfIntersections and the self-penetration energy of each stored pair (smplpp_self_penetration): pairEnergy [N,maxPairs], 0 past count
  struct SelfPenetration
  {
    Tensor pairs, count, pairEnergy;
  };
  SelfPenetration selfPenetration(float sigma = 2.0f, int64_t maxPairs = 32768) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    SelfPenetration r{Tensor({n, maxPairs, 2}, kInt64), Tensor({n}, kInt64), Tensor({n, maxPairs})};
    check(smplpp_self_penetration(m_.get(), n, verts_.ptr(), maxPairs, sigma, r.pairs.idata.data(), r.count.idata.data(), r.pairEnergy.ptr(),
                                  SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Its backward pass (smplpp_self_penetration_vjp) at the pairs and count selfPenetration gave: dL/dverts [N,V,3] for
  // dL/dpairEnergy = gradPairEnergy [N,maxPairs].  `accumulate` non-null: the product is added into it (and it is returned).
  Tensor selfPenetrationBackward(const SelfPenetration & fwd, const Tensor & gradPairEnergy, float sigma = 2.0f,
                                 Tensor * accumulate = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot back-propagate through the self-penetration energy!";
    if(fwd.pairs.dim() != 3 || fwd.pairs.size(0) != n || fwd.count.numel() != n || gradPairEnergy.dtype != kFloat32 ||
       gradPairEnergy.numel() != fwd.pairEnergy.numel())
      throw Exception("SMPL", what);
    const int64_t maxPairs = fwd.pairs.size(1);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3) throw Exception("SMPL", what);
    }
    else
      out = Tensor({n, V_, 3});
    check(smplpp_self_penetration_vjp(m_.get(), n, verts_.ptr(), maxPairs, sigma, fwd.pairs.idata.data(), fwd.count.idata.data(),
                                      gradPairEnergy.ptr(), out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return out;
  }
  // The last launch's meshes through a pinhole camera into an H x W image (smplpp_depth_raster): face [N,H,W] kInt64 (-1 =
  // background), depth [N,H,W] (0 at background), bary [N,H,W,3], visible [N,V] kInt64 0 / 1, culled [N] kInt64.  camera [N,16] or
  // [16] (one camera for every frame): R row-major (world -> camera), t, fx, fy, cx, cy.
  struct DepthRaster
  {
    Tensor face, depth, bary, visible, culled;
  };
  DepthRaster depthRaster(const Tensor & camera, int64_t H, int64_t W, float near = 0.05f) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot rasterise the mesh!";
    const std::vector<float> cam = cameraRows(camera, n, what);
    if(H < 1 || W < 1) throw Exception("SMPL", what);
    std::vector<uint8_t> vis((size_t)(n * V_));
    DepthRaster r{Tensor({n, H, W}, kInt64), Tensor({n, H, W}), Tensor({n, H, W, 3}), Tensor({n, V_}, kInt64), Tensor({n}, kInt64)};
    check(smplpp_depth_raster(m_.get(), n, verts_.ptr(), cam.data(), H, W, near, r.face.idata.data(), r.depth.ptr(), r.bary.ptr(), vis.data(),
                              r.culled.idata.data(), SMPLPP_HOST, nullptr),
          "SMPL");
    for(size_t i = 0; i < vis.size(); i++) r.visible.idata[i] = vis[i];
    return r;
  }
  // Its backward pass (smplpp_depth_raster_vjp) at the faces `face` [N,H,W] it gave: dL/dverts [N,V,3] for dL/ddepth = gradDepth
  // [N,H,W].  `accumulate` non-null: the product is added into it (and it is returned).
  Tensor depthRasterBackward(const Tensor & camera, const Tensor & face, const Tensor & gradDepth, Tensor * accumulate = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot back-propagate through the depth image!";
    const std::vector<float> cam = cameraRows(camera, n, what);
    if(face.dim() != 3 || face.size(0) != n || (face.dtype != kInt64 && face.dtype != kInt32) || gradDepth.dtype != kFloat32 ||
       gradDepth.numel() != face.numel())
      throw Exception("SMPL", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3) throw Exception("SMPL", what);
    }
    else
      out = Tensor({n, V_, 3});
    check(smplpp_depth_raster_vjp(m_.get(), n, verts_.ptr(), cam.data(), face.size(1), face.size(2), face.idata.data(), gradDepth.ptr(),
                                  out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return out;
  }
  // A per-vertex quantity attr [N,V,C] (C <= 32) carried into the image of depthRaster (smplpp_raster_interpolate): image [N,H,W,C]
  // from `face` [N,H,W] and `bary` [N,H,W,3] as depthRaster gave them; 0 at background.
  Tensor rasterInterpolate(const Tensor & attr, const Tensor & face, const Tensor & bary) const
  {
    const char * what = "Cannot interpolate over the image!";
    if(attr.dim() != 3 || attr.dtype != kFloat32 || attr.size(1) != V_ || face.dim() != 3 || face.size(0) != attr.size(0) ||
       (face.dtype != kInt64 && face.dtype != kInt32) || bary.dtype != kFloat32 || bary.numel() != face.numel() * 3)
      throw Exception("SMPL", what);
    const int64_t n = attr.size(0), C = attr.size(2), H = face.size(1), W = face.size(2);
    Tensor image({n, H, W, C});
    check(smplpp_raster_interpolate(m_.get(), n, attr.ptr(), C, H, W, face.idata.data(), bary.ptr(), image.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return image;
  }
  // Its backward pass (smplpp_raster_interpolate_vjp) on the last launch's vertices, with the camera and near of the depthRaster call
  // that gave `face` and `bary`: dL/dattr [N,V,C] and, through the barycentrics, dL/dverts [N,V,3] for dL/dimage = gradImage
  // [N,H,W,C].  wantAttr / wantVerts false: that output stays undefined.  accumulate: an output that is defined on entry is added
  // into.
  struct RasterInterpolateGrad
  {
    Tensor attr, verts;
  };
  RasterInterpolateGrad rasterInterpolateBackward(const Tensor & attr, const Tensor & camera, const Tensor & face, const Tensor & bary,
                                                  const Tensor & gradImage, float near = 0.05f, bool wantAttr = true,
                                                  bool wantVerts = true, RasterInterpolateGrad * accumulate = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot back-propagate through the interpolated image!";
    const std::vector<float> cam = cameraRows(camera, n, what);
    if(attr.dim() != 3 || attr.dtype != kFloat32 || attr.size(0) != n || attr.size(1) != V_ || face.dim() != 3 || face.size(0) != n ||
       (face.dtype != kInt64 && face.dtype != kInt32) || bary.dtype != kFloat32 || bary.numel() != face.numel() * 3 ||
       gradImage.dtype != kFloat32 || gradImage.numel() != face.numel() * attr.size(2) || (!wantAttr && !wantVerts))
      throw Exception("SMPL", what);
    RasterInterpolateGrad local;
    RasterInterpolateGrad & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(wantAttr != out.attr.defined() || wantVerts != out.verts.defined() ||
         (wantAttr && (out.attr.dtype != kFloat32 || out.attr.numel() != attr.numel())) ||
         (wantVerts && (out.verts.dtype != kFloat32 || out.verts.numel() != n * V_ * 3)))
        throw Exception("SMPL", what);
    }
    else
    {
      if(wantAttr) out.attr = Tensor(attr.shape);
      if(wantVerts) out.verts = Tensor({n, V_, 3});
    }
    check(smplpp_raster_interpolate_vjp(m_.get(), n, attr.ptr(), attr.size(2), verts_.ptr(), cam.data(), face.size(1), face.size(2), near,
                                        face.idata.data(), bary.ptr(), gradImage.ptr(), wantAttr ? out.attr.ptr() : nullptr,
                                        wantVerts ? out.verts.ptr() : nullptr, accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return out;
  }
  // SMPL+D on the last launch (smplpp_vertex_offsets): the posed vertices and the rest shape of the body whose rest shape carries the
  // per-vertex offsets `offsets`, [V,3] or [1,V,3] (one field for every frame) or [N,V,3].  The stored launch is left as it is.
  struct VertexOffsets
  {
    Tensor verts, rest;
  };
  VertexOffsets vertexOffsets(const Tensor & offsets) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    if(offsets.dtype != kFloat32 || (offsets.numel() != V_ * 3 && offsets.numel() != n * V_ * 3))
      throw Exception("SMPL", "Cannot displace the vertices!");
    VertexOffsets r{Tensor({n, V_, 3}), Tensor({n, V_, 3})};
    check(smplpp_vertex_offsets(m_.get(), n, verts_.ptr(), xforms_.ptr(), offsets.ptr(), offsets.numel() / (V_ * 3), rest_.ptr(), r.rest.ptr(),
                                r.verts.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Its backward pass to the offsets (smplpp_vertex_offsets_vjp) at the last launch's transforms: dL/doffsets [N,V,3], or [1,V,3] with
  // `shared` (one field for every frame), for dL/dverts = gradVerts [N,V,3].  `accumulate` non-null: the product is added into it (and
  // it is returned).  (dL/dbeta and dL/dtheta of the displaced body: launchBackward's entry point with VertexOffsets::rest.)
  Tensor vertexOffsetsBackward(const Tensor & gradVerts, bool shared = false, Tensor * accumulate = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0), frames = shared ? 1 : n;
    const char * what = "Cannot back-propagate through the vertex offsets!";
    if(gradVerts.dtype != kFloat32 || gradVerts.numel() != n * V_ * 3) throw Exception("SMPL", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(accumulate->dtype != kFloat32 || accumulate->numel() != frames * V_ * 3) throw Exception("SMPL", what);
    }
    else
      out = Tensor({frames, V_, 3});
    check(smplpp_vertex_offsets_vjp(m_.get(), n, xforms_.ptr(), gradVerts.ptr(), frames, out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return out;
  }
  // The mesh Laplacian of a per-vertex field x [N,V,C], C <= 32 (smplpp_mesh_laplacian): twice the graph Laplacian on a closed manifold
  // mesh, and its own backward pass.  `accumulate` non-null: the result is added into it (and it is returned).
  Tensor meshLaplacian(const Tensor & x, Tensor * accumulate = nullptr) const
  {
    const char * what = "Cannot apply the mesh Laplacian!";
    if(x.dim() != 3 || x.dtype != kFloat32 || x.size(1) != V_) throw Exception("SMPL", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(accumulate->dtype != kFloat32 || accumulate->numel() != x.numel()) throw Exception("SMPL", what);
    }
    else
      out = Tensor(x.shape);
    check(smplpp_mesh_laplacian(m_.get(), x.size(0), x.ptr(), x.size(2), out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST, nullptr), "SMPL");
    return out;
  }
  // Bound points (smplpp_skin_points, smplpp_unskin_points and their backward passes): K points that are not the model's vertices,
  // carried by the blend of the joint transforms of `skeleton` (world [N,24,3,4], joints [N,24,3]).  points is [K,3] or [1,K,3] (one
  // cloud for every frame) or [N,K,3].  A binding is face [K] | [B,K] (kInt64) with bary [B,K,3], what pointMeshDistance returns as
  // face and weights, or dense weights [B,K,24] used as given, B = 1 or N; the other members stay empty.
  struct PointBinding
  {
    Tensor face, bary, weights;
  };
  // out [N,K,3]; blend [N,K,3,4], each point's own transform; valid [N,K] kInt64, 1 for a live point (a dead one gives zeros)
  struct BoundPoints
  {
    Tensor out, blend, valid;
  };
  BoundPoints skinPoints(const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & binding) const
  {
    return boundPoints(false, world, joints, points, binding);
  }
  // the inverse: points are posed points, out the rest-pose points that skinPoints carries onto them under the same binding
  BoundPoints unskinPoints(const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & binding) const
  {
    return boundPoints(true, world, joints, points, binding);
  }
  // points: shaped [P,K,3] like the cloud (P = 1: the frames' sum); world [N,24,3,4] and joints [N,24,3]: the cotangents
  // skeletonBackward takes; weights [B,K,24]: for a weight binding only (empty otherwise)
  struct BoundPointsGrad
  {
    Tensor points, world, joints, weights;
  };
  BoundPointsGrad skinPointsBackward(const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & binding,
                                     const Tensor & gradOut) const
  {
    return boundPointsBackward(false, world, joints, points, binding, gradOut);
  }
  BoundPointsGrad unskinPointsBackward(const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & binding,
                                       const Tensor & gradOut) const
  {
    return boundPointsBackward(true, world, joints, points, binding, gradOut);
  }
  // Exact Euclidean feature transform of binary images mask [N,H,W] (integer tensor, nonzero = set; smplpp_mask_distance_transform):
  // nearest [N,H,W] kInt64 (the linear index of the nearest set pixel of the frame, the lowest among equal distances; -1 without a
  // set pixel) and sqdist [N,H,W] kInt64 (px^2).
  struct MaskDistance
  {
    Tensor nearest, sqdist;
  };
  MaskDistance maskDistanceTransform(const Tensor & mask) const
  {
    const char * what = "Cannot transform the mask!";
    const std::vector<uint8_t> mk = maskBytes(mask, what);
    const int64_t n = mask.size(0), H = mask.size(1), W = mask.size(2);
    MaskDistance r{Tensor({n, H, W}, kInt64), Tensor({n, H, W}, kInt64)};
    std::vector<int32_t> sq(mk.size());
    check(smplpp_mask_distance_transform(m_.get(), n, mk.data(), H, W, r.nearest.idata.data(), sq.data(), SMPLPP_HOST, nullptr), "SMPL");
    for(size_t i = 0; i < sq.size(); i++) r.sqdist.idata[i] = sq[i];
    return r;
  }
  // The silhouette residuals of the last launch's meshes against the target mask [N,H,W] (smplpp_silhouette), at the face image
  // `face` [N,H,W] depthRaster gave for the same camera and near: vertTarget [N,V] kInt64 and vertSq [N,V] (model -> mask, px^2),
  // pixSource [N,H,W] kInt64 and pixSq [N,H,W] (mask -> model); -1 and 0 where there is no residual.
  struct Silhouette
  {
    Tensor vertTarget, vertSq, pixSource, pixSq;
  };
  Silhouette silhouette(const Tensor & camera, const Tensor & face, const Tensor & mask, float near = 0.05f) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot evaluate the silhouette term!";
    const std::vector<float> cam = cameraRows(camera, n, what);
    const std::vector<uint8_t> mk = maskBytes(mask, what);
    if(face.dim() != 3 || face.size(0) != n || (face.dtype != kInt64 && face.dtype != kInt32) || mask.shape != face.shape)
      throw Exception("SMPL", what);
    const int64_t H = face.size(1), W = face.size(2);
    Silhouette r{Tensor({n, V_}, kInt64), Tensor({n, V_}), Tensor({n, H, W}, kInt64), Tensor({n, H, W})};
    check(smplpp_silhouette(m_.get(), n, verts_.ptr(), cam.data(), H, W, near, face.idata.data(), mk.data(), r.vertTarget.idata.data(),
                            r.vertSq.ptr(), r.pixSource.idata.data(), r.pixSq.ptr(), SMPLPP_HOST, nullptr),
          "SMPL");
    return r;
  }
  // Its backward pass (smplpp_silhouette_vjp) at the correspondences `fwd` and the face image: dL/dverts [N,V,3] for dL/dvertSq =
  // gradVertSq [N,V] and dL/dpixSq = gradPixSq [N,H,W]; an undefined (default-constructed) cotangent is left out.  `accumulate`
  // non-null: the product is added into it (and it is returned).
  Tensor silhouetteBackward(const Tensor & camera, const Tensor & face, const Silhouette & fwd, const Tensor & gradVertSq,
                            const Tensor & gradPixSq, float near = 0.05f, Tensor * accumulate = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const char * what = "Cannot back-propagate through the silhouette term!";
    const std::vector<float> cam = cameraRows(camera, n, what);
    const bool gv = gradVertSq.defined(), gp = gradPixSq.defined();
    if(face.dim() != 3 || face.size(0) != n || (face.dtype != kInt64 && face.dtype != kInt32) || (!gv && !gp) ||
       (gv && (gradVertSq.dtype != kFloat32 || gradVertSq.numel() != n * V_ || fwd.vertTarget.numel() != n * V_)) ||
       (gp && (gradPixSq.dtype != kFloat32 || gradPixSq.numel() != face.numel() || fwd.pixSource.numel() != face.numel())))
      throw Exception("SMPL", what);
    Tensor local;
    Tensor & out = accumulate ? *accumulate : local;
    if(accumulate)
    {
      if(accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3) throw Exception("SMPL", what);
    }
    else
      out = Tensor({n, V_, 3});
    check(smplpp_silhouette_vjp(m_.get(), n, verts_.ptr(), cam.data(), face.size(1), face.size(2), near, face.idata.data(),
                                gv ? fwd.vertTarget.idata.data() : nullptr, gp ? fwd.pixSource.idata.data() : nullptr,
                                gv ? gradVertSq.ptr() : nullptr, gp ? gradPixSq.ptr() : nullptr, out.ptr(), accumulate ? 1 : 0, SMPLPP_HOST,
                                nullptr),
          "SMPL");
    return out;
  }
  // The sweep grid of node/node.cpp:1023-1073 for frame `index`: the grid indices (cell position = 0.025 m x index) whose
  // winding number exceeds 0.5 — the keys the reference enters into g_sweepGridList
  std::vector<std::array<int32_t, 3>> calcSweepGrid(int64_t index = 0) const
  {
    need(verts_);
    const float * v = verts_.ptr() + (size_t)index * V_ * 3;
    int32_t g0[3], gn[3];
    int64_t cells = 0;
    check(smplpp_sweep_grid(m_.get(), v, g0, gn, 0, nullptr, nullptr, &cells, SMPLPP_HOST, nullptr), "SMPL");
    std::vector<uint8_t> inside((size_t)cells);
    check(smplpp_sweep_grid(m_.get(), v, g0, gn, cells, nullptr, inside.data(), &cells, SMPLPP_HOST, nullptr), "SMPL");
    std::vector<std::array<int32_t, 3>> out;
    int64_t i = 0;
    for(int32_t x = 0; x < gn[0]; x++)
      for(int32_t y = 0; y < gn[1]; y++)
        for(int32_t z = 0; z < gn[2]; z++, i++)
          if(inside[(size_t)i]) out.push_back({g0[0] + x, g0[1] + y, g0[2] + z});
    return out;
  }
  // SMPL::out (src/SMPL.cpp:757-790): Wavefront OBJ of frame `index` of the last launch into the path of setVertPath
  void out(int64_t index) const
  {
    if(verts_.data.empty() || index < 0 || index >= verts_.size(0) || vertPath_.empty()) throw Exception("SMPL", "Cannot export the deformed mesh!");
    std::ofstream f(vertPath_);
    if(!f) throw Exception("SMPL", "Cannot export the deformed mesh!");
    for(int64_t v = 0; v < V_; v++)
      f << 'v' << ' ' << verts_.data[((size_t)index * V_ + v) * 3] << ' ' << verts_.data[((size_t)index * V_ + v) * 3 + 1] << ' '
        << verts_.data[((size_t)index * V_ + v) * 3 + 2] << '\n';
    for(int64_t t = 0; t < F_; t++)
      f << 'f' << ' ' << faces1_.idata[(size_t)t * 3] << ' ' << faces1_.idata[(size_t)t * 3 + 1] << ' ' << faces1_.idata[(size_t)t * 3 + 2] << '\n';
  }

  smplpp_model * handle() const { return m_.get(); }
  int64_t vertexNum() const { return V_; }
  int64_t faceNum() const { return F_; }

private:
  // the argument checks of the skeleton calls
  static const float * optional(const Tensor & t) { return t.data.empty() ? nullptr : t.ptr(); }
  void checkSkeletonRotmat(const Tensor & beta, const Tensor & trans, const Tensor & rot) const
  {
    if(!m_ || rot.shape.size() != 4 || rot.size(1) != JOINT_NUM || rot.size(2) != 3 || rot.size(3) != 3 || rot.dtype != kFloat32
       || (!beta.data.empty() && (beta.numel() != rot.size(0) * SHAPE_BASIS_DIM || beta.dtype != kFloat32))
       || (!trans.data.empty() && (trans.numel() != rot.size(0) * 3 || trans.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot pose the skeleton of a SMPL model!");
  }
  static void checkSkeletonGrads(int64_t n, const Tensor & gw, const Tensor & gp, const Tensor & gj)
  {
    const bool hw = !gw.data.empty(), hp = !gp.data.empty(), hj = !gj.data.empty();
    if((!hw && !hp && !hj) || (hw && (gw.numel() != n * JOINT_NUM * 12 || gw.dtype != kFloat32))
       || (hp && (gp.numel() != n * JOINT_NUM * 3 || gp.dtype != kFloat32)) || (hj && (gj.numel() != n * JOINT_NUM * 3 || gj.dtype != kFloat32)))
      throw Exception("SMPL", "Cannot back-propagate through the skeleton of a SMPL model!");
  }
  // the shapes of a bound-points call: frames n, points K, the frames of the cloud and of the binding
  struct BoundShape
  {
    int64_t n, K, pointFrames, bindFrames;
    bool byWeights;
  };
  BoundShape checkBound(const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & b, const char * what) const
  {
    const bool hw = !b.weights.data.empty(), hf = !b.face.idata.empty(), hb = !b.bary.data.empty();
    if(!m_ || world.dim() != 4 || world.size(1) != JOINT_NUM || world.size(2) != 3 || world.size(3) != 4 || world.dtype != kFloat32
       || world.size(0) < 1 || joints.dtype != kFloat32 || joints.numel() != world.size(0) * JOINT_NUM * 3 || points.dtype != kFloat32
       || points.dim() < 2 || points.dim() > 3 || points.size(points.dim() - 1) != 3 || points.numel() < 3 || hw == (hf || hb) || hf != hb)
      throw Exception("SMPL", what);
    BoundShape s{world.size(0), points.size(points.dim() - 2), points.dim() == 3 ? points.size(0) : 1, 0, hw};
    const int64_t rows = hw ? b.weights.numel() / JOINT_NUM : b.bary.numel() / 3;
    s.bindFrames = rows / s.K;
    if((s.pointFrames != 1 && s.pointFrames != s.n) || rows % s.K != 0 || (s.bindFrames != 1 && s.bindFrames != s.n)
       || (hw ? b.weights.dtype != kFloat32 || b.weights.numel() != rows * JOINT_NUM
              : b.bary.dtype != kFloat32 || b.bary.numel() != rows * 3 || b.face.dtype != kInt64 || b.face.numel() != rows))
      throw Exception("SMPL", what);
    return s;
  }
  BoundPoints boundPoints(bool unskin, const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & b) const
  {
    const BoundShape s = checkBound(world, joints, points, b, unskin ? "Cannot unskin the points!" : "Cannot skin the points!");
    BoundPoints r{Tensor({s.n, s.K, 3}), Tensor({s.n, s.K, 3, 4}), Tensor({s.n, s.K}, kInt64)};
    std::vector<uint8_t> valid((size_t)(s.n * s.K));
    check((unskin ? smplpp_unskin_points : smplpp_skin_points)(m_.get(), s.n, world.ptr(), joints.ptr(), s.K, points.ptr(), s.pointFrames,
                                                              s.byWeights ? nullptr : b.face.idata.data(), optional(b.bary), optional(b.weights),
                                                              s.bindFrames, r.out.ptr(), r.blend.ptr(), valid.data(), SMPLPP_HOST, nullptr),
          "SMPL");
    for(size_t i = 0; i < valid.size(); i++) r.valid.idata[i] = valid[i];
    return r;
  }
  BoundPointsGrad boundPointsBackward(bool unskin, const Tensor & world, const Tensor & joints, const Tensor & points, const PointBinding & b,
                                      const Tensor & gradOut) const
  {
    const char * what = "Cannot back-propagate through the bound points!";
    const BoundShape s = checkBound(world, joints, points, b, what);
    if(gradOut.dtype != kFloat32 || gradOut.numel() != s.n * s.K * 3) throw Exception("SMPL", what);
    BoundPointsGrad g{Tensor({s.pointFrames, s.K, 3}), Tensor({s.n, JOINT_NUM, 3, 4}), Tensor({s.n, JOINT_NUM, 3}),
                      s.byWeights ? Tensor({s.bindFrames, s.K, JOINT_NUM}) : Tensor()};
    check((unskin ? smplpp_unskin_points_vjp : smplpp_skin_points_vjp)(
              m_.get(), s.n, world.ptr(), joints.ptr(), s.K, points.ptr(), s.pointFrames, s.byWeights ? nullptr : b.face.idata.data(),
              optional(b.bary), optional(b.weights), s.bindFrames, gradOut.ptr(), g.points.ptr(), g.world.ptr(), g.joints.ptr(),
              s.byWeights ? g.weights.ptr() : nullptr, 0, SMPLPP_HOST, nullptr),
          "SMPL");
    return g;
  }
  // an integer mask tensor [N,H,W] as bytes (nonzero = set)
  static std::vector<uint8_t> maskBytes(const Tensor & mask, const char * what)
  {
    if(mask.dim() != 3 || (mask.dtype != kInt64 && mask.dtype != kInt32) || mask.numel() < 1) throw Exception("SMPL", what);
    std::vector<uint8_t> b(mask.idata.size());
    for(size_t i = 0; i < b.size(); i++) b[i] = mask.idata[i] != 0;
    return b;
  }
  static const Tensor & need(const Tensor & t)
  {
    if(t.data.empty()) throw Exception("LinearBlendSknning", "Failed to get vertices of new pose!"); // LinearBlendSkinning.cpp:413
    return t;
  }
  // T of a forward-mode call: every non-empty tangent holds tf x T rows of its width
  static int64_t tangentCount(int64_t tf, std::initializer_list<const Tensor *> tangents, std::initializer_list<int64_t> widths)
  {
    int64_t T = 0;
    auto w = widths.begin();
    for(const Tensor * t : tangents)
    {
      const int64_t row = tf * *w++;
      if(t->data.empty()) continue;
      if(t->dtype != kFloat32 || t->numel() == 0 || t->numel() % row != 0 || (T && t->numel() / row != T))
        throw Exception("SMPL", "Cannot push a tangent through a SMPL model!");
      T = t->numel() / row;
    }
    if(T == 0) throw Exception("SMPL", "Cannot push a tangent through a SMPL model!");
    return T;
  }
  Tensor normalsBackward(int kind, const std::vector<int64_t> & ids, const Tensor & gradNormal, Tensor * accumulate) const
  {
    need(verts_);
    const int64_t n = verts_.size(0), rows = kind == 2 ? V_ : (int64_t)ids.size();
    if(gradNormal.dtype != kFloat32 || gradNormal.numel() != n * rows * 3 || (kind != 2 && ids.empty()) ||
       (accumulate && (accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3)))
      throw Exception("SMPL", "Cannot back-propagate through the normals!");
    Tensor fresh;
    if(!accumulate) fresh = Tensor(verts_.shape);
    Tensor & g = accumulate ? *accumulate : fresh;
    const int acc = accumulate ? 1 : 0;
    if(kind == 2)
      check(smplpp_mesh_vertex_normals_vjp(m_.get(), n, verts_.ptr(), gradNormal.ptr(), g.ptr(), acc, SMPLPP_HOST, nullptr), "SMPL");
    else
      check((kind == 1 ? smplpp_vertex_normals_vjp : smplpp_face_normals_vjp)(m_.get(), n, verts_.ptr(), rows, ids.data(), gradNormal.ptr(),
                                                                             g.ptr(), acc, SMPLPP_HOST, nullptr),
            "SMPL");
    return g;
  }
  std::vector<float> cameraRows(const Tensor & camera, int64_t n, const char * what) const // camera [16] or [N,16] as N rows
  {
    if(camera.dtype != kFloat32 || !(camera.numel() == 16 || (camera.dim() == 2 && camera.size(0) == n && camera.size(1) == 16)))
      throw Exception("SMPL", what);
    std::vector<float> rows((size_t)(n * 16));
    for(size_t i = 0; i < rows.size(); i++) rows[i] = camera.data[camera.numel() == 16 ? i % 16 : i];
    return rows;
  }
  int64_t pointsFor(const Tensor & points, const char * what) const // frames of the last launch, checked against points [N,K,3]
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    if(points.dtype != kFloat32 || points.dim() != 3 || points.size(0) != n || points.size(1) < 1 || points.size(2) != 3)
      throw Exception("SMPL", what);
    return n;
  }
  // frames of the last launch, checked against rays origin and dir [1 or N,K,3]; rf = the rays' frames
  int64_t raysFor(const Tensor & origin, const Tensor & dir, int64_t & rf, const char * what) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    if(origin.dtype != kFloat32 || dir.dtype != kFloat32 || origin.dim() != 3 || origin.shape != dir.shape || (origin.size(0) != 1 && origin.size(0) != n)
       || origin.size(1) < 1 || origin.size(2) != 3)
      throw Exception("SMPL", what);
    rf = origin.size(0);
    return n;
  }
  // the *DistanceBackward: ids and gradSqdist hold one entry per vertex (perVertex) or per point; inside non-null: the signed distance's
  Tensor distanceBackward(decltype(&smplpp_point_mesh_distance_vjp) vjp, bool perVertex, const Tensor & points, const Tensor & ids,
                          const Tensor & gradSqdist, Tensor * gradPoints, Tensor * accumulate, const char * what,
                          const uint8_t * inside = nullptr) const
  {
    need(verts_);
    const int64_t n = verts_.size(0);
    const int64_t K = points.dim() == 3 ? points.size(1) : 0, rows = n * (perVertex ? V_ : K);
    if(points.dtype != kFloat32 || points.dim() != 3 || points.size(0) != n || K < 1 || points.size(2) != 3 ||
       (ids.dtype != kInt64 && ids.dtype != kInt32) || ids.numel() != rows || gradSqdist.dtype != kFloat32 || gradSqdist.numel() != rows ||
       (accumulate && (accumulate->dtype != kFloat32 || accumulate->numel() != n * V_ * 3)) ||
       (accumulate && gradPoints && (gradPoints->dtype != kFloat32 || gradPoints->numel() != n * K * 3)))
      throw Exception("SMPL", what);
    Tensor fresh;
    if(!accumulate) fresh = Tensor(verts_.shape);
    Tensor & g = accumulate ? *accumulate : fresh;
    if(gradPoints && !accumulate) *gradPoints = Tensor({n, K, 3});
    if(inside)
      check(smplpp_point_mesh_signed_distance_vjp(m_.get(), n, verts_.ptr(), K, points.ptr(), ids.idata.data(), inside, gradSqdist.ptr(), g.ptr(),
                                                  gradPoints ? gradPoints->ptr() : nullptr, accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
            "SMPL");
    else
      check(vjp(m_.get(), n, verts_.ptr(), K, points.ptr(), ids.idata.data(), gradSqdist.ptr(), g.ptr(),
                gradPoints ? gradPoints->ptr() : nullptr, accumulate ? 1 : 0, SMPLPP_HOST, nullptr),
            "SMPL");
    return g;
  }
  std::shared_ptr<smplpp_model> m_;
  std::shared_ptr<const std::vector<std::unordered_map<int64_t, float>>> adjacent_;
  Device device_;
  std::string path_, vertPath_;
  int64_t V_ = 0, F_ = 0;
  Tensor faces1_;
  Tensor verts_, rest_, joints_, xforms_;
  Tensor beta_, theta_; // inputs of the last launch (launchBackward)
  Tensor betaR_, transR_, rot_; // inputs of the last launchRotmat (launchRotmatBackward)
};
} // namespace smplpp
#endif
