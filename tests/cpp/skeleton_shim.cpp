// SMPL::skeleton, skeletonBackward, skeletonRotmat and skeletonRotmatBackward through the header-only C++ shim; driven by
// tests/test_skeleton_gpu.py, which restates these inputs and compares the printed values with the Python binding's.
// usage: skeleton_shim <model.json>
#include <cstdio>

#include <smplpp/SMPL.h>

static void dump(const char * key, const smplpp::Tensor & t)
{
  std::printf("%s", key);
  for(float x : t.toVector<float>()) std::printf(" %.9g", (double)x);
  std::printf("\n");
}

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    auto smpl = std::make_shared<smplpp::SMPL>();
    smpl->setDevice(smplpp::Device("CUDA", 0));
    smpl->setModelPath(argv[1]);
    smpl->init();
    const int64_t n = 5;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), gw({n, 24, 3, 4}), gp({n, 24, 3}), gj({n, 24, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < gw.numel(); i++) gw.data[(size_t)i] = (float)(i % 13 - 6) * 0.1f;
    for(int64_t i = 0; i < gp.numel(); i++) gp.data[(size_t)i] = (float)(i % 9 - 4) * 0.25f;
    for(int64_t i = 0; i < gj.numel(); i++) gj.data[(size_t)i] = (float)(i % 5 - 2) * 0.1f;
    const smplpp::SMPL::Skeleton s = smpl->skeleton(beta, theta);
    dump("WORLD", s.world);
    dump("POSED", s.posed);
    dump("JOINTS", s.joints);
    const auto g = smpl->skeletonBackward(beta, theta, gw, gp, gj);
    dump("GRAD_BETA", g.first);
    dump("GRAD_THETA", g.second);
    // the rotation-matrix entry on matrices that are not orthonormal (used as given)
    smplpp::Tensor aa({n, 24, 3}), trans({n, 3});
    for(int64_t f = 0; f < n; f++)
      for(int64_t i = 0; i < 75; i++)
        (i < 3 ? trans.data[(size_t)(f * 3 + i)] : aa.data[(size_t)(f * 72 + i - 3)]) = theta.data[(size_t)(f * 75 + i)];
    smplpp::Tensor bent = smpl->axisAngleToRotmat(aa);
    for(int64_t i = 0; i < bent.numel(); i++) bent.data[(size_t)i] += (float)(i % 17 - 8) * 0.005f;
    const smplpp::SMPL::Skeleton r = smpl->skeletonRotmat(beta, trans, bent);
    dump("R_WORLD", r.world);
    dump("R_POSED", r.posed);
    dump("R_JOINTS", r.joints);
    const auto h = smpl->skeletonRotmatBackward(beta, trans, bent, gw, smplpp::Tensor(), gj);
    dump("R_GRAD_BETA", std::get<0>(h));
    dump("R_GRAD_TRANS", std::get<1>(h));
    dump("R_GRAD_ROT", std::get<2>(h));
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
