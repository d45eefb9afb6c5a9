// SMPL::axisAngleToRotmat, launchRotmat and launchRotmatBackward through the header-only C++ shim; driven by
// tests/test_fk_rotmat_gpu.py, which restates these inputs and compares the printed values with the Python binding's.
// usage: fk_rotmat_shim <model.json>
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
    const int64_t n = 33, V = smpl->vertexNum();
    smplpp::Tensor beta({n, 10}), trans({n, 3}), aa({n, 24, 3}), gv({n, V, 3}), gj({n, 24, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < trans.numel(); i++) trans.data[(size_t)i] = (float)(i % 9 - 4) * 0.25f;
    for(int64_t i = 0; i < aa.numel(); i++) aa.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < gv.numel(); i++) gv.data[(size_t)i] = (float)(i % 13 - 6) * 0.1f;
    for(int64_t i = 0; i < gj.numel(); i++) gj.data[(size_t)i] = (float)(i % 5 - 2) * 0.1f;
    const smplpp::Tensor rot = smpl->axisAngleToRotmat(aa);
    // (not orthonormal: the matrices are used as given)
    smplpp::Tensor bent = rot;
    for(int64_t i = 0; i < bent.numel(); i++) bent.data[(size_t)i] += (float)(i % 17 - 8) * 0.005f;
    smpl->launchRotmat(beta, trans, bent);
    dump("ROT", rot);
    dump("VERTS", smpl->getVertex());
    dump("JOINTS", smpl->getRestJoint());
    dump("XFORMS", smpl->getTransformation());
    dump("REST", smpl->getRestShape());
    auto g = smpl->launchRotmatBackward(gv, gj);
    dump("GRAD_BETA", std::get<0>(g));
    dump("GRAD_TRANS", std::get<1>(g));
    dump("GRAD_ROT", std::get<2>(g));
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
