// SMPL::launchBackward through the header-only C++ shim; driven by tests/test_fk_vjp_gpu.py, which restates these inputs and compares
// the printed gradients with the Python binding's.
// usage: fk_vjp_shim <model.json>
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
    const int64_t n = 2, V = smpl->vertexNum();
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), gv({n, V, 3}), gj({n, 24, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < gv.numel(); i++) gv.data[(size_t)i] = (float)(i % 13 - 6) * 0.1f;
    for(int64_t i = 0; i < gj.numel(); i++) gj.data[(size_t)i] = (float)(i % 5 - 2) * 0.1f;
    smpl->launch(beta, theta);
    auto g = smpl->launchBackward(gv, gj);
    dump("GRAD_BETA", g.first);
    dump("GRAD_THETA", g.second);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
