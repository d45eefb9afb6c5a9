// SMPL::launchTangent and SMPL::launchRotmatTangent through the header-only C++ shim; driven by tests/test_fk_jvp_gpu.py, which
// restates these inputs and compares the printed tangents with the Python binding's.
// usage: fk_jvp_shim <model.json>
#include <cstdio>

#include <smplpp/SMPL.h>

static void dump(const char * key, const smplpp::Tensor & t)
{
  std::printf("%s", key);
  for(float x : t.toVector<float>()) std::printf(" %.9g", (double)x);
  std::printf("\n");
}

static void fill(smplpp::Tensor & t, int mod, int off, float scale)
{
  for(int64_t i = 0; i < t.numel(); i++) t.data[(size_t)i] = (float)(i % mod - off) * scale;
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
    const int64_t n = 2, T = 3;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), dbeta({n, T, 10}), dtheta({n, T, 25, 3}), sbeta({T, 10}), drot({T, 24, 3, 3}), dtrans({T, 3});
    fill(beta, 7, 3, 0.1f);
    fill(theta, 11, 5, 0.05f);
    fill(dbeta, 5, 2, 0.25f);
    fill(dtheta, 13, 6, 0.125f);
    fill(sbeta, 3, 1, 0.5f);
    fill(drot, 9, 4, 0.0625f);
    fill(dtrans, 4, 1, 0.5f);
    smpl->launch(beta, theta);
    auto a = smpl->launchTangent(dbeta, dtheta);
    dump("VERTS", a.verts);
    dump("JOINTS", a.joints);
    dump("WORLD", a.world);
    smplpp::Tensor aa({n, 24, 3}), trans({n, 3});
    for(int64_t f = 0; f < n; f++)
      for(int64_t i = 0; i < 75; i++) (i < 3 ? trans.data[(size_t)(f * 3 + i)] : aa.data[(size_t)(f * 72 + i - 3)]) = theta.data[(size_t)(f * 75 + i)];
    smpl->launchRotmat(beta, trans, smpl->axisAngleToRotmat(aa));
    auto r = smpl->launchRotmatTangent(sbeta, dtrans, drot, true);
    dump("R_VERTS", r.verts);
    dump("R_JOINTS", r.joints);
    dump("R_WORLD", r.world);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
