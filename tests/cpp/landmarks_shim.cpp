// smplpp::Landmarks (regress / regressBackward) and smplpp::projectPoints / projectPointsBackward through the header-only C++ shim on
// a launch; driven by tests/test_keypoints_gpu.py, which restates these inputs and compares every output with the Python binding's,
// bit for bit.
// usage: landmarks_shim <model.json> <out.bin>
//   (out, float32: points, uv, energy, valid, grad_points, grad_camera, grad_camera added into ones, grad_verts, grad_joints)
#include <cstdio>

#include <smplpp/Landmarks.h>

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  try
  {
    auto smpl = std::make_shared<smplpp::SMPL>();
    smpl->setDevice(smplpp::Device("CUDA", 0));
    smpl->setModelPath(argv[1]);
    smpl->init();
    const int64_t n = 3, L = 6;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    const int64_t S = smpl->vertexNum() + 24;
    // a joint pick, a vertex pick, four rows of nine entries
    std::vector<int64_t> rowPtr = {0, 1, 2}, col = {smpl->vertexNum() + 3, 7};
    std::vector<float> val = {1.0f, 1.0f};
    for(int64_t l = 2; l < L; l++)
    {
      for(int64_t i = 0; i < 9; i++)
      {
        col.push_back((l * 7 + i * 5) % S);
        val.push_back((float)(i % 4 + 1) * 0.125f - 0.2f);
      }
      rowPtr.push_back((int64_t)col.size());
    }
    const smplpp::Landmarks lm(*smpl, rowPtr, col, val);
    const smplpp::Tensor points = lm.regress(smpl->getVertex(), smpl->getRestJoint());
    smplpp::Tensor camera({16});
    const float cam[16] = {1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 3, 300, 300, 160, 120};
    for(int i = 0; i < 16; i++) camera.data[(size_t)i] = cam[i];
    smplpp::Tensor target({n, L, 3}), gradUv({n, L, 2}), gradEnergy({n, L});
    for(int64_t i = 0; i < n * L; i++)
    {
      target.data[(size_t)i * 3] = 160.0f + (float)(i % 7) * 3.0f;
      target.data[(size_t)i * 3 + 1] = 120.0f - (float)(i % 5) * 4.0f;
      target.data[(size_t)i * 3 + 2] = (float)(i % 3) * 0.5f;
      gradEnergy.data[(size_t)i] = (float)(i % 4) * 0.25f;
    }
    for(int64_t i = 0; i < gradUv.numel(); i++) gradUv.data[(size_t)i] = (float)(i % 5 - 2) * 0.5f;
    const float rho = 100.0f;
    const smplpp::Projection p = smplpp::projectPoints(points, camera, target, rho);
    const smplpp::ProjectionGradients g = smplpp::projectPointsBackward(points, camera, target, rho, gradUv, gradEnergy);
    smplpp::ProjectionGradients acc{smplpp::Tensor({n, L, 3}, 1.0f), smplpp::Tensor({n, 16}, 1.0f)};
    smplpp::projectPointsBackward(points, camera, target, rho, gradUv, gradEnergy, 0.05f, &acc);
    const smplpp::Landmarks::Gradients back = lm.regressBackward(g.points);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    for(const smplpp::Tensor & t : {points, p.uv, p.energy, p.valid.to(smplpp::kFloat32), g.points, g.camera, acc.camera, back.verts, back.joints})
      std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
