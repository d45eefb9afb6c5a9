// SMPL::calcNormalBackward / calcVertexNormalBackward / calcMeshVertexNormalsBackward through the header-only C++ shim, accumulated
// into one buffer; driven by tests/test_normals_vjp_gpu.py, which restates these inputs and compares the gradient with the Python
// binding's.
// usage: normals_vjp_shim <model.json> <out.bin>
#include <cstdio>

#include <smplpp/SMPL.h>

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  try
  {
    auto smpl = std::make_shared<smplpp::SMPL>();
    smpl->setDevice(smplpp::Device("CUDA", 0));
    smpl->setModelPath(argv[1]);
    smpl->init();
    const int64_t n = 2, V = smpl->vertexNum();
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), gm({n, V, 3}), g1({n, 4, 3}), g2({n, 4, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < gm.numel(); i++) gm.data[(size_t)i] = (float)(i % 13 - 6) * 0.1f;
    for(int64_t i = 0; i < g1.numel(); i++) g1.data[(size_t)i] = (float)(i % 5 - 2) * 0.1f;
    for(int64_t i = 0; i < g2.numel(); i++) g2.data[(size_t)i] = (float)(i % 3 - 1) * 0.2f;
    smpl->launch(beta, theta);
    const std::vector<int64_t> ids = {3, 7, 3, 11};
    smplpp::Tensor g = smpl->calcMeshVertexNormalsBackward(gm);
    smpl->calcVertexNormalBackward(ids, g1, &g);
    smpl->calcNormalBackward(ids, g2, &g);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    std::fwrite(g.data.data(), sizeof(float), g.data.size(), f);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
