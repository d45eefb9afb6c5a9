// SMPL::selfIntersections / selfPenetration / selfPenetrationBackward through the header-only C++ shim on the last launch's vertices;
// driven by tests/test_self_penetration_gpu.py, which restates these inputs and compares every output with the Python binding's, bit
// for bit.
// usage: self_penetration_shim <model.json> <out.bin>
//   (out: pairs, count | pairs, count, pair_energy | grad_verts, all int64 or float32)
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
    const int64_t n = 2, maxPairs = 4096;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    const smplpp::SMPL::SelfIntersections si = smpl->selfIntersections(maxPairs);
    const smplpp::SMPL::SelfPenetration sp = smpl->selfPenetration(1.5f, maxPairs);
    smplpp::Tensor g(sp.pairEnergy.shape);
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    const smplpp::Tensor gv = smpl->selfPenetrationBackward(sp, g, 1.5f);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [f](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(const smplpp::Tensor * t : {&si.pairs, &si.count, &sp.pairs, &sp.count, &sp.pairEnergy, &gv}) put(*t);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
