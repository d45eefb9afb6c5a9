// smplpp::Measure through the header-only C++ shim; driven by tests/test_measure_gpu.py, which restates these inputs and compares
// every output with the Python binding's, bit for bit.
// usage: measure_shim <model.json> <out.bin>
//   (out: float32 unless said.  Planes per frame, then one set for all frames: area, volume, section, crossings (int64); their
//    backward: verts, planes)
#include <cstdio>

#include <smplpp/Measure.h>

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  try
  {
    auto smpl = std::make_shared<smplpp::SMPL>();
    smpl->setDevice(smplpp::Device("CUDA", 0));
    smpl->setModelPath(argv[1]);
    smpl->init();
    const int64_t n = 3, R = 4, S = 4;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    const smplpp::Tensor verts = smpl->getVertex();
    const int64_t F = 128;
    // all faces; every third; none; the upper half in descending order
    std::vector<std::vector<int64_t>> regions(4);
    for(int64_t f = 0; f < F; f++) regions[0].push_back(f);
    for(int64_t f = 0; f < F; f += 3) regions[1].push_back(f);
    for(int64_t f = F - 1; f > F / 2; f--) regions[3].push_back(f);
    const smplpp::Measure ms(*smpl, regions, {0, 1, 0, 3});
    smplpp::Tensor planes({n, S, 4}), center({n, 3}), ga({n, R}), gv({n, R}), gs({n, S});
    for(int64_t i = 0; i < planes.numel(); i++) planes.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f + 0.125f;
    for(int64_t i = 0; i < center.numel(); i++) center.data[(size_t)i] = (float)(i % 4 - 1) * 0.125f;
    for(int64_t i = 0; i < ga.numel(); i++) ga.data[(size_t)i] = (float)(i % 5 - 2) * 0.5f, gv.data[(size_t)i] = (float)(i % 3 - 1) * 0.75f;
    for(int64_t i = 0; i < gs.numel(); i++) gs.data[(size_t)i] = (float)(i % 4 - 1) * 0.5f;
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(int64_t pf : {n, (int64_t)1})
    {
      const smplpp::Tensor pl = planes.index({smplpp::Slice(0, pf)});
      const smplpp::Measure::Result r = ms.evaluate(verts, pl, center);
      const smplpp::Measure::Gradients b = ms.evaluateBackward(verts, pl, center, ga, gv, gs);
      for(const smplpp::Tensor & t : {r.area, r.volume, r.section, r.crossings, b.verts, b.planes}) put(t);
    }
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
