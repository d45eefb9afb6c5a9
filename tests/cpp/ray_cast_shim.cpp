// SMPL::rayCast / rayCastBackward through the header-only C++ shim; driven by tests/test_ray_cast_gpu.py, which restates these inputs
// and compares every output with the Python binding's, bit for bit.
// usage: ray_cast_shim <model.json> <out.bin>
//   (out: float32 unless said.  Shared rays, both facings: face (int64), t, bary, hits (int64); their backward: verts, origin, dir.
//    Per-frame rays, front faces up to t = 1.25: face (int64), t, bary, hits (int64); their backward: verts, origin, dir)
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
    const int64_t n = 3, K = 70;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(int64_t rf : {(int64_t)1, n})
    {
      // origins on a box of side 6 about the body, aimed at a lattice of points inside it
      smplpp::Tensor origin({rf, K, 3}), dir({rf, K, 3}), g({n, K});
      for(int64_t i = 0; i < rf * K; i++)
      {
        const float o[3] = {(float)(i % 5 - 2) * 1.5f, (float)(i % 3 - 1) * 3.0f, (float)(i % 7 - 3)};
        const float p[3] = {(float)(i % 4 - 2) * 0.125f, (float)(i % 9 - 4) * 0.0625f, (float)(i % 6 - 3) * 0.125f};
        for(int x = 0; x < 3; x++) origin.data[(size_t)i * 3 + x] = o[x], dir.data[(size_t)i * 3 + x] = p[x] - o[x];
      }
      for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
      const smplpp::SMPL::RayCast r = rf == 1 ? smpl->rayCast(origin, dir) : smpl->rayCast(origin, dir, 0.0f, 1.25f, 1);
      const smplpp::SMPL::RayCastGrad b = smpl->rayCastBackward(origin, dir, r.face, g);
      for(const smplpp::Tensor & t : {r.face, r.t, r.bary, r.hits, b.verts, b.origin, b.dir}) put(t);
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
