// SMPL::pointMeshWinding / pointMeshSignedDistance / pointMeshSignedDistanceBackward through the header-only C++ shim on the last
// launch's vertices; driven by tests/test_signed_distance_gpu.py, which restates these inputs and compares every output with the
// Python binding's, bit for bit.
// usage: signed_distance_shim <model.json> <out.bin>
//   (out: winding, inside int64 | face int64, weights, closest, winding, inside int64, signed_sqdist | grad_verts, grad_points)
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
    const int64_t n = 2, K = 24;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), points({n, K, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < points.numel(); i++) points.data[(size_t)i] = (float)(i % 17 - 8) * 0.03f;
    smpl->launch(beta, theta);
    const smplpp::SMPL::PointMeshWinding w = smpl->pointMeshWinding(points);
    const smplpp::SMPL::PointMeshSignedDistance d = smpl->pointMeshSignedDistance(points);
    smplpp::Tensor g(d.signedSqdist.shape);
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    smplpp::Tensor gradPoints;
    const smplpp::Tensor gv = smpl->pointMeshSignedDistanceBackward(points, d.face, d.inside, g, &gradPoints);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [f](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(const smplpp::Tensor * t : {&w.winding, &w.inside, &d.face, &d.weights, &d.closest, &d.winding, &d.inside, &d.signedSqdist, &gv,
                                    static_cast<const smplpp::Tensor *>(&gradPoints)})
      put(*t);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
