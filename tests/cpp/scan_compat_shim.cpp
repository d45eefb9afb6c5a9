// SMPL::pointMeshDistanceCompatible / meshPointDistanceCompatible and their backward passes through the header-only C++ shim on the
// last launch's vertices; driven by tests/test_scan_compat_gpu.py, which restates these inputs and compares every output with the
// Python binding's, bit for bit.
// usage: scan_compat_shim <model.json> <out.bin>
//   out: face int64, weights, closest, sqdist, grad_verts, grad_points (point -> mesh); index int64, sqdist, grad_verts, grad_points
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
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3}), points({n, K, 3}), normals({n, K, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    for(int64_t i = 0; i < points.numel(); i++) points.data[(size_t)i] = (float)(i % 17 - 8) * 0.03f;
    for(int64_t i = 0; i < normals.numel(); i++) normals.data[(size_t)i] = (float)(i % 13 - 6) * 0.25f;
    smpl->launch(beta, theta);
    const float cosMin = 0.25f, maxSqdist = 0.04f;
    const smplpp::SMPL::PointMeshDistance d = smpl->pointMeshDistanceCompatible(points, normals, cosMin, maxSqdist);
    smplpp::Tensor g(d.sqdist.shape);
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    smplpp::Tensor gp;
    const smplpp::Tensor gv = smpl->pointMeshDistanceCompatibleBackward(points, d.face, g, &gp);
    const smplpp::SMPL::MeshPointDistance e = smpl->meshPointDistanceCompatible(points, normals, cosMin, maxSqdist);
    smplpp::Tensor h(e.sqdist.shape);
    for(int64_t i = 0; i < h.numel(); i++) h.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    smplpp::Tensor hp;
    const smplpp::Tensor hv = smpl->meshPointDistanceBackward(points, e.index, h, &hp);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    std::fwrite(d.face.idata.data(), sizeof(int64_t), d.face.idata.size(), f);
    for(const smplpp::Tensor * t : {&d.weights, &d.closest, &d.sqdist, &gv, static_cast<const smplpp::Tensor *>(&gp)})
      std::fwrite(t->data.data(), sizeof(float), t->data.size(), f);
    std::fwrite(e.index.idata.data(), sizeof(int64_t), e.index.idata.size(), f);
    for(const smplpp::Tensor * t : {&e.sqdist, &hv, static_cast<const smplpp::Tensor *>(&hp)})
      std::fwrite(t->data.data(), sizeof(float), t->data.size(), f);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
