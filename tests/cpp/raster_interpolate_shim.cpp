// SMPL::rasterInterpolate / rasterInterpolateBackward through the header-only C++ shim on the last launch's vertices; driven by
// tests/test_raster_interpolate_gpu.py, which restates these inputs and compares every output with the Python binding's, bit for
// bit.
// usage: raster_interpolate_shim <model.json> <out.bin>
//   (out: face, image, grad_attr, grad_verts, then grad_attr alone added into ones; int64 or float32)
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
    const int64_t n = 2, H = 48, W = 64, C = 3;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    smplpp::Tensor camera({16});
    const float cam[16] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.05f, -0.1f, 2.0f, 70.0f, -70.0f, 32.0f, 24.0f};
    for(int i = 0; i < 16; i++) camera.data[(size_t)i] = cam[i];
    const smplpp::SMPL::DepthRaster r = smpl->depthRaster(camera, H, W, 0.1f);
    smplpp::Tensor attr({n, smpl->getVertex().size(1), C});
    for(int64_t i = 0; i < attr.numel(); i++) attr.data[(size_t)i] = (float)(i % 13 - 6) * 0.125f;
    const smplpp::Tensor image = smpl->rasterInterpolate(attr, r.face, r.bary);
    smplpp::Tensor g(image.shape);
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    const smplpp::SMPL::RasterInterpolateGrad both = smpl->rasterInterpolateBackward(attr, camera, r.face, r.bary, g, 0.1f);
    smplpp::SMPL::RasterInterpolateGrad acc;
    acc.attr = smplpp::Tensor(attr.shape, 1.0f);
    smpl->rasterInterpolateBackward(attr, camera, r.face, r.bary, g, 0.1f, true, false, &acc);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [f](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(const smplpp::Tensor & t : {r.face, image, both.attr, both.verts, acc.attr}) put(t);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
