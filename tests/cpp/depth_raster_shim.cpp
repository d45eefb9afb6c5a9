// SMPL::depthRaster / depthRasterBackward through the header-only C++ shim on the last launch's vertices; driven by
// tests/test_depth_raster_gpu.py, which restates these inputs and compares every output with the Python binding's, bit for bit.
// usage: depth_raster_shim <model.json> <out.bin>
//   (out: face, depth, bary, visible, culled, grad_verts, all int64 or float32)
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
    const int64_t n = 2, H = 48, W = 64;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    // identity rotation, the body 2 m in front of the camera, y flipped by the sign of fy
    smplpp::Tensor camera({16});
    const float cam[16] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.05f, -0.1f, 2.0f, 70.0f, -70.0f, 32.0f, 24.0f};
    for(int i = 0; i < 16; i++) camera.data[(size_t)i] = cam[i];
    const smplpp::SMPL::DepthRaster r = smpl->depthRaster(camera, H, W, 0.1f);
    smplpp::Tensor g(r.depth.shape);
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    const smplpp::Tensor gv = smpl->depthRasterBackward(camera, r.face, g);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [f](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(const smplpp::Tensor * t : {&r.face, &r.depth, &r.bary, &r.visible, &r.culled, &gv}) put(*t);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
