// SMPL::maskDistanceTransform / silhouette / silhouetteBackward through the header-only C++ shim on the last launch's vertices; driven
// by tests/test_silhouette_gpu.py, which restates these inputs and compares every output with the Python binding's, bit for bit.
// usage: silhouette_shim <model.json> <out.bin>
//   (out: nearest, sqdist, vert_target, vert_sq, pix_source, pix_sq, grad_verts, all int64 or float32)
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
    const int64_t n = 1, H = 48, W = 64;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    smplpp::Tensor camera({16});
    const float cam[16] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.05f, -0.1f, 2.0f, 70.0f, -70.0f, 32.0f, 24.0f};
    for(int i = 0; i < 16; i++) camera.data[(size_t)i] = cam[i];
    const smplpp::SMPL::DepthRaster r = smpl->depthRaster(camera, H, W, 0.1f);
    // the target: the coverage moved three columns to the right and one row down
    smplpp::Tensor mask({n, H, W}, smplpp::kInt64);
    for(int64_t j = 1; j < H; j++)
      for(int64_t i = 3; i < W; i++) mask.idata[(size_t)(j * W + i)] = r.face.idata[(size_t)((j - 1) * W + i - 3)] >= 0;
    const smplpp::SMPL::MaskDistance t = smpl->maskDistanceTransform(mask);
    const smplpp::SMPL::Silhouette s = smpl->silhouette(camera, r.face, mask, 0.1f);
    smplpp::Tensor gv(s.vertSq.shape), gp(s.pixSq.shape);
    for(int64_t i = 0; i < gv.numel(); i++) gv.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    for(int64_t i = 0; i < gp.numel(); i++) gp.data[(size_t)i] = (float)(i % 7 - 3) * 0.5f;
    const smplpp::Tensor g = smpl->silhouetteBackward(camera, r.face, s, gv, gp, 0.1f);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [f](const smplpp::Tensor & x) {
      if(x.dtype == smplpp::kInt64) std::fwrite(x.idata.data(), sizeof(int64_t), x.idata.size(), f);
      else std::fwrite(x.data.data(), sizeof(float), x.data.size(), f);
    };
    for(const smplpp::Tensor * x : {&t.nearest, &t.sqdist, &s.vertTarget, &s.vertSq, &s.pixSource, &s.pixSq, &g}) put(*x);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
