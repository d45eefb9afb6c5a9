// SMPL::skinPoints / unskinPoints / skinPointsBackward / unskinPointsBackward through the header-only C++ shim; driven by
// tests/test_skin_points_gpu.py, which restates these inputs and compares every output with the Python binding's, bit for bit.
// usage: skin_points_shim <model.json> <out.bin>
//   (out: float32 unless said.  A shared cloud under a face binding: skin out, blend, valid (int64); its backward: points, world,
//    joints.  The posed points unskinned under per-frame dense weights: out, blend, valid (int64); its backward: points, world, joints,
//    weights)
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
    const int64_t n = 3, K = 70, F = smpl->faceNum();
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    const smplpp::SMPL::Skeleton sk = smpl->skeleton(beta, theta);
    smplpp::Tensor cloud({1, K, 3}), g({n, K, 3});
    for(int64_t i = 0; i < cloud.numel(); i++) cloud.data[(size_t)i] = (float)(i % 9 - 4) * 0.05f;
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    smplpp::SMPL::PointBinding byFace, byWeights;
    byFace.face = smplpp::Tensor({1, K}, smplpp::kInt64);
    byFace.bary = smplpp::Tensor({1, K, 3});
    for(int64_t k = 0; k < K; k++)
    {
      const float a = (float)(k % 5 + 1), b = (float)(k % 3 + 1), c = (float)(k % 7 + 1), sum = (a + b) + c;
      byFace.face.idata[(size_t)k] = (k * 5) % F;
      byFace.bary.data[(size_t)k * 3] = a / sum, byFace.bary.data[(size_t)k * 3 + 1] = b / sum, byFace.bary.data[(size_t)k * 3 + 2] = c / sum;
    }
    byWeights.weights = smplpp::Tensor({n, K, 24});
    for(int64_t i = 0; i < byWeights.weights.numel(); i++) byWeights.weights.data[(size_t)i] = (float)((i * 7) % 5) * 0.125f;
    const smplpp::SMPL::BoundPoints posed = smpl->skinPoints(sk.world, sk.joints, cloud, byFace);
    const smplpp::SMPL::BoundPointsGrad gs = smpl->skinPointsBackward(sk.world, sk.joints, cloud, byFace, g);
    const smplpp::SMPL::BoundPoints back = smpl->unskinPoints(sk.world, sk.joints, posed.out, byWeights);
    const smplpp::SMPL::BoundPointsGrad gu = smpl->unskinPointsBackward(sk.world, sk.joints, posed.out, byWeights, g);
    if(!gs.weights.data.empty()) return 4; // (a face binding has no gradient to weights)
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    for(const smplpp::Tensor & t : {posed.out, posed.blend, posed.valid, gs.points, gs.world, gs.joints, back.out, back.blend, back.valid, gu.points,
                                    gu.world, gu.joints, gu.weights})
      put(t);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
