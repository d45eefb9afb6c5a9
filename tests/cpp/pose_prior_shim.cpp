// smplpp::PosePrior (evaluate / evaluateBackward) through the header-only C++ shim; driven by tests/test_pose_prior_gpu.py, which
// restates these inputs and compares every output with the Python binding's, bit for bit.
// usage: pose_prior_shim <out.bin>
//   (out, float32: energy, component, residual, limit energy, grad_pose; then on theta [n,25,3]: energy, limit energy, grad_theta,
//    grad_theta added into ones)
#include <cstdio>

#include <smplpp/PosePrior.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t n = 5;
    std::FILE * f = std::fopen(argv[1], "wb");
    if(!f) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      const smplpp::Tensor x = t.dtype == smplpp::kFloat32 ? t : t.to(smplpp::kFloat32);
      std::fwrite(x.data.data(), sizeof(float), x.data.size(), f);
    };
    for(const int64_t D : {int64_t(7), int64_t(69)})
    {
      const int64_t M = 3;
      std::vector<float> mean((size_t)(M * D)), mat((size_t)(M * D * D)), offset((size_t)M), lo((size_t)D), hi((size_t)D), w((size_t)D);
      for(size_t i = 0; i < mean.size(); i++) mean[i] = (float)((int)(i % 13) - 6) * 0.03125f;
      for(size_t i = 0; i < mat.size(); i++) mat[i] = (float)((int)(i % 17) - 8) * 0.0625f + (i % (size_t)(D + 1) == 0 ? 2.0f : 0.0f);
      for(size_t i = 0; i < offset.size(); i++) offset[i] = (float)i * 0.5f;
      for(int64_t k = 0; k < D; k++) lo[(size_t)k] = -0.125f, hi[(size_t)k] = 0.0625f * (float)(k % 3), w[(size_t)k] = 0.25f * (float)(k % 4);
      const smplpp::PosePrior prior(M, D, mean, mat, offset, lo, hi, w);
      smplpp::Tensor gradEnergy({n}), gradResidual({n, D}), gradLimit({n});
      for(int64_t i = 0; i < n; i++) gradEnergy.data[(size_t)i] = (float)(i % 3) * 0.5f, gradLimit.data[(size_t)i] = (float)(i % 2 + 1) * 0.25f;
      for(int64_t i = 0; i < n * D; i++) gradResidual.data[(size_t)i] = (float)(i % 5 - 2) * 0.125f;
      if(D == 7)
      {
        smplpp::Tensor pose({n, D});
        for(int64_t i = 0; i < pose.numel(); i++) pose.data[(size_t)i] = (float)(i % 11 - 5) * 0.0625f;
        const smplpp::PosePrior::Terms t = prior.evaluate(pose);
        const smplpp::Tensor g = prior.evaluateBackward(pose, gradEnergy, gradResidual, gradLimit, t.component);
        put(t.energy), put(t.component), put(t.residual), put(t.limitEnergy), put(g);
      }
      else
      {
        smplpp::Tensor theta({n, 25, 3});
        for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.0625f;
        const smplpp::PosePrior::Terms t = prior.evaluate(theta);
        const smplpp::Tensor g = prior.evaluateBackward(theta, gradEnergy, smplpp::Tensor(), gradLimit);
        smplpp::Tensor acc({n, 25, 3}, 1.0f);
        prior.evaluateBackward(theta, gradEnergy, smplpp::Tensor(), gradLimit, smplpp::Tensor(), &acc);
        put(t.energy), put(t.limitEnergy), put(g), put(acc);
      }
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
