// smplpp::imageSample / imageTerm / imageTermBackward through the header-only C++ shim on a small image; driven by
// tests/test_image_gpu.py, which restates every output with tests/image_oracle.py and compares bit for bit.
// usage: image_shim <out.bin>
//   (out, float32: value [n,K,C], gradient [n,K,C,2], valid [n,K] as floats; energy [n], point_energy [n,K], value [n,K,C], valid [n,K] as
//    floats; grad_uv [n,K,2], grad_image [B,H,W,C]; both after a second, accumulating call; then with `channel`: value [n,K,1], energy [n],
//    grad_image [B,H,W,C])
#include <cstdio>

#include <smplpp/Image.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t H = 4, W = 5, C = 3, n = 2, K = 6;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    auto put_flags = [&](const smplpp::Tensor & t) {
      smplpp::Tensor f = t.to(smplpp::kFloat32);
      put(f);
    };
    smplpp::Tensor image({1, H, W, C}), uv({n, K, 2}), target({n, K, C}), weight({1, K}), ge({n}), gpe({n, K}), gv({n, K, C});
    for(int64_t i = 0; i < H * W * C; i++) image.data[(size_t)i] = (float)((i * 7) % 13 - 6) * 0.0625f;
    for(int64_t i = 0; i < n * K; i++)
    {
      uv.data[(size_t)(2 * i)] = 0.75f + 0.3125f * (float)(i % 11);
      uv.data[(size_t)(2 * i + 1)] = 0.625f + 0.4375f * (float)(i % 7);
      gpe.data[(size_t)i] = 0.5f - 0.125f * (float)i;
    }
    uv.data[2 * 4] = 7.0f; // one point outside
    for(int64_t i = 0; i < n * K * C; i++)
    {
      target.data[(size_t)i] = 0.125f * (float)(i % 5) - 0.25f;
      gv.data[(size_t)i] = -0.25f + 0.0625f * (float)(i % 9);
    }
    weight.data = {1.0f, 0.5f, 0.0f, 2.0f, 1.0f, 0.75f};
    ge.data = {1.0f, -0.5f};
    const smplpp::ImageSample s = smplpp::imageSample(uv, image);
    put(s.value), put(s.gradient), put_flags(s.valid);
    const smplpp::ImageTerm t = smplpp::imageTerm(uv, image, target, weight, 0.25f);
    put(t.energy), put(t.pointEnergy), put(t.value), put_flags(t.valid);
    smplpp::ImageGradients g = smplpp::imageTermBackward(uv, image, ge, gpe, gv, target, weight, 0.25f);
    put(g.uv), put(g.image);
    smplpp::imageTermBackward(uv, image, ge, smplpp::Tensor(), smplpp::Tensor(), target, weight, 0.25f, smplpp::Tensor(), &g);
    put(g.uv), put(g.image);
    const smplpp::IndexTensor channel({2, 0, 1, 1, 2, 0});
    put(smplpp::imageSample(uv, image, channel).value);
    put(smplpp::imageTerm(uv, image, smplpp::Tensor(), weight, 0.0f, channel).energy);
    put(smplpp::imageTermBackward(uv, image, ge, smplpp::Tensor(), smplpp::Tensor(), smplpp::Tensor(), weight, 0.0f, channel).image);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
