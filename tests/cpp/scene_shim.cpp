// smplpp::Volume through the header-only C++ shim on a small grid; driven by tests/test_scene_gpu.py, which restates every output with
// tests/scene_oracle.py and compares bit for bit.
// usage: scene_shim <out.bin>
//   (out, float32: Gx, Gy, Gz as floats; value [n,K], gradient [n,K,3], valid [n,K] as floats; energy [n], point_energy [n,K], value [n,K],
//    valid [n,K] as floats; grad_points [n,K,3]; grad_points after a second, accumulating call; value [n,K] after set() of the negated grid)
#include <cstdio>

#include <smplpp/Scene.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t Gx = 5, Gy = 4, Gz = 3, n = 2, K = 6;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    auto put_flags = [&](const smplpp::Tensor & t) {
      smplpp::Tensor f = t.to(smplpp::kFloat32);
      put(f);
    };
    smplpp::Tensor values({Gz, Gy, Gx}), xf({3, 4});
    for(int64_t i = 0; i < Gx * Gy * Gz; i++) values.data[(size_t)i] = (float)((i * 7) % 13 - 6) * 0.0625f;
    xf.data = {1.0f, 0.25f, 0.0f, 0.125f, -0.25f, 1.0f, 0.5f, 0.0f, 0.0f, 0.125f, 0.75f, -0.0625f};
    smplpp::Volume vol(values, {-0.25f, 0.125f, -0.5f}, {0.25f, 0.5f, 0.375f}, xf);
    if(vol.Gx() != Gx || vol.Gy() != Gy || vol.Gz() != Gz) return 4;
    smplpp::Tensor dims({3});
    dims.data = {(float)vol.Gx(), (float)vol.Gy(), (float)vol.Gz()};
    put(dims);
    smplpp::Tensor points({n, K, 3}), wPen({K}), wCon({K}), ge({n}), gpe({n, K}), gv({n, K});
    for(int64_t i = 0; i < n * K; i++)
    {
      points.data[(size_t)(3 * i)] = -0.125f + 0.0625f * (float)(i % 7);
      points.data[(size_t)(3 * i + 1)] = 0.25f + 0.09375f * (float)(i % 5);
      points.data[(size_t)(3 * i + 2)] = -0.375f + 0.0625f * (float)(i % 4);
      gpe.data[(size_t)i] = 0.5f - 0.125f * (float)i;
      gv.data[(size_t)i] = -0.25f + 0.0625f * (float)i;
    }
    points.data[3 * 4] = 7.0f; // one point outside
    wPen.data = {1.0f, 0.5f, 0.0f, 2.0f, 1.0f, 0.0f};
    wCon.data = {0.0f, 0.25f, 0.0f, 1.0f, 0.5f, 0.75f};
    ge.data = {1.0f, -0.5f};
    const smplpp::Volume::Sample s = vol.sample(points);
    put(s.value), put(s.gradient), put_flags(s.valid);
    const smplpp::Volume::Term t = vol.term(points, wPen, wCon, 0.25f);
    put(t.energy), put(t.pointEnergy), put(t.value), put_flags(t.valid);
    smplpp::Tensor grad = vol.termBackward(points, ge, gpe, gv, wPen, wCon, 0.25f);
    put(grad);
    vol.termBackward(points, ge, smplpp::Tensor(), smplpp::Tensor(), wPen, wCon, 0.25f, &grad);
    put(grad);
    for(float & v : values.data) v = -v;
    vol.set(values);
    put(vol.sample(points).value);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
