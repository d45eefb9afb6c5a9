// smplpp::alignPoints / alignPointsBackward through the header-only C++ shim on two small frames; driven by tests/test_align_gpu.py,
// which restates every output with tests/align_oracle.py and compares bit for bit.
// usage: align_shim <out.bin>
//   (out, float32: similarity with weights: transform [n,13], aligned [n,K,3], energy [n], point_error [n,K], gap [n], status [n] as
//    floats; rigid onto the first frame's target, no weights: transform [n,13], energy [n]; grad_source, grad_target [n,K,3] of the first;
//    both after a second, accumulating call)
#include <cstdio>

#include <smplpp/Align.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t n = 2, K = 7;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    smplpp::Tensor x({n, K, 3}), y({n, K, 3}), y0({1, K, 3}), w({1, K}), gtr({n, 13}), gal({n, K, 3}), ge({n});
    for(int64_t j = 0; j < n * K * 3; j++)
    {
      x.data[(size_t)j] = (float)((j * 7) % 23 - 11) * 0.0625f;
      y.data[(size_t)j] = (float)((j * 5) % 19 - 9) * 0.125f;
      gal.data[(size_t)j] = -0.25f + 0.0625f * (float)(j % 9);
    }
    for(int64_t j = 0; j < K * 3; j++) y0.data[(size_t)j] = y.data[(size_t)j];
    for(int64_t m = 0; m < n * 13; m++) gtr.data[(size_t)m] = 0.25f - 0.0625f * (float)(m % 7);
    w.data = {1.0f, 0.5f, 0.0f, 2.0f, 1.0f, 0.75f, 1.5f};
    ge.data = {1.0f, -0.5f};
    const smplpp::Alignment a = smplpp::alignPoints(x, y, w, true);
    put(a.transform), put(a.aligned), put(a.energy), put(a.pointError), put(a.gap), put(a.status.to(smplpp::kFloat32));
    const smplpp::Alignment b = smplpp::alignPoints(x, y0);
    put(b.transform), put(b.energy);
    smplpp::AlignGradients g = smplpp::alignPointsBackward(x, y, gtr, gal, ge, w, true);
    put(g.source), put(g.target);
    smplpp::alignPointsBackward(x, y, smplpp::Tensor(), smplpp::Tensor(), ge, w, true, 1e-3f, &g);
    put(g.source), put(g.target);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
