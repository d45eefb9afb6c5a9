// smplpp::SequenceLayout through the header-only C++ shim on a small buffer; driven by tests/test_sequence_gpu.py, which restates every
// output with tests/sequence_oracle.py and compares bit for bit.
// usage: sequence_shim <out.bin>
//   (out, float32: frame_start [P+1] as floats; frames [F,6]; shared [F,3]; then per order 1, 2: frame_energy [F], point_energy [F,2],
//    grad_x [F,2,3]; merged rows [n,8]; the rows after a second, accumulating merge; problem values [P]; the values after an accumulating sum)
#include <cstdio>

#include <smplpp/Sequence.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const std::vector<int64_t> groups = {4, 3};
    const int64_t n = 7, D = 8, K = 2, C = 3;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    smplpp::SequenceLayout seq(groups, 1);
    const int64_t F = seq.frameNum(), P = seq.problemNum();
    if(F != 5 || P != 2 || seq.rowNum() != n || seq.sharedRows() != 1) return 4;
    smplpp::Tensor fs({P + 1});
    for(int64_t p = 0; p <= P; p++) fs.data[(size_t)p] = (float)seq.frameStart()[(size_t)p];
    put(fs);
    smplpp::Tensor rows({n, D});
    for(int64_t i = 0; i < n * D; i++) rows.data[(size_t)i] = (float)((i * 7) % 11 - 5) * 0.125f + (float)(i / D) * 0.0625f;
    const smplpp::SequenceLayout::Parts parts = seq.split(rows, 2, K * C, 3);
    put(parts.frames), put(parts.shared);
    smplpp::Tensor x = parts.frames.view({F, K, C}), weight({K}), gfe({F}), gpe({F, K});
    weight.data = {0.5f, 2.0f};
    for(int64_t f = 0; f < F; f++)
    {
      gfe.data[(size_t)f] = 1.0f + 0.25f * (float)f;
      for(int64_t k = 0; k < K; k++) gpe.data[(size_t)(f * K + k)] = 0.5f - 0.125f * (float)(f + k);
    }
    smplpp::Tensor grad;
    for(int order = 1; order <= 2; order++)
    {
      const smplpp::SequenceLayout::Energies e = seq.smoothness(x, order, weight, order == 1 ? 0.0f : 0.75f);
      put(e.frameEnergy), put(e.pointEnergy);
      grad = seq.smoothnessBackward(x, gfe, gpe, order, weight, order == 1 ? 0.0f : 0.75f);
      put(grad);
    }
    smplpp::Tensor merged = seq.merge(grad.view({F, K * C}), 2, parts.shared, D);
    put(merged);
    seq.merge(grad.view({F, K * C}), 2, parts.shared, D, &merged);
    put(merged);
    smplpp::Tensor pv = seq.sum(gfe, 0.5f);
    put(pv);
    seq.sum(gfe, 3.0f, &pv);
    put(pv);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
