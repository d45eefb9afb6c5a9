// SMPL::vertexOffsets / vertexOffsetsBackward / meshLaplacian through the header-only C++ shim on the last launch; driven by
// tests/test_vertex_offsets_gpu.py, which restates these inputs and compares every output with the Python binding's, bit for bit.
// usage: vertex_offsets_shim <model.json> <out.bin>
//   (out, float32: shared verts, shared rest, per-frame verts, per-frame grad, shared grad, shared grad added into ones,
//    Laplacian of the offsets, the same added into ones)
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
    const int64_t n = 3;
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    const int64_t V = smpl->getVertex().size(1);
    smplpp::Tensor one({1, V, 3}), each({n, V, 3}), g({n, V, 3});
    for(int64_t i = 0; i < one.numel(); i++) one.data[(size_t)i] = (float)(i % 9 - 4) * 0.004f;
    for(int64_t i = 0; i < each.numel(); i++) each.data[(size_t)i] = (float)(i % 13 - 6) * 0.003f;
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.25f;
    const smplpp::SMPL::VertexOffsets a = smpl->vertexOffsets(one), b = smpl->vertexOffsets(each);
    const smplpp::Tensor ge = smpl->vertexOffsetsBackward(g), gs = smpl->vertexOffsetsBackward(g, true);
    smplpp::Tensor acc({1, V, 3}, 1.0f);
    smpl->vertexOffsetsBackward(g, true, &acc);
    const smplpp::Tensor lap = smpl->meshLaplacian(each);
    smplpp::Tensor lacc(each.shape, 1.0f);
    smpl->meshLaplacian(each, &lacc);
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    for(const smplpp::Tensor & t : {a.verts, a.rest, b.verts, ge, gs, acc, lap, lacc}) std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
