// smplpp::SelfContact and SMPL::meshGeodesic through the header-only C++ shim; driven by tests/test_self_contact_gpu.py, which restates
// these inputs and compares every output with the Python binding's, bit for bit.
// usage: self_contact_shim <model.json> <out.bin>
//   (out: float32 unless said.  geodesics [n,3,V] from the sets {0}, {V/2, V-1}, {} capped at 1.5; far_pairs, words per row (int64);
//    the mask [V,W] (int64); without normals: index (int64), sqdist; with the rest normals and a cap: index (int64), sqdist; the
//    backward of the first search: verts, and the same added into a tensor of ones)
#include <cstdio>

#include <smplpp/Contact.h>

int main(int argc, char ** argv)
{
  if(argc < 3) return 1;
  try
  {
    auto smpl = std::make_shared<smplpp::SMPL>();
    smpl->setDevice(smplpp::Device("CUDA", 0));
    smpl->setModelPath(argv[1]);
    smpl->init();
    const int64_t n = 2, V = smpl->vertexNum();
    smplpp::Tensor beta({n, 10}), theta({n, 25, 3});
    for(int64_t i = 0; i < beta.numel(); i++) beta.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    for(int64_t i = 0; i < theta.numel(); i++) theta.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    smpl->launch(beta, theta);
    const smplpp::Tensor verts = smpl->getVertex(), rest = smpl->getRestShape();
    std::FILE * f = std::fopen(argv[2], "wb");
    if(!f) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      if(t.dtype == smplpp::kInt64) std::fwrite(t.idata.data(), sizeof(int64_t), t.idata.size(), f);
      else std::fwrite(t.data.data(), sizeof(float), t.data.size(), f);
    };
    put(smpl->meshGeodesic({{0}, {V / 2, V - 1}, {}}, 1.5f));
    const smplpp::SelfContact sc(*smpl, rest, 0.6f);
    const int64_t info[2] = {sc.farPairs(), sc.wordsPerRow()};
    std::fwrite(info, sizeof(int64_t), 2, f);
    put(sc.mask());
    const smplpp::SelfContact::Partners a = sc.search(verts);
    put(a.index), put(a.sqdist);
    // any normals do: the rest shape's coordinates, per frame
    const smplpp::SelfContact::Partners b = sc.search(verts, rest, 0.1f, 1.0f);
    put(b.index), put(b.sqdist);
    smplpp::Tensor g({n, V}), ones({n, V, 3});
    for(int64_t i = 0; i < g.numel(); i++) g.data[(size_t)i] = (float)(i % 5 - 2) * 0.5f;
    for(int64_t i = 0; i < ones.numel(); i++) ones.data[(size_t)i] = 1.0f;
    put(sc.searchBackward(verts, a.index, g));
    put(sc.searchBackward(verts, a.index, g, &ones));
    std::fclose(f);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
