// smplpp::cloudKnn / cloudNormals / cloudFarthestPoints through the header-only C++ shim on two small frames; driven by
// tests/test_cloud_gpu.py, which makes the same calls through the Python package and compares bit for bit.
// usage: cloud_shim <out.bin>
//   (out, every tensor as float32: kNN of separate queries under a cap: index [n,Q,k], sqdist [n,Q,k], count [n,Q]; the cloud's kNN on
//    itself: the same three with Q = K; the normals from those lists towards a viewpoint: normal [n,K,3], curvature [n,K], status [n,K];
//    farthest points from the starts (3, 0): index [n,M], radius_sq [n,M], min_sqdist [n,K])
#include <cstdio>

#include <smplpp/Cloud.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t n = 2, K = 40, Q = 7, M = 12;
    const int k = 5;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) {
      const smplpp::Tensor f = t.to(smplpp::kFloat32);
      std::fwrite(f.data.data(), sizeof(float), f.data.size(), out);
    };
    smplpp::Tensor p({n, K, 3}), q({n, Q, 3}), view({3}), start({n}, smplpp::kInt64);
    for(int64_t j = 0; j < n * K * 3; j++) p.data[(size_t)j] = (float)((j * 7) % 23 - 11) * 0.0625f + (float)((j * 3) % 5) * 0.03125f;
    for(int64_t j = 0; j < n * Q * 3; j++) q.data[(size_t)j] = (float)((j * 5) % 19 - 9) * 0.125f;
    view.data = {0.5f, -0.25f, 4.0f};
    start.idata = {3, 0};
    const smplpp::CloudNeighbours a = smplpp::cloudKnn(p, k, q, 0.5f);
    put(a.index), put(a.sqdist), put(a.count);
    const smplpp::CloudNeighbours b = smplpp::cloudKnn(p, k);
    put(b.index), put(b.sqdist), put(b.count);
    const smplpp::CloudNormals c = smplpp::cloudNormals(p, b.index, view, 0.01f);
    put(c.normal), put(c.curvature), put(c.status);
    const smplpp::CloudSample d = smplpp::cloudFarthestPoints(p, M, start);
    put(d.index), put(d.radiusSq), put(d.minSqdist);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
