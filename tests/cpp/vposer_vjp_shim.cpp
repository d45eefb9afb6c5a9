// VPoserDecoder::launchBackward through the header-only C++ shim; driven by tests/test_vposer_vjp_gpu.py, which restates these inputs
// and compares the printed gradient with the Python binding's.
// usage: vposer_vjp_shim <vposer.json>
#include <cstdio>

#include <smplpp/VPoser.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    smplpp::VPoserDecoder vposer;
    vposer->loadParamsFromJson(argv[1]);
    vposer->eval();
    const int64_t n = 3;
    smplpp::Tensor z({n, 32}), go({n, 21, 3});
    for(int64_t i = 0; i < z.numel(); i++) z.data[(size_t)i] = (float)(i % 9 - 4) * 0.2f;
    for(int64_t i = 0; i < go.numel(); i++) go.data[(size_t)i] = (float)(i % 7 - 3) * 0.1f;
    smplpp::Tensor gz = vposer->launchBackward(z, go);
    std::printf("GRAD_Z");
    for(float x : gz.toVector<float>()) std::printf(" %.9g", (double)x);
    std::printf("\n");
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
