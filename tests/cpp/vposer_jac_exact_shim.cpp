// VPoserDecoder::jacobian (and, compiled only, IkSolver::setExactArithmetic) through the header-only C++ shim; driven by
// tests/test_vposer_jac_exact_gpu.py, which restates these inputs and compares the printed values with the Python binding's.
// usage: vposer_jac_exact_shim <vposer.json>
#include <cstdio>

#include <smplpp/IkTask.h>
#include <smplpp/VPoser.h>

// (IkSolver::setExactArithmetic is compiled here under -Wall -Werror; its run is in tests/test_ik_exact_gpu.py)
static void (smplpp::IkSolver::*const set_exact)(bool) = &smplpp::IkSolver::setExactArithmetic;

int main(int argc, char ** argv)
{
  if(argc < 2 || !set_exact) return 1;
  try
  {
    smplpp::VPoserDecoder vposer;
    vposer->loadParamsFromJson(argv[1]);
    vposer->eval();
    const int64_t n = 3;
    smplpp::Tensor z({n, 32});
    for(int64_t i = 0; i < z.numel(); i++) z.data[(size_t)i] = (float)(i % 9 - 4) * 0.2f;
    smplpp::Tensor out;
    smplpp::Tensor jac = vposer->jacobian(z, &out);
    std::printf("JAC");
    for(float x : jac.toVector<float>()) std::printf(" %.9g", (double)x);
    std::printf("\nOUT");
    for(float x : out.toVector<float>()) std::printf(" %.9g", (double)x);
    std::printf("\n");
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
