// smplpp::BatchedLbfgs with groups of rows through the header-only C++ shim on a small diagonal quadratic; driven by
// tests/test_lbfgs_groups_gpu.py, which restates the energies and compares every output with the Python class's, bit for bit.
// usage: lbfgs_groups_shim <out.bin>
//   (out, float32: x [n,D] after each of CALLS calls; then status, iterations, evaluations (as floats) [3,P], f_best [P], step [P], the
//    running count, and x after best())
#include <cstdio>

#include <smplpp/Lbfgs.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const std::vector<int64_t> groups = {2, 1, 3};
    const int64_t n = 6, P = 3, D = 5, CALLS = 12;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    smplpp::BatchedLbfgs::Options o;
    o.tolGrad = 1e-3f;
    smplpp::BatchedLbfgs opt(groups, D, 3, o);
    if(opt.frameNum() != n || opt.problemNum() != P) return 4;
    smplpp::Tensor x({n, D}), f({P}), g({n, D});
    for(int64_t i = 0; i < n * D; i++) x.data[(size_t)i] = (float)(i % 7 - 3) * 0.25f;
    for(int64_t call = 0; call < CALLS; call++)
    {
      // f_p = sum over the rows i of problem p, then k, of (0.5 lam_k) (e_k e_k) in that order from +0, e_k = x_ik - c_k,
      // lam_k = 1 + k (1 + i), c_k = 0.125 (k - i); g_ik = lam_k e_k
      int64_t i = 0;
      for(int64_t p = 0; p < P; p++)
      {
        float s = 0.0f;
        for(int64_t r = 0; r < groups[(size_t)p]; r++, i++)
          for(int64_t k = 0; k < D; k++)
          {
            const float lam = 1.0f + (float)(k * (1 + i)), e = x.data[(size_t)(i * D + k)] - 0.125f * (float)(k - i);
            const float ee = e * e, h = 0.5f * lam, term = h * ee;
            s = s + term;
            g.data[(size_t)(i * D + k)] = lam * e;
          }
        f.data[(size_t)p] = s;
      }
      opt.step(x, f, g);
      put(x);
    }
    const smplpp::BatchedLbfgs::State s = opt.state();
    smplpp::Tensor ints({3, P});
    for(int64_t p = 0; p < P; p++)
      ints.data[(size_t)p] = (float)s.status[(size_t)p], ints.data[(size_t)(P + p)] = (float)s.iterations[(size_t)p],
      ints.data[(size_t)(2 * P + p)] = (float)s.evaluations[(size_t)p];
    put(ints), put(s.fBest), put(s.step);
    put(smplpp::Tensor({1}, (float)s.running));
    opt.best(x);
    put(x);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
