// smplpp::BatchedLbfgs through the header-only C++ shim on a small diagonal quadratic; driven by tests/test_lbfgs_gpu.py, which
// restates the energies and compares every output with the Python class's, bit for bit.
// usage: lbfgs_shim <out.bin>
//   (out, float32: x [n,D] after each of CALLS calls; then status, iterations, evaluations (as floats), f_best, step, the running count,
//    and x after best())
#include <cstdio>

#include <smplpp/Lbfgs.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t n = 3, D = 5, CALLS = 12;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    smplpp::BatchedLbfgs::Options o;
    o.tolGrad = 1e-3f;
    smplpp::BatchedLbfgs opt(n, D, 3, o);
    smplpp::Tensor x({n, D}), f({n}), g({n, D});
    for(int64_t i = 0; i < n * D; i++) x.data[(size_t)i] = (float)(i % 7 - 3) * 0.25f;
    for(int64_t call = 0; call < CALLS; call++)
    {
      // f_i = sum_k (0.5 lam_k) (e_k e_k) in ascending k from +0, e_k = x_k - c_k, lam_k = 1 + k (1 + i), c_k = 0.125 (k - i); g_k = lam_k e_k
      for(int64_t i = 0; i < n; i++)
      {
        float s = 0.0f;
        for(int64_t k = 0; k < D; k++)
        {
          const float lam = 1.0f + (float)(k * (1 + i)), e = x.data[(size_t)(i * D + k)] - 0.125f * (float)(k - i);
          const float ee = e * e, h = 0.5f * lam, term = h * ee;
          s = s + term;
          g.data[(size_t)(i * D + k)] = lam * e;
        }
        f.data[(size_t)i] = s;
      }
      opt.step(x, f, g);
      put(x);
    }
    const smplpp::BatchedLbfgs::State s = opt.state();
    smplpp::Tensor ints({3, n});
    for(int64_t i = 0; i < n; i++)
      ints.data[(size_t)i] = (float)s.status[(size_t)i], ints.data[(size_t)(n + i)] = (float)s.iterations[(size_t)i],
      ints.data[(size_t)(2 * n + i)] = (float)s.evaluations[(size_t)i];
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
