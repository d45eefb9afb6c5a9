// smplpp::orientationTerm / orientationTermBackward and SMPL::axisAngleToRotmatBackward through the header-only C++ shim on small
// inputs; driven by tests/test_orientation_gpu.py, which restates them, calls the Python binding and compares bit for bit.
// usage: orientation_shim <out.bin>
//   (out, float32: C = 3 on [n,J,3,4] with offsets and a shared weight row: energy [n], sensor_energy [n,S], residual [n,S,3,3];
//    grad_frames [n,J,3,4], grad_offset [S,3,3], grad_target [n,S,3,3]; the three again after a second, accumulating call;
//    C = 1 on [n,J,3,3] with a shared target, no offset, rho = 0.5: energy [n], grad_frames [n,J,3,3], grad_offset [S,3,1],
//    grad_target [1,S,3,1]; grad_aa [n,J,3] of the Rodrigues VJP, and again after an accumulating call)
#include <cstdio>

#include <smplpp/Orientation.h>

int main(int argc, char ** argv)
{
  if(argc < 2) return 1;
  try
  {
    const int64_t n = 3, J = 5, S = 4;
    std::FILE * out = std::fopen(argv[1], "wb");
    if(!out) return 2;
    auto put = [&](const smplpp::Tensor & t) { std::fwrite(t.data.data(), sizeof(float), t.data.size(), out); };
    smplpp::Tensor world({n, J, 3, 4}), rot({n, J, 3, 3}), joint({S}, smplpp::kInt64), offset({S, 3, 3}), target({n, S, 3, 3}), axis({1, S, 3, 1}),
        weight({1, S}), ge({n}), gse({n, S}), gr({n, S, 3, 3}), aa({n, J, 3});
    for(int64_t i = 0; i < world.numel(); i++) world.data[(size_t)i] = (float)((i * 7) % 23 - 11) * 0.0625f;
    for(int64_t i = 0; i < rot.numel(); i++) rot.data[(size_t)i] = (float)((i * 5) % 19 - 9) * 0.125f;
    for(int64_t i = 0; i < offset.numel(); i++) offset.data[(size_t)i] = (float)((i * 3) % 11 - 5) * 0.25f;
    for(int64_t i = 0; i < target.numel(); i++) target.data[(size_t)i] = (float)((i * 11) % 17 - 8) * 0.125f;
    for(int64_t i = 0; i < axis.numel(); i++) axis.data[(size_t)i] = (float)(i % 5 - 2) * 0.5f;
    for(int64_t i = 0; i < gse.numel(); i++) gse.data[(size_t)i] = (float)(i % 7 - 3) * 0.25f;
    for(int64_t i = 0; i < gr.numel(); i++) gr.data[(size_t)i] = -0.25f + 0.0625f * (float)(i % 9);
    for(int64_t i = 0; i < aa.numel(); i++) aa.data[(size_t)i] = (float)(i % 11 - 5) * 0.05f;
    joint.idata = {4, 1, 1, 0};
    weight.data = {1.0f, 0.5f, 2.0f, 0.0f};
    ge.data = {1.0f, -0.5f, 0.25f};
    const smplpp::OrientationTerm a = smplpp::orientationTerm(world, joint, target, offset, weight);
    put(a.energy), put(a.sensorEnergy), put(a.residual);
    smplpp::OrientationGradients g = smplpp::orientationTermBackward(world, joint, target, ge, gse, gr, offset, weight);
    put(g.frames), put(g.offset), put(g.target);
    smplpp::orientationTermBackward(world, joint, target, ge, smplpp::Tensor(), smplpp::Tensor(), offset, weight, 0.0f, 3, &g);
    put(g.frames), put(g.offset), put(g.target);
    const smplpp::OrientationTerm b = smplpp::orientationTerm(rot, joint, axis, smplpp::Tensor(), smplpp::Tensor(), 0.5f, 1);
    put(b.energy);
    const smplpp::OrientationGradients h =
        smplpp::orientationTermBackward(rot, joint, axis, ge, smplpp::Tensor(), smplpp::Tensor(), smplpp::Tensor(), smplpp::Tensor(), 0.5f, 1);
    put(h.frames), put(h.offset), put(h.target);
    smplpp::SMPL smpl;
    smpl.setDevice(smplpp::Device("CUDA", 0));
    smplpp::Tensor ga = smpl.axisAngleToRotmatBackward(aa, rot);
    put(ga);
    smpl.axisAngleToRotmatBackward(aa, rot, &ga);
    put(ga);
    std::fclose(out);
  }
  catch(const std::exception & e)
  {
    std::printf("ERROR %s\n", e.what());
    return 3;
  }
  return 0;
}
