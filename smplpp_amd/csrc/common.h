// Internal definitions shared by the translation units of libsmplpp_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "layout.h"

namespace smplpp_hip
{
// column of vertex v, coordinate x, in the B operand (layout.h, VG)
__host__ __device__ inline int64_t bcol(int64_t v, int x)
{
  return (v / VG) * (3 * VG) + x * VG + (v % VG);
}

// x = p0 + p1 + p2 exactly (round-to-nearest-even pieces; finite inputs)
__host__ __device__ inline uint16_t bf16_rn_bits(float x)
{
  uint32_t u;
  memcpy(&u, &x, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float bf16_bits_to_float(uint16_t b)
{
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
__host__ __device__ inline void split_bf16x3(float x, uint16_t & p0, uint16_t & p1, uint16_t & p2)
{
  p0 = bf16_rn_bits(x);
  const float r1 = x - bf16_bits_to_float(p0);
  p1 = bf16_rn_bits(r1);
  const float r2 = r1 - bf16_bits_to_float(p1);
  p2 = bf16_rn_bits(r2);
}

// the two fp16 pieces of a value of the fp16x2 form (layout.h, HB_*)
__host__ __device__ inline void split_f16x2(float xs, _Float16 & hi, _Float16 & lo) // xs: already scaled
{
  hi = (_Float16)xs;
  lo = (_Float16)(xs - (float)hi);
}

void set_error(const std::string & msg);
int fail(int code, const std::string & msg);
int hip_fail(hipError_t e, const char * what, const char * file, int line);

#define HIP_TRY(expr)                                                              \
  do                                                                               \
  {                                                                                \
    hipError_t _e = (expr);                                                        \
    if(_e != hipSuccess) return smplpp_hip::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while(0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is an opt-in per DEVICE: one flag per (call site, device)
struct PerDeviceOnce
{
  bool done[64] = {};
};
inline hipError_t lds_opt_in(PerDeviceOnce & o, int device, const void * fn, int bytes)
{
  if(o.done[device & 63]) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if(e == hipSuccess) o.done[device & 63] = true;
  else if(getenv("SMPLPP_DEBUG_LDS"))
  {
    hipFuncAttributes a;
    hipError_t e2 = hipFuncGetAttributes(&a, fn);
    fprintf(stderr, "[smplpp dbg] lds_opt_in(%d bytes) failed: %s; attributes (%s): static %zu, max dynamic %d, regs %d, max threads %d\n", bytes,
            hipGetErrorString(e), hipGetErrorString(e2), a.sharedSizeBytes, a.maxDynamicSharedSizeBytes, a.numRegs, a.maxThreadsPerBlock);
  }
  return e;
}
inline int device_cus(int device) // compute units of a device (cached per device)
{
  static int cus[64] = {};
  int & c = cus[device & 63];
  if(!c)
  {
    hipDeviceProp_t prop;
    c = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return c;
}

// Owners of device memory: DevPtr for an exact-size array, DevBuf for a buffer grown on demand.
struct HipFree
{
  void operator()(void * p) const { (void)hipFree(p); }
};
template<class T>
using DevPtr = std::unique_ptr<T, HipFree>;
// count elements of T (at least one: hipMalloc of 0 bytes gives no pointer)
template<class T>
hipError_t dev_alloc(DevPtr<T> & p, size_t count)
{
  T * raw = nullptr;
  hipError_t e = hipMalloc((void **)&raw, sizeof(T) * (count ? count : 1));
  p.reset(raw);
  return e;
}

// Growable device buffer: a reserve that grows it frees the old allocation first and keeps 25 % slack
struct DevBuf
{
  DevPtr<void> p;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf && o) noexcept : p(std::move(o.p)), cap(std::exchange(o.cap, 0)) {}
  DevBuf & operator=(DevBuf && o) noexcept
  {
    p = std::move(o.p);
    cap = std::exchange(o.cap, 0);
    return *this;
  }
  hipError_t reserve(size_t bytes)
  {
    if(bytes <= cap) return hipSuccess;
    p.reset();
    cap = 0;
    size_t want = bytes + bytes / 4;
    void * raw = nullptr;
    hipError_t e = hipMalloc(&raw, want);
    p.reset(raw);
    if(e == hipSuccess) cap = want;
    return e;
  }
  template<class T>
  T * as() const
  {
    return static_cast<T *>(p.get());
  }
};

// The staging slots of a handle's host-space calls (staging.h): slot k holds the k-th staged argument of whichever call is running
constexpr int ARENA_SLOTS = 11; // the widest call stages 11 arguments: smplpp_orientation_term_vjp (smplpp_image_term_vjp 10, smplpp_image_term 9)
struct Arena
{
  DevBuf slot[ARENA_SLOTS];
};

struct Workspace
{
  DevBuf AT;      // [KP][ldA] fp32, K-major A operand (pose coefficients | beta | 1)
  DevBuf A3;      // the same coefficients as bf16x3 pieces in fragment order (skin_b.hip)
  DevBuf A2h;     // the same coefficients as fp16x2 pieces in fragment order (skin_h.hip)
  DevBuf G2h;     // relative transforms as fp16x2 pieces, the A operand of the blend MFMAs (skin_h.hip)
  DevBuf Gp;      // [n][24][12] relative transforms, 3x4 row-major
  DevBuf root;    // [n][25][3], row 0 written: smplpp_fk_rotmat's root translation where the fused kernels read theta[f][0][:]
  int64_t ldA = 0;
};
// Per-feature state of a handle, created by the feature's first call on it and owned by the handle
struct VjpState;        // smplpp_fk_vjp's operand image and workspace (fk_vjp.hip)
struct NormalsVjpState; // the normals' backward pass (mesh_vjp.hip)
struct PointDistState;  // point-to-mesh distance and its backward pass (point_distance.hip)
struct MeshPointDistState; // mesh-to-point distance and its backward pass (mesh_point_distance.hip)
struct WindingState;    // batched winding numbers and the signed point-to-mesh distance (winding.hip)
struct SelfPenState;    // self-intersections, the self-penetration energy and its backward pass (self_penetration.hip)
struct DepthRasterState; // the depth rasteriser, its backward pass and that of the raster interpolation (raster_walk.h)
struct SilhouetteState;  // the mask distance transform, the silhouette residuals and their backward pass (silhouette.hip)
struct VertexOffsetsState; // the tile sums of the shared SMPL+D backward (vertex_offsets.hip)
struct RayCastState;     // ray casting: the rays' keys, the backward pass's records and per-frame terms (ray_cast.hip)
struct GeodesicState;    // surface geodesics: the model's edge table and the frames' edge lengths (geodesic.hip)
struct VPoserJxWork;    // a workspace of the exact-fp32 decoder Jacobian (vposer_jac_exact.hip): the decoder's own, or an IK solver's
// each overload is `delete s`, defined where its state is
struct StateDelete
{
  void operator()(VjpState * s) const;
  void operator()(NormalsVjpState * s) const;
  void operator()(PointDistState * s) const;
  void operator()(MeshPointDistState * s) const;
  void operator()(WindingState * s) const;
  void operator()(SelfPenState * s) const;
  void operator()(DepthRasterState * s) const;
  void operator()(SilhouetteState * s) const;
  void operator()(VertexOffsetsState * s) const;
  void operator()(RayCastState * s) const;
  void operator()(GeodesicState * s) const;
  void operator()(VPoserJxWork * s) const;
};
template<class T>
using StatePtr = std::unique_ptr<T, StateDelete>;
} // namespace smplpp_hip

struct smplpp_model
{
  int device = 0;
  int64_t V = 0, F = 0;
  int64_t VGn = 0;  // vertex groups of 32
  int64_t ldB = 0;  // VGn * 96
  int maxw = 0;     // skinning weights kept per vertex: 4, 8 or 24
  // device arrays
  smplpp_hip::DevPtr<float> Bm; // [KP][ldB]
  smplpp_hip::DevPtr<uint8_t> B3; // Bm as bf16x3 pieces in MFMA fragment order (layout.h, BB_*)
  int64_t VGPn = 0;            // vertex-group pairs: ceil(V / 64)
  smplpp_hip::DevPtr<uint8_t> B2h; // bases + skinning weights as fp16x2 pieces in MFMA fragment order (layout.h, HB_*)
  float sB = 1.0f, sG = 1.0f;  // power-of-two scales of the basis operand and of the relative transforms (fp16 range)
  smplpp_hip::DevPtr<int> range_flag; // device words [RANGE_SLOTS]: bit 0 = a launch of the fp16x2 form met an operand outside fp16's range
  smplpp_hip::DevPtr<uint8_t> B3e; // bases + skinning tables of the exact form, one 20 KiB image per (vertex group, k-step) (layout.h, EB_*)
  char form = 'e';             // fused-kernel form of smplpp_fk (SMPLPP_SKIN, read once at model creation): e | h | b | v
  char form_ik = 'h';          // ... of the IK / VPoser loops' internal launches (h unless SMPLPP_SKIN chose one form for everything)
  smplpp_hip::DevPtr<uint8_t> wIdx; // [VGn*32][maxw] joints of a vertex's weights, ascending (rows past V: zeros)
  smplpp_hip::DevPtr<float> wVal; // [VGn*32][maxw]
  smplpp_hip::DevPtr<float> wSum; // [VGn*32]  sum_j W[v,j] in ascending j (the blended homogeneous w)
  smplpp_hip::DevPtr<float> J0; // [24][3]      Jreg . T
  smplpp_hip::DevPtr<float> JS; // [24][3][10]  Jreg . S
  smplpp_hip::DevPtr<float> JSp; // [72][12] the two once more, a 48-byte row per joint coordinate: [JS row (10) | J0 | 0]
                                 // (pose_kernel: three 16-byte loads)
  smplpp_hip::DevPtr<int32_t> parent; // [24]
  smplpp_hip::DevPtr<int32_t> lvl; // [CT_OFF + 60 CT_LEV 2] kinematic tree by depth: 25 level offsets, the 24 joints sorted by level, then from CT_OFF
                                   // the pose kernel's chain table (layout.h, CT_*)
  int nlev = 0;                // levels of the tree (SMPL: 9)
  bool chain_fast = false;     // the chain table covers the tree: at most CT_LEV levels of at most 5 joints (other trees: the pose kernel's generic loop)
  smplpp_hip::DevPtr<int32_t> faces; // [F][3] 0-based
  smplpp_hip::DevPtr<int32_t> adjOff; // [V+1]
  smplpp_hip::DevPtr<int32_t> adjFace; // [adjOff[V]] ascending face id per vertex
  int madj = smplpp_hip::MAXADJ;  // width of the IK ring tables below: MAXADJ, or MAXADJ_WIDE when some vertex has more than MAXADJ adjacent faces
  smplpp_hip::DevPtr<uint16_t> faceRing; // [F][3 (madj + 1) + 2] IK ring of a task on face f: count, the face's three vertices, then the distinct
                                         // vertices of the faces adjacent to them in (vertex, adjacent face, corner) order (V <= 65535)
  smplpp_hip::DevPtr<uint8_t> faceMap; // [F][3 madj 3] (vertex of the face, adjacent face, corner) -> slot in that ring
  smplpp_hip::DevPtr<int32_t> anc; // [TREE_SIZE] tree tables of the IK evaluation (layout.h, TREE_*)
  smplpp_hip::DevPtr<float> Wdense; // [V][24] original weights (stage entry points / IK)
  smplpp_hip::DevPtr<float> Pvm; // [V][3][207] posedirs, vertex-major (IK Jacobian: pose-corrective term of a few vertices)
  smplpp_hip::DevPtr<float> Svm; // [V][3][10]  shapedirs, vertex-major (IK Jacobian: beta columns)
  // host mirrors
  std::vector<int32_t> h_parent, h_faces, h_adjOff, h_adjFace;
  // measurement hook (smplpp_profile_*)
  bool profiling = false;
  std::vector<hipEvent_t> prof_events; // begin/end pairs around the fused kernel
  smplpp_hip::Workspace ws;
  smplpp_hip::Arena arena;      // staging of the host-space calls on this model
  smplpp_hip::StatePtr<smplpp_hip::VjpState> vjp; // backward pass (smplpp_fk_vjp): null until its first call on the model
  smplpp_hip::StatePtr<smplpp_hip::NormalsVjpState> nvjp; // backward pass of the normal queries (mesh_vjp.hip): null until its first call
  char pd_form = 0;             // point-to-mesh distance form (SMPLPP_POINT_DISTANCE_FORM, read at model creation): 0 = by K | q | t
  smplpp_hip::StatePtr<smplpp_hip::PointDistState> pd; // point-to-mesh distance workspace (point_distance.hip): null until its first call
  smplpp_hip::StatePtr<smplpp_hip::MeshPointDistState> mpd; // mesh-to-point distance workspace (mesh_point_distance.hip): null until its first call
  smplpp_hip::StatePtr<smplpp_hip::WindingState> wn; // winding-number and signed-distance workspace (winding.hip): null until its first call
  smplpp_hip::StatePtr<smplpp_hip::SelfPenState> sp; // self-intersection and self-penetration workspace (self_penetration.hip): null until its first call
  int dr_inline = -1;           // depth rasteriser: box pixels a face's own thread walks (SMPLPP_DEPTH_RASTER_INLINE, read at model creation): -1 = default
  smplpp_hip::StatePtr<smplpp_hip::DepthRasterState> dr; // workspace of the depth rasteriser and of the raster interpolation's backward pass (raster_walk.h): null until its first call
  smplpp_hip::StatePtr<smplpp_hip::SilhouetteState> sil; // silhouette workspace (silhouette.hip): null until its first call
  int vo_frames = 0;            // SMPL+D: frames per tile of the forward and the per-frame backward (SMPLPP_VERTEX_OFFSETS_FRAMES, read at model creation): 0 = by n
  smplpp_hip::StatePtr<smplpp_hip::VertexOffsetsState> vo; // SMPL+D shared-backward workspace (vertex_offsets.hip): null until its first call
  int sp_frames = 0;            // bound points: frames a workgroup of sp_point_kernel holds in LDS (SMPLPP_SKIN_POINTS_FRAMES, read at model creation): 0 = by n and K
  int sp_split = 0;             // bound points: threads per partial of the per-joint sums (SMPLPP_SKIN_POINTS_SPLIT = 4 | 1, read at model creation): 0 = by K
  int ray_slices = 0;           // ray casting: workgroups that share a (frame, ray block)'s face chunks (SMPLPP_RAY_SLICES, read at model creation): 0 = by n and K
  smplpp_hip::StatePtr<smplpp_hip::RayCastState> rc; // ray casting workspace (ray_cast.hip): null until its first call
  smplpp_hip::StatePtr<smplpp_hip::GeodesicState> geo; // edge table and edge-length workspace of smplpp_mesh_geodesic (geodesic.hip): null until its first call
  ~smplpp_model(); // (model.hip) destroys prof_events, then the members free themselves
};
