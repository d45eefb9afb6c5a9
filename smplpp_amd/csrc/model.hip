// Model creation: replaces SMPL::init (/root/reference/src/SMPL.cpp:560-643) minus the JSON parse.
//
// HBM layout produced here (all fp32 unless noted, resident for the life of the handle; ~37 MB for SMPL):
//   Bm   [220][ldB]   B operand of the fused blend-shape GEMM, K-major: rows 0..206 posedirs, 207..216 shapedirs,
//                     217 template, 218..219 zero.  Columns are grouped per 32 vertices as [32 x | 32 y | 32 z] so
//                     that one 32x32 MFMA tile is one coordinate of 32 consecutive vertices (ldB = ceil(V/32)*96).
//   wIdx/wVal [Vpad][maxw]  skinning weights, the maxw (4, 8 or 24) non-zeros per vertex in ascending joint order.
//   wSum [Vpad]       sum_j W[v,j]: the blended homogeneous coordinate the reference divides by
//                     (src/LinearBlendSkinning.cpp:545-550).
//   J0 [24][3], JS [24][3][10]  joint regressor folded through template and shapedirs:
//                     joints = J0 + JS . beta  ==  Jreg . (T + S . beta)   (src/JointRegression.cpp:588-590)
//   faces, adjOff/adjFace      0-based faces and the per-vertex adjacent-face table (src/SMPL.cpp:620-640).
//   Pvm [V][3][207], Svm [V][3][10]  the bases once more in the file's vertex-major order, for the IK Jacobian of a
//                     handful of task vertices (a K-major gather would touch 207 cache lines per vertex).
#include "common.h"
#include "model_tables.h"

#include <cstdlib>
#include <tuple>

namespace smplpp_hip
{
typedef _Float16 f16x8h __attribute__((ext_vector_type(8)));
static thread_local std::string g_last_error;

void set_error(const std::string & msg)
{
  g_last_error = msg;
}

int fail(int code, const std::string & msg)
{
  g_last_error = msg;
  return code;
}

int hip_fail(hipError_t e, const char * what, const char * file, int line)
{
  char buf[512];
  snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
  g_last_error = buf;
  return SMPLPP_ERR_HIP;
}

// Bm[k][bcol(v,x)] <- P[v][x][k] (k < 207) | S[v][x][k-207] | T[v][x] | 0
__global__ void relayout_basis_kernel(const float * __restrict__ P, const float * __restrict__ S, const float * __restrict__ T,
                                      float * __restrict__ Bm, int64_t V, int64_t ldB)
{
  int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(col >= ldB) return;
  int64_t g = col / (3 * VG);
  int x = (int)((col % (3 * VG)) / VG);
  int64_t v = g * VG + col % VG;
  for(int k = 0; k < KP; k++)
  {
    float val = 0.0f;
    if(v < V)
    {
      if(k < NP)
        val = P[(v * 3 + x) * NP + k];
      else if(k < NP + NB)
        val = S[(v * 3 + x) * NB + (k - NP)];
      else if(k == K_ONE)
        val = T[v * 3 + x];
    }
    Bm[(int64_t)k * ldB + col] = val;
  }
}

// B3 <- Bm as bf16x3 pieces in MFMA fragment order (layout: layout.h).  One thread per (vertex-group pair, k-step,
// piece, lane): 8 consecutive k of one column.
__global__ void relayout_basis_bf16x3_kernel(const float * __restrict__ Bm, int64_t ldB, int64_t V, int64_t nvgp,
                                             uint16_t * __restrict__ B3)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // ((vgp * KS + ks) * 6 + vh * 3 + x) * 64 + lane
  if(i >= nvgp * BB_KS * 6 * 64) return;
  const int lane = (int)(i % 64), h = lane >> 5, r = lane & 31;
  const int vx = (int)((i / 64) % 6), vh = vx / 3, x = vx % 3;
  const int ks = (int)((i / (64 * 6)) % BB_KS);
  const int64_t vgp = i / (64 * 6 * BB_KS);
  const int64_t v = vgp * 64 + vh * 32 + r;
  uint16_t pc[3][8];
  for(int j = 0; j < 8; j++)
  {
    const int k = ks * 16 + 8 * h + j;
    const float val = (v < V && k < KP) ? Bm[(int64_t)k * ldB + bcol(v, x)] : 0.0f;
    split_bf16x3(val, pc[0][j], pc[1][j], pc[2][j]);
  }
  for(int s = 0; s < 3; s++)
  {
    uint16_t * dst = B3 + ((((vgp * BB_KS + ks) * 6 + vx) * 3 + s) * 64 + lane) * 8;
    for(int j = 0; j < 8; j++) dst[j] = pc[s][j];
  }
}

// B3e <- Bm as bf16x3 pieces in MFMA fragment order, one 20 KiB image per (vertex group, k-step) (layout: layout.h, EB_*).  One
// thread per (vertex group, k-step, vertex half and coordinate, lane): 8 consecutive k of one column, its three pieces.
__global__ void relayout_basis_exact_kernel(const float * __restrict__ Bm, int64_t ldB, int64_t V, int64_t nvg, uint8_t * __restrict__ B3e)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // ((vg * KS + ks) * 6 + vh * 3 + x) * 64 + lane
  if(i >= nvg * EB_KS * 6 * 64) return;
  const int lane = (int)(i % 64), h = lane >> 5, r = lane & 31;
  const int vx = (int)((i / 64) % 6), vh = vx / 3, x = vx % 3;
  const int ks = (int)((i / (64 * 6)) % EB_KS);
  const int64_t vg = i / (64 * 6 * EB_KS);
  const int64_t v = vg * 64 + vh * 32 + r;
  uint16_t pc[3][8];
  for(int j = 0; j < 8; j++)
  {
    const int k = ks * 16 + 8 * h + j;
    const float val = (v < V && k < KP) ? Bm[(int64_t)k * ldB + bcol(v, x)] : 0.0f;
    split_bf16x3(val, pc[0][j], pc[1][j], pc[2][j]);
  }
  for(int s = 0; s < 3; s++)
  {
    uint16_t * dst = reinterpret_cast<uint16_t *>(B3e + (vg * EB_KS + ks) * (int64_t)EB_IMG) + ((int64_t)(vx * 3 + s) * 64 + lane) * 8;
    for(int j = 0; j < 8; j++) dst[j] = pc[s][j];
  }
}
// the skinning tables of a vertex group, in the 2 KiB behind the fragments of its first k-steps (one thread per vertex slot)
__global__ void skin_tables_exact_kernel(const uint8_t * __restrict__ wIdx, const float * __restrict__ wVal, const float * __restrict__ wSum,
                                         int maxw, int64_t V, int64_t nvg, uint8_t * __restrict__ B3e)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= nvg * 64) return;
  const int64_t vg = i / 64, v = i;
  const int c = (int)(i % 64);
  uint8_t * g = B3e + vg * (int64_t)(EB_KS * EB_IMG);
  for(int q = 0; q < maxw && q < 8; q++)
  {
    uint8_t * tab = g + (q < 4 ? 0 : 2) * EB_IMG + EB_TAB_OFF;
    reinterpret_cast<int32_t *>(tab)[c * 4 + (q & 3)] = v < V ? (int32_t)wIdx[v * maxw + q] * 48 : 0;
    reinterpret_cast<float *>(tab + 1024)[c * 4 + (q & 3)] = v < V ? wVal[v * maxw + q] : 0.0f;
  }
  reinterpret_cast<float *>(g + EB_IMG + EB_TAB_OFF)[c] = v < V ? 1.0f / wSum[v] : 0.0f;
}

// B2h <- Bm and the skinning weights as fp16x2 pieces in MFMA fragment order (layout: layout.h).  One thread per 16-byte
// chunk pair (hi, lo): slots 0..13: ((vg * 15 + ks) * 6 + vh * 3 + x) * 64 + lane; slot 14: weights, cw, padding.
// hperm [nvg * 64]: the vertex in each slot of each group (-1: none), gflags [nvg]: the group's k-step flags (layout.h, HB_PERM_OFF).
__global__ void relayout_basis_f16x2_kernel(const float * __restrict__ Bm, int64_t ldB, const float * __restrict__ W,
                                            const float * __restrict__ wSum, int64_t V, int64_t nvg, float sB, float sG,
                                            uint8_t * __restrict__ B2h, const int32_t * __restrict__ hperm,
                                            const int32_t * __restrict__ gflags)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_vg = HB_KS * 6 * 64 + 4 * 64 + 64; // basis chunk pairs + weight chunk pairs + cw entries
  if(i >= nvg * per_vg) return;
  const int64_t vg = i / per_vg;
  const int q = (int)(i % per_vg);
  uint8_t * base = B2h + vg * (int64_t)(HB_SLOTS * HB_IMG);
  f16x8h hi, lo;
  if(q < HB_KS * 6 * 64)
  {
    const int lane = q % 64, h = lane >> 5, r = lane & 31;
    const int vx = (q / 64) % 6, vh = vx / 3, x = vx % 3, ks = q / (64 * 6);
    const int64_t v = hperm[vg * 64 + vh * 32 + r];
    for(int j = 0; j < 8; j++)
    {
      const int k = ks * 16 + 8 * h + j;
      const float val = (v >= 0 && k < KP) ? Bm[(int64_t)k * ldB + bcol(v, x)] : 0.0f;
      _Float16 a, b;
      split_f16x2(val * sB, a, b);
      hi[j] = a;
      lo[j] = b;
    }
    uint8_t * dst = base + ks * HB_IMG + ((vh * 3 + x) * 2) * 1024 + lane * 16;
    *reinterpret_cast<f16x8h *>(dst) = hi;
    *reinterpret_cast<f16x8h *>(dst + 1024) = lo;
  }
  else if(q < HB_KS * 6 * 64 + 4 * 64)
  {
    const int w = q - HB_KS * 6 * 64, lane = w % 64, h = lane >> 5, r = lane & 31, vh = (w / 64) % 2, ks = w / 128;
    const int64_t v = hperm[vg * 64 + vh * 32 + r];
    for(int j = 0; j < 8; j++)
    {
      const int k = ks * 16 + 8 * h + j; // joint
      const float val = (v >= 0 && k < NJ) ? W[v * NJ + k] : 0.0f;
      _Float16 a, b;
      split_f16x2(val * HB_SW, a, b);
      hi[j] = a;
      lo[j] = b;
    }
    uint8_t * dst = base + HB_KS * HB_IMG + ((ks * 2 + vh) * 2) * 1024 + lane * 16;
    *reinterpret_cast<f16x8h *>(dst) = hi;
    if(ks == 0)
      *reinterpret_cast<f16x8h *>(dst + 1024) = lo;
    else if(h == 0)
    {
      // k-step 1 has eight live k (joints 16..23): its second fragment is [hi | lo] over the two lane halves, so that one
      // MFMA against the G' hi piece (read by both halves) is Ghi.Whi + Ghi.Wlo (skin_h.hip)
      *reinterpret_cast<f16x8h *>(dst + 1024) = hi;
      *reinterpret_cast<f16x8h *>(dst + 1024 + 512) = lo;
    }
  }
  else
  {
    // cw = 1 / (sG sW h[3]) with h[3] = sum_j W[v,j], the homogeneous coordinate the reference divides by
    // (src/LinearBlendSkinning.cpp:545-550): one reciprocal per vertex (<= 1 ulp from the division)
    const int c = q - (HB_KS * 6 * 64 + 4 * 64);
    const int64_t v = hperm[vg * 64 + c];
    uint8_t * s14 = base + HB_KS * HB_IMG;
    float * cw = reinterpret_cast<float *>(s14 + HB_CW_OFF);
    cw[c] = v >= 0 ? (1.0f / wSum[v]) / (sG * HB_SW) : 0.0f;
    reinterpret_cast<int32_t *>(s14 + HB_PERM_OFF)[c] = (int32_t)v; // where this slot's vertex goes in the outputs
    // the flags word, then zeros up to the end of the slot (its DMA copies whole 12 KiB images)
    int32_t * tail = reinterpret_cast<int32_t *>(s14 + HB_FLAGS_OFF);
    for(int i = c; i < (HB_IMG - HB_FLAGS_OFF) / 4; i += 64) tail[i] = (i == 0) ? gflags[vg] : 0;
  }
}

// One block per (joint j, coordinate x, term t): t < 10 -> JS[j][x][t] = sum_v Jreg[j,v] S[v,x,t];
// t == 10 -> J0[j][x] = sum_v Jreg[j,v] T[v,x].  Wavefront (64-lane) shuffle reduction, then across the 4 waves.
__global__ __launch_bounds__(256) void fold_regressor_kernel(const float * __restrict__ Jreg, const float * __restrict__ S,
                                                              const float * __restrict__ T, float * __restrict__ J0,
                                                              float * __restrict__ JS, int64_t V)
{
  const int t = blockIdx.x % (NB + 1);
  const int x = (blockIdx.x / (NB + 1)) % 3;
  const int j = blockIdx.x / (3 * (NB + 1));
  double acc = 0.0; // fp64 partials: the reference's GEMM summation order over 6890 terms is BLAS-defined
  for(int64_t v = threadIdx.x; v < V; v += blockDim.x)
  {
    float w = Jreg[(int64_t)j * V + v];
    float b = (t < NB) ? S[(v * 3 + x) * NB + t] : T[v * 3 + x];
    acc += (double)w * (double)b;
  }
  for(int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double part[4];
  if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if(threadIdx.x == 0)
  {
    double s = (part[0] + part[1]) + (part[2] + part[3]);
    if(t < NB)
      JS[(j * 3 + x) * NB + t] = (float)s;
    else
      J0[j * 3 + x] = (float)s;
  }
}

// [72][12]: row t = [JS[t][0..9] | J0[t] | 0]
__global__ void pack_regressor_rows_kernel(const float * __restrict__ J0, const float * __restrict__ JS, float * __restrict__ JSp)
{
  const int t = threadIdx.x;
  for(int k = 0; k < NB; k++) JSp[t * 12 + k] = JS[t * NB + k];
  JSp[t * 12 + 10] = J0[t];
  JSp[t * 12 + 11] = 0.0f;
}

template<class T>
static hipError_t upload(DevPtr<T> & dst, const T * src, size_t count)
{
  hipError_t e = dev_alloc(dst, count);
  if(e != hipSuccess) return e;
  if(count) e = hipMemcpy(dst.get(), src, sizeof(T) * count, hipMemcpyHostToDevice);
  return e;
}
} // namespace smplpp_hip

using namespace smplpp_hip;

extern "C" const char * smplpp_last_error(void)
{
  return g_last_error.c_str();
}

extern "C" int smplpp_device_count(int * count)
{
  if(!count) return fail(SMPLPP_ERR_INVALID, "smplpp_device_count: null argument");
  *count = 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if(e != hipSuccess || n <= 0)
  {
    (void)hipGetLastError();
    return fail(SMPLPP_ERR_HIP, "no HIP device visible (libsmplpp_hip.so is MI355X-only and has no CPU path)");
  }
  *count = n;
  return SMPLPP_OK;
}

smplpp_model::~smplpp_model()
{
  (void)hipSetDevice(device);
  for(hipEvent_t e : prof_events) (void)hipEventDestroy(e);
}

extern "C" int smplpp_model_destroy(smplpp_model * m)
{
  if(m) delete m;
  return SMPLPP_OK;
}

// SMPLPP_SKIN, SMPLPP_POINT_DISTANCE_FORM, SMPLPP_DEPTH_RASTER_INLINE, SMPLPP_VERTEX_OFFSETS_FRAMES, SMPLPP_SKIN_POINTS_* and SMPLPP_RAY_SLICES are read here, once per model (m.maxw and m.VGPn are set)
static void read_env(smplpp_model & m)
{
  std::tie(m.form, m.form_ik) = choose_forms(getenv("SMPLPP_SKIN"), m.maxw, m.VGPn);
  const char * pd_env = getenv("SMPLPP_POINT_DISTANCE_FORM"); // query | tiled: one form of smplpp_point_mesh_distance for every K
  m.pd_form = pd_env && (pd_env[0] == 'q' || pd_env[0] == 't') ? pd_env[0] : 0;
  const char * dr_env = getenv("SMPLPP_DEPTH_RASTER_INLINE"); // 0..4096: the largest box a face's own thread walks in smplpp_depth_raster
  m.dr_inline = dr_env && dr_env[0] >= '0' && dr_env[0] <= '9' ? atoi(dr_env) : -1;
  const char * vo_env = getenv("SMPLPP_VERTEX_OFFSETS_FRAMES"); // 1..32: frames per tile of smplpp_vertex_offsets and its per-frame backward (no bit depends on it)
  const int vo_ft = vo_env ? atoi(vo_env) : 0;
  m.vo_frames = vo_ft >= 1 && vo_ft <= SMPLPP_VERTEX_OFFSETS_TILE ? vo_ft : 0;
  const char * spf_env = getenv("SMPLPP_SKIN_POINTS_FRAMES"); // 1..32: frames a workgroup of the bound points' per-point kernel holds (no bit depends on it)
  const int sp_ft = spf_env ? atoi(spf_env) : 0;
  m.sp_frames = sp_ft >= 1 && sp_ft <= SMPLPP_VERTEX_OFFSETS_TILE ? sp_ft : 0;
  const char * sps_env = getenv("SMPLPP_SKIN_POINTS_SPLIT"); // 4 | 1: partials per thread of the bound points' per-joint sums (no bit depends on it)
  const int sp_nq = sps_env ? atoi(sps_env) : 0;
  m.sp_split = sp_nq == 4 || sp_nq == 1 ? sp_nq : 0;
  const char * rs_env = getenv("SMPLPP_RAY_SLICES"); // 1..4096: workgroups that share a (frame, ray block)'s face chunks in smplpp_ray_cast (no bit depends on it)
  const int rs = rs_env ? atoi(rs_env) : 0;
  m.ray_slices = rs >= 1 && rs <= 4096 ? rs : 0;
}

// Validate, build the host tables (model_tables.h), then upload them and lay the bases out on the device.
extern "C" int smplpp_model_create(int64_t V, int64_t F, const float * vt, const float * S, const float * P,
                                   const float * Jreg, const float * W, const int64_t * kintree, const int32_t * faces1,
                                   int device, smplpp_model ** out)
{
  if(!out) return fail(SMPLPP_ERR_INVALID, "smplpp_model_create: null output");
  *out = nullptr;
  if(V <= 0 || F < 0 || !vt || !S || !P || !Jreg || !W || !kintree || (F > 0 && !faces1))
    return fail(SMPLPP_ERR_INVALID, "Cannot initialize a SMPL model!"); // src/SMPL.cpp:616
  int ndev = 0;
  int rc = smplpp_device_count(&ndev);
  if(rc) return rc;
  if(device < 0 || device >= ndev) return fail(SMPLPP_ERR_INVALID, "Failed to fetch device index!"); // src/SMPL.cpp:295
  std::vector<int32_t> parent;
  if(const char * why = check_tree(kintree, parent)) return fail(SMPLPP_ERR_INVALID, why);
  if(const char * why = check_faces(faces1, F, V)) return fail(SMPLPP_ERR_INVALID, why);

  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<smplpp_model> m(new smplpp_model());
  m->device = device;
  m->V = V;
  m->F = F;
  m->VGn = (V + VG - 1) / VG;
  m->ldB = m->VGn * 3 * VG;
  m->VGPn = (V + 63) / 64;

  // --- host tables; only the operand layouts the chosen forms read are built
  const SkinWeights sw = skin_weights(W, V);
  m->maxw = sw.maxw;
  read_env(*m);
  auto uses = [&](char f) { return m->form == f || m->form_ik == f; };
  VertexGroups hgroups;
  if(uses('h'))
  {
    const HScales hs = h_scales(P, S, vt, V);
    if(hs.refusal) return fail(SMPLPP_ERR_INVALID, hs.refusal);
    m->sB = hs.sB;
    m->sG = hs.sG;
    hgroups = h_vertex_groups(W, V);
  }
  const JointLevels levels = joint_levels(parent);
  const ChainTables chain = chain_tables(parent, levels);
  const std::vector<int32_t> anc = ik_tree_tables(parent, levels);
  Adjacency adj = adjacency(faces1, F, V);
  const RingTables ring = ik_ring_tables(adj.faces.data(), adj.adjOff.data(), adj.adjFace.data(), F, V);
  m->nlev = levels.nlev;
  m->chain_fast = chain.chain_fast;
  m->madj = ring.madj;
  m->h_parent = parent;
  m->h_faces = std::move(adj.faces);
  m->h_adjOff = std::move(adj.adjOff);
  m->h_adjFace = std::move(adj.adjFace);

  // --- blend bases -> Bm, regressor fold (device side; the raw arrays are only needed transiently)
  HIP_TRY(upload(m->Pvm, P, (size_t)V * 3 * NP)); // kept: vertex-major copies serve the sparse IK Jacobian (contiguous 2.5 KB per vertex)
  HIP_TRY(upload(m->Svm, S, (size_t)V * 3 * NB));
  DevPtr<float> dT, dJreg;
  HIP_TRY(upload(dT, vt, (size_t)V * 3));
  HIP_TRY(upload(dJreg, Jreg, (size_t)NJ * V));
  HIP_TRY(dev_alloc(m->Bm, (size_t)KP * m->ldB));
  HIP_TRY(dev_alloc(m->J0, NJ * 3));
  HIP_TRY(dev_alloc(m->JS, NJ * 3 * NB));
  relayout_basis_kernel<<<dim3((unsigned)((m->ldB + 255) / 256)), dim3(256)>>>(m->Pvm.get(), m->Svm.get(), dT.get(), m->Bm.get(), V, m->ldB);
  fold_regressor_kernel<<<dim3(NJ * 3 * (NB + 1)), dim3(256)>>>(dJreg.get(), m->Svm.get(), dT.get(), m->J0.get(), m->JS.get(), V);
  HIP_TRY(dev_alloc(m->JSp, NJ * 3 * 12));
  pack_regressor_rows_kernel<<<dim3(1), dim3(NJ * 3)>>>(m->J0.get(), m->JS.get(), m->JSp.get());
  if(uses('b'))
  {
    HIP_TRY(dev_alloc(m->B3, (size_t)m->VGPn * BB_KS * BB_B_BYTES));
    const int64_t cnt = m->VGPn * BB_KS * 6 * 64;
    relayout_basis_bf16x3_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256)>>>(m->Bm.get(), m->ldB, V, m->VGPn,
                                                                                  reinterpret_cast<uint16_t *>(m->B3.get()));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  dT.reset(); // (here, before the launches below: freeing device memory waits for the device)
  dJreg.reset();

  // --- skinning weights, then the operand images of the e and h forms
  HIP_TRY(upload(m->wIdx, sw.wIdx.data(), sw.wIdx.size()));
  HIP_TRY(upload(m->wVal, sw.wVal.data(), sw.wVal.size()));
  HIP_TRY(upload(m->wSum, sw.wSum.data(), sw.wSum.size()));
  HIP_TRY(upload(m->Wdense, W, (size_t)V * NJ));
  if(uses('e'))
  {
    HIP_TRY(dev_alloc(m->B3e, (size_t)m->VGPn * EB_KS * EB_IMG));
    HIP_TRY(hipMemset(m->B3e.get(), 0, (size_t)m->VGPn * EB_KS * EB_IMG));
    const int64_t cnt = m->VGPn * EB_KS * 6 * 64;
    relayout_basis_exact_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256)>>>(m->Bm.get(), m->ldB, V, m->VGPn, m->B3e.get());
    skin_tables_exact_kernel<<<dim3((unsigned)((m->VGPn * 64 + 255) / 256)), dim3(256)>>>(m->wIdx.get(), m->wVal.get(), m->wSum.get(), m->maxw, V,
                                                                                       m->VGPn, m->B3e.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  if(uses('h'))
  {
    HIP_TRY(dev_alloc(m->B2h, (size_t)m->VGPn * HB_SLOTS * HB_IMG));
    DevPtr<int32_t> dPerm, dFlags;
    HIP_TRY(upload(dPerm, hgroups.perm.data(), hgroups.perm.size()));
    HIP_TRY(upload(dFlags, hgroups.flags.data(), hgroups.flags.size()));
    const int64_t cnt = m->VGPn * (HB_KS * 6 * 64 + 4 * 64 + 64);
    relayout_basis_f16x2_kernel<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256)>>>(m->Bm.get(), m->ldB, m->Wdense.get(), m->wSum.get(), V,
                                                                                 m->VGPn, m->sB, m->sG, m->B2h.get(), dPerm.get(), dFlags.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  if(!uses('v')) m->Bm.reset(); // only the fp32-MFMA form reads the K-major fp32 basis

  // --- the small tables: kinematic tree, faces and adjacency, IK tree and ring tables
  HIP_TRY(upload(m->parent, parent.data(), parent.size()));
  {
    const int zero[RANGE_SLOTS] = {};
    HIP_TRY(upload(m->range_flag, zero, RANGE_SLOTS));
  }
  HIP_TRY(upload(m->lvl, chain.lvl.data(), chain.lvl.size()));
  HIP_TRY(upload(m->faces, m->h_faces.data(), m->h_faces.size()));
  HIP_TRY(upload(m->adjOff, m->h_adjOff.data(), m->h_adjOff.size()));
  HIP_TRY(upload(m->adjFace, m->h_adjFace.data(), m->h_adjFace.size()));
  HIP_TRY(upload(m->anc, anc.data(), anc.size()));
  if(!ring.faceRing.empty())
  {
    HIP_TRY(upload(m->faceRing, ring.faceRing.data(), ring.faceRing.size()));
    HIP_TRY(upload(m->faceMap, ring.faceMap.data(), ring.faceMap.size()));
  }
  *out = m.release();
  return SMPLPP_OK;
}

extern "C" int smplpp_model_info(const smplpp_model * m, int64_t * V, int64_t * F, int * wpv, int * device)
{
  if(!m) return fail(SMPLPP_ERR_INVALID, "smplpp_model_info: null model");
  if(V) *V = m->V;
  if(F) *F = m->F;
  if(wpv) *wpv = m->maxw;
  if(device) *device = m->device;
  return SMPLPP_OK;
}

extern "C" int smplpp_adjacent_faces(const smplpp_model * m, int64_t vertex, int64_t cap, int64_t * faces, float * weights,
                                     int64_t * count)
{
  if(!m || !count) return fail(SMPLPP_ERR_INVALID, "smplpp_adjacent_faces: null argument");
  if(vertex < 0 || vertex >= m->V) return fail(SMPLPP_ERR_INVALID, "smplpp_adjacent_faces: vertex out of range");
  int32_t b = m->h_adjOff[vertex], e = m->h_adjOff[vertex + 1];
  *count = e - b;
  float sum = 0.0f;
  for(int32_t q = b; q < e; q++) sum += 1.0f;
  for(int32_t q = b; q < e && q - b < cap; q++)
  {
    if(faces) faces[q - b] = m->h_adjFace[q];
    if(weights) weights[q - b] = 1.0f / sum; // uniform 1/deg (src/SMPL.cpp:630-639)
  }
  return SMPLPP_OK;
}
