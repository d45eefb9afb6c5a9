// The IK loop of the reference (node/node.cpp:645-1002) for a batch of independent frames, one workgroup per frame.
//
//  ik_eval_kernel    node.cpp:798-877.  The reference gets each Jacobian row by a full reverse-mode autograd pass
//                    through the 6890-vertex FK graph (3-4 passes per task); here the same derivative is the analytic
//                    forward-mode Jacobian of only the vertices the tasks touch: per frame the chain
//                    derivatives dG'_i/dtheta_{j,k} of all 72 rotation columns are built once in LDS (41 KB: three columns per
//                    ancestor depth), one tree level per step, then every
//                    task reads them for its face vertices (and their 1-rings when a normal is involved: per-face ring
//                    tables built with the model).  In the VPoser layout it also writes the latent rows (node.cpp:761-772).
//  ik_solve_kernel   node.cpp:883-968: A = J^T J + damping in fp64 built straight from J staged through LDS, right-looking
//                    Cholesky of the packed lower-triangular augmented system in LDS (fp64) or the box QP by a primal
//                    active set around it, config update, query points for the re-projection.
//  proj_scan/finish  node.cpp:970-1001: exact closest point on the posed mesh (all 13776 faces, sphere-culled against the
//                    distance to each task's current face; each face gathered once per frame for all K queries), new
//                    face id and area-ratio weights.
// All fp32 where the reference is fp32 (FK, task geometry, autograd gradients), fp64 where it is fp64 (Eigen).
#include "ik_types.h"
#include "ik_eval.h"
#include "ik_solve.h"
#include "ik_proj.h"
#include "vposer_state.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <type_traits>

using namespace smplpp_hip;

struct smplpp_ik
{
  smplpp_model * m = nullptr;
  smplpp_vposer * vp = nullptr;
  int64_t n = 0, K = 0;
  int64_t frame_base = 0; // global index of frame 0 when this solver holds a shard of a larger job (smplpp_ik_set_frame_base)
  int theta_dim = TD75;
  TaskArrays ta{};
  float *theta = nullptr, *beta = nullptr, *theta25 = nullptr, *vjac = nullptr;
  float *verts = nullptr, *rest = nullptr, *joints = nullptr, *poserot = nullptr, *pts = nullptr;
  double *e = nullptr, *J = nullptr, *Jl = nullptr, *e2 = nullptr, *xout = nullptr;
  int *skip = nullptr, *status = nullptr, *sticky = nullptr, *list_cnt = nullptr, *list_f = nullptr;
  int * range_word = nullptr; // this solver's own "an operand left the fp16x2 form's range" word (status bit 3): its loops' forward passes report here
  int32_t * roles = nullptr; // [DMAX][EVAL_NT] the chain-derivative entries of every thread of ik_eval_kernel (slot u: row u)
  float * list_d = nullptr;
  std::vector<DevPtr<void>> owned; // what the raw pointers of this struct point to
  bool have_eval = false;
  int64_t last_D = 0; // unknowns of the last solve (theta_dim + 2K + beta_dim): the row length of xout (smplpp_ik_get_step)
  // re-projection beside the solve: when no task's surface coordinates can move (phiLimit_ <= 0 everywhere, or the
  // motion stage's forced zero, node.cpp:699) the query points are the actual positions the evaluation already wrote,
  // so the face scan does not depend on the solve and runs on a second stream while the solve is in flight
  // The posed mesh is double-buffered so that the side stream can still read iteration i's mesh (scan + finish) while the
  // main stream already writes iteration i+1's; the join sits in front of iteration i+1's evaluation, the first kernel that
  // reads what the finish kernel wrote (face, weights). Both events ride on a kernel's own completion signal
  // (hipExtLaunchKernelGGL): a separate hipEventRecord costs the recording stream ~7 us per iteration.
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool phi_locked = false;
  bool side_pending = false; // a finish kernel is in flight on the side stream; ev_join / the join flag marks its end
  // hand-over between the two streams through device flags (wg_signal + hipStreamWaitValue32) instead of events: [0] fork
  // flag, [16] its workgroup counter, [32] join flag, [48] its counter (one 64-byte line each)
  int * dbg_buf = nullptr;
  unsigned * sig = nullptr;
  unsigned tick_fork = 0, tick_join = 0, tick_done = 0; // ([64] / [80]: the solve's "configuration final" flag and its counter)
  bool use_flags = false;
  // Latent layout with few frames (a capture fit's chains: one decoder workgroup per frame, most of the chip idle).  The decoder's
  // VALUE is all the pose step, the fused kernel and the evaluation's direct rows need; its Jacobian (two thirds of the kernel's
  // 29 us) only the pull-back behind them.  So when another iteration follows, the side stream — idle once scan + finish are done,
  // well before the solve ends — waits for the solve's "configuration final" flag and makes the NEXT iteration's Jacobian there
  // (vposer_jac2_kernel<NF, false>, `out` null, raising the join flag at its end), while the main stream decodes the value with the
  // kernel's value-only instantiation (<NF, true>: the same bits, 18 us), poses, skins and joins: the Jacobian is there when the
  // evaluation (which pulls its rows back through it) starts.  Same kernels' arithmetic, another schedule: bit-identical
  // (tests/test_mocap_gpu.py).  SMPLPP_IK_LATENT_SPLIT=0/1 (read at creation) overrides the n <= 128 rule.
  double last_enqueue_us = 0.0; // host time of the last smplpp_ik_solve_sequence's / smplpp_ik_iterate's enqueue loop
  bool latent_split = false;
  bool latent_split_default = false; // (what creation chose: the default arithmetic mode's schedule)
  // smplpp_ik_set_arithmetic(SMPLPP_IK_ARITH_EXACT): the loops' forward passes run the model's smplpp_fk form (m->form), and the
  // decoder decodes with the exact-fp32 value kernel and makes vjac with the exact-fp32 Jacobian kernels (vposer_jac_exact.hip), on
  // the main stream, in this solver's own workspace jxw; latent_split is off
  bool exact = false;
  StatePtr<VPoserJxWork> jxw;
  bool jac_ahead = false; // the decoder Jacobian of the CURRENT configuration is (being) made on the side stream; the join flag follows it
  // development switches, read ONCE at creation (never in the per-call path): SMPLPP_DEBUG_SYNC, SMPLPP_IK_DBG_STOP,
  // SMPLPP_IK_OVERLAP=0 (re-projection behind the solve on one stream), SMPLPP_SCAN_BLOCKS
  bool dbg_sync = false, overlap_ok = true;
  int dbg_stop = 0;
  int64_t scan_blocks = 1536;
  int scan_form = -1; // development switch SMPLPP_SCAN_FORM (read at creation): 0 forces the K > 8 instantiations of the face scan
  float * vbuf[2] = {nullptr, nullptr};
  int vcur = 0;
  Arena arena; // staging of the host-space calls on this solver (its own: the model is another handle, maybe another thread's)
  ~smplpp_ik()
  {
    (void)hipSetDevice(m->device);
    if(side) (void)hipStreamSynchronize(side);
    if(ev_fork) (void)hipEventDestroy(ev_fork);
    if(ev_join) (void)hipEventDestroy(ev_join);
    if(side) (void)hipStreamDestroy(side);
  }
};

// What a solver buffer holds when it has just been made.  AS_ALLOCATED: nothing — it is written before it is read.
enum Fill { AS_ALLOCATED, ZERO_BYTES, VALUE, DEFAULT_NORMAL };

// one device buffer of the solver: allocated, handed to s->owned, and filled (null stream); VALUE and DEFAULT_NORMAL are float fills
template<class T>
static hipError_t dalloc(smplpp_ik * s, T *& p, size_t count, Fill fill, float v = 0.0f)
{
  DevPtr<T> d;
  hipError_t e = dev_alloc(d, count);
  p = d.get();
  if(e != hipSuccess) return e;
  s->owned.emplace_back(std::move(d));
  if(fill == AS_ALLOCATED) return hipSuccess;
  if(fill == ZERO_BYTES) return hipMemset(p, 0, sizeof(T) * count);
  if constexpr(std::is_same_v<T, float>)
  {
    const dim3 grid((unsigned)((count + 255) / 256));
    if(fill == VALUE) fill_f32_kernel<<<grid, 256>>>(p, v, (int64_t)count);
    if(fill == DEFAULT_NORMAL) fill_nrm_kernel<<<grid, 256>>>(p, (int64_t)count);
    return hipGetLastError();
  }
  return hipErrorInvalidValue; // (a float fill of a buffer of another type)
}

static ModelView view_of(const smplpp_model * m)
{
  ModelView mv;
  mv.faces = m->faces.get();
  mv.adjOff = m->adjOff.get();
  mv.adjFace = m->adjFace.get();
  mv.parent = m->parent.get();
  mv.wIdx = m->wIdx.get();
  mv.wVal = m->wVal.get();
  mv.wSum = m->wSum.get();
  mv.Pvm = m->Pvm.get();
  mv.Svm = m->Svm.get();
  mv.JS = m->JS.get();
  mv.faceRing = m->faceRing.get();
  mv.faceMap = m->faceMap.get();
  mv.anc = m->anc.get();
  mv.nlev = m->nlev;
  mv.V = m->V;
  mv.maxw = m->maxw;
  return mv;
}

extern "C" int smplpp_ik_destroy(smplpp_ik * s)
{
  if(s) delete s;
  return SMPLPP_OK;
}

extern "C" int smplpp_ik_set_frame_base(smplpp_ik * s, int64_t frame_base)
{
  if(!s || frame_base < 0) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_frame_base: bad argument");
  s->frame_base = frame_base;
  s->jac_ahead = false;
  return SMPLPP_OK;
}

extern "C" int smplpp_ik_set_arithmetic(smplpp_ik * s, int mode)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_arithmetic: null solver");
  if(mode != SMPLPP_IK_ARITH_DEFAULT && mode != SMPLPP_IK_ARITH_EXACT) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_arithmetic: unknown mode");
  if(mode == SMPLPP_IK_ARITH_EXACT && s->m->form == 'h')
    return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_arithmetic: the model's forward form is the fp16x2 one (SMPLPP_SKIN=h)");
  HIP_TRY(hipSetDevice(s->m->device));
  // whatever the side stream still has in flight for the old mode (a Jacobian made ahead writes vjac) ends first
  if(s->side) HIP_TRY(hipStreamSynchronize(s->side));
  HIP_TRY(hipDeviceSynchronize());
  s->exact = mode == SMPLPP_IK_ARITH_EXACT;
  s->latent_split = s->exact ? false : s->latent_split_default;
  s->jac_ahead = false;
  return SMPLPP_OK;
}

extern "C" int smplpp_ik_create(smplpp_model * m, int64_t n, int64_t K, smplpp_vposer * vposer, smplpp_ik ** out)
{
  if(!m || !out || n <= 0 || K <= 0) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: bad argument");
  *out = nullptr;
  if(m->F <= 0) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: the model has no faces");
  if(m->nlev > DMAX) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: kinematic trees deeper than 12 levels are not supported");
  if(m->V > 65535) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: at most 65535 vertices are supported (ring tables hold 16-bit ids)");
  if(!m->faceRing || !m->faceMap || !m->anc) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: the model carries no ring tables");
  // the per-thread entries of the evaluation's chain-derivative steps (ik_plan.h: eval_roles); every level must fit the workgroup
  // (SMPL: at most 5 x 9 x 9 = 405 of 1024)
  std::vector<int32_t> roles;
  if(const char * why = eval_roles(m->h_parent, EVAL_NT, roles)) return fail(SMPLPP_ERR_INVALID, why);
  if(K > PROJ_MAXK) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: at most 48 tasks per frame are supported");
  if(TD75 + 2 * K + NB > MAXD)
    return fail(SMPLPP_ERR_INVALID, "smplpp_ik_create: too many tasks for the in-LDS solver (75 + 2K + 10 must be <= 181)");
  // (a vertex with more than 16 adjacent faces — the widest table the evaluation is instantiated for — does not stop the solver from being created: position-only tasks anywhere and
  // normal-term tasks away from such a vertex are unaffected; a normal-term task that touches one is reported when it is evaluated)
  HIP_TRY(hipSetDevice(m->device));
  std::unique_ptr<smplpp_ik> s(new smplpp_ik());
  s->m = m;
  s->vp = vposer;
  s->n = n;
  s->K = K;
  s->theta_dim = vposer ? TD44 : TD75;
  {
    const char * e;
    s->dbg_sync = getenv("SMPLPP_DEBUG_SYNC") != nullptr;
    if((e = getenv("SMPLPP_IK_DBG_STOP"))) s->dbg_stop = atoi(e);
    if((e = getenv("SMPLPP_IK_OVERLAP"))) s->overlap_ok = e[0] != '0';
    if(s->dbg_sync) s->overlap_ok = false;
    s->scan_blocks = default_scan_blocks(n, K, m->F); // (workgroups of the face scan: ik_plan.h; SMPLPP_SCAN_BLOCKS overrides)
    if((e = getenv("SMPLPP_SCAN_BLOCKS"))) s->scan_blocks = atoll(e);
    if((e = getenv("SMPLPP_SCAN_FORM"))) s->scan_form = atoi(e);
    s->latent_split = vposer != nullptr && n <= 128 && s->dbg_stop == 0;
    // (a debug stop ends the solve kernel in front of its "configuration final" flag: never beside the schedule that waits for it)
    if((e = getenv("SMPLPP_IK_LATENT_SPLIT"))) s->latent_split = vposer != nullptr && e[0] != '0' && s->dbg_stop == 0;
  }
  const size_t nk = (size_t)n * K;
  const size_t Dmax = TD75 + 2 * K + NB;
  const size_t nV3 = (size_t)n * m->V * 3;
  smplpp_ik * const p = s.get();
  // IkTask defaults (include/smplpp/IkTask.h:54-84)
  HIP_TRY(dalloc(p, p->ta.face, nk, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->ta.vw, nk * 3, VALUE, 1.0f / 3.0f));
  HIP_TRY(dalloc(p, p->ta.tang, nk * 6, VALUE, 0.0f));
  HIP_TRY(dalloc(p, p->ta.tpos, nk * 3, VALUE, 0.0f));
  HIP_TRY(dalloc(p, p->ta.tnrm, nk * 3, DEFAULT_NORMAL));
  HIP_TRY(dalloc(p, p->ta.posw, nk, VALUE, 1.0f));
  HIP_TRY(dalloc(p, p->ta.nrmw, nk, VALUE, 1.0f));
  HIP_TRY(dalloc(p, p->ta.philim, nk, VALUE, 0.04f));
  HIP_TRY(dalloc(p, p->ta.noff, nk, VALUE, 0.0f));
  // what the evaluation writes for the solve and the re-projection
  HIP_TRY(dalloc(p, p->ta.apos, nk * 3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->ta.anrm, nk * 3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->ta.hint, nk, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->ta.roww, nk * 2, AS_ALLOCATED));
  // the configuration
  HIP_TRY(dalloc(p, p->theta, (size_t)n * p->theta_dim, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->beta, (size_t)n * NB, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->theta25, (size_t)n * 75, ZERO_BYTES));
  // the forward pass's outputs
  HIP_TRY(dalloc(p, p->vbuf[0], nV3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->vbuf[1], nV3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->rest, nV3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->joints, (size_t)n * NJ * 3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->poserot, (size_t)n * NJ * 9, AS_ALLOCATED));
  // evaluation -> solve -> re-projection
  HIP_TRY(dalloc(p, p->pts, nk * 3, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->e, nk * 4, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->J, nk * 4 * Dmax, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->e2, (size_t)n, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->xout, (size_t)n * Dmax, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->roles, roles.size(), AS_ALLOCATED)); // (uploaded below)
  HIP_TRY(dalloc(p, p->list_cnt, nk, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->list_d, nk * PROJ_LIST, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->list_f, nk * PROJ_LIST, AS_ALLOCATED));
  HIP_TRY(dalloc(p, p->skip, (size_t)n, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->status, (size_t)n, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->sticky, (size_t)n, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->range_word, 1, ZERO_BYTES));
  HIP_TRY(dalloc(p, p->sig, 128, ZERO_BYTES));
  if(vposer)
  {
    HIP_TRY(dalloc(p, p->Jl, nk * 4 * Dmax, AS_ALLOCATED));
    HIP_TRY(dalloc(p, p->vjac, (size_t)n * 63 * 32, AS_ALLOCATED));
  }
  HIP_TRY(hipMemcpy(s->roles, roles.data(), sizeof(int32_t) * roles.size(), hipMemcpyHostToDevice));
  s->ta.flags = s->sticky;
  s->verts = s->vbuf[0];
  // (default priority: a lowest-priority side stream — tried against the scan being dispatched ahead of the solve — halved the
  // latent-IK leg of bench.py, where several solvers' streams exist; what fixes that order is the solve kernel's own "all my
  // workgroups run" flag, see ik_solve_kernel)
  HIP_TRY(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
  {
    // stream memory operations are optional in HIP: probe once (flag 0 >= 0 is satisfied at once); SMPLPP_IK_EVENTS=1 keeps events
    const char * e = getenv("SMPLPP_IK_EVENTS");
    if(!(e && e[0] != '0'))
    {
      s->use_flags = hipStreamWaitValue32(s->side, s->sig, 0u, hipStreamWaitValueGte, 0xffffffffu) == hipSuccess;
      (void)hipGetLastError();
    }
    if(!s->use_flags) s->latent_split = false; // (the hand-overs of that schedule are flags)
    s->latent_split_default = s->latent_split;
  }
  HIP_TRY(hipDeviceSynchronize());
  *out = s.release();
  return SMPLPP_OK;
}

// copy caller array -> solver array with optional conversion
template<class Src, class Dst, class Conv>
static int set_array(Frame & fr, const Src * src, Dst * dst, size_t count, Conv conv)
{
  if(!src) return SMPLPP_OK;
  const Src * d = fr.in(src, count);
  if(!d) return fr.finish(); // (the staging failed)
  conv(d, dst, (int64_t)count);
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

extern "C" int smplpp_ik_set_tasks(smplpp_ik * s, const int64_t * face_idx, const float * vertex_weights, const float * target_pos,
                                   const float * target_normal, const double * pos_task_weight, const double * normal_task_weight,
                                   const double * phi_limit, const double * normal_offset, int space)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_tasks: null solver");
  int rc = check_space(space, "smplpp_ik_set_tasks");
  if(rc) return rc;
  const size_t nk = (size_t)s->n * s->K;
  if(face_idx && space == SMPLPP_HOST && (rc = ids_in("smplpp_ik_set_tasks", "face index", face_idx, (int64_t)nk, 0, s->m->F))) return rc;
  static_assert(ARENA_SLOTS >= 8, "smplpp_ik_set_tasks stages one slot per array given: up to 8");
  Frame fr(s->m->device, &s->arena, space, nullptr, nullptr);
  auto g = [](int64_t c) { return dim3((unsigned)((c + 255) / 256)); };
  auto cpf = [](const float * a, float * b, int64_t c) { (void)hipMemcpy(b, a, sizeof(float) * c, hipMemcpyDeviceToDevice); };
  auto cvd = [&](const double * a, float * b, int64_t c) { f64_to_f32_kernel<<<g(c), 256>>>(a, b, c); };
  auto cvi = [&](const int64_t * a, int32_t * b, int64_t c) { i64_to_i32_kernel<<<g(c), 256>>>(a, b, c); };
  // bit 2 of the status word (a normal term on a vertex beyond MAXADJ faces) belongs to the tasks the evaluation met: new faces,
  // weights or normal terms start clean, and the next evaluation raises it again where it still applies
  if(face_idx || normal_task_weight || normal_offset || vertex_weights)
  {
    clear_bits_kernel<<<g((int64_t)s->n), 256>>>(s->sticky, 4, (int64_t)s->n);
    HIP_TRY(hipGetLastError());
  }
  if((rc = set_array(fr, face_idx, s->ta.face, nk, cvi))) return rc;
  if((rc = set_array(fr, vertex_weights, s->ta.vw, nk * 3, cpf))) return rc;
  if((rc = set_array(fr, target_pos, s->ta.tpos, nk * 3, cpf))) return rc;
  if((rc = set_array(fr, target_normal, s->ta.tnrm, nk * 3, cpf))) return rc;
  if((rc = set_array(fr, pos_task_weight, s->ta.posw, nk, cvd))) return rc;
  if((rc = set_array(fr, normal_task_weight, s->ta.nrmw, nk, cvd))) return rc;
  if((rc = set_array(fr, phi_limit, s->ta.philim, nk, cvd))) return rc;
  if((rc = set_array(fr, normal_offset, s->ta.noff, nk, cvd))) return rc;
  if(phi_limit)
  {
    // the one synchronisation of the call: uploads, conversions and copies above run on the null stream in program order, each
    // staged array in a slot of its own, so nothing in front of this read-back needed one
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> h(nk);
    HIP_TRY(hipMemcpy(h.data(), s->ta.philim, sizeof(float) * nk, hipMemcpyDeviceToHost));
    bool locked = true;
    for(size_t i = 0; i < nk && locked; i++) locked = !(h[i] > 0.0f);
    s->phi_locked = locked;
  }
  return fr.finish();
}

extern "C" int smplpp_ik_set_config(smplpp_ik * s, const float * beta, const float * theta, int space)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_set_config: null solver");
  int rc = check_space(space, "smplpp_ik_set_config");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, nullptr, nullptr);
  fr.store(s->beta, beta, (size_t)s->n * NB);
  fr.store(s->theta, theta, (size_t)s->n * s->theta_dim);
  return fr.run([&]() -> int {
    // status bit 1 (smplpp_ik_get_status) reports failures "since the configuration was set": a new configuration starts clean
    s->jac_ahead = false; // (a Jacobian made ahead belongs to the configuration it was made for)
    HIP_TRY(hipMemset(s->status, 0, sizeof(int) * s->n));
    HIP_TRY(hipMemset(s->sticky, 0, sizeof(int) * s->n));
    if(s->range_word) HIP_TRY(hipMemset(s->range_word, 0, sizeof(int))); // (status bit 3: same lifetime; this solver's own word)
    if(theta && s->vp) // latent layout: the entries that pass through to theta25 (the decoder fills the rest at every evaluation)
    {
      ik_splice_kernel<<<dim3((unsigned)((s->n * 75 + 255) / 256)), 256>>>(s->theta, nullptr, s->theta25, s->n);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return SMPLPP_OK;
  });
}

extern "C" int smplpp_ik_get_config(smplpp_ik * s, float * beta, float * theta, int space)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_get_config: null solver");
  int rc = check_space(space, "smplpp_ik_get_config");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, nullptr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  fr.fetch(beta, s->beta, (size_t)s->n * NB);
  fr.fetch(theta, s->theta, (size_t)s->n * s->theta_dim);
  return fr.finish();
}

extern "C" int smplpp_ik_get_tasks(smplpp_ik * s, int64_t * face_idx, float * vertex_weights, float * tangents, float * actual_pos,
                                   float * actual_normal, int space)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_get_tasks: null solver");
  int rc = check_space(space, "smplpp_ik_get_tasks");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, nullptr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  const size_t nk = (size_t)s->n * s->K;
  int64_t * fo = fr.out(face_idx, nk);
  return fr.run([&]() -> int { // (kernels and copies: the null stream, in program order)
    if(fo) i32_to_i64_kernel<<<dim3((unsigned)((nk + 255) / 256)), 256>>>(s->ta.face, fo, (int64_t)nk);
    // IkTask::calcActualNormal() evaluated on demand at the current task state (face, weights) and the last posed mesh
    if(actual_normal)
      ik_actual_normals_kernel<<<dim3((unsigned)((nk + 63) / 64)), 64>>>(view_of(s->m), s->ta, s->verts, (int)s->K, (int64_t)nk);
    HIP_TRY(hipGetLastError());
    fr.fetch(vertex_weights, s->ta.vw, nk * 3);
    fr.fetch(tangents, s->ta.tang, nk * 6);
    fr.fetch(actual_pos, s->ta.apos, nk * 3);
    fr.fetch(actual_normal, s->ta.anrm, nk * 3);
    return SMPLPP_OK;
  });
}

static int ik_join(smplpp_ik * s, hipStream_t st)
{
  if(s->side_pending) // everything the caller does next on its stream is ordered behind the last re-projection
  {
    if(s->use_flags)
      HIP_TRY(hipStreamWaitValue32(st, s->sig + 32, s->tick_join, hipStreamWaitValueGte, 0xffffffffu));
    else
      HIP_TRY(hipStreamWaitEvent(st, s->ev_join, 0));
    s->side_pending = false;
  }
  return SMPLPP_OK;
}

// The instantiations of ik_eval_kernel, by tree depth (deep: more than 9 levels; see EvalPlan) and by the width of the adjacency
// tables (wide: a topology with a vertex of 13..16 faces: 16-face tables, fewer normal tasks per group): kernel, dynamic LDS, launch
struct EvalCall
{
  const float * th25;
  int optimize_beta, phi_live, min_valid, tsplit;
  size_t shmem;
  hipStream_t st;
  hipEvent_t done;
};
template<int DM, int RC, int NG, int MA>
static void eval_launch(smplpp_ik * s, const EvalCall & c)
{
  smplpp_model * m = s->m;
  hipExtLaunchKernelGGL((ik_eval_kernel<DM, RC, NG, MA>), dim3((unsigned)(s->n * c.tsplit)), dim3(EVAL_NT), c.shmem, c.st, nullptr, c.done, 0,
                        view_of(m), s->ta, c.th25, (const float *)s->verts, (const float *)s->rest, (const float *)m->ws.Gp.as<float>(),
                        (const float *)s->joints, (const float *)s->poserot, (int)s->K, c.optimize_beta, c.phi_live, c.min_valid, s->pts, s->e,
                        s->J, s->skip, s->dbg_stop, c.tsplit, s->roles, s->vp ? (const float *)s->vjac : (const float *)nullptr,
                        s->vp ? s->Jl : (double *)nullptr);
}
struct EvalForm
{
  const void * kfn;
  size_t lds;
  void (*launch)(smplpp_ik *, const EvalCall &);
};
template<int DM, int RC, int NG, int MA>
static EvalForm eval_form()
{
  return {reinterpret_cast<const void *>(&ik_eval_kernel<DM, RC, NG, MA>), sizeof(float) * EvalPlan<DM, RC, NG>::L_END + L_ANC_BYTES,
          &eval_launch<DM, RC, NG, MA>};
}

// forward + eval for all frames (enqueue only)
static int ik_forward_eval(smplpp_ik * s, int optimize_beta, int phi_live, int64_t min_valid, hipStream_t st, hipEvent_t eval_done = nullptr)
{
  smplpp_model * m = s->m;
  const int64_t n = s->n;
  const int K = (int)s->K;
  const float * th25 = s->theta;
  // latent_split: this configuration's decoder Jacobian is being made on the side stream (smplpp_ik::jac_ahead) — here only the value
  const bool jac_elsewhere = s->vp && s->jac_ahead;
  {
    TraceRange tr_fwd("forward SMPL"); // node.cpp:752-781 (the VPoser splice is inside that span there too)
    if(s->vp && s->exact) // node.cpp:761-772 in the reference's arithmetic: exact-fp32 value and Jacobian
    {
      int rc = vposer_jacobian_device(s->vp, s->jxw, n, s->theta + 6, TD44, s->theta25 + 6, 75, s->vjac, st);
      if(rc) return rc;
      th25 = s->theta25;
    }
    else if(s->vp) // node.cpp:761-772
    {
      // the decoder writes its 63 angles straight into theta25[:, 6:69]; the pass-through entries (root translation / rotation,
      // joints 22-23) are kept current by whoever changes the configuration: smplpp_ik_set_config and the solve kernel's update
      int rc = jac_elsewhere ? vposer_forward_device(s->vp, n, s->theta + 6, TD44, s->theta25 + 6, 75, nullptr, st, s->frame_base, true)
                             : vposer_forward_device(s->vp, n, s->theta + 6, TD44, s->theta25 + 6, 75, s->vjac, st, s->frame_base);
      if(rc) return rc;
      th25 = s->theta25;
    }
    s->vcur ^= 1;
    s->verts = s->vbuf[s->vcur];
    int rc = fk_device(m, n, s->beta, th25, s->verts, s->joints, nullptr, s->rest, s->poserot, st, RANGE_INTERNAL, s->range_word,
                       s->exact ? m->form : 0); // node.cpp:777
    if(rc) return rc;
  }
  TraceRange tr_eval("calculate IK matrices"); // node.cpp:796-881
  // the previous iteration's re-projection (side stream) wrote the faces / weights read from here on
  if(int rc = ik_join(s, st)) return rc;
  s->jac_ahead = false; // (consumed by the evaluation below: the join above covers the Jacobian kernel, which raised it)
  const bool deep = m->nlev > 9, wide = m->madj > MAXADJ;
  static const EvalForm forms[4] = {eval_form<DMAX, 64, 3, MAXADJ_WIDE>(), eval_form<DMAX, 64, 3, MAXADJ>(), eval_form<9, 76, 4, MAXADJ_WIDE>(),
                                    eval_form<9, 76, 6, MAXADJ>()};
  static PerDeviceOnce once_eval[4];
  const int fi = (deep ? 0 : 2) + (wide ? 0 : 1);
  HIP_TRY(lds_opt_in(once_eval[fi], m->device, forms[fi].kfn, (int)forms[fi].lds));
  const int tsplit = frame_split(n, K); // (a CU's LDS is one evaluation workgroup's)
  if(s->use_flags) eval_done = nullptr; // (flags mode: the fork is the solve kernel's start flag; the evaluation's end is signalled in events mode only)
  forms[fi].launch(s, {th25, optimize_beta, phi_live, (int)min_valid, tsplit, forms[fi].lds, st, eval_done});
  HIP_TRY(hipGetLastError());
  s->have_eval = true;
  return SMPLPP_OK;
}

// The per-frame words of the solve kernel (status: the last solve's outcome; sticky: bit 0 some solve failed, bit 2 raised by the
// evaluation, see TaskArrays::flags), read once; the caller's stream is idle
struct StatusWords
{
  std::vector<int> status, sticky;
};

static int ik_read_status(smplpp_ik * s, StatusWords & w)
{
  w.status.resize((size_t)s->n);
  w.sticky.resize((size_t)s->n);
  HIP_TRY(hipMemcpy(w.status.data(), s->status, sizeof(int) * s->n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(w.sticky.data(), s->sticky, sizeof(int) * s->n, hipMemcpyDeviceToHost));
  return SMPLPP_OK;
}

// what a host-space call reports: the valence condition first (such a frame's solve reports itself as skipped too), then a failed
// solve in `llt` (w.status: the last solve; w.sticky: any solve of the sequence; null: the call solved nothing)
static int ik_first_error(const StatusWords & w, const std::vector<int> * llt)
{
  for(int f : w.sticky)
    if(f & 4)
      return fail(SMPLPP_ERR_INVALID, "a task with a normal term (normal weight or normal offset) touches a vertex with more than 12 adjacent "
                                      "faces: the Jacobian of such a term is not supported");
  if(llt)
    for(int f : *llt)
      if(f & 1) return fail(SMPLPP_ERR_NUMERIC, "LLT has numerical issue!"); // node.cpp:934-937
  return SMPLPP_OK;
}

static int ik_report(smplpp_ik * s, int space, std::vector<int> StatusWords::*llt)
{
  if(space != SMPLPP_HOST) return SMPLPP_OK;
  StatusWords w;
  if(int rc = ik_read_status(s, w)) return rc;
  return ik_first_error(w, llt ? &(w.*llt) : nullptr);
}

extern "C" int smplpp_ik_eval(smplpp_ik * s, int optimize_beta, double * e, double * J, int space, void * stream)
{
  if(!s) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_eval: null solver");
  int rc = check_space(space, "smplpp_ik_eval");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  rc = fr.run([&]() -> int {
    if(int rc = ik_forward_eval(s, optimize_beta, 1, 0, fr.st)) return rc;
    const size_t rows = (size_t)s->n * s->K * 4, D = s->theta_dim + 2 * s->K + (optimize_beta ? NB : 0);
    fr.fetch(e, s->e, rows);
    fr.fetch(J, s->vp ? s->Jl : s->J, rows * D);
    return SMPLPP_OK;
  });
  return rc ? rc : ik_report(s, space, nullptr);
}

// What the sequence driver wants done around the LAST of the iterations: the configuration after it recorded (by the solve
// kernel itself) and the NEXT frame's targets put in place (by the re-projection's finish kernel, wherever it runs: the
// evaluation that read the old targets is over by then, nothing else reads them, and the next evaluation waits for it).
struct SeqHook
{
  float * theta_record = nullptr;        // [n][theta_dim]
  const float * next_tpos = nullptr;     // [n][K][3]
  const uint8_t * next_valid = nullptr;  // [n][K]
  int shared = 0;                        // next_tpos / next_valid are [K] / [K][3]: one capture for every chain
};

// ---- one iteration's launches behind the evaluation.  Each kernel's instantiations are named once, in a table or a chain of tests;
// which one runs, with how much LDS, is the plan's (ik_plan.h)
struct SolveCall
{
  SolvePlan p;
  SidePlan sp;
  int beta_dim, phi_live;
  float * theta_record; // the sequence driver's record of the configuration after this solve, or null
  hipStream_t st;
};
template<bool DUAL_ONLY, int NTR>
static void solve_launch(smplpp_ik * s, const SolveCall & c)
{
  const SolvePlan & p = c.p;
  const bool go = c.sp.go, ahead = c.sp.ahead;
  ik_solve_kernel<DUAL_ONLY, NTR><<<dim3((unsigned)s->n), dim3(256), p.shmem, c.st>>>(
      s->ta, s->e, s->vp ? s->Jl : s->J, s->theta, s->beta, c.sp.beside ? nullptr : s->pts, (int)s->K, s->theta_dim, c.beta_dim, c.phi_live, p.qp_k,
      s->vp ? 1 : 0, p.chunk_rows, s->skip, s->e2, s->status, s->sticky, s->xout, s->dbg_stop, p.m_dim, s->vp ? s->theta25 : (float *)nullptr,
      c.theta_record, go ? s->sig : (unsigned *)nullptr, go ? s->sig + 16 : (unsigned *)nullptr, s->tick_fork,
      ahead ? s->sig + 64 : (unsigned *)nullptr, ahead ? s->sig + 80 : (unsigned *)nullptr, s->tick_done);
}
struct SolveForm
{
  bool dual_only;
  int ntr;
  const void * kfn;
  void (*launch)(smplpp_ik *, const SolveCall &);
};
template<bool DUAL_ONLY, int NTR>
static SolveForm solve_form()
{
  return {DUAL_ONLY, NTR, reinterpret_cast<const void *>(&ik_solve_kernel<DUAL_ONLY, NTR>), &solve_launch<DUAL_ONLY, NTR>};
}
constexpr int SOLVE_FORMS = 5;
static const SolveForm * solve_forms()
{
  static const SolveForm forms[SOLVE_FORMS] = {solve_form<false, 6>(), solve_form<true, 6>(), solve_form<false, 11>(), solve_form<false, 5>(),
                                               solve_form<false, 3>()};
  return forms;
}

static int ik_enqueue_solve(smplpp_ik * s, const SolveCall & c)
{
  {
    TraceRange tr_solve("solve IK"); // node.cpp:907-943
    const SolveForm * f = solve_forms();
    while(f->dual_only != c.p.dual_only || f->ntr != c.p.ntr) f++; // (solve_plan's ntr is 3, 5, 6 or 11; 6 with dual_only)
    f->launch(s, c);
  }
  HIP_TRY(hipGetLastError());
  return SMPLPP_OK;
}

template<int KPR, int NBT>
static void scan_launch(smplpp_ik * s, int chunks, const float * qpts, const float * hint, hipStream_t pst)
{
  proj_scan_kernel<KPR, NBT><<<dim3((unsigned)(s->n * chunks)), dim3(256), 0, pst>>>(view_of(s->m), s->ta, s->verts, qpts, hint, s->m->F, (int)s->K, chunks,
                                                                                    s->skip, s->list_cnt, s->list_d, s->list_f, s->dbg_stop);
}

// scan + finish of iteration `it`, on the side stream when sp.beside; last: the sequence driver's hook on the last of its iterations
static int ik_enqueue_reproject(smplpp_ik * s, const SidePlan & sp, int it, const SeqHook * last, hipStream_t st)
{
  smplpp_model * m = s->m;
  const int K = (int)s->K;
  const bool dbg = s->dbg_sync, beside = sp.beside;
  TraceRange tr_proj("project point"); // node.cpp:974-988
  const float * qpts = beside ? s->ta.apos : s->pts;
  hipStream_t pst = st;
  if(beside)
  {
    if(s->use_flags)
      HIP_TRY(hipStreamWaitValue32(s->side, s->sig, s->tick_fork, hipStreamWaitValueGte, 0xffffffffu));
    else
      HIP_TRY(hipStreamWaitEvent(s->side, s->ev_fork, 0));
    pst = s->side;
  }
  const ScanPlan sc = scan_plan(s->n, K, m->F, s->scan_blocks, s->scan_form);
  const float * hint = beside ? s->ta.hint : nullptr; // the evaluation's distance is to the ACTUAL position
  if(sc.nbt3) scan_launch<0, 3>(s, sc.chunks, qpts, hint, pst);
  else if(sc.kpr == 0) scan_launch<0, CP_BATCH>(s, sc.chunks, qpts, hint, pst);
  else if(sc.kpr == 2) scan_launch<2, CP_BATCH>(s, sc.chunks, qpts, hint, pst);
  else scan_launch<4, CP_BATCH>(s, sc.chunks, qpts, hint, pst);
  HIP_TRY(hipGetLastError());
  int *& dbg_buf = s->dbg_buf; // (SMPLPP_DEBUG_SYNC only; owned by the solver, on its device)
  if(dbg && !dbg_buf) HIP_TRY(dalloc(s, dbg_buf, 8, AS_ALLOCATED)); // (zeroed on the stream below, every iteration)
  if(dbg) HIP_TRY(hipMemsetAsync(dbg_buf, 0, sizeof(int) * 8, st));
  const int fsplit = frame_split(s->n, K);
  if(sp.go) s->tick_join++;
  hipExtLaunchKernelGGL(proj_finish_kernel, dim3((unsigned)(s->n * fsplit)), dim3(256), 0, pst, nullptr,
                        (beside && !s->use_flags) ? s->ev_join : nullptr, 0,
                        view_of(m), s->ta, (const float *)s->verts, qpts, m->F, K, (const int *)s->skip, s->list_cnt, s->list_d,
                        s->list_f, dbg ? dbg_buf : (int *)nullptr, fsplit, sp.join_flag ? s->sig + 32 : (unsigned *)nullptr,
                        sp.join_flag ? s->sig + 48 : (unsigned *)nullptr, s->tick_join, last ? last->next_tpos : (const float *)nullptr,
                        last ? last->next_valid : (const uint8_t *)nullptr, last ? last->shared : 0);
  HIP_TRY(hipGetLastError());
  if(sp.ahead)
  {
    HIP_TRY(hipStreamWaitValue32(s->side, s->sig + 64, s->tick_done, hipStreamWaitValueGte, 0xffffffffu));
    int rc = vposer_forward_device(s->vp, s->n, s->theta + 6, TD44, nullptr, 75, s->vjac, s->side, s->frame_base, false, s->sig + 32,
                                   s->sig + 48, s->tick_join);
    if(rc) return rc;
    s->jac_ahead = true;
  }
  if(beside) s->side_pending = true;
  if(dbg)
  {
    int h[8];
    HIP_TRY(hipMemcpy(h, dbg_buf, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "[smplpp dbg] it %d: project lists: tasks %d, empty %d, overflow %d, nan %d, max cnt %d\n", it, h[0], h[1], h[2], h[3], h[4]);
  }
  return SMPLPP_OK;
}

// `iters` iterations enqueued on st (+ the solver's side stream); leaves the last re-projection pending on the side
// stream (s->side_pending) — the caller joins (ik_join) before anything else may touch the task arrays or the mesh.
// more_follows: the caller enqueues another iteration right behind this call's last one (the sequence driver, frame after frame)
static int ik_iterate_enqueue(smplpp_ik * s, int iters, int enable_qp, int optimize_beta_from, int64_t min_valid, hipStream_t st,
                              const SeqHook * hook = nullptr, bool more_follows = false)
{
  int rc = SMPLPP_OK;
  const int K = (int)s->K;
  static PerDeviceOnce once_solve[SOLVE_FORMS];
  for(int i = 0; i < SOLVE_FORMS; i++) HIP_TRY(lds_opt_in(once_solve[i], s->m->device, solve_forms()[i].kfn, (int)SOLVE_LDS_MAX));
  if(s->use_flags && (s->tick_fork > 0x7fff0000u || s->tick_join > 0x7fff0000u || s->tick_done > 0x7fff0000u))
  {
    // the hand-over flags carry iteration numbers compared with >=: start over long before they could wrap
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipStreamSynchronize(s->side));
    HIP_TRY(hipMemset(s->sig, 0, sizeof(unsigned) * 128));
    s->tick_fork = s->tick_join = s->tick_done = 0;
  }
  auto dbg_sync = [&](int it, const char * tag) -> int {
    if(!s->dbg_sync) return SMPLPP_OK;
    fprintf(stderr, "[smplpp dbg] it %d: %s ...\n", it, tag);
    HIP_TRY(hipStreamSynchronize(st));
    fprintf(stderr, "[smplpp dbg] it %d: %s done\n", it, tag);
    return SMPLPP_OK;
  };
  for(int it = 0; it < iters; it++)
  {
    // the plan (ik_plan.h) ...
    const IterFlags f = iter_flags(optimize_beta_from, it);
    const bool phi_free = f.phi_live && !s->phi_locked;
    const int beta_dim = f.opt_beta ? NB : 0;
    const SolvePlan p = solve_plan(K, s->theta_dim, beta_dim, phi_free, enable_qp != 0, s->dbg_stop == 9);
    const SidePlan sp = side_plan(s->overlap_ok, phi_free, s->use_flags, s->latent_split, f.opt_beta != 0, it + 1 < iters || more_follows);
    // ... the evaluation ...
    if((rc = ik_forward_eval(s, f.opt_beta, f.phi_live, min_valid, st, sp.beside ? s->ev_fork : nullptr))) return rc;
    if((rc = dbg_sync(it, "forward+eval"))) return rc;
    s->last_D = p.D;
    if(p.refusal) return fail(SMPLPP_ERR_INVALID, SOLVE_TOO_LARGE);
    // ... the solve: it raises the side stream's fork once all its workgroups run, and "configuration final" for a Jacobian made ahead ...
    const SeqHook * last = (hook && it == iters - 1) ? hook : nullptr;
    if(sp.go) s->tick_fork++;
    if(sp.ahead) s->tick_done++;
    if((rc = ik_enqueue_solve(s, {p, sp, beta_dim, f.phi_live, last ? last->theta_record : nullptr, st}))) return rc;
    if((rc = dbg_sync(it, "solve"))) return rc;
    // ... and the re-projection, beside the solve when no task's surface coordinates can move
    if((rc = ik_enqueue_reproject(s, sp, it, last, st))) return rc;
    if((rc = dbg_sync(it, "project"))) return rc;
  }
  return SMPLPP_OK;
}

extern "C" int smplpp_ik_iterate(smplpp_ik * s, int iters, int enable_qp, int optimize_beta_from, int64_t min_valid,
                                 double * e_sqnorm, int space, void * stream)
{
  if(!s || iters < 0) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_iterate: bad argument");
  int rc = check_space(space, "smplpp_ik_iterate");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  rc = fr.run([&]() -> int {
    const auto enq_t0 = std::chrono::steady_clock::now();
    const int rc = ik_iterate_enqueue(s, iters, enable_qp, optimize_beta_from, min_valid, fr.st);
    s->last_enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - enq_t0).count();
    const int jrc = ik_join(s, fr.st); // (after a failed enqueue too)
    if(rc || jrc) return rc ? rc : jrc;
    fr.fetch(e_sqnorm, s->e2, (size_t)s->n);
    return SMPLPP_OK;
  });
  return rc ? rc : ik_report(s, space, &StatusWords::status);
}

// node/node.cpp:1369-1407 with :681-700 — the frame loop of solveMocapMotion on the device: frame t's marker targets
// replace the task targets (a missing marker: target 0, weight 0), `warmup_iters` iterations on the first frame and
// `iters_per_frame` on every later one, warm-started; nothing returns to the host between frames.
__global__ void ik_seq_frame_kernel(const float * __restrict__ tpos_t, const uint8_t * __restrict__ valid_t, float * __restrict__ tpos,
                                    float * __restrict__ posw, int64_t nk, const float * __restrict__ theta, float * __restrict__ theta_prev_out,
                                    int64_t ntheta, int64_t shared_K)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if(tpos_t && i < nk)
  {
    const int64_t j = shared_K > 0 ? i % shared_K : i; // (shared_K: the targets are one capture's [K] for every chain)
    const bool v = valid_t[j] != 0;
    posw[i] = v ? 1.0f : 0.0f;
    for(int x = 0; x < 3; x++) tpos[i * 3 + x] = v ? tpos_t[j * 3 + x] : 0.0f;
  }
  if(theta_prev_out && i < ntheta) theta_prev_out[i] = theta[i];
}

// Development hook (not part of include/smplpp_hip.h): host microseconds the last smplpp_ik_solve_sequence / smplpp_ik_iterate spent enqueueing.
extern "C" int smplpp_debug_ik_enqueue_us(smplpp_ik * s, double * out)
{
  if(!s || !out) return fail(SMPLPP_ERR_INVALID, "smplpp_debug_ik_enqueue_us: bad argument");
  *out = s->last_enqueue_us;
  return SMPLPP_OK;
}

static int ik_solve_sequence_impl(smplpp_ik * s, int64_t T, const float * target_pos, const uint8_t * valid, bool shared, int warmup_iters,
                                  int iters_per_frame, int enable_qp, int64_t min_valid, float * theta_out, int space, void * stream)
{
  if(!s || T <= 0 || !target_pos || !valid || !theta_out || warmup_iters < 0 || iters_per_frame < 0)
    return fail(SMPLPP_ERR_INVALID, "smplpp_ik_solve_sequence: bad argument");
  int rc = check_space(space, "smplpp_ik_solve_sequence");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  hipStream_t st = fr.st;
  const int64_t nk = s->n * s->K, ntheta = s->n * s->theta_dim;
  const int64_t tk = shared ? s->K : nk; // targets per frame of the sequence as the caller holds them
  const float * tp = fr.in(target_pos, (size_t)(T * tk * 3));
  const uint8_t * vl = fr.in(valid, (size_t)(T * tk));
  float * th = fr.out(theta_out, (size_t)(T * ntheta));
  rc = fr.run([&]() -> int {
    HIP_TRY(hipMemsetAsync(s->sticky, 0, sizeof(int) * s->n, st));
    const int64_t cnt = nk > ntheta ? nk : ntheta;
    const dim3 grid((unsigned)((cnt + 255) / 256));
    // frame 0's targets go in here; every later switch and every frame's record ride on the iterations themselves (SeqHook): no
    // kernel of its own between one frame's solve and the next frame's pose step
    ik_seq_frame_kernel<<<grid, 256, 0, st>>>(tp, vl, s->ta.tpos, s->ta.posw, nk, nullptr, nullptr, 0, shared ? s->K : 0);
    HIP_TRY(hipGetLastError());
    const auto enq_t0 = std::chrono::steady_clock::now();
    int rc = SMPLPP_OK;
    for(int64_t t = 0; t < T; t++)
    {
      const int iters = t == 0 ? warmup_iters : iters_per_frame;
      SeqHook hook;
      hook.theta_record = th + t * ntheta;
      if(t + 1 < T)
      {
        hook.next_tpos = tp + (t + 1) * tk * 3;
        hook.next_valid = vl + (t + 1) * tk;
        hook.shared = shared ? 1 : 0;
      }
      if(iters > 0)
        rc = ik_iterate_enqueue(s, iters, enable_qp, -1, min_valid, st, &hook, /*more_follows=*/t + 1 < T && iters_per_frame > 0);
      else // (no iteration to carry the hook)
      {
        ik_seq_frame_kernel<<<grid, 256, 0, st>>>(hook.next_tpos, hook.next_valid, s->ta.tpos, s->ta.posw, nk, s->theta, hook.theta_record,
                                                  ntheta, shared ? s->K : 0);
        HIP_TRY(hipGetLastError());
      }
      if(rc) break;
    }
    const int jrc = ik_join(s, st);
    // (development figure, smplpp_debug_ik_enqueue_us: what the HOST spent handing the T frames' launches to the two streams — when
    // it approaches the frames' time on the GPU, the chains wait for the host)
    s->last_enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - enq_t0).count();
    return rc ? rc : jrc;
  });
  return rc ? rc : ik_report(s, space, &StatusWords::sticky);
}

extern "C" int smplpp_ik_solve_sequence(smplpp_ik * s, int64_t T, const float * target_pos, const uint8_t * valid, int warmup_iters,
                                        int iters_per_frame, int enable_qp, int64_t min_valid, float * theta_out, int space, void * stream)
{
  return ik_solve_sequence_impl(s, T, target_pos, valid, false, warmup_iters, iters_per_frame, enable_qp, min_valid, theta_out, space, stream);
}

// The same loop when every chain fits the SAME capture (the multi-restart fit: BASELINE configs[3], 64 restarts x one sequence):
// target_pos [T,K,3] and valid [T,K] once, handed to all n chains by the frame switch on the device — the caller neither builds nor
// uploads n copies (100 MB for 64 restarts of sample_walk.c3d; 83 ms of host work in front of 0.39 s of GPU work).
extern "C" int smplpp_ik_solve_sequence_shared(smplpp_ik * s, int64_t T, const float * target_pos, const uint8_t * valid, int warmup_iters,
                                               int iters_per_frame, int enable_qp, int64_t min_valid, float * theta_out, int space,
                                               void * stream)
{
  return ik_solve_sequence_impl(s, T, target_pos, valid, true, warmup_iters, iters_per_frame, enable_qp, min_valid, theta_out, space, stream);
}

// Per-frame outcome of the solves so far: flags[f] bit 0 = the last solve of frame f failed ("LLT has numerical issue!",
// node/node.cpp:934-937: the update of that frame was skipped), bit 1 = some solve since the last set_config /
// solve_sequence start failed, bit 2 = an evaluation since the tasks were last set (smplpp_ik_set_tasks clears it; so do set_config
// and solve_sequence) met a task with a normal term on a vertex of more than 12 adjacent faces: its Jacobian rows are not supported,
// and the solve skips that frame's update (bit 0 then reads 1 as for any skipped update).  SMPLPP_HOST calls of iterate / solve_sequence report the same condition as an error; a
// SMPLPP_DEVICE (enqueue-only) caller reads it here once its stream has reached the point of interest.  Bit 4 = the last solve of
// frame f was a box QP that used all its active-set passes without meeting its optimality test (the update was applied; no call
// reports it as an error).
extern "C" int smplpp_ik_get_status(smplpp_ik * s, int32_t * flags, int space, void * stream)
{
  if(!s || !flags) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_get_status: bad argument");
  int rc = check_space(space, "smplpp_ik_get_status");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  if(!fr.sync()) return fr.finish();
  StatusWords w;
  if((rc = ik_read_status(s, w))) return rc;
  const std::vector<int> &a = w.status, &b = w.sticky;
  // bit 3: a forward pass INSIDE this solver's loops met an operand outside the fp16x2 form's range since the last set_config
  // (one word per solver — which frame is not recorded, so every frame of the batch carries it; such a frame's vertices are not
  // finite and its solve then fails on its own)
  int internal = 0;
  if(s->range_word && s->m->form_ik == 'h') HIP_TRY(hipMemcpy(&internal, s->range_word, sizeof(int), hipMemcpyDeviceToHost));
  std::vector<int32_t> h((size_t)s->n);
  for(int64_t f = 0; f < s->n; f++)
    h[(size_t)f] = (a[(size_t)f] == 1 ? 1 : 0) | ((b[(size_t)f] & 1) ? 2 : 0) | (b[(size_t)f] & 4) | ((internal & 1) ? 8 : 0) |
                   (a[(size_t)f] == 2 ? 16 : 0); // bit 4: the box QP ran out of active-set passes (ik_solve_kernel's status 2)
  if(space == SMPLPP_HOST)
    memcpy(flags, h.data(), sizeof(int32_t) * (size_t)s->n);
  else
    HIP_TRY(hipMemcpy(flags, h.data(), sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice)); // (composed here, on the host)
  return fr.finish();
}

// The step x = (theta, phi, beta) of the last solve of every frame, fp64, as the solve kernel wrote it (xout, [n][last_D])
extern "C" int smplpp_ik_get_step(smplpp_ik * s, double * x, int64_t * D, int space, void * stream)
{
  if(!s || !D) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_get_step: bad argument");
  int rc = check_space(space, "smplpp_ik_get_step");
  if(rc) return rc;
  *D = s->last_D;
  if(!x || s->last_D == 0) return SMPLPP_OK;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  fr.fetch(x, s->xout, (size_t)(s->n * s->last_D));
  return fr.finish();
}

extern "C" int smplpp_ik_get_vertices(smplpp_ik * s, float * verts, int space, void * stream)
{
  if(!s || !verts) return fail(SMPLPP_ERR_INVALID, "smplpp_ik_get_vertices: bad argument");
  if(!s->have_eval) return fail(SMPLPP_ERR_STATE, "Failed to get vertices of new pose!");
  int rc = check_space(space, "smplpp_ik_get_vertices");
  if(rc) return rc;
  Frame fr(s->m->device, &s->arena, space, stream, nullptr);
  fr.fetch(verts, s->verts, (size_t)s->n * s->m->V * 3);
  return fr.finish();
}
