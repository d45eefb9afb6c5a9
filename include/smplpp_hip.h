/* smplpp_hip.h — C ABI of libsmplpp_hip.so, the MI355X (gfx950) engine behind the reference's smplpp::SMPL /
 * smplpp::IkTask API.  Plain pointers and sizes only; no torch / libtorch types.
 *
 * The reference has no FFI: its boundary is the C++ class API of libsmplpp.so
 * (/root/reference/include/smplpp/SMPL.h:241-269, include/smplpp/IkTask.h:20-84) and its one caller
 * node/node.cpp.  Each entry point below names the reference interface it stands in for; include/smplpp/SMPL.h and
 * include/smplpp/IkTask.h in this repository re-expose the reference's class names on top of it.
 *
 * Conventions
 *  - every function returns SMPLPP_OK (0) or an error code; smplpp_last_error() gives the message (thread-local).
 *    The C++ shim turns non-zero into `throw smplpp::Exception` to keep smpl_error semantics
 *    (include/smplpp/toolbox/Exception.h:48-49).
 *  - arrays are row-major with the reference's shapes.  `space` says where CALLER buffers live:
 *    SMPLPP_HOST (pageable/pinned host memory; the call stages and synchronises) or SMPLPP_DEVICE (HIP device
 *    memory on the model's device; the call only enqueues work on `stream` and returns).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - face ids are 0-based in this ABI (IkTask::faceIdx_ is 0-based; the model FILE is 1-based and is converted at
 *    create time like src/SMPL.cpp:520 does at every use).
 *  - one caller thread per handle (the reference is single-threaded, node/node.cpp:1414).
 *  - a handle keeps the staging of its largest host-space call (device copies of that call's arguments) until it is destroyed.
 */
#ifndef SMPLPP_HIP_H
#define SMPLPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPLPP_JOINT_NUM 24        /* include/smplpp/definition/def.h:10 */
#define SMPLPP_SHAPE_BASIS_DIM 10  /* def.h:11 */
#define SMPLPP_POSE_BASIS_DIM 207  /* def.h:12 */
#define SMPLPP_LATENT_DIM 32       /* def.h:14 */
#define SMPLPP_THETA_DIM 75        /* 3 * (JOINT_NUM + 1), node/node.cpp:787 */
#define SMPLPP_LATENT_POSE_DIM 44  /* LATENT_DIM + 12, node/node.cpp:42 */

enum
{
  SMPLPP_OK = 0,
  SMPLPP_ERR_INVALID = 1, /* bad shape / argument: the reference's smpl_error("...", "Cannot ...") cases */
  SMPLPP_ERR_HIP = 2,     /* HIP runtime failure, including "no GPU" */
  SMPLPP_ERR_NUMERIC = 3, /* "LLT has numerical issue!" node/node.cpp:934-937 */
  SMPLPP_ERR_STATE = 4    /* call order (e.g. a getter before any launch) */
};

enum
{
  SMPLPP_HOST = 0,
  SMPLPP_DEVICE = 1
};

typedef struct smplpp_model smplpp_model;   /* stands in for smplpp::SMPL            (SMPL.h:140-270) */
typedef struct smplpp_ik smplpp_ik;         /* the IK loop state of node/node.cpp:645-1002, batched over frames */
typedef struct smplpp_vposer smplpp_vposer; /* stands in for smplpp::VPoserDecoder   (VPoser.h:53-90) */
struct smplpp_landmarks;                    /* a sparse landmark regressor over a model's vertices and joints (no reference counterpart);
                                               written `struct smplpp_landmarks` throughout: the name alone is the regression call below */
struct smplpp_pose_prior;                   /* a max-mixture Gaussian pose prior with joint limits (no reference counterpart); written
                                               `struct smplpp_pose_prior` throughout, as above: the name alone is the evaluation call */
struct smplpp_lbfgs;                        /* a batched L-BFGS over n independent frames (no reference counterpart); written
                                               `struct smplpp_lbfgs` throughout, as the two above */
struct smplpp_sequence;                     /* the layout of sequences inside a grouped L-BFGS buffer (no reference counterpart); written
                                               `struct smplpp_sequence` throughout, as the three above */
struct smplpp_volume;                       /* a signed-distance grid of a static scene, resident on the device (no reference
                                               counterpart); written `struct smplpp_volume` throughout, as the four above */
struct smplpp_measure;                      /* regions of a model's faces and plane sections through them, for body measurements (no
                                               reference counterpart); written `struct smplpp_measure` throughout, as the five above */
struct smplpp_self_contact;                 /* the far relation of a model's rest mesh, for the self-contact search (no reference
                                               counterpart); written `struct smplpp_self_contact` throughout, as the six above */

const char * smplpp_last_error(void);
/* Number of HIP devices visible; SMPLPP_ERR_HIP (and *count = 0) when there is none. */
int smplpp_device_count(int * count);

/* ------------------------------------------------------------------ model: SMPL::setDevice/setModelPath/init */
/* Replaces SMPL::init (src/SMPL.cpp:560-643) minus the JSON parse, which stays on the host side: the seven arrays
 * of scripts/preprocess.py:98-117, host pointers.  vertex_num may differ from 6890 (the reference makes VERTEX_NUM
 * a variable, def.h:9).  Re-lays the blend bases out for the fused kernel, folds the joint regressor, builds the
 * adjacent-face table (:620-640). */
int smplpp_model_create(int64_t vertex_num, int64_t face_num, const float * vertices_template /*[V,3]*/,
                        const float * shape_blend_shapes /*[V,3,10]*/, const float * pose_blend_shapes /*[V,3,207]*/,
                        const float * joint_regressor /*[24,V]*/, const float * weights /*[V,24]*/,
                        const int64_t * kinematic_tree /*[2,24]*/, const int32_t * face_indices_1based /*[F,3]*/,
                        int device, smplpp_model ** out);
int smplpp_model_destroy(smplpp_model * m);
/* vertex_num, face_num, and the number of skinning weights kept per vertex (4, 8 or 24 = dense). */
int smplpp_model_info(const smplpp_model * m, int64_t * vertex_num, int64_t * face_num, int * weights_per_vertex,
                      int * device);

/* ------------------------------------------------------------------ FK: SMPL::launch + getters */
/* SMPL::launch(beta [n,10], theta [n,25,3]) (src/SMPL.cpp:671-737): theta[:,0,:] is the root translation,
 * theta[:,1:,:] the 24 axis-angles.  Any output may be NULL:
 *   verts  [n,V,3]      SMPL::getVertex          (:492-506)
 *   joints [n,24,3]     SMPL::getRestJoint       (:457-471)
 *   xforms [n,24,4,4]   WorldTransformation::getTransformation (relative transforms G')
 *   rest   [n,V,3]      SMPL::getRestShape
 * Two kernels: pose/chain, then the fused blend-shape GEMM + linear blend skinning.  The fused kernel computes in the reference's
 * arithmetic (every fp32 operand of the contraction carried exactly, as three bf16 pieces on the matrix pipe; fp32 accumulate; the
 * skinning in fp32 FMAs: src/BlendShape.cpp:762-765, src/LinearBlendSkinning.cpp:463-467).  SMPLPP_SKIN in the environment of
 * smplpp_model_create selects another form for every launch on the model: h (fp16x2 operand pieces, 22 bits, 3e-7 m: the form
 * the IK loops' internal forward passes use by default), b (round 1's bf16x3 kernel), v (fp32 MFMA). */
int smplpp_fk(smplpp_model * m, int64_t n, const float * beta, const float * theta, float * verts, float * joints,
              float * xforms, float * rest, int space, void * stream);
/* Vector-Jacobian product of smplpp_fk (the backward pass the reference gets from libtorch autograd through SMPL::launch, e.g.
 * node/node.cpp:823-869): given dL/dverts [n,V,3] and/or dL/djoints [n,24,3] (either may be NULL = zero), writes dL/dbeta [n,10]
 * and dL/dtheta [n,25,3] (row 0 = root translation; either output may be NULL).  rest [n,V,3]: the rest shape smplpp_fk returned for
 * these inputs; NULL = recomputed inside the call with the model's form, in the backward's own workspace (smplpp_fk's workspace,
 * status words and profiling record are left as they were).  Overwrites its outputs; deterministic (same inputs -> same bits).
 * The first call on a model builds the basis operand image of the backward (~19 MB for SMPL; freed by smplpp_model_destroy). */
int smplpp_fk_vjp(smplpp_model * m, int64_t n, const float * beta, const float * theta, const float * rest, const float * grad_verts,
                  const float * grad_joints, float * grad_beta, float * grad_theta, int space, void * stream);
/* smplpp_fk from rotation matrices (what smplx calls pose2rot=False): rot [n,24,3,3] row-major, joint 0 the root orientation (the
 * layout of a rotation-matrix or 6-D regressor's output); trans [n,3] the root translation (NULL = zero); beta [n,10] (NULL = zero).
 * With rot = smplpp_axis_angle_to_rotmat(theta[:,1:]) and trans = theta[:,0] every output has the bits of smplpp_fk(beta, theta).
 * The matrices are used AS GIVEN: no re-orthonormalisation and no determinant check, so the call is the polynomial map
 * rest = T + S beta + P vec(R_j - I, j >= 1), A_0 = R_0, A_j = A_parent(j) R_j.  Outputs, NULL handling, forms (SMPLPP_SKIN), the
 * range word of the fp16x2 form (there also: entries of R_j - I below 1023) and smplpp_fk_status: as smplpp_fk. */
int smplpp_fk_rotmat(smplpp_model * m, int64_t n, const float * beta /*[n,10], NULL = 0*/, const float * trans /*[n,3], NULL = 0*/,
                     const float * rot /*[n,24,3,3]*/, float * verts, float * joints, float * xforms, float * rest, int space, void * stream);
/* Vector-Jacobian product of smplpp_fk_rotmat: given dL/dverts [n,V,3] and/or dL/djoints [n,24,3] (either may be NULL = zero), writes
 * dL/dbeta [n,10], dL/dtrans [n,3] and dL/drot [n,24,3,3] (any may be NULL).  grad_rot is the gradient to NINE INDEPENDENT ENTRIES per
 * joint (the map above is polynomial in them): it is not projected onto the tangent space of the rotations and has no singularity at
 * rotation 0 or pi; a caller that parametrises R (6-D, quaternion, axis-angle) contracts it with that parametrisation's derivative.
 * trans is accepted for symmetry and not read (nothing here depends on it).  rest: as smplpp_fk_vjp (NULL = recomputed in the
 * backward's own workspace; pass rest + D for an SMPL+D body).  Overwrites its outputs; deterministic.  grad_beta and grad_trans have the
 * bits smplpp_fk_vjp gives for the same body: the two calls share everything but the last contraction. */
int smplpp_fk_rotmat_vjp(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot, const float * rest /*nullable*/,
                         const float * grad_verts, const float * grad_joints, float * grad_beta /*[n,10]*/, float * grad_trans /*[n,3]*/,
                         float * grad_rot /*[n,24,3,3]*/, int space, void * stream);
/* The skeleton alone: the kinematic chain without a vertex, and its backward pass (no reference counterpart: the reference returns the
 * rest joints, SMPL::getRestJoint, and keeps the world transforms inside WorldTransformation).  Outputs, any may be NULL but not all:
 *   world  [n,24,3,4]  row-major [A_j | posed_j]: the world orientation and position of joint j
 *   posed  [n,24,3]    the posed joints of the chain (what smplx returns as `joints`)
 *   joints [n,24,3]    the rest joints J, the `joints` of smplpp_fk
 * Forward rule, per frame: R_j = Rodrigues(theta[1+j]) as smplpp_fk computes it (rotmat entry: rot[j] used as given, as smplpp_fk_rotmat
 * does); J = J0 + JS.beta; A_0 = R_0, g_0 = J_0; A_j = A_p R_j, g_j = A_p (J_j - J_p) + g_p, one tree level at a time, with the
 * operations and operand order of smplpp_fk's pose step; posed_j = g_j + trans (one fp32 add), trans = theta[0] (rotmat entry: trans,
 * NULL = +0).  So world[..., :3] has the BITS of the 3x3 block of the xforms of smplpp_fk / smplpp_fk_rotmat on the same inputs, and
 * joints the bits of their joints.
 * Backward rule, per frame (the forward is recomputed, no state is kept; every operation is rounded on its own):
 *   seeds: dA_j = grad_world[j][:, :3], dg_j = grad_world[j][:, 3] + grad_posed[j], dJ_j = grad_joints[j]; a NULL cotangent reads as +0
 *   grad_trans = sum of the 24 seed dg_j in ascending j from +0
 *   from the deepest level to level 1, joint j with parent p: dR_j = A_p^T dA_j; cA_j = dA_j R_j^T + dg_j (J_j - J_p)^T;
 *     cJ_j = A_p^T dg_j, dJ_j += cJ_j; the parent then gathers its children in ascending joint order: dA_p += cA_i, dg_p += dg_i,
 *     dJ_p -= cJ_i
 *   root: dR_0 = dA_0, dJ_0 += dg_0
 *   grad_beta[k] = sum of JS[i][k] dJ[i] over i = 0..71 in ascending order from +0
 *   grad_theta[1+j][m] = sum_q dR_j[q] dRodrigues(theta_j)/dtheta_m [q] in ascending q (row 0 = grad_trans); rotmat entry: grad_rot = dR,
 *     NINE INDEPENDENT ENTRIES per joint (the convention of smplpp_fk_rotmat_vjp)
 * accumulate = 0 stores the finished value, 1 adds it to the output (one fp32 add): after smplpp_fk_vjp into the same buffers that is
 * the gradient of a loss on vertices AND skeleton.  At least one cotangent must be given and one gradient asked for.
 * One kernel launch per call on the caller's stream; a device-space call touches nothing in the handle (no workspace, no status word,
 * no profiling record).  A frame's bits depend on that frame's inputs only: not on n, its place in the batch, the memory space, or
 * which outputs or cotangents are asked for; a frame of NaNs leaves its neighbours alone.  Any tree smplpp_model_create accepts works.
 * SMPLPP_ERR_INVALID (outputs untouched): n <= 0, NULL theta or rot, nothing asked for, no cotangent, accumulate not 0 or 1. */
int smplpp_skeleton(smplpp_model * m, int64_t n, const float * beta /*[n,10], NULL = 0*/, const float * theta /*[n,25,3]*/,
                    float * world /*[n,24,3,4] nullable*/, float * posed /*[n,24,3] nullable*/, float * joints /*[n,24,3] nullable*/,
                    int space, void * stream);
int smplpp_skeleton_rotmat(smplpp_model * m, int64_t n, const float * beta /*nullable*/, const float * trans /*[n,3] nullable*/,
                           const float * rot /*[n,24,3,3]*/, float * world, float * posed, float * joints, int space, void * stream);
int smplpp_skeleton_vjp(smplpp_model * m, int64_t n, const float * beta, const float * theta, const float * grad_world /*[n,24,3,4] nullable*/,
                        const float * grad_posed /*[n,24,3] nullable*/, const float * grad_joints /*[n,24,3] nullable*/,
                        float * grad_beta /*[n,10] nullable*/, float * grad_theta /*[n,25,3] nullable*/, int accumulate, int space,
                        void * stream);
int smplpp_skeleton_rotmat_vjp(smplpp_model * m, int64_t n, const float * beta, const float * trans, const float * rot,
                               const float * grad_world, const float * grad_posed, const float * grad_joints, float * grad_beta,
                               float * grad_trans /*[n,3]*/, float * grad_rot /*[n,24,3,3]*/, int accumulate, int space, void * stream);
/* Jacobian-vector product (forward mode) of smplpp_fk and smplpp_skeleton (no reference counterpart: the reference differentiates in
 * reverse mode only): for T tangents per frame it returns how the vertices, the rest joints and the world joint frames change,
 *   dverts  [n,T,V,3]     tangent of smplpp_fk's verts
 *   djoints [n,T,24,3]    tangent of the rest joints (smplpp_fk's joints)
 *   dworld  [n,T,24,3,4]  tangent of smplpp_skeleton's world = [dA_j | dg_j + dtrans]
 * (any may be NULL, not all).  dbeta [tf,T,10] and dtheta [tf,T,25,3] (row 0 = the tangent of the root translation) are the tangents,
 * NULL = zero, not both; shared = 0: tf = n, one set of T tangents per frame; shared = 1: tf = 1, ONE set of T tangents applied to
 * every frame (the one-hot basis of a Jacobian, held once).  With dtheta = the pose rate the outputs are velocities.
 * Rule, per frame and tangent, with R, J, A, g, G'_j = [A_j | t_j = g_j - A_j J_j], rest and wSum_v = sum_j w_vj as smplpp_fk has them:
 *   dR_j = sum_m dtheta[1+j][m] dRodrigues(theta_j)/dtheta_m, the derivative smplpp_fk_vjp contracts with (finite at theta = 0 and at
 *     |theta| = pi);  dJ = JS dbeta;  drest_v = S_v dbeta + P_v vec(dR_j, j >= 1)
 *   dA_0 = dR_0, dg_0 = dJ_0; level by level, joint j with parent p: dA_j = dA_p R_j + A_p dR_j,
 *     dg_j = dA_p (J_j - J_p) + A_p (dJ_j - dJ_p) + dg_p;  dt_j = dg_j - dA_j J_j - A_j dJ_j
 *   dverts_v = ((sum_j w_vj dA_j) rest_v + sum_j w_vj dt_j + (sum_j w_vj A_j) drest_v) / wSum_v + dtrans
 * rest: as smplpp_fk_vjp (the rest shape the forward returned, rest + D for an SMPL+D body, NULL = recomputed with the model's form in
 * the backward's own workspace; smplpp_fk's workspace, status words and profiling record stay as they were); read for dverts only.
 * All tangent arithmetic is fp32 whatever SMPLPP_SKIN is: the drest contraction on v_mfma_f32_32x32x2_f32 (operands carried exactly),
 * everything else in fp32 FMAs.  No atomics; the outputs are overwritten; same inputs -> same bits.  The bits of a (frame, tangent)
 * depend on that frame's inputs and that tangent only: not on n, T, the place in the batch, `shared`, the memory space or which
 * outputs are asked for; a frame or tangent of NaNs leaves its neighbours alone.  Without dverts the call is one kernel launch that
 * touches nothing in the handle in device space, on any tree smplpp_model_create accepts; with dverts the first call on a model builds
 * the operand image smplpp_fk_vjp builds (shared with it).  n T <= 2^31 - 1; element offsets are 64-bit.
 * SMPLPP_ERR_INVALID (outputs untouched): n <= 0 or T <= 0, NULL beta or theta, every tangent NULL, no output asked for, shared not
 * 0 or 1. */
int smplpp_fk_jvp(smplpp_model * m, int64_t n, int64_t T, const float * beta /*[n,10]*/, const float * theta /*[n,25,3]*/,
                  const float * rest /*[n,V,3] nullable*/, const float * dbeta /*[tf,T,10] nullable = 0*/,
                  const float * dtheta /*[tf,T,25,3] nullable = 0*/, int shared /*0: tf = n, 1: tf = 1*/,
                  float * dverts /*[n,T,V,3] nullable*/, float * djoints /*[n,T,24,3] nullable*/,
                  float * dworld /*[n,T,24,3,4] nullable*/, int space, void * stream);
/* smplpp_fk_jvp for the rotation-matrix entry (smplpp_fk_rotmat / smplpp_skeleton_rotmat): the tangents are dbeta [tf,T,10], dtrans
 * [tf,T,3] and drot [tf,T,24,3,3], NINE INDEPENDENT ENTRIES per joint used as given (dR_j = drot[j]: the map is polynomial in them, no
 * projection onto the rotations), any NULL = zero, not all.  beta NULL = zero; trans is accepted for symmetry and not read (no tangent
 * depends on it).  With drot = sum_m dtheta_m dRodrigues/dtheta_m and dtrans = dtheta[0] it is smplpp_fk_jvp to rounding; with drot
 * NULL or zero and the same dbeta the two entries agree bit for bit on a body with rot = smplpp_axis_angle_to_rotmat(theta[:,1:]).
 * Everything else as smplpp_fk_jvp; SMPLPP_ERR_INVALID also for NULL rot. */
int smplpp_fk_rotmat_jvp(smplpp_model * m, int64_t n, int64_t T, const float * beta /*nullable*/, const float * trans /*nullable*/,
                         const float * rot /*[n,24,3,3]*/, const float * rest /*nullable*/, const float * dbeta /*nullable*/,
                         const float * dtrans /*[tf,T,3] nullable*/, const float * drot /*[tf,T,24,3,3] nullable*/, int shared,
                         float * dverts, float * djoints, float * dworld, int space, void * stream);
/* Input range of the fp16x2 form (SMPLPP_SKIN=h): |beta| < 1023 and relative transforms whose
 * translations stay within 16 x the template's extent (65504 / sG).  Outside it the operand pieces overflow fp16 and the
 * vertices of the frame are not finite, where the reference and the default form (and SMPLPP_SKIN=b|v) stay finite.  A launch that
 * meets such an operand sets bit 0 of the model's status word: a host-space smplpp_fk returns SMPLPP_ERR_NUMERIC itself;
 * an enqueue-only (device-space) caller reads it here — the call synchronises `stream`, returns the word and clears it. */
int smplpp_fk_status(smplpp_model * m, int * bits, void * stream);

/* Measurement hook (bench.py): while enabled, every launch of the fused blend-shape + skinning kernel is bracketed by
 * HIP events on the stream it is launched on; smplpp_profile_read waits for them, returns the number of launches
 * and the mean kernel duration in milliseconds since the last read, and clears the record. */
int smplpp_profile_enable(smplpp_model * m, int enable);
int smplpp_profile_read(smplpp_model * m, int64_t * launches, double * mean_skin_kernel_ms);

/* Stage-level entry points with the reference's stage semantics on arbitrary inputs (the Tester.cpp KATs feed
 * non-rotation matrices and 4x4 transforms with a non-trivial last row).  Host or device pointers.
 *   BlendShape::blend            src/BlendShape.cpp:620-647     JointRegression::regress   src/JointRegression.cpp:507-532
 *   WorldTransformation::transform  src/WorldTransformation.cpp:421-468
 *   LinearBlendSkinning::skinning   src/LinearBlendSkinning.cpp:445-483 (root_pos may be NULL) */
int smplpp_stage_blend_shape(int device, int64_t vertex_num, int64_t n, const float * beta, const float * theta24,
                             const float * shape_basis, const float * pose_basis, float * shape_blend, float * pose_blend,
                             float * pose_rot, int space, void * stream);
int smplpp_stage_joint_regression(int device, int64_t vertex_num, int64_t n, const float * template_shape,
                                  const float * joint_regressor, const float * shape_blend, const float * pose_blend,
                                  float * rest_shape, float * joints, int space, void * stream);
int smplpp_stage_world_transformation(int device, int64_t n, const int64_t * kinematic_tree, const float * joints,
                                      const float * pose_rot, float * xforms, int space, void * stream);
int smplpp_stage_skinning(int device, int64_t vertex_num, int64_t n, const float * weights, const float * rest_shape,
                          const float * xforms, const float * root_pos, float * verts, int space, void * stream);

/* ------------------------------------------------------------------ mesh queries on posed vertices */
/* SMPL::calcNormal (src/SMPL.cpp:518-525) and SMPL::calcVertexNormal (:527-535) for lists of ids, on frame-major
 * vertices [n,V,3]; outputs [n,count,3].  Adjacent faces are summed in ascending face id. */
int smplpp_face_normals(smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * face_ids,
                        float * normals, int space, void * stream);
int smplpp_vertex_normals(smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * vertex_ids,
                          float * normals, int space, void * stream);
/* igl::point_mesh_squared_distance as called at node/node.cpp:982: for each of n frames, K query points against that
 * frame's posed mesh.  face [n,K] (0-based), closest [n,K,3], sqdist [n,K] (nullable). */
int smplpp_closest_points(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                          int64_t * face, float * closest, float * sqdist, int space, void * stream);
/* SMPL::calcVertexNormal (src/SMPL.cpp:527-535) for EVERY vertex of every frame: normals [n,V,3]. */
int smplpp_mesh_vertex_normals(smplpp_model * m, int64_t n, const float * verts, float * normals, int space, void * stream);
/* Vector-Jacobian products of the three normal queries above (the backward pass libtorch autograd runs through
 * SMPL::calcNormal / calcVertexNormal in the reference's IK residual, node/node.cpp:803-869): grad_verts [n,V,3] for
 * dL/dnormals = grad_normals ([n,count,3] for the list forms, [n,V,3] for the whole mesh), at `verts`.
 *  - what is differentiated: exactly the forward the matching call computes (cross3 / normalize3, weights 1/deg, adjacent
 *    faces in ascending face id, torch's normalize x / max(|x|, 1e-12)).  A face enters a vertex's sum once, even when the
 *    vertex is repeated in it.
 *  - where a face's cross product or a vertex's weighted sum is shorter than 1e-12, the product is torch's gradient of that
 *    branch, g / 1e-12 (finite, not NaN).  A vertex without faces gets zero.
 *  - accumulate = 0: grad_verts is overwritten; vertices the query does not touch get 0.  accumulate = 1: the product is
 *    added into grad_verts (so normal and position terms can share one buffer for smplpp_fk_vjp).
 *  - an id list may repeat ids: their cotangents sum.
 *  - deterministic: no floating-point atomics; each element is one fixed-order sum (a vertex's adjacent faces in ascending
 *    face id for the whole mesh, list order for the list forms), so a frame's bits do not depend on n or on its position
 *    in the batch.  No bound on a vertex's valence, and no status bit.
 *  - the list forms touch only the vertices of the faces involved (with accumulate = 0 they also zero the rest).
 *  - SMPLPP_ERR_INVALID: bad arguments, host-space ids out of range (device-space ids are not read on the host, like the
 *    forward; an id out of range there contributes nothing), a model without faces.  SMPLPP_ERR_HIP without a GPU. */
int smplpp_face_normals_vjp(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t count, const int64_t * face_ids,
                            const float * grad_normals /*[n,count,3]*/, float * grad_verts /*[n,V,3]*/, int accumulate, int space,
                            void * stream);
int smplpp_vertex_normals_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t count, const int64_t * vertex_ids,
                              const float * grad_normals /*[n,count,3]*/, float * grad_verts, int accumulate, int space, void * stream);
int smplpp_mesh_vertex_normals_vjp(smplpp_model * m, int64_t n, const float * verts, const float * grad_normals /*[n,V,3]*/,
                                   float * grad_verts, int accumulate, int space, void * stream);
/* Point-to-mesh distance for many query points per frame (fitting to a point cloud or scan): for each of n frames, the
 * closest face of that frame's posed mesh verts [n,V,3] to each of K points [n,K,3].
 *  - face [n,K], closest [n,K,3] and sqdist [n,K] have the bits smplpp_closest_points gives on the same inputs (the same
 *    rule: the lowest face id with d <= mn (1 + 1e-6) + 1e-12, every distance from the same point-triangle evaluation).
 *  - weights [n,K,3]: the vertex weights of the closest point, from the branch of the point-triangle evaluation that produced
 *    it: one-hot at a vertex, (1-v, v, 0) / (1-w, 0, w) / (0, 1-w, w) on edge ab / ac / bc, (1-v-w, v, w) inside.  They sum
 *    to 1 and sum_j w_j v_j is `closest` up to rounding (at a region boundary a weight may round to a few ulps below 0).  (Not the IK tasks' area-ratio weights of an arbitrary position.)
 *  - form: a tiled scan (64 queries per workgroup, Morton-ordered within the frame, triangles through LDS) when the call has
 *    n * K >= 8192 queries, one workgroup per query below; SMPLPP_POINT_DISTANCE_FORM = query | tiled, read at model creation,
 *    forces one.  Every form returns the same bits.
 *  - weights and closest are nullable; face and sqdist are not.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, n * K beyond int32 indexing. */
int smplpp_point_mesh_distance(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t K, const float * points /*[n,K,3]*/,
                               int64_t * face /*[n,K]*/, float * weights /*[n,K,3] nullable*/, float * closest /*[n,K,3] nullable*/,
                               float * sqdist /*[n,K]*/, int space, void * stream);
/* Vector-Jacobian product of sqdist above: grad_verts [n,V,3] and grad_points [n,K,3] for dL/dsqdist = grad_sqdist [n,K], at
 * the faces `face` [n,K] the forward chose.  The point c and weights w are recomputed from (verts, points, face) with the
 * forward's evaluation (no new search); with r = p - c and g = grad_sqdist:
 *    grad_points[k] = 2 g_k r_k,    grad_verts[u] = sum over (k, corner j) with faces[face_k][j] == u of -2 g_k w_kj r_k.
 *  - exact in every region (envelope theorem); where tied faces share the closest point, they give the same gradient.
 *  - accumulate = 0: both outputs are overwritten (vertices no query touches get 0); accumulate = 1: the product is added
 *    (so the distance term can share one buffer with normal and position terms on its way to smplpp_fk_vjp).  Either output
 *    may be NULL, not both.
 *  - a query whose cotangent is exactly 0 contributes nothing, even if its point is NaN (padded rows of ragged scans).
 *  - deterministic: no floating-point atomics; each element of grad_verts is one fixed-order sum in ascending k, then corner
 *    j, so a frame's bits do not depend on n or on its position in the batch.  No cap on the records one vertex receives.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, n * K beyond int32 indexing, host-space face ids out of
 *    range (a device-space face id out of range contributes nothing). */
int smplpp_point_mesh_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                   const int64_t * face /*[n,K]*/, const float * grad_sqdist /*[n,K]*/,
                                   float * grad_verts /*[n,V,3] nullable*/, float * grad_points /*[n,K,3] nullable*/,
                                   int accumulate, int space, void * stream);
/* Mesh-to-point distance, the other direction of a two-sided scan registration (Chamfer) loss: for each of n frames, the nearest
 * of K points [n,K,3] to each vertex of that frame's posed mesh verts [n,V,3].  A brute-force scan; faces are not used, so a
 * model created without faces is accepted.  Exact rule (a float32 restatement reproduces every bit):
 *  - sqdist[f,v] is the fp32 value of ((dx*dx + dy*dy) + dz*dz), d = v - p, every operation rounded on its own (no FMA);
 *  - index[f,v] is the point with the smallest such distance; on equal distances the lowest point index wins;
 *  - a pair whose distance is not finite (NaN, inf, fp32 overflow of huge coordinates) is never chosen; a vertex with no
 *    eligible point (a frame of NaN padding) gets index = -1 and sqdist = 0;
 *  - the bits do not depend on n, on the frame's position in the batch, or on how the call splits K: few frames split K into
 *    chunks (chosen from n and K alone), each with a partial (d, k), then a lexicographic (d, k) minimum over the chunks.
 *  - SMPLPP_ERR_INVALID: bad arguments, n * K or n * V beyond int32 indexing. */
int smplpp_mesh_point_distance(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t K, const float * points /*[n,K,3]*/,
                               int64_t * index /*[n,V]*/, float * sqdist /*[n,V]*/, int space, void * stream);
/* Vector-Jacobian product of sqdist above: grad_verts [n,V,3] and grad_points [n,K,3] for dL/dsqdist = grad_sqdist [n,V], at
 * the points `index` [n,V] the forward chose.  With r = v - p[index] and g = grad_sqdist:
 *    grad_verts[v] = 2 g_v r_v,    grad_points[k] = sum over the vertices v with index_v == k of -2 g_v r_v.
 *  - accumulate = 0: both outputs are overwritten (points no vertex chose get 0); accumulate = 1: the product is added.  Either
 *    output may be NULL, not both.
 *  - a vertex with index = -1, or with a cotangent of exactly 0, contributes nothing (masking vertices, e.g. back-facing ones for
 *    a single-view depth cloud, is done with zero cotangents).
 *  - deterministic: no floating-point atomics; each element of grad_points is one fixed-order sum in ascending v, so a frame's
 *    bits do not depend on n or on its position in the batch.  No cap on how many vertices one point receives.
 *  - SMPLPP_ERR_INVALID: bad arguments, n * K or n * V beyond int32 indexing, a host-space index outside [-1, K) (the outputs are
 *    left untouched); a device-space index out of range contributes nothing. */
int smplpp_mesh_point_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                   const int64_t * index /*[n,V]*/, const float * grad_sqdist /*[n,V]*/,
                                   float * grad_verts /*[n,V,3] nullable*/, float * grad_points /*[n,K,3] nullable*/,
                                   int accumulate, int space, void * stream);
/* Normal-compatible, distance-capped scan correspondences: smplpp_point_mesh_distance and smplpp_mesh_point_distance with the two
 * filters of every registration pipeline INSIDE the search (a filter after the search loses the point: the right face was never
 * found).  The rule, stated once; a float32 numpy restatement reproduces every bit:
 *  - compatibility of two normals m, q (neither is normalised by the library): s = (m.x q.x + m.y q.y) + m.z q.z, and mm, qq
 *    formed the same way from (m, m) and (q, q); compatible iff  s >= 0  &&  mm*qq > 0  &&  s*s >= (cos_min*cos_min)*(mm*qq).
 *    Every operation is rounded to fp32 on its own (no FMA).  A NaN anywhere makes the pair incompatible, and so does a zero
 *    normal (mm*qq = 0).  cos_min lies in [0, 1]: the angle between the normals is at most acos(cos_min).
 *  - face normal: m = (b - a) x (c - a) of the face's stored corners a, b, c, with e1 = b - a, e2 = c - a:
 *    m.x = (e1.y*e2.z) - (e1.z*e2.y), m.y = (e1.z*e2.x) - (e1.x*e2.z), m.z = (e1.x*e2.y) - (e1.y*e2.x), unfused.  A degenerate
 *    face has mm = 0 and is never compatible.
 *  - vertex normals: vert_normals is the caller's (smplpp_mesh_vertex_normals gives one); the library adds no rule.
 *  - point -> mesh: a face is a candidate iff it is compatible with the query's normal and its squared distance d, from the
 *    point-triangle evaluation of smplpp_point_mesh_distance, has d <= max_sqdist.  With mn the minimum of d over the candidates, the
 *    answer is the lowest face id among the candidates with d <= mn (1 + 1e-6) + 1e-12; weights, closest and sqdist are those
 *    smplpp_point_mesh_distance gives for that face.
 *  - mesh -> point: smplpp_mesh_point_distance's rule (the smallest d, on equal d the lowest point index, a non-finite d never
 *    chosen) over the points that are compatible with the vertex's normal and have d <= max_sqdist.
 *  - max_sqdist may be +inf (no cap); a threshold equal to an attained d keeps it (<=).
 *  - no candidate: face / index = -1 and every other output of that row is +0.
 *  - a query or vertex with a non-finite coordinate or (when given) normal is unmatched, whatever the filter; a point with a
 *    non-finite normal is never chosen.
 *  - a NULL normals pointer: no normal test.  smplpp_mesh_point_distance_compatible tests normals only when BOTH arrays are given.
 *    Without a normal test and with max_sqdist = +inf, finite inputs (whose distances do not overflow) give exactly the bits of
 *    smplpp_point_mesh_distance / smplpp_mesh_point_distance.
 *  - the bits do not depend on n, on the frame's position in the batch, on the memory space, on the dispatch form
 *    (SMPLPP_POINT_DISTANCE_FORM, as for smplpp_point_mesh_distance: both forms evaluate the minimum and every face of the band;
 *    the tiled form's cull radius starts at max_sqdist, not at the nearest vertex, which may have ineligible faces only) or on how
 *    the mesh -> point call splits K.  One exception, inherited: `weights` has the bits smplpp_point_mesh_distance gives in the same
 *    form, and that call's two forms round the weights of a point inside a face differently (measured: the last bits, never face,
 *    closest or sqdist).
 *  - backward: there is no new product.  smplpp_point_mesh_distance_vjp and smplpp_mesh_point_distance_vjp take the face / index
 *    returned here.  In device space both ignore -1.  In HOST space smplpp_mesh_point_distance_vjp accepts -1 but
 *    smplpp_point_mesh_distance_vjp refuses it: replace the face of an unmatched query by 0 and give it a zero cotangent (a zero
 *    cotangent contributes nothing); the Python wrappers do so.
 *  - weights and closest are nullable; face / index and sqdist are not.
 *  - SMPLPP_ERR_INVALID (outputs untouched): bad arguments, cos_min outside [0, 1] or NaN, max_sqdist negative or NaN, the limits
 *    of the unfiltered calls (point -> mesh: a model without faces, n * K beyond int32; mesh -> point: n * K or n * V beyond int32). */
int smplpp_point_mesh_distance_compatible(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t K,
                                          const float * points /*[n,K,3]*/, const float * point_normals /*[n,K,3] nullable*/, float cos_min,
                                          float max_sqdist, int64_t * face /*[n,K]*/, float * weights /*[n,K,3] nullable*/,
                                          float * closest /*[n,K,3] nullable*/, float * sqdist /*[n,K]*/, int space, void * stream);
int smplpp_mesh_point_distance_compatible(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/,
                                          const float * vert_normals /*[n,V,3] nullable*/, int64_t K, const float * points /*[n,K,3]*/,
                                          const float * point_normals /*[n,K,3] nullable*/, float cos_min, float max_sqdist,
                                          int64_t * index /*[n,V]*/, float * sqdist /*[n,V]*/, int space, void * stream);
/* Generalized winding numbers at K query points per frame (which points lie inside the body: penetration and one-sided scan
 * terms): for each of n frames, igl::winding_number of that frame's posed mesh verts [n,V,3] at each of K points [n,K,3].
 *  - winding [n,K] has exactly the bits smplpp_sweep_grid gives at a cell of the same fp32 position: the same per-face term
 *    atan2f(det, den), summed in fp32 in ascending face order within each 256-face chunk, the chunk partials summed in fp64 in
 *    ascending chunk order, then (float)(acc / (2 pi)).  On a closed, outward-oriented mesh w ~ 1 inside, ~ 0 outside, ~ 2 where
 *    the posed mesh overlaps itself.
 *  - inside [n,K] (nullable) = w > 0.5f.  A NaN point or vertex gives w = NaN and inside = 0 (no refusal of device data).
 *  - the bits do not depend on n, on the frame's position in the batch, or on how the call splits the faces over workgroups (few
 *    frames: at 256-face chunk boundaries, chosen from n and K alone).
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, n * K beyond int32 indexing. */
int smplpp_point_mesh_winding(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t K, const float * points /*[n,K,3]*/,
                              float * winding /*[n,K]*/, uint8_t * inside /*[n,K] nullable*/, int space, void * stream);
/* Signed point-to-mesh distance: smplpp_point_mesh_distance and smplpp_point_mesh_winding in one call.
 *  - face, weights, closest have exactly the bits of smplpp_point_mesh_distance; winding and inside those of
 *    smplpp_point_mesh_winding, on the same inputs.
 *  - signed_sqdist = inside ? -sqdist : sqdist.  The SQUARED distance on purpose: sigma d^2 is continuous and C1 across the surface
 *    (both sides reach 0 with zero slope), so a penetration loss such as relu(-signed_sqdist) has no step there.
 *  - weights, closest and winding are nullable; face, inside and signed_sqdist are not.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, n * K beyond int32 indexing. */
int smplpp_point_mesh_signed_distance(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t K, const float * points /*[n,K,3]*/,
                                      int64_t * face /*[n,K]*/, float * weights /*[n,K,3] nullable*/, float * closest /*[n,K,3] nullable*/,
                                      float * winding /*[n,K] nullable*/, uint8_t * inside /*[n,K]*/, float * signed_sqdist /*[n,K]*/,
                                      int space, void * stream);
/* Vector-Jacobian product of signed_sqdist above, at the faces `face` and the flags `inside` the forward gave.  The sign is
 * piecewise constant, so this is smplpp_point_mesh_distance_vjp at the cotangent g * (inside ? -1 : 1), bit for bit (the
 * multiplication by -1 is exact), with all of its rules: accumulate = 0 overwrites, 1 adds; either output may be NULL, not both; a
 * zero cotangent contributes nothing, even on a NaN row; deterministic, no floating-point atomics.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, n * K beyond int32 indexing, host-space face ids out of range (a
 *    device-space face id out of range contributes nothing). */
int smplpp_point_mesh_signed_distance_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t K, const float * points,
                                          const int64_t * face /*[n,K]*/, const uint8_t * inside /*[n,K]*/,
                                          const float * grad_signed_sqdist /*[n,K]*/, float * grad_verts /*[n,V,3] nullable*/,
                                          float * grad_points /*[n,K,3] nullable*/, int accumulate, int space, void * stream);
/* Ray casting: where each of K rays per frame first meets that frame's posed mesh verts [n,V,3] (range sensors that are no pinhole
 * grid, normal shooting, occlusion of arbitrary segments, thickness).  A ray is origin + t dir; dir is used as given, not
 * normalised, and t is in units of |dir|.  With ray_frames = 1 the one set of rays [1,K,3] is cast against every frame.
 * The rule is fp32, every operation rounded on its own (no FMA), divisions correctly rounded:
 *  - per ray: kz = the axis of the largest |dir| (the lowest on a tie), kx = (kz + 1) mod 3, ky = (kz + 2) mod 3, Sx = dir[kx] / dir[kz],
 *    Sy = dir[ky] / dir[kz].  A ray is DEAD when a coordinate of origin or dir is not finite or dir[kz] == 0: face -1, t 0, bary 0,
 *    hits 0.
 *  - per (ray, vertex): P = x - origin, X = P[kx] - Sx P[kz], Y = P[ky] - Sy P[kz]: the vertex in the ray's own sheared plane.  These
 *    two fp32 numbers depend on the ray and the vertex only, never on the face, so two faces see a shared edge identically.
 *  - per edge p -> q of a face, in stored corner order (c0,c1), (c1,c2), (c2,c0): e = the sign of the EXACT real number
 *    X_p Y_q - Y_p X_q (the two rounded fp32 products compared where they differ, which is exact because rounding is monotone; in
 *    fp64, where both products are exact, where they are equal).  Where that number is zero, e = the sign of Y_p - Y_q, and where
 *    that is zero too, of X_q - X_p: the sign the edge function takes when the ray is moved by (eps, eps^2) in its plane for every
 *    small enough eps > 0.  (A tie rule on vertex ids, p < q, gives a ray on a shared edge to one of its two faces but a ray through a
 *    vertex to as many faces of its fan as the ids happen to descend through it, none or several; the shift is one geometric
 *    direction for all faces, so the ray is inside exactly the faces a generic ray beside it is inside.)
 *  - a face is COVERED with sign s in {+1, -1} when its three edges have e = s, and is FRONT when s sign(dir[kz]) < 0 (in exact
 *    arithmetic s |dir[kz]| has the sign of n . dir, n = (b - a) x (c - a): front = the ray runs against the stored winding's normal),
 *    else BACK.  facing = 1 keeps front faces, 2 back faces, 3 both.  A face with a corner that is not finite covers nothing (device
 *    data is never refused).  On a closed consistently oriented mesh every live ray is covered by as many front as back faces.
 *  - range of a covered face (a, b, c): A = a - origin, e1 = b - a, e2 = c - a, n = e1 x e2 (each component u v - w z),
 *    na = (n.x A.x + n.y A.y) + n.z A.z, nd the same form with dir, t = na / nd.  The candidate is dropped unless t is finite and
 *    t_min < t <= t_max.
 *  - the winner is the smallest t, on equal bits the lowest face id: the minimum of bits(t) << 32 | face (monotone: t > t_min >= 0).
 *    face = -1 and t = 0 when nothing is left.
 *  - bary [n,K,3] (nullable), as smplpp_depth_raster forms it from the hit point: w = t dir - A,
 *    beta_b = (w x e2) . n / nn, beta_c = (e1 x w) . n / nn, beta_a = (1 - beta_b) - beta_c, nn = (n.x n.x + n.y n.y) + n.z n.z,
 *    every cross component u v - w z and every dot (x + y) + z.  0 without a hit.
 *  - hits [n,K,2] (nullable) = (front, back) counts of the ray's accepted candidates under `facing` (integers).
 *  - the bits do not depend on n, on the frame's slot, on ray_frames, on the memory space, on the outputs asked for or on how the call
 *    deals the 256-face chunks over workgroups (from n and K alone; SMPLPP_RAY_SLICES = 1..4096 in the environment of
 *    smplpp_model_create fixes the count, for tests).  Workgroups meet through a 64-bit integer minimum and integer adds; there are
 *    no floating-point atomics.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, ray_frames not 1 or n, K < 1, t_min not finite or < 0, t_max NaN or
 *    <= t_min (+inf is allowed), facing outside 1..3, n K, n V or n F beyond int32 indexing. */
int smplpp_ray_cast(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t ray_frames /*1 or n*/, int64_t K,
                    const float * origin /*[ray_frames,K,3]*/, const float * dir /*[ray_frames,K,3]*/, float t_min, float t_max,
                    int facing /*1 front, 2 back, 3 both*/, int64_t * face /*[n,K]*/, float * t /*[n,K]*/,
                    float * bary /*[n,K,3] nullable*/, int32_t * hits /*[n,K,2] nullable*/, int space, void * stream);
/* Vector-Jacobian product of t above for g = grad_t [n,K], at the faces `face` the forward gave, held fixed.  The range is recomputed
 * on the named face (na, nd, t, then the barycentrics of t dir as above) and no state is kept.  For a ray with 0 <= face < F, not
 * dead, and g != 0:
 *    vec = (g / nd) n;   corner i (a, b, c) receives beta_i vec;   grad_origin = -vec;   grad_dir = -(t vec).
 * Every other ray (face = -1, a dead ray, g == 0, a device-space id out of range) contributes nothing, even on NaN data.
 *  - grad_verts [n,V,3] is one fixed-order sum per vertex from +0: ascending ray, then corner (the record gather of the scan
 *    distances); no floating-point atomics.
 *  - ray_frames = 1: grad_origin and grad_dir [1,K,3] are the frames' sums in the two-level order of smplpp_vertex_offsets_vjp (tiles
 *    of SMPLPP_VERTEX_OFFSETS_TILE frames, ascending within a tile from its first term, then across the tiles; a ray that contributes
 *    nothing is the term +0).
 *  - any output may be NULL, not all.  accumulate = 0 stores the finished value, 1 adds it to what the output holds (one addition at
 *    the end).  There is no cotangent for bary: a hit point's cotangent is composed by the caller through origin + t dir.
 *  - SMPLPP_ERR_INVALID: as the forward's (without t_min, t_max, facing), accumulate not 0 or 1, a host-space face id outside [-1, F)
 *    (the outputs are untouched). */
int smplpp_ray_cast_vjp(smplpp_model * m, int64_t n, const float * verts, int64_t ray_frames, int64_t K, const float * origin,
                        const float * dir, const int64_t * face /*[n,K], held fixed*/, const float * grad_t /*[n,K]*/,
                        float * grad_verts /*[n,V,3] nullable*/, float * grad_origin /*[ray_frames,K,3] nullable*/,
                        float * grad_dir /*[ray_frames,K,3] nullable*/, int accumulate, int space, void * stream);
/* Self-intersections of each frame's posed mesh verts [n,V,3]: every pair of the model's faces (f, g), f < g, that share no vertex
 * and intersect under this exact fp32 rule (every operation rounded on its own, no FMA):
 *  - orient(a,b,c,d): u = b-a, v = c-a, w = d-a; cx = u.y v.z - u.z v.y, cy = u.z v.x - u.x v.z, cz = u.x v.y - u.y v.x;
 *    (cx w.x + cy w.y) + cz w.z.
 *  - edge pq crosses triangle abc iff orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs and orient(p,q,a,b),
 *    orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0.  A triangle's edges are (c0,c1), (c1,c2), (c2,c0) of its stored
 *    corners.
 *  - f and g intersect iff their closed fp32 AABBs overlap and some edge of either crosses the other.  Coplanar and merely
 *    touching pairs are not reported; a face with a non-finite coordinate intersects nothing.
 *  - pairs [n,max_pairs,2] (nullable when max_pairs = 0) in ascending (f, g); count [n] the true total, also beyond max_pairs
 *    (then the lowest max_pairs pairs are stored); rows past min(count, max_pairs) are -1.
 *  - the bits do not depend on n or on the frame's position in the batch; no floating-point atomics.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, max_pairs < 0, n * max_pairs, n * F or n * V beyond int32
 *    indexing. */
int smplpp_self_intersections(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t max_pairs,
                              int64_t * pairs /*[n,max_pairs,2]*/, int64_t * count /*[n]*/, int space, void * stream);
/* smplpp_self_intersections, then one self-penetration energy per stored pair (0 past min(count, max_pairs)): each pair is scored
 * both ways, receiver f with g's corners, then receiver g with f's.  For a receiver (a, b, c): o = (a+b+c)/3,
 * n = normalize((b-a) x (c-a)), rho^2 = (|a-o|^2 + |b-o|^2 + |c-o|^2)/3; an intruder corner x gives h = (x-o).n,
 * q^2 = |x-o|^2 - h^2, phi = max(0, 1 - q^2 / (sigma^2 rho^2)) and contributes phi^2 h^2 if h < 0, else 0.  C1 in all six corners;
 * a receiver of zero area contributes 0.  sigma (default 2) must be finite and > 0.  pairs and count as smplpp_self_intersections. */
int smplpp_self_penetration(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t max_pairs, float sigma,
                            int64_t * pairs /*[n,max_pairs,2]*/, int64_t * count /*[n]*/, float * pair_energy /*[n,max_pairs]*/,
                            int space, void * stream);
/* Vector-Jacobian product of pair_energy above to the vertices, at the pairs the forward gave (held fixed): accumulate = 0
 * overwrites grad_verts, 1 adds; rows past min(count, max_pairs) and a zero cotangent contribute nothing, even on a NaN row;
 * deterministic, no floating-point atomics.
 *  - SMPLPP_ERR_INVALID: as the forward, host-space face ids out of range in the rows below min(count, max_pairs) (a device-space
 *    pair with an id out of range contributes nothing).
 *  - the handle keeps a record workspace of 384 bytes per (frame, row): n * max_pairs * 384 bytes (the counts are on the device
 *    when the call is enqueued), grown to the largest call and held until the model is destroyed; pass a max_pairs near the counts
 *    the forward returned to keep it small. */
int smplpp_self_penetration_vjp(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t max_pairs, float sigma,
                                const int64_t * pairs /*[n,max_pairs,2]*/, const int64_t * count /*[n]*/,
                                const float * grad_pair_energy /*[n,max_pairs]*/, float * grad_verts /*[n,V,3]*/, int accumulate,
                                int space, void * stream);
/* Depth rasteriser: each frame's posed mesh verts [n,V,3] through a pinhole camera into a face-id + depth image of H rows and W
 * columns.  camera [n,16] per frame: R (9, row-major, world -> camera), t (3), fx, fy, cx, cy; the camera looks along +z, x right,
 * y down; pixel (row j, column i) has its centre at (i + 0.5, j + 0.5).  The rule, in fp32 with every operation rounded on its own
 * (no FMA; correctly rounded divisions) unless it says integer:
 *  - vertex: xc.k = ((R[3k] x + R[3k+1] y) + R[3k+2] z) + t[k]; u = (fx xc.x) / xc.z + cx, v = (fy xc.y) / xc.z + cy;
 *    su = rintf(u * 256), sv = rintf(v * 256) (ties to even).  The vertex is refused unless xc is finite, xc.z > near and
 *    |su|, |sv| <= 2^23 (a guard band of 32768 px: edge functions below stay under 2^51).  X = (int) su, Y = (int) sv.
 *  - a face (a, b, c) of the model with a refused corner is skipped, and counted in culled[frame] (no clipping).  Otherwise, in
 *    int64: A2 = (Xb-Xa)(Yc-Ya) - (Yb-Ya)(Xc-Xa); A2 = 0 covers nothing; s = sign(A2).  For each corner k, with p, q the next two
 *    corners in cyclic order: ex = s (Xq-Xp), ey = s (Yq-Yp), E = ex (Py-Yp) - ey (Px-Xp) at the pixel centre
 *    (Px, Py) = (256 i + 128, 256 j + 128).  The pixel is covered iff for all three E > 0, or E = 0 and (ey < 0, or ey = 0 and
 *    ex > 0) (top-left rule: a centre on an edge two faces share belongs to exactly one of them).  Both orientations are drawn.
 *  - depth of a covered pixel: in camera space e1 = b-a, e2 = c-a, n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *    e1.x e2.y - e1.y e2.x), na = (n.x a.x + n.y a.y) + n.z a.z; the centre's ray d = ((((float) i + 0.5) - cx) / fx,
 *    (((float) j + 0.5) - cy) / fy, 1); nd = (n.x d.x + n.y d.y) + n.z; depth = na / nd.  A candidate whose depth is not finite or
 *    <= near is dropped.
 *  - depth test: the smallest depth wins, on equal depth bits the lowest face id (the minimum of depth bits << 32 | face id).
 *  - face [n,H,W]: the winner, -1 at background.  depth [n,H,W]: its depth, 0 at background.  bary [n,H,W,3] (nullable): with
 *    w = (depth d.x - a.x, depth d.y - a.y, depth - a.z), nn = (n.x n.x + n.y n.y) + n.z n.z, dot(p, q) = (p.x q.x + p.y q.y) +
 *    p.z q.z and cross() as n above: beta_b = dot(cross(w, e2), n) / nn, beta_c = dot(cross(e1, w), n) / nn,
 *    beta_a = (1 - beta_b) - beta_c; stored (beta_a, beta_b, beta_c), 0 at background.  They are the weights of the hit point
 *    depth d in 3-D, consistent with depth; a pixel the snap put just outside the true triangle has one a little below 0.
 *  - visible [n,V] (nullable): 1 iff the vertex is a corner of a face that owns at least one pixel of the frame, else 0.  Exact and
 *    parameter-free; it depends on the resolution (a face that falls between pixel centres is not seen), and a corner of a partly
 *    hidden face counts as seen.  culled [n] (nullable): the skipped faces.
 *  - the bits of a frame do not depend on n, on its position in the batch, on the memory space or on how the work is split
 *    (SMPLPP_DEPTH_RASTER_INLINE, read at model creation); no floating-point atomics.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, H or W outside [1, 8192], near not finite or <= 0, n H W, n V or n F
 *    beyond int32 indexing.  Device data is never refused: NaN vertices give skipped faces. */
int smplpp_depth_raster(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, const float * camera /*[n,16]*/, int64_t H,
                        int64_t W, float near, int64_t * face /*[n,H,W]*/, float * depth /*[n,H,W]*/,
                        float * bary /*[n,H,W,3] nullable*/, uint8_t * visible /*[n,V] nullable*/, int64_t * culled /*[n] nullable*/,
                        int space, void * stream);
/* Vector-Jacobian product of depth above to the world-space vertices, at the faces the forward chose (face [n,H,W], held fixed;
 * coverage is not differentiated): with g = grad_depth at a pixel, beta, n, nd as above, corner i of the pixel's face receives
 * R^T (g beta_i n / nd).  In fp32: per face, s_i = sum of beta_i * (g / nd) over the pixel centres of its snapped bounding box
 * (clipped to the image, row-major) that name the face and have g != 0, entry r of the box summed by lane r mod 8 in ascending r,
 * the eight partial sums combined as ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7)); the face's vector for corner i is s_i n; a vertex sums
 * the vectors of its faces in ascending face id, and R^T is applied once.  accumulate = 0 overwrites grad_verts (untouched
 * vertices get 0), 1 adds.  A pixel with face = -1 or a cotangent of exactly 0 contributes nothing, even when its data is NaN;
 * so does a pixel outside its face's snapped bounding box and a face with a non-finite or out-of-band projection (the forward
 * names neither).  Deterministic, no floating-point atomics.  No gradient to camera.
 *  - SMPLPP_ERR_INVALID: as the forward, accumulate not 0 or 1, a host-space face id outside [-1, F) (the output is untouched; a
 *    device-space id out of range contributes nothing). */
int smplpp_depth_raster_vjp(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, const float * camera /*[n,16]*/, int64_t H,
                            int64_t W, const int64_t * face /*[n,H,W]*/, const float * grad_depth /*[n,H,W]*/,
                            float * grad_verts /*[n,V,3]*/, int accumulate, int space, void * stream);
/* Raster attribute interpolation: a per-vertex quantity attr [n,V,C], C in [1, 32], carried into the image of smplpp_depth_raster.
 * face [n,H,W] and bary [n,H,W,3] are that call's outputs.  In fp32 with every operation rounded on its own (no FMA): for a pixel
 * with f = face in [0, F), (a, b, c) the model's corners of f and (beta_a, beta_b, beta_c) = bary at the pixel, for each channel k
 *    image[k] = (beta_a attr[a][k] + beta_b attr[b][k]) + beta_c attr[c][k];
 * a background pixel (face = -1) gives +0 in every channel, whatever its bary and the attributes hold; so does a device-space id
 * outside [-1, F).  image [n,H,W,C].  The bits of a frame do not depend on n, on its position in the batch or on the memory space.
 *  - SMPLPP_ERR_INVALID: bad arguments, a model without faces, H or W outside [1, 8192], C outside [1, 32], n H W C, n V C, n V or
 *    n F beyond int32 indexing, a host-space face id outside [-1, F) (the output is untouched).  Device data is never refused. */
int smplpp_raster_interpolate(smplpp_model * m, int64_t n, const float * attr /*[n,V,C]*/, int64_t C, int64_t H, int64_t W,
                              const int64_t * face /*[n,H,W]*/, const float * bary /*[n,H,W,3]*/, float * image /*[n,H,W,C]*/,
                              int space, void * stream);
/* Vector-Jacobian product of image above to the attributes and to the world-space vertices.  verts, camera, H, W, near are the
 * arguments of the smplpp_depth_raster call that gave face and bary.  With g = grad_image [n,H,W,C] at a pixel:
 *  - grad_attr [n,V,C] (face and bary held fixed as data): corner i of the pixel's face receives beta_i g[k] in channel k.
 *  - grad_verts [n,V,3] is the gradient through the barycentrics (face and the pixel's ray held fixed, coverage not differentiated):
 *    the function differentiated is sum_i beta_i(verts) (sum_k g[k] attr[i][k]), beta as the rasteriser defines them (the hit
 *    point of the pixel centre's ray on the plane of the face's camera-space corners).  With e1, e2, n, nn, d, nd, dot and cross of
 *    the rasteriser's rule, in fp32: gamma_i = sum over k, ascending from +0, of g[k] attr[i][k]; c1 = cross(e2, n),
 *    c2 = cross(n, e1); q.x = ((gamma_b - gamma_a) c1.x + (gamma_c - gamma_a) c2.x) / nn (y, z alike); s = dot(q, d) / nd;
 *    h.x = n.x s - q.x (y, z alike); camera-space corner i receives beta_i h (beta from bary), and R^T is applied once per vertex.
 *  - the order of every sum: per face, its snapped bounding box (the rasteriser's vertex rule with `near`, clipped to the image,
 *    row-major) is walked, entry r by lane r mod 8 in ascending r, over the pixels that name the face; the eight partial sums are
 *    combined as ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7)); a vertex sums its faces' values in ascending face id, each from +0; for
 *    grad_verts R^T follows as in smplpp_depth_raster_vjp.  accumulate = 0 stores the sum (untouched vertices get 0), 1 adds it to
 *    the output.  No floating-point atomics; the bits do not depend on n, on the frame's position in the batch, on the memory space,
 *    on which of the two outputs is asked for, or on SMPLPP_DEPTH_RASTER_INLINE (which is not read).
 *  - a cotangent element g[k] of exactly 0 contributes nothing to either output, even on NaN data: a pixel whose C values are all 0
 *    is as good as absent.  So is a pixel with face = -1 (or, in device space, an id out of range), a pixel outside its face's
 *    snapped box, and a face with a refused corner.
 *  - grad_attr or grad_verts may be NULL, not both.  No gradient to camera.
 *  - SMPLPP_ERR_INVALID: as the forward, near not finite or <= 0, accumulate not 0 or 1, both outputs NULL (the outputs are
 *    untouched).
 *  - the handle keeps 24 bytes per (frame, vertex) and 48 bytes per (frame, face) of workspace, grown to the largest call and shared
 *    with smplpp_depth_raster and smplpp_depth_raster_vjp: concurrent calls on one handle from different streams need the caller's
 *    own ordering (see "Streams and sharing" below). */
int smplpp_raster_interpolate_vjp(smplpp_model * m, int64_t n, const float * attr /*[n,V,C]*/, int64_t C,
                                  const float * verts /*[n,V,3]*/, const float * camera /*[n,16]*/, int64_t H, int64_t W, float near,
                                  const int64_t * face /*[n,H,W]*/, const float * bary /*[n,H,W,3]*/,
                                  const float * grad_image /*[n,H,W,C]*/, float * grad_attr /*[n,V,C] nullable*/,
                                  float * grad_verts /*[n,V,3] nullable*/, int accumulate, int space, void * stream);
#define SMPLPP_VERTEX_OFFSETS_TILE 32 /* frames per tile of the shared sum of smplpp_vertex_offsets_vjp */
/* SMPL+D: per-vertex offsets D in the rest pose, carried through linear blend skinning, verts_D = LBS(rest + D, G') with the joints
 * regressed from the undisplaced shape.  Skinning is linear in the rest position, so verts_D = verts + (sum_j w_vj R'_fj) D_v / wSum_v,
 * with verts, xforms (G', of which R'_fj is the upper-left 3x3 of joint j in frame f) as smplpp_fk returned them, whatever form
 * (SMPLPP_SKIN) computed them.  In fp32 with every operation rounded on its own (no FMA), per (frame f, vertex v), with w the model's
 * skinning weights and wSum_v the model's sum of them in ascending j (the homogeneous divide of smplpp_fk):
 *    M[a][b]  = the sum over the joints j with w_vj != 0, in ascending j, starting from +0, of w_vj * R'_fj[a][b];
 *    delta[a] = ((M[a][0] d[0] + M[a][1] d[1]) + M[a][2] d[2]) / wSum_v,   d = offsets[f][v] (offset_frames = n) or offsets[0][v] (= 1);
 *    verts_out[f][v][a] = verts[f][v][a] + delta[a];      rest_displaced[f][v][a] = rest[f][v][a] + d[a].
 * A joint with a zero weight is not read, so models that keep 4, 8 or 24 weights per vertex follow the one rule.  A zero offsets row
 * returns the vertex (== ; the sign of a zero may differ).  verts_out may be verts, and rest_displaced may be rest (in place: the same
 * bits).  rest and rest_displaced may both be NULL; rest alone is ignored.  rest_displaced is the `rest` smplpp_fk_vjp takes to give the
 * exact dL/dbeta and dL/dtheta of the displaced body.  The bits do not depend on n, on the frame's position in the batch or on the
 * memory space, nor on the frames a workgroup takes (by n; SMPLPP_VERTEX_OFFSETS_FRAMES = 1..32 in the environment of
 * smplpp_model_create fixes it, for tests).
 *  - SMPLPP_ERR_INVALID: n <= 0, a NULL verts, xforms, offsets or verts_out, offset_frames neither 1 nor n, rest_displaced without
 *    rest, n * V * 3 beyond int32 indexing (the outputs are untouched, nothing is launched). */
int smplpp_vertex_offsets(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, const float * xforms /*[n,24,4,4]*/,
                          const float * offsets /*[offset_frames,V,3]*/, int64_t offset_frames /*1 or n*/,
                          const float * rest /*[n,V,3] nullable*/, float * rest_displaced /*[n,V,3] nullable*/,
                          float * verts_out /*[n,V,3], may be == verts*/, int space, void * stream);
/* Vector-Jacobian product of verts_out above to the offsets (to verts it is the identity; to beta and theta it is smplpp_fk_vjp with
 * rest = rest_displaced).  Per (f, v), with M as above and g = grad_verts[f][v], in fp32, every operation rounded on its own:
 *    gt[a] = g[a] / wSum_v;      t[b] = (M[0][b] gt[0] + M[1][b] gt[1]) + M[2][b] gt[2].
 *  - offset_frames = n: grad_offsets[f][v] = t.
 *  - offset_frames = 1 (one field shared by all frames): grad_offsets[0][v] is the sum of t over the frames in a fixed two-level
 *    order: the frames are cut into consecutive tiles of SMPLPP_VERTEX_OFFSETS_TILE; a tile's sum starts from its first frame's t and
 *    adds the others in ascending frame; the result starts from the first tile's sum and adds the others in ascending tile.  It
 *    depends on n through that tree only, never on the launch geometry.
 *  - accumulate = 0 stores the finished value, 1 adds it to what grad_offsets holds (one addition at the end).
 *  - a vertex whose cotangent rows are all zero receives 0.  No floating-point atomics; the same inputs give the same bits, in
 *    either memory space.
 *  - SMPLPP_ERR_INVALID: n <= 0, a NULL xforms, grad_verts or grad_offsets, grad_offsets == grad_verts, offset_frames neither 1 nor
 *    n, accumulate not 0 or 1, n * V * 3 beyond int32 indexing (the output is untouched, nothing is launched).
 *  - the shared sum keeps 12 bytes per (tile, vertex) of workspace on the handle, grown to the largest call. */
int smplpp_vertex_offsets_vjp(smplpp_model * m, int64_t n, const float * xforms /*[n,24,4,4]*/, const float * grad_verts /*[n,V,3]*/,
                              int64_t offset_frames /*1 or n*/, float * grad_offsets /*[offset_frames,V,3]*/, int accumulate,
                              int space, void * stream);
/* Mesh Laplacian of a per-vertex field x [n,V,C], C in [1, 32], the smoothness operator for the offsets.  In fp32, per (frame,
 * vertex v, channel): over the faces t that contain v, in ascending t (the adjacency of the normals' backward pass), starting from +0,
 *    (L x)_v = sum_t ((x_v - x_a) + (x_v - x_b)),   a, b = the other two corners of t in its cyclic order after v.
 * Every edge of a closed manifold mesh lies in two faces, so there L is twice the graph Laplacian (deg(v) x_v - sum of the
 * neighbours).  L is symmetric, so it is its own vector-Jacobian product: lambda |L D|^2 has the gradient 2 lambda L (L D), two
 * calls.  A field that is constant over the mesh gives exactly 0.  accumulate = 0 stores, 1 adds the finished value to out.
 *  - SMPLPP_ERR_INVALID: n <= 0, C outside [1, 32], a NULL x or out, out == x, a model without faces, accumulate not 0 or 1,
 *    n * V * C beyond int32 indexing (the output is untouched, nothing is launched). */
int smplpp_mesh_laplacian(smplpp_model * m, int64_t n, const float * x /*[n,V,C], 1 <= C <= 32*/, int64_t C, float * out /*[n,V,C]*/,
                          int accumulate, int space, void * stream);
#define SMPLPP_UNSKIN_MIN_DET 1e-4f /* smplpp_unskin_points: a blend with |det M| <= this * s^3 has collapsed (a blend of rotations has det / s^3 in (0, 1]) */
/* Skinning of bound points: K points that are not the model's vertices (a garment, hair, the samples of an avatar, markers off the
 * skin), each carried by the blend of the world joint transforms.  world [n,24,3,4] = [A_j | p_j] and joints [n,24,3] = J_j are what
 * smplpp_skeleton returned; the root translation is inside p_j, there is no separate trans.  The translation of joint j's relative
 * transform is c_j[a] = p_j[a] - ((A_j[a][0] J_j[0] + A_j[a][1] J_j[1]) + A_j[a][2] J_j[2]).  points is [point_frames,K,3] and the
 * binding is over bind_frames, each 1 (shared by the frames) or n.  Exactly one binding is given, the other's pointers are NULL:
 *  - a face binding, face [bind_frames,K] and bary [bind_frames,K,3], the `face` and `weights` outputs of smplpp_point_mesh_distance:
 *    with (v0, v1, v2) the corners of the face and W the model's kept skinning weights (0 where none is kept),
 *    w_j = (bary0 W[v0][j] + bary1 W[v1][j]) + bary2 W[v2][j];
 *  - a weight binding, weights [bind_frames,K,24], used as given: w_j = weights[k][j].  They need not sum to 1.
 * In fp32 with every operation rounded on its own (no FMA), per (frame, point), over the joints with w_j != 0 in ascending j, each
 * sum starting from +0:
 *    s = sum w_j,    M[a][b] = sum w_j A_j[a][b],    t[a] = sum w_j c_j[a];
 *    h[a] = ((M[a][0] x[0] + M[a][1] x[1]) + M[a][2] x[2]) + t[a],    out[a] = h[a] / s,         x = the rest-pose point.
 * blend [n,K,3,4] (nullable) is the point's own transform, blend[a][b] = M[a][b] / s and blend[a][3] = t[a] / s, with which a caller
 * rotates normals or covariances; valid [n,K] (nullable) is 1 for a live point.  A point is DEAD when its face id is outside [0, F)
 * (device space; a host-space id out of range is refused), when a coordinate of it, a bary or one of its 24 weights is not finite,
 * or when !(s > 0).  A dead point gives +0 in every output and valid = 0 and never touches its neighbours.  The bits do not depend on
 * n, on the frame's position in the batch, on the memory space, on which outputs are asked for, or on the frames a workgroup takes
 * (by n and K; SMPLPP_SKIN_POINTS_FRAMES = 1..32 in the environment of smplpp_model_create fixes it, for tests).  A device-space call
 * touches nothing in the handle and keeps no workspace.
 *  - SMPLPP_ERR_INVALID: n <= 0 or K <= 0, a NULL world, joints, points or out, both bindings or neither, a face binding on a model
 *    without faces, point_frames or bind_frames neither 1 nor n, a host-space face id out of range, n * K * 24 (or n * 288) beyond
 *    int32 indexing (the outputs are untouched, nothing is launched). */
int smplpp_skin_points(smplpp_model * m, int64_t n, const float * world /*[n,24,3,4]*/, const float * joints /*[n,24,3]*/, int64_t K,
                       const float * points /*[point_frames,K,3]*/, int64_t point_frames /*1 or n*/,
                       const int64_t * face /*[bind_frames,K] or NULL*/, const float * bary /*[bind_frames,K,3] or NULL*/,
                       const float * weights /*[bind_frames,K,24] or NULL*/, int64_t bind_frames /*1 or n*/, float * out /*[n,K,3]*/,
                       float * blend /*[n,K,3,4] nullable*/, uint8_t * valid /*[n,K] nullable*/, int space, void * stream);
/* The inverse (unposing, canonicalisation): points are POSED points y and out the rest-pose points x with skin(x) = y under the same
 * binding.  With s, M, t as above, indices taken mod 3:
 *    q[a] = s y[a] - t[a];      C[a][b] = M[a+1][b+1] M[a+2][b+2] - M[a+1][b+2] M[a+2][b+1]      (the cofactors, in cyclic form);
 *    det = (M[0][0] C[0][0] + M[0][1] C[0][1]) + M[0][2] C[0][2];      out[b] = ((C[0][b] q[0] + C[1][b] q[1]) + C[2][b] q[2]) / det.
 * blend and valid are as in smplpp_skin_points (the transform of the FORWARD map: out goes to y by it).  A point is dead as there,
 * and also when !(|det| > ((SMPLPP_UNSKIN_MIN_DET s) s) s): the blend has collapsed, as half and half of two rotations pi apart does.
 * Refusals as smplpp_skin_points. */
int smplpp_unskin_points(smplpp_model * m, int64_t n, const float * world /*[n,24,3,4]*/, const float * joints /*[n,24,3]*/, int64_t K,
                         const float * points /*[point_frames,K,3]*/, int64_t point_frames /*1 or n*/,
                         const int64_t * face /*[bind_frames,K] or NULL*/, const float * bary /*[bind_frames,K,3] or NULL*/,
                         const float * weights /*[bind_frames,K,24] or NULL*/, int64_t bind_frames /*1 or n*/, float * out /*[n,K,3]*/,
                         float * blend /*[n,K,3,4] nullable*/, uint8_t * valid /*[n,K] nullable*/, int space, void * stream);
/* Vector-Jacobian product of smplpp_skin_points for g = grad_out [n,K,3].  The forward is recomputed; no state is kept.  Per live
 * (frame, point), with s, M as above:
 *    gt[a] = g[a] / s;      grad_points[b] = (M[0][b] gt[0] + M[1][b] gt[1]) + M[2][b] gt[2].
 * Per (frame, joint j), by sum1024 over the points k (FIXED-ORDER SUMS below: element k goes to partial k mod 1024), leaving out the
 * points with w_kj == 0 and the dead ones, which is bit-neutral under that rule:
 *    dc[a] = sum1024_k (w_kj gt_k[a]);      dR[a][b] = sum1024_k ((w_kj gt_k[a]) x_k[b]);
 * and, written once per (frame, joint) in the cotangent layout smplpp_skeleton_vjp takes,
 *    grad_world[j][a][b] = dR[a][b] - dc[a] J_j[b];      grad_world[j][a][3] = dc[a];
 *    grad_joints[j][b] = -((A_j[0][b] dc[0] + A_j[1][b] dc[1]) + A_j[2][b] dc[2]).
 * The weights are divided by their sum, so sum_j dc_j = sum_k g_k: the grad_trans that smplpp_skeleton_vjp forms from column 3 of
 * grad_world is the right one, and no separate translation gradient exists.  For a weight binding only, for all 24 joints including
 * those with w_j = 0 (the gradient a learned skinning field needs):
 *    d[a] = (((A_j[a][0] x[0] + A_j[a][1] x[1]) + A_j[a][2] x[2]) + c_j[a]) - out[a];      grad_weights[k][j] = (gt[0] d[0] + gt[1] d[1]) + gt[2] d[2].
 * There is no gradient to face or bary: they are fixed correspondences.  A dead point contributes no term and receives +0.
 *  - point_frames = 1: grad_points [1,K,3] is the sum over the frames; bind_frames = 1: grad_weights [1,K,24] likewise.  Both use the
 *    two-level order of smplpp_vertex_offsets_vjp: tiles of SMPLPP_VERTEX_OFFSETS_TILE frames, ascending within a tile from its first
 *    term and then across the tiles (a dead (frame, point) is the term +0).
 *  - any output may be NULL, not all.  accumulate = 0 stores the finished value, 1 adds it to what the output holds (one addition at
 *    the end), so grad_world can share a buffer with smplpp_orientation_term_vjp's grad_frames.
 *  - the bits do not depend on n, on the slot, on the memory space, on which outputs are asked for, on the frames a workgroup takes or
 *    on who holds which partial of sum1024 (by K, as frame_sum_split; SMPLPP_SKIN_POINTS_SPLIT = 4 or 1 in the environment of
 *    smplpp_model_create fixes a workgroup of 256 or 1024 threads, for tests).
 *  - SMPLPP_ERR_INVALID: as the forward, a NULL grad_out, every gradient NULL, grad_weights with a face binding, accumulate not 0 or
 *    1 (the outputs are untouched, nothing is launched). */
int smplpp_skin_points_vjp(smplpp_model * m, int64_t n, const float * world /*[n,24,3,4]*/, const float * joints /*[n,24,3]*/, int64_t K,
                           const float * points /*[point_frames,K,3]*/, int64_t point_frames /*1 or n*/,
                           const int64_t * face /*[bind_frames,K] or NULL*/, const float * bary /*[bind_frames,K,3] or NULL*/,
                           const float * weights /*[bind_frames,K,24] or NULL*/, int64_t bind_frames /*1 or n*/,
                           const float * grad_out /*[n,K,3]*/, float * grad_points /*[point_frames,K,3] nullable*/,
                           float * grad_world /*[n,24,3,4] nullable*/, float * grad_joints /*[n,24,3] nullable*/,
                           float * grad_weights /*[bind_frames,K,24] nullable*/, int accumulate, int space, void * stream);
/* Vector-Jacobian product of smplpp_unskin_points for g = grad_out = dL/dx [n,K,3].  Per live (frame, point), with C, det, s and the
 * recomputed forward output x as above:
 *    u[a] = ((C[a][0] g[0] + C[a][1] g[1]) + C[a][2] g[2]) / det;      grad_points[a] = s u[a]      (to the posed points).
 * The per-joint sums, grad_world and grad_joints are exactly those of smplpp_skin_points_vjp with gt := -u and x := the recomputed
 * forward output.  For a weight binding, with y the posed point given:
 *    r_j[a] = ((A_j[a][0] x[0] + A_j[a][1] x[1]) + A_j[a][2] x[2]) + c_j[a];      d[a] = y[a] - r_j[a];
 *    grad_weights[k][j] = (u[0] d[0] + u[1] d[1]) + u[2] d[2].
 * Shared inputs, accumulate, the independence of the bits and the refusals are those of smplpp_skin_points_vjp. */
int smplpp_unskin_points_vjp(smplpp_model * m, int64_t n, const float * world /*[n,24,3,4]*/, const float * joints /*[n,24,3]*/, int64_t K,
                             const float * points /*[point_frames,K,3]*/, int64_t point_frames /*1 or n*/,
                             const int64_t * face /*[bind_frames,K] or NULL*/, const float * bary /*[bind_frames,K,3] or NULL*/,
                             const float * weights /*[bind_frames,K,24] or NULL*/, int64_t bind_frames /*1 or n*/,
                             const float * grad_out /*[n,K,3]*/, float * grad_points /*[point_frames,K,3] nullable*/,
                             float * grad_world /*[n,24,3,4] nullable*/, float * grad_joints /*[n,24,3] nullable*/,
                             float * grad_weights /*[bind_frames,K,24] nullable*/, int accumulate, int space, void * stream);
/* Exact Euclidean feature transform of n binary images mask [n,H,W] (a nonzero byte = set), all in integers.  For pixel p = (row j,
 * column i) and the set pixels q = (j', i') of the same frame, d2(p, q) = (i-i')^2 + (j-j')^2: sqdist[p] is the minimum and
 * nearest[p] the linear index j' W + i' of the set pixel that attains it; among equal distances the lowest linear index wins (the
 * minimum of the key d2 << 32 | linear index).  A set pixel names itself with 0; a frame without a set pixel gives nearest = -1 and
 * sqdist = 0 everywhere.  Either output may be NULL, not both.  The bits do not depend on n, on the frame's position in the batch
 * or on the memory space.  (Computed separably: each column's nearest set pixel per row, the upper one on a tie, then the minimum
 * key over a row's columns; a pixel that is not its column's nearest can never tie for the minimum.)
 *  - SMPLPP_ERR_INVALID: bad arguments, H or W outside [1, 8192], n H W beyond int32 indexing (the outputs are untouched).
 *  - the handle keeps 2 bytes per (frame, pixel) of workspace, grown to the largest call and shared with smplpp_silhouette. */
int smplpp_mask_distance_transform(smplpp_model * m, int64_t n, const uint8_t * mask /*[n,H,W]*/, int64_t H, int64_t W,
                                   int64_t * nearest /*[n,H,W] nullable*/, int32_t * sqdist /*[n,H,W] nullable*/, int space,
                                   void * stream);
/* Silhouette residuals of each frame's posed mesh against a target mask [n,H,W] (a nonzero byte = set).  verts, camera, H, W, near as
 * smplpp_depth_raster; face [n,H,W] is that call's output for the same arguments (coverage is face >= 0).  With T_mask and T_cov
 * the transform above of the mask and of the coverage, in fp32 with every operation rounded on its own:
 *  - model -> mask, per vertex (every vertex, seen or hidden, should project into the target): the vertex is projected by the
 *    rasteriser's vertex rule (same operations, same refusal; the unsnapped u, v).  A refused vertex gives vert_target = -1,
 *    vert_sq = 0.  Else pixel (i, j) = (floorf(u), floorf(v)), each clamped into the image; if that pixel is set in the mask, or the
 *    frame's mask is empty: (-1, 0); else t = T_mask.nearest there = j_t W + i_t, r = (u - ((float) i_t + 0.5), v - ((float) j_t +
 *    0.5)), vert_sq = r.x r.x + r.y r.y, vert_target = t.  Units: px^2.
 *  - mask -> model, per pixel (the body should cover the target): for a pixel q that is set in the mask and not covered,
 *    pix_source = s = T_cov.nearest at q and pix_sq = (float) T_cov.sqdist at q; every other pixel, and every pixel of a frame without
 *    coverage: (-1, 0).
 *  - vert_target [n,V] int64, vert_sq [n,V], pix_source [n,H,W] int64, pix_sq [n,H,W]: each may be NULL, not all four.  The bits do
 *    not depend on n, on the frame's position in the batch, on the memory space or on how the work is split.
 *  - SMPLPP_ERR_INVALID: as smplpp_depth_raster, and a host-space face id outside [-1, F) (the outputs are untouched).  Device data
 *    is never refused: NaN vertices are refused vertices.
 *  - the handle keeps 4 bytes per (frame, pixel) of workspace (the two column passes), grown to the largest call. */
int smplpp_silhouette(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, const float * camera /*[n,16]*/, int64_t H, int64_t W,
                      float near, const int64_t * face /*[n,H,W]*/, const uint8_t * mask /*[n,H,W]*/,
                      int64_t * vert_target /*[n,V] nullable*/, float * vert_sq /*[n,V] nullable*/,
                      int64_t * pix_source /*[n,H,W] nullable*/, float * pix_sq /*[n,H,W] nullable*/, int space, void * stream);
/* Vector-Jacobian product of vert_sq and pix_sq above to the world-space vertices at the correspondences the forward chose
 * (vert_target, pix_source and face held fixed; the mask itself is not read: the correspondences carry what it decided).  With
 * pull(x, k) = R^T J^T k at the camera-space point x, in fp32: jx = (fx k.x) / x.z, jy = (fy k.y) / x.z, jz = -((jx x.x + jy x.y) /
 * x.z), world component a = (R[a] jx + R[3+a] jy) + R[6+a] jz:
 *  - vertex term: vertex v with target t >= 0 and g = grad_vert_sq != 0, not refused by the vertex rule: r as in the forward, its
 *    term is pull(xc_v, ((2 g) r.x, (2 g) r.y)).
 *  - pixel term: pixel q with source s >= 0 and g = grad_pix_sq != 0, f = face[s]: the corners of f in camera space, the plane n,
 *    na, the ray d of pixel s, depth = na / nd and the barycentrics beta of the hit point y = (depth d.x, depth d.y, depth) as the
 *    rasteriser states them; the function differentiated is |pi(sum_i beta_i x_i) - c_q|^2 with beta, f, s held fixed (pix_sq at
 *    the point of evaluation, up to the rounding of beta); w = pull(y, ((2 g) (float)(i_s - i_q), (2 g) (float)(j_s - j_q))) and
 *    corner i of f receives beta_i w (each component one product).
 *  - each element of grad_verts is one fixed-order sum: the vertex's pixel shares in ascending linear index of q, then corner,
 *    starting from +0; then its own term is added; then accumulate = 0 stores the sum (untouched vertices get 0), 1 adds it to
 *    grad_verts.  No floating-point atomics; the bits do not depend on n or on the frame's position in the batch.
 *  - a cotangent of exactly 0 or an id of -1 contributes nothing, even on NaN data; in device space a target or source outside
 *    [0, H W), or a source whose face is -1 or outside [0, F), contributes nothing.  grad_vert_sq [n,V] (with vert_target) or
 *    grad_pix_sq [n,H,W] (with pix_source) may be NULL, not both.  No gradient to camera or mask.
 *  - SMPLPP_ERR_INVALID: as the forward, accumulate not 0 or 1, a host-space face id outside [-1, F), a host-space vert_target or
 *    pix_source outside [-1, H W) (the output is untouched).
 *  - with grad_pix_sq the handle keeps a record workspace of 64 bytes per (frame, pixel) (the live records are compacted per frame
 *    in pixel order; their count is on the device when the call is enqueued) and 12 bytes per (frame, vertex), grown to the largest
 *    call and held until the model is destroyed. */
int smplpp_silhouette_vjp(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, const float * camera /*[n,16]*/, int64_t H,
                          int64_t W, float near, const int64_t * face /*[n,H,W]*/, const int64_t * vert_target /*[n,V] nullable*/,
                          const int64_t * pix_source /*[n,H,W] nullable*/, const float * grad_vert_sq /*[n,V] nullable*/,
                          const float * grad_pix_sq /*[n,H,W] nullable*/, float * grad_verts /*[n,V,3]*/, int accumulate, int space,
                          void * stream);
/* ------------------------------------------------------------------ FIXED-ORDER SUMS
 * The energies and shared gradients of the sections below are each ONE fixed-order sum in fp32, every addition rounded on its own, by
 * one of two rules over an index k < N that the call names:
 *    sum64:    element k goes to partial k mod 64, the partials summed in ascending k starting from +0; then the 64 partials p_i meet
 *              as p_i = p_i + p_(i xor s) for s = 32, 16, 8, 4, 2, 1, and the sum is p_0.
 *    sum1024:  the same with 1024 partials, the meeting continued by s = 512, 256, 128, 64.
 * A partial that no element reaches is +0 and one that elements reach is never -0, so how a call splits the work over its threads
 * changes no bit.  For N <= 64 the two rules coincide; from 65 on they do not. */
/* ------------------------------------------------------------------ keypoints: landmark regression, projection, 2-D energy
 * A landmark regressor is a CSR matrix of L rows over V + 24 source columns: column c < V is vertex c, column V + j is joint j of
 * smplpp_fk's `joints`.  One regressor so expresses the 24 joints, vertex picks (nose, ears, toes) and sparse rows over the vertices
 * (H36M- or COCO-style joints); its two gradients are the grad_verts and grad_joints smplpp_fk_vjp and smplpp_fk_rotmat_vjp take.
 * row_ptr [L+1], col [nnz = row_ptr[L]], val [nnz] are host pointers, like the arrays of smplpp_model_create; a column may repeat
 * within a row (it is summed like any other entry), a row may be empty.  The handle copies what it needs of the model (V, the device):
 * it may outlive it.  Creation builds, on the host, the CSR with int32 columns and the transposed lists (per source, its entries in
 * ascending e), and uploads them once.
 *  - SMPLPP_ERR_INVALID: L outside [1, 65535], row_ptr[0] != 0, row_ptr not non-decreasing, a column outside [0, V + 24), a val that
 *    is not finite, nnz beyond int32 indexing (*out = NULL). */
int smplpp_landmarks_create(smplpp_model * m, int64_t L, const int64_t * row_ptr /*[L+1]*/, const int64_t * col /*[nnz]*/,
                            const float * val /*[nnz]*/, struct smplpp_landmarks ** out);
int smplpp_landmarks_destroy(struct smplpp_landmarks * lm);
int smplpp_landmarks_info(const struct smplpp_landmarks * lm, int64_t * L, int64_t * nnz);
/* points [n,L,3] = A [verts; joints].  In fp32 with every operation rounded on its own (no FMA), per (frame, row l, component): entry
 * e of the row has rank r = e - row_ptr[l]; partial p = r mod 8 runs s_p = s_p + val[e] * x[col[e]] over its entries in ascending r,
 * starting from +0; the result is ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7)).  An empty row gives +0.  The bits of a frame do
 * not depend on n, on its position in the batch, on the memory space or on the work split.
 * Column V + j reads row j of WHATEVER [n,24,3] array is passed as `joints`: smplpp_fk's rest joints, or the `posed` of
 * smplpp_skeleton, which makes those columns the posed skeleton; the grad_joints smplpp_landmarks_vjp returns is then the
 * grad_posed of smplpp_skeleton_vjp.
 *  - SMPLPP_ERR_INVALID: n <= 0, a NULL array, n (V + 24) or n L 3 beyond int32 indexing (the output is untouched). */
int smplpp_landmarks(struct smplpp_landmarks * lm, int64_t n, const float * verts /*[n,V,3]*/, const float * joints /*[n,24,3]*/,
                     float * points /*[n,L,3]*/, int space, void * stream);
/* Vector-Jacobian product of smplpp_landmarks.  Each element of grad_verts [n,V,3] and grad_joints [n,24,3] is one sequential sum,
 * starting from +0, of val[e] * grad_points[l(e)] over the entries e that name that source, in ascending e; then accumulate = 0 stores
 * it (untouched sources get 0) and 1 adds it to the output.  No floating-point atomics; the same independence as the forward.  Either
 * output may be NULL, not both.
 *  - SMPLPP_ERR_INVALID: as the forward, accumulate not 0 or 1, both outputs NULL (the outputs are untouched). */
int smplpp_landmarks_vjp(struct smplpp_landmarks * lm, int64_t n, const float * grad_points /*[n,L,3]*/, float * grad_verts /*[n,V,3] nullable*/,
                         float * grad_joints /*[n,24,3] nullable*/, int accumulate, int space, void * stream);
/* Projection of any points [n,K,3] (K = L for landmarks, K = V for raw vertices) and a 2-D keypoint energy against target [n,K,3] =
 * (u, v, confidence).  camera [n,16] and the projection are smplpp_depth_raster's vertex rule, unchanged: the same operations and the
 * same refusal (xc finite, xc.z > near, the guard band).  A refused point gives valid = 0, uv = (0, 0), energy = 0; else valid = 1 and
 * uv is the unsnapped (u, v).  Energy, in fp32 with every operation rounded on its own, with c = the target's confidence:
 *    c == 0: 0, and nothing else of the target row is read into the result, even on NaN data;
 *    else r = (u - tu, v - tv), q = r.x r.x + r.y r.y;  rho == 0: energy = (c c) q;
 *    rho > 0: p2 = rho rho, energy = (c c) ((p2 q) / (p2 + q))  (Geman-McClure on the squared pixel distance, as SMPLify has it).
 * uv [n,K,2], energy [n,K] (needs target), valid [n,K] bytes: each may be NULL, not all three.  Takes no handle: `device` as the stage
 * calls.  The bits do not depend on n, on the frame's position in the batch or on the memory space.
 *  - SMPLPP_ERR_INVALID: n or K <= 0, n K 3 beyond int32 indexing, near not finite or <= 0, rho < 0 or not finite, a NULL points or
 *    camera, energy without target (the outputs are untouched). */
int smplpp_project_points(int device, int64_t n, int64_t K, const float * points /*[n,K,3]*/, const float * camera /*[n,16]*/, float near,
                          const float * target /*[n,K,3]: u, v, confidence; nullable*/, float rho,
                          float * uv /*[n,K,2] nullable*/, float * energy /*[n,K] nullable, needs target*/, uint8_t * valid /*[n,K] nullable*/,
                          int space, void * stream);
/* Vector-Jacobian product of uv and energy above to the points and to the camera row: the library's gradient to the camera.  Per
 * live (not refused) point, in fp32, every operation rounded on its own:
 *    k = grad_uv (NULL reads as +0);  if grad_energy is given, g = grad_energy != 0 and c != 0: w = c c (rho == 0), else d = p2 /
 *    (p2 + q), w = (c c) (d d);  k.x = k.x + ((2 g) w) r.x, k.y likewise.  A NULL input, a g of exactly 0 or a confidence of 0
 *    contributes nothing, even on NaN data;
 *    jx = (fx k.x) / xc.z, jy = (fy k.y) / xc.z, jz = -((jx xc.x + jy xc.y) / xc.z)  (the pull of smplpp_silhouette_vjp);
 *    grad_points, world component a = (R[a] jx + R[3+a] jy) + R[6+a] jz; a refused point gets +0.
 *  - grad_camera [n,16] in the layout of camera, R as NINE INDEPENDENT ENTRIES (the convention of smplpp_fk_rotmat_vjp): R[3a+b] sums
 *    j_a * x_b with x the world point, t[a] sums j_a, fx sums k.x * (xc.x / xc.z), fy sums k.y * (xc.y / xc.z), cx sums k.x, cy sums
 *    k.y, over the live points of the frame.  Each of the 16 is sum64 (FIXED-ORDER SUMS above) over the frame's points k; a point
 *    that is not live is left out of its partial.
 *  - accumulate = 0 stores, 1 adds the finished value to the output, for both outputs.  grad_uv or grad_energy (needs target) may be
 *    NULL, not both; grad_points or grad_camera may be NULL, not both.  No floating-point atomics; the bits do not depend on n, on the
 *    frame's position in the batch, on the memory space or on which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: as the forward, accumulate not 0 or 1 (the outputs are untouched). */
int smplpp_project_points_vjp(int device, int64_t n, int64_t K, const float * points, const float * camera, float near,
                              const float * target /*nullable*/, float rho, const float * grad_uv /*[n,K,2] nullable*/,
                              const float * grad_energy /*[n,K] nullable, needs target*/, float * grad_points /*[n,K,3] nullable*/,
                              float * grad_camera /*[n,16] nullable*/, int accumulate, int space, void * stream);
/* ------------------------------------------------------------------ pose priors: max-mixture Gaussian and joint limits
 * One handle carries a mixture of M components over D pose coordinates and, optionally, per-coordinate limits: the two pose terms a
 * single-view fit pairs with the keypoint energy.  mean [M,D], mat [M,D,D] (row j gives output j), offset [M], lo, hi, limit_weight [D]
 * are host pointers, like the arrays of smplpp_landmarks_create.  With mat = sqrt(1/2) L^T, where the precision of component m is
 * L L^T, and offset[m] = -log w_m + 1/2 log det Sigma_m - (the least of these over m), the energy below is the negative log of the best
 * component up to a constant common to all of them.  lo, hi and limit_weight are all given or all NULL; +-inf in lo or hi means no limit
 * on that side.  M = 0 needs limits.  Creation validates the arrays on the host, makes the two device images of mat (as given, and
 * transposed) and uploads everything once.
 *  - SMPLPP_ERR_INVALID: M outside [0, 32], D outside [1, 128], M = 0 without limits, M > 0 with a NULL mean, mat or offset, only some
 *    of lo, hi, limit_weight, a mean, mat or offset that is not finite, a NaN in lo or hi, lo[k] > hi[k], a limit_weight that is
 *    negative or not finite (*out = NULL). */
int smplpp_pose_prior_create(int device, int64_t M, int64_t D, const float * mean /*[M,D]*/, const float * mat /*[M,D,D], row j = output j*/,
                             const float * offset /*[M]*/, const float * lo /*[D] nullable*/, const float * hi /*[D] nullable*/,
                             const float * limit_weight /*[D] nullable*/, struct smplpp_pose_prior ** out);
int smplpp_pose_prior_destroy(struct smplpp_pose_prior * prior);
int smplpp_pose_prior_info(const struct smplpp_pose_prior * prior, int64_t * M, int64_t * D, int * has_limits);
/* Both terms of n frames.  `pose` points at coordinate 0 of frame 0; frame i starts i ld floats later, ld >= D: the body pose of a
 * theta [n,25,3] buffer is (theta + 6, ld = 75, D = 69) with no copy.  A host-space call stages (n-1) ld + D floats.  In fp32 with every
 * operation rounded on its own (no FMA), per frame:
 *  mixture, per component m:  d_k = pose_k - mean[m][k];  y_j = sum_k mat[m][j][k] d_k, where partial p = k mod 8 runs s_p = s_p +
 *    mat[m][j][k] d_k in ascending k from +0 and y_j = ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7));  q_m = sum_j y_j y_j by
 *    sum64 (FIXED-ORDER SUMS above) over j;  e_m = q_m + offset[m].
 *    The component starts at 0 and, for m = 1 .. M-1 in order, is replaced when e_m < e_best: a tie goes to the lowest m, a NaN e_m
 *    never replaces and a NaN e_0 is never replaced.  energy [n] = e of the chosen component, component [n] = its index, residual
 *    [n,D] = its y (energy = |residual|^2 + offset[component]).
 *  limits:  per coordinate a = pose_k - hi_k, b = lo_k - pose_k, v = a if a > 0, else b if b > 0, else +0 (so a NaN pose_k gives 0, and
 *    a coordinate exactly at a limit contributes nothing);  limit_energy [n] = sum_k limit_weight_k (v v) by sum64 over k.
 * Each output may be NULL, not all four.  The bits of a frame do not depend on n, on its position in the batch, on the memory space, on
 * the work split or on which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: n <= 0, ld < D, a NULL pose, every output NULL, energy, component or residual on a prior with M = 0,
 *    limit_energy on a prior without limits, a bad space, n ld beyond int32 indexing (the outputs are untouched). */
int smplpp_pose_prior(struct smplpp_pose_prior * prior, int64_t n, const float * pose, int64_t ld, float * energy /*[n] nullable*/,
                      int64_t * component /*[n] nullable*/, float * residual /*[n,D] nullable*/, float * limit_energy /*[n] nullable*/,
                      int space, void * stream);
/* Vector-Jacobian product of energy, residual and limit_energy above to the pose; grad_pose has the rows of `pose` (the same ld), and
 * only its D coordinates per row are written: with accumulate = 1 it lands directly in a grad_theta buffer.  Per frame i, in fp32 with
 * every operation rounded on its own:
 *  mixture (when grad_energy or grad_residual is given):  the component is component[i] when that array is given, else it is chosen
 *    as in the forward (the selection has no gradient);  v_j = (2 g) y_j with g = grad_energy[i], y recomputed by the forward's rule,
 *    or +0 when grad_energy is NULL or g is exactly 0, even on NaN data;  then v_j = v_j + grad_residual[i][j] when that is given;
 *    t_k = sum_j mat[m][j][k] v_j by the 8-partial rule over j.  A device-space component outside [0, M) gives t = +0.
 *  limits (when grad_limit_energy is given):  u_k = ((2 g_l) limit_weight_k) a on the upper side, -(((2 g_l) limit_weight_k) b) on the
 *    lower side, +0 when g_l = grad_limit_energy[i] is exactly 0 or neither side is active.
 *  The element is t_k + u_k, or the one alone when the other part's cotangents are NULL; accumulate = 0 stores it, 1 adds it to the
 *  output.  No floating-point atomics; the same independence as the forward.
 *  - SMPLPP_ERR_INVALID: as the forward (cotangents for outputs), a NULL grad_pose, accumulate not 0 or 1, a host-space component
 *    outside [0, M) (the output is untouched).  Without a mixture cotangent `component` is not read, in either space. */
int smplpp_pose_prior_vjp(struct smplpp_pose_prior * prior, int64_t n, const float * pose, int64_t ld, const int64_t * component /*[n] nullable*/,
                          const float * grad_energy /*[n] nullable*/, const float * grad_residual /*[n,D] nullable*/,
                          const float * grad_limit_energy /*[n] nullable*/, float * grad_pose /*rows of ld*/, int accumulate, int space,
                          void * stream);
/* ------------------------------------------------------------------ a batched L-BFGS with a device-side line search
 * One handle optimises n independent frames of D unknowns each.  Every frame has its own history of at most m pairs, its own step
 * length, line-search state and status; all of it stays on the device between calls.  The caller evaluates energies f [n] and gradients
 * g (rows of ld_g floats) at the points x it holds (rows of ld_x floats, D coordinates per row touched, the convention of
 * smplpp_pose_prior: (theta + 3, ld = 75, D = 72) optimises rotation and pose inside a theta buffer), and smplpp_lbfgs_step consumes
 * them and overwrites x with the next points to evaluate: one kernel launch per evaluation, nothing read back.  Options: c1 in (0, 1)
 * (1e-4 is usual), tol_grad >= 0 (1e-5), tol_f >= 0 (0 = off), max_ls in [1, 64] (20), curv_eps in [0, 1) (1e-10).
 *  - SMPLPP_ERR_INVALID: n or D <= 0, m outside [1, 32], n m D beyond int32 indexing, an option out of range or not finite
 *    (*out = NULL). */
int smplpp_lbfgs_create(int device, int64_t n, int64_t D, int64_t m, float c1, float tol_grad, float tol_f, int max_ls, float curv_eps,
                        struct smplpp_lbfgs ** out);
int smplpp_lbfgs_destroy(struct smplpp_lbfgs * opt);
int smplpp_lbfgs_info(const struct smplpp_lbfgs * opt, int64_t * n, int64_t * D, int64_t * m);
/* Every frame back to "not evaluated yet" (status 0, counters 0, an empty history), enqueued on `stream`. */
int smplpp_lbfgs_reset(struct smplpp_lbfgs * opt, void * stream);
/* One evaluation of every running frame.  In fp32 with every operation rounded on its own (no FMA).  sum(v) below is sum64 (FIXED-ORDER
 * SUMS above) over the frame's coordinates k.  `finite` means: f and every g_k are neither NaN nor +-inf.
 * gmax = max_k |g_k|.  A frame keeps x0, f0, g0 (its last accepted point), d, t, gtd, ls, a ring of at most m pairs (s_i, y_i, sy_i)
 * and gamma.  Per frame whose status is 0:
 *  first evaluation:  evaluations = 1; x0 = x, f0 = f.  Not finite: status 4.  Else gmax <= tol_grad: status 1.  Else g0 = g, d_k = -g_k,
 *    t = min(1, 1 / sum(|g_k|)), gtd = sum(g_k d_k), x_k = x0_k + t d_k, ls = 0.
 *  later:  evaluations + 1.  The trial is accepted iff finite and f <= f0 + (c1 t) gtd.
 *  accepted:  s_k = x_k - x0_k, y_k = g_k - g0_k, sy = sum(s_k y_k), yy = sum(y_k y_k).  When yy > 0 and sy > curv_eps yy the pair enters
 *    the ring with its sy (a full ring loses its oldest pair) and gamma = sy / yy.  Let fo = f0; then x0 = x, f0 = f, g0 = g;
 *    iterations + 1.  gmax <= tol_grad: status 1.  Else tol_f > 0 and fo - f <= tol_f max(max(|fo|, |f|), 1): status 2.  Else the
 *    two-loop recursion: q = g; for the pairs from the newest to the oldest, alpha_i = sum(s_ik q_k) / sy_i, then q_k = q_k - alpha_i
 *    y_ik;  r_k = gamma q_k (r = q with no pair);  from the oldest to the newest, c = alpha_i - sum(y_ik r_k) / sy_i, then r_k = r_k +
 *    c s_ik;  d_k = -r_k, gtd = sum(g_k d_k).  Unless gtd < 0: the ring is emptied, d_k = -g_k, gtd = -sum(g_k g_k).  Then t = 1,
 *    ls = 0, x_k = x0_k + d_k.
 *  rejected:  ls + 1.  ls > max_ls: status 3 and x = x0.  Else tn = 0.5 t; when f is finite and den = 2 ((f - f0) - gtd t) > 0:
 *    tn = -((gtd t) t) / den, raised to 0.1 t unless tn >= 0.1 t (so a NaN becomes 0.1 t), then lowered to 0.5 t if above.  t = tn,
 *    x_k = x0_k + t d_k.
 * Status: 0 running, 1 gradient tolerance met, 2 energy tolerance met, 3 line search exhausted, 4 not finite at the first evaluation.
 * A frame whose status is not 0 has its accepted point in x from the call in which it stopped; after that call its row of x, f and g
 * is neither read nor written by the kernel, whatever it holds.  The bits of a frame do not depend on n, on its slot in the batch, on
 * the memory space, on ld_x or ld_g, on what the other frames do or on the work split.  In device space the call enqueues one kernel
 * on `stream`: no allocation, no synchronisation.  A host-space call stages (n-1) ld + D floats of x and g and copies x back.
 *  - SMPLPP_ERR_INVALID: ld_x or ld_g < D, n ld beyond int32 indexing, a NULL x, f or g, a bad space (x and the state are untouched). */
int smplpp_lbfgs_step(struct smplpp_lbfgs * opt, float * x, int64_t ld_x, const float * f /*[n]*/, const float * g, int64_t ld_g, int space,
                      void * stream);
/* The state of every frame: status [n], iterations [n] (accepted steps), evaluations [n], all int32; f_best [n] = f0 and step [n] = t
 * (floats; before the first evaluation both are 0); running [1] int64 = the number of frames with status 0.  Each may be NULL, not all.
 *  - SMPLPP_ERR_INVALID: every output NULL, a bad space. */
int smplpp_lbfgs_state(struct smplpp_lbfgs * opt, int32_t * status, int32_t * iterations, int32_t * evaluations, float * f_best, float * step,
                       int64_t * running, int space, void * stream);
/* x0 of every frame into x (rows of ld_x floats, D per row written) and f0 into f [n] (nullable): what a caller needs when its
 * evaluation budget ends while some frames are in the middle of a line search.  A frame not evaluated yet is left as it is.
 *  - SMPLPP_ERR_INVALID: ld_x < D, n ld_x beyond int32 indexing, a NULL x, a bad space (the outputs are untouched). */
int smplpp_lbfgs_best(struct smplpp_lbfgs * opt, float * x, int64_t ld_x, float * f /*[n] nullable*/, int space, void * stream);
/* ------------------------------------------------------------------ L-BFGS problems that span groups of rows
 * A grouped handle holds P problems where smplpp_lbfgs_create holds n frames.  Problem p owns the rows row_start[p] .. row_start[p+1]-1 of
 * the caller's x and g (rows ld floats apart, D coordinates per row touched, as above); its unknown vector has N_p = (rows of p) D
 * elements, element j = r D + k being coordinate k of the problem's r-th row.  It has ONE history of at most m pairs of N_p elements, one
 * step length, one line search and one status: what a β shared by the frames of a sequence, a velocity term between consecutive frames or
 * one SMPL+D offset field need.  Problems of different lengths share a handle.  A vector shared by T frames of a θ buffer takes a row of
 * its own: a buffer [T+1, 75] whose last row carries β in its first 10 coordinates; the unused coordinates have gradient 0 and never move.
 * smplpp_lbfgs_step, _state, _best, _reset, _info and _destroy take such a handle unchanged: f and every array of _state (and f of _best)
 * have P entries, `running` counts problems, _info still reports n, D and m.
 * The rule of a grouped handle is the per-frame rule of smplpp_lbfgs_step word for word, applied to the problem's N elements (read
 * "problem" for "frame" and j < N for k), with one change: sum(v) is sum1024 (FIXED-ORDER SUMS above) over the
 * problem's elements j.  `finite` and gmax run over all N elements.  fp32 throughout, every operation rounded on its own, no FMA contraction, no atomics.  A
 * grouped handle always uses this rule, also for a problem of one row, whose bits therefore differ from those of the same row on a handle
 * from smplpp_lbfgs_create: per-frame fits belong on the ungrouped handle (one wavefront a frame; a problem here costs a workgroup of 1024).
 * The bits of a problem depend on nothing but the problem: not on P, on its slot, on the lengths of the other problems, on the memory
 * space, on ld_x or ld_g, or on what the other problems do.  After the call in which a problem stops, none of its rows in x and g and not
 * its entry of f is read or written.  One kernel launch per smplpp_lbfgs_step, one workgroup per problem.
 *  - SMPLPP_ERR_INVALID (*out = NULL): P <= 0, a NULL row_start, row_start[0] != 0, a row_start that does not strictly increase,
 *    row_start[P] != n, and what smplpp_lbfgs_create refuses. */
int smplpp_lbfgs_create_grouped(int device, int64_t n, int64_t D, int64_t m, int64_t P, const int64_t * row_start /*[P+1], host*/, float c1,
                                float tol_grad, float tol_f, int max_ls, float curv_eps, struct smplpp_lbfgs ** out);
/* The groups of a handle: *P (nullable) and row_start [P+1] (host, nullable).  A handle from smplpp_lbfgs_create reports P = n and
 * row_start = 0 .. n. */
int smplpp_lbfgs_groups(const struct smplpp_lbfgs * opt, int64_t * P, int64_t * row_start /*[P+1] host, nullable*/);
/* ------------------------------------------------------------------ sequence terms: temporal smoothness, shared rows and group sums
 * What makes the rows of a grouped problem a sequence.  A layout handle is built from the optimiser's grouping (row_start, exactly what
 * smplpp_lbfgs_groups returns): problem p owns the rows row_start[p] .. row_start[p+1]-1, and its last shared_rows rows (0 or 1) are not
 * frames: the recipe above, a buffer [T+1, 75] whose last row carries beta.  Frames are numbered compactly in row order: F = rows - P
 * shared_rows, problem p owns the frames frame_start[p] .. frame_start[p+1]-1 with frame_start[p+1] - frame_start[p] = rows_p -
 * shared_rows, and every frame-side array below is compact [F, ...].  Creation validates on the host and uploads four small tables.
 * All five calls below are fp32 with every operation rounded on its own (no FMA), without floating-point atomics, and every output
 * element is one fixed-order sum.  sum1024(v) is that rule (FIXED-ORDER SUMS above) over the frame's index j within its problem, or over
 * the point k of a frame.  The bits of a problem depend on nothing but that problem: not on P, on
 * its slot, on the other problems' lengths, on the memory space, on ld, on the work split or on which outputs are asked for.
 *  - SMPLPP_ERR_INVALID (*out = NULL): P <= 0, what smplpp_lbfgs_create_grouped refuses for row_start, more rows than int32 indexes,
 *    shared_rows not 0 or 1, a problem with no frame beside its shared row. */
int smplpp_sequence_create(int device, int64_t P, const int64_t * row_start /*[P+1], host*/, int shared_rows /*0 or 1*/,
                           struct smplpp_sequence ** out);
int smplpp_sequence_destroy(struct smplpp_sequence * seq);
int smplpp_sequence_info(const struct smplpp_sequence * seq, int64_t * P, int64_t * rows, int64_t * frames, int * shared_rows,
                         int64_t * frame_start /*[P+1] host, nullable*/);
/* The optimiser buffer (rows ld floats apart) -> the per-frame arrays, in one launch: frames[f] = rows[row of f][off_f .. off_f + C_f),
 * shared[f] = rows[the shared row of f's problem][0 .. C_s).  With (off_f, C_f, C_s) = (0, 75, 10) these are theta [F,25,3] and beta
 * [F,10], the inputs of smplpp_fk.  The copies are bit-exact, whatever the other floats of a row hold.  A host-space call stages the rows
 * up to the last float read.
 *  - SMPLPP_ERR_INVALID: a NULL seq or rows, both outputs NULL, ld <= 0, rows ld beyond int32 indexing; with frames: off_f < 0, C_f < 1,
 *    off_f + C_f > ld; with shared: a layout with shared_rows = 0, C_s < 1, C_s > ld; outputs beyond int32 indexing; a bad space (the
 *    outputs are untouched).  The arguments of an output that is NULL are not read. */
int smplpp_sequence_split(struct smplpp_sequence * seq, const float * rows, int64_t ld, int64_t off_f, int64_t C_f,
                          float * frames /*[F,C_f] nullable*/, int64_t C_s, float * shared /*[F,C_s] nullable, needs shared_rows = 1*/, int space,
                          void * stream);
/* Its vector-Jacobian product.  ALL D coordinates of every row of grad_rows (rows ld floats apart, D <= ld: what smplpp_lbfgs_step
 * reads) are written: a frame row gets grad_frames[f] in [off_f, off_f + C_f) and +0 elsewhere (+0 everywhere when grad_frames is NULL);
 * a shared row gets, per coordinate c < C_s, sum1024 over the problem's frames j of grad_shared[frame_start[p] + j][c], and +0 elsewhere
 * (+0 everywhere when grad_shared is NULL).  accumulate = 0 stores the element, 1 adds it to what is there.
 *  - SMPLPP_ERR_INVALID: a NULL seq or grad_rows, both inputs NULL, D < 1, D > ld, rows ld beyond int32 indexing; with grad_frames:
 *    off_f < 0, C_f < 1, D < off_f + C_f; with grad_shared: a layout with shared_rows = 0, C_s < 1, D < C_s; inputs beyond int32
 *    indexing; accumulate not 0 or 1; a bad space (the output is untouched). */
int smplpp_sequence_merge(struct smplpp_sequence * seq, const float * grad_frames /*[F,C_f] nullable*/, int64_t off_f, int64_t C_f,
                          const float * grad_shared /*[F,C_s] nullable*/, int64_t C_s, float * grad_rows, int64_t ld, int64_t D, int accumulate,
                          int space, void * stream);
/* problem_values[p] = scale * sum1024 over the problem's frames j of frame_values[frame_start[p] + j]; with accumulate = 1 that product
 * is added to what is there, so a caller folds several terms into the f [P] of smplpp_lbfgs_step one call each.
 *  - SMPLPP_ERR_INVALID: a NULL seq, frame_values or problem_values, accumulate not 0 or 1, a bad space (the output is untouched). */
int smplpp_sequence_sum(struct smplpp_sequence * seq, const float * frame_values /*[F]*/, float scale, float * problem_values /*[P]*/,
                        int accumulate, int space, void * stream);
/* The temporal term.  Frame f of x is K points of C coordinates at x + f ld, ld >= K C, 1 <= C <= 16: joints [F,24,3] are (joints, 72,
 * 24, 3), the rotations of a theta buffer (theta + 3, 75, 24, 3) with no copy, vertices (verts, 3V, V, 3), rotation matrices (rot, 216,
 * 24, 9).  A stencil never crosses a problem boundary.  Per frame f and point k, with x[f] short for the point's C coordinates:
 *  order 1:  a stencil exists at f when f+1 is in f's problem;  d_c = x[f+1]_c - x[f]_c.
 *  order 2:  a stencil exists at f when f-1 and f+1 are both in f's problem;  d_c = (x[f+1]_c - x[f]_c) - (x[f]_c - x[f-1]_c).
 *  q = sum_c d_c d_c in ascending c from +0;  w = weight[k] (NULL reads as 1).  Without a stencil or with w == 0: e = +0, and nothing of
 *  x reaches the result, even NaN.  Else rho == 0: e = w q;  rho > 0: p2 = rho rho, e = w ((p2 q) / (p2 + q)), the Geman-McClure form of
 *  smplpp_project_points.
 * point_energy [F,K] = e;  frame_energy [F] = sum1024 of e over k.  Either may be NULL, not both.  A host-space call stages (F-1) ld +
 * K C floats of x.
 *  - SMPLPP_ERR_INVALID: a NULL seq or x, K <= 0, C outside [1, 16], ld < K C, order not 1 or 2, rho negative or not finite, a
 *    host-space weight that is negative or not finite, every output NULL, F ld beyond int32 indexing, a bad space (the outputs are
 *    untouched). */
int smplpp_sequence_smoothness(struct smplpp_sequence * seq, const float * x, int64_t ld, int64_t K, int64_t C, int order /*1 or 2*/,
                               const float * weight /*[K] nullable*/, float rho, float * frame_energy /*[F] nullable*/,
                               float * point_energy /*[F,K] nullable*/, int space, void * stream);
/* Its vector-Jacobian product to x; grad_x has the rows of x (the same ld), and only the K C coordinates of a row are written: with
 * accumulate = 1 it lands directly in a grad_theta buffer.  A gather: each output element recomputes the at most three stencils that
 * touch it.  For the stencil at frame h and point k:  g = grad_frame_energy[h] (NULL: +0), plus grad_point_energy[h,k] when given;
 * v_c = +0 when g is exactly 0, when w == 0 or when there is no stencil at h, even on NaN data;  else s = (2 g) w for rho == 0, and for
 * rho > 0 t = p2 / (p2 + q), s = ((2 g) w) (t t);  v_c = s d_c.  Then, an absent stencil (or a frame outside the problem) reading as +0:
 *  order 1:  grad_x[f,k,c] = v[f-1]_c - v[f]_c.
 *  order 2:  grad_x[f,k,c] = (v[f-1]_c + v[f+1]_c) - (2 v[f]_c).
 * accumulate = 0 stores the element, 1 adds it to what is there.
 *  - SMPLPP_ERR_INVALID: as the forward (cotangents for outputs), a NULL grad_x, accumulate not 0 or 1 (the output is untouched). */
int smplpp_sequence_smoothness_vjp(struct smplpp_sequence * seq, const float * x, int64_t ld, int64_t K, int64_t C, int order,
                                   const float * weight /*[K] nullable*/, float rho, const float * grad_frame_energy /*[F] nullable*/,
                                   const float * grad_point_energy /*[F,K] nullable*/, float * grad_x /*rows of ld*/, int accumulate, int space,
                                   void * stream);
/* ------------------------------------------------------------------ the scene term: trilinear SDF volumes, penetration and contact
 * Where the body is relative to what is not the body.  A volume handle holds a signed-distance grid of a static scene on the device:
 * node (i, j, k), i < Gx, j < Gy, k < Gz, holds values[(k Gy + j) Gx + i] and sits at origin + (i hx, j hy, k hz) in VOLUME coordinates;
 * world_to_volume [12] is a row-major [R|t] (R[0..8], t[0..2] below; NULL: the identity, and then no arithmetic is done on a point).
 * `space` says where `values` lives (NULL: zeros); host-space values are not inspected, so a NaN node is legal.  The grid is stored in
 * one of two layouts, `linear` (the array as given) or `cells` (one 32-byte record of its eight nodes per cell; 8 x the memory, and only
 * while the records fit 1 GiB: above that the handle is linear); SMPLPP_VOLUME_LAYOUT=linear|cells, read at creation, forces one, and
 * NO OUTPUT BIT DEPENDS ON THE LAYOUT.  smplpp_volume_info reports it as 0 (linear) or 1 (cells); every output of info is nullable.
 *  - SMPLPP_ERR_INVALID (*out = NULL): a NULL out, a G outside [2, 1024], Gx Gy Gz > 2^27, a NULL origin or spacing, a spacing that is not
 *    finite and positive, a non-finite origin or transform entry, a bad space, an unknown value of SMPLPP_VOLUME_LAYOUT. */
int smplpp_volume_create(int device, int64_t Gx, int64_t Gy, int64_t Gz, const float origin[3], const float spacing[3],
                         const float * world_to_volume /*[12] row-major [R|t], nullable = identity*/,
                         const float * values /*[Gz,Gy,Gx], nullable: zeros*/, int space, struct smplpp_volume ** out);
/* New node values into the handle's layout.  In device space it is one kernel on `stream`, with no allocation and no synchronisation:
 * a grid can be refreshed inside an optimisation loop (from the signed distances of another body, say).
 *  - SMPLPP_ERR_INVALID: a NULL vol or values, a bad space (the grid is untouched). */
int smplpp_volume_set(struct smplpp_volume * vol, const float * values /*[Gz,Gy,Gx]*/, int space, void * stream);
int smplpp_volume_info(const struct smplpp_volume * vol, int64_t G[3], float origin[3], float spacing[3], float world_to_volume[12],
                       int * layout);
int smplpp_volume_destroy(struct smplpp_volume * vol);
/* THE SAMPLING RULE, for the world point p = (x, y, z).  All arithmetic is fp32, every operation rounded on its own (no FMA).
 *  transform:   p'_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a];  without a transform p' = p.
 *  coordinate:  g_a = (p'_a - origin_a) / h_a, a true division.
 *  inside:      every g_a is finite and 0 <= g_a <= G_a - 1.
 *  cell:        i_a = min((int)floor(g_a), G_a - 2),  f_a = g_a - (float)i_a: the far face belongs to the last cell with f = 1.
 *  value:       with v_xyz the node (i_x + x, i_y + y, i_z + z):  d_yz = v_1yz - v_0yz,  c_yz = v_0yz + f_x d_yz;
 *               e_z = c_1z - c_0z,  c_z = c_0z + f_y e_z;  s = c_0 + f_z (c_1 - c_0).
 *  gradient in volume coordinates:  x_z = d_0z + f_y (d_1z - d_0z),  g_x = (x_0 + f_z (x_1 - x_0)) / h_x;
 *               g_y = (e_0 + f_z (e_1 - e_0)) / h_y;  g_z = (c_1 - c_0) / h_z.  It is the derivative of the interpolant at a fixed cell.
 *  gradient in world coordinates:  (R[a] g_x + R[3+a] g_y) + R[6+a] g_z (the pull of smplpp_project_points_vjp, right for any affine
 *               transform); without a transform it is (g_x, g_y, g_z) as it stands.
 *  valid:       1 when the point is inside and s is finite.  A point that is not valid gives value +0, gradient +0, energy +0 and
 *               contributes to no gradient: the convention of refused points in smplpp_project_points.  A NaN node therefore takes out
 *               the points of the (at most eight) cells that touch it and no others.
 * points [n,K,3]; value [n,K], gradient [n,K,3] (d value / d world point) and valid [n,K] may each be NULL, not all.  A thread per point.
 *  - SMPLPP_ERR_INVALID: a NULL vol or points, n or K <= 0, n K 3 beyond int32 indexing, every output NULL, a bad space (the outputs are
 *    untouched). */
int smplpp_volume_sample(struct smplpp_volume * vol, int64_t n, int64_t K, const float * points /*[n,K,3]*/, float * value /*[n,K] nullable*/,
                         float * gradient /*[n,K,3] nullable*/, uint8_t * valid /*[n,K] nullable*/, int space, void * stream);
/* THE TERM.  wp = w_pen[k] (NULL reads as 1), wc = w_con[k] (NULL reads as 0).  Per valid point, with s its sample and q = s s:
 *  penetration:  e_pen = wp q when s < 0, else +0;
 *  contact:      e_con = wc q for rho == 0, else p2 = rho rho, e_con = wc ((p2 q) / (p2 + q)), the Geman-McClure form of
 *                smplpp_project_points;
 *  point_energy = e_pen + e_con.  A point with wp == 0 and wc == 0 reads no grid value and its energy is +0, whatever the grid holds
 *  there; its value and valid outputs, when asked for, are still computed.
 * energy [n] = sum1024 (FIXED-ORDER SUMS above) of point_energy over the frame's points k.  The work
 * split follows K (a wavefront per frame up to 64, a workgroup of 256 up to 1024, of 1024 above; a thread per point without energy) and
 * changes no bit; nor do n, the frame's slot, the memory space, the layout or which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: as smplpp_volume_sample, rho negative or not finite (the outputs are untouched). */
int smplpp_scene_term(struct smplpp_volume * vol, int64_t n, int64_t K, const float * points /*[n,K,3]*/, const float * w_pen /*[K] nullable = 1*/,
                      const float * w_con /*[K] nullable = 0*/, float rho, float * energy /*[n] nullable*/, float * point_energy /*[n,K] nullable*/,
                      float * value /*[n,K] nullable*/, uint8_t * valid /*[n,K] nullable*/, int space, void * stream);
/* Its vector-Jacobian product to the points, a thread per point with the sample recomputed by the forward's operations; no sums.  A NULL
 * cotangent reads as +0.  Per valid point:
 *  g = grad_energy[f] + grad_point_energy[f,k];
 *  dE/ds = pen + con,  pen = (2 wp) s when s < 0, else +0;  con = (2 wc) s for rho == 0, else d = p2 / (p2 + q), con = ((2 wc) (d d)) s;
 *  t = g dE/ds, or +0 when wp == 0 and wc == 0;  kk = grad_value[f,k] + t;  grad_points[f,k,a] = kk (the world gradient)_a.
 * A point that is not valid, or one with wp == 0 and wc == 0 under a NULL grad_value (it reads no grid value), gets +0.  accumulate = 0
 * stores the element, 1 adds it to what is there.
 *  - SMPLPP_ERR_INVALID: as the forward (cotangents for outputs), a NULL grad_points, accumulate not 0 or 1 (the output is untouched). */
int smplpp_scene_term_vjp(struct smplpp_volume * vol, int64_t n, int64_t K, const float * points, const float * w_pen, const float * w_con,
                          float rho, const float * grad_energy /*[n] nullable*/, const float * grad_point_energy /*[n,K] nullable*/,
                          const float * grad_value /*[n,K] nullable*/, float * grad_points /*[n,K,3]*/, int accumulate, int space,
                          void * stream);
/* ------------------------------------------------------------------ the image term: bilinear sampling at projected points
 * A dense image that a network produced (joint heatmaps, feature or colour maps, flow, a distance map) read at the unsnapped uv [n,K,2]
 * of smplpp_project_points, with the gradient to uv and to the image.  image [B,H,W,C] is channels-last, as smplpp_raster_interpolate
 * writes it; B, Tn and Wn are each 1 (shared by all frames) or n.  Without `channel` a point samples all C channels (Cs = C); with
 * channel [K], point k samples channel channel[k] alone (Cs = 1: heatmap j for joint j).  The calls take no handle: `device` as the
 * stage calls.  All arithmetic is fp32, every operation rounded on its own (no FMA), and there are no floating-point atomics.
 * THE SAMPLING RULE, for the point (u, v):
 *  coordinate:  pixel (row j, column i) has its centre at (i + 0.5, j + 0.5), the convention of smplpp_depth_raster and
 *               smplpp_project_points: gx = u - 0.5, gy = v - 0.5.
 *  inside:      both are finite, 0 <= gx <= W - 1 and 0 <= gy <= H - 1.
 *  cell:        i = min((int)floor(gx), W - 2), fx = gx - (float)i;  j, fy alike from gy and H: the far edge belongs to the last cell
 *               with f = 1.
 *  value:       per sampled channel c, with v_xy the pixel (j + y, i + x):  d_y = v_1y - v_0y,  c_y = v_0y + fx d_y;  e = c_1 - c_0,
 *               s = c_0 + fy e.
 *  gradient:    ds/du = d_0 + fy (d_1 - d_0),  ds/dv = e, in pixels: the derivative of the interpolant at a fixed cell.
 *  valid:       1 when the point is inside and every sampled s is finite.  A point that is not valid gives +0 in every output and
 *               contributes to no gradient: the convention of smplpp_volume_sample.  A NaN pixel therefore takes out the points of the
 *               (at most four) cells that touch it and no others.  A device-space channel[k] outside [0, C) makes the point not valid.
 * value [n,K,Cs], gradient [n,K,Cs,2] = (ds/du, ds/dv) and valid [n,K] may each be NULL, not all.  A thread per point.
 *  - SMPLPP_ERR_INVALID: n or K <= 0, H or W outside [2, 8192], C outside [1, 32], B not 1 or n, n K Cs 2 or B H W C beyond int32
 *    indexing, a NULL uv or image, every output NULL, a bad space, a host-space channel entry outside [0, C) (the outputs are
 *    untouched).  Device data is never refused. */
int smplpp_image_sample(int device, int64_t n, int64_t K, const float * uv /*[n,K,2]*/, const float * image /*[B,H,W,C]*/, int64_t B, int64_t H,
                        int64_t W, int64_t C, const int64_t * channel /*[K] nullable*/, float * value /*[n,K,Cs] nullable*/,
                        float * gradient /*[n,K,Cs,2] nullable*/, uint8_t * valid /*[n,K] nullable*/, int space, void * stream);
/* THE TERM.  w = weight[f or 0][k] (NULL reads as 1), t_c = target[f or 0][k][c] (NULL reads as 0).  Per valid point:
 *  r_c = s_c - t_c;  q = the sum of r_c r_c over the sampled channels c, ascending from +0;
 *  point_energy = w q for rho == 0, else p2 = rho rho, point_energy = w ((p2 q) / (p2 + q)), the Geman-McClure form of
 *  smplpp_project_points.  A point with w == 0 reads no image value or target and its energy is +0, whatever they hold; its value and
 *  valid outputs, when asked for, are still computed.
 * energy [n] = sum1024 (FIXED-ORDER SUMS above) of point_energy over the frame's points k.  The work split follows K (a wavefront per
 * frame up to 64, a workgroup of 256 up to 1024, of 1024 above; a thread per point without energy) and changes no bit; nor do n, the
 * frame's slot, the memory space or which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: as smplpp_image_sample, a given target or weight with Tn or Wn not 1 or n, rho negative or not finite (the
 *    outputs are untouched). */
int smplpp_image_term(int device, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W, int64_t C,
                      const int64_t * channel /*[K] nullable*/, const float * target /*[Tn,K,Cs] nullable = 0*/, int64_t Tn,
                      const float * weight /*[Wn,K] nullable = 1*/, int64_t Wn, float rho, float * energy /*[n] nullable*/,
                      float * point_energy /*[n,K] nullable*/, float * value /*[n,K,Cs] nullable*/, uint8_t * valid /*[n,K] nullable*/,
                      int space, void * stream);
/* Its vector-Jacobian product to uv and to the image, with the sample recomputed by the forward's operations.  A NULL cotangent reads
 * as +0.  Per valid point:
 *  g = grad_energy[f] + grad_point_energy[f,k];  m = w for rho == 0, else d = p2 / (p2 + q), m = w (d d);
 *  gamma_c = grad_value[f,k,c] + ((2 g) m) r_c; when w == 0 the second term is +0 and nothing of the term is read.
 *  grad_uv[f,k] = (sum_c gamma_c ds_c/du, sum_c gamma_c ds_c/dv), each sum over c ascending from +0.  No sums across points.
 *  grad_image:  with ax = 1 - fx, ay = 1 - fy, the point contributes (ax ay) gamma_c, (fx ay) gamma_c, (ax fy) gamma_c and
 *  (fx fy) gamma_c to the pixels (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1) of its cell, in its sampled channels; a product that is 0
 *  is included.  Element (b, j, i, c) is the sum of its contributions, from +0, IN ASCENDING FLAT POINT INDEX f K + k over the frames
 *  that read image b (f = b when B = n, every f when B = 1): one fixed-order sum per element, a gather with no atomics.
 * A point that is not valid, or one with w == 0 under a NULL grad_value (it reads no image value), contributes nothing: +0 in grad_uv.
 * accumulate = 0 stores the finished value (untouched pixels get +0), 1 adds it to what is there, for both outputs.  grad_uv or
 * grad_image may be NULL, not both.  The bits do not depend on n, on the frame's slot (B = n), on the memory space or on which output is
 * asked for.  grad_image costs tiles x points (a workgroup per 16 x 16 pixels and 4 channels scans the points of its image).
 *  - SMPLPP_ERR_INVALID: as the forward (cotangents for outputs), both outputs NULL, accumulate not 0 or 1 (the outputs are
 *    untouched). */
int smplpp_image_term_vjp(int device, int64_t n, int64_t K, const float * uv, const float * image, int64_t B, int64_t H, int64_t W, int64_t C,
                          const int64_t * channel, const float * target, int64_t Tn, const float * weight, int64_t Wn, float rho,
                          const float * grad_energy /*[n] nullable*/, const float * grad_point_energy /*[n,K] nullable*/,
                          const float * grad_value /*[n,K,Cs] nullable*/, float * grad_uv /*[n,K,2] nullable*/,
                          float * grad_image /*[B,H,W,C] nullable*/, int accumulate, int space, void * stream);
/* ------------------------------------------------------------------ rigid and similarity alignment of point sets
 * Per frame, the rotation R, translation t and scale s that minimise sum_k w_k |s (R x_k) + t - y_k|^2 over source x [n,K,3], target
 * y [Tn,K,3] and weight w [Wn,K] (NULL reads as 1); Tn and Wn are each 1 (shared by all frames) or n.  It is closed form (Horn's
 * quaternion method), and so is its vector-Jacobian product.  The calls take no handle: `device` as the stage calls.  All arithmetic is
 * fp32, every operation rounded on its own (no FMA), '/' and sqrt are the correctly rounded ones, every sum over a frame's points is
 * sum1024 (FIXED-ORDER SUMS above), and there are no floating-point atomics.  Products and sums associate from the left as written.
 * THE FORWARD RULE, per frame:
 *  1 live:      point k is live iff w_k is finite and > 0 and its six coordinates are finite.  A point that is not live adds +0 to every
 *               sum below.  It is `moved` iff its three source coordinates are finite (a live point is).
 *  2 centroids: W = sum w;  cx_a = (sum w x_a) / W,  cy_a = (sum w y_a) / W;  x~ = x - cx,  y~ = y - cy, in a second pass.
 *  3 moments:   S_ab = sum (w x~_a) y~_b, nine sums;  vx = sum w ((x~_0 x~_0 + x~_1 x~_1) + x~_2 x~_2).
 *  4 matrix:    the symmetric N [4,4]:  N00 = (Sxx + Syy) + Szz,  N11 = (Sxx - Syy) - Szz,  N22 = ((-Sxx) + Syy) - Szz,
 *               N33 = ((-Sxx) - Syy) + Szz;  N01 = Syz - Szy,  N02 = Szx - Sxz,  N03 = Sxy - Syx,  N12 = Sxy + Syx,  N13 = Szx + Sxz,
 *               N23 = Syz + Szy.
 *  5 Jacobi:    V = I; SEVEN sweeps over the pairs (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3).  A pair with N_pq == 0 is skipped.
 *               Else theta = (N_qq - N_pp) / (2 N_pq);  t = sg / (|theta| + sqrt(theta theta + 1)), sg = -1 for theta < 0, else 1 (a
 *               theta theta that overflows gives t = 0, not a NaN);  c = 1 / sqrt(t t + 1);  s = t c;  h = t N_pq;  N_pp -= h;
 *               N_qq += h;  N_pq = 0;  for r not in {p, q}: (N_rp, N_rq) = (c N_rp - s N_rq, s N_rp + c N_rq), on the old values and
 *               kept symmetric;  for every r: (V_rp, V_rq) = (c V_rp - s V_rq, s V_rp + c V_rq).  lambda_i = N_ii, with column i of V.
 *  6 rotation:  `top` is the index of the largest lambda, the lowest on ties; e = column top of V;  q = e / sqrt(((e0 e0 + e1 e1) +
 *               e2 e2) + e3 e3) = (w, x, y, z);  R = [((ww + xx) - yy) - zz, 2 (xy - wz), 2 (xz + wy);  2 (xy + wz), ((ww - xx) + yy) - zz,
 *               2 (yz - wx);  2 (xz - wy), 2 (yz + wx), ((ww - xx) - yy) + zz], ww = w w and so on.  Always a proper rotation: a
 *               mirrored target gets the best rotation, as the SVD rule with the determinant correction does.
 *  7 scale:     s = (sum_ab R_ab S_ba, a outer, b inner, from the first product) / vx with with_scale, else 1;
 *               t_a = cy_a - s ((R_a0 cx_0 + R_a1 cx_1) + R_a2 cx_2).
 *  8 outputs:   aligned_k,a = s ((R_a0 x_0 + R_a1 x_1) + R_a2 x_2) + t_a for EVERY k, live or not (align on a subset, move everything);
 *               d = aligned_k - y_k;  point_error_k = (d_0 d_0 + d_1 d_1) + d_2 d_2, +0 where the point is not live;
 *               energy = sum w point_error;  gap = (l1 - l2) / (l1 - l4) for the largest, second and smallest lambda, 0 unless
 *               l1 - l4 > 0.  transform [n,13] = R row-major, t, s.
 *  9 status:    bit 0: W is not finite and > 0: the transform is the identity, energy and gap are 0 and no other bit is set.  That is
 *               a frame without a live point, and also one whose weights sum past the largest float: its live points then keep the
 *               point_error of the identity, and in the backward the direct part (2 ge w) (aligned - y) of such a frame still flows,
 *               as for every frame with a status bit.  Bit 1: vx == 0 (one live point, or coincident ones at weights whose centroid is exact): R = I, s = 1,
 *               t = cy - cx.  Bit 2: gap <= min_gap: the rotation is not unique; the transform is still the rule's.
 * Every output is nullable, not all.  The work split follows K (a wavefront per frame up to 64, a workgroup of 256 up to 1024, of 1024
 * above) and changes no bit; nor do n, the frame's slot, the memory space or which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: n or K <= 0, Tn or Wn not 1 or n, with_scale not 0 or 1, min_gap negative or not finite, a NULL source or
 *    target, every output NULL, n K 3 beyond int32 indexing, a bad space (the outputs are untouched).  Device data is never refused. */
int smplpp_align(int device, int64_t n, int64_t K, const float * source /*[n,K,3]*/, const float * target /*[Tn,K,3]*/, int64_t Tn,
                 const float * weight /*[Wn,K] nullable = 1*/, int64_t Wn, int with_scale, float min_gap,
                 float * transform /*[n,13] nullable*/, float * aligned /*[n,K,3] nullable*/, float * energy /*[n] nullable*/,
                 float * point_error /*[n,K] nullable*/, float * gap /*[n] nullable*/, int32_t * status /*[n] nullable*/, int space,
                 void * stream);
/* Its vector-Jacobian product to source and target, with the forward recomputed by the forward's operations.  A NULL cotangent reads as
 * +0; (gR [9], gt [3], gs) = grad_transform[f], R as nine independent entries (the convention of smplpp_fk_rotmat_vjp).  Per frame, with
 * ge = grad_energy[f], c2_k = (2 ge) w_k and d_k = aligned_k - y_k:
 *  ga_k = grad_aligned_k + c2_k d_k, the second term for live points only.
 *  sums:  sg_a = sum ga_a and P_ab = sum ga_a x_b over the MOVED points (a point of weight 0 is moved with the rest, and its cotangent
 *         reaches the transform), twelve sum1024.
 *  G_t = gt + sg;  rc = R cx (as in step 7);  G_s = (gs + sum_ab R_ab P_ab) - ((G_t0 rc_0 + G_t1 rc_1) + G_t2 rc_2), 0 without with_scale;
 *  G_R_ab = ((gR_ab + s P_ab) - (s G_t,a) cx_b) + (G_s S_ba) / vx;  g2 = 2 ((-(G_s s)) / vx).
 *  g_q = 2 M q, M the matrix of step 4 built from G_R^T in S's place, each row ((M_r0 w + M_r1 x) + M_r2 y) + M_r3 z.
 *  co_i = (((V_0i g_q0 + V_1i g_q1) + V_2i g_q2) + V_3i g_q3) / (lambda_top - lambda_i), +0 for i = top;
 *  u_r = ((V_r0 co_0 + V_r1 co_1) + V_r2 co_2) + V_r3 co_3;  D_i = u_i q_i,  H_ij = u_i q_j + u_j q_i;
 *  G_S: xx = ((D0 + D1) - D2) - D3, yy = ((D0 - D1) + D2) - D3, zz = ((D0 - D1) - D2) + D3, yz = H23 + H01, zy = H23 - H01,
 *       zx = H13 + H02, xz = H13 - H02, xy = H12 + H03, yx = H12 - H03;   G_M_ab = (G_s R_ab) / vx + G_S_ba;  cs = -(s (R^T G_t)).
 *  grad_source_k,a = s ((R_0a ga_0 + R_1a ga_1) + R_2a ga_2), and for a live point of a frame with status 0
 *       (that + w ((G_M^T y~)_a + g2 x~_a)) + (w / W) cs_a;
 *  grad_target_k,a = 0 - c2 d_a for a live point, else +0, and for a live point of a frame with status 0
 *       (that + w (G_M x~)_a) + (w / W) G_t,a.
 * The centring correction of the moment terms vanishes identically and is not computed.  A frame with any status bit set keeps its
 * transform constant.  grad_target is always per frame [n,K,3]: with Tn = 1 the caller sums it.  There is no gradient to the weights.
 * accumulate = 0 stores, 1 adds to what is there.  grad_source or grad_target may be NULL, not both.  The bits do not depend on n, the
 * frame's slot, the memory space or which output is asked for.
 *  - SMPLPP_ERR_INVALID: as the forward, every cotangent NULL, both outputs NULL, accumulate not 0 or 1 (the outputs are untouched). */
int smplpp_align_vjp(int device, int64_t n, int64_t K, const float * source, const float * target, int64_t Tn, const float * weight, int64_t Wn,
                     int with_scale, float min_gap, const float * grad_transform /*[n,13] nullable*/,
                     const float * grad_aligned /*[n,K,3] nullable*/, const float * grad_energy /*[n] nullable*/,
                     float * grad_source /*[n,K,3] nullable*/, float * grad_target /*[n,K,3] nullable*/, int accumulate, int space,
                     void * stream);
/* ------------------------------------------------------------------ the orientation term on world joint frames
 * What consumes the orientations smplpp_skeleton returns: per frame f and sensor s, the 3 x 3 block A of joint joint[s] in
 * frames [n,J,3,row_stride] against a target, through a constant bone-to-sensor offset.  frames is read in place: row_stride = 4 takes
 * smplpp_skeleton's `world` as it is (column 3 is never read, and never written in grad_frames), row_stride = 3 a stack of matrices
 * [n,J,3,3].  C = 3 compares whole orientations (an IMU), C = 1 or 2 the images of one or two bone-frame axes (a foot's up axis against
 * the ground normal, a gaze direction, gravity).  O = offset[s] [3,C] (NULL reads as the first C columns of the identity, with the bits
 * of passing them), T = target[f or 0][s] [3,C], w = weight[f or 0][s] (NULL reads as 1); Tn and Wn are each 1 (shared by all frames) or
 * n.  The calls take no handle and no workspace: `device` as the stage calls.  All arithmetic is fp32, every operation rounded on its
 * own (no FMA), '/' is the correctly rounded one, and there are no atomics.
 * THE FORWARD RULE, per live sensor:
 *  M_rc = (A_r0 O_0c + A_r1 O_1c) + A_r2 O_2c;   E = M - T, and residual = E;
 *  q = the sum of E_rc E_rc, row-major (r outer, c inner), ascending from +0;
 *  sensor_energy = w q for rho == 0, else p2 = rho rho, sensor_energy = w ((p2 q) / (p2 + q)), the Geman-McClure form of
 *  smplpp_image_term.  For rotations and C = 3, q = 4 (1 - cos phi), phi the geodesic angle between A O and T.
 * energy [n] = sum1024 (FIXED-ORDER SUMS above) of sensor_energy over the frame's sensors s.  The work split follows S (a wavefront per
 * frame up to 64, a workgroup of 256 up to 1024, of 1024 above; a thread per sensor without energy) and changes no bit.
 * DEAD SENSORS.  A sensor is dead when w is 0 or not finite, when joint[s] is outside [0, J) (nothing is read through it), or when any
 * of the 9 entries of A, the 3 C of O or the 3 C of T is not finite.  It gives +0 in every output and every gradient, and touches
 * neither its neighbours nor its frame's other sums.  (A negative finite weight is live.)
 * energy [n], sensor_energy [n,S] and residual [n,S,3,C] may each be NULL, not all.  The bits do not depend on n, on the frame's slot, on
 * the memory space or on which outputs are asked for.
 *  - SMPLPP_ERR_INVALID: n, J or S <= 0, C outside 1..3, row_stride not 3 or 4, Tn or Wn not 1 or n, rho negative or not finite, a NULL
 *    frames, joint or target, every output NULL, n J 12 or n S 9 beyond int32 indexing, a bad space (the outputs are untouched).  Device
 *    data is never refused. */
int smplpp_orientation_term(int device, int64_t n, int64_t J, int64_t row_stride /*3 or 4*/, const float * frames /*[n,J,3,row_stride]*/,
                            int64_t S, int64_t C /*1, 2 or 3*/, const int64_t * joint /*[S]*/, const float * offset /*[S,3,C] nullable*/,
                            const float * target /*[Tn,S,3,C]*/, int64_t Tn, const float * weight /*[Wn,S] nullable = 1*/, int64_t Wn,
                            float rho, float * energy /*[n] nullable*/, float * sensor_energy /*[n,S] nullable*/,
                            float * residual /*[n,S,3,C] nullable*/, int space, void * stream);
/* Its vector-Jacobian product to the frames, the offsets and the target, with the forward recomputed by the forward's operations.  A NULL
 * cotangent reads as +0.  Per live sensor:
 *  g = grad_energy[f] + grad_sensor_energy[f,s];  m = w for rho == 0, else d = p2 / (p2 + q), m = w (d d);
 *  G_rc = ((2 g) m) E_rc + grad_residual[f,s]_rc.
 *  grad_frames[f,j]_rk, the 3 x 3 entries only: the sum over the live sensors with joint[s] = j, IN ASCENDING s FROM +0, of (G O^T)_rk =
 *       the sum over c of G_rc O_kc, ascending c from the first product (G_r0 O_k0, then + G_r1 O_k1, then + G_r2 O_k2, up to C).  A
 *       gather with no atomics: several sensors may share a joint.  A joint with no live sensor gets +0, and is left alone under
 *       accumulate.  Column 3 of a row_stride = 4 buffer is never written, so with accumulate = 1 the result lands in the grad_world
 *       buffer that goes to smplpp_skeleton_vjp.
 *  grad_target[f,s] = -G for Tn = n; for Tn = 1, grad_target[0,s]_rc = sum1024 over the frames f, ascending, of -G_rc.
 *  grad_offset[s]_kc = sum1024 over the frames f, ascending, of (A^T G)_kc = (A_0k G_0c + A_1k G_1c) + A_2k G_2c.  It may be asked for
 *       under a NULL offset (the gradient at the identity columns).
 * A dead sensor adds +0 to every sum.  There is no gradient to the weights.  accumulate = 0 stores, 1 is one fp32 add onto what is there.
 * Each output may be NULL, not all.  The bits do not depend on n (per-frame outputs), on the memory space or on which outputs and
 * cotangents are given.  At most two launches: grad_frames and a per-frame grad_target together (a thread per (frame, sensor), then a
 * thread per (frame, joint) that adds its sensors from LDS), and the sums across the frames (a workgroup of 1024 per sensor).
 *  - SMPLPP_ERR_INVALID: as the forward (cotangents for outputs), every cotangent NULL, accumulate not 0 or 1 (the outputs are
 *    untouched). */
int smplpp_orientation_term_vjp(int device, int64_t n, int64_t J, int64_t row_stride, const float * frames, int64_t S, int64_t C,
                                const int64_t * joint, const float * offset, const float * target, int64_t Tn, const float * weight, int64_t Wn,
                                float rho, const float * grad_energy /*[n] nullable*/, const float * grad_sensor_energy /*[n,S] nullable*/,
                                const float * grad_residual /*[n,S,3,C] nullable*/, float * grad_frames /*[n,J,3,row_stride] nullable*/,
                                float * grad_offset /*[S,3,C] nullable*/, float * grad_target /*[Tn,S,3,C] nullable*/, int accumulate,
                                int space, void * stream);
/* The sweep grid of node/node.cpp:1023-1073 for ONE frame of posed vertices [V,3]: cells of GRID_SCALE = 0.025 m
 * (toolbox/GridUtils.hpp:28) from getGridIdxFloor(min) to getGridIdxCeil(max) per axis (:46-60) -> grid_min [3] (cell
 * index of the first cell), grid_num [3]; cells are ordered x outermost, z innermost like the reference's loops (:1037-1048).
 * winding [cap] (nullable) = generalized winding number of the mesh at each cell position (igl::winding_number, :1052),
 * inside [cap] (nullable) = winding number > 0.5 on the REAL-valued number.  Deviation, deliberate: the reference stores
 * igl::winding_number's result in an Eigen::VectorXi (:1051-1057), which truncates towards zero before the `> 0.5` test, so
 * there a cell counts as inside only when the number reaches 1 (0.99999 of an interior point becomes 0); compare `winding`
 * with 1 - eps yourself to reproduce that list.  *cells = the grid's cell count; at most `cap` cells are evaluated (call with
 * cap = 0 to size the arrays).  Non-finite or absurd (beyond +-25 km) vertices: SMPLPP_ERR_NUMERIC. */
int smplpp_sweep_grid(smplpp_model * m, const float * verts, int32_t * grid_min, int32_t * grid_num, int64_t cap,
                      float * winding, uint8_t * inside, int64_t * cells, int space, void * stream);
/* SMPL::getAdjacentFaces (src/SMPL.cpp:537-540): host copy; returns the count in *count, fills up to cap. */
int smplpp_adjacent_faces(const smplpp_model * m, int64_t vertex, int64_t cap, int64_t * faces, float * weights,
                          int64_t * count);

/* ------------------------------------------------------------------ IK: IkTask + the loop of node/node.cpp */
/* A batch of n independent frames, each with K tasks in the caller's std::map order (node/node.cpp:47,798).
 * Unknown layout per frame: [theta (75, or 44 with a VPoser) | phi (2K) | beta (10 when optimised)] (:787-791). */
int smplpp_ik_create(smplpp_model * m, int64_t n, int64_t K, smplpp_vposer * vposer /*nullable*/, smplpp_ik ** out);
int smplpp_ik_destroy(smplpp_ik * s);
/* This solver holds frames [frame_base, frame_base + n) of a larger job (contiguous shards per GPU).  Everything a
 * frame computes is independent of the frames beside it; the one kernel that orders its fp32 sums by frame position (the VPoser
 * decoder's Jacobian) takes the position from the GLOBAL index, so a frame's trajectory has the same bits on 1, 2, 4 or 8 GPUs.
 * Default 0.  No reference counterpart (single device, node/node.cpp:372). */
int smplpp_ik_set_frame_base(smplpp_ik * s, int64_t frame_base);
/* Arithmetic of the solver's loops (smplpp_ik_eval, _iterate, _solve_sequence, _solve_sequence_shared, the body stage included).
 * EXACT is the reference's (node/node.cpp:761-777 in fp32 libtorch): the internal forward passes run the model's smplpp_fk form
 * instead of the loops' fp16x2 one, and a latent solver decodes with the exact-fp32 value kernel and pulls its rows back through
 * smplpp_vposer_jacobian's exact-fp32 Jacobian (its own workspace, the caller's stream; no side-stream schedule).  Status bit 3
 * is never raised in this mode.  Per solver; takes effect from the next call; EXACT is refused on a model created with
 * SMPLPP_SKIN=h; an unknown mode is SMPLPP_ERR_INVALID. */
#define SMPLPP_IK_ARITH_DEFAULT 0 /* today's loops: the model's IK form (h) and the fp16x2 decoder Jacobian */
#define SMPLPP_IK_ARITH_EXACT 1   /* the reference's arithmetic inside the loops */
int smplpp_ik_set_arithmetic(smplpp_ik * s, int mode);
/* IkTask public fields (IkTask.h:54-84), struct-of-arrays over [n,K]; any pointer may be NULL = keep current.
 * Defaults match the header: weights 1, phiLimit 0.04, normalOffset 0, vertexWeights 1/3, targetNormal +Z. */
int smplpp_ik_set_tasks(smplpp_ik * s, const int64_t * face_idx /*[n,K]*/, const float * vertex_weights /*[n,K,3]*/,
                        const float * target_pos /*[n,K,3]*/, const float * target_normal /*[n,K,3]*/,
                        const double * pos_task_weight /*[n,K]*/, const double * normal_task_weight /*[n,K]*/,
                        const double * phi_limit /*[n,K]*/, const double * normal_offset /*[n,K]*/, int space);
/* g_beta [n,10] and g_theta [n,theta_dim] (node/node.cpp:44-45, :377). */
int smplpp_ik_set_config(smplpp_ik * s, const float * beta, const float * theta, int space);
int smplpp_ik_get_config(smplpp_ik * s, float * beta, float * theta, int space);
int smplpp_ik_get_tasks(smplpp_ik * s, int64_t * face_idx, float * vertex_weights, float * tangents /*[n,K,3,2]*/,
                        float * actual_pos /*[n,K,3]*/, float * actual_normal /*[n,K,3]*/, int space);
/* One evaluation of node/node.cpp:750-877 for every frame: forward, tangents + vertex weights refresh (:803-804),
 * residual e [n,4K] and the analytic Jacobian J [n,4K,D] (fp64, row-major) that replaces the per-row autograd
 * backward() of :823-869.  D = theta_dim + 2K + (optimize_beta ? 10 : 0). */
int smplpp_ik_eval(smplpp_ik * s, int optimize_beta, double * e, double * J, int space, void * stream);
/* `iters` repetitions of the loop body :704-1001 on every frame: eval, A = J^T J + damping (:883-904), solve
 * (enable_qp: box QP :909-930, else LLT :931-939), config update (:945-968), mesh re-projection (:970-1001).
 * optimize_beta_from >= 0 mirrors solveMocapBody: beta optimised and phi limits live from that iteration (:655,:695).
 * Frames whose number of tasks with pos_task_weight > 0 is < min_valid skip the solve (:785).
 * e_sqnorm [n] (nullable) receives |e|^2 of the last evaluation. */
int smplpp_ik_iterate(smplpp_ik * s, int iters, int enable_qp, int optimize_beta_from, int64_t min_valid,
                      double * e_sqnorm, int space, void * stream);
/* The frame loop of solveMocapMotion (node/node.cpp:1369-1407 with the per-frame target switch of :681-700) for n chains
 * (sequences / restarts) in lock step, enqueued without a host round trip per frame: for t = 0..T-1 the marker targets of
 * frame t become the task targets (valid == 0: target 0 and posTaskWeight_ 0, else posTaskWeight_ 1), then `warmup_iters`
 * (t == 0; the reference advances once ikIter > 30) or `iters_per_frame` iterations of smplpp_ik_iterate's loop body run,
 * warm-started from the previous frame; theta_out[t] receives g_theta after frame t. Every other task field (faces,
 * weights, offsets, phi limits) is what smplpp_ik_set_tasks left. Layouts: target_pos [T,n,K,3], valid [T,n,K] (bytes),
 * theta_out [T,n,theta_dim]. */
int smplpp_ik_solve_sequence(smplpp_ik * s, int64_t T, const float * target_pos, const uint8_t * valid, int warmup_iters,
                             int iters_per_frame, int enable_qp, int64_t min_valid, float * theta_out, int space, void * stream);
/* The same loop when every chain fits the SAME capture — the multi-restart fit the reference runs by hand (one sample_walk.c3d, many
 * initial poses; node/node.cpp:1369-1407 once per restart): target_pos [T,K,3] and valid [T,K] are given once and handed to all n
 * chains by the frame switch on the device; theta_out [T,n,theta_dim] as above. Results are those of smplpp_ik_solve_sequence with
 * the targets repeated n times, bit for bit. */
int smplpp_ik_solve_sequence_shared(smplpp_ik * s, int64_t T, const float * target_pos, const uint8_t * valid, int warmup_iters,
                                    int iters_per_frame, int enable_qp, int64_t min_valid, float * theta_out, int space, void * stream);
/* Vertices of the last forward inside the solver [n,V,3] (SMPL::getVertex after the loop's launch). */
int smplpp_ik_get_vertices(smplpp_ik * s, float * verts, int space, void * stream);
/* Outcome of the solves so far, per frame: bit 0 = the LAST solve failed with the reference's "LLT has numerical issue!"
 * (node/node.cpp:934-937; that frame's update was skipped), bit 1 = some solve failed since the configuration was set /
 * the sequence started, bit 2 = an evaluation since the tasks were last set met a task WITH A NORMAL TERM (normal weight or normal
 * offset) on a vertex of more than 16 adjacent faces: the analytic Jacobian differentiates vertex normals through per-face tables
 * whose width smplpp_model_create takes from the topology — 12 faces per vertex, 16 when some vertex has more (SMPL's own mesh:
 * at most 9; src/SMPL.cpp:527-535 puts no bound on it) — so beyond 16 those rows are unsupported — the solve SKIPS the update of such a frame
 * (no caller moves on a truncated Jacobian) and smplpp_ik_set_tasks clears the bit (it belongs to the tasks; the next evaluation
 * raises it again where it still applies); position-only tasks are unaffected and any model gets its solver.  Bit 3 = a forward
 * pass inside a loop on this model met an operand outside the fp16x2 form's range since the last smplpp_ik_set_config (one word per
 * model: every frame of the batch carries it).  Bit 4 = the last solve of the frame was a box QP (enable_qp) that used all of its
 * 4 D + 20 active-set passes without meeting its optimality test; its last iterate was applied as the update.  Host-space eval /
 * iterate / solve_sequence calls return SMPLPP_ERR_NUMERIC (bits 0, 1) or SMPLPP_ERR_INVALID (bit 2) themselves, and no error for
 * bit 4; enqueue-only (SMPLPP_DEVICE) callers have no return value to inspect and read it here (waits for `stream` first). flags [n]. */
int smplpp_ik_get_status(smplpp_ik * s, int32_t * flags, int space, void * stream);
/* The step of the last solve of every frame, fp64: x [n,D] = (d theta [theta_dim] | phi [2K] | d beta [beta_dim]) as the solve
 * computed it, before the fp32 update (node/node.cpp:938-968), with D = theta_dim + 2K + beta_dim of that solve (beta_dim 10 when
 * it optimised beta, else 0); *D receives it, and x may be NULL to ask for D alone (0 before the first solve).  Rows are defined
 * only for frames whose last solve ran and succeeded: a skipped frame (min_valid) keeps what an earlier solve wrote, and a frame
 * with status bit 0 holds the values of the failed solve.  Pinned surface coordinates (phi limit 0) read 0.  Waits for `stream`
 * in host space; in device space the copy is enqueued on it. */
int smplpp_ik_get_step(smplpp_ik * s, double * x, int64_t * D, int space, void * stream);

/* Streams and sharing.  A model owns ONE workspace (pose coefficients, relative transforms of the last forward pass) that
 * smplpp_fk and every smplpp_ik built on the model write: all work on one model handle must be issued in stream order on
 * ONE caller stream (or be separated by the caller's own synchronisation).  The setters (set_tasks / set_config) are
 * host-synchronous on the NULL stream; call them only when no enqueue-only call on the solver is still in flight. */

/* ------------------------------------------------------------------ multi-GPU: the final gather
 * Frames (FK, independent IK) and restarts (capture fitting) shard across GPUs with no exchange in the data path; the only
 * collective is the gather of result rows at the end.  `comm` is an ncclComm_t (RCCL) the HOST created — one rank per GPU,
 * ncclCommInitRank / ncclCommInitAll — passed as an opaque pointer; RCCL is resolved at run time (the symbols already in the
 * process, else librccl.so), so single-GPU users carry no dependency on it.  Every rank passes its block `send`
 * [rows_per_rank[rank], row_floats] and receives all blocks in rank order in `recv` [sum rows_per_rank, row_floats] (device
 * pointers; `send` may alias its own slot of `recv`).  Equal blocks travel as one ncclAllGather, ragged ones as grouped
 * broadcasts; enqueued on `stream`.  What it replaces: nothing in the single-GPU reference — this is the SURVEY's proposed
 * `smplpp_gather(comm, ...)`. */
int smplpp_gather(void * comm, const float * send, float * recv, const int64_t * rows_per_rank, int world, int rank,
                  int64_t row_floats, void * stream);
/* The same exchange to ONE rank (the usual consumer of a job's results): every other rank sends its block once, over its own
 * xGMI link, straight into its slot of root's `recv` (grouped ncclSend / ncclRecv; `recv` may be NULL elsewhere) — an eighth
 * of the all-gather's traffic at eight ranks.  In place on root when `send` is its own slot of `recv`. */
int smplpp_gather_to_root(void * comm, const float * send, float * recv, const int64_t * rows_per_rank, int world, int rank, int root,
                          int64_t row_floats, void * stream);
/* Start-up check of the RCCL binding (resolved at run time, see above): `rank` exchanges `count_floats` floats with ITSELF in one
 * ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd — the calls smplpp_gather_to_root makes for a peer — so a host learns before
 * the job, not at its end, whether the library it loaded speaks this ABI.  Device pointers, `send` != `recv`; enqueued on `stream`. */
int smplpp_gather_selfcheck(void * comm, int rank, const float * send, float * recv, int64_t count_floats, void * stream);
/* Where each rank's block lies in the gathered array: offsets[world + 1] in floats (the last entry is the total).  Host-only
 * arithmetic shared by the two collectives; callable without a GPU. */
int smplpp_gather_offsets(const int64_t * rows_per_rank, int world, int64_t row_floats, int64_t * offsets);

/* ------------------------------------------------------------------ body measurements: part areas, volumes and plane girths
 * How large the posed body is: the surface area and the enclosed volume of regions of the mesh, and the length of the curve a plane
 * cuts from a region (chest, waist, hip, thigh).  No reference counterpart.  A REGION is a list of faces of the model (0-based ids): a
 * body part, or all faces.  1 <= R <= 256; regions may overlap ("whole body" and "torso" on one handle); a region may be empty; a face
 * appears at most once in a region; the order of a region's list is the order of its sums.  A SECTION is a plane paired with the
 * region whose faces it cuts, 0 <= S <= 256: the chest plane paired with the torso keeps the arms out of the chest girth.  region_ptr
 * [R+1], region_face [nnz = region_ptr[R]] and section_region [S] are host pointers.  The handle copies what it needs of the model (V,
 * the faces, the per-vertex adjacency, the device): it may outlive it.  Creation builds, on the host, the region lists as int32, for
 * every face the (region, slot) pairs that hold it in ascending region, and for every region its sections in ascending s.
 *  - SMPLPP_ERR_INVALID: R outside [1, 256], S outside [0, 256], region_ptr[0] != 0 or not non-decreasing, a face id outside [0, F), a
 *    face twice in one region, a section_region outside [0, R), a NULL array that is needed (*out = NULL). */
int smplpp_measure_create(smplpp_model * m, int64_t R, const int64_t * region_ptr /*[R+1] host*/,
                          const int64_t * region_face /*[nnz] host, 0-based face ids*/, int64_t S,
                          const int64_t * section_region /*[S] host*/, struct smplpp_measure ** out);
int smplpp_measure_destroy(struct smplpp_measure * ms);
int smplpp_measure_info(const struct smplpp_measure * ms, int64_t * R, int64_t * nnz, int64_t * S);
/* area [n,R], volume [n,R], section [n,S], crossings [n,S] of verts [n,V,3].  fp32, every operation rounded on its own (no FMA),
 * division and square root correctly rounded.
 * Per face f with corners 0, 1, 2 in stored order, p_i = v_i - c with c = center[frame] (NULL: zeros, the same bits as a zero array):
 *    a = p1 - p0, b = p2 - p0, cr = a x b,   area_f = 0.5f * sqrtf((cr.x cr.x + cr.y cr.y) + cr.z cr.z)
 *    w = p1 x p2,                             vol_f  = ((p0.x w.x + p0.y w.y) + p0.z w.z) / 6.0f
 * (u x v = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x)).  On a closed, outward-oriented region `volume` is the enclosed
 * volume and in exact arithmetic does not depend on center; an open region's volume is that of the cone from center over it.  center
 * exists because a body 2.5 m from the origin loses digits to cancellation; it is a constant of the definition and has no cotangent.
 * Section s of region r, plane (nx, ny, nz, d) = planes[frame or 0][s], the plane n.x = d, used as given (not normalised):
 *    per corner, on the raw vertex:  s_i = ((nx x_i + ny y_i) + nz z_i) - d,  above_i = (s_i >= 0)    (no face enters: both faces of
 *    an edge see the same value); the face is crossed iff one or two corners are above.  L is the corner alone on its side, M and N
 *    the other two in cyclic corner order after L.  For the edges (L, M) and (L, N) in turn, a is the end below and b the end above:
 *    t = s_a / (s_a - s_b),  q = a + t (b - a) per coordinate (s_a < 0 <= s_b: the divisor is never zero);  with e = q_(L,N) - q_(L,M)
 *    the face's term is sqrtf((e.x e.x + e.y e.y) + e.z e.z).  crossings counts the crossed faces.
 * This is the contour of {s >= 0} on the surface, the plane moved by +eps: an edge lying in the plane is counted once, by the face
 * below it; a face lying in the plane contributes nothing itself and its border is counted by its below-side neighbours; a plane
 * through a vertex needs no special case.
 * area[i,r], volume[i,r] and section[i,s] are each ONE sum1024 (FIXED-ORDER SUMS) over the region's list index k; a face that is not
 * crossed adds +0.  Dead data: a face with a corner that is not finite adds +0 to every sum and is not counted; a plane with an entry
 * that is not finite or with a zero normal gives section 0 and crossings 0.  Each output may be NULL, not all.  The bits of a frame do
 * not depend on n, on its position in the batch, on the memory space, on the outputs asked for or on what else shares the handle.
 *  - SMPLPP_ERR_INVALID: n <= 0, verts NULL, plane_frames not 1 or n, planes NULL with S > 0, no output, n V 3, n R or n S 4 beyond
 *    int32 indexing (the outputs are untouched). */
int smplpp_measure(struct smplpp_measure * ms, int64_t n, const float * verts /*[n,V,3]*/, const float * center /*[n,3] nullable = 0*/,
                   const float * planes /*[plane_frames,S,4] (nx,ny,nz,d): n.x = d; NULL iff S = 0*/, int64_t plane_frames /*1 or n*/,
                   float * area /*[n,R] nullable*/, float * volume /*[n,R] nullable*/, float * section /*[n,S] nullable*/,
                   int32_t * crossings /*[n,S] nullable*/, int space, void * stream);
/* Its vector-Jacobian product in closed form, at the crossing pattern of the forward.  A TERM is the gradient of one face's share
 * of one output; it exists only where its cotangent is given and not 0, the face is live and, for a section, the plane is live, the
 * face is crossed and its term is not 0; for an area, |cr| != 0.  With g the cotangent:
 *    area:    k = (g 0.5f) / |cr|, gc = k cr;  to corner 1: ga = b x gc, to corner 2: gb = gc x a, to corner 0: -(ga + gb)
 *    volume:  k = g / 6.0f;  to corner 0: k (p1 x p2), to corner 1: k (p2 x p0), to corner 2: k (p0 x p1)
 *    section: gu = g (e / len) per coordinate; the edge (L, M) takes gq = -gu, the edge (L, N) gq = gu.  Per edge, with ba = b - a:
 *             gt = (gq.x ba.x + gq.y ba.y) + gq.z ba.z,  r = gt / (s_a - s_b),  gsa = -(r (s_b / (s_a - s_b))),  gsb = r t;
 *             to a: (1.0f - t) gq + gsa n, to b: t gq + gsb n (each coordinate: product + product);
 *             to the plane: (gsa a + gsb b per coordinate, (-gsa) - gsb).
 *             L receives its share of (L, M) plus its share of (L, N); the plane the share of (L, M) plus that of (L, N).
 * grad_verts[i,v] is one sequential sum from +0 of the terms that exist, in this order: the vertex's incident faces in the order of
 * the model's adjacency table (ascending face id); for a face, its corners that are v in ascending corner (one, unless the face is
 * degenerate); then the regions that list the face in ascending r; for each region the area term, the volume term, then the region's
 * sections in ascending s.  grad_planes[i,s,:] is four sum1024 over the region's list index k (a face without a term adds +0); with
 * plane_frames = 1 and n > 1 the frames' sums are then summed in the two-level tile order of smplpp_vertex_offsets_vjp.  accumulate =
 * 0 stores, 1 adds the finished sum once.  A NULL cotangent is zero and costs nothing.  No floating-point atomics; the handle's own
 * workspace ([n,S,4] floats for shared planes); deterministic, with the independence of the forward.  One caller thread per handle.
 *  - SMPLPP_ERR_INVALID: as the forward, accumulate not 0 or 1 (the outputs are untouched). */
int smplpp_measure_vjp(struct smplpp_measure * ms, int64_t n, const float * verts, const float * center, const float * planes,
                       int64_t plane_frames, const float * grad_area /*[n,R] nullable = 0*/, const float * grad_volume /*nullable*/,
                       const float * grad_section /*[n,S] nullable*/, float * grad_verts /*[n,V,3] nullable*/,
                       float * grad_planes /*[plane_frames,S,4] nullable*/, int accumulate, int space, void * stream);
/* ------------------------------------------------------------------ VPoser decoder (src/VPoser.cpp) */
/* VPoserDecoderImpl (VPoser.h:53-90): Linear(32,512) LeakyReLU Dropout(eval) Linear(512,512) LeakyReLU
 * Linear(512,126) -> 6D -> rotation (Gram-Schmidt, :129-141) -> axis-angle (:25-120).  Weights are
 * torch::nn::Linear layout [out,in] as loadParamsFromJson stores them (:169-238), host pointers. */
int smplpp_vposer_create(int device, const float * w0 /*[512,32]*/, const float * b0 /*[512]*/,
                         const float * w1 /*[512,512]*/, const float * b1 /*[512]*/, const float * w2 /*[126,512]*/,
                         const float * b2 /*[126]*/, smplpp_vposer ** out);
int smplpp_vposer_destroy(smplpp_vposer * v);
/* VPoserDecoderImpl::forward (src/VPoser.cpp:163-167): z [n,32] -> axis-angles [n,21,3];
 * jac (nullable) [n,63,32] = d(out)/dz, the quantity autograd supplies in node/node.cpp:761-772. */
int smplpp_vposer_forward(smplpp_vposer * v, int64_t n, const float * z, float * out, float * jac, int space,
                          void * stream);
/* The same for a SHARD of a larger job: frame_base = the global index of this call's frame 0.  The Jacobian kernel orders its
 * fp32 sums by the frame's global index, so a latent decodes to the same bits whether the job runs on 1 GPU or is cut over
 * 2, 4 or 8 (smplpp_vposer_forward is frame_base = 0).  No reference counterpart: the reference is single-device
 * (node/node.cpp:372); SURVEY 8(e). */
int smplpp_vposer_forward_at(smplpp_vposer * v, int64_t n, int64_t frame_base, const float * z, float * out, float * jac, int space,
                             void * stream);
/* Vector-Jacobian product of smplpp_vposer_forward_at (the backward pass the reference gets from libtorch autograd through
 * vposer->forward(latent), node/node.cpp:761-772): given dL/dout [n,21,3], writes dL/dz [n,32] (overwritten).
 * out (nullable) [n,21,3]: the decoded angles the product was taken at, bit-identical to smplpp_vposer_forward with jac NULL (the
 * product differentiates that exact-fp32 decode, so the LeakyReLU masks and the axis-angle branches are the ones the caller's loss
 * saw).  Deterministic; a frame's bits do not depend on n or frame_base.  The first call on a decoder builds copies of its
 * weights in [out][in] layout (1.3 MB, freed by smplpp_vposer_destroy).  One workspace per decoder: concurrent calls on one
 * handle from different streams need the caller's own ordering. */
int smplpp_vposer_vjp(smplpp_vposer * v, int64_t n, int64_t frame_base, const float * z, const float * grad_out,
                      float * grad_z, float * out, int space, void * stream);
/* d(out)/dz [n,63,32] in exact fp32 (fp32 products and sums, as libtorch autograd runs the reference's node/node.cpp:761-772),
 * at the decode smplpp_vposer_forward returns with jac NULL.  out (nullable) [n,21,3]: those angles, bit-identical to that call.
 * Deterministic; a frame's bits do not depend on n or frame_base.  The decoder owns the workspace (64 KB per frame, grown to n,
 * freed by smplpp_vposer_destroy): concurrent calls on one handle from different streams need the caller's own ordering. */
int smplpp_vposer_jacobian(smplpp_vposer * v, int64_t n, int64_t frame_base, const float * z, float * out, float * jac, int space,
                           void * stream);
/* convertRotMatToAxisAngle (src/VPoser.cpp:25-120): rot [n,3,3] -> aa [n,3]. */
int smplpp_rotmat_to_axis_angle(int device, int64_t n, const float * rot, float * aa, int space, void * stream);
/* The inverse companion: aa [n,3] -> rot [n,3,3] row-major by the reference's Rodrigues formula (src/BlendShape.cpp:803-844:
 * angle = ||aa + 1e-8||, so aa = 0 gives the identity without a branch), with the operation order of smplpp_fk's pose step: the bits
 * smplpp_fk computes internally for the same axis-angle. */
int smplpp_axis_angle_to_rotmat(int device, int64_t n, const float * aa /*[n,3]*/, float * rot /*[n,3,3]*/, int space, void * stream);
/* Its vector-Jacobian product: grad_aa[i][m] = sum_q grad_rot[i][q] dR_q/daa_m, q ascending from +0, each product and each sum rounded
 * on its own, grad_rot as nine independent entries per row.  dR/daa_m is the derivative of the same formula, ||aa + 1e-8|| included, by
 * the function smplpp_skeleton_vjp and smplpp_fk_vjp contract with: it is finite at aa = 0 and at |aa| = pi.  So fed with the grad_rot
 * of smplpp_skeleton_rotmat_vjp it gives grad_theta[:, 1:] of smplpp_skeleton_vjp (to rounding: the shared function is compiled into
 * each kernel).  With smplpp_sequence_smoothness_vjp at C = 9 it carries a rotation-space smoothness back to theta.  accumulate = 0
 * stores, 1 is one fp32 add onto what is there.  A thread per (row, m); no handle, no workspace.
 *  - SMPLPP_ERR_INVALID: n <= 0, a NULL pointer, accumulate not 0 or 1, a bad space (grad_aa is untouched). */
int smplpp_axis_angle_to_rotmat_vjp(int device, int64_t n, const float * aa /*[n,3]*/, const float * grad_rot /*[n,3,3]*/,
                                    float * grad_aa /*[n,3]*/, int accumulate, int space, void * stream);
/* ------------------------------------------------------------------ scan preparation: neighbours, normals, farthest points
 * What a raw cloud needs before the scan terms take it: the k nearest cloud points of every query, a normal and a surface variation
 * per point from those lists, and a thinning to M well-spread points.  The scan is data, so none has a vector-Jacobian product.  The
 * calls take no handle and no workspace: `device` as the stage calls.  All arithmetic is fp32, every operation rounded on its own (no
 * FMA), '/' and sqrt are the correctly rounded ones, every sum is sequential in the stated order, every choice is the minimum or maximum
 * of a total order, and there are no floating-point atomics: no bit depends on the work split, on n, on the frame's slot, on the memory
 * space or on which outputs are asked for.  THE DISTANCE of all three:  d(a, b) = ((dx dx + dy dy) + dz dz),  dx = a_x - b_x and so on
 * (the distance of smplpp_mesh_point_distance).
 *
 * smplpp_cloud_knn: for every query q of frame f, the k nearest of the frame's K points.  queries NULL: the cloud queries itself
 * (Q is not read and taken as K), and candidate j = q, the query's own index, is left out; another point with the same coordinates is
 * listed at d = 0.  THE RULE: candidate j is listed iff d = d(query, p_j) is finite and d <= max_sqdist (+inf: no cap).  The listed
 * candidates are ordered by the pair (d, j) lexicographically, ascending; count = min(k, how many are listed); rank r < count holds
 * (index, sqdist) = the r-th pair, every rank from count on holds (-1, +0).  A query with a coordinate that is not finite has no finite
 * d, so its count is 0.  index [n,Q,k] int32, sqdist [n,Q,k], count [n,Q] int32; each nullable, not all.  n, K or Q = 0 is no work
 * (K = 0 with queries: every count 0).
 *  - SMPLPP_ERR_INVALID: k outside 1..32, a negative n, K or Q, a NaN max_sqdist, every output NULL, a NULL points with K > 0, n Q k or
 *    n K 3 or n Q 3 beyond int32 indexing, a bad space (the outputs are untouched). */
int smplpp_cloud_knn(int device, int64_t n, int64_t K, const float * points /*[n,K,3]*/, int64_t Q, const float * queries /*[n,Q,3] nullable*/,
                     int k, float max_sqdist, int32_t * index /*[n,Q,k] nullable*/, float * sqdist /*[n,Q,k] nullable*/,
                     int32_t * count /*[n,Q] nullable*/, int space, void * stream);
/* smplpp_cloud_normals: per point i of frame f, from its neighbour list index[f][i][0..k) (smplpp_cloud_knn in self-query mode; any
 * k >= 1).  THE RULE, p = p_i:
 *  1 neighbours: in rank order, each listed j with 0 <= j < K and e = p_j - p finite in all three components counts; any other entry is
 *                skipped (a j >= K is skipped on the device and refused from host space).  m = that count + 1: the point itself, e = 0.
 *  2 covariance: s_a = sum e_a and T_ab = sum e_a e_b (a <= b), both from +0 in rank order;  mean_a = s_a / m;
 *                C_ab = T_ab - m (mean_a mean_b), m as a float.
 *  3 Jacobi:     V = I; FOUR sweeps over the pairs (p, q) = (0,1), (0,2), (1,2).  A pair with C_pq == 0 is skipped.  Else
 *                tau = (C_qq - C_pp) / (2 C_pq);  t = sg / (|tau| + sqrt(tau tau + 1)), sg = -1 for tau < 0, else 1 (t = 1 at tau = 0;
 *                a tau tau that overflows gives t = 0);  c = 1 / sqrt(t t + 1);  s = t c;  h = t C_pq;  C_pp -= h;  C_qq += h;
 *                C_pq = 0;  for the third index r: (C_rp, C_rq) = (c C_rp - s C_rq, s C_rp + c C_rq), on the old values and kept
 *                symmetric;  for every r: (V_rp, V_rq) = (c V_rp - s V_rq, s V_rp + c V_rq).  lambda_i = C_ii, with column i of V.
 *  4 order:      (lambda_0, lambda_1, lambda_2) with their columns sorted ascending by (value, column): the exchanges (0,1), (1,2),
 *                (0,1), each made iff the later value < the earlier one.
 *  5 normal:     v = the column of lambda_0;  normal = v / sqrt((v0 v0 + v1 v1) + v2 v2).  With a viewpoint c (Vn = 1: one for all
 *                frames; Vn = n: one per frame) it is negated iff (n0 (c0 - p0) + n1 (c1 - p1)) + n2 (c2 - p2) < 0; with Vn = 0 iff the
 *                component of largest magnitude (the lowest axis on ties) is < 0.
 *  6 curvature:  lambda_0 / ((lambda_0 + lambda_1) + lambda_2), the surface variation, +0 unless that sum is > 0.
 *  7 status:     1 (bit 0): m < 3 or p is not finite: normal and curvature are +0 and no other bit is set.  2 (bit 1): lambda_2 <= 0 or
 *                (lambda_1 - lambda_0) < min_gap lambda_2: the normal is not unique (a line, a point); it is still written.
 * A zero normal is what the compatible scan searches treat as unmatched, so `normal` goes straight into them.  normal [n,K,3],
 * curvature [n,K], status [n,K] int32; each nullable, not all.  n or K = 0 is no work.
 *  - SMPLPP_ERR_INVALID: k < 1, a negative n or K, Vn not 0, 1 or n, a NULL viewpoint with Vn > 0, min_gap negative or not finite,
 *    every output NULL, a NULL points or index, n K k or n K 3 beyond int32 indexing, a host-space index >= K, a bad space (the outputs
 *    are untouched). */
int smplpp_cloud_normals(int device, int64_t n, int64_t K, const float * points /*[n,K,3]*/, int k, const int32_t * index /*[n,K,k]*/,
                         const float * viewpoint /*[Vn,3]*/, int64_t Vn, float min_gap, float * normal /*[n,K,3] nullable*/,
                         float * curvature /*[n,K] nullable*/, int32_t * status /*[n,K] nullable*/, int space, void * stream);
/* smplpp_cloud_farthest_points: per frame, M of the K points by farthest-point sampling.  THE RULE: dmin_j = +inf for every finite
 * point; a point that is not finite is never chosen.  Pick 0 is start[f] (NULL: 0) if that is a finite point of the frame, else the
 * lowest finite index.  After pick s:  dmin_j = d < dmin_j ? d : dmin_j  with d = d(p_j, p_s) for every finite j, and s is marked
 * chosen.  The next pick is the unchosen finite point with the largest dmin, the lowest index on ties (a total order, so the reduction
 * tree is free).  radius_sq[i] is the pick's dmin when it was chosen (+inf for pick 0): the sequence never increases, and radius_sq[M-1]
 * bounds the spacing of the sample from below.  When no unchosen finite point is left, the remaining picks hold (-1, +0).  min_sqdist
 * [n,K] is every point's final dmin, +0 for the chosen points and for the ones that are not finite: the coverage of the sample.  It is
 * required: above 16384 points it is the kernel's working array.  index [n,M] int32 and radius_sq [n,M] are nullable.  n = 0 is no work.
 *  - SMPLPP_ERR_INVALID: a negative n, K or M, M outside 1..K, a NULL points or min_sqdist, n K 3 beyond int32 indexing, a host-space
 *    start outside [0, K) (on the device it reads as "not a finite point"), a bad space (the outputs are untouched). */
int smplpp_cloud_farthest_points(int device, int64_t n, int64_t K, const float * points /*[n,K,3]*/, int64_t M,
                                 const int32_t * start /*[n] nullable = 0*/, int32_t * index /*[n,M] nullable*/,
                                 float * radius_sq /*[n,M] nullable*/, float * min_sqdist /*[n,K]*/, int space, void * stream);
/* ------------------------------------------------------------------ surface geodesics and the self-contact search
 * Distance along the surface, and with it the rule "a vertex's contact partner is the nearest other vertex in space among those that
 * are far along the surface" (the self-contact terms of TUCH and SMPLify-XMC).  All arithmetic is fp32, every operation rounded on its
 * own (no FMA), sqrt is the correctly rounded one, every choice is the minimum of a total order, and there are no floating-point atomics:
 * no bit depends on n, on the frame's slot, on the memory space, on the other fields of a call or on how the work is split.
 *
 * smplpp_mesh_geodesic: field s of frame i is the distance along the edges of the mesh from the source set
 * source_vertex[source_ptr[s] .. source_ptr[s+1]), which the frames share.  The edges are the undirected edges of the model's faces,
 * each once.  THE RULE:
 *  length    w(u, v) = sqrt((dx dx + dy dy) + dz dz),  d = x_hi - x_lo,  lo = min(u, v),  hi = max(u, v): the same bits in both
 *            directions.  An edge whose length is not finite does not exist (a NaN or inf vertex is routed around); 0 is a length.
 *  distance  dist[v] = the minimum over all edge paths from any source of the set to v of the left-to-right fp32 sum of the path's
 *            lengths, the sum starting from +0 at the source.  fl(a + w) is monotone in a, so this is the fixed point of
 *            dist[v] <- min(dist[v], fl(dist[u] + w(u, v)))  from dist = +inf, dist[source] = 0, reached in any order of relaxation
 *            (smplpp_amd/csrc/edge_tables.h carries the argument).
 *  outputs   an unreachable vertex: +inf.  An empty set: all +inf.  A repeated source is harmless.  dist[v] > max_dist is reported as
 *            +inf: the bits of thresholding the uncapped field (max_dist = +inf: no cap).
 * The distance is a graph distance, an upper bound of the exact surface geodesic.  It has no vector-Jacobian product.
 *  - SMPLPP_ERR_INVALID (dist untouched): n <= 0 or S <= 0; a NULL verts, source_ptr or dist, or a NULL source_vertex with a source
 *    listed; source_ptr not starting at 0 or not non-decreasing (a device-space source_ptr is read back for this check: the call then
 *    waits for the stream once); a HOST-space source outside [0, V) (a device-space one is ignored); max_dist negative or NaN; a model
 *    without faces; n S V or n V 3 beyond int32 indexing; V > 32768 (the field of a workgroup lives in LDS); a bad space. */
int smplpp_mesh_geodesic(smplpp_model * m, int64_t n, const float * verts /*[n,V,3]*/, int64_t S, const int64_t * source_ptr /*[S+1]*/,
                         const int64_t * source_vertex /*[source_ptr[S]]*/, float max_dist, float * dist /*[n,S,V]*/, int space,
                         void * stream);
/* The self-contact handle: the far relation of a rest mesh.  Creation runs smplpp_mesh_geodesic's rule on `rest` (the template, or a frame
 * of smplpp_fk's `rest` for the subject's beta; a HOST array) from every vertex as a single source.  THE RELATION, for v != u:
 *   far(v, u) = far(u, v) = (the field of source min(v, u), read at max(v, u)) > geo_min;      far(v, v) = 0.
 * The lower index is named as the source because the fp32 sum along a path is not the sum along its reverse.  An unreachable pair is
 * far.  THE MASK is a bit matrix [V, W = ceil(V / 32)] of uint32: bit (u & 31) of word (u >> 5) of row v holds far(v, u); bits past V
 * are 0.  far_pairs counts the unordered far pairs.  The handle copies what it needs of the model and may outlive it.
 *  - SMPLPP_ERR_INVALID (*out = NULL): geo_min negative or not finite, a rest value not finite, a NULL rest, a model without faces,
 *    V > 32768. */
int smplpp_self_contact_create(smplpp_model * m, const float * rest /*[V,3] host*/, float geo_min, struct smplpp_self_contact ** out);
int smplpp_self_contact_destroy(struct smplpp_self_contact * sc);
/* Each output nullable. */
int smplpp_self_contact_info(const struct smplpp_self_contact * sc, int64_t * V, int64_t * words_per_row, float * geo_min,
                             int64_t * far_pairs);
/* The mask [V,W] copied out in `space`. */
int smplpp_self_contact_mask(const struct smplpp_self_contact * sc, uint32_t * mask /*[V,W]*/, int space, void * stream);
/* smplpp_self_contact: for vertex v of frame i, vertex u of the same frame is a CANDIDATE when all of these hold:
 *  - far(v, u);
 *  - d = ((dx dx + dy dy) + dz dz), dx = x_v - x_u and so on, is finite and d <= max_sqdist (+inf: no cap);
 *  - with vert_normals, the two normals oppose (touching surfaces face each other): with m = n_v, q = n_u,
 *    s = (m.x q.x + m.y q.y) + m.z q.z, mm and qq the same sums of m with m and q with q:
 *      s <= 0  &&  mm qq > 0  &&  s s >= (cos_min cos_min) (mm qq),      cos_min in [0, 1]
 *    which are the bits of the normal test of smplpp_mesh_point_distance_compatible on (m, -q).  A normal that is not finite, or zero,
 *    matches nothing.
 * The answer is the candidate of smallest d, on equal d the lowest u: index [n,V], sqdist [n,V].  Without a candidate (also: a vertex
 * that is not finite) index = -1 and sqdist = +0.
 *  - SMPLPP_ERR_INVALID (outputs untouched): no handle, n <= 0, a NULL verts, index or sqdist, cos_min outside [0, 1], max_sqdist
 *    negative or NaN, n V 3 beyond int32 indexing, a bad space.
 * smplpp_self_contact_vjp: sqdist's vector-Jacobian product at the partners `index` the search chose.  There is no new product:
 * grad_verts has exactly the bits of two device calls in this order,
 *   smplpp_mesh_point_distance_vjp(verts, K = V, points = verts, index, grad_sqdist, grad_verts, NULL, accumulate), then
 *   smplpp_mesh_point_distance_vjp(the same, NULL, grad_points = grad_verts, accumulate = 1):
 * each vertex gets its own 2 g r, r = x_v - x_index, then one add brings in the ascending-v sum of -2 g r over the vertices that chose
 * it.  A zero cotangent or an index of -1 contributes nothing; a HOST-space index outside [-1, V) is refused.
 *  - SMPLPP_ERR_INVALID: as above, and a NULL index, grad_sqdist or grad_verts, accumulate not 0 or 1. */
int smplpp_self_contact(struct smplpp_self_contact * sc, int64_t n, const float * verts /*[n,V,3]*/,
                        const float * vert_normals /*[n,V,3] nullable*/, float cos_min, float max_sqdist, int64_t * index /*[n,V]*/,
                        float * sqdist /*[n,V]*/, int space, void * stream);
int smplpp_self_contact_vjp(struct smplpp_self_contact * sc, int64_t n, const float * verts /*[n,V,3]*/, const int64_t * index /*[n,V]*/,
                            const float * grad_sqdist /*[n,V]*/, float * grad_verts /*[n,V,3]*/, int accumulate, int space, void * stream);

#ifdef __cplusplus
}
#endif
#endif /* SMPLPP_HIP_H */
