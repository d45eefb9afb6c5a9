"""Host-side mirror of `smplpp::IkTask` (include/smplpp/IkTask.h:20-84), `smplpp::VPoserDecoder`
(include/smplpp/VPoser.h:53-90) and of the IK loop that lives in the reference's node `main()`
(node/node.cpp:645-1002), batched over independent frames, over the C ABI.

`IkTask` keeps the reference's public field names; `IkSolver` gathers a `dict name -> IkTask` per frame in
`std::map` (lexicographic) order — that order fixes the rows of e/J and the phi column blocks (node.cpp:47,798).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import DEVICE, HOST, SmplppError, check
from .smpl import SMPL, _Call, _np32, _ptr, torch

LATENT_DIM = 32
LATENT_POSE_DIM = LATENT_DIM + 12  # node/node.cpp:42


class IkTask:
    """One surface-point task.  Same public fields and defaults as the reference class."""

    def __init__(self, smpl: SMPL, faceIdx: int, targetPos=None, targetNormal=None):
        self.smpl_ = smpl
        self.faceIdx_ = int(faceIdx)
        self.posTaskWeight_ = 1.0
        self.normalTaskWeight_ = 1.0
        self.phiLimit_ = 0.04
        self.normalOffset_ = 0.0
        self.targetPos_ = np.zeros(3, np.float32) if targetPos is None else _np32(targetPos, (3,)).copy()
        self.targetNormal_ = np.array([0, 0, 1], np.float32) if targetNormal is None else _np32(targetNormal, (3,)).copy()
        self.vertexWeights_ = np.full(3, 1.0 / 3.0, np.float32)
        self.tangents_ = np.zeros((3, 2), np.float32)
        self.phi_ = np.zeros(2, np.float32)

    # The four methods evaluate on batch 0 of the SMPL instance's last launch, like the reference (src/IkTask.cpp:33-86);
    # they are thin host compositions of engine queries and exist for API parity — the batched solver does the same
    # arithmetic on the GPU for every frame.
    def _face_vertices(self):
        idx = self.smpl_.getFaceIndexRaw(self.faceIdx_).astype(np.int64) - 1
        v = self.smpl_.getVertexRaw(idx)
        return idx, (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v))

    def calcTangents(self):
        _, fv = self._face_vertices()
        t1 = fv[1] - fv[0]
        n = np.cross(t1, fv[2] - fv[0])
        t2 = np.cross(n, t1)
        t1 = t1 / max(np.linalg.norm(t1), 1e-12)
        t2 = t2 / max(np.linalg.norm(t2), 1e-12)
        self.tangents_ = np.stack([t1, t2], axis=1).astype(np.float32)

    def calcVertexWeights(self, actualPos):
        _, fv = self._face_vertices()
        pos = _np32(actualPos, (3,)) + self.tangents_ @ self.phi_
        w = np.array([np.linalg.norm(np.cross(fv[(i + 1) % 3] - pos, fv[(i + 2) % 3] - pos)) for i in range(3)], np.float32)
        self.vertexWeights_ = (w / w.sum()).astype(np.float32)

    def calcActualNormal(self):
        idx, _ = self._face_vertices()
        vn = self.smpl_.calcVertexNormal(idx)
        vn = vn.detach().cpu().numpy() if hasattr(vn, "detach") else np.asarray(vn)
        n = (self.vertexWeights_[:, None] * vn).sum(axis=0)
        return (n / max(np.linalg.norm(n), 1e-12)).astype(np.float32)

    def calcActualPos(self):
        _, fv = self._face_vertices()
        p = fv.T @ self.vertexWeights_
        if self.normalOffset_ > 0.0:
            p = p + np.float32(self.normalOffset_) * self.calcActualNormal()
        return p.astype(np.float32)


class VPoserDecoder:
    """smplpp::VPoserDecoder: weights in torch::nn::Linear layout, keys as scripts/preprocess_vposer.py:42-47 writes."""

    KEYS = ("decoder_net.0.weight", "decoder_net.0.bias", "decoder_net.3.weight", "decoder_net.3.bias",
            "decoder_net.5.weight", "decoder_net.5.bias")

    def __init__(self, params: Dict[str, np.ndarray], device=0):
        self.params = {k: _np32(params[k]) for k in self.KEYS}
        shapes = [(512, 32), (512,), (512, 512), (512,), (126, 512), (126,)]
        for k, s in zip(self.KEYS, shapes):
            if self.params[k].shape != s:
                raise SmplppError(1, "VPoser parameter %s has shape %s, expected %s" % (k, self.params[k].shape, s))
        _lib.require_gpu()
        h = C.c_void_p()
        check(_lib.load().smplpp_vposer_create(device, *[_ptr(self.params[k]) for k in self.KEYS], C.byref(h)))
        self._h = h

    @classmethod
    def loadParamsFromJson(cls, path, device=0):
        """VPoserDecoderImpl::loadParamsFromJson (src/VPoser.cpp:169-238); `.npz` from the same script also accepted."""
        if path.endswith(".npz"):
            with np.load(path) as z:
                return cls({k: z[k] for k in cls.KEYS}, device)
        import json

        with open(path) as f:
            raw = json.load(f)
        return cls({k: np.asarray(raw[k]) for k in cls.KEYS}, device)

    @staticmethod
    def synthetic_params(seed=3):
        """Stand-in weights (the real VPoser parameters are license-gated and absent): torch::nn::Linear
        default init (U(-1/sqrt(in), 1/sqrt(in))) with a fixed seed, except that the last layer is scaled by 0.3 and
        biased to the identity rotation in the 6D representation ([1,0, 0,1, 0,0] per joint) so that latents near zero
        decode to moderate poses, like a trained pose prior does, instead of uniformly random rotations."""
        rng = np.random.default_rng(seed)
        out = {}
        for (w, b), (o, i) in zip((("decoder_net.0.weight", "decoder_net.0.bias"), ("decoder_net.3.weight", "decoder_net.3.bias"),
                                   ("decoder_net.5.weight", "decoder_net.5.bias")), ((512, 32), (512, 512), (126, 512))):
            k = 1.0 / np.sqrt(i)
            out[w] = rng.uniform(-k, k, (o, i)).astype(np.float32)
            out[b] = rng.uniform(-k, k, (o,)).astype(np.float32)
        out["decoder_net.5.weight"] *= np.float32(0.3)
        out["decoder_net.5.bias"] = (np.float32(0.3) * out["decoder_net.5.bias"]
                                     + np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), 21)).astype(np.float32)
        return out

    def forward(self, latent, want_jac=False, frame_base=0):
        """`frame_base`: global index of latent[0] when the call decodes a shard of a larger job (same bits as the unsharded call)."""
        c, z = self._latent("forward", _np32(latent))
        out, jac = self._decode(c, z, want_jac, frame_base)
        return (out, jac) if want_jac else out

    def _latent(self, name, latent, *others, device_only=False):
        """The call of `name` and its latent [N,32] (numpy input: any shape of N * 32 values)."""
        c = _Call(name, latent, *others, device_only=device_only)
        z = latent if c.dev else _np32(latent).reshape(-1, 32)
        return c, c.input(z, (len(z), 32))

    def _decode(self, c, z, want_jac, frame_base):
        n = len(z)
        out, jac = c.empty((n, 21, 3)), c.empty((n, 63, 32)) if want_jac else None
        check(_lib.load().smplpp_vposer_forward_at(self._h, n, int(frame_base), _ptr(z), _ptr(out), _ptr(jac), c.space, c.stream))
        return out, jac

    def launchBackward(self, latent, grad_out, frame_base=0, want_out=False):
        """Vector-Jacobian product of the decode (smplpp_vposer_vjp): dL/dz [N,32] for dL/dout = grad_out [N,21,3] at latent
        [N,32].  The product is taken at the exact-fp32 decode `forward(latent)` returns; want_out=True also returns those angles
        ((grad_z, out)).  numpy in, numpy out (the call synchronises), or float32 device tensors (enqueued on torch's current
        stream).  `frame_base`: as in `forward` (the result does not depend on it)."""
        c, z = self._latent("launchBackward", latent, grad_out)
        n = len(z)
        g = c.input(grad_out, (n, 21, 3))
        gz, out = c.empty((n, 32)), c.empty((n, 21, 3)) if want_out else None
        check(_lib.load().smplpp_vposer_vjp(self._h, n, int(frame_base), _ptr(z), _ptr(g), _ptr(gz), _ptr(out), c.space, c.stream))
        return (gz, out) if want_out else gz

    def jacobian(self, latent, frame_base=0, want_out=False):
        """d(out)/dz [N,63,32] in exact fp32 (smplpp_vposer_jacobian) at latent [N,32], taken at the exact-fp32 decode `forward(latent)`
        returns; want_out=True also returns those angles ((jac, out)).  numpy in, numpy out (the call synchronises), or a float32
        device tensor (enqueued on torch's current stream).  `frame_base`: as in `forward` (the result does not depend on it)."""
        c, z = self._latent("jacobian", latent)
        n = len(z)
        jac, out = c.empty((n, 63, 32)), c.empty((n, 21, 3)) if want_out else None
        check(_lib.load().smplpp_vposer_jacobian(self._h, n, int(frame_base), _ptr(z), _ptr(out), _ptr(jac), c.space, c.stream))
        return (jac, out) if want_out else jac

    def forward_differentiable(self, latent):
        """Joint angles [N,21,3] for a float32 device tensor latent [N,32], differentiable with torch.autograd: the forward is
        smplpp_vposer_forward without a Jacobian (the exact-fp32 decode), the backward one smplpp_vposer_vjp, both on torch's
        current stream.  First derivatives with respect to the latent only."""
        if torch is None:
            raise SmplppError(1, "forward_differentiable needs torch")
        return _VPoserFunction.apply(latent, self)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().smplpp_vposer_destroy(self._h)
                self._h = None
        except Exception:
            pass


if torch is not None:
    class _VPoserFunction(torch.autograd.Function):
        """smplpp_vposer_forward (jac NULL) forward / smplpp_vposer_vjp backward (VPoserDecoder.forward_differentiable)."""

        @staticmethod
        def forward(ctx, latent, vposer):
            c, z = vposer._latent("forward_differentiable", latent, device_only=True)
            out, _ = vposer._decode(c, z, False, 0)
            ctx.vposer = vposer
            ctx.save_for_backward(z)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            z, = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None
            return ctx.vposer.launchBackward(z, grad_out), None


def theta_from_latent_layout(vposer: VPoserDecoder, q):
    """theta [N,25,3] from the reference's 44-d configuration q [N,44] = [root pos 3 | root rot 3 | z 32 | joint 22 aa 3 |
    joint 23 aa 3] (node/node.cpp:761-772, mocap.py's decode_theta): rows 0-1 and 23-24 are copied, rows 2-22 are the decode of z.
    Differentiable with torch.autograd (VPoserDecoder.forward_differentiable) for a float32 device tensor q."""
    if torch is None:
        raise SmplppError(1, "theta_from_latent_layout needs torch")
    if q.dim() != 2 or q.shape[1] != LATENT_POSE_DIM:
        raise SmplppError(1, "theta_from_latent_layout: expected q [N,%d], got %s" % (LATENT_POSE_DIM, tuple(q.shape)))
    n = q.shape[0]
    body = vposer.forward_differentiable(q[:, 6:38])
    return torch.cat([q[:, :6].reshape(n, 2, 3), body, q[:, 38:44].reshape(n, 2, 3)], dim=1)


def convertRotMatToAxisAngle(rotMat, device=0):
    """smplpp::convertRotMatToAxisAngle (src/VPoser.cpp:25-120)."""
    r = _np32(rotMat).reshape(-1, 3, 3)
    aa = np.empty((r.shape[0], 3), np.float32)
    check(_lib.load().smplpp_rotmat_to_axis_angle(device, r.shape[0], _ptr(r), _ptr(aa), HOST, None))
    return aa


class IkSolver:
    """The loop body of node/node.cpp:645-1002 for `n` independent frames with `K` tasks each."""

    def __init__(self, smpl: SMPL, n: int, K: int, vposer: Optional[VPoserDecoder] = None, frame_base: int = 0, exact: bool = False):
        """`frame_base`: global index of this solver's frame 0 when it holds one shard of a larger job (dist.shard_range).
        `exact`: the loops run the reference's arithmetic (smplpp_ik_set_arithmetic EXACT): the model's smplpp_fk form and the
        exact-fp32 decoder Jacobian; see setExactArithmetic."""
        self.smpl, self.n, self.K, self.vposer = smpl, int(n), int(K), vposer
        self.theta_dim = LATENT_POSE_DIM if vposer is not None else 75
        h = C.c_void_p()
        check(_lib.load().smplpp_ik_create(smpl.handle, self.n, self.K, vposer._h if vposer is not None else None, C.byref(h)))
        self._h = h
        if frame_base:
            check(_lib.load().smplpp_ik_set_frame_base(self._h, int(frame_base)))
        if exact:
            self.setExactArithmetic(True)
        self.task_names: Optional[List[str]] = None

    def setExactArithmetic(self, exact: bool = True):
        """smplpp_ik_set_arithmetic: True, the reference's arithmetic inside the loops (refused on a model created with
        SMPLPP_SKIN=h); False, the default (fp16x2 forward form and decoder Jacobian).  Takes effect from the next call."""
        check(_lib.load().smplpp_ik_set_arithmetic(self._h, 1 if exact else 0))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().smplpp_ik_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- tasks
    def setTasks(self, face_idx=None, vertex_weights=None, target_pos=None, target_normal=None, pos_task_weight=None,
                 normal_task_weight=None, phi_limit=None, normal_offset=None):
        """Struct-of-arrays over [n, K]; a [K]-shaped array is broadcast to every frame; None keeps the current value."""
        n, K = self.n, self.K

        def prep(a, dtype, tail):
            if a is None:
                return None
            a = np.asarray(a, dtype)
            if a.shape == (K,) + tail:
                a = np.broadcast_to(a, (n, K) + tail)
            if a.shape != (n, K) + tail:
                raise SmplppError(1, "task array has shape %s, expected %s" % (a.shape, (n, K) + tail))
            return np.ascontiguousarray(a)

        args = [prep(face_idx, np.int64, ()), prep(vertex_weights, np.float32, (3,)), prep(target_pos, np.float32, (3,)),
                prep(target_normal, np.float32, (3,)), prep(pos_task_weight, np.float64, ()),
                prep(normal_task_weight, np.float64, ()), prep(phi_limit, np.float64, ()), prep(normal_offset, np.float64, ())]
        check(_lib.load().smplpp_ik_set_tasks(self._h, *[_ptr(a) for a in args], HOST))

    def setTaskList(self, ikTaskList: Dict[str, IkTask]):
        """One `std::map<std::string, IkTask>` (node.cpp:47) broadcast to every frame, in its iteration order."""
        names = sorted(ikTaskList)
        if len(names) != self.K:
            raise SmplppError(1, "expected %d tasks, got %d" % (self.K, len(names)))
        self.task_names = names
        t = [ikTaskList[k] for k in names]
        self.setTasks([x.faceIdx_ for x in t], [x.vertexWeights_ for x in t], [x.targetPos_ for x in t],
                      [x.targetNormal_ for x in t], [x.posTaskWeight_ for x in t], [x.normalTaskWeight_ for x in t],
                      [x.phiLimit_ for x in t], [x.normalOffset_ for x in t])

    def getTasks(self):
        n, K = self.n, self.K
        face = np.empty((n, K), np.int64)
        vw = np.empty((n, K, 3), np.float32)
        tang = np.empty((n, K, 3, 2), np.float32)
        apos = np.empty((n, K, 3), np.float32)
        anrm = np.empty((n, K, 3), np.float32)
        check(_lib.load().smplpp_ik_get_tasks(self._h, _ptr(face), _ptr(vw), _ptr(tang), _ptr(apos), _ptr(anrm), HOST))
        return dict(face_idx=face, vertex_weights=vw, tangents=tang, actual_pos=apos, actual_normal=anrm)

    def getStatus(self):
        """Per-frame solve outcome (bit 0: the last solve hit "LLT has numerical issue!", node.cpp:934-937; bit 1: some
        solve did since setConfig / the sequence start; bit 4: the last solve was a box QP that ran out of active-set passes
        without meeting its optimality test) — what an enqueue-only caller checks after synchronising."""
        f = np.zeros(self.n, np.int32)
        check(_lib.load().smplpp_ik_get_status(self._h, _ptr(f), HOST, None))
        return f

    def getStep(self):
        """The fp64 step x [n, D] of the last solve of every frame (smplpp_ik_get_step): d theta [theta_dim] | phi [2K] |
        d beta [10 if that solve optimised beta], before the fp32 update.  Defined only for frames whose last solve ran and
        succeeded (not skipped, getStatus() bit 0 clear).  None before the first solve."""
        D = C.c_int64(0)
        check(_lib.load().smplpp_ik_get_step(self._h, None, C.byref(D), HOST, None))
        if D.value == 0:
            return None
        x = np.empty((self.n, D.value), np.float64)
        check(_lib.load().smplpp_ik_get_step(self._h, _ptr(x), C.byref(D), HOST, None))
        return x

    # ---- configuration g_beta / g_theta (node.cpp:44-45)
    def setConfig(self, beta=None, theta=None):
        b = _np32(beta, (self.n, 10)) if beta is not None else None
        t = _np32(theta).reshape(self.n, self.theta_dim) if theta is not None else None
        check(_lib.load().smplpp_ik_set_config(self._h, _ptr(b), _ptr(t), HOST))

    def getConfig(self):
        b = np.empty((self.n, 10), np.float32)
        t = np.empty((self.n, self.theta_dim), np.float32)
        check(_lib.load().smplpp_ik_get_config(self._h, _ptr(b), _ptr(t), HOST))
        return b, (t.reshape(self.n, 25, 3) if self.theta_dim == 75 else t)

    # ---- node.cpp:750-877
    def eval(self, optimize_beta=False):
        D = self.theta_dim + 2 * self.K + (10 if optimize_beta else 0)
        e = np.empty((self.n, 4 * self.K), np.float64)
        J = np.empty((self.n, 4 * self.K, D), np.float64)
        check(_lib.load().smplpp_ik_eval(self._h, int(optimize_beta), _ptr(e), _ptr(J), HOST, None))
        return e, J

    # ---- node.cpp:704-1001 x iters
    def iterate(self, iters, enable_qp=False, optimize_beta_from=-1, min_valid=0, sync=True, stream=None):
        e2 = np.empty(self.n, np.float64) if sync else None
        check(_lib.load().smplpp_ik_iterate(self._h, int(iters), int(enable_qp), int(optimize_beta_from), int(min_valid),
                                            _ptr(e2), HOST if sync else DEVICE, stream))
        return e2

    # ---- node.cpp:1369-1407 (+ :681-700): the frame loop of solveMocapMotion without a host round trip per frame
    def solveSequence(self, target_pos, valid, warmup_iters=32, iters_per_frame=1, enable_qp=True, min_valid=0):
        """target_pos [T,n,K,3] float32, valid [T,n,K] bool -> theta [T,n,theta_dim] after every frame.  target_pos [T,K,3] with valid
        [T,K]: ONE capture for all n chains (smplpp_ik_solve_sequence_shared: the targets are repeated on the device, not here)."""
        tp = np.ascontiguousarray(target_pos, np.float32)
        vl = np.ascontiguousarray(valid, np.uint8)
        T = tp.shape[0]
        shared = tp.ndim == 3
        if shared:
            assert tp.shape == (T, self.K, 3) and vl.shape == (T, self.K)
        else:
            assert tp.shape == (T, self.n, self.K, 3) and vl.shape == (T, self.n, self.K)
        out = np.empty((T, self.n, self.theta_dim), np.float32)
        fn = _lib.load().smplpp_ik_solve_sequence_shared if shared else _lib.load().smplpp_ik_solve_sequence
        check(fn(self._h, T, _ptr(tp), _ptr(vl), int(warmup_iters), int(iters_per_frame), int(enable_qp), int(min_valid), _ptr(out), HOST, None))
        return out

    def getVertices(self):
        v = np.empty((self.n, self.smpl.vertex_num, 3), np.float32)
        check(_lib.load().smplpp_ik_get_vertices(self._h, _ptr(v), HOST, None))
        return v


def task_surface_differentiable(smpl: SMPL, verts, face_idx, vertex_weights, normal_offset):
    """IkTask::calcActualPos / calcActualNormal (src/IkTask.cpp:58-86) batched over frames and tasks, differentiable with
    torch.autograd in `verts` [n,V,3] and in `vertex_weights` [n,K,3] (so a torch calcTriangleVertexWeights carries phi):
    face_idx [n,K] (0-based), normal_offset [n,K].  Returns (actual_pos [n,K,3], actual_normal [n,K,3]):
    actual_normal = normalize(sum_i w_i calcVertexNormal(face vertex i)), actual_pos = sum_i w_i v_i, plus
    normal_offset * actual_normal where normal_offset > 0.  The vertex normals are the engine's (vertex_normals_differentiable over
    the distinct vertices of the tasks' faces, backward through smplpp_vertex_normals_vjp); the rest is a few gathers."""
    if torch is None:
        raise SmplppError(1, "task_surface_differentiable needs torch")
    dev = verts.device
    n = verts.shape[0]
    faces = getattr(smpl, "_faces0_dev", None)
    if faces is None or faces.device != dev:
        faces = torch.from_numpy(smpl.getFaceIndex().astype(np.int64) - 1).to(dev)
        smpl._faces0_dev = faces
    face_idx = torch.as_tensor(face_idx, dtype=torch.int64, device=dev).reshape(n, -1)
    K = face_idx.shape[1]
    fv = faces[face_idx]  # [n,K,3] vertex ids
    ids, inv = torch.unique(fv.reshape(-1), sorted=True, return_inverse=True)
    vn = smpl.vertex_normals_differentiable(verts, ids)  # [n,U,3]
    fvn = vn.gather(1, inv.reshape(n, K * 3)[..., None].expand(n, K * 3, 3)).reshape(n, K, 3, 3)
    pts = verts.gather(1, fv.reshape(n, K * 3)[..., None].expand(n, K * 3, 3)).reshape(n, K, 3, 3)
    w = torch.as_tensor(vertex_weights, device=dev).to(verts.dtype).reshape(n, K, 3)
    # the reference's order: zeros, then += w_i * n_i for i = 0, 1, 2
    acc = w[..., 0:1] * fvn[:, :, 0]
    acc = acc + w[..., 1:2] * fvn[:, :, 1]
    acc = acc + w[..., 2:3] * fvn[:, :, 2]
    normal = torch.nn.functional.normalize(acc, dim=-1, eps=1e-12)
    # torch::matmul(faceVertices^T, vertexWeights)
    pos = (pts * w[..., None]).sum(dim=2)
    off = torch.as_tensor(normal_offset, device=dev).to(verts.dtype).reshape(n, K)
    off = torch.where(off > 0, off, torch.zeros_like(off))
    pos = pos + off[..., None] * normal
    return pos, normal


def reference_task_faces(K=6):
    """The reference's four end-effector tasks (node/node.cpp:538-550: LeftFoot f5925, LeftHand f2581, RightFoot f12812,
    RightHand f9469) plus HeadTop f7324 and Chest f6842 from its mocap table (:455,:459), in std::map order."""
    table = {"LeftHand": 2581, "RightHand": 9469, "LeftFoot": 5925, "RightFoot": 12812, "HeadTop": 7324, "Chest": 6842}
    names = sorted(list(table)[:K])
    return names, np.array([table[k] for k in names], np.int64)
