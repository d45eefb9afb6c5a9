"""Host-side mirror of the reference's `smplpp::SMPL` façade (include/smplpp/SMPL.h:140-270) over the C ABI.

Same method names and argument meaning as the reference class; tensors are numpy arrays (host: the call stages
and synchronises) or torch tensors on the MI355X (device: the call only enqueues on torch's current stream).
PyTorch is used for device memory and streams only — every number is produced by libsmplpp_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib, model_io
from ._lib import DEVICE, HOST, SmplppError, check

try:  # torch is plumbing (device buffers, streams); the package works with numpy alone
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _np32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a


def _ptr(a):
    """Address of a numpy array / torch tensor / None."""
    if a is None:
        return None
    if _is_torch(a):
        return a.data_ptr()
    return a.ctypes.data


def _stream():
    if torch is not None and torch.cuda.is_available():
        return torch.cuda.current_stream().cuda_stream
    return None


SELF_PAIRS_DEFAULT = 32768  # default max_pairs of the self-intersection calls


def pinhole_camera(R, t, fx, fy, cx, cy, n=None):
    """The camera rows smplpp_depth_raster reads, [n,16] float32: R (world -> camera, row-major), t, fx, fy, cx, cy.  The camera looks
    along +z, x right, y down; pixel (row j, column i) has its centre at (i + 0.5, j + 0.5).  R [3,3] or [n,3,3], t [3] or [n,3],
    scalars or [n]; one camera is broadcast to n frames."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    k = n if n is not None else max([1] + [len(a) for a, d in ((R, 3), (t, 2)) if a.ndim == d] +
                                    [np.size(a) for a in (fx, fy, cx, cy) if np.ndim(a) > 0])
    cam = np.empty((k, 16), np.float32)
    cam[:, :9] = R.reshape(-1, 9)
    cam[:, 9:12] = t.reshape(-1, 3)
    for j, a in enumerate((fx, fy, cx, cy)):
        cam[:, 12 + j] = np.asarray(a, np.float64).reshape(-1)
    return cam


def pinhole_camera_rows(camera, n):
    """camera [16] or [n,16] as contiguous float32 [n,16]."""
    camera = np.asarray(camera, np.float32)
    if camera.ndim == 1:
        camera = np.broadcast_to(camera, (n,) + camera.shape)
    return np.ascontiguousarray(camera)


def camera_rays(camera, H, W):
    """The depth rasteriser's pixel-centre rays in world space, for SMPL.rayCast: (origin [n,H*W,3], dir [n,H*W,3]) float32 of camera
    rows [n,16] (or [16]) as pinhole_camera lays them out.  Pixel (row j, column i) is ray j * W + i with origin -R^T t and
    dir = R^T ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1), so the range t along it is the rasteriser's depth.  Formed in float64,
    then rounded once."""
    cam = np.asarray(camera, np.float64).reshape(-1, 16)
    R, t = cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12]
    j, i = np.meshgrid(np.arange(int(H), dtype=np.float64), np.arange(int(W), dtype=np.float64), indexing="ij")
    dx = ((i.reshape(1, -1) + 0.5) - cam[:, 14:15]) / cam[:, 12:13]
    dy = ((j.reshape(1, -1) + 0.5) - cam[:, 15:16]) / cam[:, 13:14]
    dc = np.stack([dx, dy, np.ones_like(dx)], 2)
    origin = np.broadcast_to(-np.einsum("nji,nj->ni", R, t)[:, None], dc.shape)
    return np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(np.einsum("nji,nkj->nki", R, dc), np.float32)


class _Call:
    """The memory space of one ABI call, decided by its first array argument: numpy arrays are host space (converted to float32; the
    call stages and synchronises), torch tensors device space (CUDA float32 only; enqueued on torch's current stream).  `fail` is
    the message of every refusal when the reference words it; `device_only` refuses host space."""

    def __init__(self, name, *arrays, fail=None, device_only=False):
        self.name, self.fail = name, fail
        first = next(a for a in arrays if a is not None)
        self.dev = _is_torch(first)
        for a in arrays:
            if a is not None and _is_torch(a) != self.dev:
                self.refuse("mix of torch tensors and numpy arrays")
        if device_only and not self.dev:
            self.refuse("expected float32 device tensors")
        self.space, self.stream = (DEVICE, _stream()) if self.dev else (HOST, None)
        self.device = first.device if self.dev else None

    def refuse(self, what):
        raise SmplppError(1, self.fail or "%s: %s" % (self.name, what))

    def input(self, a, shape):
        """`a` checked against `shape` and ready to pass (None stays None)."""
        if a is None:
            return None
        if self.dev:
            if not (a.is_cuda and a.dtype == torch.float32 and a.shape == shape):
                self.refuse("expected a float32 device tensor of shape %s" % (shape,))
            return (a.detach() if a.requires_grad else a).contiguous()  # a detach() is a new tensor object per call
        a = _np32(a)
        if a.shape != shape:
            self.refuse("expected shape %s, got %s" % (shape, a.shape))
        return a

    def inout(self, a, shape):
        """An array the call adds into: checked, never converted."""
        if self.dev:
            ok = a.is_cuda and a.dtype == torch.float32 and a.shape == shape and a.is_contiguous()
        else:
            ok = isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == shape and a.flags.c_contiguous
        if not ok:
            self.refuse("out must be a contiguous float32 array of shape %s" % (shape,))
        return a.detach() if self.dev else a

    def ids(self, ids):
        """Flat int64 ids in this call's space."""
        if self.dev and _is_torch(ids) and ids.is_cuda:
            return ids.detach().to(dtype=torch.int64).contiguous().reshape(-1)
        ids = np.ascontiguousarray(ids.detach().cpu().numpy() if _is_torch(ids) else np.atleast_1d(ids), np.int64).reshape(-1)
        return torch.from_numpy(ids).to(self.device) if self.dev else ids

    def flags(self, flags):
        """Flat uint8 flags (nonzero = set) in this call's space."""
        if self.dev and _is_torch(flags) and flags.is_cuda:
            return flags.detach().to(dtype=torch.uint8).contiguous().reshape(-1)
        flags = np.ascontiguousarray(flags.detach().cpu().numpy() if _is_torch(flags) else np.atleast_1d(flags), np.uint8).reshape(-1)
        return torch.from_numpy(flags).to(self.device) if self.dev else flags

    def empty(self, shape, dtype="float32"):
        if self.dev:
            return torch.empty(shape, dtype=getattr(torch, dtype), device=self.device)
        return np.empty(shape, dtype)


def _pp_inputs(c, points, camera, target, device):
    """(n, K, points, camera, target, device index) of a projection call in the space of `c`."""
    if len(points.shape) != 3 or points.shape[2] != 3 or min(points.shape) < 1:
        c.refuse("expected points of shape (N, K, 3)")
    n, K = int(points.shape[0]), int(points.shape[1])
    if not c.dev:
        camera = pinhole_camera_rows(camera, n)
    dev = c.device.index if c.dev and c.device.index is not None else device
    return n, K, c.input(points, (n, K, 3)), c.input(camera, (n, 16)), c.input(target, (n, K, 3)), int(dev)


def project_points(points, camera, target=None, rho=0.0, near=0.05, want=("uv", "energy", "valid"), device=0):
    """Any points [N,K,3] (landmarks, or raw vertices) through the cameras [N,16] ([16] with numpy: one camera for every frame) by the
    depth rasteriser's vertex rule, and their 2-D keypoint energy against target [N,K,3] = (u, v, confidence) (smplpp_project_points):
    a dict of uv [N,K,2], energy [N,K] (with a target; c^2 q for rho = 0, else the Geman-McClure form c^2 rho^2 q / (rho^2 + q) on the
    squared pixel distance q) and valid [N,K] uint8.  A refused point (behind `near`, not finite, outside the guard band) gives
    valid 0, uv 0 and energy 0.  numpy (the call synchronises, on `device`) or float32 device tensors (torch's current stream)."""
    c = _Call("project_points", points, target)
    n, K, points, camera, target, dev = _pp_inputs(c, points, camera, target, device)
    shapes = {"uv": ((n, K, 2), "float32"), "energy": ((n, K), "float32"), "valid": ((n, K), "uint8")}
    out = {k: c.empty(*shapes[k]) for k in shapes if k in want and (k != "energy" or target is not None)}
    check(_lib.load().smplpp_project_points(dev, n, K, _ptr(points), _ptr(camera), float(near), _ptr(target), float(rho), _ptr(out.get("uv")),
                                            _ptr(out.get("energy")), _ptr(out.get("valid")), c.space, c.stream))
    return out


def project_points_backward(points, camera, target=None, rho=0.0, grad_uv=None, grad_energy=None, near=0.05, want=("points", "camera"),
                            out=None, device=0):
    """Vector-Jacobian product of project_points (smplpp_project_points_vjp): {"points": [N,K,3], "camera": [N,16]} for dL/duv =
    grad_uv [N,K,2] and dL/denergy = grad_energy [N,K] (either may be None).  "camera" is in the layout of the camera rows, with R as
    nine independent entries.  `want` drops one; with `out` (a dict keyed the same way) the gradients are added into its arrays."""
    acc = out is not None
    c = _Call("project_points_backward", points, target, grad_uv, grad_energy, *(out.values() if acc else ()))
    n, K, points, camera, target, dev = _pp_inputs(c, points, camera, target, device)
    guv, ge = c.input(grad_uv, (n, K, 2)), c.input(grad_energy, (n, K))
    shapes = {"points": (n, K, 3), "camera": (n, 16)}
    keys = [k for k in shapes if k in (out if acc else want)]
    if not keys:
        c.refuse("points or camera must be asked for")
    res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
    check(_lib.load().smplpp_project_points_vjp(dev, n, K, _ptr(points), _ptr(camera), float(near), _ptr(target), float(rho), _ptr(guv),
                                                _ptr(ge), _ptr(res.get("points")), _ptr(res.get("camera")), int(acc), c.space, c.stream))
    return res


def project_points_differentiable(points, camera, target, rho, near=0.05):
    """(uv [N,K,2], energy [N,K], valid [N,K] bool) of device tensors points [N,K,3], camera [N,16], target [N,K,3] (the bits of
    project_points), differentiable in points AND camera through torch.autograd: smplpp_project_points forward,
    smplpp_project_points_vjp backward, on torch's current stream.  A keypoint term is energy.sum()."""
    if torch is None:
        raise SmplppError(1, "project_points_differentiable needs torch")
    return _ProjectPointsFunction.apply(points, camera, target, float(rho), float(near))


def rot6d_to_rotmat(x):
    """The 6-D rotation representation as rotation matrices, [..., 6] -> [..., 3, 3], in plain differentiable torch: x[..., 0::2] and
    x[..., 1::2] are read as the first two columns (the [..., 3, 2] view of the reference's decoder, src/VPoser.cpp:129-141); b1 =
    normalize(a1), b2 = normalize(a2 - (b1 . a2) b1), b3 = b1 x b2, stacked as columns.  On the first two columns of a rotation
    it is the identity.  With SMPL.forward_rotmat_differentiable the 6-D output of a regressor drives the body end to end, with
    no axis-angle in between."""
    if torch is None:
        raise SmplppError(1, "rot6d_to_rotmat needs torch")
    if x.shape[-1] != 6:
        raise SmplppError(1, "rot6d_to_rotmat: expected [..., 6], got %s" % (tuple(x.shape),))
    m = x.reshape(*x.shape[:-1], 3, 2)
    a1, a2 = m[..., 0], m[..., 1]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack([b1, b2, b3], dim=-1)


def parse_device(device) -> int:
    """Reference: `torch::Device` with an explicit index (src/SMPL.cpp:289-297); "CUDA" selects the GPU engine
    (node/node.cpp:360-371).  There is no CPU engine here."""
    if isinstance(device, int):
        return device
    s = str(device).lower()
    if s.startswith("cpu"):
        raise SmplppError(1, "smplpp_amd has no CPU engine: use device 'cuda:<i>' / 'hip:<i>' (MI355X)")
    if ":" not in s:
        raise SmplppError(1, "Failed to fetch device index!")  # src/SMPL.cpp:295
    return int(s.split(":")[1])


class SMPL:
    def __init__(self):
        self._h = None
        self._device = 0
        self._path = None
        self._model = None
        self._out = {}
        self._n = 0

    # ---- setters / init (SMPL.h:241-246)
    def setDevice(self, device):
        self._device = parse_device(device)

    def getDevice(self):
        return "cuda:%d" % self._device

    def setModelPath(self, modelPath: str):
        self._path = modelPath

    def init(self, model: Optional[dict] = None):
        """SMPL::init (src/SMPL.cpp:560-643).  `model` (the seven arrays of scripts/preprocess.py:98-117) may be
        passed directly instead of a path — needed here because the real parameter files are license-gated."""
        if model is None:
            if self._path is None:
                raise SmplppError(1, "Cannot initialize a SMPL model!")
            model = model_io.load_model(self._path)
        m = model_io._normalise(model)
        self._model = m
        L = _lib.load()
        _lib.require_gpu()
        if self._h:
            check(L.smplpp_model_destroy(self._h))
            self._h = None
        h = C.c_void_p()
        check(L.smplpp_model_create(
            m["vertices_template"].shape[0], m["face_indices"].shape[0], _ptr(m["vertices_template"]),
            _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]), _ptr(m["joint_regressor"]), _ptr(m["weights"]),
            _ptr(m["kinematic_tree"]), _ptr(m["face_indices"]), self._device, C.byref(h)))
        self._h = h
        self.vertex_num = m["vertices_template"].shape[0]
        self.face_num = m["face_indices"].shape[0]

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "Cannot launch a SMPL model!")  # src/SMPL.cpp:676
        return self._h

    def info(self):
        V, F, w, d = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        check(_lib.load().smplpp_model_info(self.handle, C.byref(V), C.byref(F), C.byref(w), C.byref(d)))
        return dict(vertex_num=V.value, face_num=F.value, weights_per_vertex=w.value, device=d.value)

    # ---- measurement hook
    def profileEnable(self, enable=True):
        check(_lib.load().smplpp_profile_enable(self.handle, int(enable)))

    def profileRead(self):
        """(launches, mean fused-kernel duration in ms) since the last read; HIP events on the launch stream."""
        n, ms = C.c_int64(), C.c_double()
        check(_lib.load().smplpp_profile_read(self.handle, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # ---- launch (SMPL.h:268, src/SMPL.cpp:671-737)
    def launch(self, beta, theta, want=("verts", "joints", "xforms", "rest"), out=None):
        """beta [N,10], theta [N,25,3] (row 0 = root translation).  Outputs are kept for the getters.
        `out` (optional dict of preallocated arrays/tensors keyed like `want`) avoids per-call allocation."""
        c = _Call("launch", beta, theta, fail="Cannot launch a SMPL model!")
        _, theta, out = self._fk(c, beta, theta, want, out)
        self._out, self._n, self._theta = out, theta.shape[0], theta
        return out

    def _fk(self, c, beta, theta, want, out=None):
        """smplpp_fk in the space of `c`: (beta, theta as passed to it, {"verts", "joints", "xforms", "rest"})."""
        n, V = beta.shape[0] if c.dev else len(beta), self.vertex_num  # shape[0]: Tensor.__len__ is Python code
        beta, theta = c.input(beta, (n, 10)), c.input(theta, (n, 25, 3))
        pre = out or {}
        out = {k: pre[k] if k in pre else (c.empty(s) if k in want else None)
               for k, s in (("verts", (n, V, 3)), ("joints", (n, 24, 3)), ("xforms", (n, 24, 4, 4)), ("rest", (n, V, 3)))}
        check(_lib.load().smplpp_fk(self.handle, n, _ptr(beta), _ptr(theta), _ptr(out["verts"]), _ptr(out["joints"]),
                                    _ptr(out["xforms"]), _ptr(out["rest"]), c.space, c.stream))
        return beta, theta, out

    def launchBackward(self, beta, theta, grad_verts=None, grad_joints=None, rest=None):
        """Vector-Jacobian product of `launch` (smplpp_fk_vjp): dL/dbeta [N,10] and dL/dtheta [N,25,3] for dL/dverts = grad_verts
        [N,V,3] and dL/djoints = grad_joints [N,24,3] (None = zero).  `rest` [N,V,3] is the rest shape `launch` returned for these
        inputs; None recomputes it inside the call.  numpy in, numpy out (the call synchronises), or torch tensors on the device
        (enqueued on torch's current stream).  Returns {"beta": ..., "theta": ...}."""
        c = _Call("launchBackward", beta, theta, grad_verts, grad_joints, rest)
        n, V = len(beta), self.vertex_num
        beta, theta = c.input(beta, (n, 10)), c.input(theta, (n, 25, 3))
        gv, gj, rest = c.input(grad_verts, (n, V, 3)), c.input(grad_joints, (n, 24, 3)), c.input(rest, (n, V, 3))
        out = {"beta": c.empty((n, 10)), "theta": c.empty((n, 25, 3))}
        check(_lib.load().smplpp_fk_vjp(self.handle, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), _ptr(gj), _ptr(out["beta"]),
                                        _ptr(out["theta"]), c.space, c.stream))
        return out

    def forward_differentiable(self, beta, theta):
        """(verts [N,V,3], joints [N,24,3]) for device tensors beta [N,10], theta [N,25,3], differentiable with torch.autograd:
        the forward is one smplpp_fk (rest shape kept for the backward), the backward one smplpp_fk_vjp, both on torch's current
        stream.  First derivatives with respect to beta and theta only."""
        if torch is None:
            raise SmplppError(1, "forward_differentiable needs torch")
        return _FKFunction.apply(beta, theta, self)

    # ---- launch from rotation matrices (smplpp_axis_angle_to_rotmat / smplpp_fk_rotmat / smplpp_fk_rotmat_vjp)
    def axisAngleToRotmat(self, aa):
        """Axis-angles [..., 3] as rotation matrices [..., 3, 3], row-major (smplpp_axis_angle_to_rotmat): the reference's Rodrigues
        formula with the bits `launch` computes internally, so launchRotmat(beta, theta[:, 0], axisAngleToRotmat(theta[:, 1:]))
        returns the bits of launch(beta, theta).  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("axisAngleToRotmat", aa)
        shape = tuple(aa.shape) if c.dev else np.shape(aa)
        if not shape or shape[-1] != 3 or int(np.prod(shape)) == 0:
            c.refuse("expected axis-angles of shape (..., 3)")
        rows = int(np.prod(shape[:-1]))
        aa = c.input(aa.reshape(rows, 3) if c.dev else _np32(aa).reshape(rows, 3), (rows, 3))
        rot = c.empty((rows, 3, 3))
        check(_lib.load().smplpp_axis_angle_to_rotmat(self._device, rows, _ptr(aa), _ptr(rot), c.space, c.stream))
        return rot.reshape(tuple(shape[:-1]) + (3, 3))

    def axisAngleToRotmatBackward(self, aa, grad_rot, out=None):
        """Vector-Jacobian product of axisAngleToRotmat (smplpp_axis_angle_to_rotmat_vjp): dL/daa [..., 3] for dL/drot = grad_rot
        [..., 3, 3], nine independent entries per matrix, by the derivative skeletonBackward and launchBackward contract with (finite
        at aa = 0 and at |aa| = pi).  With `out` the gradient is added into it.  orientation.axis_angle_to_rotmat_differentiable is
        the autograd form."""
        from . import orientation

        return orientation.axis_angle_to_rotmat_backward(aa, grad_rot, out=out, device=self._device)

    def _fk_rotmat(self, c, beta, trans, rot, want, out=None):
        """smplpp_fk_rotmat in the space of `c`: (beta, trans, rot as passed to it, {"verts", "joints", "xforms", "rest"})."""
        n, V = int(rot.shape[0]) if c.dev else len(rot), self.vertex_num
        beta, trans, rot = c.input(beta, (n, 10)), c.input(trans, (n, 3)), c.input(rot, (n, 24, 3, 3))
        pre = out or {}
        out = {k: pre[k] if k in pre else (c.empty(s) if k in want else None)
               for k, s in (("verts", (n, V, 3)), ("joints", (n, 24, 3)), ("xforms", (n, 24, 4, 4)), ("rest", (n, V, 3)))}
        check(_lib.load().smplpp_fk_rotmat(self.handle, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(out["verts"]), _ptr(out["joints"]),
                                           _ptr(out["xforms"]), _ptr(out["rest"]), c.space, c.stream))
        return beta, trans, rot, out

    def launchRotmat(self, beta, trans, rot, want=("verts", "joints", "xforms", "rest"), out=None):
        """`launch` from rotation matrices (smplpp_fk_rotmat): beta [N,10] (None = zero), trans [N,3] the root translation (None =
        zero), rot [N,24,3,3] row-major with joint 0 the root orientation.  The matrices are used as given, without
        re-orthonormalisation.  Outputs are kept for the getters, as launch keeps them; `out` as in launch.  The result feeds
        vertexOffsets directly (it returns xforms), and launchRotmatBackward(rest=rest + D) then gives the SMPL+D chain rule exactly
        as launchBackward does."""
        c = _Call("launchRotmat", rot, beta, trans, fail="Cannot launch a SMPL model!")
        _, _, rot, out = self._fk_rotmat(c, beta, trans, rot, want, out)
        self._out, self._n = out, rot.shape[0]
        return out

    def launchRotmatBackward(self, beta, trans, rot, grad_verts=None, grad_joints=None, rest=None):
        """Vector-Jacobian product of `launchRotmat` (smplpp_fk_rotmat_vjp): {"beta": dL/dbeta [N,10], "trans": dL/dtrans [N,3],
        "rot": dL/drot [N,24,3,3]} for dL/dverts = grad_verts [N,V,3] and dL/djoints = grad_joints [N,24,3] (None = zero).  "rot" is
        the gradient to nine independent entries per joint (no projection onto the rotations, no singularity).  `rest` as in
        launchBackward: the rest shape launchRotmat returned, rest + D for an SMPL+D body, or None to recompute it."""
        c = _Call("launchRotmatBackward", rot, beta, trans, grad_verts, grad_joints, rest)
        n, V = int(rot.shape[0]) if c.dev else len(rot), self.vertex_num
        beta, trans, rot = c.input(beta, (n, 10)), c.input(trans, (n, 3)), c.input(rot, (n, 24, 3, 3))
        gv, gj, rest = c.input(grad_verts, (n, V, 3)), c.input(grad_joints, (n, 24, 3)), c.input(rest, (n, V, 3))
        out = {"beta": c.empty((n, 10)), "trans": c.empty((n, 3)), "rot": c.empty((n, 24, 3, 3))}
        check(_lib.load().smplpp_fk_rotmat_vjp(self.handle, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(rest), _ptr(gv), _ptr(gj),
                                               _ptr(out["beta"]), _ptr(out["trans"]), _ptr(out["rot"]), c.space, c.stream))
        return out

    def forward_rotmat_differentiable(self, beta, trans, rot):
        """(verts [N,V,3], joints [N,24,3], xforms [N,24,4,4]) for device tensors beta [N,10], trans [N,3], rot [N,24,3,3],
        differentiable with torch.autograd in all three inputs: the forward is one smplpp_fk_rotmat (rest shape kept for the
        backward), the backward one smplpp_fk_rotmat_vjp, on torch's current stream.  First derivatives only.  xforms carries no
        gradient (it is marked non-differentiable), as forward_differentiable returns none for them: it is there to feed
        vertexOffsets.  rot6d_to_rotmat in front gives the 6-D parametrisation."""
        if torch is None:
            raise SmplppError(1, "forward_rotmat_differentiable needs torch")
        return _FKRotmatFunction.apply(beta, trans, rot, self)

    # ---- forward mode (smplpp_fk_jvp / smplpp_fk_rotmat_jvp): tangents of the vertices, the rest joints and the world joint frames
    _TANGENT_OUT = (("verts", None), ("joints", (24, 3)), ("world", (24, 3, 4)))

    def _tangent(self, name, rot_in, beta, trans, pose, tangents, rest, shared, want, out):
        """One forward-mode call: `tangents` = (dbeta, dtheta) or (dbeta, dtrans, drot), each [n,T,...] or, shared, [T,...]."""
        c = _Call(name, pose, beta, trans, rest, *tangents, *((out or {}).values()))
        n, V = int(pose.shape[0]) if c.dev else len(pose), self.vertex_num
        first = next((t for t in tangents if t is not None), None)
        if first is None:
            c.refuse("at least one tangent must be given")
        shape = tuple(first.shape) if c.dev else np.shape(first)
        lead = 1 if shared else 2
        if len(shape) < lead + 1 or (not shared and shape[0] != n):
            c.refuse("tangents carry a T axis: [n,T,...], or [T,...] when shared")
        T = int(shape[lead - 1])
        pre = (T,) if shared else (n, T)
        tails = ((10,), (3,), (24, 3, 3)) if rot_in else ((10,), (25, 3))
        tangents = [c.input(t, pre + s) for t, s in zip(tangents, tails)]
        beta, trans = c.input(beta, (n, 10)), c.input(trans, (n, 3))
        pose, rest = c.input(pose, (n, 24, 3, 3) if rot_in else (n, 25, 3)), c.input(rest, (n, V, 3))
        given = out or {}
        res = {k: c.inout(given[k], (n, T) + (s or (V, 3))) if k in given else (c.empty((n, T) + (s or (V, 3))) if k in want else None)
               for k, s in self._TANGENT_OUT}
        if all(v is None for v in res.values()):
            c.refuse("verts, joints or world must be asked for")
        ptrs = [_ptr(res[k]) for k, _ in self._TANGENT_OUT]
        L = _lib.load()
        if rot_in:
            check(L.smplpp_fk_rotmat_jvp(self.handle, n, T, _ptr(beta), _ptr(trans), _ptr(pose), _ptr(rest), _ptr(tangents[0]),
                                         _ptr(tangents[1]), _ptr(tangents[2]), int(bool(shared)), *ptrs, c.space, c.stream))
        else:
            check(L.smplpp_fk_jvp(self.handle, n, T, _ptr(beta), _ptr(pose), _ptr(rest), _ptr(tangents[0]), _ptr(tangents[1]),
                                  int(bool(shared)), *ptrs, c.space, c.stream))
        return {k: v for k, v in res.items() if v is not None}

    def launchTangent(self, beta, theta, dbeta=None, dtheta=None, rest=None, shared=False, want=("verts", "joints", "world"), out=None):
        """Jacobian-vector product of `launch` and `skeleton` (smplpp_fk_jvp): for T tangents (dbeta [N,T,10], dtheta [N,T,25,3]; None =
        zero, not both; row 0 of dtheta is the tangent of the root translation) a dict of verts [N,T,V,3], joints [N,T,24,3] (the REST
        joints) and world [N,T,24,3,4] (`skeleton`'s world): how each output changes along each tangent.  With dtheta = the pose rate
        these are velocities.  shared=True: the tangents are [T,10] / [T,25,3], one set applied to every frame.  `rest` as in
        launchBackward (None recomputes it; rest + D for an SMPL+D body).  `want` drops outputs (without "verts" the call is one
        small kernel); `out` (a dict keyed the same way) supplies preallocated arrays.  numpy (the call synchronises) or float32
        device tensors (torch's current stream).  Deterministic; a (frame, tangent)'s bits do not depend on N, T or its place."""
        return self._tangent("launchTangent", False, beta, None, theta, (dbeta, dtheta), rest, shared, want, out)

    def launchRotmatTangent(self, beta, trans, rot, dbeta=None, dtrans=None, drot=None, rest=None, shared=False,
                            want=("verts", "joints", "world"), out=None):
        """launchTangent for the rotation-matrix entry (smplpp_fk_rotmat_jvp): tangents dbeta [N,T,10], dtrans [N,T,3] and drot
        [N,T,24,3,3] (nine independent entries per joint, used as given; None = zero, not all three); shared=True drops their
        leading N.  beta and trans may be None (zero).  Outputs, `rest`, `want` and `out` as in launchTangent."""
        return self._tangent("launchRotmatTangent", True, beta, trans, rot, (dbeta, dtrans, drot), rest, shared, want, out)

    def jacobian(self, beta, theta, wrt=("beta", "theta"), rest=None, want=("verts",)):
        """The dense Jacobian of `launch` / `skeleton` by one launchTangent on the shared one-hot basis: a dict keyed like `want` of
        verts [N,T,V,3], joints [N,T,24,3], world [N,T,24,3,4], whose axis 1 is the TANGENT AXIS: T = 10 (if "beta" in wrt) + 75 (if
        "theta" in wrt), beta's ten columns first, then theta's 25 x 3 in row-major order (row 0 = the root translation).  So
        out["verts"][f].reshape(T, -1).T is the [3V, T] Jacobian of frame f."""
        c = _Call("jacobian", beta, theta, rest)
        nb, nt = (10 if "beta" in wrt else 0), (75 if "theta" in wrt else 0)
        if nb + nt == 0:
            c.refuse("wrt must name beta or theta")
        eye = np.eye(nb + nt, dtype=np.float32)
        db = np.ascontiguousarray(eye[:, :nb]) if nb else None
        dt = np.ascontiguousarray(eye[:, nb:]).reshape(nb + nt, 25, 3) if nt else None
        if c.dev:
            db, dt = (None if a is None else torch.from_numpy(a).to(c.device) for a in (db, dt))
        return self.launchTangent(beta, theta, dbeta=db, dtheta=dt, rest=rest, shared=True, want=want)

    # ---- the skeleton alone (smplpp_skeleton / smplpp_skeleton_rotmat and their vector-Jacobian products)
    _SKELETON_OUT = (("world", (24, 3, 4)), ("posed", (24, 3)), ("joints", (24, 3)))

    def _skeleton(self, c, beta, trans, pose, rot_in, want, out=None):
        """smplpp_skeleton (pose = theta) or smplpp_skeleton_rotmat (pose = rot) in the space of `c`: (beta, trans, pose as passed to
        it, {"world", "posed", "joints"})."""
        n = int(pose.shape[0]) if c.dev else len(pose)
        beta, trans = c.input(beta, (n, 10)), c.input(trans, (n, 3))
        pose = c.input(pose, (n, 24, 3, 3) if rot_in else (n, 25, 3))
        pre = out or {}
        out = {k: c.inout(pre[k], (n,) + s) if k in pre else (c.empty((n,) + s) if k in want else None) for k, s in self._SKELETON_OUT}
        if all(v is None for v in out.values()):
            c.refuse("world, posed or joints must be asked for")
        ptrs = [_ptr(out[k]) for k, _ in self._SKELETON_OUT]
        L = _lib.load()
        if rot_in:
            check(L.smplpp_skeleton_rotmat(self.handle, n, _ptr(beta), _ptr(trans), _ptr(pose), *ptrs, c.space, c.stream))
        else:
            check(L.smplpp_skeleton(self.handle, n, _ptr(beta), _ptr(pose), *ptrs, c.space, c.stream))
        return beta, trans, pose, {k: v for k, v in out.items() if v is not None}

    def _skeleton_backward(self, name, beta, trans, pose, rot_in, grad_world, grad_posed, grad_joints, want, out):
        acc = out is not None
        c = _Call(name, pose, beta, trans, grad_world, grad_posed, grad_joints, *(out.values() if acc else ()))
        n = int(pose.shape[0]) if c.dev else len(pose)
        beta, trans = c.input(beta, (n, 10)), c.input(trans, (n, 3))
        pose = c.input(pose, (n, 24, 3, 3) if rot_in else (n, 25, 3))
        gw, gp, gj = c.input(grad_world, (n, 24, 3, 4)), c.input(grad_posed, (n, 24, 3)), c.input(grad_joints, (n, 24, 3))
        if gw is None and gp is None and gj is None:
            c.refuse("grad_world, grad_posed or grad_joints must be given")
        shapes = {"beta": (n, 10), "trans": (n, 3), "rot": (n, 24, 3, 3)} if rot_in else {"beta": (n, 10), "theta": (n, 25, 3)}
        keys = [k for k in shapes if k in (out if acc else want)]
        if not keys:
            c.refuse("%s must be asked for" % " or ".join(shapes))
        res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
        L = _lib.load()
        if rot_in:
            check(L.smplpp_skeleton_rotmat_vjp(self.handle, n, _ptr(beta), _ptr(trans), _ptr(pose), _ptr(gw), _ptr(gp), _ptr(gj),
                                               _ptr(res.get("beta")), _ptr(res.get("trans")), _ptr(res.get("rot")), int(acc), c.space,
                                               c.stream))
        else:
            check(L.smplpp_skeleton_vjp(self.handle, n, _ptr(beta), _ptr(pose), _ptr(gw), _ptr(gp), _ptr(gj), _ptr(res.get("beta")),
                                        _ptr(res.get("theta")), int(acc), c.space, c.stream))
        return res

    def skeleton(self, beta, theta, want=("world", "posed", "joints"), out=None):
        """The kinematic chain alone, without a vertex (smplpp_skeleton): beta [N,10] (None = zero), theta [N,25,3] as in launch.
        Returns a dict of world [N,24,3,4] (row-major [A_j | posed_j]: the world orientation and position of every joint), posed
        [N,24,3] (the posed joints, what smplx calls joints) and joints [N,24,3] (the REST joints launch returns).  world[..., :3]
        and joints have the bits of launch's xforms[:, :, :3, :3] and joints.  One kernel launch; nothing in the model's workspace is
        touched and nothing is kept for the getters.  `want` drops outputs; `out` (a dict keyed the same way) supplies preallocated
        arrays.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("skeleton", theta, beta)
        return self._skeleton(c, beta, None, theta, False, want, out)[3]

    def skeletonBackward(self, beta, theta, grad_world=None, grad_posed=None, grad_joints=None, want=("beta", "theta"), out=None):
        """Vector-Jacobian product of `skeleton` (smplpp_skeleton_vjp): {"beta": dL/dbeta [N,10], "theta": dL/dtheta [N,25,3]} for the
        cotangents grad_world [N,24,3,4], grad_posed [N,24,3] and grad_joints [N,24,3] (None = zero; at least one).  `want` drops
        one; with `out` (a dict keyed the same way) the gradients are ADDED into its arrays, so the arrays launchBackward filled then
        hold the gradient of a loss on vertices and skeleton."""
        return self._skeleton_backward("skeletonBackward", beta, None, theta, False, grad_world, grad_posed, grad_joints, want, out)

    def skeletonRotmat(self, beta, trans, rot, want=("world", "posed", "joints"), out=None):
        """`skeleton` from rotation matrices (smplpp_skeleton_rotmat): beta [N,10] (None = zero), trans [N,3] (None = zero), rot
        [N,24,3,3] used as given, as launchRotmat uses them."""
        c = _Call("skeletonRotmat", rot, beta, trans)
        return self._skeleton(c, beta, trans, rot, True, want, out)[3]

    def skeletonRotmatBackward(self, beta, trans, rot, grad_world=None, grad_posed=None, grad_joints=None, want=("beta", "trans", "rot"),
                               out=None):
        """Vector-Jacobian product of `skeletonRotmat` (smplpp_skeleton_rotmat_vjp): {"beta": [N,10], "trans": [N,3], "rot": [N,24,3,3]},
        "rot" as nine independent entries per joint (the convention of launchRotmatBackward).  Cotangents, `want` and `out` as in
        skeletonBackward."""
        return self._skeleton_backward("skeletonRotmatBackward", beta, trans, rot, True, grad_world, grad_posed, grad_joints, want, out)

    def skeleton_differentiable(self, beta, theta):
        """(world [N,24,3,4], posed [N,24,3], joints [N,24,3]) for device tensors beta [N,10], theta [N,25,3], differentiable with
        torch.autograd in both: one smplpp_skeleton forward, one smplpp_skeleton_vjp backward, on torch's current stream.  First
        derivatives only.  The outputs feed project_points_differentiable, align, Landmarks (as its `joints`) and the sequence terms."""
        if torch is None:
            raise SmplppError(1, "skeleton_differentiable needs torch")
        return _SkeletonFunction.apply(beta, theta, self)

    def skeleton_rotmat_differentiable(self, beta, trans, rot):
        """skeleton_differentiable from rotation matrices: differentiable in beta [N,10], trans [N,3] and rot [N,24,3,3] (nine
        independent entries per joint): smplpp_skeleton_rotmat forward, smplpp_skeleton_rotmat_vjp backward."""
        if torch is None:
            raise SmplppError(1, "skeleton_rotmat_differentiable needs torch")
        return _SkeletonRotmatFunction.apply(beta, trans, rot, self)

    def launchStatus(self):
        """Status word of the launches since the last read (synchronises the current stream): bit 0 = an operand left the
        input range of the default fused kernel (include/smplpp_hip.h, smplpp_fk_status).  Host-space launches raise instead."""
        bits = C.c_int(0)
        check(_lib.load().smplpp_fk_status(self.handle, C.byref(bits), _stream()))
        return bits.value

    def _need(self, key):
        if self._out.get(key) is None:
            raise SmplppError(4, "Failed to get vertices of new pose!")  # src/LinearBlendSkinning.cpp:413
        return self._out[key]

    # ---- getters (SMPL.h:248-262)
    def getVertex(self):
        v = self._need("verts")
        return v.clone() if _is_torch(v) else v.copy()  # :492-506 returns a clone

    def getRestShape(self):
        v = self._need("rest")
        return v.clone() if _is_torch(v) else v.copy()

    def getRestJoint(self):
        v = self._need("joints")
        return v.clone() if _is_torch(v) else v.copy()

    def getTransformation(self):
        v = self._need("xforms")
        return v.clone() if _is_torch(v) else v.copy()

    def getFaceIndex(self):
        return self._model["face_indices"].copy()  # [F,3] int32, 1-based (src/SMPL.cpp:418-433)

    def getFaceIndexRaw(self, idx):
        return self._model["face_indices"][idx]  # :435-438

    def getVertexRaw(self, idx):
        return self._need("verts")[0, idx]  # batch 0 only (src/LinearBlendSkinning.cpp:419-427)

    def getAdjacentFaces(self, idx):
        """{face id: weight} like the reference's unordered_map (src/SMPL.cpp:537-540)."""
        L, cap, cnt = _lib.load(), 64, C.c_int64()
        while True:  # a vertex of more than 64 faces: ask again with the reported count (as include/smplpp/SMPL.h does)
            faces, w = (C.c_int64 * cap)(), (C.c_float * cap)()
            check(L.smplpp_adjacent_faces(self.handle, int(idx), cap, faces, w, C.byref(cnt)))
            if cnt.value <= cap:
                return {int(faces[i]): float(w[i]) for i in range(cnt.value)}
            cap = cnt.value

    def _normals(self, ids, vertex, frame=None):
        verts = self._need("verts")
        v = verts if frame is None else verts[frame:frame + 1]
        c = _Call("calcVertexNormal" if vertex else "calcNormal", v)
        out, _ = self._normals_at(c, c.input(v, (len(v), self.vertex_num, 3)), 1 if vertex else 0, ids)
        if frame is not None:
            out = out[0]
            return out[0] if np.isscalar(ids) else out
        return out

    def _normals_at(self, c, verts, kind, ids):
        """The normal queries at `verts` [N,V,3] in the space of `c`: kind 0 = face list, 1 = vertex list, 2 = whole mesh.
        Returns (normals, ids as passed to the call)."""
        L = _lib.load()
        n = len(verts)
        if kind == 2:
            out = c.empty((n, self.vertex_num, 3))
            check(L.smplpp_mesh_vertex_normals(self.handle, n, _ptr(verts), _ptr(out), c.space, c.stream))
            return out, None
        idt = c.ids(ids)
        out = c.empty((n, len(idt), 3))
        fn = L.smplpp_vertex_normals if kind == 1 else L.smplpp_face_normals
        check(fn(self.handle, n, _ptr(verts), len(idt), _ptr(idt), _ptr(out), c.space, c.stream))
        return out, idt

    def calcNormal(self, faceIdx):
        """SMPL::calcNormal (src/SMPL.cpp:518-525): batch 0, like the reference."""
        return self._normals(faceIdx, False, frame=0)

    def calcVertexNormal(self, idx):
        """SMPL::calcVertexNormal (src/SMPL.cpp:527-535): batch 0."""
        return self._normals(idx, True, frame=0)

    def calcNormalBatch(self, faceIds):
        return self._normals(faceIds, False)

    def calcVertexNormalBatch(self, vertexIds):
        return self._normals(vertexIds, True)

    def calcMeshVertexNormals(self):
        """SMPL::calcVertexNormal (src/SMPL.cpp:527-535) for every vertex of every frame of the last launch: [N,V,3]."""
        verts = self._need("verts")
        c = _Call("calcMeshVertexNormals", verts)
        return self._normals_at(c, c.input(verts, (len(verts), self.vertex_num, 3)), 2, None)[0]

    # ---- backward of the normal queries (smplpp_face_normals_vjp / smplpp_vertex_normals_vjp / smplpp_mesh_vertex_normals_vjp)
    def _normals_vjp(self, kind, verts, ids, grad_normals, out):
        """kind 0 = face list, 1 = vertex list, 2 = whole mesh.  Returns grad_verts [N,V,3]; `out` given = accumulate into it."""
        c = _Call(("calcNormalBackward", "calcVertexNormalBackward", "calcMeshVertexNormalsBackward")[kind], verts, grad_normals, out)
        n, V = len(verts), self.vertex_num
        idt = None if kind == 2 else c.ids(ids)
        count = V if kind == 2 else len(idt)
        verts, gn = c.input(verts, (n, V, 3)), c.input(grad_normals, (n, count, 3))
        acc = out is not None
        out = c.inout(out, (n, V, 3)) if acc else c.empty((n, V, 3))
        L = _lib.load()
        if kind == 2:
            check(L.smplpp_mesh_vertex_normals_vjp(self.handle, n, _ptr(verts), _ptr(gn), _ptr(out), int(acc), c.space, c.stream))
        else:
            fn = L.smplpp_vertex_normals_vjp if kind == 1 else L.smplpp_face_normals_vjp
            check(fn(self.handle, n, _ptr(verts), count, _ptr(idt), _ptr(gn), _ptr(out), int(acc), c.space, c.stream))
        return out

    def calcNormalBackward(self, verts, face_ids, grad_normals, out=None):
        """Vector-Jacobian product of calcNormalBatch at `verts` [N,V,3]: dL/dverts for dL/dnormals = grad_normals [N,count,3]
        (smplpp_face_normals_vjp).  numpy (the call synchronises) or float32 device tensors (torch's current stream).  `out`
        [N,V,3] given: the product is added into it (and returned)."""
        return self._normals_vjp(0, verts, face_ids, grad_normals, out)

    def calcVertexNormalBackward(self, verts, vertex_ids, grad_normals, out=None):
        """Vector-Jacobian product of calcVertexNormalBatch at `verts` (smplpp_vertex_normals_vjp); as calcNormalBackward."""
        return self._normals_vjp(1, verts, vertex_ids, grad_normals, out)

    def calcMeshVertexNormalsBackward(self, verts, grad_normals, out=None):
        """Vector-Jacobian product of calcMeshVertexNormals at `verts` for grad_normals [N,V,3] (smplpp_mesh_vertex_normals_vjp)."""
        return self._normals_vjp(2, verts, None, grad_normals, out)

    def face_normals_differentiable(self, verts, face_ids):
        """Unit face normals [N,count,3] of device vertices verts [N,V,3] (the bits of calcNormalBatch), differentiable in verts with
        torch.autograd: smplpp_face_normals forward, smplpp_face_normals_vjp backward, on torch's current stream."""
        if torch is None:
            raise SmplppError(1, "face_normals_differentiable needs torch")
        return _NormalsFunction.apply(verts, self, 0, face_ids)

    def vertex_normals_differentiable(self, verts, vertex_ids=None):
        """Vertex normals [N,count,3] (vertex_ids given; the bits of calcVertexNormalBatch) or [N,V,3] (None: the whole mesh, the
        bits of calcMeshVertexNormals) of device vertices verts [N,V,3], differentiable in verts with torch.autograd."""
        if torch is None:
            raise SmplppError(1, "vertex_normals_differentiable needs torch")
        return _NormalsFunction.apply(verts, self, 2 if vertex_ids is None else 1, vertex_ids)

    def calcSweepGrid(self, frame=0):
        """The sweep grid of node/node.cpp:1023-1073 for one frame of the last launch: dict(grid_min [3], grid_num [3],
        winding [cells], inside [cells] bool, grid_idx [cells,3] int32 in the reference's cell order, positions = 0.025 *
        grid_idx). `inside` marks the cells the reference enters into g_sweepGridList (winding number > 0.5)."""
        verts = self._need("verts")
        c = _Call("calcSweepGrid", verts)
        v = c.input(verts[frame], (self.vertex_num, 3))
        L = _lib.load()
        gmin = np.zeros(3, np.int32)
        gnum = np.zeros(3, np.int32)
        cells = C.c_int64(0)
        check(L.smplpp_sweep_grid(self.handle, _ptr(v), _ptr(gmin), _ptr(gnum), 0, None, None, C.byref(cells), c.space, c.stream))
        n = int(cells.value)
        w, ins = c.empty(n), c.empty(n, "uint8")
        check(L.smplpp_sweep_grid(self.handle, _ptr(v), _ptr(gmin), _ptr(gnum), n, _ptr(w), _ptr(ins), C.byref(cells), c.space, c.stream))
        if c.dev:
            torch.cuda.synchronize()
            w, ins = w.cpu().numpy(), ins.cpu().numpy()
        ix, iy, iz = np.meshgrid(*[np.arange(gmin[a], gmin[a] + gnum[a], dtype=np.int32) for a in range(3)], indexing="ij")
        gidx = np.stack([ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)], axis=1)
        return dict(grid_min=gmin, grid_num=gnum, winding=w, inside=ins.astype(bool), grid_idx=gidx)

    def closestPoints(self, points):
        """igl::point_mesh_squared_distance as used at node/node.cpp:982 — points [N,K,3] vs each frame's mesh."""
        verts = self._need("verts")
        c = _Call("closestPoints", verts, points)
        n = len(verts)
        points = points if c.dev else _np32(points).reshape(n, -1, 3)
        K = points.shape[1]
        verts, points = c.input(verts, (n, self.vertex_num, 3)), c.input(points, (n, K, 3))
        face, closest, sq = c.empty((n, K), "int64"), c.empty((n, K, 3)), c.empty((n, K))
        check(_lib.load().smplpp_closest_points(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(face), _ptr(closest), _ptr(sq),
                                                c.space, c.stream))
        return face, closest, sq

    # ---- point-to-mesh distance (smplpp_point_mesh_distance / smplpp_point_mesh_distance_vjp)
    def _pmd_inputs(self, c, verts, points):
        """verts [N,V,3] and points [N,K,3] checked in the space of `c`; returns (verts, points, K)."""
        n = len(verts)
        shape = tuple(points.shape) if c.dev else np.shape(points)
        if len(shape) != 3 or shape[0] != n or shape[1] < 1 or shape[2] != 3:
            c.refuse("expected points of shape (%d, K, 3), got %s" % (n, shape))
        K = int(shape[1])
        return c.input(verts, (n, self.vertex_num, 3)), c.input(points, (n, K, 3)), K

    def _pmd(self, c, verts, points, K, want_closest=True):
        n = len(verts)
        face, w, sq = c.empty((n, K), "int64"), c.empty((n, K, 3)), c.empty((n, K))
        closest = c.empty((n, K, 3)) if want_closest else None
        check(_lib.load().smplpp_point_mesh_distance(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(face), _ptr(w), _ptr(closest), _ptr(sq),
                                                     c.space, c.stream))
        return face, w, closest, sq

    def _distance_vjp(self, mesh_to_point, c, verts, points, K, ids, grad_sqdist, out, grad_points, want_verts=True, want_points=True,
                      inside=None):
        """smplpp_point_mesh_distance_vjp (ids = the forward's face [N,K]), with `inside` [N,K] smplpp_point_mesh_signed_distance_vjp,
        or, mesh_to_point, smplpp_mesh_point_distance_vjp (ids = the forward's index [N,V]); grad_sqdist has the shape of ids."""
        n, V = len(verts), self.vertex_num
        name, rows = ("index", V) if mesh_to_point else ("face", K)
        idt = c.ids(ids)
        if idt.shape[0] != n * rows:
            c.refuse("expected %s of shape (%d, %d)" % (name, n, rows))
        g = c.input(grad_sqdist, (n, rows))
        acc = out is not None or grad_points is not None

        def buf(a, shape, want):
            if a is not None:
                return c.inout(a, shape)
            if not want:
                return None
            if not acc:
                return c.empty(shape)
            return torch.zeros(shape, dtype=torch.float32, device=c.device) if c.dev else np.zeros(shape, np.float32)

        gv, gp = buf(out, (n, V, 3), want_verts), buf(grad_points, (n, K, 3), want_points)
        L = _lib.load()
        if inside is not None:
            ins = c.flags(inside)
            if ins.shape[0] != n * rows:
                c.refuse("expected inside of shape (%d, %d)" % (n, rows))
            check(L.smplpp_point_mesh_signed_distance_vjp(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(idt), _ptr(ins), _ptr(g), _ptr(gv),
                                                          _ptr(gp), int(acc), c.space, c.stream))
            return gv, gp
        vjp = L.smplpp_mesh_point_distance_vjp if mesh_to_point else L.smplpp_point_mesh_distance_vjp
        check(vjp(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(idt), _ptr(g), _ptr(gv), _ptr(gp), int(acc), c.space, c.stream))
        return gv, gp

    def pointMeshDistance(self, verts, points):
        """The closest face of each frame's mesh verts [N,V,3] to each of K points [N,K,3] (smplpp_point_mesh_distance): returns
        (face [N,K] int64, weights [N,K,3], closest [N,K,3], sqdist [N,K]).  face / closest / sqdist have the bits of closestPoints;
        weights are the closest point's vertex weights (sum_j weights[..., j] * verts[face[..., j]] = closest up to rounding).
        numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("pointMeshDistance", verts, points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        return self._pmd(c, verts, points, K)

    def pointMeshDistanceBackward(self, verts, points, face, grad_sqdist, out=None, grad_points=None):
        """Vector-Jacobian product of pointMeshDistance's sqdist at the faces `face` [N,K] it chose: (grad_verts [N,V,3],
        grad_points [N,K,3]) for dL/dsqdist = grad_sqdist [N,K] (smplpp_point_mesh_distance_vjp).  `out` [N,V,3] and / or
        `grad_points` [N,K,3] given: the product is added into them (and they are returned); an array not given is then
        returned holding the product alone."""
        c = _Call("pointMeshDistanceBackward", verts, points, grad_sqdist, out, grad_points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        return self._distance_vjp(False, c, verts, points, K, face, grad_sqdist, out, grad_points)

    def point_mesh_distance_differentiable(self, verts, points):
        """(face [N,K], weights [N,K,3], sqdist [N,K]) of device points [N,K,3] against device vertices verts [N,V,3] (the bits of
        pointMeshDistance), with sqdist differentiable in both verts and points through torch.autograd: smplpp_point_mesh_distance
        forward, smplpp_point_mesh_distance_vjp backward, on torch's current stream.  face and weights are not differentiable.
        For a fixed-correspondence or point-to-plane (ICP-style) term, pass face and weights to ik.task_surface_differentiable,
        which gives the position and normal of those surface points differentiably."""
        if torch is None:
            raise SmplppError(1, "point_mesh_distance_differentiable needs torch")
        return _PointDistanceFunction.apply(verts, points, self)

    # ---- mesh-to-point distance (smplpp_mesh_point_distance / smplpp_mesh_point_distance_vjp)
    def _mpd(self, c, verts, points, K):
        n, V = len(verts), self.vertex_num
        index, sq = c.empty((n, V), "int64"), c.empty((n, V))
        check(_lib.load().smplpp_mesh_point_distance(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(index), _ptr(sq), c.space, c.stream))
        return index, sq

    def meshPointDistance(self, verts, points):
        """The nearest of K points [N,K,3] to each vertex of each frame's mesh verts [N,V,3] (smplpp_mesh_point_distance): returns
        (index [N,V] int64, sqdist [N,V]).  sqdist is the fp32 ((dx*dx + dy*dy) + dz*dz) of d = v - p without FMA; the lowest
        index wins ties; non-finite distances are never chosen, and a vertex with no eligible point gets (-1, 0).  The other
        direction of pointMeshDistance.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("meshPointDistance", verts, points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        return self._mpd(c, verts, points, K)

    def meshPointDistanceBackward(self, verts, points, index, grad_sqdist, out=None, grad_points=None):
        """Vector-Jacobian product of meshPointDistance's sqdist at the points `index` [N,V] it chose: (grad_verts [N,V,3],
        grad_points [N,K,3]) for dL/dsqdist = grad_sqdist [N,V] (smplpp_mesh_point_distance_vjp).  `out` [N,V,3] and / or
        `grad_points` [N,K,3] given: the product is added into them (and they are returned); an array not given is then
        returned holding the product alone.  A zero cotangent masks a vertex out."""
        c = _Call("meshPointDistanceBackward", verts, points, grad_sqdist, out, grad_points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        return self._distance_vjp(True, c, verts, points, K, index, grad_sqdist, out, grad_points)

    def mesh_point_distance_differentiable(self, verts, points):
        """(index [N,V], sqdist [N,V]) of device vertices verts [N,V,3] against device points [N,K,3] (the bits of
        meshPointDistance), with sqdist differentiable in both verts and points through torch.autograd: smplpp_mesh_point_distance
        forward, smplpp_mesh_point_distance_vjp backward, on torch's current stream.  index is not differentiable.  With
        point_mesh_distance_differentiable, the two halves of a two-sided (Chamfer) scan registration loss."""
        if torch is None:
            raise SmplppError(1, "mesh_point_distance_differentiable needs torch")
        return _MeshPointDistanceFunction.apply(verts, points, self)

    # ---- normal-compatible, distance-capped correspondences (smplpp_point_mesh_distance_compatible / smplpp_mesh_point_distance_compatible)
    @staticmethod
    def _compat_cap(max_dist, max_sqdist):
        """The squared cap as the fp32 value the call receives: max_sqdist as given, else fp32(max_dist)^2, else +inf."""
        if max_sqdist is not None:
            return float(np.float32(max_sqdist))
        if max_dist is None:
            return float("inf")
        return float(np.float32(max_dist) * np.float32(max_dist))

    def _pmdc(self, c, verts, points, normals, K, cos_min, cap, want_closest=True):
        n = len(verts)
        normals = c.input(normals, (n, K, 3))
        face, w, sq = c.empty((n, K), "int64"), c.empty((n, K, 3)), c.empty((n, K))
        closest = c.empty((n, K, 3)) if want_closest else None
        check(_lib.load().smplpp_point_mesh_distance_compatible(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(normals), float(cos_min), cap,
                                                                _ptr(face), _ptr(w), _ptr(closest), _ptr(sq), c.space, c.stream))
        return face, w, closest, sq

    def _mpdc(self, c, verts, points, point_normals, vert_normals, K, cos_min, cap):
        n, V = len(verts), self.vertex_num
        pn = c.input(point_normals, (n, K, 3))
        vn = c.input(vert_normals, (n, V, 3))
        if pn is not None and vn is None:
            vn = self._normals_at(c, verts, 2, None)[0]
        index, sq = c.empty((n, V), "int64"), c.empty((n, V))
        check(_lib.load().smplpp_mesh_point_distance_compatible(self.handle, n, _ptr(verts), _ptr(vn), K, _ptr(points), _ptr(pn), float(cos_min),
                                                                cap, _ptr(index), _ptr(sq), c.space, c.stream))
        return index, sq

    def pointMeshDistanceCompatible(self, verts, points, point_normals, cos_min=0.5, max_dist=None, max_sqdist=None):
        """pointMeshDistance restricted, inside the search, to the faces whose normal is compatible with the query's and that lie
        within max_dist (smplpp_point_mesh_distance_compatible, which states the exact rule): returns (face [N,K] int64, weights
        [N,K,3], closest [N,K,3], sqdist [N,K], matched [N,K] bool).  point_normals [N,K,3] need not be unit (None: no normal test);
        a face passes when the angle between its normal and the query's is at most acos(cos_min).  max_dist in metres (None: no
        cap); max_sqdist gives the squared cap directly.  An unmatched query (no candidate, or a non-finite row) has face -1, zeros
        elsewhere and matched False.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("pointMeshDistanceCompatible", verts, points, point_normals)
        verts, points, K = self._pmd_inputs(c, verts, points)
        face, w, closest, sq = self._pmdc(c, verts, points, point_normals, K, cos_min, self._compat_cap(max_dist, max_sqdist))
        return face, w, closest, sq, face >= 0

    def pointMeshDistanceCompatibleBackward(self, verts, points, face, grad_sqdist, out=None, grad_points=None):
        """pointMeshDistanceBackward at the faces pointMeshDistanceCompatible chose: unmatched queries (face -1) contribute
        nothing.  (In host space smplpp_point_mesh_distance_vjp refuses -1, so they are passed as face 0 with a zero cotangent.)"""
        c = _Call("pointMeshDistanceCompatibleBackward", verts, points, grad_sqdist, out, grad_points)
        if not c.dev:
            face = np.asarray(face, np.int64)
            grad_sqdist = np.where(face < 0, np.float32(0), _np32(grad_sqdist).reshape(face.shape))
            face = np.where(face < 0, 0, face)
        return self.pointMeshDistanceBackward(verts, points, face, grad_sqdist, out, grad_points)

    def point_mesh_distance_compatible_differentiable(self, verts, points, point_normals, cos_min=0.5, max_dist=None, max_sqdist=None):
        """(face [N,K], weights [N,K,3], matched [N,K] bool, sqdist [N,K]) of device points [N,K,3] with normals point_normals
        against device vertices verts [N,V,3] (the bits of pointMeshDistanceCompatible), with sqdist differentiable in verts and
        points through torch.autograd: smplpp_point_mesh_distance_compatible forward, smplpp_point_mesh_distance_vjp backward.  The
        normals steer the selection only: nothing flows to them, and an unmatched query has sqdist 0 and no gradient."""
        if torch is None:
            raise SmplppError(1, "point_mesh_distance_compatible_differentiable needs torch")
        return _PointDistanceCompatibleFunction.apply(verts, points, self, point_normals, cos_min, self._compat_cap(max_dist, max_sqdist))

    def meshPointDistanceCompatible(self, verts, points, point_normals, vert_normals=None, cos_min=0.5, max_dist=None, max_sqdist=None):
        """meshPointDistance restricted, inside the search, to the points whose normal is compatible with the vertex's and that lie
        within max_dist (smplpp_mesh_point_distance_compatible): returns (index [N,V] int64, sqdist [N,V], matched [N,V] bool).
        vert_normals [N,V,3] None: the whole-mesh vertex normals of verts (smplpp_mesh_vertex_normals).  point_normals None: no
        normal test.  A vertex without an eligible point has (-1, 0, False)."""
        c = _Call("meshPointDistanceCompatible", verts, points, point_normals, vert_normals)
        verts, points, K = self._pmd_inputs(c, verts, points)
        index, sq = self._mpdc(c, verts, points, point_normals, vert_normals, K, cos_min, self._compat_cap(max_dist, max_sqdist))
        return index, sq, index >= 0

    def mesh_point_distance_compatible_differentiable(self, verts, points, point_normals, vert_normals=None, cos_min=0.5, max_dist=None,
                                                      max_sqdist=None):
        """(index [N,V], matched [N,V] bool, sqdist [N,V]) of device vertices against device points with normals (the bits of
        meshPointDistanceCompatible), with sqdist differentiable in verts and points through torch.autograd:
        smplpp_mesh_point_distance_compatible forward, smplpp_mesh_point_distance_vjp backward.  The normals (vert_normals None: the
        whole-mesh normals of verts) steer the selection only: nothing flows to them or through them."""
        if torch is None:
            raise SmplppError(1, "mesh_point_distance_compatible_differentiable needs torch")
        return _MeshPointDistanceCompatibleFunction.apply(verts, points, self, point_normals, vert_normals, cos_min,
                                                          self._compat_cap(max_dist, max_sqdist))

    # ---- surface geodesics (smplpp_mesh_geodesic); the self-contact search built on them is smplpp_amd.contact
    def meshGeodesic(self, verts, sources, max_dist=None):
        """Distance along the mesh's edges from S source sets to every vertex of each frame of verts [N,V,3] (smplpp_mesh_geodesic):
        dist [N,S,V].  `sources` is a list of S lists of vertex indices (a set may be empty: its field is +inf), or a 1-D array of S
        single sources; the frames share them.  dist is the exact fp32 minimum over edge paths of the left-to-right sum of the edge
        lengths: +inf where no path leads, and where dist > max_dist (None: no cap).  A graph distance, an upper bound of the
        surface's.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("meshGeodesic", verts)
        if len(verts.shape) != 3 or verts.shape[0] < 1:
            c.refuse("expected verts of shape (N, V, 3)")
        n, V = int(verts.shape[0]), self.vertex_num
        verts = c.input(verts, (n, V, 3))
        if _is_torch(sources):
            sources = sources.detach().cpu().numpy()
        if isinstance(sources, np.ndarray) and sources.ndim == 1:
            sets = [[int(s)] for s in sources]
        else:
            sets = [np.asarray(s, np.int64).reshape(-1).tolist() for s in sources]
        if not sets:
            c.refuse("at least one source set is needed")
        ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
        ids = np.asarray([v for s in sets for v in s] + [0], np.int64)  # (one spare entry: never an empty array)
        if ids[:-1].size and (ids[:-1].min() < 0 or ids[:-1].max() >= V):
            c.refuse("a source vertex is outside [0, V)")
        S = len(sets)
        if c.dev:
            ptr, ids = torch.from_numpy(ptr).to(c.device), torch.from_numpy(ids).to(c.device)
        dist = c.empty((n, S, V))
        cap = float("inf") if max_dist is None else float(np.float32(max_dist))
        check(_lib.load().smplpp_mesh_geodesic(self.handle, n, _ptr(verts), S, _ptr(ptr), _ptr(ids), cap, _ptr(dist), c.space, c.stream))
        return dist

    # ---- winding numbers and the signed point-to-mesh distance (smplpp_point_mesh_winding / smplpp_point_mesh_signed_distance[_vjp])
    def pointMeshWinding(self, verts, points):
        """Generalized winding numbers of each frame's mesh verts [N,V,3] at K points [N,K,3] (smplpp_point_mesh_winding): returns
        (winding [N,K], inside [N,K] bool).  winding has the bits calcSweepGrid gives at a cell of the same fp32 position; inside =
        winding > 0.5 (~1 inside the closed body, ~0 outside, ~2 where the posed mesh overlaps itself).  A NaN point gives NaN and
        False.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("pointMeshWinding", verts, points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        n = len(verts)
        w, ins = c.empty((n, K)), c.empty((n, K), "uint8")
        check(_lib.load().smplpp_point_mesh_winding(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(w), _ptr(ins), c.space, c.stream))
        return w, ins.bool() if c.dev else ins.astype(bool)

    def _psd(self, c, verts, points, K, want_closest=True, want_winding=True):
        n = len(verts)
        face, w, sq, ins = c.empty((n, K), "int64"), c.empty((n, K, 3)), c.empty((n, K)), c.empty((n, K), "uint8")
        closest = c.empty((n, K, 3)) if want_closest else None
        wn = c.empty((n, K)) if want_winding else None
        check(_lib.load().smplpp_point_mesh_signed_distance(self.handle, n, _ptr(verts), K, _ptr(points), _ptr(face), _ptr(w), _ptr(closest),
                                                            _ptr(wn), _ptr(ins), _ptr(sq), c.space, c.stream))
        return face, w, closest, wn, ins, sq

    def pointMeshSignedDistance(self, verts, points):
        """pointMeshDistance and pointMeshWinding in one call (smplpp_point_mesh_signed_distance): returns (face [N,K] int64,
        weights [N,K,3], closest [N,K,3], winding [N,K], inside [N,K] bool, signed_sqdist [N,K]) with signed_sqdist = -sqdist where
        inside, else sqdist (squared on purpose: continuous and C1 across the surface).  The other outputs have the bits of the two
        calls.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("pointMeshSignedDistance", verts, points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        face, w, closest, wn, ins, sq = self._psd(c, verts, points, K)
        return face, w, closest, wn, ins.bool() if c.dev else ins.astype(bool), sq

    def pointMeshSignedDistanceBackward(self, verts, points, face, inside, grad, out=None, grad_points=None):
        """Vector-Jacobian product of pointMeshSignedDistance's signed_sqdist at the faces `face` [N,K] and flags `inside` [N,K] it
        gave: (grad_verts [N,V,3], grad_points [N,K,3]) for dL/dsigned_sqdist = grad [N,K] (smplpp_point_mesh_signed_distance_vjp):
        the bits of pointMeshDistanceBackward at grad * (inside ? -1 : 1).  `out` and / or `grad_points` as in
        pointMeshDistanceBackward."""
        c = _Call("pointMeshSignedDistanceBackward", verts, points, grad, out, grad_points)
        verts, points, K = self._pmd_inputs(c, verts, points)
        return self._distance_vjp(False, c, verts, points, K, face, grad, out, grad_points, inside=inside)

    def point_mesh_signed_distance_differentiable(self, verts, points):
        """(face [N,K], weights [N,K,3], inside [N,K] bool, signed_sqdist [N,K]) of device points [N,K,3] against device vertices
        verts [N,V,3] (the bits of pointMeshSignedDistance), with signed_sqdist differentiable in both verts and points through
        torch.autograd: smplpp_point_mesh_signed_distance forward, smplpp_point_mesh_signed_distance_vjp backward, on torch's current
        stream.  A penetration term is e.g. relu(-signed_sqdist).sum()."""
        if torch is None:
            raise SmplppError(1, "point_mesh_signed_distance_differentiable needs torch")
        return _SignedDistanceFunction.apply(verts, points, self)

    # ---- ray casting (smplpp_ray_cast / smplpp_ray_cast_vjp)
    def _ray_inputs(self, c, verts, origin, dir):
        """verts [N,V,3] and the rays ([K,3] or [1,K,3]: one set for every frame; [N,K,3]: one per frame) checked in the space of `c`;
        returns (n, frames of the rays, K, verts, origin, dir)."""
        n = len(verts)
        if not c.dev:
            origin, dir = _np32(origin), _np32(dir)
        if len(origin.shape) == 2:
            origin = origin.reshape((1,) + tuple(origin.shape))
        if len(dir.shape) == 2:
            dir = dir.reshape((1,) + tuple(dir.shape))
        shape = tuple(origin.shape)
        if len(shape) != 3 or shape[0] not in (1, n) or shape[1] < 1 or shape[2] != 3 or tuple(dir.shape) != shape:
            c.refuse("expected origin and dir of one shape (K, 3), (1, K, 3) or (%d, K, 3), got %s and %s" % (n, shape, tuple(dir.shape)))
        rf, K = int(shape[0]), int(shape[1])
        return n, rf, K, c.input(verts, (n, self.vertex_num, 3)), c.input(origin, (rf, K, 3)), c.input(dir, (rf, K, 3))

    def _ray_cast(self, c, n, rf, K, verts, origin, dir, t_min, t_max, facing, want):
        face, t = c.empty((n, K), "int64"), c.empty((n, K))
        bary = c.empty((n, K, 3)) if "bary" in want else None
        hits = c.empty((n, K, 2), "int32") if "hits" in want else None
        check(_lib.load().smplpp_ray_cast(self.handle, n, _ptr(verts), rf, K, _ptr(origin), _ptr(dir), float(t_min), float(t_max), int(facing),
                                          _ptr(face), _ptr(t), _ptr(bary), _ptr(hits), c.space, c.stream))
        return face, t, bary, hits

    def rayCast(self, verts, origin, dir, t_min=0.0, t_max=float("inf"), facing=3, want=("bary", "hits")):
        """Where each ray origin + t dir first meets each frame's mesh verts [N,V,3] (smplpp_ray_cast).  origin and dir are [K,3] or
        [1,K,3] (one set of rays cast against every frame) or [N,K,3]; dir is used as given, so t is in units of |dir|.  Returns a dict
        of face [N,K] int64 (-1: no hit), t [N,K] (0 without a hit), bary [N,K,3] (of the face's corners at the hit), hits [N,K,2]
        int32 (front and back faces met in (t_min, t_max]) and hit [N,K] bool = face >= 0.  facing = 1 keeps the faces the ray meets
        against their normal (front), 2 the others (back), 3 both; only t_min < t <= t_max counts.  The hit point is
        origin + t[..., None] * dir.  A ray with a coordinate that is not finite, or a zero dir, hits nothing.  `want` drops bary or hits.
        numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        c = _Call("rayCast", verts, origin, dir)
        n, rf, K, verts, origin, dir = self._ray_inputs(c, verts, origin, dir)
        face, t, bary, hits = self._ray_cast(c, n, rf, K, verts, origin, dir, t_min, t_max, facing, want)
        out = dict(face=face, t=t, hit=face >= 0)
        if bary is not None:
            out["bary"] = bary
        if hits is not None:
            out["hits"] = hits
        return out

    def rayCastBackward(self, verts, origin, dir, face, grad_t, want=("verts", "origin", "dir"), out=None):
        """Vector-Jacobian product of rayCast's t at the faces `face` [N,K] it gave, held fixed (smplpp_ray_cast_vjp): a dict of "verts"
        [N,V,3], "origin" and "dir" (the rays' shape as cast: [1,K,3] for shared rays, the frames' sum) for dL/dt = grad_t [N,K].  A ray
        without a hit contributes nothing.  `want` drops outputs; with `out` (a dict keyed the same way) the gradients are ADDED into
        its arrays."""
        acc = out is not None
        c = _Call("rayCastBackward", verts, origin, dir, grad_t, *(out.values() if acc else ()))
        n, rf, K, verts, origin, dir = self._ray_inputs(c, verts, origin, dir)
        ids = c.ids(face)
        if ids.shape[0] != n * K:
            c.refuse("expected face ids of shape %s" % ((n, K),))
        g = c.input(grad_t, (n, K))
        shapes = {"verts": (n, self.vertex_num, 3), "origin": (rf, K, 3), "dir": (rf, K, 3)}
        keys = [k for k in shapes if k in (out if acc else want)]
        if not keys:
            c.refuse("verts, origin or dir must be asked for")
        res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
        check(_lib.load().smplpp_ray_cast_vjp(self.handle, n, _ptr(verts), rf, K, _ptr(origin), _ptr(dir), _ptr(ids), _ptr(g), _ptr(res.get("verts")),
                                              _ptr(res.get("origin")), _ptr(res.get("dir")), int(acc), c.space, c.stream))
        return res

    def ray_cast_differentiable(self, verts, origin, dir, t_min=0.0, t_max=float("inf"), facing=3):
        """rayCast's dict for device tensors (the same bits), with t differentiable in verts, origin and dir through torch.autograd:
        smplpp_ray_cast forward, smplpp_ray_cast_vjp backward at the faces hit, on torch's current stream.  face, bary, hits and hit
        are constants; a hit point with a gradient is origin + t[..., None] * dir.  A range term is e.g. ((t - measured)[hit] ** 2).sum()."""
        if torch is None:
            raise SmplppError(1, "ray_cast_differentiable needs torch")
        face, t, bary, hits, hit = _RayCastFunction.apply(verts, origin, dir, self, float(t_min), float(t_max), int(facing))
        return dict(face=face, t=t, bary=bary, hits=hits, hit=hit)

    # ---- self-intersections and the self-penetration energy (smplpp_self_intersections / smplpp_self_penetration[_vjp])
    def _sp_forward(self, name, verts, max_pairs, sigma, check_count, energy, device_only=False):
        c = _Call(name, verts, device_only=device_only)
        n = verts.shape[0] if c.dev else len(verts)
        verts = c.input(verts, (n, self.vertex_num, 3))
        max_pairs = SELF_PAIRS_DEFAULT if max_pairs is None else int(max_pairs)
        if max_pairs < 0:
            c.refuse("max_pairs must be >= 0")
        pairs, count = c.empty((n, max_pairs, 2), "int64"), c.empty((n,), "int64")
        L = _lib.load()
        if energy:
            e = c.empty((n, max_pairs))
            check(L.smplpp_self_penetration(self.handle, n, _ptr(verts), max_pairs, float(sigma), _ptr(pairs), _ptr(count), _ptr(e), c.space,
                                            c.stream))
        else:
            e = None
            check(L.smplpp_self_intersections(self.handle, n, _ptr(verts), max_pairs, _ptr(pairs), _ptr(count), c.space, c.stream))
        if check_count:
            most = int(count.max().item()) if c.dev else int(count.max())  # one read of count on the device
            if most > max_pairs:
                raise SmplppError(1, "%s: %d intersecting face pairs in a frame, more than max_pairs = %d" % (name, most, max_pairs))
        return pairs, count, e

    def selfIntersections(self, verts, max_pairs=None, check=True):
        """The intersecting face pairs of each frame's posed mesh verts [N,V,3] (smplpp_self_intersections): returns (pairs
        [N,max_pairs,2] int64, count [N] int64).  Pairs (f, g), f < g, share no vertex and intersect under the exact fp32 edge-crossing
        rule of the C header, in ascending (f, g); rows past count are -1.  max_pairs defaults to 32768; a frame with more pairs
        raises (one read of count) unless check=False, when count holds the true total and the lowest max_pairs pairs are stored.
        numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        pairs, count, _ = self._sp_forward("selfIntersections", verts, max_pairs, 1.0, check, False)
        return pairs, count

    def selfPenetration(self, verts, sigma=2.0, max_pairs=None, check=True):
        """selfIntersections and one self-penetration energy per stored pair (smplpp_self_penetration): returns (pairs, count,
        pair_energy [N,max_pairs], 0 past count).  Each pair is scored both ways: the intruding corners below the receiver's plane,
        phi^2 h^2 with phi = max(0, 1 - q^2 / (sigma^2 rho^2)) (the C header states the field)."""
        return self._sp_forward("selfPenetration", verts, max_pairs, sigma, check, True)

    def selfPenetrationBackward(self, verts, pairs, count, grad_pair_energy, sigma=2.0, out=None):
        """Vector-Jacobian product of selfPenetration's pair_energy at the pairs [N,max_pairs,2] and count [N] it gave (the pair set
        held fixed): grad_verts [N,V,3] for dL/dpair_energy = grad_pair_energy [N,max_pairs] (smplpp_self_penetration_vjp).  With
        `out` [N,V,3] the gradient is added into it and it is returned.  The model keeps a workspace of N * max_pairs * 384 bytes
        (max_pairs from the shape of `pairs`), grown to the largest call."""
        c = _Call("selfPenetrationBackward", verts, grad_pair_energy, out)
        n = verts.shape[0] if c.dev else len(verts)
        verts = c.input(verts, (n, self.vertex_num, 3))
        pr, cn = c.ids(pairs), c.ids(count)
        if pr.shape[0] % (2 * n) or cn.shape[0] != n:
            c.refuse("expected pairs of shape (%d, max_pairs, 2) and count of shape (%d,)" % (n, n))
        max_pairs = pr.shape[0] // (2 * n)
        g = c.input(grad_pair_energy, (n, max_pairs))
        acc = out is not None
        gv = c.inout(out, (n, self.vertex_num, 3)) if acc else c.empty((n, self.vertex_num, 3))
        check(_lib.load().smplpp_self_penetration_vjp(self.handle, n, _ptr(verts), max_pairs, float(sigma), _ptr(pr), _ptr(cn), _ptr(g),
                                                      _ptr(gv), int(acc), c.space, c.stream))
        return gv

    def self_penetration_differentiable(self, verts, sigma=2.0, max_pairs=None, check=True):
        """(pairs [N,max_pairs,2], count [N], pair_energy [N,max_pairs]) of device vertices verts [N,V,3] (the bits of
        selfPenetration), with pair_energy differentiable in verts through torch.autograd: smplpp_self_penetration forward,
        smplpp_self_penetration_vjp backward at the same pairs, on torch's current stream.  A loss is e.g. pair_energy.sum()."""
        if torch is None:
            raise SmplppError(1, "self_penetration_differentiable needs torch")
        return _SelfPenetrationFunction.apply(verts, self, float(sigma), max_pairs, check)

    # ---- depth rasteriser (smplpp_depth_raster / smplpp_depth_raster_vjp)
    def _dr_inputs(self, c, verts, camera, H, W):
        n = verts.shape[0] if c.dev else len(verts)
        verts = c.input(verts, (n, self.vertex_num, 3))
        if c.dev and not _is_torch(camera):
            camera = torch.from_numpy(pinhole_camera_rows(camera, n)).to(c.device)
        elif c.dev and camera.dim() == 1:
            camera = camera.expand(n, 16)
        elif not c.dev:
            camera = pinhole_camera_rows(camera, n)
        camera = c.input(camera, (n, 16))
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            c.refuse("H and W must be >= 1")
        return n, verts, camera, H, W

    def _depth_raster(self, name, verts, camera, H, W, near, want=("bary", "visible", "culled"), device_only=False):
        c = _Call(name, verts, device_only=device_only)
        n, verts, camera, H, W = self._dr_inputs(c, verts, camera, H, W)
        r = {"face": c.empty((n, H, W), "int64"), "depth": c.empty((n, H, W))}
        if "bary" in want:
            r["bary"] = c.empty((n, H, W, 3))
        if "visible" in want:
            r["visible"] = c.empty((n, self.vertex_num), "uint8")
        if "culled" in want:
            r["culled"] = c.empty((n,), "int64")
        check(_lib.load().smplpp_depth_raster(self.handle, n, _ptr(verts), _ptr(camera), H, W, float(near), _ptr(r["face"]),
                                              _ptr(r["depth"]), _ptr(r.get("bary")), _ptr(r.get("visible")), _ptr(r.get("culled")),
                                              c.space, c.stream))
        return r

    def depthRaster(self, verts, camera, H, W, near=0.05, want=("bary", "visible", "culled")):
        """Each frame's posed mesh verts [N,V,3] through a pinhole camera into an H x W image (smplpp_depth_raster): a dict of face
        [N,H,W] int64 (-1 = background), depth [N,H,W] (camera-space z of the pixel-centre ray's hit, 0 at background), bary [N,H,W,3]
        (3-D barycentrics of the hit in the face's corners), visible [N,V] uint8 (1 iff the vertex is a corner of a face that owns a
        pixel) and culled [N] int64 (faces skipped: a corner at or behind `near`, non-finite, or beyond the guard band).  camera
        [N,16] or [16] as pinhole_camera packs it.  The rule is exact and stated in the C header.  numpy (the call synchronises) or
        float32 device tensors (torch's current stream); `want` drops optional outputs."""
        return self._depth_raster("depthRaster", verts, camera, H, W, near, want)

    def depthRasterBackward(self, verts, camera, H, W, face, grad_depth, out=None):
        """Vector-Jacobian product of depthRaster's depth at the faces it gave (held fixed; coverage is not differentiated):
        grad_verts [N,V,3] for dL/ddepth = grad_depth [N,H,W] (smplpp_depth_raster_vjp).  A pixel with face -1 or a cotangent of
        exactly 0 contributes nothing.  With `out` [N,V,3] the gradient is added into it and it is returned."""
        c = _Call("depthRasterBackward", verts, grad_depth, out)
        n, verts, camera, H, W = self._dr_inputs(c, verts, camera, H, W)
        f = c.ids(face)
        if f.shape[0] != n * H * W:
            c.refuse("expected face of shape (%d, %d, %d)" % (n, H, W))
        g = c.input(grad_depth, (n, H, W))
        acc = out is not None
        gv = c.inout(out, (n, self.vertex_num, 3)) if acc else c.empty((n, self.vertex_num, 3))
        check(_lib.load().smplpp_depth_raster_vjp(self.handle, n, _ptr(verts), _ptr(camera), H, W, _ptr(f), _ptr(g), _ptr(gv), int(acc),
                                                  c.space, c.stream))
        return gv

    def depth_raster_differentiable(self, verts, camera, H, W, near=0.05):
        """(depth [N,H,W], face [N,H,W], visible [N,V]) of device vertices verts [N,V,3] (the bits of depthRaster), with depth
        differentiable in verts through torch.autograd: smplpp_depth_raster forward, smplpp_depth_raster_vjp backward at the same
        faces, on torch's current stream.  A projective-ICP term is e.g. ((depth - target)[(face >= 0) & (target > 0)] ** 2).sum()."""
        if torch is None:
            raise SmplppError(1, "depth_raster_differentiable needs torch")
        return _DepthRasterFunction.apply(verts, self, camera, int(H), int(W), float(near))

    # ---- raster attribute interpolation (smplpp_raster_interpolate / smplpp_raster_interpolate_vjp)
    def _ri_inputs(self, c, attr, face, bary):
        if len(attr.shape) != 3 or attr.shape[1] != self.vertex_num or not 1 <= attr.shape[2] <= 32:
            c.refuse("expected attr of shape (N, %d, C) with C in [1, 32]" % self.vertex_num)
        if len(bary.shape) != 4 or bary.shape[0] != attr.shape[0] or bary.shape[3] != 3 or min(bary.shape) < 1:
            c.refuse("expected bary of shape (N, H, W, 3)")
        n, Cn = int(attr.shape[0]), int(attr.shape[2])
        H, W = int(bary.shape[1]), int(bary.shape[2])
        attr, bary, f = c.input(attr, (n, self.vertex_num, Cn)), c.input(bary, (n, H, W, 3)), c.ids(face)
        if f.shape[0] != n * H * W:
            c.refuse("expected face of shape (%d, %d, %d)" % (n, H, W))
        return n, Cn, H, W, attr, f, bary

    def _raster_interpolate(self, name, attr, face, bary, device_only=False):
        c = _Call(name, attr, bary, device_only=device_only)
        n, Cn, H, W, attr, f, bary = self._ri_inputs(c, attr, face, bary)
        image = c.empty((n, H, W, Cn))
        check(_lib.load().smplpp_raster_interpolate(self.handle, n, _ptr(attr), Cn, H, W, _ptr(f), _ptr(bary), _ptr(image), c.space,
                                                    c.stream))
        return image

    def rasterInterpolate(self, attr, face, bary):
        """A per-vertex quantity attr [N,V,C] (C <= 32) carried into the image of depthRaster (smplpp_raster_interpolate): image
        [N,H,W,C] with image = (beta_a attr[a] + beta_b attr[b]) + beta_c attr[c] at a pixel whose face [N,H,W] has the corners
        (a, b, c) and whose barycentrics are bary [N,H,W,3]; 0 at background.  face and bary are depthRaster's outputs.  The rule is
        exact and stated in the C header.  numpy (the call synchronises) or float32 device tensors (torch's current stream)."""
        return self._raster_interpolate("rasterInterpolate", attr, face, bary)

    def rasterInterpolateBackward(self, attr, verts, camera, H, W, face, bary, grad_image, near=0.05, want=("attr", "verts"), out=None):
        """Vector-Jacobian product of rasterInterpolate's image (smplpp_raster_interpolate_vjp): a dict of `attr`, grad_attr [N,V,C]
        (face and bary held fixed), and `verts`, grad_verts [N,V,3], the gradient through the barycentrics (face and the pixels'
        rays held fixed; coverage is not differentiated), for dL/dimage = grad_image [N,H,W,C].  verts, camera, H, W, near are the
        arguments of the depthRaster call that gave face and bary.  A cotangent of exactly 0 or a pixel with face -1 contributes
        nothing.  `want` drops an output; with `out`, a dict of arrays under the same keys, a gradient is added into its array."""
        c = _Call("rasterInterpolateBackward", attr, verts, bary, grad_image, *(out or {}).values())
        want = tuple(want)
        if not want or any(k not in ("attr", "verts") for k in want) or any(k not in want for k in (out or {})):
            c.refuse("want must name attr and / or verts, and out only what want names")
        n, Cn, Hb, Wb, attr, f, bary = self._ri_inputs(c, attr, face, bary)
        n, verts, camera, H, W = self._dr_inputs(c, verts, camera, H, W)
        if (H, W) != (Hb, Wb) or n != attr.shape[0]:
            c.refuse("expected face and bary of %d frames of %d x %d" % (n, H, W))
        g = c.input(grad_image, (n, H, W, Cn))
        acc = bool(out)
        if acc and set(out) != set(want):
            c.refuse("out must hold every output that want names")
        shapes = {"attr": (n, self.vertex_num, Cn), "verts": (n, self.vertex_num, 3)}
        r = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in want}
        check(_lib.load().smplpp_raster_interpolate_vjp(self.handle, n, _ptr(attr), Cn, _ptr(verts), _ptr(camera), H, W, float(near),
                                                        _ptr(f), _ptr(bary), _ptr(g), _ptr(r.get("attr")), _ptr(r.get("verts")), int(acc),
                                                        c.space, c.stream))
        return r

    def raster_interpolate_differentiable(self, attr, verts, camera, H, W, near=0.05):
        """(image [N,H,W,C], face [N,H,W], depth [N,H,W]) of device attributes attr [N,V,C] on device vertices verts [N,V,3]: one
        depthRaster and one rasterInterpolate, with image differentiable through torch.autograd in attr and, through the
        barycentrics, in verts (smplpp_raster_interpolate_vjp at the same face and bary), on torch's current stream.  depth carries
        no gradient here (depth_raster_differentiable does that)."""
        if torch is None:
            raise SmplppError(1, "raster_interpolate_differentiable needs torch")
        return _RasterInterpolateFunction.apply(attr, verts, self, camera, int(H), int(W), float(near))

    def normal_map_differentiable(self, verts, camera, H, W, near=0.05):
        """(normals [N,H,W,3], face [N,H,W]) of device vertices verts [N,V,3]: the whole-mesh vertex normals
        (vertex_normals_differentiable) rotated into camera space, interpolated by raster_interpolate_differentiable and normalised
        per pixel in torch; 0 at background.  The gradient reaches verts through the vertex normals and through the barycentrics."""
        if torch is None:
            raise SmplppError(1, "normal_map_differentiable needs torch")
        n = verts.shape[0]
        cam = camera if _is_torch(camera) else torch.from_numpy(pinhole_camera_rows(camera, n)).to(verts.device)
        R = (cam.expand(n, 16) if cam.dim() == 1 else cam)[:, :9].reshape(n, 3, 3)
        nc = torch.matmul(self.vertex_normals_differentiable(verts), R.transpose(1, 2))
        image, face, _ = self.raster_interpolate_differentiable(nc, verts, cam, H, W, near)
        length = image.norm(dim=-1, keepdim=True)
        covered = (face >= 0).unsqueeze(-1) & (length > 0)
        return torch.where(covered, image / torch.where(covered, length, torch.ones_like(length)), torch.zeros_like(image)), face

    # ---- SMPL+D: vertex offsets through skinning and the mesh Laplacian (smplpp_vertex_offsets / _vjp / smplpp_mesh_laplacian)
    def _offset_rows(self, c, offsets, n):
        """offsets [V,3], [1,V,3] or [n,V,3] as the call's input: (array [frames,V,3], frames)."""
        V = self.vertex_num
        shape = tuple(offsets.shape)
        if shape == (V, 3):
            offsets, shape = offsets.reshape(1, V, 3), (1, V, 3)
        if shape not in ((1, V, 3), (n, V, 3)):
            c.refuse("expected offsets of shape (%d, 3), (1, %d, 3) or (%d, %d, 3)" % (V, V, n, V))
        return c.input(offsets, shape), shape[0]

    def _vertex_offsets(self, c, verts, xforms, offsets, rest, out=None):
        n, V = int(verts.shape[0]), self.vertex_num
        verts, xforms, rest = c.input(verts, (n, V, 3)), c.input(xforms, (n, 24, 4, 4)), c.input(rest, (n, V, 3))
        d, frames = self._offset_rows(c, offsets, n)
        vo = c.inout(out, (n, V, 3)) if out is not None else c.empty((n, V, 3))
        rd = c.empty((n, V, 3)) if rest is not None else None
        check(_lib.load().smplpp_vertex_offsets(self.handle, n, _ptr(verts), _ptr(xforms), _ptr(d), frames, _ptr(rest), _ptr(rd), _ptr(vo),
                                                c.space, c.stream))
        return vo, rd

    def vertexOffsets(self, verts, xforms, offsets, rest=None, out=None):
        """SMPL+D (smplpp_vertex_offsets): the posed vertices of the body whose rest shape carries the per-vertex offsets `offsets`
        ([V,3] or [1,V,3]: one field for every frame; [N,V,3]: one per frame), LBS(rest + D, G'), from `verts` [N,V,3] and `xforms`
        [N,24,4,4] as launch returned them.  With `rest` [N,V,3] it returns (verts_displaced, rest_displaced), and rest_displaced is
        the `rest` launchBackward takes for the displaced body.  `out` [N,V,3] receives the vertices (it may be `verts`: in place).
        The rule is exact and stated in the C header.  numpy (the call synchronises) or float32 device tensors (torch's current
        stream)."""
        c = _Call("vertexOffsets", verts, xforms, offsets, rest, out)
        vo, rd = self._vertex_offsets(c, verts, xforms, offsets, rest, out)
        return vo if rest is None else (vo, rd)

    def vertexOffsetsBackward(self, xforms, grad_verts, shared=False, out=None):
        """Vector-Jacobian product of vertexOffsets to the offsets (smplpp_vertex_offsets_vjp): grad_offsets [N,V,3] for dL/dverts =
        grad_verts [N,V,3], or [1,V,3] with `shared` (one field for every frame: the frames' sum in the fixed order of the C
        header).  With `out` the gradient is added into it and it is returned."""
        c = _Call("vertexOffsetsBackward", xforms, grad_verts, out)
        n, V = int(grad_verts.shape[0]), self.vertex_num
        xforms, g = c.input(xforms, (n, 24, 4, 4)), c.input(grad_verts, (n, V, 3))
        frames = 1 if shared else n
        acc = out is not None
        go = c.inout(out, (frames, V, 3)) if acc else c.empty((frames, V, 3))
        check(_lib.load().smplpp_vertex_offsets_vjp(self.handle, n, _ptr(xforms), _ptr(g), frames, _ptr(go), int(acc), c.space, c.stream))
        return go

    def meshLaplacian(self, x, out=None):
        """The mesh Laplacian of a per-vertex field x [N,V,C], C <= 32 (smplpp_mesh_laplacian): (L x)_v = the sum over the faces at v
        of (x_v - x_a) + (x_v - x_b), twice the graph Laplacian on a closed manifold mesh.  L is symmetric: the gradient of
        |L D|^2 is 2 L (L D).  With `out` the result is added into it and it is returned."""
        c = _Call("meshLaplacian", x, out)
        if len(x.shape) != 3 or x.shape[1] != self.vertex_num or not 1 <= x.shape[2] <= 32:
            c.refuse("expected x of shape (N, %d, C) with C in [1, 32]" % self.vertex_num)
        shape = tuple(int(k) for k in x.shape)
        x = c.input(x, shape)
        acc = out is not None
        o = c.inout(out, shape) if acc else c.empty(shape)
        check(_lib.load().smplpp_mesh_laplacian(self.handle, shape[0], _ptr(x), shape[2], _ptr(o), int(acc), c.space, c.stream))
        return o

    def mesh_laplacian_differentiable(self, x):
        """meshLaplacian of a device tensor x [N,V,C], differentiable with torch.autograd (the operator is its own backward)."""
        if torch is None:
            raise SmplppError(1, "mesh_laplacian_differentiable needs torch")
        return _LaplacianFunction.apply(x, self)

    def forward_displaced_differentiable(self, beta, theta, offsets):
        """(verts [N,V,3], joints [N,24,3]) of the SMPL+D body for device tensors beta [N,10], theta [N,25,3] and offsets [V,3],
        [1,V,3] (one field for every frame) or [N,V,3], differentiable with torch.autograd in all three: the forward is one
        smplpp_fk and one smplpp_vertex_offsets, the backward smplpp_vertex_offsets_vjp and smplpp_fk_vjp on the displaced rest
        shape, on torch's current stream.  The joints are those of the undisplaced shape."""
        if torch is None:
            raise SmplppError(1, "forward_displaced_differentiable needs torch")
        return _FKDisplacedFunction.apply(beta, theta, offsets, self)

    # ---- bound points: skinning and its inverse (smplpp_skin_points / smplpp_unskin_points and their VJPs)
    def _bound_inputs(self, c, world, joints, points, face, bary, weights):
        """(n, K, world, joints, points, point_frames, face, bary, weights, bind_frames) of a bound-points call in the space of `c`.
        points [K,3], [1,K,3] or [n,K,3]; the binding is (face [K] | [1,K] | [n,K] with bary of the same frames) or weights
        [K,24] | [1,K,24] | [n,K,24]."""
        if len(world.shape) != 4 or tuple(world.shape[1:]) != (24, 3, 4) or world.shape[0] < 1:
            c.refuse("expected world of shape (N, 24, 3, 4)")
        n = int(world.shape[0])
        world, joints = c.input(world, (n, 24, 3, 4)), c.input(joints, (n, 24, 3))
        if joints is None or points is None:
            c.refuse("joints and points must be given")
        if len(points.shape) == 2:
            points = points.reshape((1,) + tuple(points.shape))
        if len(points.shape) != 3 or points.shape[2] != 3 or points.shape[0] not in (1, n) or points.shape[1] < 1:
            c.refuse("expected points of shape (K, 3), (1, K, 3) or (N, K, 3)")
        pf, K = int(points.shape[0]), int(points.shape[1])
        points = c.input(points, (pf, K, 3))
        if (weights is None) == (face is None and bary is None) or (weights is None and (face is None or bary is None)):
            c.refuse("give face and bary, or weights")
        if weights is not None:
            if len(weights.shape) == 2:
                weights = weights.reshape((1,) + tuple(weights.shape))
            if len(weights.shape) != 3 or tuple(weights.shape[1:]) != (K, 24) or weights.shape[0] not in (1, n):
                c.refuse("expected weights of shape (K, 24), (1, K, 24) or (N, K, 24)")
            bf = int(weights.shape[0])
            return n, K, world, joints, points, pf, None, None, c.input(weights, (bf, K, 24)), bf
        if len(bary.shape) == 2:
            bary = bary.reshape((1,) + tuple(bary.shape))
        if len(bary.shape) != 3 or tuple(bary.shape[1:]) != (K, 3) or bary.shape[0] not in (1, n):
            c.refuse("expected bary of shape (K, 3), (1, K, 3) or (N, K, 3)")
        bf = int(bary.shape[0])
        face = c.ids(face)
        if face.shape[0] != bf * K:
            c.refuse("expected face ids of shape %s" % ((bf, K),))
        return n, K, world, joints, points, pf, face, c.input(bary, (bf, K, 3)), None, bf

    def _bound_forward(self, name, unskin, world, joints, points, face, bary, weights, want, device_only=False):
        c = _Call(name, world, joints, points, bary, weights, device_only=device_only)
        n, K, world, joints, points, pf, face, bary, weights, bf = self._bound_inputs(c, world, joints, points, face, bary, weights)
        out = c.empty((n, K, 3))
        blend = c.empty((n, K, 3, 4)) if "blend" in want else None
        valid = c.empty((n, K), "uint8") if "valid" in want else None
        L = _lib.load()
        fn = L.smplpp_unskin_points if unskin else L.smplpp_skin_points
        check(fn(self.handle, n, _ptr(world), _ptr(joints), K, _ptr(points), pf, _ptr(face), _ptr(bary), _ptr(weights), bf, _ptr(out),
                 _ptr(blend), _ptr(valid), c.space, c.stream))
        return out, blend, valid

    def skinPoints(self, world, joints, points, face=None, bary=None, weights=None, want=("blend", "valid")):
        """Skinning of bound points (smplpp_skin_points): K rest-pose points `points` ([K,3] or [1,K,3]: one cloud for every frame;
        [N,K,3]: one per frame) carried by the blend of the joint transforms `world` [N,24,3,4] and `joints` [N,24,3] as `skeleton`
        returns them.  The binding is either `face` and `bary` (the face and weights of pointMeshDistance: the model's skinning
        weights interpolated over the face) or dense `weights` [K,24] | [1,K,24] | [N,K,24] used as given.  Returns (out [N,K,3],
        blend [N,K,3,4], valid [N,K] uint8): the posed points, each point's own transform (for normals or covariances) and 1 for a
        live point; a dead point (C header) gives zeros.  An output missing from `want` is returned as None.  numpy (the call
        synchronises) or float32 device tensors (torch's current stream)."""
        return self._bound_forward("skinPoints", False, world, joints, points, face, bary, weights, want)

    def unskinPoints(self, world, joints, points, face=None, bary=None, weights=None, want=("blend", "valid")):
        """The inverse of skinPoints (smplpp_unskin_points): `points` are posed points and the result the rest-pose points that
        skinPoints carries onto them under the same binding: the canonicalisation of a posed scan.  A point whose blend has
        collapsed (|det| <= 1e-4 s^3) is dead.  Arguments and returns as skinPoints; blend is the transform of the forward map."""
        return self._bound_forward("unskinPoints", True, world, joints, points, face, bary, weights, want)

    def _bound_backward(self, name, unskin, world, joints, points, grad_out, face, bary, weights, want, out):
        acc = out is not None
        c = _Call(name, world, joints, points, bary, weights, grad_out, *(out.values() if acc else ()))
        n, K, world, joints, points, pf, face, bary, weights, bf = self._bound_inputs(c, world, joints, points, face, bary, weights)
        if grad_out is None:
            c.refuse("grad_out must be given")
        g = c.input(grad_out, (n, K, 3))
        shapes = {"points": (pf, K, 3), "world": (n, 24, 3, 4), "joints": (n, 24, 3), "weights": (bf, K, 24)}
        keys = [k for k in shapes if k in (out if acc else want) and (k != "weights" or weights is not None or acc)]
        if not keys:
            c.refuse("points, world, joints or weights must be asked for")
        res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
        L = _lib.load()
        fn = L.smplpp_unskin_points_vjp if unskin else L.smplpp_skin_points_vjp
        check(fn(self.handle, n, _ptr(world), _ptr(joints), K, _ptr(points), pf, _ptr(face), _ptr(bary), _ptr(weights), bf, _ptr(g),
                 _ptr(res.get("points")), _ptr(res.get("world")), _ptr(res.get("joints")), _ptr(res.get("weights")), int(acc), c.space,
                 c.stream))
        return res

    def skinPointsBackward(self, world, joints, points, grad_out, face=None, bary=None, weights=None,
                           want=("points", "world", "joints", "weights"), out=None):
        """Vector-Jacobian product of skinPoints (smplpp_skin_points_vjp) for grad_out = dL/dout [N,K,3]: a dict of "points" (the
        shape of the points as passed, [1,K,3] for a shared cloud: the frames' sum), "world" [N,24,3,4] and "joints" [N,24,3] (the
        cotangents skeletonBackward takes) and, for a weight binding, "weights" ([1,K,24] for shared weights: the frames' sum).
        `want` drops outputs; with `out` (a dict keyed the same way) the gradients are ADDED into its arrays."""
        return self._bound_backward("skinPointsBackward", False, world, joints, points, grad_out, face, bary, weights, want, out)

    def unskinPointsBackward(self, world, joints, points, grad_out, face=None, bary=None, weights=None,
                             want=("points", "world", "joints", "weights"), out=None):
        """Vector-Jacobian product of unskinPoints (smplpp_unskin_points_vjp) for grad_out = dL/d(rest points) [N,K,3]; "points" is
        the gradient to the posed points.  Otherwise as skinPointsBackward."""
        return self._bound_backward("unskinPointsBackward", True, world, joints, points, grad_out, face, bary, weights, want, out)

    def skin_points_differentiable(self, world, joints, points, face=None, bary=None, weights=None):
        """skinPoints' posed points [N,K,3] for device tensors, differentiable with torch.autograd in world, joints, points and
        weights (not in face or bary: fixed correspondences); composes with skeleton_differentiable.  smplpp_skin_points forward,
        smplpp_skin_points_vjp backward, on torch's current stream.  First derivatives only."""
        if torch is None:
            raise SmplppError(1, "skin_points_differentiable needs torch")
        return _SkinPointsFunction.apply(world, joints, points, weights, face, bary, self, False)

    def unskin_points_differentiable(self, world, joints, points, face=None, bary=None, weights=None):
        """unskinPoints' rest-pose points [N,K,3], differentiable as skin_points_differentiable (points: the posed points)."""
        if torch is None:
            raise SmplppError(1, "unskin_points_differentiable needs torch")
        return _SkinPointsFunction.apply(world, joints, points, weights, face, bary, self, True)

    # ---- silhouette term (smplpp_mask_distance_transform / smplpp_silhouette / smplpp_silhouette_vjp)
    def maskDistanceTransform(self, mask, want=("nearest", "sqdist")):
        """Exact Euclidean feature transform of binary images mask [N,H,W] (nonzero = set; smplpp_mask_distance_transform): returns
        (nearest [N,H,W] int64, sqdist [N,H,W] int32): the linear index j' W + i' of the nearest set pixel of the same frame (the lowest
        index among equal distances) and the squared distance in px^2; a frame without a set pixel gives -1 and 0.  numpy (the call
        synchronises) or device tensors (torch's current stream); an output missing from `want` is returned as None."""
        c = _Call("maskDistanceTransform", mask)
        if len(mask.shape) != 3 or min(mask.shape) < 1:
            c.refuse("expected a mask of shape (N, H, W)")
        n, H, W = (int(x) for x in mask.shape)
        mk = c.flags(mask)
        nearest = c.empty((n, H, W), "int64") if "nearest" in want else None
        sqdist = c.empty((n, H, W), "int32") if "sqdist" in want else None
        check(_lib.load().smplpp_mask_distance_transform(self.handle, n, _ptr(mk), H, W, _ptr(nearest), _ptr(sqdist), c.space, c.stream))
        return nearest, sqdist

    def _sil_images(self, c, n, H, W, face, mask):
        f, mk = c.ids(face), c.flags(mask)
        if f.shape[0] != n * H * W or mk.shape[0] != n * H * W:
            c.refuse("expected face and mask of shape (%d, %d, %d)" % (n, H, W))
        return f, mk

    def _silhouette(self, name, verts, camera, H, W, mask, near, face, want, device_only=False):
        c = _Call(name, verts, device_only=device_only)
        n, verts, camera, H, W = self._dr_inputs(c, verts, camera, H, W)
        if face is None:
            r = {"face": c.empty((n, H, W), "int64"), "depth": c.empty((n, H, W))}
            check(_lib.load().smplpp_depth_raster(self.handle, n, _ptr(verts), _ptr(camera), H, W, float(near), _ptr(r["face"]),
                                                  _ptr(r["depth"]), None, None, None, c.space, c.stream))
            face = r["face"]
        f, mk = self._sil_images(c, n, H, W, face, mask)
        shapes = {"vert_target": ((n, self.vertex_num), "int64"), "vert_sq": ((n, self.vertex_num), "float32"),
                  "pix_source": ((n, H, W), "int64"), "pix_sq": ((n, H, W), "float32")}
        out = {k: c.empty(*shapes[k]) for k in shapes if k in want}
        check(_lib.load().smplpp_silhouette(self.handle, n, _ptr(verts), _ptr(camera), H, W, float(near), _ptr(f), _ptr(mk),
                                            _ptr(out.get("vert_target")), _ptr(out.get("vert_sq")), _ptr(out.get("pix_source")),
                                            _ptr(out.get("pix_sq")), c.space, c.stream))
        out["face"] = face
        return out

    def silhouette(self, verts, camera, H, W, mask, near=0.05, face=None, want=("vert_target", "vert_sq", "pix_source", "pix_sq")):
        """The two silhouette residual sets of each frame's posed mesh verts [N,V,3] against a target mask [N,H,W] (nonzero = set;
        smplpp_silhouette): a dict of vert_target [N,V] int64 and vert_sq [N,V] (a vertex that projects outside the mask: the nearest
        mask pixel's linear index and the squared distance of the projection to its centre, px^2; else -1 and 0), pix_source [N,H,W]
        int64 and pix_sq [N,H,W] (a mask pixel the body does not cover: the nearest covered pixel and the squared distance; else -1
        and 0), and `face`, the rasteriser's face image the coverage was read from: the `face` given (depthRaster's output for the
        same arguments), or a rasterisation the call runs itself.  camera [N,16] or [16] as pinhole_camera packs it.  numpy (the call
        synchronises) or device tensors (torch's current stream); `want` drops outputs."""
        return self._silhouette("silhouette", verts, camera, H, W, mask, near, face, want)

    def silhouetteBackward(self, verts, camera, H, W, face, vert_target=None, pix_source=None, grad_vert_sq=None, grad_pix_sq=None,
                           near=0.05, out=None):
        """Vector-Jacobian product of silhouette's vert_sq and pix_sq at the correspondences it gave (vert_target, pix_source and face
        held fixed): grad_verts [N,V,3] for dL/dvert_sq = grad_vert_sq [N,V] and dL/dpix_sq = grad_pix_sq [N,H,W], either of which
        may be None (smplpp_silhouette_vjp).  A cotangent of exactly 0 or an id of -1 contributes nothing.  With `out` [N,V,3] the
        gradient is added into it and it is returned.  With grad_pix_sq the model keeps a workspace of N * H * W * 64 bytes."""
        c = _Call("silhouetteBackward", verts, grad_vert_sq, grad_pix_sq, out)
        n, verts, camera, H, W = self._dr_inputs(c, verts, camera, H, W)
        if grad_vert_sq is None and grad_pix_sq is None:
            c.refuse("grad_vert_sq or grad_pix_sq must be given")
        if (grad_vert_sq is not None and vert_target is None) or (grad_pix_sq is not None and pix_source is None):
            c.refuse("a cotangent needs its correspondences (vert_target, pix_source)")
        f = c.ids(face)
        if f.shape[0] != n * H * W:
            c.refuse("expected face of shape (%d, %d, %d)" % (n, H, W))
        vt = ps = gs = gp = None
        if grad_vert_sq is not None:
            vt, gs = c.ids(vert_target), c.input(grad_vert_sq, (n, self.vertex_num))
            if vt.shape[0] != n * self.vertex_num:
                c.refuse("expected vert_target of shape (%d, %d)" % (n, self.vertex_num))
        if grad_pix_sq is not None:
            ps, gp = c.ids(pix_source), c.input(grad_pix_sq, (n, H, W))
            if ps.shape[0] != n * H * W:
                c.refuse("expected pix_source of shape (%d, %d, %d)" % (n, H, W))
        acc = out is not None
        gv = c.inout(out, (n, self.vertex_num, 3)) if acc else c.empty((n, self.vertex_num, 3))
        check(_lib.load().smplpp_silhouette_vjp(self.handle, n, _ptr(verts), _ptr(camera), H, W, float(near), _ptr(f), _ptr(vt), _ptr(ps),
                                                _ptr(gs), _ptr(gp), _ptr(gv), int(acc), c.space, c.stream))
        return gv

    def silhouette_differentiable(self, verts, camera, H, W, mask, near=0.05):
        """(vert_sq [N,V], pix_sq [N,H,W]) of device vertices verts [N,V,3] against the target mask [N,H,W] (the bits of silhouette,
        which rasterises the frame itself), differentiable in verts through torch.autograd: smplpp_silhouette forward,
        smplpp_silhouette_vjp backward at the same correspondences, on torch's current stream.  A silhouette term is e.g.
        vert_sq.mean() + pix_sq.sum() / (pix_sq > 0).sum()."""
        if torch is None:
            raise SmplppError(1, "silhouette_differentiable needs torch")
        return _SilhouetteFunction.apply(verts, self, camera, int(H), int(W), mask, float(near))

    def out(self, index: int, path: str):
        """SMPL::out (src/SMPL.cpp:757-790): Wavefront OBJ of frame `index` (v lines, then 1-based f lines)."""
        verts = self._need("verts")
        v = verts[index].detach().cpu().numpy() if _is_torch(verts) else verts[index]
        with open(path, "w") as f:
            for p in v:
                f.write("v %f %f %f\n" % (p[0], p[1], p[2]))
            for t in self._model["face_indices"]:
                f.write("f %d %d %d\n" % (t[0], t[1], t[2]))


if torch is not None:
    class _FKFunction(torch.autograd.Function):
        """smplpp_fk forward / smplpp_fk_vjp backward (SMPL.forward_differentiable)."""

        @staticmethod
        def forward(ctx, beta, theta, smpl):
            c = _Call("forward_differentiable", beta, theta, fail="Cannot launch a SMPL model!", device_only=True)
            beta, theta, out = smpl._fk(c, beta, theta, ("verts", "joints", "rest"))
            ctx.smpl = smpl
            ctx.save_for_backward(beta, theta, out["rest"])
            ctx.save_for_forward(beta, theta, out["rest"])
            return out["verts"], out["joints"]

        @staticmethod
        def backward(ctx, grad_verts, grad_joints):
            beta, theta, rest = ctx.saved_tensors
            if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
                return None, None, None
            g = ctx.smpl.launchBackward(beta, theta, grad_verts=grad_verts, grad_joints=grad_joints, rest=rest)
            return (g["beta"] if ctx.needs_input_grad[0] else None, g["theta"] if ctx.needs_input_grad[1] else None, None)

        @staticmethod
        def jvp(ctx, dbeta, dtheta, _):
            """Forward mode (torch.autograd.forward_ad): one smplpp_fk_jvp with T = 1; a tangent of None counts as zero."""
            beta, theta, rest = ctx.saved_tensors
            if dbeta is None and dtheta is None:
                return None, None
            d = ctx.smpl.launchTangent(beta, theta, dbeta=None if dbeta is None else dbeta.unsqueeze(1),
                                       dtheta=None if dtheta is None else dtheta.unsqueeze(1), rest=rest, want=("verts", "joints"))
            return d["verts"].squeeze(1), d["joints"].squeeze(1)

    class _FKRotmatFunction(torch.autograd.Function):
        """smplpp_fk_rotmat forward / smplpp_fk_rotmat_vjp backward (SMPL.forward_rotmat_differentiable)."""

        @staticmethod
        def forward(ctx, beta, trans, rot, smpl):
            c = _Call("forward_rotmat_differentiable", rot, beta, trans, fail="Cannot launch a SMPL model!", device_only=True)
            beta, trans, rot, out = smpl._fk_rotmat(c, beta, trans, rot, ("verts", "joints", "xforms", "rest"))
            ctx.smpl = smpl
            ctx.save_for_backward(beta, trans, rot, out["rest"])
            ctx.save_for_forward(beta, trans, rot, out["rest"])
            ctx.mark_non_differentiable(out["xforms"])
            return out["verts"], out["joints"], out["xforms"]

        @staticmethod
        def jvp(ctx, dbeta, dtrans, drot, _):
            """Forward mode: one smplpp_fk_rotmat_jvp with T = 1; a tangent of None counts as zero, xforms has no tangent."""
            beta, trans, rot, rest = ctx.saved_tensors
            if dbeta is None and dtrans is None and drot is None:
                return None, None, None
            t = [None if a is None else a.unsqueeze(1) for a in (dbeta, dtrans, drot)]
            d = ctx.smpl.launchRotmatTangent(beta, trans, rot, dbeta=t[0], dtrans=t[1], drot=t[2], rest=rest, want=("verts", "joints"))
            return d["verts"].squeeze(1), d["joints"].squeeze(1), None

        @staticmethod
        def backward(ctx, grad_verts, grad_joints, _grad_xforms):
            beta, trans, rot, rest = ctx.saved_tensors
            if not any(ctx.needs_input_grad[:3]):
                return None, None, None, None
            g = ctx.smpl.launchRotmatBackward(beta, trans, rot, grad_verts=grad_verts, grad_joints=grad_joints, rest=rest)
            return tuple(g[k] if need else None for k, need in zip(("beta", "trans", "rot"), ctx.needs_input_grad)) + (None,)

    class _SkeletonFunction(torch.autograd.Function):
        """smplpp_skeleton forward / smplpp_skeleton_vjp backward (SMPL.skeleton_differentiable)."""

        @staticmethod
        def forward(ctx, beta, theta, smpl):
            c = _Call("skeleton_differentiable", theta, beta, device_only=True)
            beta, _, theta, out = smpl._skeleton(c, beta, None, theta, False, ("world", "posed", "joints"))
            ctx.smpl = smpl
            ctx.save_for_backward(beta, theta)
            return out["world"], out["posed"], out["joints"]

        @staticmethod
        def backward(ctx, grad_world, grad_posed, grad_joints):
            beta, theta = ctx.saved_tensors
            want = tuple(k for k, need in zip(("beta", "theta"), ctx.needs_input_grad) if need)
            if not want or (grad_world is None and grad_posed is None and grad_joints is None):
                return None, None, None
            g = ctx.smpl.skeletonBackward(beta, theta, grad_world, grad_posed, grad_joints, want=want)
            return g.get("beta"), g.get("theta"), None

    class _SkeletonRotmatFunction(torch.autograd.Function):
        """smplpp_skeleton_rotmat forward / smplpp_skeleton_rotmat_vjp backward (SMPL.skeleton_rotmat_differentiable)."""

        @staticmethod
        def forward(ctx, beta, trans, rot, smpl):
            c = _Call("skeleton_rotmat_differentiable", rot, beta, trans, device_only=True)
            beta, trans, rot, out = smpl._skeleton(c, beta, trans, rot, True, ("world", "posed", "joints"))
            ctx.smpl = smpl
            ctx.save_for_backward(beta, trans, rot)
            return out["world"], out["posed"], out["joints"]

        @staticmethod
        def backward(ctx, grad_world, grad_posed, grad_joints):
            beta, trans, rot = ctx.saved_tensors
            want = tuple(k for k, need in zip(("beta", "trans", "rot"), ctx.needs_input_grad) if need)
            if not want or (grad_world is None and grad_posed is None and grad_joints is None):
                return None, None, None, None
            g = ctx.smpl.skeletonRotmatBackward(beta, trans, rot, grad_world, grad_posed, grad_joints, want=want)
            return g.get("beta"), g.get("trans"), g.get("rot"), None

    class _FKDisplacedFunction(torch.autograd.Function):
        """smplpp_fk + smplpp_vertex_offsets forward / smplpp_vertex_offsets_vjp + smplpp_fk_vjp(rest = rest_displaced) backward
        (SMPL.forward_displaced_differentiable)."""

        @staticmethod
        def forward(ctx, beta, theta, offsets, smpl):
            c = _Call("forward_displaced_differentiable", beta, theta, offsets, fail="Cannot launch a SMPL model!", device_only=True)
            beta, theta, out = smpl._fk(c, beta, theta, ("verts", "joints", "xforms", "rest"))
            _, rd = smpl._vertex_offsets(c, out["verts"], out["xforms"], offsets, out["rest"], out=out["verts"])
            ctx.smpl, ctx.offsets_shape = smpl, tuple(offsets.shape)
            ctx.save_for_backward(beta, theta, out["xforms"], rd)
            return out["verts"], out["joints"]

        @staticmethod
        def backward(ctx, grad_verts, grad_joints):
            beta, theta, xforms, rd = ctx.saved_tensors
            gb = gt = gd = None
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
                g = ctx.smpl.launchBackward(beta, theta, grad_verts=grad_verts, grad_joints=grad_joints, rest=rd)
                gb, gt = (g["beta"] if ctx.needs_input_grad[0] else None), (g["theta"] if ctx.needs_input_grad[1] else None)
            if ctx.needs_input_grad[2]:
                n, V = beta.shape[0], ctx.smpl.vertex_num
                shared = ctx.offsets_shape != (n, V, 3)
                gd = ctx.smpl.vertexOffsetsBackward(xforms, grad_verts.contiguous(), shared=shared).reshape(ctx.offsets_shape)
            return gb, gt, gd, None

    class _SkinPointsFunction(torch.autograd.Function):
        """smplpp_skin_points / smplpp_unskin_points forward, their VJPs backward (SMPL.skin_points_differentiable and
        unskin_points_differentiable)."""

        @staticmethod
        def forward(ctx, world, joints, points, weights, face, bary, smpl, unskin):
            name = "unskin_points_differentiable" if unskin else "skin_points_differentiable"
            out, _, _ = smpl._bound_forward(name, unskin, world, joints, points, face, bary, weights, (), device_only=True)
            ctx.smpl, ctx.unskin, ctx.face = smpl, unskin, face
            ctx.shapes = (tuple(points.shape), None if weights is None else tuple(weights.shape))
            ctx.save_for_backward(world, joints, points, weights, bary)
            return out

        @staticmethod
        def backward(ctx, grad_out):
            world, joints, points, weights, bary = ctx.saved_tensors
            keys = ("world", "joints", "points", "weights")
            want = tuple(k for k, need in zip(keys, ctx.needs_input_grad) if need and (k != "weights" or weights is not None))
            if not want:
                return (None,) * 8
            fn = ctx.smpl.unskinPointsBackward if ctx.unskin else ctx.smpl.skinPointsBackward
            g = fn(world, joints, points, grad_out.contiguous(), face=ctx.face, bary=bary, weights=weights, want=want)
            gp, gw = g.get("points"), g.get("weights")
            return (g.get("world"), g.get("joints"), None if gp is None else gp.reshape(ctx.shapes[0]),
                    None if gw is None else gw.reshape(ctx.shapes[1]), None, None, None, None)

    class _LaplacianFunction(torch.autograd.Function):
        """smplpp_mesh_laplacian forward and, the operator being symmetric, backward (SMPL.mesh_laplacian_differentiable)."""

        @staticmethod
        def forward(ctx, x, smpl):
            ctx.smpl = smpl
            return smpl.meshLaplacian(x.detach().contiguous())

        @staticmethod
        def backward(ctx, grad):
            return (ctx.smpl.meshLaplacian(grad.contiguous()) if ctx.needs_input_grad[0] else None), None

    class _NormalsFunction(torch.autograd.Function):
        """The normal queries forward / their vector-Jacobian products backward (SMPL.face_normals_differentiable,
        SMPL.vertex_normals_differentiable).  kind 0 = face list, 1 = vertex list, 2 = whole mesh."""

        @staticmethod
        def forward(ctx, verts, smpl, kind, ids):
            c = _Call("normals_differentiable", verts, device_only=True)
            verts = c.input(verts, (len(verts), smpl.vertex_num, 3))
            out, idt = smpl._normals_at(c, verts, kind, ids)
            ctx.smpl, ctx.kind, ctx.idt = smpl, kind, idt
            ctx.save_for_backward(verts)
            return out

        @staticmethod
        def backward(ctx, grad):
            (verts,) = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None, None
            gv = ctx.smpl._normals_vjp(ctx.kind, verts, ctx.idt, grad, None)
            return gv, None, None, None

    class _DistanceFunction(torch.autograd.Function):
        """The backward of both scan distances: a subclass's forward saves (verts, points, the chosen ids) and sets ctx.smpl,
        ctx.K, ctx.call_name and ctx.mesh_to_point (and ctx.inside, the flags of the signed distance); sqdist is its last output."""

        @staticmethod
        def backward(ctx, *grads):
            verts, points, ids = ctx.saved_tensors
            grad_sqdist = grads[-1]
            want_v, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if grad_sqdist is None or not (want_v or want_p):
                return None, None, None
            c = _Call(ctx.call_name, verts, device_only=True)
            gv, gp = ctx.smpl._distance_vjp(ctx.mesh_to_point, c, verts, points, ctx.K, ids, grad_sqdist.contiguous(), None, None, want_v,
                                            want_p, inside=getattr(ctx, "inside", None))
            return gv, gp, None

    class _PointDistanceFunction(_DistanceFunction):
        """smplpp_point_mesh_distance forward / smplpp_point_mesh_distance_vjp backward (SMPL.point_mesh_distance_differentiable)."""

        @staticmethod
        def forward(ctx, verts, points, smpl):
            ctx.call_name, ctx.mesh_to_point = "point_mesh_distance_differentiable", False
            c = _Call(ctx.call_name, verts, points, device_only=True)
            verts, points, K = smpl._pmd_inputs(c, verts, points)
            face, w, _, sq = smpl._pmd(c, verts, points, K, want_closest=False)
            ctx.mark_non_differentiable(face, w)
            ctx.smpl, ctx.K = smpl, K
            ctx.save_for_backward(verts, points, face)
            return face, w, sq

    class _MeshPointDistanceFunction(_DistanceFunction):
        """smplpp_mesh_point_distance forward / smplpp_mesh_point_distance_vjp backward (SMPL.mesh_point_distance_differentiable)."""

        @staticmethod
        def forward(ctx, verts, points, smpl):
            ctx.call_name, ctx.mesh_to_point = "mesh_point_distance_differentiable", True
            c = _Call(ctx.call_name, verts, points, device_only=True)
            verts, points, K = smpl._pmd_inputs(c, verts, points)
            index, sq = smpl._mpd(c, verts, points, K)
            ctx.mark_non_differentiable(index)
            ctx.smpl, ctx.K = smpl, K
            ctx.save_for_backward(verts, points, index)
            return index, sq

    class _PointDistanceCompatibleFunction(_DistanceFunction):
        """smplpp_point_mesh_distance_compatible forward / smplpp_point_mesh_distance_vjp backward, which ignores face -1 in device
        space (SMPL.point_mesh_distance_compatible_differentiable).  The normals and the filter's arguments get no gradient."""

        @staticmethod
        def forward(ctx, verts, points, smpl, normals, cos_min, cap):
            ctx.call_name, ctx.mesh_to_point = "point_mesh_distance_compatible_differentiable", False
            c = _Call(ctx.call_name, verts, points, normals, device_only=True)
            verts, points, K = smpl._pmd_inputs(c, verts, points)
            face, w, _, sq = smpl._pmdc(c, verts, points, normals, K, cos_min, cap, want_closest=False)
            matched = face >= 0
            ctx.mark_non_differentiable(face, w, matched)
            ctx.smpl, ctx.K = smpl, K
            ctx.save_for_backward(verts, points, face)
            return face, w, matched, sq

        @staticmethod
        def backward(ctx, *grads):
            return _DistanceFunction.backward(ctx, *grads) + (None, None, None)

    class _MeshPointDistanceCompatibleFunction(_DistanceFunction):
        """smplpp_mesh_point_distance_compatible forward / smplpp_mesh_point_distance_vjp backward
        (SMPL.mesh_point_distance_compatible_differentiable)."""

        @staticmethod
        def forward(ctx, verts, points, smpl, point_normals, vert_normals, cos_min, cap):
            ctx.call_name, ctx.mesh_to_point = "mesh_point_distance_compatible_differentiable", True
            c = _Call(ctx.call_name, verts, points, point_normals, vert_normals, device_only=True)
            verts, points, K = smpl._pmd_inputs(c, verts, points)
            index, sq = smpl._mpdc(c, verts, points, point_normals, vert_normals, K, cos_min, cap)
            matched = index >= 0
            ctx.mark_non_differentiable(index, matched)
            ctx.smpl, ctx.K = smpl, K
            ctx.save_for_backward(verts, points, index)
            return index, matched, sq

        @staticmethod
        def backward(ctx, *grads):
            return _DistanceFunction.backward(ctx, *grads) + (None, None, None, None)


    class _SignedDistanceFunction(_DistanceFunction):
        """smplpp_point_mesh_signed_distance forward / smplpp_point_mesh_signed_distance_vjp backward
        (SMPL.point_mesh_signed_distance_differentiable)."""

        @staticmethod
        def forward(ctx, verts, points, smpl):
            ctx.call_name, ctx.mesh_to_point = "point_mesh_signed_distance_differentiable", False
            c = _Call(ctx.call_name, verts, points, device_only=True)
            verts, points, K = smpl._pmd_inputs(c, verts, points)
            face, w, _, _, ins, sq = smpl._psd(c, verts, points, K, want_closest=False, want_winding=False)
            inside = ins.bool()
            ctx.mark_non_differentiable(face, w, inside)
            ctx.smpl, ctx.K, ctx.inside = smpl, K, ins
            ctx.save_for_backward(verts, points, face)
            return face, w, inside, sq


    class _RayCastFunction(torch.autograd.Function):
        """smplpp_ray_cast forward / smplpp_ray_cast_vjp backward (SMPL.ray_cast_differentiable)."""

        @staticmethod
        def forward(ctx, verts, origin, dir, smpl, t_min, t_max, facing):
            c = _Call("ray_cast_differentiable", verts, origin, dir, device_only=True)
            n, rf, K, v, o, d = smpl._ray_inputs(c, verts, origin, dir)
            face, t, bary, hits = smpl._ray_cast(c, n, rf, K, v, o, d, t_min, t_max, facing, ("bary", "hits"))
            hit = face >= 0
            ctx.mark_non_differentiable(face, bary, hits, hit)
            ctx.smpl, ctx.shapes = smpl, (tuple(origin.shape), tuple(dir.shape))
            ctx.save_for_backward(v, o, d, face)
            return face, t, bary, hits, hit

        @staticmethod
        def backward(ctx, _gf, grad_t, _gb, _gh, _ghit):
            v, o, d, face = ctx.saved_tensors
            want = tuple(k for k, need in zip(("verts", "origin", "dir"), ctx.needs_input_grad) if need)
            if not want:
                return (None,) * 7
            g = ctx.smpl.rayCastBackward(v, o, d, face, grad_t.contiguous(), want=want)
            go, gd = g.get("origin"), g.get("dir")
            return (g.get("verts"), None if go is None else go.reshape(ctx.shapes[0]), None if gd is None else gd.reshape(ctx.shapes[1]), None,
                    None, None, None)

    class _SelfPenetrationFunction(torch.autograd.Function):
        """smplpp_self_penetration forward / smplpp_self_penetration_vjp backward (SMPL.self_penetration_differentiable)."""

        @staticmethod
        def forward(ctx, verts, smpl, sigma, max_pairs, check_count):
            verts = verts.detach().contiguous()
            pairs, count, e = smpl._sp_forward("self_penetration_differentiable", verts, max_pairs, sigma, check_count, True,
                                               device_only=True)
            ctx.mark_non_differentiable(pairs, count)
            ctx.smpl, ctx.sigma = smpl, sigma
            ctx.save_for_backward(verts, pairs, count)
            return pairs, count, e

        @staticmethod
        def backward(ctx, _gp, _gc, grad_e):
            verts, pairs, count = ctx.saved_tensors
            if grad_e is None or not ctx.needs_input_grad[0]:
                return None, None, None, None, None
            gv = ctx.smpl.selfPenetrationBackward(verts, pairs, count, grad_e.contiguous(), ctx.sigma)
            return gv, None, None, None, None


    class _DepthRasterFunction(torch.autograd.Function):
        """smplpp_depth_raster forward / smplpp_depth_raster_vjp backward (SMPL.depth_raster_differentiable)."""

        @staticmethod
        def forward(ctx, verts, smpl, camera, H, W, near):
            verts = verts.detach().contiguous()
            camera = torch.from_numpy(pinhole_camera_rows(camera, verts.shape[0])).to(verts.device) if not _is_torch(camera) else camera
            r = smpl._depth_raster("depth_raster_differentiable", verts, camera, H, W, near, want=("visible",), device_only=True)
            ctx.mark_non_differentiable(r["face"], r["visible"])
            ctx.smpl, ctx.size = smpl, (H, W)
            ctx.save_for_backward(verts, camera, r["face"])
            return r["depth"], r["face"], r["visible"]

        @staticmethod
        def backward(ctx, grad_depth, _gf, _gv):
            verts, camera, face = ctx.saved_tensors
            if grad_depth is None or not ctx.needs_input_grad[0]:
                return None, None, None, None, None, None
            gv = ctx.smpl.depthRasterBackward(verts, camera, ctx.size[0], ctx.size[1], face, grad_depth.contiguous())
            return gv, None, None, None, None, None


    class _RasterInterpolateFunction(torch.autograd.Function):
        """smplpp_depth_raster + smplpp_raster_interpolate forward / smplpp_raster_interpolate_vjp backward
        (SMPL.raster_interpolate_differentiable)."""

        @staticmethod
        def forward(ctx, attr, verts, smpl, camera, H, W, near):
            attr, verts = attr.detach().contiguous(), verts.detach().contiguous()
            camera = torch.from_numpy(pinhole_camera_rows(camera, verts.shape[0])).to(verts.device) if not _is_torch(camera) else camera
            r = smpl._depth_raster("raster_interpolate_differentiable", verts, camera, H, W, near, want=("bary",), device_only=True)
            image = smpl._raster_interpolate("raster_interpolate_differentiable", attr, r["face"], r["bary"], device_only=True)
            ctx.mark_non_differentiable(r["face"], r["depth"])
            ctx.smpl, ctx.size, ctx.near = smpl, (H, W), near
            ctx.save_for_backward(attr, verts, camera, r["face"], r["bary"])
            return image, r["face"], r["depth"]

        @staticmethod
        def backward(ctx, grad_image, _gf, _gd):
            attr, verts, camera, face, bary = ctx.saved_tensors
            want = tuple(k for k, need in zip(("attr", "verts"), ctx.needs_input_grad[:2]) if need)
            if grad_image is None or not want:
                return None, None, None, None, None, None, None
            g = ctx.smpl.rasterInterpolateBackward(attr, verts, camera, ctx.size[0], ctx.size[1], face, bary, grad_image.contiguous(),
                                                   near=ctx.near, want=want)
            return g.get("attr"), g.get("verts"), None, None, None, None, None


    class _SilhouetteFunction(torch.autograd.Function):
        """smplpp_depth_raster + smplpp_silhouette forward / smplpp_silhouette_vjp backward (SMPL.silhouette_differentiable)."""

        @staticmethod
        def forward(ctx, verts, smpl, camera, H, W, mask, near):
            verts = verts.detach().contiguous()
            camera = torch.from_numpy(pinhole_camera_rows(camera, verts.shape[0])).to(verts.device) if not _is_torch(camera) else camera
            r = smpl._silhouette("silhouette_differentiable", verts, camera, H, W, mask, near, None,
                                 ("vert_target", "vert_sq", "pix_source", "pix_sq"), device_only=True)
            ctx.smpl, ctx.size, ctx.near = smpl, (H, W), near
            ctx.set_materialize_grads(False)  # an output the loss does not use: None, and its half of the backward is skipped
            ctx.save_for_backward(verts, camera, r["face"], r["vert_target"], r["pix_source"])
            return r["vert_sq"], r["pix_sq"]

        @staticmethod
        def backward(ctx, grad_vert_sq, grad_pix_sq):
            verts, camera, face, vt, ps = ctx.saved_tensors
            if (grad_vert_sq is None and grad_pix_sq is None) or not ctx.needs_input_grad[0]:
                return None, None, None, None, None, None, None
            gv = ctx.smpl.silhouetteBackward(verts, camera, ctx.size[0], ctx.size[1], face, vt if grad_vert_sq is not None else None,
                                             ps if grad_pix_sq is not None else None,
                                             None if grad_vert_sq is None else grad_vert_sq.contiguous(),
                                             None if grad_pix_sq is None else grad_pix_sq.contiguous(), near=ctx.near)
            return gv, None, None, None, None, None, None


    class _ProjectPointsFunction(torch.autograd.Function):
        """smplpp_project_points forward / smplpp_project_points_vjp backward (project_points_differentiable)."""

        @staticmethod
        def forward(ctx, points, camera, target, rho, near):
            points, camera = points.detach().contiguous(), camera.detach().contiguous()
            r = project_points(points, camera, target, rho, near)
            valid = r["valid"].bool()
            ctx.mark_non_differentiable(valid)
            ctx.rho, ctx.near = rho, near
            ctx.set_materialize_grads(False)  # an output the loss does not use: None, and the backward does not read it
            ctx.save_for_backward(points, camera, target.detach())
            return r["uv"], r["energy"], valid

        @staticmethod
        def backward(ctx, grad_uv, grad_energy, _gv):
            points, camera, target = ctx.saved_tensors
            want = tuple(k for k, need in zip(("points", "camera"), ctx.needs_input_grad[:2]) if need)
            if (grad_uv is None and grad_energy is None) or not want:
                return None, None, None, None, None
            g = project_points_backward(points, camera, target, ctx.rho, None if grad_uv is None else grad_uv.contiguous(),
                                        None if grad_energy is None else grad_energy.contiguous(), near=ctx.near, want=want)
            return g.get("points"), g.get("camera"), None, None, None


# ---- stage classes' functional forms (BlendShape / JointRegression / WorldTransformation / LinearBlendSkinning)
def stage_blend_shape(beta, theta24, shape_basis, pose_basis, device=0):
    beta, theta24, S, P = _np32(beta), _np32(theta24), _np32(shape_basis), _np32(pose_basis)
    n, V = beta.shape[0], S.shape[0]
    bs, bp, rot = np.empty((n, V, 3), np.float32), np.empty((n, V, 3), np.float32), np.empty((n, 24, 3, 3), np.float32)
    check(_lib.load().smplpp_stage_blend_shape(device, V, n, _ptr(beta), _ptr(theta24), _ptr(S), _ptr(P), _ptr(bs), _ptr(bp),
                                               _ptr(rot), HOST, None))
    return bs, bp, rot


def stage_joint_regression(T, Jreg, shape_blend, pose_blend, device=0):
    T, Jreg, bs, bp = _np32(T), _np32(Jreg), _np32(shape_blend), _np32(pose_blend)
    n, V = bs.shape[0], T.shape[0]
    rest, joints = np.empty((n, V, 3), np.float32), np.empty((n, 24, 3), np.float32)
    check(_lib.load().smplpp_stage_joint_regression(device, V, n, _ptr(T), _ptr(Jreg), _ptr(bs), _ptr(bp), _ptr(rest),
                                                    _ptr(joints), HOST, None))
    return rest, joints


def stage_world_transformation(kintree, joints, pose_rot, device=0):
    kt = np.ascontiguousarray(kintree, np.int64)
    joints, pose_rot = _np32(joints), _np32(pose_rot)
    n = joints.shape[0]
    out = np.empty((n, 24, 4, 4), np.float32)
    check(_lib.load().smplpp_stage_world_transformation(device, n, _ptr(kt), _ptr(joints), _ptr(pose_rot), _ptr(out), HOST, None))
    return out


def stage_skinning(weights, rest, xforms, root_pos=None, device=0):
    W, rest, xforms = _np32(weights), _np32(rest), _np32(xforms)
    n, V = rest.shape[0], W.shape[0]
    root = _np32(root_pos).reshape(n, 3) if root_pos is not None else None
    out = np.empty((n, V, 3), np.float32)
    check(_lib.load().smplpp_stage_skinning(device, V, n, _ptr(W), _ptr(rest), _ptr(xforms), _ptr(root), _ptr(out), HOST, None))
    return out
