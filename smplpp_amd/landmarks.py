"""Sparse landmark regression over a posed body (smplpp_landmarks_create / smplpp_landmarks / smplpp_landmarks_vjp): the 24 joints,
vertex picks and sparse rows over the vertices as one CSR matrix over [verts; joints].  With smpl.project_points it turns the body
into 2-D keypoints.  numpy arrays are host space (the call stages and synchronises), torch tensors device space (enqueued on
torch's current stream); every number is produced by libsmplpp_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _ptr, torch


class Landmarks:
    """An L-row regressor over the V + 24 sources of `smpl` (an initialised SMPL): column c < V is vertex c, column V + j is joint j
    of launch's joints.  row_ptr [L+1], col [nnz], val [nnz] as in scipy's csr_matrix; a column may repeat within a row.
    Column V + j reads row j of whatever [N,24,3] array is passed as `joints`: launch's rest joints, or the `posed` of
    SMPL.skeleton, which makes those columns the posed skeleton; the returned grad_joints is then SMPL.skeletonBackward's grad_posed."""

    def __init__(self, smpl, row_ptr, col, val):
        self._h = None
        self.vertex_num = smpl.vertex_num
        row_ptr = np.ascontiguousarray(row_ptr, np.int64).reshape(-1)
        col = np.ascontiguousarray(col, np.int64).reshape(-1)
        val = np.ascontiguousarray(val, np.float32).reshape(-1)
        if len(row_ptr) < 2 or len(col) != len(val) or (row_ptr[-1] != len(col) and 0 <= row_ptr[-1] <= 0x7FFFFFFF):
            raise SmplppError(1, "Landmarks: row_ptr [L+1] must end at the length of col and val")
        h = C.c_void_p()
        check(_lib.load().smplpp_landmarks_create(smpl.handle, len(row_ptr) - 1, _ptr(row_ptr), _ptr(col), _ptr(val), C.byref(h)))
        self._h = h
        self.landmark_num = len(row_ptr) - 1

    @classmethod
    def from_dense(cls, smpl, A_verts, A_joints=None):
        """The regressor of a dense A_verts [L,V] (and A_joints [L,24]): its non-zeros, row by row in ascending column."""
        A = np.asarray(A_verts, np.float32)
        if A_joints is not None:
            A = np.concatenate([A, np.asarray(A_joints, np.float32)], axis=1)
        if A.ndim != 2:
            raise SmplppError(1, "Landmarks.from_dense: expected A_verts [L,V] and A_joints [L,24]")
        rows, cols = np.nonzero(A)
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))])
        return cls(smpl, row_ptr, cols, A[rows, cols])

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_landmarks_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "Landmarks: no regressor")
        return self._h

    def info(self):
        L, nnz = C.c_int64(), C.c_int64()
        check(_lib.load().smplpp_landmarks_info(self.handle, C.byref(L), C.byref(nnz)))
        return dict(landmark_num=L.value, nnz=nnz.value)

    def regress(self, verts, joints):
        """points [N,L,3] from verts [N,V,3] and joints [N,24,3] as launch returned them (smplpp_landmarks)."""
        c = _Call("regress", verts, joints)
        n = int(verts.shape[0])
        verts, joints = c.input(verts, (n, self.vertex_num, 3)), c.input(joints, (n, 24, 3))
        points = c.empty((n, self.landmark_num, 3))
        check(_lib.load().smplpp_landmarks(self.handle, n, _ptr(verts), _ptr(joints), _ptr(points), c.space, c.stream))
        return points

    def regressBackward(self, grad_points, want=("verts", "joints"), out=None):
        """Vector-Jacobian product of regress (smplpp_landmarks_vjp): {"verts": [N,V,3], "joints": [N,24,3]} for dL/dpoints =
        grad_points [N,L,3]; the two are what SMPL.launchBackward takes as grad_verts and grad_joints.  `want` drops one; with `out`
        (a dict of arrays keyed the same way) the gradients are added into its arrays and it is returned."""
        acc = out is not None
        c = _Call("regressBackward", grad_points, *(out.values() if acc else ()))
        n = int(grad_points.shape[0])
        g = c.input(grad_points, (n, self.landmark_num, 3))
        shapes = {"verts": (n, self.vertex_num, 3), "joints": (n, 24, 3)}
        keys = [k for k in shapes if k in (out if acc else want)]
        if not keys:
            c.refuse("verts or joints must be asked for")
        res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
        check(_lib.load().smplpp_landmarks_vjp(self.handle, n, _ptr(g), _ptr(res.get("verts")), _ptr(res.get("joints")), int(acc), c.space,
                                               c.stream))
        return res

    def forward_differentiable(self, verts, joints):
        """regress on device tensors, differentiable in verts and joints with torch.autograd: smplpp_landmarks forward,
        smplpp_landmarks_vjp backward, on torch's current stream."""
        if torch is None:
            raise SmplppError(1, "forward_differentiable needs torch")
        return _LandmarksFunction.apply(verts, joints, self)


if torch is not None:
    class _LandmarksFunction(torch.autograd.Function):
        """smplpp_landmarks forward / smplpp_landmarks_vjp backward (Landmarks.forward_differentiable)."""

        @staticmethod
        def forward(ctx, verts, joints, lm):
            ctx.lm = lm
            return lm.regress(verts.detach().contiguous(), joints.detach().contiguous())

        @staticmethod
        def backward(ctx, grad):
            want = tuple(k for k, need in zip(("verts", "joints"), ctx.needs_input_grad[:2]) if need)
            if not want:
                return None, None, None
            g = ctx.lm.regressBackward(grad.contiguous(), want=want)
            return g.get("verts"), g.get("joints"), None
