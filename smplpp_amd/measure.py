"""Body measurements on the posed mesh (smplpp_measure_create / smplpp_measure / smplpp_measure_vjp): the surface area and enclosed
volume of regions of faces, and the length of the curve a plane cuts from a region (a girth), with gradients to the vertices and to
the planes.  numpy arrays are host space (the call stages and synchronises), torch tensors device space (enqueued on torch's current
stream); every number is produced by libsmplpp_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _ptr, torch

FORWARD = ("area", "volume", "section", "crossings")


def regions_by_joint(model, groups):
    """One region per group of joints: the 0-based ids, ascending, of the faces whose three corners all have their dominant skinning
    joint (the first largest weight) in the group.  `model` is the dict of model arrays (weights [V,24], face_indices 1-based) or an
    initialised SMPL; `groups` a list of lists of joint indices."""
    m = getattr(model, "_model", model)
    dominant = np.argmax(np.asarray(m["weights"]), axis=1)
    faces = np.asarray(m["face_indices"], np.int64) - 1
    return [np.nonzero(np.isin(dominant, np.asarray(g, np.int64))[faces].all(axis=1))[0].astype(np.int64) for g in groups]


def plane_through(point, normal):
    """The plane rows [..., 4] = (normal, normal . point) through `point` [..., 3] with `normal` [..., 3] (not normalised): plain torch,
    differentiable in both, so a plane can follow the `posed` joints of SMPL.skeleton_differentiable."""
    return torch.cat([normal, (normal * point).sum(-1, keepdim=True)], dim=-1)


class Measure:
    """Regions and sections on the faces of `smpl` (an initialised SMPL).  `regions`: a list of arrays of 0-based face ids (a body
    part, or all faces; they may overlap, one may be empty; the order of a list is the order of its sums).  `sections`: a list of
    region indices, one per plane: section s is planes[..., s, :] cutting the faces of region sections[s]."""

    def __init__(self, smpl, regions, sections=()):
        self._h = None
        self.vertex_num = smpl.vertex_num
        regions = [np.ascontiguousarray(r, np.int64).reshape(-1) for r in regions]
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in regions])]).astype(np.int64)
        face = np.ascontiguousarray(np.concatenate(regions + [np.zeros(0, np.int64)]), np.int64)
        sec = np.ascontiguousarray(sections, np.int64).reshape(-1)
        h = C.c_void_p()
        check(_lib.load().smplpp_measure_create(smpl.handle, len(regions), _ptr(ptr), _ptr(face), len(sec), _ptr(sec), C.byref(h)))
        self._h = h
        self.region_num, self.section_num = len(regions), len(sec)

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_measure_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "Measure: no handle")
        return self._h

    def info(self):
        R, nnz, S = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.load().smplpp_measure_info(self.handle, C.byref(R), C.byref(nnz), C.byref(S)))
        return dict(region_num=R.value, nnz=nnz.value, section_num=S.value)

    def _inputs(self, c, verts, planes, center):
        """(n, plane_frames, verts, planes, center) checked in the space of `c`."""
        if len(verts.shape) != 3 or verts.shape[0] < 1:
            c.refuse("expected verts of shape (N, V, 3)")
        n, S = int(verts.shape[0]), self.section_num
        if S and planes is None:
            c.refuse("the handle has sections: planes [N or 1, S, 4] are needed")
        pf = 1
        if S:
            if len(planes.shape) != 3 or int(planes.shape[0]) not in (1, n):
                c.refuse("expected planes of shape (N or 1, S, 4)")
            pf = int(planes.shape[0])
        return (n, pf, c.input(verts, (n, self.vertex_num, 3)), c.input(planes, (pf, S, 4)) if S else None, c.input(center, (n, 3)))

    def evaluate(self, verts, planes=None, center=None, want=FORWARD):
        """A dict of area [N,R], volume [N,R], section [N,S] and crossings [N,S] int32 (the faces each plane crosses) of verts [N,V,3]
        (smplpp_measure).  planes [N,S,4] or [1,S,4] (one set for every frame) are rows (nx, ny, nz, d) of the planes n . x = d, used
        as given; center [N,3] (None: zeros) is the point the volume's cones are taken from: for a body far from the origin pass a
        point inside it (the root joint).  `want` drops outputs; without sections the last two are left out."""
        c = _Call("evaluate", verts, planes, center)
        n, pf, verts, planes, center = self._inputs(c, verts, planes, center)
        R, S = self.region_num, self.section_num
        shapes = {"area": ((n, R), "float32"), "volume": ((n, R), "float32"), "section": ((n, S), "float32"), "crossings": ((n, S), "int32")}
        keys = [k for k in FORWARD if k in want and (S or k in ("area", "volume"))]
        if not keys:
            c.refuse("no output is asked for")
        res = {k: c.empty(*shapes[k]) for k in keys}
        check(_lib.load().smplpp_measure(self.handle, n, _ptr(verts), _ptr(center), _ptr(planes), pf, _ptr(res.get("area")),
                                         _ptr(res.get("volume")), _ptr(res.get("section")), _ptr(res.get("crossings")), c.space, c.stream))
        return res

    def evaluateBackward(self, verts, planes=None, center=None, grad_area=None, grad_volume=None, grad_section=None,
                         want=("verts", "planes"), out=None):
        """Vector-Jacobian product of evaluate (smplpp_measure_vjp): {"verts": [N,V,3], "planes": the shape of planes} for the
        cotangents grad_area [N,R], grad_volume [N,R] and grad_section [N,S] (None = zero).  "verts" is what SMPL.launchBackward takes
        as grad_verts.  `want` drops one; with `out` (a dict of arrays keyed the same way) the gradients are added into its arrays
        and it is returned.  center has no gradient: it is a constant of the definition."""
        acc = out is not None
        c = _Call("evaluateBackward", verts, planes, center, grad_area, grad_volume, grad_section, *(out.values() if acc else ()))
        n, pf, verts, planes, center = self._inputs(c, verts, planes, center)
        R, S = self.region_num, self.section_num
        ga, gvol = c.input(grad_area, (n, R)), c.input(grad_volume, (n, R))
        gs = c.input(grad_section, (n, S)) if S else None
        shapes = {"verts": (n, self.vertex_num, 3), "planes": (pf, S, 4)}
        keys = [k for k in shapes if k in (out if acc else want) and (S or k == "verts")]
        if not keys:
            c.refuse("verts or planes must be asked for")
        res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
        check(_lib.load().smplpp_measure_vjp(self.handle, n, _ptr(verts), _ptr(center), _ptr(planes), pf, _ptr(ga), _ptr(gvol), _ptr(gs),
                                             _ptr(res.get("verts")), _ptr(res.get("planes")), int(acc), c.space, c.stream))
        return res

    def forward_differentiable(self, verts, planes=None, center=None):
        """(area [N,R], volume [N,R], section [N,S]) on device tensors, differentiable in verts and planes with torch.autograd:
        smplpp_measure forward, smplpp_measure_vjp backward, on torch's current stream.  center is detached.  Without sections the
        third is an empty [N,0] tensor."""
        if torch is None:
            raise SmplppError(1, "forward_differentiable needs torch")
        return _MeasureFunction.apply(verts, planes, center, self)


if torch is not None:
    class _MeasureFunction(torch.autograd.Function):
        """smplpp_measure forward / smplpp_measure_vjp backward (Measure.forward_differentiable)."""

        @staticmethod
        def forward(ctx, verts, planes, center, ms):
            ctx.ms = ms
            v = verts.detach().contiguous()
            p = None if planes is None else planes.detach().contiguous()
            cc = None if center is None else center.detach().contiguous()
            ctx.save_for_backward(v, p, cc)
            r = ms.evaluate(v, p, cc, want=("area", "volume", "section"))
            return r["area"], r["volume"], r.get("section", v.new_zeros((v.shape[0], 0)))

        @staticmethod
        def backward(ctx, g_area, g_volume, g_section):
            v, p, cc = ctx.saved_tensors
            want = tuple(k for k, need in zip(("verts", "planes"), ctx.needs_input_grad[:2]) if need and (k == "verts" or p is not None))
            if not want:
                return None, None, None, None
            gs = g_section.contiguous() if ctx.ms.section_num else None
            g = ctx.ms.evaluateBackward(v, p, cc, g_area.contiguous(), g_volume.contiguous(), gs, want=want)
            return g.get("verts"), g.get("planes"), None, None
