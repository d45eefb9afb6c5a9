"""Self-contact on the posed body (smplpp_self_contact_create / smplpp_self_contact / smplpp_self_contact_vjp): a vertex's contact
partner is the nearest other vertex in space among those that are far along the surface.  "Far" is a static bit mask, built once per
subject from the geodesic distances of the rest mesh (smplpp_mesh_geodesic's rule; SMPL.meshGeodesic gives the fields themselves).
The loss on the partner distances (weights, a robustifier) stays in torch.  numpy arrays are host space (the call stages and
synchronises), torch tensors device space (enqueued on torch's current stream); every number is produced by libsmplpp_hip.so, except
filter_pairs, which is a lookup in the mask."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _ptr, torch


def mask_bits(mask, v, u):
    """far(v, u) of a mask [V,W] (numpy uint32, or a torch int32 / int64 tensor holding the same words) at index arrays v, u."""
    if _is_torch(mask):
        return ((mask[v, u >> 5].to(torch.int64) >> (u & 31)) & 1).bool()
    return ((mask[v, u >> 5] >> (u & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def filter_pairs(pairs, faces, mask):
    """Which rows of a selfIntersections pair list [..., 2] (face ids; -1 rows are padding) have all nine corner pairs far in `mask`
    [V,W]: a bool array of shape pairs.shape[:-1], so that pairs[keep] are the intersections between parts of the body that are not
    neighbours along the surface.  `faces` [F,3] 0-based.  numpy arrays, or torch tensors on one device."""
    if _is_torch(pairs):
        faces = torch.as_tensor(faces, dtype=torch.int64, device=pairs.device)
        valid = (pairs >= 0).all(-1)
        p = pairs.clamp(min=0).to(torch.int64)
        a, b = faces[p[..., 0]], faces[p[..., 1]]  # [..., 3]
        keep = valid
        for i in range(3):
            for j in range(3):
                keep = keep & mask_bits(mask, a[..., i], b[..., j])
        return keep
    pairs, faces = np.asarray(pairs, np.int64), np.asarray(faces, np.int64)
    valid = (pairs >= 0).all(-1)
    p = np.maximum(pairs, 0)
    a, b = faces[p[..., 0]], faces[p[..., 1]]
    keep = valid
    for i in range(3):
        for j in range(3):
            keep = keep & mask_bits(mask, a[..., i], b[..., j])
    return keep


class SelfContact:
    """The far relation of `smpl` (an initialised SMPL) on the rest mesh `rest` [V,3] (None: the model's template; for a subject, a
    frame of launch()'s "rest" at their beta): far(v, u) iff the geodesic distance between them is above geo_min metres."""

    def __init__(self, smpl, rest=None, geo_min=0.3):
        self._h = None
        self._mask_host = None
        self._mask_dev = {}
        self.vertex_num = smpl.vertex_num
        self.faces = np.ascontiguousarray(smpl._model["face_indices"], np.int64) - 1
        if rest is None:
            rest = smpl._model["vertices_template"]
        if _is_torch(rest):
            rest = rest.detach().cpu().numpy()
        rest = np.ascontiguousarray(rest, np.float32)
        if rest.shape != (self.vertex_num, 3):
            raise SmplppError(1, "SelfContact: expected rest of shape (%d, 3)" % self.vertex_num)
        h = C.c_void_p()
        check(_lib.load().smplpp_self_contact_create(smpl.handle, _ptr(rest), float(geo_min), C.byref(h)))
        self._h = h
        V, W, g, fp = C.c_int64(), C.c_int64(), C.c_float(), C.c_int64()
        check(_lib.load().smplpp_self_contact_info(self._h, C.byref(V), C.byref(W), C.byref(g), C.byref(fp)))
        self.words_per_row, self.geo_min, self.far_pairs = W.value, g.value, fp.value

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_self_contact_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "SelfContact: no handle")
        return self._h

    def mask(self, device=None):
        """The mask [V,W]: bit (u & 31) of word (u >> 5) of row v is far(v, u).  A numpy uint32 array, or with `device` a torch int32
        tensor there holding the same words.  Read once per space and kept: treat it as read-only."""
        if device is None:
            if self._mask_host is None:
                m = np.empty((self.vertex_num, self.words_per_row), np.uint32)
                check(_lib.load().smplpp_self_contact_mask(self.handle, _ptr(m), _lib.HOST, None))
                self._mask_host = m
            return self._mask_host
        key = str(device)
        if key not in self._mask_dev:
            m = torch.empty((self.vertex_num, self.words_per_row), dtype=torch.int32, device=device)
            c = _Call("mask", m)
            check(_lib.load().smplpp_self_contact_mask(self.handle, _ptr(m), c.space, c.stream))
            self._mask_dev[key] = m
        return self._mask_dev[key]

    def filter_pairs(self, pairs):
        """filter_pairs(pairs, the model's faces, this handle's mask): a bool array over the rows of a selfIntersections pair list."""
        return filter_pairs(pairs, self.faces, self.mask(pairs.device) if _is_torch(pairs) else self.mask())

    @staticmethod
    def _cap(max_dist, max_sqdist=None):
        """The squared cap as the fp32 value the call receives: max_sqdist as given, else fp32(max_dist)^2, else +inf."""
        if max_sqdist is not None:
            return float(np.float32(max_sqdist))
        return float("inf") if max_dist is None else float(np.float32(max_dist) * np.float32(max_dist))

    def _search(self, c, verts, vert_normals, cos_min, cap):
        if len(verts.shape) != 3 or verts.shape[0] < 1:
            c.refuse("expected verts of shape (N, V, 3)")
        n, V = int(verts.shape[0]), self.vertex_num
        verts, vn = c.input(verts, (n, V, 3)), c.input(vert_normals, (n, V, 3))
        index, sq = c.empty((n, V), "int64"), c.empty((n, V))
        check(_lib.load().smplpp_self_contact(self.handle, n, _ptr(verts), _ptr(vn), float(cos_min), cap, _ptr(index), _ptr(sq), c.space, c.stream))
        return verts, index, sq

    def search(self, verts, vert_normals=None, cos_min=0.0, max_dist=None, max_sqdist=None):
        """Each vertex's contact partner in each frame of verts [N,V,3] (smplpp_self_contact): (index [N,V] int64, sqdist [N,V],
        matched [N,V] bool).  The partner is the nearest vertex of the same frame that is far along the surface, within max_dist
        metres (None: no cap; max_sqdist gives the squared cap directly) and, with vert_normals [N,V,3] (for instance those of
        SMPL.vertex_normals_differentiable; not necessarily unit), whose normal opposes the vertex's by at least cos_min: touching
        surfaces face each other.  On equal distances the lowest index; a vertex without a partner has (-1, 0, False)."""
        c = _Call("search", verts, vert_normals)
        _, index, sq = self._search(c, verts, vert_normals, cos_min, self._cap(max_dist, max_sqdist))
        return index, sq, index >= 0

    def searchBackward(self, verts, index, grad_sqdist, out=None):
        """Vector-Jacobian product of search's sqdist at the partners `index` [N,V] it chose: grad_verts [N,V,3] for dL/dsqdist =
        grad_sqdist [N,V] (smplpp_self_contact_vjp), to a vertex both as a query and as a partner.  With `out` [N,V,3] the gradient
        is added into it and it is returned.  Unmatched vertices (-1) and zero cotangents contribute nothing."""
        c = _Call("searchBackward", verts, grad_sqdist, out)
        n, V = int(verts.shape[0]), self.vertex_num
        verts = c.input(verts, (n, V, 3))
        idt = c.ids(index)
        if idt.shape[0] != n * V:
            c.refuse("expected index of shape (%d, %d)" % (n, V))
        g = c.input(grad_sqdist, (n, V))
        gv = c.inout(out, (n, V, 3)) if out is not None else c.empty((n, V, 3))
        check(_lib.load().smplpp_self_contact_vjp(self.handle, n, _ptr(verts), _ptr(idt), _ptr(g), _ptr(gv), int(out is not None), c.space,
                                                  c.stream))
        return gv

    def search_differentiable(self, verts, vert_normals=None, cos_min=0.0, max_dist=None, max_sqdist=None):
        """(index [N,V], matched [N,V] bool, sqdist [N,V]) of device vertices (the bits of search), with sqdist differentiable in
        verts through torch.autograd: smplpp_self_contact forward, smplpp_self_contact_vjp backward, on torch's current stream.
        The normals steer the selection only: nothing flows to them."""
        if torch is None:
            raise SmplppError(1, "search_differentiable needs torch")
        return _SelfContactFunction.apply(verts, self, vert_normals, cos_min, self._cap(max_dist, max_sqdist))


if torch is not None:
    class _SelfContactFunction(torch.autograd.Function):
        """smplpp_self_contact forward / smplpp_self_contact_vjp backward (SelfContact.search_differentiable)."""

        @staticmethod
        def forward(ctx, verts, sc, vert_normals, cos_min, cap):
            c = _Call("search_differentiable", verts, vert_normals, device_only=True)
            v, index, sq = sc._search(c, verts, vert_normals, cos_min, cap)
            matched = index >= 0
            ctx.mark_non_differentiable(index, matched)
            ctx.sc = sc
            ctx.save_for_backward(v, index)
            return index, matched, sq

        @staticmethod
        def backward(ctx, _gi, _gm, g_sq):
            v, index = ctx.saved_tensors
            gv = ctx.sc.searchBackward(v, index, g_sq.contiguous()) if ctx.needs_input_grad[0] else None
            return gv, None, None, None, None
