"""The per-vertex bar of the backward passes that hand a gradient to the posed vertices, the queries or a per-vertex attribute, and
the cases it is asserted on (tests/test_vertex_blocks_cpu.py runs the fp32 oracles through them, tests/test_vertex_blocks_gpu.py the
kernels).

A frame's L2 norm runs over up to 6890 three-vectors and has a floor of 1e-5: one vertex can be wrong by 1e-3 of its own size inside
it.  Here every output is cut into the blocks a caller reads as one quantity,

    output                  block
    grad_verts  [n,V,3]     each (frame, vertex) three-vector
    grad_points [n,K,3]     each (frame, query) three-vector
    grad_attr   [n,V,C]     each (frame, vertex) row

and a block is scaled by the ABSOLUTE SUM of what enters it, not by its own size: with c_r the contributions a fixed-order sum
adds into component i of vertex v, A[v,i] = sum_r |c_r[i]| in float64 and scale(v) = max_i A[v,i] (the textbook bound of a sum in
any order; a vertex whose shares nearly cancel is not measured against its luck).  E = max over blocks of max_i |x_i - ref_i| /
scale; a block of scale 0 must be exactly zero (either sign), otherwise E = inf; no block is left out.  E is held to bar(e32) =
max(4 e32, 4 x 2^-24) (stage_oracle.bar), e32 the E of the fp32 evaluation of the same oracle graph on the same case against the same
float64 reference and scales: the maximum over ALL the case's blocks of that output.

The contributions come from the oracles themselves, evaluated on an EXPLODED mesh: every record (a vertex's point, a covered pixel,
a face) gets vertices of its own, copies of its corners, so what the oracle returns per exploded vertex is the record's share of
that corner; the shares are then summed per target in record order (numpy add.at, in the oracle's dtype), |share| beside share.
  point -> mesh, signed    the closed form of point_distance_oracle.closed_form, its shares kept per (query, corner)
  mesh -> point            autograd of mesh_point_distance_oracle.sqdist, one point per vertex record
  depth, interpolation     the closed forms depth_raster_oracle.vjp / raster_interpolate_oracle.vjp, one triangle per live pixel
  silhouette               autograd of silhouette_oracle.loss on [verts; verts[faces]], one triangle per face (the pixel side's
                           shares summed per face) and the vertex side's own share
  normals                  autograd of normals_vjp_oracle.face_normals / vertex_normals on verts[faces], one triangle per face

A yardstick above 64 x 2^-24 makes its bar too weak to mean anything, so the inputs are chosen for the fp32 oracle to stay under
it, each choice written down where it is made with what the plain input measured: the points of the distances stand over
well-shaped faces near the origin, half to one edge away (surface_points); the body's faces are carried on `relaxed_body`, whose
triangles have no slivers; face-normal cotangents keep away from the faces' edges (face_cotangent); the raster cotangents are zero
at grazing faces and on a face's rim (well_conditioned_pixels) and where a silhouette residual is small beside its coordinates
(far_residuals).  The depth and interpolation of the `body` scene of tests/raster_vjp_cases.py cannot be brought under it by any
cotangent (tests/test_vertex_blocks_cpu.py says why): the bar gets the same body from `near` (raster_case), and `body` is held to four
times its own yardstick beside it.

numpy only at import; torch and the oracles are imported inside the helpers."""
import numpy as np

from stage_oracle import EPS32, bar  # noqa: F401  (bar(e32) = max(4 e32, 4 x 2^-24); restated nowhere else)
from vjp_blocks import l2_rel  # noqa: F401  (the old figure, printed beside the new one)

E32_MAX = 64 * EPS32  # a case whose fp32 oracle alone is worse than this has a bar too weak to mean anything: change its inputs
GATHER_T, GATHER_TILE = 256, 1024  # smplpp_amd/csrc/distance_vjp.h: targets per workgroup, records per LDS tile
LIST_LDS_BYTES = 64 * 1024  # smplpp_amd/csrc/mesh_vjp.hip: the list forms' per-frame buffer stays in LDS up to this size


# ------------------------------------------------------------------------------------------------ the figure
def block_errors(x, ref64, scale):
    """x, ref64 [..., B, C], scale [..., B] -> per block max_i |x_i - ref_i| / scale; a block of scale 0 gives 0 if x is exactly zero
    there (either sign of zero) and inf otherwise; a non-finite x gives inf."""
    x, ref64, scale = np.asarray(x, np.float64), np.asarray(ref64, np.float64), np.asarray(scale, np.float64)
    assert x.shape == ref64.shape and scale.shape == x.shape[:-1], (x.shape, ref64.shape, scale.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(x - ref64).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale == 0, np.where(np.abs(x).max(axis=-1) == 0, 0.0, np.inf), err / scale)
    return np.where(np.isfinite(err), e, np.inf)


def figure(x, ref64, scale):
    """(E, index of the worst block)."""
    e = block_errors(x, ref64, scale)
    if e.size == 0:
        return 0.0, ()
    w = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[w]), tuple(int(i) for i in w)


def frame_l2(x, ref64):
    """The existing tests' figure: the largest per-frame ||x - ref|| / ||ref||."""
    return max(l2_rel(a, b) for a, b in zip(x, ref64))


def l2_bar_accepts(x, ref64, x32):
    """The existing tests' rule (_check_vjp / _check_frames): every frame within max(4 x fp32's L2 error, 1e-5)."""
    return all(l2_rel(a, b) <= max(4 * l2_rel(c, b), 1e-5) for a, b, c in zip(x, ref64, x32))


def scatter(contrib, target, ntarget):
    """contrib [R,C] summed per target [R] (-1: none) in record order, in contrib's dtype: (sum [ntarget,C], sum of |.|)."""
    contrib = np.asarray(contrib)
    target = np.asarray(target, np.int64)
    keep = target >= 0
    out = np.zeros((ntarget, contrib.shape[1]), contrib.dtype)
    A = np.zeros_like(out)
    np.add.at(out, target[keep], contrib[keep])
    np.add.at(A, target[keep], np.abs(contrib[keep]))
    return out, A


def _stack(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def signed_sum_matches(ref, A, oracle, tol=1e-12):
    """The summed shares reproduce an existing float64 oracle: |ref - oracle| <= tol x A element by element."""
    return bool((np.abs(np.asarray(ref, np.float64) - np.asarray(oracle, np.float64)) <= tol * A).all())


# ------------------------------------------------------------------------------------------------ references
# Every reference returns {output: (value [n,B,C], A [n,B,C])} in `dtype` ("float64": the reference and its scales; "float32": the
# yardstick, whose A is not used).
def point_mesh_reference(verts, faces, points, face, grad, dtype="float64", inside=None):
    """pointMeshDistanceBackward (inside None) / pointMeshSignedDistanceBackward at the given faces, by the closed form
    (point_distance_oracle.closed_form: grad_points = 2 g r, corner j of the query's face receives -2 g w_j r, with g negated
    where `inside`); a query of face -1 (unmatched) contributes nothing.  fp32 autograd through the region's parameters is no
    yardstick here: its envelope terms cancel only analytically."""
    import point_distance_oracle as PO

    torch = PO.torch
    dt = getattr(torch, dtype)
    face = np.asarray(face, np.int64)
    n, K = face.shape
    live = face >= 0
    corner = np.asarray(faces, np.int64)[np.where(live, face, 0)]  # [n,K,3]
    g = np.where(live, np.asarray(grad, np.float64), 0.0) * (1.0 if inside is None else 1.0 - 2.0 * np.asarray(inside))
    with torch.no_grad():
        tri = torch.tensor(np.asarray(verts, np.float64)[np.arange(n)[:, None, None], corner], dtype=dt)  # [n,K,3,3]
        p, g = torch.tensor(np.asarray(points, np.float64), dtype=dt), torch.tensor(g, dtype=dt)
        cp, w = PO.closest(p, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])
        r = p - cp
        gp = (2 * g[..., None] * r).numpy()
        c = (-2 * g[..., None, None] * w[..., None] * r[:, :, None, :]).reshape(n, 3 * K, 3).numpy()
    target = np.where(live[..., None], corner, -1).reshape(n, 3 * K)
    return {"verts": _stack([scatter(c[f], target[f], verts.shape[1]) for f in range(n)]), "points": (gp, np.abs(gp))}


def mesh_point_reference(verts, points, index, grad, dtype="float64"):
    """meshPointDistanceBackward at the given indices (-1: no point).  One exploded point per vertex record."""
    import mesh_point_distance_oracle as MO

    torch = MO.torch
    dt = getattr(torch, dtype)
    index = np.asarray(index, np.int64)
    n, V = index.shape
    K = points.shape[1]
    valid = index >= 0
    px = np.asarray(points, np.float64)[np.arange(n)[:, None], np.where(valid, index, 0)]
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dt, requires_grad=True)
    p = torch.tensor(px, dtype=dt, requires_grad=True)
    d = MO.sqdist(v, p, np.where(valid, np.arange(V)[None], -1))
    gv, c = torch.autograd.grad((d * torch.tensor(np.asarray(grad, np.float64), dtype=dt)).sum(), (v, p))
    gv, c = gv.numpy(), c.numpy()
    return {"verts": (gv, np.abs(gv)), "points": _stack([scatter(c[f], index[f], K) for f in range(n)])}


def explode_pixels(faces, face_img, live):
    """The live pixels of one frame, each given a triangle of its own: (corner [P,3] vertex ids, faces [P,3] of the exploded mesh,
    its face image [H,W])."""
    fi = np.asarray(face_img, np.int64)
    p = np.nonzero(np.asarray(live).reshape(-1))[0]
    corner = np.asarray(faces, np.int64)[fi.reshape(-1)[p]]
    img = np.full(fi.size, -1, np.int64)
    img[p] = np.arange(len(p))
    return corner, np.arange(3 * len(p)).reshape(len(p), 3), img.reshape(fi.shape)


def depth_reference(verts, faces, cams, face, grad_depth, dtype="float64"):
    """depthRasterBackward: depth_raster_oracle.vjp with one exploded triangle per covered pixel of nonzero cotangent."""
    import depth_raster_oracle as DR

    dt = np.dtype(dtype).type
    out = []
    for f in range(len(verts)):
        fi = np.asarray(face[f], np.int64)
        corner, fx, img = explode_pixels(faces, fi, (fi >= 0) & (fi < len(faces)) & (grad_depth[f] != 0))
        with np.errstate(all="ignore"):
            c = DR.vjp(verts[f][corner.reshape(-1)], fx, cams[f], img, grad_depth[f], dt) if len(fx) else np.zeros((0, 3), dt)
        out.append(scatter(c, corner.reshape(-1), verts.shape[1]))
    return {"verts": _stack(out)}


def interpolate_reference(attr, verts, faces, cams, face, grad_image, dtype="float64"):
    """rasterInterpolateBackward: raster_interpolate_oracle.vjp with one exploded triangle per pixel with a nonzero cotangent."""
    import raster_interpolate_oracle as RI

    dt = np.dtype(dtype).type
    oa, ov = [], []
    for f in range(len(verts)):
        corner, fx, img = explode_pixels(faces, face[f], RI._live(face[f], grad_image[f], len(faces)) >= 0)
        t = corner.reshape(-1)
        if len(fx):
            with np.errstate(all="ignore"):
                ca, cv = RI.vjp(attr[f][t], verts[f][t], fx, cams[f], img, grad_image[f], dt)
        else:
            ca, cv = np.zeros((0, attr.shape[2]), dt), np.zeros((0, 3), dt)
        oa.append(scatter(ca, t, verts.shape[1]))
        ov.append(scatter(cv, t, verts.shape[1]))
    return {"attr": _stack(oa), "verts": _stack(ov)}


def silhouette_reference(verts, faces, cams, H, W, face, vert_target, pix_source, grad_vert_sq, grad_pix_sq, dtype="float64"):
    """silhouetteBackward: autograd of silhouette_oracle.loss on [verts; verts[faces]]: the vertex side's share stays on the vertex,
    the pixel side's shares arrive per (face, corner)."""
    import silhouette_oracle as SO

    torch = SO.torch
    dt = getattr(torch, dtype)
    faces = np.asarray(faces, np.int64)
    V, F = verts.shape[1], len(faces)
    fx = V + np.arange(3 * F).reshape(F, 3)
    out = []
    for f in range(len(verts)):
        vx = np.concatenate([verts[f], verts[f][faces.reshape(-1)]]).astype(np.float64)
        leaf = torch.tensor(vx, dtype=dt, requires_grad=True)
        loss = SO.loss(leaf, fx, cams[f], H, W, face[f], vert_target[f], pix_source[f], grad_vert_sq[f], grad_pix_sq[f])
        c = torch.autograd.grad(loss, leaf)[0].numpy() if loss.requires_grad else np.zeros(vx.shape, np.dtype(dtype))
        s, A = scatter(c[V:], faces.reshape(-1), V)
        out.append((c[:V] + s, np.abs(c[:V]) + A))
    return {"verts": _stack(out)}


class ExplodedMesh:
    """normals_vjp_oracle.Mesh with every face on three vertices of its own (the rows of verts[faces]) and the adjacency of the
    original mesh: face_normals / vertex_normals of verts[:, faces].reshape(n, 3F, 3) are those of verts on the mesh itself."""

    def __init__(self, mesh):
        F = len(mesh.faces)
        self.faces = mesh.faces.new_tensor(np.arange(3 * F).reshape(F, 3))
        self.V, self.adj, self.deg, self.mask = mesh.V, mesh.adj, mesh.deg, mesh.mask


def normals_fn(mesh, kind, ids):
    """tests/test_normals_vjp_gpu.py::_fn."""
    import normals_vjp_oracle as NO

    if kind == "face":
        return lambda x: NO.face_normals(mesh, x, ids)
    if kind == "vertex":
        return lambda x: NO.vertex_normals(mesh, x, ids)
    return lambda x: NO.vertex_normals(mesh, x)


def normals_reference(mesh, kind, ids, verts, grad, dtype="float64"):
    """calcNormalBackward ("face"), calcVertexNormalBackward ("vertex"), calcMeshVertexNormalsBackward ("mesh"): the shares per
    (face, corner) by autograd on verts[faces]."""
    import normals_vjp_oracle as NO

    faces = mesh.faces.numpy()
    n, V = verts.shape[:2]
    vx = np.asarray(verts, np.float64)[:, faces.reshape(-1)]
    c = NO.vjp(normals_fn(ExplodedMesh(mesh), kind, ids), vx, grad, getattr(NO.torch, dtype))
    return {"verts": _stack([scatter(c[f], faces.reshape(-1), V) for f in range(n)])}


# ------------------------------------------------------------------------------------------------ meshes
MESHES = ("ico", "body", "fan")
FAN_HUB, FAN_VALENCE, FAN_V = 256, 16, 257
_meshes = {}


def fan_faces():
    """257 vertices: 16 rings of 16 (ids 16 r + i) joined by strips, closed in the middle by a fan of 16 faces about the hub, vertex
    256: the first target of the record gather's second workgroup, of valence 16."""
    R = FAN_VALENCE
    f = [(FAN_HUB, i, (i + 1) % R) for i in range(R)]
    for r in range(FAN_V // R - 1):
        for i in range(R):
            a, b, c, d = r * R + i, r * R + (i + 1) % R, (r + 1) * R + i, (r + 1) * R + (i + 1) % R
            f += [(a, c, d), (a, d, b)]
    return np.array(f, np.int64)


def _fan_template():
    """Log-polar rings (radius 1 cm x 1.35^r, every other ring turned half a step) on a shallow bowl about the hub at the origin:
    the strips' faces keep one shape at every size, and a face's distance from the origin stays a few of its edges."""
    R = FAN_VALENCE
    r, i = np.divmod(np.arange(FAN_V - 1), R)
    rad, ang = 0.01 * 1.35 ** r, 2 * np.pi * (i + 0.5 * (r % 2)) / R
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.3 * rad ** 2 + 0.05 * rad * np.cos(3 * ang)], 1)
    return np.concatenate([ring, [[0.0, 0.0, -0.002]]])


def mesh(which):
    """dict(model, faces [F,3] 0-based, V, oracle mesh, valence [V]) of one of MESHES (built once; never modified): the icosphere of
    642 = 2 x 256 + 130 vertices, the synthetic body's faces (V = 6890, valences 5 to 7; its vertices are `relaxed_body`), the fan."""
    import normals_vjp_oracle as NO
    from smplpp_amd import model_io

    if which not in _meshes:
        if which == "body":
            md = model_io.synthetic_model()
            faces = np.asarray(md["face_indices"], np.int64) - 1
        else:
            import self_penetration_oracle as SP

            faces = SP.icosphere(3)[1] if which == "ico" else fan_faces()
            md = model_io.tiny_model(int(faces.max()) + 1, seed=3, faces=faces + 1)  # test_depth_raster_gpu._model_for's model
        V = md["vertices_template"].shape[0]
        om = NO.Mesh(faces, V)
        _meshes[which] = dict(name=which, model=md, faces=faces, V=V, oracle=om, valence=om.deg.numpy())
    return _meshes[which]


def relaxed_body():
    """The body's 6890 vertices moved to where its 13776 faces are well shaped (float64 [V,3], built once): on the sphere of radius
    0.5 m, 1000 sweeps of "each vertex to the mean of its neighbours, back onto the sphere".  The posed body has faces whose 2 area /
    (longest edge)^2 is below 0.01; the gradient of such a face's unit normal is wrong by hundreds of 2^-24 in any fp32 evaluation
    (measured: the whole-mesh yardstick is 170 to 400 x 2^-24 there), and the largest share at its corners is that face's."""
    if "relaxed" not in _meshes:
        F, V = mesh("body")["faces"], mesh("body")["V"]
        i = np.concatenate([F[:, 0], F[:, 1], F[:, 2], F[:, 1], F[:, 2], F[:, 0]])
        j = np.concatenate([F[:, 1], F[:, 2], F[:, 0], F[:, 0], F[:, 1], F[:, 2]])
        deg = np.bincount(i, minlength=V).astype(np.float64)
        v = np.asarray(mesh("body")["model"]["vertices_template"], np.float64)
        v = v - v.mean(0)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        for _ in range(1000):
            v = 0.5 * v + 0.5 * np.stack([np.bincount(i, weights=v[j, k], minlength=V) for k in range(3)], 1) / deg[:, None]
            v /= np.linalg.norm(v, axis=1, keepdims=True)
        _meshes["relaxed"] = 0.5 * v
    return _meshes["relaxed"]


def mesh_verts(which, n, seed):
    """n frames of fp32 vertices [n,V,3]: the icosphere (radius 0.5) with N(0, 5 mm) on every vertex, `relaxed_body` with N(0, 1 mm),
    the fan with N(0, 2 % of its distance from the hub)."""
    rng = np.random.default_rng(seed)
    if which == "fan":
        vt = _fan_template()
        return (vt[None] + 0.02 * np.linalg.norm(vt, axis=1)[None, :, None] * rng.normal(0, 1, (n,) + vt.shape)).astype(np.float32)
    if which == "ico":
        import self_penetration_oracle as SP

        vt = SP.icosphere(3, radius=0.5)[0]
    else:
        vt = relaxed_body()
    return (vt[None] + rng.normal(0, 0.005 if which == "ico" else 0.001, (n,) + vt.shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ a. record gather
GATHER_K = [1, GATHER_TILE - 1, GATHER_TILE, GATHER_TILE + 1, 2 * GATHER_TILE + 1]
POINT_K = [GATHER_T - 1, GATHER_T, GATHER_T + 1]  # mesh -> point: the targets are the points
LAYOUTS = ("generic", "oneface", "silent")


QMIN, RMAX, WMIN, HMIN = 0.35, 8.0, 0.2, 0.5


def well_conditioned_faces(v, faces):
    """The faces of one frame on which the fp32 closed form is well conditioned, and every face's shortest edge: shape 2 area /
    (longest edge)^2 >= QMIN (no sliver: the weights' error grows with the inverse), centroid within RMAX shortest edges of the
    origin (the residual p - closest is a difference of coordinates: its error is 2^-24 of them, not of itself)."""
    t = np.asarray(v, np.float64)[faces]
    e = np.stack([np.linalg.norm(t[:, (i + 1) % 3] - t[:, i], axis=1) for i in range(3)], 1)
    area2 = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    ok = (area2 >= QMIN * e.max(1) ** 2) & (np.linalg.norm(t.mean(1), axis=1) <= RMAX * e.min(1))
    return np.nonzero(ok)[0], e.min(1)


def surface_points(v, faces, K, rng, one_face=False):
    """K points per frame over the well-conditioned faces (all K over one of them with one_face), each above or below a point of
    its face whose weights are at least WMIN, by HMIN to 1 of the face's shortest edge along the normal: (points [n,K,3] fp32, face
    [n,K] where each was sampled, inside [n,K] = moved against the normal).  Points nearer the surface, over slivers or far from
    the origin make the fp32 oracle itself wrong by hundreds to millions of 2^-24 (measured), and the bar with it."""
    import closest_ref as cr

    n = len(v)
    P, fid, inside = np.empty((n, K, 3), np.float32), np.empty((n, K), np.int64), np.empty((n, K), bool)
    for f in range(n):
        ok, emin = well_conditioned_faces(v[f], faces)
        assert len(ok) >= 16, len(ok)
        fid[f] = ok[rng.integers(0, len(ok), 1 if one_face else K)]
        w = WMIN + (1 - 3 * WMIN) * rng.dirichlet(np.ones(3), K)
        h = rng.uniform(HMIN, 1.0, (K, 1)) * emin[fid[f]][:, None] * rng.choice([-1.0, 1.0], (K, 1))
        tri = v[f].astype(np.float64)[faces[fid[f]]]
        P[f] = (np.einsum("ki,kix->kx", w, tri) + h * cr.face_normals(v[f], faces)[fid[f]]).astype(np.float32)
        inside[f] = h[:, 0] < 0
    return P, fid, inside


def gather_case(which, K, layout="generic", n=2):
    """dict(name, mesh, verts, points, face, inside, grad [n,K], grad_mp [n,V]): the body moved so that the origin lies on it; `face` and
    `inside` are where the points were sampled (the GPU tests replace them by the forward call's own).  Layouts: generic; every
    query on one face (a tile's records all hit the same three targets); frame 1 with a zero cotangent on every third query /
    vertex."""
    assert layout in LAYOUTS
    m = mesh(which)
    seed = 7919 * MESHES.index(which) + 13 * K + LAYOUTS.index(layout)
    v = mesh_verts(which, n, seed)
    if which == "body":  # (the faces within RMAX of their edges of the origin are the well-conditioned ones: a cap of about 350)
        v = v + np.float32(0.5) * (v[:, :1] / np.linalg.norm(v[:, :1], axis=-1, keepdims=True))
    rng = np.random.default_rng(seed + 1)
    P, face, inside = surface_points(v, m["faces"], K, rng, one_face=layout == "oneface")
    g = rng.normal(size=(n, K)).astype(np.float32)
    gm = rng.normal(size=(n, m["V"])).astype(np.float32)
    if layout == "silent":
        g[1, ::3] = 0
        gm[1, ::3] = 0
    return dict(name="%s K=%d %s" % (which, K, layout), mesh=which, verts=v, points=P, face=face, inside=inside, grad=g, grad_mp=gm)


def compatible_case(which="body", K=GATHER_TILE + 1, n=2):
    """The generic case with the sampled faces' normals as query normals, a third of them reversed and a tenth zero: unmatched
    queries (face -1) among K = 1025 records, under a cap of 5 cm (the points lie within an edge, about 2 cm, of their faces)."""
    import closest_ref as cr

    c = gather_case(which, K, n=n)
    m = mesh(which)
    rng = np.random.default_rng(K)
    N = np.stack([cr.face_normals(c["verts"][f], m["faces"])[c["face"][f]] for f in range(n)]).astype(np.float32)
    r = rng.random((n, K))
    N[r < 1 / 3] *= -1
    N[r > 0.9] = 0
    c.update(name="%s K=%d compatible" % (which, K), normals=N, matched=(r >= 1 / 3) & (r <= 0.9), max_dist=0.05)
    return c


# ------------------------------------------------------------------------------------------------ c. normal queries
def face_cotangent(v, faces, ids, rng):
    """A cotangent [n,count,3] of face normals whose shares do not cancel inside themselves.  A corner's share is (its opposite edge)
    x (the cotangent's part in the face's plane) / |N|: it vanishes where the two are parallel, and a random cotangent among 300
    comes within a degree of that.  So the in-plane part, +-(1 to 2) long, lies along that bisector of two edge directions which
    keeps the largest angle to all three edges; U(-1, 1) along the normal is added; a repeated id gets its first cotangent times
    0.5 to 1.5 (two cotangents on one face are one, their sum)."""
    t = np.asarray(v, np.float64)[:, faces[ids]]  # [n,count,3,3]
    n, count = t.shape[:2]
    e = np.stack([t[:, :, (i + 2) % 3] - t[:, :, (i + 1) % 3] for i in range(3)], 2)
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    cand = np.stack([e[:, :, i] + sg * e[:, :, j] for i, j in ((0, 1), (1, 2), (2, 0)) for sg in (1.0, -1.0)], 2)  # [n,count,6,3]
    cand /= np.linalg.norm(cand, axis=-1, keepdims=True)
    sine = np.linalg.norm(np.cross(cand[:, :, :, None], e[:, :, None]), axis=-1).min(-1)  # [n,count,6]
    d = np.take_along_axis(cand, sine.argmax(-1)[..., None, None], 2)[:, :, 0]
    nrm = np.cross(e[:, :, 0], e[:, :, 1])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    g = rng.uniform(1, 2, (n, count, 1)) * rng.choice([-1.0, 1.0], (n, count, 1)) * d + rng.uniform(-1, 1, (n, count, 1)) * nrm
    first = {}
    for k, f in enumerate(np.asarray(ids).tolist()):
        if f in first:
            g[:, k] = g[:, first[f]] * rng.uniform(0.5, 1.5, (n, 1))
        first.setdefault(f, k)
    return g.astype(np.float32)


def normals_case(which, kind, n, ids=None, seed=0):
    """Posed vertices and a cotangent [n,rows,3] for one of the normal queries: "mesh", "vertex" with `ids` (N(0,1)) or "face" with
    `ids` (face_cotangent)."""
    m = mesh(which)
    s = 1000 * MESHES.index(which) + 10 * n + seed
    v = mesh_verts(which, n, s)
    rng = np.random.default_rng(s + 1)
    rows = m["V"] if kind == "mesh" else len(ids)
    g = face_cotangent(v, m["faces"], ids, rng) if kind == "face" else rng.standard_normal((n, rows, 3)).astype(np.float32)
    name = "%s %s n=%d%s" % (which, kind, n, "" if ids is None else " ids=%d" % len(ids))
    return dict(name=name, mesh=which, kind=kind, ids=ids, verts=v, grad=g)


def vertex_ids(which, count, seed=1):
    """`count` vertex ids; with count = 200 repeats are allowed, and the highest-valence vertex is always among them."""
    m = mesh(which)
    ids = np.random.default_rng(seed + count).integers(0, m["V"], count).astype(np.int64)
    ids[0] = int(np.argmax(m["valence"]))
    if count > 5:
        ids[5] = ids[2]
    return ids


def face_ids(which, count=300, seed=2):
    """`count` face ids with repeats and two faces that share an edge."""
    m = mesh(which)
    F = m["faces"]
    ids = np.random.default_rng(seed + count).integers(0, len(F), count).astype(np.int64)
    ids[7] = ids[3]
    ids[count - 1] = ids[0]
    a = set(F[ids[1]][:2].tolist())  # a neighbour of face ids[1] across its first edge
    ids[2] = next(f for f in range(len(F)) if f != ids[1] and a <= set(F[f].tolist()))
    return ids


def normals_cases(which):
    """The cases of one mesh, n in {1, 3}: the whole mesh; on the body vertex lists of 5 and of 200 ids and a face list of 300; on
    the fan the hub (twice) among four vertices, and five faces about it.  (The 200-id list at n = 3 has the seed 4: about one
    seed in three puts a random cotangent where the only two shares of some ring vertex nearly vanish inside themselves, and the fp32
    oracle is then wrong by 100 to 160 x 2^-24 there.)"""
    for n in (1, 3):
        yield normals_case(which, "mesh", n)
    if which == "body":
        yield normals_case(which, "vertex", 3, vertex_ids(which, 5))
        yield normals_case(which, "vertex", 1, vertex_ids(which, 200))
        yield normals_case(which, "vertex", 3, vertex_ids(which, 200), seed=4)
        yield normals_case(which, "face", 1, face_ids(which))
        yield normals_case(which, "face", 3, face_ids(which))
    if which == "fan":
        yield normals_case(which, "vertex", 3, np.array([FAN_HUB, 0, FAN_HUB, 17], np.int64))
        yield normals_case(which, "face", 3, np.array([0, 1, 15, 40, 0], np.int64))


def list_buffer_bytes(count, maxdeg, vertex):
    """mesh_vjp.hip::list_vjp_device restated: the per-frame buffer of a list form; above LIST_LDS_BYTES list_vjp_ws_kernel runs."""
    P = count * maxdeg if vertex else count
    return 4 * ((3 * count if vertex else 0) + 6 * P + 2 * 3 * P)


# ------------------------------------------------------------------------------------------------ b. raster walk and gather
class OracleHandle:
    """What raster_vjp_cases.scene / inputs ask of an SMPL handle, answered without a GPU: launch by the C oracle's FK, depthRaster
    and silhouette by the numpy restatements of their rules."""

    def __init__(self, model):
        self.model = model
        self.faces = np.asarray(model["face_indices"], np.int64) - 1

    def launch(self, beta, theta, want=("verts",)):
        from oracle import cpu

        return {"verts": np.ascontiguousarray(cpu.OracleModel(self.model).fk(beta, theta)["verts"], np.float32)}

    def depthRaster(self, verts, cams, H, W):
        import depth_raster_oracle as DR

        return DR.raster_batch(verts, self.faces, cams, H, W)

    def silhouette(self, verts, cams, H, W, mask, face=None, want=()):
        import silhouette_oracle as SO

        return SO.silhouette_batch(verts, cams, H, W, face, mask)


RASTER_C = (1, 5)  # of raster_vjp_cases.CHANNELS: one walk of one channel; a chunk of 4 and a chunk of 1
RASTER_SCENES = ("hand", "spheres", "near", "body")
COS_MIN, BETA_MIN = 0.3, 0.05
AMP_MAX = 40.0
NEAR_F, NEAR_D = 0.2, 0.25
NEAR_VIEWS = (((0.0, 0.0, 0.0), 0.1), ((0.1, 0.3, 0.0), 0.3), ((-0.1, -0.3, 0.0), -0.3))  # (offset from the body's centre, yaw)
SHIFT = {"hand": 2, "spheres": 24, "near": 24}  # the target mask: the scene's coverage moved this many pixels to the right
RES_DIV = 8.0


def well_conditioned_pixels(verts, faces, cams, face, amp_max=None):
    """bool [n,H,W]: the covered pixels whose ray meets its face's plane at cos >= COS_MIN and inside the face by BETA_MIN (float64).
    At a grazing face 1 / (n.d), and at a pixel on a face's rim the smallest barycentric, is wrong by 10^3 to 10^6 x 2^-24 of
    itself in any fp32 evaluation (measured on `spheres` and `body`); the cotangents are zero elsewhere.

    With amp_max also: the face is no sliver (2 area / longest edge^2 >= QMIN) and
        (farthest corner from the camera / shortest edge) / cos / smallest barycentric <= amp_max.
    A barycentric is a difference of camera-space coordinates divided by an edge, through a depth that carries 1 / cos: the
    product is the factor by which a share's fp32 error exceeds 2^-24 (measured on `near`: a share at 170 is wrong by 280 x
    2^-24, the worst block at amp_max 30 / 45 / 60 by 27 / 40 / 81)."""
    import depth_raster_oracle as DR

    n, H, W = face.shape
    ok = np.zeros(face.shape, bool)
    for f in range(n):
        fi = np.asarray(face[f], np.int64).reshape(-1)
        p = np.nonzero((fi >= 0) & (fi < len(faces)))[0]
        if len(p) == 0:
            continue
        c = np.asarray(cams[f], np.float64)
        tri = faces[fi[p]]
        with np.errstate(all="ignore"):
            a, b, cc = (np.asarray(verts[f], np.float64)[tri[:, e]] @ c[:9].reshape(3, 3).T + c[9:12] for e in range(3))
            d = DR._ray(p % W, p // W, c, np.float64)
            _, beta = DR._hit(a, b, cc, d)
            nrm = DR._cross(b - a, cc - a)
            cos = np.abs(DR._dot(nrm, d)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
            good = (cos >= COS_MIN) & (beta.min(1) >= BETA_MIN)
            if amp_max is not None:
                e = np.stack([np.linalg.norm(b - a, axis=1), np.linalg.norm(cc - b, axis=1), np.linalg.norm(a - cc, axis=1)], 1)
                far = np.stack([np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(cc, axis=1)], 1).max(1)
                good &= (np.linalg.norm(nrm, axis=1) >= QMIN * e.max(1) ** 2) & (far / e.min(1) / cos / beta.min(1) <= amp_max)
        ok.reshape(n, -1)[f, p] = good
    return ok


def silhouette_inputs(s, x, H, W, shift, seed):
    """raster_vjp_cases.inputs()'s silhouette arrays for a scene it builds none for: the coverage moved `shift` pixels to the right
    as the target mask, the handle's correspondences, seeded cotangents."""
    import raster_vjp_cases as RC

    face = x["face"]
    n, V = x["verts"].shape[:2]
    mask = np.zeros((n, H, W), np.uint8)
    mask[:, :, shift:] = face[:, :, :-shift] >= 0
    sil = s.silhouette(x["verts"], x["camera"], H, W, mask, face=face, want=("vert_target", "pix_source"))
    rng = np.random.default_rng(seed + 2)
    return dict(mask=mask, vert_target=sil["vert_target"], pix_source=sil["pix_source"],
                grad_vert_sq=rng.normal(size=(n, V)).astype(np.float32), grad_pix_sq=RC._cotangent(rng, (n, H, W)))


def raster_case(name, on_gpu):
    """(handle, faces [F,3], H, W, inputs) of one of RASTER_SCENES: `hand`, `spheres` and `body` of tests/raster_vjp_cases.py, and
    `near`, the posed body of `body` from NEAR_D m off its centre through a lens of focal length NEAR_F H (135 degrees): faces a few
    pixels wide a few of their edges from the camera, which is where an fp32 evaluation of the barycentrics is conditioned.  The
    inputs are raster_vjp_cases.inputs()'s (silhouette_inputs where it has none), with the pixel cotangents set to zero outside
    `well_conditioned_pixels` (not on `hand`: focal length 1, every ray but the middle ones grazing, and a yardstick of 8 x 2^-24
    as it is) and a silhouette pixel's where its source pixel is outside.  Without a GPU the scene's handles are OracleHandles for
    the length of the call (raster_vjp_cases.scene() takes no handle factory, so its two module names are set and put back)."""
    import depth_raster_oracle as DR
    import raster_vjp_cases as RC
    from smplpp_amd import model_io

    base = "body" if name == "near" else name
    saved = RC._model_for, RC._synth
    if not on_gpu:
        RC._model_for = lambda nverts, faces: OracleHandle(model_io.tiny_model(nverts, seed=3, faces=np.asarray(faces) + 1))
        RC._synth = OracleHandle
    try:
        s, v, cams, H, W = RC.scene(base, model_io.synthetic_model())
        if name == "near":
            cams = np.stack([DR.look_at_camera((u.min(0) + u.max(0)) / 2 + np.array(off), NEAR_D, yaw, H, W, f=NEAR_F)
                             for u, (off, yaw) in zip(v, NEAR_VIEWS)])
        x = dict(RC.inputs(base, s, v, cams, H, W))
        if name in SHIFT:
            x.update(silhouette_inputs(s, x, H, W, SHIFT[name], 1000 * (1 + RC.NAMES.index(base))))
    finally:
        RC._model_for, RC._synth = saved
    faces = s.getFaceIndex().astype(np.int64) - 1 if on_gpu else s.faces
    if name == "hand":
        return s, faces, H, W, x
    ok = well_conditioned_pixels(x["verts"], faces, x["camera"], x["face"], AMP_MAX if name == "near" else None)
    x["grad_depth"] = np.where(ok, x["grad_depth"], np.float32(0))
    for C in RASTER_C:
        x["grad_image_%d" % C] = np.where(ok[..., None], x["grad_image_%d" % C], np.float32(0))
    src = x["pix_source"]
    src_ok = np.take_along_axis(ok.reshape(len(ok), -1), np.maximum(src, 0).reshape(len(ok), -1), 1).reshape(src.shape)
    vert_far, pix_far = far_residuals(x, H, W)
    x["grad_pix_sq"] = np.where((src >= 0) & src_ok & pix_far, x["grad_pix_sq"], np.float32(0))
    x["grad_vert_sq"] = np.where(vert_far, x["grad_vert_sq"], np.float32(0))
    return s, faces, H, W, x


def far_residuals(x, H, W):
    """(bool [n,V], bool [n,H,W]): the silhouette residuals at least 1 / RES_DIV of the image coordinates they are the difference of.
    A projection at 100 px that lies 1 px from its target's centre has a residual wrong by 100 x 2^-24 of itself in fp32 (measured
    without this: 134 to 330 x 2^-24 on the vertex side of `spheres` and `near`); those cotangents are zero."""
    import silhouette_oracle as SO

    vt, src = x["vert_target"], x["pix_source"]
    vert_far = np.zeros(vt.shape, bool)
    for f in range(len(vt)):
        with np.errstate(all="ignore"):
            u, v, _ = SO.project(x["verts"][f], x["camera"][f], 0.05, dtype=np.float64)
            cu, cv = vt[f] % W + 0.5, vt[f] // W + 0.5
            vert_far[f] = (vt[f] >= 0) & (np.hypot(u - cu, v - cv) * RES_DIV >= np.maximum(np.abs(u), np.abs(v)))
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    su, sv = src % W + 0.5, src // W + 0.5
    pix_far = (src >= 0) & (np.hypot(su - i[None], sv - j[None]) * RES_DIV >= np.maximum(np.maximum(su, sv), np.maximum(i, j)[None]))
    return vert_far, pix_far


# ---- the silhouette's pixel side: an open patch that faces the camera
PATCH_G, PATCH_F, PATCH_CELL, PATCH_GAP, PATCH_COPIES, PATCH_BETA_MIN = 17, 12.0, 3, 14, 3, 0.1


def patch_faces(G=PATCH_G):
    """A G x G grid of vertices (id = row G + column), two faces per cell, the diagonals alternating."""
    f = []
    for r in range(G - 1):
        for c in range(G - 1):
            a, b, d, e = r * G + c, r * G + c + 1, (r + 1) * G + c, (r + 1) * G + c + 1
            f += [(a, e, b), (a, d, e)] if (r + c) % 2 == 0 else [(a, d, b), (b, d, e)]
    return np.array(f, np.int64)


def patch_case(make_handle, n=2, seed=0):
    """(handle, faces, H, W, inputs) of the case that holds silhouetteBackward's pixel side: its records (one per mask pixel outside
    the coverage, compacted per 256 pixels with a prefix over the frame) and their gather.  On a closed surface a record's source
    pixel, the nearest covered one, lies on the coverage's rim, where every face is grazing; here the mesh is an open sheet of 17 x
    17 vertices (289: two target workgroups, the right column's ids 16, 33, ... in both) one unit in front of a camera at the origin
    (R = 1, t = 0), cells 3 pixels wide through a focal length of 12, its right rim on the optical axis, and the mask is the coverage
    moved right three times, from 14 pixels off the rim on: 5200 mask pixels a frame on about 25 source pixels each row's own,
    2800 to 3100 of them live (three 1024-record tiles), every residual at least an eighth of its coordinates.  The cotangents are
    |N(0,1)| with one in seven zero: the shares of one face then add (a residual points from the mask to the rim), so the
    reference's absolute sum per (face, corner) is the sum over its records; with both signs the shares of a face's two sources cancel
    inside the face and the scale falls short (measured: yardsticks of 100 to 370 x 2^-24 in half the seeds).  A source pixel is
    live where its smallest barycentric is at least PATCH_BETA_MIN and cos >= COS_MIN.  Seed 0 measures 19 x 2^-24; seeds 0 to 7 give 18 to
    70 (an inner vertex whose only source has a barycentric of 0.1).  `make_handle(nverts, faces)` gives the handle
    (test_depth_raster_gpu._model_for, or an OracleHandle)."""
    import depth_raster_oracle as DR

    G, f = PATCH_G, PATCH_F
    faces = patch_faces(G)
    rng = np.random.default_rng(seed)
    cell = PATCH_CELL / f
    wpx = (G - 1) * PATCH_CELL
    H, W = wpx + 8, 4 + wpx + PATCH_GAP + PATCH_COPIES * wpx + 4
    rc = np.stack(np.meshgrid(np.arange(G), np.arange(G), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    xy = np.c_[(rc[:, 1] - (G - 1)) * cell, (rc[:, 0] - (G - 1) / 2) * cell]
    v = np.stack([np.c_[xy + rng.normal(0, 0.05 * cell, xy.shape),
                        1.0 + 0.05 * cell * G * ((xy / (G * cell)) ** 2).sum(1) + rng.normal(0, 0.05 * cell, len(xy))] for _ in range(n)])
    v = v.astype(np.float32)
    cams = np.stack([DR.pinhole(np.eye(3), np.zeros(3), f, f, 4 + wpx, H / 2)] * n)
    s = make_handle(G * G, faces)
    face = s.depthRaster(v, cams, H, W)["face"]
    mask = np.zeros((n, H, W), np.uint8)
    for k in range(PATCH_COPIES):
        shift = wpx + PATCH_GAP + k * wpx
        mask[:, :, shift:] |= (face[:, :, :-shift] >= 0).astype(np.uint8)
    sil = s.silhouette(v, cams, H, W, mask, face=face, want=("vert_target", "pix_source"))
    x = dict(verts=v, camera=cams, face=face, mask=mask, vert_target=sil["vert_target"], pix_source=sil["pix_source"])
    rng = np.random.default_rng(seed + 2)
    gp = np.abs(rng.normal(size=(n, H, W))).astype(np.float32)
    gp[rng.random((n, H, W)) < 1.0 / 7.0] = 0
    x["grad_vert_sq"] = np.zeros((n, G * G), np.float32)  # the pixel side alone: a vertex's own share would only widen its scale
    x["base_verts"] = rng.normal(size=v.shape).astype(np.float32)
    global BETA_MIN
    saved, BETA_MIN = BETA_MIN, PATCH_BETA_MIN
    try:
        ok = well_conditioned_pixels(v, faces, cams, face)
    finally:
        BETA_MIN = saved
    src = x["pix_source"]
    src_ok = np.take_along_axis(ok.reshape(n, -1), np.maximum(src, 0).reshape(n, -1), 1).reshape(src.shape)
    x["grad_pix_sq"] = np.where((src >= 0) & src_ok & far_residuals(x, H, W)[1], gp, np.float32(0))
    return s, faces, H, W, x
