"""The Python bindings' host-space marshalling without a GPU: `smplpp_amd._lib._lib` is replaced by a stub that records every
`smplpp_*` call and returns 0, so these tests pin which entry point each method calls, with which scalars and NULL slots, what it
returns, and which inputs it refuses before any call."""
import numpy as np
import pytest
import torch

from smplpp_amd import _lib, model_io
from smplpp_amd._lib import HOST, SmplppError
from smplpp_amd.ik import VPoserDecoder
from smplpp_amd.smpl import SMPL

N = 2
V = 6890
SWEEP_CELLS = 8


class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("smplpp_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name in ("smplpp_model_create", "smplpp_vposer_create", "smplpp_device_count"):
                args[-1]._obj.value = 1
            elif name == "smplpp_sweep_grid":
                args[7]._obj.value = SWEEP_CELLS
            return 0

        return fn

    def last(self, name):
        assert self.calls and self.calls[-1][0] == name, [c[0] for c in self.calls[-3:]]
        return self.calls[-1][1]


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(_lib, "_lib", s)
    return s


@pytest.fixture(scope="module")
def model():
    return model_io.synthetic_model()


@pytest.fixture
def smpl(stub, model):
    s = SMPL()
    s.init(model)
    yield s
    s._h = None  # the stub's handle must never reach the real library's destroy


@pytest.fixture
def launched(smpl):
    beta, theta = model_io.synthetic_inputs(N)
    smpl.launch(beta, theta)
    return smpl


def _addr(a):
    return a.ctypes.data


def _refused(stub, fn, *args, **kw):
    before = len(stub.calls)
    with pytest.raises(SmplppError) as e:
        fn(*args, **kw)
    assert e.value.code == 1
    assert len(stub.calls) == before, "refused input reached the ABI"


def test_launch(stub, smpl):
    beta, theta = model_io.synthetic_inputs(N)
    out = smpl.launch(beta.astype(np.float64), theta)
    h, n, b, t, verts, joints, xforms, rest, space, stream = stub.last("smplpp_fk")
    assert (n, space, stream) == (N, HOST, None)
    assert all(isinstance(p, int) for p in (b, t, verts, joints, xforms, rest))
    assert out["verts"].shape == (N, V, 3) and out["rest"].shape == (N, V, 3)
    assert out["joints"].shape == (N, 24, 3) and out["xforms"].shape == (N, 24, 4, 4)
    assert all(a.dtype == np.float32 for a in out.values())
    assert (verts, joints, xforms, rest) == tuple(_addr(out[k]) for k in ("verts", "joints", "xforms", "rest"))
    assert smpl._out is out and smpl._n == N and smpl._theta.dtype == np.float32

    pre = np.empty((N, V, 3), np.float32)
    out = smpl.launch(beta, theta, want=("verts",), out={"verts": pre})
    _, _, _, _, verts, joints, xforms, rest, space, stream = stub.last("smplpp_fk")
    assert out["verts"] is pre and verts == _addr(pre)
    assert (joints, xforms, rest) == (None, None, None)
    assert out["joints"] is None and out["rest"] is None


def test_launch_refuses(stub, smpl):
    beta, theta = model_io.synthetic_inputs(N)
    _refused(stub, smpl.launch, beta, theta[:, :24])
    _refused(stub, smpl.launch, beta[:, :9], theta)
    _refused(stub, smpl.launch, beta, torch.from_numpy(theta))
    _refused(stub, smpl.launch, torch.from_numpy(beta), torch.from_numpy(theta))  # torch inputs must be on the device


def test_launch_backward(stub, smpl):
    beta, theta = model_io.synthetic_inputs(N)
    gv = np.ones((N, V, 3))
    g = smpl.launchBackward(beta, theta, grad_verts=gv)
    h, n, b, t, rest, pgv, pgj, gb, gt, space, stream = stub.last("smplpp_fk_vjp")
    assert (n, space, stream) == (N, HOST, None)
    assert rest is None and pgj is None and isinstance(pgv, int)
    assert g["beta"].shape == (N, 10) and g["theta"].shape == (N, 25, 3)
    assert g["beta"].dtype == np.float32 and g["theta"].dtype == np.float32
    assert (gb, gt) == (_addr(g["beta"]), _addr(g["theta"]))

    r = np.zeros((N, V, 3), np.float32)
    smpl.launchBackward(beta, theta, grad_joints=np.ones((N, 24, 3), np.float32), rest=r)
    _, _, _, _, rest, pgv, pgj, _, _, _, _ = stub.last("smplpp_fk_vjp")
    assert pgv is None and isinstance(pgj, int) and rest == _addr(r)


def test_launch_backward_refuses(stub, smpl):
    beta, theta = model_io.synthetic_inputs(N)
    _refused(stub, smpl.launchBackward, beta, theta, grad_verts=np.ones((N, V - 1, 3), np.float32))
    _refused(stub, smpl.launchBackward, beta, theta, grad_joints=np.ones((N, 23, 3), np.float32))
    _refused(stub, smpl.launchBackward, beta, theta[:1])
    _refused(stub, smpl.launchBackward, beta, theta, grad_verts=torch.ones((N, V, 3)))
    _refused(stub, smpl.launchBackward, beta, theta, rest=torch.ones((N, V, 3)))


@pytest.mark.parametrize("vertex", [False, True])
def test_normals(stub, launched, vertex):
    entry = "smplpp_vertex_normals" if vertex else "smplpp_face_normals"
    one, batch = (launched.calcVertexNormal, launched.calcVertexNormalBatch) if vertex else (launched.calcNormal, launched.calcNormalBatch)
    r = one(5)
    h, n, verts, count, ids, out, space, stream = stub.last(entry)
    assert (n, count, space, stream) == (1, 1, HOST, None)
    assert verts == _addr(launched._out["verts"])
    assert r.shape == (3,) and r.dtype == np.float32
    r = one([1, 2, 3])
    assert stub.last(entry)[1:4:2] == (1, 3) and r.shape == (3, 3)
    r = batch(np.array([4, 7], np.int32))
    h, n, verts, count, ids, out, space, stream = stub.last(entry)
    assert (n, count, space, stream) == (N, 2, HOST, None)
    assert r.shape == (N, 2, 3) and r.dtype == np.float32 and out == _addr(r)


def test_mesh_vertex_normals(stub, launched):
    r = launched.calcMeshVertexNormals()
    h, n, verts, out, space, stream = stub.last("smplpp_mesh_vertex_normals")
    assert (n, space, stream) == (N, HOST, None)
    assert verts == _addr(launched._out["verts"]) and out == _addr(r)
    assert r.shape == (N, V, 3) and r.dtype == np.float32


@pytest.mark.parametrize("kind", [0, 1])
def test_normals_backward_list(stub, smpl, kind):
    entry = ("smplpp_face_normals_vjp", "smplpp_vertex_normals_vjp")[kind]
    fn = (smpl.calcNormalBackward, smpl.calcVertexNormalBackward)[kind]
    verts = np.zeros((N, V, 3))
    r = fn(verts, [3, 1, 4], np.ones((N, 3, 3)))
    h, n, v, count, ids, gn, gv, acc, space, stream = stub.last(entry)
    assert (n, count, acc, space, stream) == (N, 3, 0, HOST, None)
    assert all(isinstance(p, int) for p in (v, ids, gn))
    assert r.shape == (N, V, 3) and r.dtype == np.float32 and gv == _addr(r)

    out = np.zeros((N, V, 3), np.float32)
    r = fn(verts, torch.tensor([2, 5]), np.ones((N, 2, 3), np.float32), out=out)
    _, n, _, count, _, _, gv, acc, _, _ = stub.last(entry)
    assert (n, count, acc) == (N, 2, 1)
    assert r is out and gv == _addr(out)


def test_normals_backward_mesh(stub, smpl):
    r = smpl.calcMeshVertexNormalsBackward(np.zeros((N, V, 3), np.float32), np.ones((N, V, 3), np.float32))
    h, n, v, gn, gv, acc, space, stream = stub.last("smplpp_mesh_vertex_normals_vjp")
    assert (n, acc, space, stream) == (N, 0, HOST, None)
    assert r.shape == (N, V, 3) and r.dtype == np.float32 and gv == _addr(r)
    out = np.zeros((N, V, 3), np.float32)
    r = smpl.calcMeshVertexNormalsBackward(np.zeros((N, V, 3), np.float32), np.ones((N, V, 3), np.float32), out=out)
    assert stub.last("smplpp_mesh_vertex_normals_vjp")[5] == 1 and r is out


def test_normals_backward_refuses(stub, smpl):
    verts, g = np.zeros((N, V, 3), np.float32), np.ones((N, 2, 3), np.float32)
    _refused(stub, smpl.calcNormalBackward, verts[:, :-1], [0, 1], g)
    _refused(stub, smpl.calcNormalBackward, verts, [0, 1, 2], g)
    _refused(stub, smpl.calcVertexNormalBackward, verts, [0, 1], torch.from_numpy(g))
    _refused(stub, smpl.calcVertexNormalBackward, verts, [0, 1], g, out=np.zeros((N, V, 3), np.float64))
    _refused(stub, smpl.calcVertexNormalBackward, verts, [0, 1], g, out=torch.zeros((N, V, 3)))
    _refused(stub, smpl.calcMeshVertexNormalsBackward, verts, g)
    _refused(stub, smpl.calcMeshVertexNormalsBackward, verts, np.ones((N, V, 3)), out=np.zeros((V, N, 3), np.float32).transpose(1, 0, 2))


def test_sweep_grid(stub, launched):
    r = launched.calcSweepGrid(frame=1)
    (n0, a0), (n1, a1) = stub.calls[-2:]
    assert n0 == n1 == "smplpp_sweep_grid"
    assert a0[1] == _addr(launched._out["verts"][1])
    assert a0[4:7] == (0, None, None) and a0[8:] == (HOST, None)
    assert a1[4] == SWEEP_CELLS and isinstance(a1[5], int) and isinstance(a1[6], int) and a1[8:] == (HOST, None)
    assert r["winding"].shape == (SWEEP_CELLS,) and r["winding"].dtype == np.float32
    assert r["inside"].shape == (SWEEP_CELLS,) and r["inside"].dtype == bool
    assert r["grid_idx"].shape == (0, 3)


def test_closest_points(stub, launched):
    face, closest, sq = launched.closestPoints(np.zeros((N, 5, 3)))
    h, n, verts, K, pts, pf, pc, ps, space, stream = stub.last("smplpp_closest_points")
    assert (n, K, space, stream) == (N, 5, HOST, None)
    assert face.shape == (N, 5) and face.dtype == np.int64
    assert closest.shape == (N, 5, 3) and closest.dtype == np.float32
    assert sq.shape == (N, 5) and sq.dtype == np.float32
    assert (pf, pc, ps) == (_addr(face), _addr(closest), _addr(sq))


@pytest.fixture
def vposer(stub):
    v = VPoserDecoder(VPoserDecoder.synthetic_params())
    yield v
    v._h = None


def test_vposer_forward(stub, vposer):
    z = np.zeros((N, 32))
    out = vposer.forward(z, frame_base=7)
    h, n, fb, pz, po, pj, space, stream = stub.last("smplpp_vposer_forward_at")
    assert (n, fb, pj, space, stream) == (N, 7, None, HOST, None)
    assert out.shape == (N, 21, 3) and out.dtype == np.float32 and po == _addr(out)
    out, jac = vposer.forward(z, want_jac=True)
    _, n, fb, _, po, pj, _, _ = stub.last("smplpp_vposer_forward_at")
    assert (n, fb) == (N, 0) and jac.shape == (N, 63, 32) and jac.dtype == np.float32 and pj == _addr(jac)


def test_vposer_backward(stub, vposer):
    z = np.zeros((N, 32))
    gz = vposer.launchBackward(z, np.ones((N, 21, 3)), frame_base=3)
    h, n, fb, pz, pg, pgz, po, space, stream = stub.last("smplpp_vposer_vjp")
    assert (n, fb, po, space, stream) == (N, 3, None, HOST, None)
    assert gz.shape == (N, 32) and gz.dtype == np.float32 and pgz == _addr(gz)
    gz, out = vposer.launchBackward(z, np.ones((N, 21, 3)), want_out=True)
    assert stub.last("smplpp_vposer_vjp")[6] == _addr(out) and out.shape == (N, 21, 3) and out.dtype == np.float32
    _refused(stub, vposer.launchBackward, z, np.ones((N, 20, 3)))
    _refused(stub, vposer.launchBackward, z, torch.ones((N, 21, 3)))


def test_vposer_jacobian(stub, vposer):
    z = np.zeros((N, 32))
    jac = vposer.jacobian(z, frame_base=5)
    h, n, fb, pz, po, pj, space, stream = stub.last("smplpp_vposer_jacobian")
    assert (n, fb, po, space, stream) == (N, 5, None, HOST, None)
    assert jac.shape == (N, 63, 32) and jac.dtype == np.float32 and pj == _addr(jac)
    jac, out = vposer.jacobian(z, want_out=True)
    assert stub.last("smplpp_vposer_jacobian")[4] == _addr(out) and out.shape == (N, 21, 3)


def test_stub_handles(stub, smpl, vposer):
    assert smpl.handle.value == 1 and vposer._h.value == 1
