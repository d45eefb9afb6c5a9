"""Inputs and comparisons shared by test_point_distance_gpu.py and test_mesh_point_distance_gpu.py."""
import numpy as np

import closest_ref as cr


def _verts(s, n, seed):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    return s.launch(beta, theta, want=("verts",))["verts"]


def _surface_points(v, faces, K, rng, off=0.015):
    """K points per frame sampled on the posed surface and moved up to +-off along the face normal (the scan-like case)."""
    n = len(v)
    out = np.empty((n, K, 3), np.float32)
    for f in range(n):
        fid = rng.integers(0, len(faces), K)
        w = rng.dirichlet(np.ones(3), K)
        tri = v[f].astype(np.float64)[faces[fid]]
        nrm = cr.face_normals(v[f], faces)[fid]
        out[f] = (np.einsum("ki,kix->kx", w, tri) + rng.uniform(-off, off, (K, 1)) * nrm).astype(np.float32)
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _rel(a, b):
    return np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30)
