"""The VPoser decoder's Jacobian d(out)/dz by torch autograd, for the exact-Jacobian tests: oracle/vposer_torch.py's decoder (the
op-for-op restatement of src/VPoser.cpp, tests/vposer_vjp_oracle.decoder) with module and input in float64 is the oracle of
smplpp_vposer_jacobian; in float32 it measures what a plain fp32 autograd Jacobian of the same graph gets wrong."""
import numpy as np
import torch


def jacobian(dec, z, dtype=torch.float64):
    """d(out)/dz [n,63,32] of `dec` (a tests/vposer_vjp_oracle.decoder) at z [n,32], one frame at a time, in `dtype`."""
    dec = dec.to(dtype)
    zz = torch.as_tensor(np.asarray(z), dtype=dtype).reshape(-1, 32)
    rows = []
    for f in range(zz.shape[0]):
        J = torch.autograd.functional.jacobian(lambda x: dec(x[None]).reshape(63), zz[f].clone())
        rows.append(J.detach().numpy().astype(np.float64))
    return np.stack(rows)
