"""The VPoser decoder's vector-Jacobian product by torch autograd, for the backward-pass tests: oracle/vposer_torch.py's decoder
(the op-for-op restatement of src/VPoser.cpp) with module and inputs in float64 is the oracle of smplpp_vposer_vjp; in float32 it
measures what a plain fp32 autograd of the same graph gets wrong."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vposer_torch as VT  # noqa: E402


def decoder(params, dtype=torch.float64):
    return VT.VPoserDecoder(params).to(dtype)


def vjp(dec, z, grad_out, dtype=torch.float64):
    """(dL/dz [n,32], out [n,21,3]) for dL/dout = grad_out, by autograd of `dec` (a `decoder`) in `dtype`."""
    dec = dec.to(dtype)
    zt = torch.as_tensor(np.asarray(z), dtype=dtype).clone().requires_grad_(True)
    out = dec(zt)
    gz, = torch.autograd.grad((out * torch.as_tensor(np.asarray(grad_out), dtype=dtype)).sum(), zt)
    return gz.detach().numpy().astype(np.float64), out.detach().numpy().astype(np.float64)
