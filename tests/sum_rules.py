"""The two fixed-order sums of the library (include/smplpp_hip.h, FIXED-ORDER SUMS; smplpp_amd/csrc/fixed_sum.h) restated in numpy, once
for every oracle: element k goes to partial k mod `parts` in ascending k from +0, and the partials meet by an xor tree,
p_i = p_i + p_(i xor s) for each s in turn; the sum is partial 0.  The dtype is the argument's."""
import numpy as np

TREE64 = (32, 16, 8, 4, 2, 1)
TREE1024 = TREE64 + (512, 256, 128, 64)


def accumulate(v, parts, axis=-1):
    """[..., parts]: the partials of v along `axis` (moved last), before they meet."""
    v = np.moveaxis(np.asarray(v), axis, -1)
    part = np.zeros(v.shape[:-1] + (parts,), v.dtype)
    for k0 in range(0, v.shape[-1], parts):
        w = min(parts, v.shape[-1] - k0)
        part[..., :w] = part[..., :w] + v[..., k0:k0 + w]
    return part


def meet(part, tree, axis=-1):
    """Partial 0 of `part` after the meetings of `tree` along `axis`."""
    part = np.moveaxis(part, axis, -1)
    at = np.arange(part.shape[-1])
    for s in tree:
        part = part + part[..., at ^ s]
    return part[..., 0]


def sum64(v, axis=-1):
    return meet(accumulate(v, 64, axis), TREE64)


def sum1024(v, axis=-1):
    return meet(accumulate(v, 1024, axis), TREE1024)
