"""Helpers of the kernel-level split tests (test_conv_split_gpu.py, test_conv_split_wide_gpu.py): operands through the C ABI
and the two checks against the fp64 references of oracle/fp64_ref.py (see the docstring of test_conv_split_gpu.py)."""
import gc
import zlib

import torch

from oracle import fp64_ref as R

SLAB_TOL = 1e-4
SPLIT_TERM = 2.0 ** -14


def _ops():
    from coma_unet_amd import ops, _lib
    return ops, _lib


def _buf(shape, ld, fill):
    """A (B, D, H, W, C) fp32 view with voxel pitch ld >= C whose foreign lanes hold `fill`."""
    C = shape[-1]
    b = torch.full(tuple(shape[:-1]) + (max(ld, C),), fill, dtype=torch.float32, device="cuda")
    return b[..., :C]


def _rand(shape, ld, gen, scale=1.0):
    v = _buf(shape, ld, 3.0e4)        # (finite garbage in the foreign lanes: a kernel that reads them is far off)
    v.copy_(torch.randn(tuple(shape), generator=gen, device="cuda") * scale)
    return v


def _weights(Bw, cout, cin, gen):
    """Gaussian fp32 kernel-layout weights wk[Bw, 27, Cout, Cin], outputs O(1)."""
    return (torch.randn((Bw, 27, cout, cin), generator=gen, device="cuda") * (1.0 / (27 * cin) ** 0.5)).contiguous()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def _bound(ref, A, K, base=None):
    return R.elem_bound(ref, A, 3 * K, u_out=R.U_F32, base=base) + SPLIT_TERM * A


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _check(r, what):
    ratio = R.check_elementwise(r["y"], r["ref"], _bound(r["ref"], r["A"], r["K"], r.get("base")), what)
    slab = R.slab_rel_l2(r["y"], r["ref"], 2)
    print(f"{what}: kernel {r['kernel']}, worst ratio to the element bound {ratio:.3g}, max slab rel-L2 {slab:.3g}")
    assert slab <= SLAB_TOL, (what, slab)
    return ratio, slab
