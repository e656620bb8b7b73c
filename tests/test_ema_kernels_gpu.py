"""coma_adamw_ema / coma_swap_f32 (csrc/elementwise.hip: adamw_ema_k, swap_f32_k) on their own, at the sizes of
tests/_ema_plan.py (one partly filled block; the 16-byte path past one grid pass with a scalar tail; the scalar path on slices
one element off 16-byte alignment; fewer blocks than the grid cap).  Every buffer sits between sentinels that must survive.
p, m, v are bitwise those of the kernels the new one restates; the average stays within the helper's bound (counted from the
kernel source) of the fp64 recurrence run on the kernel's own parameters."""
import gc
import zlib

import pytest
import torch

import _ema_plan as EP
import _nonconv_plan as NP
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

SENT = -7.0
HP = NP.ADAMW_HP
VARIANTS = [(0.5, False), (0.999, False), (0.5, True), (0.999, True)]          # (ema_decay, ema_warmup)


def _ops():
    from coma_unet_amd import ops
    return ops


def _adamw(p, g, m, v, lr, b1, b2, eps, wd, step, step_dev=None):
    """coma_adamw through the binding table itself (tests/test_data_parallel_cpu.py replaces ops.adamw_ with a CPU restatement
    for the rest of its process)."""
    from coma_unet_amd import _lib as L
    L.check(L.lib.coma_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, b1, b2, eps, wd, step, L.ptr(step_dev),
                             L.stream()), "coma_adamw")


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


class FlatGuard:
    """A 1-D view `t` of n cells at element offset `off` behind a 64-cell sentinel header, with a sentinel tail."""

    def __init__(self, n, dtype, off=0, fill=SENT):
        self.fill, self.lo, self.n = fill, 64 + off, n
        self.flat = torch.full((64 + off + n + 4096,), fill, dtype=dtype, device="cuda")
        self.t = self.flat[self.lo:self.lo + n]

    def untouched(self):
        return bool((self.flat[:self.lo] == self.fill).all()) and bool((self.flat[self.lo + self.n:] == self.fill).all())


def _state(n, off, gen, bufs=4):
    out = [FlatGuard(n, torch.float32, off) for _ in range(bufs)]
    out[0].t.copy_(torch.randn(n, generator=gen, device="cuda"))
    out[2].t.zero_()
    out[3].t.zero_()
    return out


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"d{v[0]}-{'warm' if v[1] else 'flat'}")
@pytest.mark.parametrize("dev_step", [False, True], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("case", EP.CASES, ids=lambda c: c[0])
def test_adamw_ema_is_adamw_and_average_follows_recurrence(case, dev_step, variant):
    """Three updates of coma_adamw beside coma_adamw_ema without counter and partials: p, m, v bitwise equal; the average
    within the helper's bound of the fp64 recurrence on the kernel's own p'.  With a device step count the host value stays 7:
    under warm-up d_t must follow the device count (2/11, 3/12, 4/13), not the host's."""
    ops = _ops()
    name, n, off = case
    decay, warm = variant
    lr, b1, b2, eps, wd = HP
    try:
        ref = _state(n, off, _gen("adamw_ema", name))
        new = _state(n, off, _gen("adamw_ema", name), bufs=5)                    # same seed: a copy of the same state
        ema = new[4]
        ema.t.copy_(torch.randn(n, generator=_gen("adamw_ema-e", name), device="cuda"))
        aligned = off == 0
        assert all((b.t.data_ptr() % 16 == 0) == aligned for b in new)
        st = EP.ema_init(ema.t)
        wrong = EP.ema_init(ema.t)                                               # the recurrence at the HOST's step count
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda") if dev_step else None
        gen = _gen("adamw_ema-g", name)
        ds = []
        for t in (1, 2, 3):
            gr = torch.randn(n, generator=gen, device="cuda") * (0.5 if t == 2 else 1.0)
            ref[1].t.copy_(gr)
            new[1].t.copy_(gr)
            if dev_step:
                step_dev.fill_(t)
            host_t = 7 if dev_step else t
            p0, g0, m0, v0 = (b.t for b in ref)
            p1, g1, m1, v1, e1 = (b.t for b in new)
            _adamw(p0, g0, m0, v0, lr, b1, b2, eps, wd, host_t, step_dev)
            ops.adamw_ema_(p1, g1, m1, v1, e1, decay, warm, lr, b1, b2, eps, wd, host_t, step_dev)
            for nm, a, b_ in (("p", p0, p1), ("m", m0, m1), ("v", v0, v1)):
                assert torch.equal(a, b_), f"{nm} update {t}: coma_adamw_ema differs from coma_adamw"
            assert torch.equal(g1, gr)
            ds.append(EP.ema_update(st, p1, decay, warm, t))
            EP.ema_update(wrong, p1, decay, warm, 7)
            ratio = R.check_elementwise(e1, st["e"], st["b"], f"ema update {t}")
            print(f"adamw_ema {name} {'step_dev' if dev_step else 'host'} d={decay} warm={warm} update {t}: d_t {ds[-1]:.6g}, "
                  f"worst ratio {ratio:.3g}")
        if warm:
            assert ds == [2 / 11, 3 / 12, 4 / 13] and len(set(ds)) == 3
            if dev_step:      # a kernel that took the host's 7 (d_t = 8/17 every time) lies far outside the bound
                far = ((new[4].t.double() - wrong["e"]).abs() > 4 * wrong["b"]).double().mean()
                assert float(far) > 0.5, "the average does not tell the device step count from the host's"
        else:
            assert ds == [NP.f32(decay)] * 3
        assert all(b.untouched() for b in ref + new)
    finally:
        _free()


@pytest.mark.parametrize("case", EP.CASES, ids=lambda c: c[0])
def test_adamw_ema_with_counter_and_clip_is_adamw_ex(case):
    """A counter of 3 and a clip that bites (half the norm of the mean gradient), device step count, three updates: p, m, v
    and norm_out are bitwise coma_adamw_ex's."""
    ops = _ops()
    name, n, off = case
    lr, b1, b2, eps, wd = HP
    K = 3
    try:
        ref = _state(n, off, _gen("adamw_ema-ex", name))
        new = _state(n, off, _gen("adamw_ema-ex", name), bufs=5)
        new[4].t.copy_(new[0].t)
        st = EP.ema_init(new[4].t)
        parts = FlatGuard(ops.ACC_PARTIALS, torch.float64, fill=float("nan"))
        norms = [FlatGuard(1, torch.float32), FlatGuard(1, torch.float32)]
        count = torch.full((1,), K, dtype=torch.int32, device="cuda")
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        gen = _gen("adamw_ema-ex-g", name)
        for t in (1, 2, 3):
            gr = torch.randn(n, generator=gen, device="cuda") * (3.0 if t == 2 else 1.0)
            ref[1].t.copy_(gr)
            new[1].t.copy_(gr)
            step_dev.fill_(t)
            max_norm = NP.f32(0.5 * float((gr.double() ** 2).sum()) ** 0.5 / K)
            parts.t.fill_(float("nan"))
            nb = ops.grad_accum_(None, ref[1].t, None, parts.t)
            p0, g0, m0, v0 = (b.t for b in ref)
            p1, g1, m1, v1, e1 = (b.t for b in new)
            before = p1.clone()
            ops.adamw_ex_(p0, g0, m0, v0, lr, b1, b2, eps, wd, 7, step_dev, count, parts.t, nb, None, max_norm, norms[0].t)
            ops.adamw_ema_(p1, g1, m1, v1, e1, 0.9, True, lr, b1, b2, eps, wd, 7, step_dev, count, parts.t, nb, None, max_norm,
                           norms[1].t)
            for nm, a, b_ in (("p", p0, p1), ("m", m0, m1), ("v", v0, v1), ("norm_out", norms[0].t, norms[1].t)):
                assert torch.equal(a, b_), f"{nm} update {t}: coma_adamw_ema differs from coma_adamw_ex"
            assert not torch.equal(p1, before)
            EP.ema_update(st, p1, 0.9, True, t)
            R.check_elementwise(e1, st["e"], st["b"], f"ema update {t}")
        assert all(b.untouched() for b in ref + new + norms) and int(count) == K
    finally:
        _free()


def test_adamw_ema_of_nothing_writes_nothing():
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    bufs = [FlatGuard(8, torch.float32) for _ in range(5)]
    p, g, m, v, e = (b.t[4:4] for b in bufs)                       # zero-length slices in the middle of live buffers
    ops.adamw_ema_(p, g, m, v, e, 0.9, False, lr, b1, b2, eps, wd, 1)
    z = torch.empty(0, dtype=torch.float32, device="cuda")
    ops.adamw_ema_(z, z, z, z, z, 0.9, True, lr, b1, b2, eps, wd, 1, torch.ones(1, dtype=torch.int32, device="cuda"))
    ops.swap_f32_(p, e)
    torch.cuda.synchronize()
    assert all(bool((b.flat == SENT).all()) for b in bufs)


def test_adamw_ema_rejects_a_decay_outside_the_open_interval():
    from coma_unet_amd._lib import ComaError
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    bufs = [FlatGuard(8, torch.float32) for _ in range(5)]
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ComaError, match="ema_decay"):
            ops.adamw_ema_(*(b.t for b in bufs), bad, False, lr, b1, b2, eps, wd, 1)
    torch.cuda.synchronize()
    assert all(bool((b.flat == SENT).all()) for b in bufs)


@pytest.mark.parametrize("case", EP.CASES, ids=lambda c: c[0])
def test_swap_exchanges_bitwise(case):
    """Random bit patterns (NaN payloads included) change places exactly; a second swap restores both."""
    ops = _ops()
    name, n, off = case
    try:
        a, b = FlatGuard(n, torch.float32, off), FlatGuard(n, torch.float32, off)
        assert (a.t.data_ptr() % 16 == 0) == (off == 0)
        bits = lambda t: t.view(torch.int32)
        gen = _gen("swap", name)
        for buf in (a, b):
            bits(buf.t).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32))
        a0, b0 = bits(a.t).clone(), bits(b.t).clone()
        assert not torch.equal(a0, b0)
        ops.swap_f32_(a.t, b.t)
        assert torch.equal(bits(a.t), b0) and torch.equal(bits(b.t), a0)
        ops.swap_f32_(a.t, b.t)
        assert torch.equal(bits(a.t), a0) and torch.equal(bits(b.t), b0)
        # the sentinel regions are compared as bit patterns too (-7.0 is no NaN: == is enough)
        assert a.untouched() and b.untouched()
    finally:
        _free()


def test_swap_refuses_one_buffer_and_overlap():
    from coma_unet_amd._lib import ComaError
    ops = _ops()
    buf = torch.arange(64, dtype=torch.float32, device="cuda")
    keep = buf.clone()
    with pytest.raises(ComaError, match="overlap"):
        ops.swap_f32_(buf[:32], buf[:32])
    with pytest.raises(ComaError, match="overlap"):
        ops.swap_f32_(buf[:32], buf[16:48])
    with pytest.raises(ComaError, match="overlap"):
        ops.swap_f32_(buf[16:48], buf[:32])
    ops.swap_f32_(buf[:32], buf[32:])                              # touching ranges are disjoint
    torch.cuda.synchronize()
    assert torch.equal(buf[:32], keep[32:]) and torch.equal(buf[32:], keep[:32])
