"""coma_grad_accum / coma_adamw_ex (csrc/elementwise.hip: grad_accum_k, adamw_ex_k) on their own, at the sizes of
tests/_grad_accum_plan.py (one partly filled block; the float4 path past one grid pass with a scalar tail; the scalar path on
slices that are not 16-byte aligned; fewer blocks than the grid cap).  Every buffer sits between sentinels that must survive,
the table of partials is prefilled with a sentinel (only the live slots may be written; a NaN behind them must not reach the
norm), bit-exact where the kernels round once or not at all, else within the bounds the helper derives from the source."""
import gc
import zlib

import pytest
import torch

import _grad_accum_plan as GP
import _nonconv_plan as NP
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

SENT = -7.0
HP = NP.ADAMW_HP


def _ops():
    from coma_unet_amd import ops
    return ops


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


def _partials():
    return FlatGuard(GP.ACC_CAP, torch.float64)


def _check_live(parts, nb):
    """Only the first nb slots were written (a sum of squares is never the negative sentinel)."""
    assert bool((parts.t[:nb] >= 0).all()), "a live partial was not written"
    assert bool((parts.t[nb:] == SENT).all()), "a slot beyond the live partials was written"
    assert parts.untouched()


@pytest.mark.parametrize("case", GP.CASES, ids=lambda c: c[0])
def test_grad_accum(case):
    """A window of three calls (count_dev = 0, 1, 2) into an accumulator prefilled with garbage, then the norm-only form."""
    ops = _ops()
    name, n, off = case
    gen = _gen("grad_accum", name)
    try:
        acc, g, parts = FlatGuard(n, torch.float32, off), FlatGuard(n, torch.float32, off), _partials()
        aligned = off == 0
        assert (acc.t.data_ptr() % 16 == 0) == aligned and (g.t.data_ptr() % 16 == 0) == aligned
        nb_want = GP.accum_blocks(n, aligned)
        acc.t.copy_(torch.randn(n, generator=gen, device="cuda") * 1e3)          # garbage the first call must not read
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        gs = []
        for k in range(3):
            g.t.copy_(torch.randn(n, generator=gen, device="cuda") * (0.5 if k == 1 else 1.0))
            gs.append(g.t.clone())
            count.fill_(k)
            parts.t.fill_(SENT)
            nb = ops.grad_accum_(acc.t, g.t, count, parts.t)
            assert nb == nb_want
            _check_live(parts, nb)
            A, b = GP.accumulate(gs)[-1]
            if k == 0:
                assert torch.equal(acc.t, gs[0]), "the window's first call must assign"
            else:
                ratio = R.check_elementwise(acc.t, A, b, f"acc after call {k}")
                print(f"grad_accum {name} call {k}: worst ratio acc {ratio:.3g}")
            assert torch.equal(g.t, gs[k]) and int(count) == k
            # the partials: fp64 sums over the fp32 values the kernel stored
            got = float(parts.t[:nb].sum())
            own = float((acc.t.double() ** 2).sum())
            assert abs(got - own) <= 2 * (n + 2) * GP.U64 * own, (got, own)     # (the kernel's sum and this one's: (n + 2) 2^-53 each)
            tot, rel = GP.sumsq(A, b)
            assert abs(got - tot) <= rel * tot, (got, tot, rel)
        from_accum = parts.t.clone()
        # without partials nothing but acc is written
        keep = acc.t.clone()
        count.fill_(0)
        parts.t.fill_(SENT)
        assert ops.grad_accum_(acc.t, keep, count, None) == nb_want
        assert torch.equal(acc.t, keep) and bool((parts.t == SENT).all())
        # norm-only form: reads its input, writes the live partials and nothing else; bitwise repeatable, and the same
        # numbers as the accumulating launch gave for the same values (same elements per thread, same order)
        runs = []
        for _ in range(2):
            parts.t.fill_(SENT)
            assert ops.grad_accum_(None, acc.t, None, parts.t) == nb_want
            _check_live(parts, nb_want)
            runs.append(parts.t.clone())
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], from_accum)
        assert torch.equal(acc.t, keep)
        assert acc.untouched() and g.untouched() and parts.untouched()
    finally:
        _free()


def test_grad_accum_of_nothing_launches_nothing():
    ops = _ops()
    parts = _partials()
    e = torch.empty(0, dtype=torch.float32, device="cuda")
    assert ops.grad_accum_(e, e, torch.zeros(1, dtype=torch.int32, device="cuda"), parts.t) == 0
    assert ops.grad_accum_(None, e, None, parts.t) == 0
    torch.cuda.synchronize()
    assert bool((parts.t == SENT).all())


def _state(n, off, gen):
    bufs = [FlatGuard(n, torch.float32, off) for _ in range(4)]
    p, g, m, v = (b.t for b in bufs)
    p.copy_(torch.randn(n, generator=gen, device="cuda"))
    m.zero_()
    v.zero_()
    return bufs


@pytest.mark.parametrize("dev_step", [False, True], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("case", GP.CASES, ids=lambda c: c[0])
def test_adamw_ex_without_scale_is_adamw(case, dev_step):
    """Three steps of coma_adamw against (1) coma_adamw_ex with no counter and no partials and (2) coma_adamw_ex with a
    counter of 1 and a clip that cannot bite (max_norm 1e30): s = 1.0f, and p, m, v are bitwise coma_adamw's.  (2)'s
    norm_out is the gradient's norm to 2 u, with NaNs behind the live partials."""
    ops = _ops()
    name, n, off = case
    lr, b1, b2, eps, wd = HP
    try:
        sets = [_state(n, off, _gen("adamw_ex", name)) for _ in range(3)]       # same seed: three copies of one state
        parts = FlatGuard(GP.ACC_CAP, torch.float64, fill=float("nan"))
        norm_out = FlatGuard(1, torch.float32)
        one = torch.ones(1, dtype=torch.int32, device="cuda")
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda") if dev_step else None
        gen = _gen("adamw_ex-g", name)
        for t in (1, 2, 3):
            gr = torch.randn(n, generator=gen, device="cuda") * (0.5 if t == 2 else 1.0)
            for bufs in sets:
                bufs[1].t.copy_(gr)
            if dev_step:
                step_dev.fill_(t)
            host_t = 7 if dev_step else t           # (with a device counter the host value is ignored)
            (p0, g0, m0, v0), (p1, g1, m1, v1), (p2, g2, m2, v2) = ([b.t for b in bufs] for bufs in sets)
            ops.adamw_(p0, g0, m0, v0, lr, b1, b2, eps, wd, host_t, step_dev)
            ops.adamw_ex_(p1, g1, m1, v1, lr, b1, b2, eps, wd, host_t, step_dev)
            parts.t.fill_(float("nan"))
            nb = ops.grad_accum_(None, g2, None, parts.t)
            assert nb == GP.accum_blocks(n, off == 0) and bool(torch.isnan(parts.t[nb:]).all())
            ops.adamw_ex_(p2, g2, m2, v2, lr, b1, b2, eps, wd, host_t, step_dev, one if t != 3 else None, parts.t, nb, None,
                          1e30, norm_out.t)
            for nm, a, b_, c in (("p", p0, p1, p2), ("m", m0, m1, m2), ("v", v0, v1, v2)):
                assert torch.equal(a, b_), f"{nm} step {t}: adamw_ex without scale differs from adamw"
                assert torch.equal(a, c), f"{nm} step {t}: adamw_ex with an inactive clip differs from adamw"
            ref = float((gr.double() ** 2).sum()) ** 0.5
            got = float(norm_out.t)
            assert abs(got - ref) <= 2 * R.U_F32 * ref, (got, ref)             # NaN beyond the live partials: not read
        assert all(b.untouched() for bufs in sets for b in bufs) and norm_out.untouched()
    finally:
        _free()


@pytest.mark.parametrize("dev_step", [False, True], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("case", GP.CASES, ids=lambda c: c[0])
def test_adamw_ex_clipped_mean(case, dev_step):
    """count = 3 and max_norm = half the true norm of the mean gradient, three updates; the second one with a non-zero
    extra_sumsq (gradients outside the buffer), which must move the norm and the scale as the helper says.  m, v and
    p - p0 within the helper's bounds."""
    ops = _ops()
    name, n, off = case
    lr, b1, b2, eps, wd = HP
    K = 3
    try:
        bufs = _state(n, off, _gen("adamw_ex-clip", name))
        p, g, m, v = (b.t for b in bufs)
        p0 = p.clone()
        st = NP.adamw_init(p0)
        parts = FlatGuard(GP.ACC_CAP, torch.float64, fill=float("nan"))
        norm_out = FlatGuard(1, torch.float32)
        count = torch.full((1,), K, dtype=torch.int32, device="cuda")
        extra = torch.zeros(1, dtype=torch.float64, device="cuda")
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda") if dev_step else None
        gen = _gen("adamw_ex-clip-g", name)
        for t in (1, 2, 3):
            g.copy_(torch.randn(n, generator=gen, device="cuda") * (3.0 if t == 2 else 1.0))     # the window's SUM
            A, zero = g.double(), torch.zeros(n, dtype=torch.float64, device="cuda")
            tot, rel = GP.sumsq(A, zero)
            ex = 0.75 * tot if t == 2 else 0.0
            extra.fill_(ex)
            true_norm = (tot + ex) ** 0.5 / K
            max_norm = NP.f32(0.5 * true_norm)
            sc = GP.scale(tot + ex, rel * tot / (tot + ex), K, max_norm)
            assert 0.49 < sc["c"] < 0.51
            if dev_step:
                step_dev.fill_(t)
            parts.t.fill_(float("nan"))
            nb = ops.grad_accum_(None, g, None, parts.t)
            ops.adamw_ex_(p, g, m, v, lr, b1, b2, eps, wd, 7 if dev_step else t, step_dev, count, parts.t, nb,
                          extra if t == 2 else None, max_norm, norm_out.t)
            GP.apply(st, A, zero, sc, t)
            assert abs(float(norm_out.t) - sc["norm"]) <= sc["b_norm"], (float(norm_out.t), sc["norm"], sc["b_norm"])
            rm = R.check_elementwise(m, st["m"], st["bm"], f"m step {t}")
            rv = R.check_elementwise(v, st["v"], st["bv"], f"v step {t}")
            ru = R.check_elementwise(p.double() - p0.double(), st["p"] - p0.double(), st["bp"], f"p - p0 step {t}")
            print(f"adamw_ex {name} {'step_dev' if dev_step else 'host'} step {t}: worst ratio m {rm:.3g} v {rv:.3g} update {ru:.3g}")
        assert all(b.untouched() for b in bufs) and norm_out.untouched() and int(count) == K
    finally:
        _free()
