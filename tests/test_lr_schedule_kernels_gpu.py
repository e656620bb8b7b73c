"""coma_adamw_sched (csrc/elementwise.hip: adamw_sched_k, adamw_sched_ema_k) on its own, at the sizes of tests/_ema_plan.py (one
partly filled block; the 16-byte path past one grid pass with a scalar tail; the scalar path on slices one element off 16-byte
alignment; fewer blocks than the grid cap).  Every buffer sits between sentinels that must survive.

lr_out stays within the bound tests/_lr_schedule_plan.py counts from the kernel source of the fp64 schedule; with no table and
lr_scale 1 p, m, v (norm_out, e) are bitwise those of coma_adamw / coma_adamw_ex / coma_adamw_ema called with lr = lr_out; with
a table every segment's elements are bitwise what the same entry point gives them with n_segs = 0 and the segment's options.

On "the slice alone": coma_adamw's own two loops do not round alike -- its 16-byte loop fuses the two moment updates into one
fma each, its scalar loop (tail, unaligned buffers) rounds product and sum separately (its ISA shows it; tests/
test_ema_step_gpu.py meets the same fact) -- and the scheduled kernels restate each loop as it is, so that the uniform case is
bitwise coma_adamw on BOTH paths.  A segment cut out at an arbitrary element would move its elements from one loop to the
other.  The reference run of a segment therefore keeps every element on the loop it is on in the whole call: elements of the
16-byte body are run as the segment rounded out to whole 16-byte chunks, in 16-byte aligned buffers; elements of the scalar
tail, and all elements of an unaligned call, are run as the exact slice in buffers one element off alignment."""
import gc
import zlib

import numpy as np
import pytest
import torch

import _lr_schedule_plan as LP
import _nonconv_plan as NP

pytestmark = pytest.mark.gpu

SENT = -7.0
HP = NP.ADAMW_HP
COS = LP.KINDS["cosine"]


def _ops():
    from coma_unet_amd import ops
    return ops


def _adamw(p, g, m, v, lr, b1, b2, eps, wd, step, step_dev=None):
    """coma_adamw through the binding table itself (tests/test_data_parallel_cpu.py replaces ops.adamw_ for its process)."""
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
    """p, g, m, v (, e): random parameters, moments of one earlier update so that nothing is zero."""
    out = [FlatGuard(n, torch.float32, off) for _ in range(bufs)]
    out[0].t.copy_(torch.randn(n, generator=gen, device="cuda"))
    out[1].t.copy_(torch.randn(n, generator=gen, device="cuda"))
    out[2].t.copy_(0.1 * torch.randn(n, generator=gen, device="cuda"))
    out[3].t.copy_(1e-3 * torch.rand(n, generator=gen, device="cuda"))
    if bufs > 4:
        out[4].t.copy_(torch.randn(n, generator=gen, device="cuda"))
    return out


def _dev(x, dtype):
    return torch.tensor([x], dtype=dtype, device="cuda")


def _args(sched):
    return LP.schedule(sched).kernel_args()


# ---- the schedule's value -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(LP.KINDS))
def test_lr_out_follows_the_device_count(kind):
    """Every kind at t in {1, 2, Wm, Wm + 1, Wm + ceil(T / 2), Wm + T, Wm + T + 5}, the count given through sched_step_dev
    while both host counts say 7: lr_out within the bound of the fp64 value; wherever the plan at t differs from the plan at 7
    a kernel that took the host's count is far outside."""
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    try:
        bufs = _state(5, 0, _gen("sched-lr", kind))
        out = FlatGuard(1, torch.float32)
        lr_dev, cnt, bc = _dev(lr, torch.float32), _dev(0, torch.int32), _dev(1, torch.int32)
        at7 = LP.lr_ref(LP.KINDS[kind], NP.f32(lr), 7)
        told, got_all = 0, []
        for t in LP.STEPS:
            cnt.fill_(t)
            ops.adamw_sched_(*(b.t for b in bufs), lr_dev, _args(LP.KINDS[kind]), b1, b2, eps, wd, 7, bc, 7, cnt, lr_out=out.t)
            got = float(out.t)
            ref, bound = LP.lr_bound(LP.KINDS[kind], lr, t)
            print(f"{kind} t={t}: lr_out {got:.9e}, fp64 {ref:.9e}, off by {abs(got - ref):.2e}, bound {bound:.2e}")
            assert abs(got - ref) <= bound, (kind, t, got, ref, bound)
            got_all.append(got)
            if abs(ref - at7) > 1e-3 * lr:
                assert abs(got - at7) > 100 * bound
                told += 1
        assert told >= 3 and len(set(got_all)) >= 4, "lr_out does not move with the device count"
        assert all(b.untouched() for b in bufs + [out])
    finally:
        _free()


def test_lr_out_long_cosine_and_fallback_counts():
    """cosine at T = 100000, t = 60001; and the count's fallbacks: sched_step_dev NULL -> the host sched_step; both unset ->
    the update's own count (step_dev first, then step)."""
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    try:
        bufs = _state(5, 0, _gen("sched-long"))
        out = FlatGuard(1, torch.float32)
        lr_dev = _dev(lr, torch.float32)
        args, t = LP.LONG
        ops.adamw_sched_(*(b.t for b in bufs), lr_dev, _args(args), b1, b2, eps, wd, 7, None, 7, _dev(t, torch.int32), lr_out=out.t)
        ref, bound = LP.lr_bound(args, lr, t)
        print(f"long cosine t={t}: lr_out {float(out.t):.9e}, fp64 {ref:.9e}, bound {bound:.2e}")
        assert abs(float(out.t) - ref) <= bound
        for kw, t in ((dict(step=9, step_dev=None, sched_step=5), 5), (dict(step=9, step_dev=_dev(6, torch.int32)), 6),
                      (dict(step=9, step_dev=None), 9)):
            ops.adamw_sched_(*(b.t for b in bufs), lr_dev, _args(COS), b1, b2, eps, wd, lr_out=out.t, **kw)
            ref, bound = LP.lr_bound(COS, lr, t)
            assert abs(float(out.t) - ref) <= bound, (kw, float(out.t), ref)
        assert all(b.untouched() for b in bufs + [out])
    finally:
        _free()


# ---- the uniform case is the existing kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LP.CASES, ids=lambda c: c[0])
def test_uniform_is_adamw_at_lr_out(case):
    """n_segs = 0, lr_scale = 1, three updates through the warm-up into the cosine: p, m, v bitwise coma_adamw's with
    lr = float(lr_out) at the same device step; the last update with the bias-correction count (5) apart from the schedule's
    (4), which lr_out must follow."""
    ops = _ops()
    name, n, off = case
    lr, b1, b2, eps, wd = HP
    try:
        ref = _state(n, off, _gen("sched-uni", name))
        new = _state(n, off, _gen("sched-uni", name))
        assert all((b.t.data_ptr() % 16 == 0) == (off == 0) for b in new)
        out = FlatGuard(1, torch.float32)
        lr_dev, step_dev, cnt = _dev(lr, torch.float32), _dev(0, torch.int32), _dev(0, torch.int32)
        gen = _gen("sched-uni-g", name)
        seen = []
        for t, ts in ((1, 1), (3, 3), (5, 4)):
            gr = torch.randn(n, generator=gen, device="cuda")
            ref[1].t.copy_(gr)
            new[1].t.copy_(gr)
            step_dev.fill_(t)
            cnt.fill_(ts)
            before = new[0].t.clone()
            ops.adamw_sched_(*(b.t for b in new), lr_dev, _args(COS), b1, b2, eps, wd, 7, step_dev, 7, cnt, lr_out=out.t)
            lr_t = float(out.t)
            want, bound = LP.lr_bound(COS, lr, ts)
            assert abs(lr_t - want) <= bound
            seen.append(lr_t)
            _adamw(*(b.t for b in ref), lr_t, b1, b2, eps, wd, 7, step_dev)
            for nm, a, b_ in zip("pgmv", ref, new):
                assert torch.equal(a.t, b_.t), f"{nm} update {t}: coma_adamw_sched differs from coma_adamw at lr_out"
            assert not torch.equal(new[0].t, before)
        assert len(set(seen)) == 3
        assert all(b.untouched() for b in ref + new + [out])
    finally:
        _free()


@pytest.mark.parametrize("case", LP.CASES, ids=lambda c: c[0])
def test_uniform_with_counter_and_clip_is_adamw_ex_and_with_average_adamw_ema(case):
    """A counter of 3 and a clip that bites, device step count, three updates: p, m, v and norm_out bitwise coma_adamw_ex's;
    with the average also e, bitwise coma_adamw_ema's."""
    ops = _ops()
    name, n, off = case
    lr, b1, b2, eps, wd = HP
    K = 3
    try:
        ref = _state(n, off, _gen("sched-ex", name))
        new = _state(n, off, _gen("sched-ex", name))
        ref_e = _state(n, off, _gen("sched-ema", name), bufs=5)
        new_e = _state(n, off, _gen("sched-ema", name), bufs=5)
        parts = FlatGuard(ops.ACC_PARTIALS, torch.float64, fill=float("nan"))
        norms = [FlatGuard(1, torch.float32) for _ in range(4)]
        out = FlatGuard(1, torch.float32)
        count, step_dev, lr_dev = _dev(K, torch.int32), _dev(0, torch.int32), _dev(lr, torch.float32)
        gen = _gen("sched-ex-g", name)
        for t in (1, 2, 3):
            gr = torch.randn(n, generator=gen, device="cuda") * (3.0 if t == 2 else 1.0)
            for s in (ref, new, ref_e, new_e):
                s[1].t.copy_(gr)
            step_dev.fill_(t)
            max_norm = NP.f32(0.5 * float((gr.double() ** 2).sum()) ** 0.5 / K)
            parts.t.fill_(float("nan"))
            nb = ops.grad_accum_(None, ref[1].t, None, parts.t)
            window = (count, parts.t, nb, None, max_norm)
            ops.adamw_sched_(*(b.t for b in new), lr_dev, _args(COS), b1, b2, eps, wd, 7, step_dev, lr_out=out.t,
                             count_dev=count, partials=parts.t, n_partials=nb, max_norm=max_norm, norm_out=norms[1].t)
            lr_t = float(out.t)
            assert abs(lr_t - LP.lr_bound(COS, lr, t)[0]) <= LP.lr_bound(COS, lr, t)[1]
            ops.adamw_ex_(*(b.t for b in ref), lr_t, b1, b2, eps, wd, 7, step_dev, *window, norms[0].t)
            for nm, a, b_ in zip(("p", "g", "m", "v", "norm_out"), ref + [norms[0]], new + [norms[1]]):
                assert torch.equal(a.t, b_.t), f"{nm} update {t}: coma_adamw_sched differs from coma_adamw_ex"
            p, g, m, v, e = (b.t for b in new_e)
            ops.adamw_sched_(p, g, m, v, lr_dev, _args(COS), b1, b2, eps, wd, 7, step_dev, lr_out=out.t, ema=e, ema_decay=0.9,
                             ema_warmup=True, count_dev=count, partials=parts.t, n_partials=nb, max_norm=max_norm,
                             norm_out=norms[3].t)
            assert float(out.t) == lr_t
            p, g, m, v, e = (b.t for b in ref_e)
            ops.adamw_ema_(p, g, m, v, e, 0.9, True, lr_t, b1, b2, eps, wd, 7, step_dev, *window, norms[2].t)
            for nm, a, b_ in zip(("p", "g", "m", "v", "e", "norm_out"), ref_e + [norms[2]], new_e + [norms[3]]):
                assert torch.equal(a.t, b_.t), f"{nm} update {t}: coma_adamw_sched differs from coma_adamw_ema"
            assert float(norms[1].t) > max_norm                                   # the clip bit
        assert all(b.untouched() for b in ref + new + ref_e + new_e + norms + [out]) and int(count) == K
    finally:
        _free()


# ---- segments -----------------------------------------------------------------------------------------------------------------
def _alone(snap, lo, hi, aligned, lr_dev, scale, wd, t_dev):
    """The same entry point on [lo, hi) of the snapshot alone, n_segs = 0, in buffers that are (not) 16-byte aligned."""
    ops = _ops()
    lr, b1, b2, eps, _ = HP
    bufs = [FlatGuard(hi - lo, torch.float32, 0 if aligned else 1) for _ in range(4)]
    for b, s in zip(bufs, snap):
        b.t.copy_(s[lo:hi])
    ops.adamw_sched_(*(b.t for b in bufs), lr_dev, _args(COS), b1, b2, eps, wd, 7, t_dev, lr_scale=scale)
    assert all(b.untouched() for b in bufs)
    return bufs


def _check_segments(got, snap, ends, scales, wds, body_end, base, lr_dev, t_dev, what):
    """got / snap: p, g, m, v after / before the call on the elements [base, base + n) of the flat coordinates; body_end: where
    the call's 16-byte loop ends (call coordinates; 0: the whole call is on the scalar loop)."""
    n = got[0].numel()
    lo_flat = 0
    for k, (end, scale, wd) in enumerate(zip(ends, scales, wds)):
        lo, hi = max(lo_flat - base, 0), min(end - base, n)
        lo_flat = end
        if hi <= lo:
            continue
        parts = []                                        # (lo, hi, window lo, window hi, aligned)
        if lo < body_end:
            b_hi = min(hi, body_end)
            parts.append((lo, b_hi, lo // 4 * 4, min(-(-b_hi // 4) * 4, body_end), True))
        if hi > body_end:
            s_lo = max(lo, body_end)
            parts.append((s_lo, hi, s_lo, hi, False))
        for a, b, wa, wb, aligned in parts:
            ref = _alone(snap, wa, wb, aligned, lr_dev, scale, wd, t_dev)
            for nm, j in (("p", 0), ("m", 2), ("v", 3)):
                assert torch.equal(got[j][a:b], ref[j].t[a - wa:b - wa]), \
                    f"{what}: {nm} of segment {k} [{lo + base}, {hi + base}) (scale {scale}, wd {wd}) differs on [{a}, {b})"
            if scale == 0.0 and wd == 0.0:
                assert torch.equal(got[0][a:b], snap[0][a:b])
        assert torch.equal(got[1][lo:hi], snap[1][lo:hi])
    assert lo_flat - base >= n


def _table(ends, scales, wds):
    return (torch.tensor(ends, dtype=torch.int64, device="cuda"), torch.tensor(scales, dtype=torch.float32, device="cuda"),
            torch.tensor(wds, dtype=torch.float32, device="cuda"))


def test_segments_take_their_own_scale_and_decay():
    """Boundaries inside and at the edge of the first chunk, between two blocks' chunks, segments of 1, 1, 2 elements inside one
    chunk, one just past the first grid pass and one inside the scalar tail; scales and decays distinct, a scale of 0 and a
    decay of 0 among them.  Then the same table on the slice [5:] with elem_base = 5: the unaligned (scalar) path."""
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    name, n, off = LP.CASES[1]
    assert name == "vec4" and off == 0
    try:
        ends = LP.segment_ends(n)
        scales, wds = LP.segment_options(len(ends))
        tab = _table(ends, scales, wds)
        lr_dev, t_dev = _dev(lr, torch.float32), _dev(5, torch.int32)
        out = FlatGuard(1, torch.float32)
        for base in (0, 5):
            st = _state(n, 0, _gen("sched-seg", base))
            snap = [b.t.clone() for b in st]
            view = [b.t[base:] for b in st]
            assert (view[0].data_ptr() % 16 == 0) == (base == 0)
            ops.adamw_sched_(*view, lr_dev, _args(COS), b1, b2, eps, 123.0, 7, t_dev, lr_scale=77.0, segs=tab, elem_base=base,
                             lr_out=out.t)                 # (with a table the uniform scale and decay must not be looked at)
            assert abs(float(out.t) - LP.lr_bound(COS, lr, 5)[0]) <= LP.lr_bound(COS, lr, 5)[1]
            for b, s in zip(st, snap):
                assert torch.equal(b.t[:base], s[:base]) and b.untouched()
            body_end = (n // 4) * 4 if base == 0 else 0
            _check_segments(view, [s[base:] for s in snap], ends, scales, wds, body_end, base, lr_dev, t_dev, f"elem_base {base}")
    finally:
        _free()


def test_longest_table_and_what_is_refused():
    """MAX_SEGS segments of 3 elements on n = 3 * MAX_SEGS (every chunk straddles a boundary): five distinct options in turn,
    each element bitwise the whole buffer run uniformly with its segment's options (the same loop for every element).  One
    segment more, T = 0, gamma = 0, an unknown kind and a null lr_dev are refused with nothing touched; n = 0 writes
    nothing."""
    from coma_unet_amd._lib import ComaError
    ops = _ops()
    lr, b1, b2, eps, wd = HP
    M = ops.MAX_SEGS
    n = 3 * M
    try:
        opts = [(1.0, 1e-2), (0.0, 0.0), (0.5, 0.2), (2.0, 0.0), (0.25, 0.05)]
        ends = [3 * (k + 1) for k in range(M)]
        tab = _table(ends, [opts[k % 5][0] for k in range(M)], [opts[k % 5][1] for k in range(M)])
        lr_dev, t_dev = _dev(lr, torch.float32), _dev(6, torch.int32)
        st = _state(n, 0, _gen("sched-max"))
        snap = [b.t.clone() for b in st]
        lr_out = FlatGuard(1, torch.float32)
        ops.adamw_sched_(*(b.t for b in st), lr_dev, _args(COS), b1, b2, eps, wd, 7, t_dev, segs=tab, lr_out=lr_out.t)
        lr_t = np.float32(float(lr_out.t))
        seg = torch.arange(n, device="cuda") // 3 % 5
        for j, (scale, w) in enumerate(opts):
            ref = _alone(snap, 0, n, True, lr_dev, scale, w, t_dev)
            # and, independent of the entry point under test: coma_adamw at lr = fp32(lr_out) * fp32(scale) with the segment's decay
            old = [x.clone() for x in snap]
            _adamw(*old, float(lr_t * np.float32(scale)), b1, b2, eps, w, 7, t_dev)
            for nm, i in (("p", 0), ("m", 2), ("v", 3)):
                assert torch.equal(st[i].t[seg == j], ref[i].t[seg == j]), f"{nm}: segments with options {j}"
                assert torch.equal(st[i].t[seg == j], old[i][seg == j]), f"{nm}: segments with options {j} against coma_adamw"
        assert lr_out.untouched()
        assert torch.equal(st[0].t[seg == 1], snap[0][seg == 1]) and not torch.equal(st[0].t[seg == 0], snap[0][seg == 0])
        assert all(b.untouched() for b in st)

        keep = [b.flat.clone() for b in st]
        out = FlatGuard(1, torch.float32)
        big = _table(ends + [n + 3], [1.0] * (M + 1), [0.0] * (M + 1))
        p, g, m, v = (b.t for b in st)
        cos0 = (1, 0, 1.0, 0, 0.0, 1, 0.1)
        bad = [(dict(segs=big), _args(COS), lr_dev, "segments"), (dict(), cos0, lr_dev, "total_steps"),
               (dict(), (2, 0, 1.0, 0, 0.0, 1, 0.1), lr_dev, "total_steps"), (dict(), (3, 0, 1.0, 1, 0.0, 1, 0.0), lr_dev, "gamma"),
               (dict(), (0, 0, 1.0, 1, 0.0, 0, 0.1), lr_dev, "step_size"), (dict(), (4, 0, 1.0, 1, 0.0, 1, 0.1), lr_dev, "kind"),
               (dict(), (-1, 0, 1.0, 1, 0.0, 1, 0.1), lr_dev, "kind"), (dict(), (0, -1, 1.0, 1, 0.0, 1, 0.1), lr_dev, "warmup_steps"),
               (dict(), (0, 0, 0.0, 1, 0.0, 1, 0.1), lr_dev, "warmup_start"), (dict(), (0, 0, 1.0, 1, 1.5, 1, 0.1), lr_dev, "min_ratio"),
               (dict(), _args(COS), None, "lr_dev")]
        for kw, args, lrd, msg in bad:
            with pytest.raises(ComaError, match=msg):
                ops.adamw_sched_(p, g, m, v, lrd, args, b1, b2, eps, wd, 7, t_dev, lr_out=out.t, **kw)
        z = [b.t[4:4] for b in st]                                         # zero-length slices in the middle of live buffers
        ops.adamw_sched_(*z, lr_dev, _args(COS), b1, b2, eps, wd, 7, t_dev, segs=tab, lr_out=out.t)
        torch.cuda.synchronize()
        assert all(torch.equal(b.flat, k) for b, k in zip(st, keep)) and bool((out.flat == SENT).all())
    finally:
        _free()
