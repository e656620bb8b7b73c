"""The scratch contract of the convolution entry points (coma_conv_fwd_ws, coma_conv_fwd_norm_stats, coma_conv_wgrad, and
the scratch-less coma_conv_fwd) through the C ABI: every launcher that picks its code path from the size of the `ws` it is
handed -- launch_gather's split-K merge, duo_takes' re-laid weights, the replica merge of the six weight-gradient launchers
behind wgrad_replicas, the bias gradient's partial rows -- with a scratch of EXACTLY the queried size (dirty, and
caller-zeroed under COMA_ZEROED_WS / COMA_ZEROED_OUT), four bytes short of it, absent, and misaligned.

The shapes come from tests/_conv_ws_plan.py (test_conv_ws_cpu.py asserts that each crosses the boundary it is listed for).
Outputs live in sentinel guards, inputs in pitched buffers whose foreign lanes hold finite garbage, and the scratch is a
byte buffer whose live extent is the queried size, filled with 0xFF (NaN as fp32 and as bf16), behind and in front of
sentinel bytes (64 KiB behind).  Whatever size is DECLARED to the library, the physical extent is never below the query's
answer.  A scratch-using path is recognised by what it leaves behind: no 0xFFFFFFFF word in the bytes its query names and
not one changed byte beyond them; a scratch-less path leaves every byte as it was.

Every element of every output is held to the worst-case bound of oracle/fp64_ref.py: |got - ref| <= u_out |ref| +
2 K 2^-24 A (+ u_out |base|), A the same operation on absolute values, K the accumulated terms (taps * Cin; voxels (* B when
batch-summed) + the 64-replica fold for a weight gradient), which holds for any summation order -- so one bound serves
every mode.  The algo-6 split kernel adds its 2^-14 term (tests/_split_abi.py).  Fused or separate statistics: mean within
1e-5 (1 + max |mean|) and rstd within 1e-5 rel-L2 of the fp64 statistics of the stored output (test_ops_gpu.py).
The worst ratio and the path of every case and mode are printed (test_zz_report: rows "ROW")."""
import math

import pytest
import torch

import _conv_ws_plan as P
from _split_abi import _bound as split_bound
from _split_abi import _free, _gen, _ops
from oracle import fp64_ref as R
from test_nonconv_sizes_gpu import FlatGuard, Guard, _pitched

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FILL = 0xFF
REPORT = {}
_PROBLEMS = {}


def _u(dt):
    return R.U_BF16 if dt == "bf16" else R.U_F32


def _pad(dt):           # extra channels of pitch: a 16-byte piece
    return 8 if dt == "bf16" else 4


def _put(name, **kv):
    REPORT[name] = kv
    print("conv_ws", name, {a: (float(f"{b:.4g}") if isinstance(b, float) else b) for a, b in kv.items()})


class Scratch:
    """A byte buffer [64 sentinel | live | 64 KiB sentinel | 4096 sentinel] at byte offset `off` of a 16-byte boundary; the
    live extent (the queried size) holds `fill`, the rest 0xFF."""

    def __init__(self, live, fill=FILL, off=0):
        self.live, self.fill = int(live), fill
        self.g = FlatGuard(self.live + P.TAIL, torch.uint8, off, fill=FILL)
        self.g.t[:self.live] = fill
        self.ptr = self.g.t.data_ptr()
        assert self.ptr % 16 == off % 16

    def outside_intact(self):
        return self.g.untouched() and bool((self.g.t[self.live:] == FILL).all())

    def extent(self):
        """one past the last live byte that no longer holds the fill (0: untouched)"""
        m = self.g.t[:self.live] != self.fill
        return int(m.nonzero()[-1]) + 1 if bool(m.any()) else 0

    def words_rewritten(self, nbytes):
        """no 4-byte word of the first nbytes still holds the 0xFF fill"""
        return not bool((self.g.t[:nbytes].view(torch.int32) == -1).any())


def _stats_check(rec, G, C, y, instance, what):
    ops, L = _ops()
    V = y.shape[1] * y.shape[2] * y.shape[3]
    mean, rstd = ops.stats_from_sums(rec, G, C, V * (1 if instance else y.shape[0]), 1e-5)
    yf = y.double()
    red = (1, 2, 3) if instance else (0, 1, 2, 3)
    m_ref = yf.mean(red).reshape(mean.shape)
    r_ref = (yf.var(red, unbiased=False).reshape(mean.shape) + 1e-5).rsqrt()
    em = float((mean.double() - m_ref).abs().max()) / (1e-5 * (1.0 + float(m_ref.abs().max())))
    er = float((rstd.double() - r_ref).norm() / r_ref.norm()) / 1e-5
    assert em < 1.0 and er < 1.0, (what, em, er)
    return max(em, er)


# ---------------------------------------------------------------------------------------------------------------------
# forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------
def _fwd_problem(c):
    """Operands and the fp64 reference of a forward case, made once."""
    if c.name in _PROBLEMS:
        return _PROBLEMS[c.name]
    dtype, gen = DT[c.dt], _gen("conv_ws", c.name)
    od, taps, Bw = P.out_dims(c.dims, c.k, c.stride, c.form), c.k ** 3, c.B if c.ps else 1
    xs = torch.randn((c.B, *c.dims, c.cin), generator=gen, device="cuda").to(dtype)
    x = _pitched((c.B, *c.dims, c.cin), c.cin + _pad(c.dt), dtype, xs)
    wk = (torch.randn((Bw, taps, c.cout, c.cin), generator=gen, device="cuda") / math.sqrt(taps * c.cin)).to(dtype).contiguous()
    bias = (torch.randn((c.B, c.cout) if c.ps else (c.cout,), generator=gen, device="cuda") * 0.5).contiguous()
    base = torch.randn((c.B, *od, c.cout), generator=gen, device="cuda").to(dtype)
    ref0, A0 = R.conv_fwd(x.double(), wk.double(), None, c.k, c.stride, c.form == 1)
    bv = bias.double().view(c.B if c.ps else 1, 1, 1, 1, c.cout)
    pr = dict(x=x, wk=wk, bias=bias, base=base, od=od, ref=ref0 + bv, A=A0 + bv.abs(), K=taps * c.cin)
    _PROBLEMS[c.name] = pr
    return pr


def _fwd_call(c, pr, ws_ptr, declared, flags, entry="ws", norm=None, accumulate=False):
    """-> (y guard, statistics guard or None, kernel name)"""
    ops, L = _ops()
    dtype = DT[c.dt]
    y = Guard((c.B, *pr["od"], c.cout), dtype, c.cout + 2 * _pad(c.dt), _pad(c.dt))
    if accumulate:
        y.t.copy_(pr["base"])
        flags |= L.ACCUMULATE
    d = ops._desc(c.k, c.stride, c.form, c.ps, 0)
    cx, cy, wd = L.ct(pr["x"]), L.ct(y.t), L.dtype_code(dtype)
    rec = None
    if norm is not None:
        G = c.B if norm == L.NORM_INSTANCE else 1
        shape = ops.stat_record(G, c.cout, 2, "cuda").shape
        assert shape == (P.STAT_REPLICAS, (G * c.cout * 2 + 7) & ~7)
        rec = FlatGuard(shape[0] * shape[1], torch.float64)
        rec.t.zero_()
        rec.rows = rec.t.view(shape)
        L.check(L.lib.coma_conv_fwd_norm_stats(d, cx, L.ptr(pr["wk"]), wd, L.ptr(pr["bias"]), cy, norm, L.ptr(rec.t), ws_ptr,
                                               declared, flags, L.stream()), "coma_conv_fwd_norm_stats")
    elif entry == "null":
        L.check(L.lib.coma_conv_fwd(d, cx, L.ptr(pr["wk"]), wd, L.ptr(pr["bias"]), cy, L.stream()), "coma_conv_fwd")
    else:
        L.check(L.lib.coma_conv_fwd_ws(d, cx, L.ptr(pr["wk"]), wd, L.ptr(pr["bias"]), cy, ws_ptr, declared, flags, L.stream()),
                "coma_conv_fwd_ws")
    return y, rec, L.lib.coma_last_kernel().decode()


@pytest.mark.parametrize("c", P.FWD_CASES, ids=lambda c: c.name)
def test_forward_scratch_modes(c):
    """coma_conv_fwd_ws / coma_conv_fwd / coma_conv_fwd_norm_stats on every forward case: exact dirty, exact caller-zeroed,
    four bytes short, declared 0, NULL (coma_conv_fwd), misaligned (duo); with a bias everywhere, COMA_ACCUMULATE onto a
    Gaussian base on the gather cases (exact and short), the statistics of both norm modes (exact and absent)."""
    ops, L = _ops()
    try:
        pr = _fwd_problem(c)
        d = ops._desc(c.k, c.stride, c.form, c.ps, 0)
        probe = Guard((c.B, *pr["od"], c.cout), DT[c.dt], c.cout + 2 * _pad(c.dt), _pad(c.dt))
        cx, cy = L.ct(pr["x"]), L.ct(probe.t)
        nws = L.lib.coma_conv_fwd_ws_bytes(d, cx, cy)
        assert nws == P.fwd_ws_bytes(c) and L.lib.coma_conv_pick_algo(d, cx, cy) == (2 if c.dt == "bf16" else 3), nws
        assert (L.lib.coma_conv_wk_frag_bytes(d, cx, cy) > 0) == (c.kind == "duo")
        assert L.lib.coma_conv_accumulate_ok(d, cx, cy) == (1 if c.kind == "gather" else 0)
        del probe
        live = nws if nws else 1 << 16            # (the control case: a scratch is offered although none is asked for)
        unused_kernel = {"gather": "conv_mfma_gather_k<", "duo": "conv_mfma_halo2_k<", "none": "conv_mfma_duo_k<"}[c.kind]
        used_kernel = {"gather": "conv_mfma_gather_k<", "duo": "conv_mfma_duo_k<", "none": "conv_mfma_duo_k<"}[c.kind]
        # (mode, fill, declared, flags, entry, offset, scratch used)
        modes = [("exact-dirty", FILL, live, 0, "ws", 0, nws > 0), ("exact-zeroed", 0, live, L.ZEROED_WS, "ws", 0, nws > 0)]
        if nws:
            modes.append(("short", FILL, nws - 4, 0, "ws", 0, False))
        modes += [("none", FILL, 0, 0, "ws", 0, False), ("null", FILL, 0, 0, "null", 0, False)]
        if c.kind == "duo":
            modes.append(("misaligned", FILL, nws, 0, "ws", 4, False))
        st = {}

        def outcome(mode, ws, y, kernel, used, ref, base=None, stats=False):
            what = f"{c.name} {mode}"
            if kernel.startswith("conv_mfma_duo_k<"):      # <1, LX>: the instance that fuses the statistics
                assert kernel.startswith("conv_mfma_duo_k<1" if stats else "conv_mfma_duo_k<0"), (what, kernel)
            st[mode] = R.check_elementwise(y.t, ref, R.elem_bound(ref, pr["A"], pr["K"], _u(c.dt), base), what)
            assert y.untouched(), what + ": wrote outside y"
            assert ws.outside_intact(), what + ": wrote outside the queried scratch"
            if used:
                assert kernel.startswith(used_kernel), (what, kernel)
                assert ws.extent() > 0, what + ": the scratch path did not run"
                if ws.fill == FILL:
                    assert ws.words_rewritten(nws), what + ": part of the queried scratch was never written"
            else:
                assert kernel.startswith(unused_kernel), (what, kernel)
                assert ws.extent() == 0, what + ": the scratch was touched on the scratch-less path"
            st[mode + "-path"] = ("ws " if used else "no-ws ") + kernel

        for mode, fill, declared, flags, entry, off, used in modes:
            ws = Scratch(live, fill, off)
            y, _, kernel = _fwd_call(c, pr, ws.ptr, declared, flags, entry)
            outcome(mode, ws, y, kernel, used, pr["ref"])
            del ws, y
        if c.kind == "gather":
            base = pr["base"].double()
            for mode, declared, used in (("accum-exact", nws, True), ("accum-short", nws - 4, False)):
                ws = Scratch(live)
                y, _, kernel = _fwd_call(c, pr, ws.ptr, declared, 0, accumulate=True)
                outcome(mode, ws, y, kernel, used, pr["ref"] + base, base)
                del ws, y
        for nm, norm in (("batch", L.NORM_BATCH), ("instance", L.NORM_INSTANCE)):
            for mode, declared, used in ((f"stats-{nm}-exact", live, nws > 0), (f"stats-{nm}-none", 0, False)):
                ws = Scratch(live)
                y, rec, kernel = _fwd_call(c, pr, ws.ptr, declared, 0, norm=norm)
                outcome(mode, ws, y, kernel, used, pr["ref"], stats=True)
                G = c.B if norm == L.NORM_INSTANCE else 1
                st[mode + "-stats"] = _stats_check(rec.rows, G, c.cout, y.t, norm == L.NORM_INSTANCE, f"{c.name} {mode}")
                assert rec.untouched(), mode + ": wrote outside the statistics record"
                assert not bool(rec.rows[:, G * c.cout * 2:].any()), mode + ": padding of the statistics record written"
                if c.kind == "gather":
                    st[mode + "-path"] += " + separate statistics pass" if used else " + fused statistics"
                del ws, y, rec
        _put(f"fwd-{c.name}", **st)
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_problem(c):
    if c.name in _PROBLEMS:
        return _PROBLEMS[c.name]
    dtype, gen = DT[c.dt], _gen("conv_ws", c.name)
    xs = torch.randn((c.B, *c.dims, c.cin), generator=gen, device="cuda").to(dtype)
    ds = torch.randn((c.B, *c.dims, c.cout), generator=gen, device="cuda").to(dtype)
    x = _pitched((c.B, *c.dims, c.cin), c.cin + _pad(c.dt), dtype, xs)
    dy = _pitched((c.B, *c.dims, c.cout), c.cout + _pad(c.dt), dtype, ds)
    ref, A = R.conv_wgrad(x.double(), dy.double(), c.k, c.stride, c.form == 1, c.ps)
    red = (1, 2, 3) if c.ps else (0, 1, 2, 3)
    pr = dict(x=x, dy=dy, ref=ref.reshape(-1), A=A.reshape(-1), K=P.wgrad_K(c), bref=dy.double().sum(red).reshape(-1),
              bA=dy.double().abs().sum(red).reshape(-1), bK=P.vol(c.dims) * (1 if c.ps else c.B))
    _PROBLEMS[c.name] = pr
    return pr


@pytest.mark.parametrize("with_dbias", [False, True], ids=["dw", "dw+dbias"])
@pytest.mark.parametrize("c", P.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_scratch_modes(c, with_dbias):
    """coma_conv_wgrad on every weight-gradient case.  By the header's contract, with `declared` bytes of scratch: a bias
    gradient with less than coma_norm_ws_bytes is refused and nothing is written; the blocks merge into replicas exactly when
    the case allows them (wsz <= 16384) and declared >= 4 * wsz * 64, else straight into dwk; COMA_ZEROED_WS speaks about the
    scratch, COMA_ZEROED_OUT about dwk, each on the branch that uses it, and a bias gradient voids COMA_ZEROED_WS."""
    ops, L = _ops()
    try:
        pr = _wgrad_problem(c)
        d = ops._desc(c.k, c.stride, c.form, c.ps, c.algo)
        cx, cdy = L.ct(pr["x"]), L.ct(pr["dy"])
        wsz = P.wgrad_out_elems(c)
        nws, nzs, nnorm = (L.lib.coma_conv_wgrad_ws_bytes(d, cx, cdy), L.lib.coma_conv_wgrad_zs_bytes(d, cx, cdy),
                           L.lib.coma_norm_ws_bytes(cdy))
        rep_bytes = 4 * wsz * P.WGRAD_NREP
        assert nws == P.wgrad_ws_bytes(c) and nzs == P.conv_mfma_wgrad_ws_bytes(c) == (rep_bytes if c.rep else 0)
        assert nnorm == P.norm_ws_bytes(c.cout)
        # beyond the threshold the query names no replica bytes: offer them all the same, they must stay untouched
        roomy = nws if c.rep else max(nws, rep_bytes)
        nb = (c.B if c.ps else 1) * c.cout
        Z = L.ZEROED_WS | L.ZEROED_OUT
        # (mode, live extent, fill, declared, flags)
        modes = [("exact-dirty", roomy, FILL, roomy, 0), ("short", roomy, FILL, nws - 4, 0), ("none", roomy, FILL, 0, 0),
                 ("short-zeroed-ws", roomy, 0, nws - 4, L.ZEROED_WS)]
        if c.rep and rep_bytes - 4 != nws - 4:
            modes.append(("short-of-replicas", roomy, FILL, rep_bytes - 4, 0))
        zlive = roomy if with_dbias or not c.rep else nzs          # dbias == NULL: ws is just the replica scratch (ops._conv_bwd)
        modes += [("zeroed-ws+out", zlive, 0, zlive, Z), ("zeroed-ws", zlive, 0, zlive, L.ZEROED_WS), ("zeroed-out", zlive, FILL, zlive, L.ZEROED_OUT)]
        st = {}
        for mode, live, fill, declared, flags in modes:
            what = f"{c.name} {'dw+dbias' if with_dbias else 'dw'} {mode}"
            ws = Scratch(live, fill)
            dwk, dbias = FlatGuard(wsz, torch.float32), FlatGuard(nb, torch.float32)
            if flags & L.ZEROED_OUT:
                dwk.t.zero_()
            rc = L.lib.coma_conv_wgrad(d, cx, cdy, L.ptr(dwk.t), L.ptr(dbias.t) if with_dbias else None, ws.ptr, declared, flags, L.stream())
            torch.cuda.synchronize()
            assert dwk.untouched() and dbias.untouched() and ws.outside_intact(), what + ": wrote outside its buffers"
            if with_dbias and declared < nnorm:
                assert rc != 0 and L.lib.coma_last_error().decode(), what + ": a bias gradient without its scratch must be refused"
                assert bool((dwk.t == dwk.fill).all()) and bool((dbias.t == dbias.fill).all()) and ws.extent() == 0, what + ": refused, yet something was written"
                st[mode + "-path"] = "refused"
                continue
            L.check(rc, what)
            kernel = L.lib.coma_last_kernel().decode()
            assert kernel.startswith(c.kernel), (what, kernel)
            if c.algo == 6:
                bound = split_bound(pr["ref"], pr["A"], pr["K"])
            else:
                bound = R.elem_bound(pr["ref"], pr["A"], pr["K"], u_out=R.U_F32)
            st[mode] = R.check_elementwise(dwk.t, pr["ref"], bound, what + " dwk")
            if with_dbias:
                st[mode + "-dbias"] = R.check_elementwise(dbias.t, pr["bref"], R.elem_bound(pr["bref"], pr["bA"], pr["bK"], u_out=R.U_F32), what + " dbias")
            else:
                assert bool((dbias.t == dbias.fill).all())
            used = c.rep and declared >= rep_bytes
            reach = max(rep_bytes if used else 0, nnorm if with_dbias else 0)       # the bytes this call may write
            ext = ws.extent()
            assert ext <= reach, what + f": scratch written up to byte {ext}, the call owns {reach}"
            if used:
                assert ext > 0, what + ": the replica path did not run"
                if fill == FILL:
                    assert ws.words_rewritten(rep_bytes), what + ": part of the replica scratch was never cleared"
            st[mode + "-path"] = ("replicas" if used else "atomics into dwk") + (" + bias rows" if with_dbias else "")
            del ws, dwk, dbias
        _put(f"wgrad-{c.name}-{'dbias' if with_dbias else 'nobias'}", kernel=c.kernel, **st)
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# the production path: scratch, statistics records and weight gradients as slices of ops.ZeroArena
# ---------------------------------------------------------------------------------------------------------------------
def _layer(name):
    c = P.FWD.get(name) or P.WGRAD[name]
    return c.dt, c.cin, c.cout, c.dims, c.B


def _arena_layer(name):
    """fp64 references of one stride-1 3x3x3 layer with shared weights (forward with bias, data gradient, weight and bias
    gradient), made once; operands contiguous, as the model holds them."""
    key = "arena-" + name
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    ops, L = _ops()
    dt, cin, cout, dims, B = _layer(name)
    dtype, gen = DT[dt], _gen("conv_ws arena", name)
    x = torch.randn((B, *dims, cin), generator=gen, device="cuda").to(dtype)
    dy = torch.randn((B, *dims, cout), generator=gen, device="cuda").to(dtype)
    a_f, a_d = ops.pick_algo(x.shape, dtype, cout, 3, 1, False, False, x.device, 0)
    assert a_f == a_d == (2 if dt == "bf16" else 3)
    wk_f = (torch.randn((1, 27, cout, cin), generator=gen, device="cuda") / math.sqrt(27 * cin)).to(dtype).contiguous()
    wk_d = wk_f.transpose(2, 3).contiguous()
    bias = torch.randn((cout,), generator=gen, device="cuda") * 0.5
    y, Ay = R.conv_fwd(x.double(), wk_f.double(), bias.double(), 3, 1, False)
    dx, Adx = R.conv_dgrad(dy.double(), wk_f.double(), dims, 3, 1, False)
    dw, Adw = R.conv_wgrad(x.double(), dy.double(), 3, 1, False, False)
    pr = dict(dt=dt, cin=cin, cout=cout, dims=dims, B=B, x=x, dy=dy, wk_f=wk_f, wk_d=wk_d, bias=bias, y=y, Ay=Ay, dx=dx, Adx=Adx,
              dw=dw, Adw=Adw, db=dy.double().sum((0, 1, 2, 3)), Adb=dy.double().abs().sum((0, 1, 2, 3)))
    _PROBLEMS[key] = pr
    return pr


def _arena_step(name, arena):
    """One layer forward (plain and with the statistics of a BatchNorm) and backward (dx + dw, without and with a bias
    gradient) through ops._conv_fwd / ops._conv_bwd inside an armed step; -> worst ratios.  Ends the step itself."""
    ops, L = _ops()
    pr = _arena_layer(name)
    u, V, st = _u(pr["dt"]), P.vol(pr["dims"]), {}
    ops.ZeroArena.begin_step()
    assert arena.armed and arena.cur == 0
    y, _ = ops._conv_fwd(pr["x"], pr["wk_f"], pr["bias"], 3, 1, 0, False, 0, None, None)
    st["y"] = R.check_elementwise(y, pr["y"], R.elem_bound(pr["y"], pr["Ay"], 27 * pr["cin"], u), name + " y")
    st["fwd"] = L.lib.coma_last_kernel().decode()
    y, sums = ops._conv_fwd(pr["x"], pr["wk_f"], pr["bias"], 3, 1, 0, False, 0, None, L.NORM_BATCH)
    st["y-norm"] = R.check_elementwise(y, pr["y"], R.elem_bound(pr["y"], pr["Ay"], 27 * pr["cin"], u), name + " y (norm)")
    st["stats"] = _stats_check(sums, 1, pr["cout"], y, False, name)
    for bias_mode in (0, 1):
        dx, dwk, dbias = ops._conv_bwd(pr["x"], pr["wk_d"], pr["dy"], 3, 1, 0, False, 0, (1, 27, pr["cout"], pr["cin"]), True, True,
                                       bias_mode, None)
        st[f"wgrad{bias_mode}"] = L.lib.coma_last_kernel().decode()
        st[f"dx{bias_mode}"] = R.check_elementwise(dx, pr["dx"], R.elem_bound(pr["dx"], pr["Adx"], 27 * pr["cout"], u), name + " dx")
        st[f"dw{bias_mode}"] = R.check_elementwise(dwk, pr["dw"], R.elem_bound(pr["dw"], pr["Adw"], V * pr["B"] + P.WGRAD_NREP, R.U_F32), name + " dwk")
        if bias_mode:
            st["dbias"] = R.check_elementwise(dbias, pr["db"], R.elem_bound(pr["db"], pr["Adb"], V * pr["B"], R.U_F32), name + " dbias")
        else:
            assert dbias is None
    torch.cuda.synchronize()
    st["cur"], st["missed"] = arena.cur, arena.missed
    assert arena.cur % 256 == 0 and not bool(arena.buf[arena.cur:].view(torch.int64).any()), name + ": a taker wrote beyond its arena slice"
    ops.ZeroArena.end_step()
    assert arena.cur == 0 and not arena.armed and not bool(arena.buf.view(torch.int64).any()), name + ": the arena is not zero after the step"
    return st


@pytest.fixture
def arena(request, monkeypatch):
    """The device's ops.ZeroArena: the real one, or (param "tiny") an instance too small for any request, put in its place
    for the test and taken out again."""
    ops, L = _ops()
    monkeypatch.setattr(ops.ZeroArena, "enabled", True)
    key = torch.cuda.current_device()
    tiny = getattr(request, "param", None) == "tiny"
    old = ops.ZeroArena._arenas.get(key)
    if tiny:
        monkeypatch.setattr(ops.ZeroArena, "nbytes", 128)
        ops.ZeroArena._arenas[key] = ops.ZeroArena(torch.device("cuda", key))
    a = ops.ZeroArena.get(key)
    try:
        yield a
    finally:
        ops.ZeroArena.end_step()
        if tiny:
            if old is None:
                del ops.ZeroArena._arenas[key]
            else:
                ops.ZeroArena._arenas[key] = old
        _free()


@pytest.mark.parametrize("name", P.ARENA_CASES)
def test_arena_slices_of_exact_size(name, arena):
    """The call a training step makes: split-K / re-layout / replica scratch, statistics records and dwk are private zeroed
    slices of exactly the queried size, 256 bytes apart, handed over with COMA_ZEROED_WS / COMA_ZEROED_OUT.  The results
    hold their fp64 bounds, nothing beyond the arena's cursor is written, and the arena is all zero after the step."""
    st = _arena_step(name, arena)
    assert st["cur"] > 0 and st["missed"] == 0, st
    _put(f"arena-{name}", **st)


@pytest.mark.parametrize("name", P.ARENA_CASES)
@pytest.mark.parametrize("arena", ["tiny"], indirect=True)
def test_arena_too_small_falls_back_to_the_workspace(name, arena):
    """With an arena no request fits into, every taker falls back (shared workspace, library memsets, torch.zeros records):
    the same results, `missed` counts the requests, and the arena itself stays zero."""
    assert arena.buf.numel() == 128
    st = _arena_step(name, arena)
    assert st["cur"] == 0 and st["missed"] > 0, st
    _put(f"arena-tiny-{name}", **st)


def test_zz_report():
    """Prints the path and the worst ratio to its bound of every case and mode that ran."""
    for k, v in REPORT.items():
        print("ROW", k, {a: (float(f"{b:.4g}") if isinstance(b, float) else b) for a, b in v.items()})
