"""Gradient accumulation and global-norm clipping (FusedAdamW(grad_acc_batch, max_grad_norm)) without a GPU: the fp64 window
reference of tests/_grad_accum_plan.py against plain torch (the yardstick is right before any kernel is judged by it), the
new symbols in the header and the binding table, and the guards that need no kernel launch."""
import os
import re

import pytest
import torch

import _grad_accum_plan as GP
import _nonconv_plan as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def test_window_reference_matches_torch_accumulation_clip_and_adamw():
    """K = 3 backward passes of loss / 3, clip_grad_norm_, torch.optim.AdamW.step in fp64, two windows: the first clip
    bites, the second does not.  The helper is fed the three un-divided gradients of each window."""
    torch.manual_seed(3)
    K = 3
    lr, b1, b2, eps, wd = (NP.f32(x) for x in NP.ADAMW_HP)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).double()
    params = list(net.parameters())
    opt = torch.optim.AdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    st = NP.adamw_init(_flat([p.detach() for p in params]))
    bites = []
    for t, max_norm in ((1, NP.f32(0.05)), (2, NP.f32(1e4))):
        xs = [torch.randn(11, 7, dtype=torch.float64) for _ in range(K)]
        ys = [torch.randn(11, 3, dtype=torch.float64) for _ in range(K)]
        gs = [_flat(torch.autograd.grad(((net(x) - y) ** 2).mean(), params)) for x, y in zip(xs, ys)]
        opt.zero_grad()
        for x, y in zip(xs, ys):
            (((net(x) - y) ** 2).mean() / K).backward()
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)
        clipped = _flat([p.grad for p in params]).clone()
        opt.step()
        w = GP.window(st, gs, t, max_norm=max_norm)
        bites.append(w["c"] < 1.0)
        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
        assert abs(w["norm"] - float(norm)) <= 1e-12 * float(norm), (w["norm"], float(norm))
        assert rel(w["ghat"], clipped) <= 1e-12, rel(w["ghat"], clipped)
        assert rel(st["p"], _flat([p.detach() for p in params])) <= 1e-12
        assert rel(st["m"], _flat([opt.state[p]["exp_avg"] for p in params])) <= 1e-12
        assert rel(st["v"], _flat([opt.state[p]["exp_avg_sq"] for p in params])) <= 1e-12
        assert all(int(opt.state[p]["step"]) == t for p in params)
        for k in ("bp", "bm", "bv"):
            assert bool(torch.isfinite(st[k]).all()) and bool((st[k] > 0).all())
        # the accumulator's bound: nothing after the assignment, at least the last add's rounding after K - 1 adds
        A, b = w["acc"][-1]
        assert bool((w["acc"][0][1] == 0).all()) and bool((b >= GP.U * A.abs()).all())
    assert bites == [True, False]


def test_unclipped_scale_is_the_exact_mean():
    """No clipping: s = 1 / count, its bound is one fp32 rounding (+ the fp64 division); count = 1: s = 1."""
    sc = GP.scale(4.0, 0.0, 1, None)
    assert sc["s"] == 1.0 and sc["c"] == 1.0 and sc["norm"] == 2.0
    sc = GP.scale(9.0, 0.0, 3, None)
    assert sc["s"] == 1.0 / 3 and sc["norm"] == 1.0 and sc["e_s"] < 1.01 * GP.U + 2 * GP.U64
    sc = GP.scale(9.0, 0.0, 3, 0.5)
    assert abs(sc["c"] - 0.5 / (1.0 + 1e-6)) < 1e-15 and abs(sc["s"] - sc["c"] / 3) < 1e-16


def test_cases_cross_the_boundaries_they_are_listed_for():
    by = {c[0]: c for c in GP.CASES}
    assert GP.accum_blocks(by["tiny"][1], True) == 1
    _, n, off = by["vec4"]
    assert off == 0 and n % 4 == 3 and GP.accum_blocks(n, True) == GP.ACC_CAP and (n // 4) > GP.ACC_CAP * GP.THREADS
    _, n, off = by["scalar"]
    assert off % 4 != 0 and GP.accum_blocks(n, False) == GP.ACC_CAP and n > GP.ACC_CAP * GP.THREADS
    _, n, off = by["few"]
    assert 1 < GP.accum_blocks(n, True) < GP.ACC_CAP and n % 4 == 2
    _, n, off = by["unroll"]
    one_pass = GP.ACC_CAP * GP.THREADS
    assert off == 0 and GP.ACC_UNROLL * one_pass < n // 4 < (GP.ACC_UNROLL + 1) * one_pass and n % 4 == 3
    assert GP.accum_blocks(0, True) == 0
    src = open(os.path.join(ROOT, "coma_unet_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"ACC_BLOCKS\s*=\s*%d\b" % GP.ACC_CAP, src)
    assert GP.ACC_UNROLL == 2 and re.search(r"i \+ stride < n4; i \+= 2 \* stride", src)


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    from coma_unet_amd import _lib, ops
    for name in ("coma_grad_accum", "coma_adamw_ex"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["coma_adamw_ex"][1]) == 19 and len(_lib.SIGNATURES["coma_grad_accum"][1]) == 7
    assert ops.ACC_PARTIALS == GP.ACC_CAP


def _opt(**kw):
    from coma_unet_amd.optim import FusedAdamW
    return FusedAdamW(torch.nn.Linear(3, 2).parameters(), **kw)


def test_option_guards():
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="grad_acc_batch"):
            _opt(grad_acc_batch=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        _opt(max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        _opt(max_grad_norm=float("nan"))
    o = _opt(grad_acc_batch=4, max_grad_norm=2.5)
    g = o.param_groups[0]
    assert g["grad_acc_batch"] == 4 and g["max_grad_norm"] == 2.5 and o.pending == 0 and o.last_grad_norm is None and o.windowed
    o.flush()                                    # nothing pending: a no-op that needs no device
    d = _opt()
    assert d.param_groups[0]["grad_acc_batch"] == 1 and d.param_groups[0]["max_grad_norm"] is None and not d.windowed
    o.param_groups[0]["grad_acc_batch"] = 0      # a value set behind the constructor's back is caught at the step
    with pytest.raises(ValueError, match="grad_acc_batch"):
        o.step()


def test_hyper_parameters_travel_with_the_state_dict():
    o = _opt(grad_acc_batch=3, max_grad_norm=0.75)
    sd = o.state_dict()
    assert sd["param_groups"][0]["grad_acc_batch"] == 3 and sd["param_groups"][0]["max_grad_norm"] == 0.75
    fresh = _opt()
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["grad_acc_batch"] == 3 and fresh.param_groups[0]["max_grad_norm"] == 0.75
    old = {"state": {}, "param_groups": [{k: v for k, v in sd["param_groups"][0].items()
                                          if k not in ("grad_acc_batch", "max_grad_norm")}]}
    keep = _opt(grad_acc_batch=2, max_grad_norm=1.5)
    keep.load_state_dict(old)                    # an older checkpoint: the constructor's values stay
    assert keep.param_groups[0]["grad_acc_batch"] == 2 and keep.param_groups[0]["max_grad_norm"] == 1.5
    o._pending = 1                               # an open window
    with pytest.raises(RuntimeError, match=r"flush\(\)"):
        o.state_dict()


def test_exchange_combinations_raise():
    from coma_unet_amd.data_parallel import GradReducer
    from coma_unet_amd.train import train_step
    from coma_unet_amd import attn_unet_data_parallel as A
    for kw in (dict(grad_acc_batch=2), dict(max_grad_norm=1.0)):
        o = _opt(**kw)
        with pytest.raises(ValueError, match="exchange"):
            train_step(None, None, o, None, GradReducer(o))
        with pytest.raises(ValueError, match="exchange"):
            o.step_shards([(0, 4)])
        plain = _opt()
        with pytest.raises(ValueError, match="exchange"):
            A.train_dp(None, _Crit(), [], None, 1, 1e-3, roi_vecs_dict={"x": {}}, reducer=GradReducer(plain), **kw)
    with pytest.raises(ValueError, match="exchange"):      # a caller's own optimizer that accumulates, under a reducer
        o = _opt(grad_acc_batch=2)
        A.train_dp(None, _Crit(), [], None, 1, 1e-3, roi_vecs_dict={"x": {}}, reducer=GradReducer(o), optimizer=o)


class _Crit:
    class gen_loss:
        batch_reduction = "mean"
