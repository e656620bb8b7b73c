"""FusedAdamW(lr_schedule, param_options) without a GPU: the new symbol in the header and the binding table, optim.LRSchedule
pinned to the installed torch's schedulers, its argument checks, the segment-table builder, the optimizer's plain-data state, and
the error bound of tests/_lr_schedule_plan.py (it must stay below 1e-5 of the base rate and hold the definition rounded to fp32)."""
import math
import os
import re

import pytest
import torch

import _lr_schedule_plan as LP
import _nonconv_plan as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WM, T = LP.WM, LP.T


def _decl_args(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, f"{name} is not declared in include/coma_unet.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_new_symbol_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    from coma_unet_amd import _lib, ops
    assert "coma_adamw_sched" in _lib.SIGNATURES and hasattr(_lib.lib, "coma_adamw_sched")
    assert len(_decl_args(hdr, "coma_adamw_sched")) == len(_lib.SIGNATURES["coma_adamw_sched"][1]) == 38
    assert ops.MAX_SEGS == LP.MAX_SEGS >= 2048          # (the kernel's own cap is met on the GPU: MAX_SEGS pass, one more is refused)
    assert ops.SCHED_KINDS == ("constant", "cosine", "linear", "step")


# ---- the schedule against torch's ---------------------------------------------------------------------------------------
def _torch_lrs(make, base, n):
    """The rates torch's scheduler(s) give updates 1 .. n: optimizer.step() then scheduler.step()."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = make(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def _pin(args, ref, base, hold_from=None):
    from coma_unet_amd.optim import LRSchedule
    sc = LRSchedule(**args)
    for s, want in enumerate(ref):
        if hold_from is not None and s > hold_from:
            want = ref[hold_from]
        got = base * sc.factor(s)
        assert abs(got - want) <= 1e-9 * abs(want), (args, s, got, want)


def test_factor_is_torchs_linear_cosine_step_and_their_sequence():
    """s = 0 .. Wm + T + 5, 1e-9 relative.  The definition holds the cosine at min_ratio from T on (u is clamped to [0, T]);
    torch's CosineAnnealingLR is periodic and climbs again past T_max, so beyond T the pin is to torch's value AT T.  The
    installed SequentialLR agrees at the milestone (it restarts the second scheduler at its epoch 0 there)."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR, StepLR
    base, n = 1e-3, WM + T + 6
    _pin(dict(warmup_steps=WM, warmup_start=0.25), _torch_lrs(lambda o: LinearLR(o, start_factor=0.25, total_iters=WM), base, n), base)
    _pin(dict(decay="cosine", total_steps=T, min_ratio=0.1),
         _torch_lrs(lambda o: CosineAnnealingLR(o, T_max=T, eta_min=0.1 * base), base, n), base, hold_from=T)
    _pin(dict(decay="step", step_size=3, gamma=0.5), _torch_lrs(lambda o: StepLR(o, step_size=3, gamma=0.5), base, n), base)
    seq = _torch_lrs(lambda o: SequentialLR(o, [LinearLR(o, start_factor=1.0 / 3.0, total_iters=WM),
                                                CosineAnnealingLR(o, T_max=T, eta_min=0.1 * base)], [WM]), base, n)
    _pin(LP.KINDS["cosine"], seq, base, hold_from=WM + T)
    # the linear decay has no torch twin with a floor: its two ends and its midpoint
    from coma_unet_amd.optim import LRSchedule
    lin = LRSchedule(**LP.KINDS["linear"])
    assert lin.factor(WM) == 1.0 and abs(lin.factor(WM + T) - 0.1) < 1e-15 and abs(lin.factor(WM + T // 2) - 0.55) < 1e-15
    assert lin.factor(WM + T + 5) == lin.factor(WM + T)
    assert LRSchedule().factor(0) == LRSchedule().factor(10 ** 6) == 1.0


@pytest.mark.parametrize("bad", [
    dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(warmup_steps=True), dict(warmup_start=0.0), dict(warmup_start=1.5),
    dict(warmup_start="x"), dict(decay="exp"), dict(decay="cosine"), dict(decay="cosine", total_steps=0),
    dict(decay="linear", total_steps=2.5), dict(total_steps=-3), dict(decay="cosine", total_steps=4, min_ratio=-0.1),
    dict(min_ratio=1.1), dict(decay="step"), dict(decay="step", step_size=0), dict(step_size=0.5),
    dict(decay="step", step_size=2, gamma=0.0), dict(gamma=1.5), dict(gamma=float("nan")), dict(warmup_steps=2 ** 31)],
    ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_schedule_rejects_bad_arguments(bad):
    from coma_unet_amd.optim import FusedAdamW, LRSchedule
    with pytest.raises(ValueError):
        LRSchedule(**bad)
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(2))], lr_schedule=bad)


def test_optimizer_rejects_bad_options():
    from coma_unet_amd.optim import FusedAdamW, LRSchedule
    ps = [torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(2))]
    for bad in ("no_decay", 3, [(1.0, None)], [(1.0, None), (-1.0, None)], [(1.0, None), (1.0, -0.1)],
                lambda n, p: dict(lr=1.0), lambda n, p: dict(lr_scale=float("inf")), lambda n, p: 1.0):
        with pytest.raises(ValueError):
            FusedAdamW(ps, param_options=bad)
    with pytest.raises(ValueError):
        FusedAdamW(ps, lr_schedule=3)
    with pytest.raises(ValueError):
        FusedAdamW(ps, lr_schedule=dict(warmup=3))
    with pytest.raises(ValueError):
        FusedAdamW(ps, param_options="no_decay_1d", param_names=["a"])
    d = LRSchedule(2, 0.5, "step", step_size=4, gamma=0.3).to_dict()
    assert LRSchedule.from_dict(d) == LRSchedule(2, 0.5, "step", step_size=4, gamma=0.3) and LRSchedule.from_dict(d).to_dict() == d
    assert all(isinstance(v, (int, float, str, type(None))) for v in d.values())


# ---- segment table --------------------------------------------------------------------------------------------------------
def test_segment_builder_merges_orders_and_caps():
    from coma_unet_amd.optim import build_segments, resolve_param_options
    shapes = [(4, 3, 3), (4,), (4,), (2, 4), (0,), (2,), (1,), (3, 1), (5,)]
    named = [(f"p{i}", torch.nn.Parameter(torch.zeros(s))) for i, s in enumerate(shapes)]
    opts = resolve_param_options("no_decay_1d", named)
    assert opts == [(1.0, None), (1.0, 0.0), (1.0, 0.0), (1.0, None), (1.0, 0.0), (1.0, 0.0), (1.0, 0.0), (1.0, None), (1.0, 0.0)]
    numels = [p.numel() for _, p in named]
    ends, scales, wds = build_segments(numels, opts, 0.01, total=64)
    # 36 | 4 + 4 merged | 8 | (empty) 2 + 1 merged | 3 | 5 and the padding up to 64
    assert ends == [36, 44, 52, 55, 58, 64] and scales == [1.0] * 6 and wds == [0.01, 0.0, 0.01, 0.0, 0.01, 0.0]
    assert all(a < b for a, b in zip(ends, ends[1:]))
    assert build_segments(numels, opts, 0.01)[0][-1] == sum(numels)
    # a decay given as the group's value merges with a neighbour that takes the group's
    assert build_segments([2, 2, 2], [(1.0, None), (1.0, 0.01), (0.5, 0.01)], 0.01) == ([4, 6], [1.0, 0.5], [0.01, 0.01])
    # a callable: names are passed, defaults fill in, None means defaults
    seen = []

    def by_name(name, p):
        seen.append(name)
        return dict(lr_scale=0.1) if name in ("p0", "p1") else (dict(weight_decay=0.5) if name == "p3" else None)
    got = resolve_param_options(by_name, named)
    assert seen == [n for n, _ in named] and got[0] == got[1] == (0.1, None) and got[3] == (1.0, 0.5) and got[2] == (1.0, None)
    assert resolve_param_options(None, named) is None
    # the cap: alternating options, one segment per tensor
    alt = [(1.0, 0.0 if i % 2 else None) for i in range(LP.MAX_SEGS + 1)]
    assert len(build_segments([3] * LP.MAX_SEGS, alt[:-1], 0.01)[0]) == LP.MAX_SEGS
    with pytest.raises(ValueError, match="at most"):
        build_segments([3] * (LP.MAX_SEGS + 1), alt, 0.01)


# ---- optimizer state ------------------------------------------------------------------------------------------------------
def _params():
    return [torch.nn.Parameter(torch.zeros(3, 3)), torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


def test_state_dict_carries_both_options_and_a_plain_file_switches_nothing_off(tmp_path):
    from coma_unet_amd.optim import FusedAdamW, LRSchedule
    sched = LRSchedule(2, 0.5, "cosine", total_steps=10, min_ratio=0.1)
    o = FusedAdamW(_params(), lr=2e-3, lr_schedule=sched, param_options="no_decay_1d")
    g = o.param_groups[0]
    assert len(o.param_groups) == 1 and o.scheduled
    assert g["lr_schedule"] == sched.to_dict() and g["param_options"] == [(1.0, None), (1.0, 0.0), (1.0, None)]
    assert o.current_lr() == 2e-3 * sched.factor(0) == 1e-3
    f = tmp_path / "o.pth"
    torch.save(o.state_dict(), f)
    sd = torch.load(f, weights_only=True)
    assert sd["param_groups"][0]["lr_schedule"] == sched.to_dict()
    # into an optimizer built without: it takes the file's; into one built with others: the file's win
    for fresh in (FusedAdamW(_params()), FusedAdamW(_params(), lr_schedule=dict(warmup_steps=9), param_options=lambda n, p: dict(lr_scale=0.5))):
        fresh.load_state_dict(sd)
        assert fresh.scheduled and fresh._schedule() == sched
        assert fresh.param_groups[0]["param_options"] == [(1.0, None), (1.0, 0.0), (1.0, None)]
        assert fresh.param_groups[0]["lr"] == 2e-3
    # a file without the options leaves a configured optimizer configured
    plain = FusedAdamW(_params(), lr=5e-4).state_dict()
    assert "lr_schedule" not in plain["param_groups"][0] and "param_options" not in plain["param_groups"][0]
    o.load_state_dict(plain)
    assert o.scheduled and o._schedule() == sched and o.param_groups[0]["param_options"][1] == (1.0, 0.0)
    assert o.param_groups[0]["lr"] == 5e-4
    only = FusedAdamW(_params(), param_options="no_decay_1d")
    assert only.scheduled and only._schedule() == LRSchedule() and only.param_groups[0]["lr_schedule"] is None
    only.load_state_dict(FusedAdamW(_params(), lr_schedule=sched).state_dict())       # (a file with one option keeps the other)
    assert only._schedule() == sched and only.param_groups[0]["param_options"][1] == (1.0, 0.0)


def test_options_off_means_no_state_and_the_keys_of_before():
    from coma_unet_amd.optim import FusedAdamW
    o = FusedAdamW(_params())
    assert not o.scheduled
    assert o._lr_dev is None and o._lr_host is None and o.last_lr is None and o._seg_tab is None and o._seg_key is None
    assert set(o.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay", "grad_acc_batch", "max_grad_norm",
                                      "ema_decay", "ema_warmup"}
    o.sync_lr()                                                   # nothing to do, nothing allocated
    assert o._lr_dev is None
    assert o.current_lr() == o.param_groups[0]["lr"]
    s = FusedAdamW(_params(), lr_schedule=dict(warmup_steps=2))   # configured, but nothing is allocated before the layout exists
    assert s.scheduled and s._lr_dev is None and s.last_lr is None and s._seg_tab is None


def test_graphed_step_hyper_leaves_the_base_rate_out_only_when_scheduled():
    from coma_unet_amd.optim import FusedAdamW
    from coma_unet_amd.train import GraphedTrainStep
    h = GraphedTrainStep.__new__(GraphedTrainStep)
    h.optimizer = FusedAdamW(_params(), lr=1e-3)
    assert h._hyper() == (1e-3, (0.9, 0.999), 1e-8, 1e-2, 1, None, None, False)           # what it returned before
    h.optimizer = FusedAdamW(_params(), lr=1e-3, lr_schedule=dict(warmup_steps=2), param_options="no_decay_1d")
    a = h._hyper()
    h.optimizer.param_groups[0]["lr"] = 2e-4
    assert h._hyper() == a and a[0] is None and a[4] == 1
    h.optimizer.param_groups[0]["lr_schedule"]["warmup_steps"] = 3
    b = h._hyper()
    assert b != a
    h.optimizer.param_groups[0]["param_options"][0] = (0.5, None)
    assert h._hyper() != b


# ---- the bound --------------------------------------------------------------------------------------------------------------
def _bound_cases():
    for name, args in LP.KINDS.items():
        for t in LP.STEPS:
            yield name, args, t
    yield ("long",) + LP.LONG
    for t in range(1, 11):
        yield "step-model", LP.STEP_SCHED, t
        yield "step-model", dict(LP.STEP_SCHED, total_steps=40), t
        yield "train_dp", LP.STEP_SCHED_LOOP, t


def test_bound_is_small_and_holds_the_rounded_definition():
    """For every case the GPU tests run: bound <= 1e-5 * base; the fp64 definition rounded to fp32 lies inside it, and so does
    the kernel's expression sequence evaluated in numpy float32 (numpy's cos / power standing in for cosf / powf).  One update
    off is far outside wherever the plan moves."""
    worst = 0.0
    for name, args, t in _bound_cases():
        for base in (LP.BASE, 0.2 * LP.BASE, 3e-4):
            ref, bound = LP.lr_bound(args, base, t)
            assert 0.0 < bound <= LP.REL_CAP * base, (name, t, bound / base)
            assert abs(NP.f32(ref) - ref) <= bound
            host = LP.lr_f32(args, base, t)
            assert abs(host - ref) <= bound, (name, t, host, ref, bound)
            worst = max(worst, bound / base)
            other = LP.lr_ref(args, base, t + 1)
            if abs(other - ref) > 1e-3 * base:
                assert abs(other - ref) > 100 * bound
    print(f"largest bound / base over the tested cases: {worst:.3e} ({worst / LP.U:.1f} u)")
    assert math.isclose(LP.lr_ref(LP.KINDS["cosine"], 1.0, WM + T + 1), 0.1)
