"""The weight average of FusedAdamW(ema_decay, ema_warmup) without a GPU: the new symbols in the header and the binding table,
the option guards that need no kernel launch, and the fp64 recurrence of tests/_ema_plan.py against torch's own
AveragedModel + get_ema_multi_avg_fn (the yardstick is right before any kernel is judged by it)."""
import os
import re

import pytest
import torch

import _ema_plan as EP
import _nonconv_plan as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decl_args(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, f"{name} is not declared in include/coma_unet.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    from coma_unet_amd import _lib
    for name, nargs in (("coma_adamw_ema", 22), ("coma_swap_f32", 4)):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert len(_decl_args(hdr, name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    # coma_adamw_ex's arguments, then ema, ema_decay, ema_warmup, then the stream
    ex, ema = _lib.SIGNATURES["coma_adamw_ex"][1], _lib.SIGNATURES["coma_adamw_ema"][1]
    assert ema[:len(ex) - 1] == ex[:-1] and len(ema) == len(ex) + 3
    assert len(_decl_args(hdr, "coma_adamw_ex")) == 19 and len(_decl_args(hdr, "coma_adamw")) == 13      # unchanged


def test_abi_version_stays_3():
    from coma_unet_amd import _lib
    assert _lib.lib.coma_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    assert re.search(r"#define\s+COMA_ABI_VERSION\s+3\b", hdr)


def test_cases_cross_the_boundaries_they_are_listed_for():
    by = {c[0]: c for c in EP.CASES}
    one_pass = EP.EW_CAP * EP.THREADS
    assert EP.blocks(by["tiny"][1], True) == 1 and by["tiny"][1] < EP.THREADS
    _, n, off = by["vec4"]
    assert off == 0 and n % 4 == 3 and n // 4 > one_pass and EP.blocks(n, True) == EP.EW_CAP
    _, n, off = by["scalar"]
    assert off % 4 == 1 and n > one_pass and EP.blocks(n, False) == EP.EW_CAP
    _, n, off = by["few"]
    assert off == 0 and 1 < EP.blocks(n, True) < EP.EW_CAP and n % 4 == 2
    assert EP.blocks(0, True) == 0
    src = open(os.path.join(ROOT, "coma_unet_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"nb > %d\) nb = %d;" % (EP.EW_CAP, EP.EW_CAP), src)
    # the warm-up constants and the fused form the bound is counted from
    assert re.search(r"fminf\(ema_decay, \(1\.f \+ st\) / \(10\.f \+ st\)\)", src) and (EP.WARM_A, EP.WARM_B) == (1.0, 10.0)
    assert re.search(r"ei = fmaf\(w, pi - ei, ei\);", src)


def _opt(**kw):
    from coma_unet_amd.optim import FusedAdamW
    return FusedAdamW(torch.nn.Linear(3, 2).parameters(), **kw)


def test_option_guards():
    for bad in (0, 1, 0.0, 1.0, -0.5, 1.5, True, False, float("nan"), "0.9"):
        with pytest.raises(ValueError, match="ema_decay"):
            _opt(ema_decay=bad)
    with pytest.raises(ValueError, match="ema_warmup"):
        _opt(ema_decay=0.9, ema_warmup=2)
    o = _opt(ema_decay=0.99, ema_warmup=True)
    g = o.param_groups[0]
    assert g["ema_decay"] == 0.99 and g["ema_warmup"] is True and o.averaging and o.flat_ema is None
    d = _opt()
    assert d.param_groups[0]["ema_decay"] is None and d.param_groups[0]["ema_warmup"] is False and not d.averaging
    assert d.flat_ema is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        d.swap_ema()
    with pytest.raises(RuntimeError, match="ema_decay"):
        d.ema_state_dict(torch.nn.Linear(3, 2))
    o.param_groups[0]["ema_decay"] = 1.0         # a value set behind the constructor's back is caught at the step
    with pytest.raises(ValueError, match="ema_decay"):
        o.step()


def test_options_travel_with_the_state_dict_and_the_state_carries_no_average():
    o = _opt(ema_decay=0.75, ema_warmup=True)
    sd = o.state_dict()
    assert sd["param_groups"][0]["ema_decay"] == 0.75 and sd["param_groups"][0]["ema_warmup"] is True
    assert sd["state"] == {}
    fresh = _opt()
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["ema_decay"] == 0.75 and fresh.param_groups[0]["ema_warmup"] is True
    keep = _opt(ema_decay=0.9)
    keep.load_state_dict(_opt().state_dict())    # a file written without the option does not switch it off
    assert keep.param_groups[0]["ema_decay"] == 0.9
    old = {"state": {}, "param_groups": [{k: v for k, v in sd["param_groups"][0].items() if not k.startswith("ema_")}]}
    keep.load_state_dict(old)                    # nor does one from before the option existed
    assert keep.param_groups[0]["ema_decay"] == 0.9 and keep.param_groups[0]["ema_warmup"] is False


def test_swapped_in_average_blocks_step_and_state_dict():
    o = _opt(ema_decay=0.9)
    o.swap_ema()                                 # no layout yet: the average IS the parameters, nothing to launch
    with pytest.raises(RuntimeError, match="swapped in"):
        o.step()
    with pytest.raises(RuntimeError, match="swapped in"):
        o.state_dict()
    o.swap_ema()
    o.state_dict()
    with o.ema_weights():
        with pytest.raises(RuntimeError, match="swapped in"):
            o.state_dict()
    o.state_dict()


def test_sharded_exchange_raises_before_anything_runs():
    o = _opt(ema_decay=0.9)
    o.shard_exchange = object()                  # what StreamedGradExchange(sharded=True) sets; no collective is involved
    with pytest.raises(ValueError, match="sharded"):
        o.step()
    with pytest.raises(ValueError, match="sharded"):
        o.step_shards([(0, 4)])
    assert not o.built and o.flat_ema is None


def test_recurrence_is_torchs_ema_from_the_second_update_on():
    """AveragedModel copies the parameters at its first update; this average starts at the parameters' values when it is
    switched on.  Started from the same first value, both follow lerp(e, p, 1 - d): equal from the second update on."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(5)
    for d in (0.5, 0.9, 0.999):
        net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).double()
        avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(d))
        flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])
        st = None
        for t in range(1, 6):
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(0.1 * torch.randn_like(p))
            avg.update_parameters(net)
            if t == 1:
                st = EP.ema_init(flat(avg.module))             # the same first value
                continue
            dt = EP.ema_update(st, flat(net), d, False, t)
            assert dt == NP.f32(d)
            # the helper takes d as the float the kernel receives: exact for 0.5, 6e-9 (0.9) / 1.6e-8 (0.999) off otherwise
            ref = flat(avg.module)
            tol = 1e-12 if d == 0.5 else 4 * abs(NP.f32(d) - d) + 1e-12
            assert float((st["e"] - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max())), (d, t)
            assert bool((st["b"] > 0).all()) and bool(torch.isfinite(st["b"]).all())


def test_warmup_decay_rises_to_the_cap():
    ds = [EP.decay_at(0.9, True, t)[0] for t in range(1, 200)]
    assert ds[0] == 2 / 11 and all(a <= b for a, b in zip(ds, ds[1:])) and ds[-1] == NP.f32(0.9)
    assert EP.decay_at(0.9, True, 79)[0] == 80 / 89 and EP.decay_at(0.9, True, 80)[0] == NP.f32(0.9)      # (81 / 90 > float(0.9))
    assert EP.decay_at(0.9, False, 1)[0] == NP.f32(0.9)
