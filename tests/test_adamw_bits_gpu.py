"""coma_adamw / coma_adamw_ex / coma_adamw_ema leave the bits they left before the three kernels became instantiations of one
body: profiles/adamw_bits.py's cases (three updates of eight configurations at the sizes of _ema_plan.CASES) hashed after every
update and compared with tests/golden/adamw_bits.json, which the same script recorded at the commit before that change.  The
other bitwise tests compare the variants with one another; this one compares them with their past.

The digests belong to one compiler: the fixture records `hipcc --version`, and under another one the test skips."""
import importlib.util
import json
import os

import pytest

import _ema_plan as EP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _runner():
    spec = importlib.util.spec_from_file_location("_adamw_bits", os.path.join(HERE, "..", "profiles", "adamw_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BITS = _runner()
with open(os.path.join(HERE, "golden", "adamw_bits.json")) as _f:
    GOLDEN = json.load(_f)


def _adamw(p, g, m, v, lr, b1, b2, eps, wd, step, step_dev=None):
    """coma_adamw through the binding table itself (tests/test_data_parallel_cpu.py replaces ops.adamw_ with a CPU restatement
    for the rest of its process)."""
    from coma_unet_amd import _lib as L
    L.check(L.lib.coma_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, b1, b2, eps, wd, step, L.ptr(step_dev),
                             L.stream()), "coma_adamw")


def test_fixture_covers_every_case():
    assert GOLDEN["updates"] == list(BITS.UPDATES)
    assert set(GOLDEN["digests"]) == {f"{c[0]}/{k}" for c in EP.CASES for k in BITS.CONFIGS}


@pytest.mark.parametrize("config", list(BITS.CONFIGS))
@pytest.mark.parametrize("case", EP.CASES, ids=lambda c: c[0])
def test_adamw_bits_are_the_recorded_ones(case, config):
    import torch
    have = BITS.compiler_version()
    if have != GOLDEN["hipcc_version"]:
        pytest.skip(f"the digests were recorded under another compiler: {GOLDEN['hipcc_version']!r}, here {have!r}")
    try:
        got = BITS.run_case(case, config, adamw=_adamw)
    finally:
        torch.cuda.empty_cache()
    want = GOLDEN["digests"][f"{case[0]}/{config}"]
    assert set(got) == set(want)
    for buf in want:
        for t, a, b in zip(BITS.UPDATES, got[buf], want[buf]):
            assert a == b, f"{case[0]} / {config}: {buf} after update {t} differs from the recorded bits"
