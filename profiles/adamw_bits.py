"""The bits coma_adamw, coma_adamw_ex and coma_adamw_ema leave behind: three consecutive updates of every configuration in
CONFIGS at every size of tests/_ema_plan.CASES (one partly filled block; the 16-byte path past one grid pass with a scalar tail;
the scalar path one element off alignment; fewer blocks than the cap), and after each update the SHA-256 of the raw bytes of
p, m, v, the average and norm_out.  The inputs are exact integer arithmetic (a multiplicative hash of the element index, its
top 20 bits scaled by a power of two), so they are the same bytes on any machine; the outputs belong to one compiler, whose
`hipcc --version` is recorded beside them.

  python profiles/adamw_bits.py > tests/golden/adamw_bits.json        (at the commit whose bits are the reference)

tests/test_adamw_bits_gpu.py runs the same cases and compares.  Only ops.adamw_ / adamw_ex_ / adamw_ema_ / grad_accum_ are
used, so the script runs unchanged at any commit that has them.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _ema_plan as EP  # noqa: E402

HP = (1e-2, 0.9, 0.999, 1e-8, 1e-2)       # lr, beta1, beta2, eps, weight decay
COUNT = 4                                 # micro-batches in the window
MAX_NORM = 2.0 ** -6                      # bites at every size (run_case asserts it)
EXTRA = 3.0                               # squared norm of "the gradients outside the buffer"
HOST_STEP = 7                             # what the host passes beside a device step count (must be ignored)
UPDATES = (1, 2, 3)

# name -> (entry point, device step count, counter, clip, extra_sumsq, (ema_decay, ema_warmup))
CONFIGS = {
    "adamw-host_step": ("adamw", False, False, False, False, None),
    "adamw-step_dev": ("adamw", True, False, False, False, None),
    "adamw_ex-count": ("ex", False, True, False, False, None),
    "adamw_ex-count-clip": ("ex", False, True, True, False, None),
    "adamw_ex-count-clip-extra": ("ex", False, True, True, True, None),
    "adamw_ema-fixed": ("ema", False, False, False, False, (0.999, False)),
    "adamw_ema-warmup-step_dev": ("ema", True, False, False, False, (0.999, True)),
    "adamw_ema-count-clip-extra": ("ema", True, True, True, True, (0.9, True)),
}


def exact(n, salt, scale, signed=True):
    """n floats in [-0.5, 0.5) * scale (signed) or [0, 1) * scale, scale a power of two: every step is exact."""
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    h = (((i + salt) * 2654435761) % (1 << 32)) >> 12          # 20 bits
    if signed:
        h = h - (1 << 19)
    return h.to(torch.float32) * (scale * 2.0 ** -20)


@functools.lru_cache(maxsize=None)
def compiler_version():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy()).hexdigest()


def run_case(case, config, adamw=None):
    """-> {buffer: [digest after update 1, 2, 3]}.  adamw: a stand-in for ops.adamw_ with its signature (the tests pass the
    binding itself: tests/test_data_parallel_cpu.py replaces ops.adamw_ for the rest of its process)."""
    from coma_unet_amd import ops
    _, n, off = case
    kind, dev_step, counter, clip, extra, ema = CONFIGS[config]

    def buf(src):
        flat = torch.zeros(off + n + 4, dtype=torch.float32, device="cuda")
        t = flat[off:off + n]
        t.copy_(src)
        assert (t.data_ptr() % 16 == 0) == (off == 0)
        return t

    p, m = buf(exact(n, 1, 1.0)), buf(exact(n, 2, 2.0 ** -6))
    v = buf(exact(n, 3, 2.0 ** -13, signed=False))             # v starts non-negative
    g = buf(exact(n, 4, 1.0))
    e = buf(exact(n, 5, 1.0)) if ema else None
    step_dev = torch.zeros(1, dtype=torch.int32, device="cuda") if dev_step else None
    count_dev = torch.full((1,), COUNT, dtype=torch.int32, device="cuda") if counter else None
    parts = torch.zeros(ops.ACC_PARTIALS, dtype=torch.float64, device="cuda") if clip else None
    extra_dev = torch.full((1,), EXTRA, dtype=torch.float64, device="cuda") if extra else None
    norm = torch.full((1,), -1.0, dtype=torch.float32, device="cuda") if clip else None
    out = {k: [] for k in ("p", "m", "v") + (("e",) if ema else ()) + (("norm_out",) if clip else ())}
    for t in UPDATES:
        g.copy_(exact(n, 100 + t, 2.0 if t == 2 else 1.0))
        step = HOST_STEP if dev_step else t
        if dev_step:
            step_dev.fill_(t)
        nb = ops.grad_accum_(None, g, None, parts) if clip else 0
        window = (count_dev, parts, nb, extra_dev, MAX_NORM if clip else 0.0, norm)
        if kind == "adamw":
            (adamw or ops.adamw_)(p, g, m, v, *HP, step, step_dev)
        elif kind == "ex":
            ops.adamw_ex_(p, g, m, v, *HP, step, step_dev, *window)
        else:
            ops.adamw_ema_(p, g, m, v, e, ema[0], ema[1], *HP, step, step_dev, *window)
        if clip:       # the clip bites: the norm of the mean gradient lies above MAX_NORM
            assert float(norm) > MAX_NORM
        for k, tns in (("p", p), ("m", m), ("v", v), ("e", e), ("norm_out", norm)):
            if k in out:
                out[k].append(sha(tns))
    return out


def run_all(adamw=None):
    return {f"{case[0]}/{config}": run_case(case, config, adamw) for case in EP.CASES for config in CONFIGS}


if __name__ == "__main__":
    json.dump({"hipcc_version": compiler_version(), "updates": list(UPDATES), "digests": run_all()}, sys.stdout, indent=1)
    print()
