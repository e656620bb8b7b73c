"""FusedAdamW(lr_schedule, param_options) through the training step at 32^3, B = 2: eager, graph-replayed, with parameter
options, beside accumulation / clipping / the weight average, slice by slice, through a checkpoint and through train_dp.

No second model and no run-to-run determinism is needed: before an update the flat parameters and moments are copied, and after
it they must be bitwise what coma_adamw makes of the copy with the step's own flat gradient and lr = float(last_lr) -- the
whole buffer at once, so that every element takes the loop (16-byte body or scalar tail) it takes in the product's launch;
parameter options are checked by running the whole copy once per distinct (lr_scale, weight_decay) and comparing every
parameter's slice with the run that has its options (tests/test_lr_schedule_kernels_gpu.py says why slices are not cut out).
last_lr itself must lie within the bound tests/_lr_schedule_plan.py counts from the kernel source of the fp64 schedule."""
import gc
import logging
import os
import re

import numpy as np
import pytest
import torch

import _lr_schedule_plan as LP
import _step_state as SS

pytestmark = pytest.mark.gpu

MODE = "fp32-direct"
LR = 1e-3
S = (32, 32, 32)
SCHED = LP.STEP_SCHED            # Wm = 2, cosine, T = 4, down to 0.1 of the base rate
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _adamw(p, g, m, v, lr, wd, step, step_dev=None):
    from coma_unet_amd import _lib as L
    L.check(L.lib.coma_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, B1, B2, EPS, wd, step, L.ptr(step_dev),
                             L.stream()), "coma_adamw")


def _snap(o):
    return [t.clone() for t in (o.flat_p, o.flat_m, o.flat_v)]


def _check_lr(o, t, base=LR, sched=SCHED, tag=""):
    """last_lr of the update that brought the count to t."""
    ref, bound = LP.lr_bound(sched, base, t)
    got = float(o.last_lr)
    print(f"{tag} update {t}: last_lr {got:.9e}, fp64 {ref:.9e}, off by {abs(got - ref):.2e}, bound {bound:.2e}")
    assert abs(got - ref) <= bound, (tag, t, got, ref, bound)
    return got


def _check_update(o, snap, t, tag, options=None, model=None):
    """flat_p, flat_m, flat_v against coma_adamw on the snapshot.  options: {parameter name: (lr_scale, weight_decay)} for the
    parameters that do not take (1, the group's)."""
    lr_t = float(o.last_lr)
    step_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
    runs = {}

    def run(scale, wd):
        if (scale, wd) not in runs:
            p, m, v = (x.clone() for x in snap)
            _adamw(p, o.flat_g, m, v, float(np.float32(lr_t) * np.float32(scale)), wd, 7, step_dev)
            runs[(scale, wd)] = (p, m, v)
        return runs[(scale, wd)]
    got = (o.flat_p, o.flat_m, o.flat_v)
    if options is None:
        for nm, a, b in zip("pmv", got, run(1.0, WD)):
            assert torch.equal(a, b), f"{tag}: flat_{nm} of update {t} is not coma_adamw at last_lr"
    else:
        kinds = set()
        for name, off, k in SS.flat_layout(model, o):
            opt = options.get(name, (1.0, WD))
            kinds.add(opt)
            for nm, a, b in zip("pmv", got, run(*opt)):
                assert torch.equal(a[off:off + k], b[off:off + k]), f"{tag}: {nm} of {name} (options {opt}), update {t}"
        assert len(kinds) >= 2, "the options under test never differ"
        pad = sum(k for _, _, k in SS.flat_layout(model, o))
        assert pad == o.flat_p.numel()                      # (pad_to = 1: no padding to account for)
    assert not torch.equal(o.flat_p, snap[0])


class Bench:
    def __init__(self, static=True, **kw):
        import coma_unet_amd as cu
        from coma_unet_amd.train import make_optimizer
        if static:
            self.model = SS.fresh_model(MODE)
        else:
            torch.manual_seed(SS.SEED)
            self.model = cu.build_model(volume_shape=S, static_prompts=False, compute_dtype=torch.float32, conv_algo=1).cuda()
            self.model.set_save_attn(None)
            self.model.train(True)
        self.crit = cu.build_reference_criterion()
        self.opt = make_optimizer(self.model, LR, **kw)
        self.k = 0

    def next_batch(self):
        self.k += 1
        return SS.batch(MODE, self.k)

    def eager(self, b=None):
        from coma_unet_amd.train import train_step
        train_step(self.model, self.crit, self.opt, b if b is not None else self.next_batch())

    def first_step(self, t, tag, options=None):
        """The step that builds the flat layout, taken apart so that it can be snapshot-checked like every other one:
        train_step's zero_grad / forward / backward by hand, the layout (with whatever load_state_dict parked), the copy, the
        update.  -> the copy (flat_p, flat_m, flat_v before the update)."""
        from coma_unet_amd import ops
        from coma_unet_amd.train import forward_loss
        o = self.opt
        assert not o.built
        o.zero_grad()
        losses, _ = forward_loss(self.model, self.crit, self.next_batch())
        losses[0].backward()
        ops.SidePrep.join()
        o._build()
        snap = _snap(o)
        o.step()
        _check_update(o, snap, t, tag, options, self.model)
        return snap


def test_eager_steps_walk_the_schedule():
    """Four steps with Wm = 2, cosine, T = 4: current_lr() before a step is the plan of that step; last_lr after it is within
    the bound; the update is coma_adamw's at last_lr."""
    try:
        bn = Bench(lr_schedule=SCHED)
        o = bn.opt
        assert o.scheduled and o._lr_dev is None and o.last_lr is None
        seen = []
        for t in (1, 2, 3, 4):
            plan = o.current_lr()
            assert plan == LP.lr_ref(SCHED, LR, t)
            if t == 1:                                       # (s = 0: the warm-up's start factor on zero moments)
                snap = bn.first_step(1, "eager")
                assert not snap[1].any() and not snap[2].any()
                assert o._seg_tab is None and o._lr_dev is not None
            else:
                snap = _snap(o)
                bn.eager()
                _check_update(o, snap, t, "eager")
            assert o._flat_step == t and int(o._step_dev) == t
            seen.append(_check_lr(o, t, tag="eager"))
        assert len(set(seen)) == 4
    finally:
        _free()


def test_graph_replays_walk_the_schedule_without_a_new_capture():
    """Two eager steps, one capture, five replays: last_lr follows the plan replay by replay and the update is coma_adamw's;
    param_groups[0]["lr"] *= 0.2 (the plateau scheduler's action) scales last_lr with no new capture; a changed schedule
    re-captures once."""
    from coma_unet_amd.train import GraphedTrainStep
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            bn = Bench(lr_schedule=SCHED)
            o = bn.opt
            bn.eager()
            bn.eager()
            calls = []
            orig = GraphedTrainStep._capture

            def counted(self):
                calls.append(1)
                return orig(self)
            GraphedTrainStep._capture = counted
            try:
                step = GraphedTrainStep(bn.model, bn.crit, o, bn.next_batch(), prewarmed=True)
                bn.k -= 1
                assert len(calls) == 1 and o._flat_step == 2
                t = 2
                seen = []
                for _ in range(5):
                    t += 1
                    snap = _snap(o)
                    step(bn.next_batch())
                    assert o._flat_step == t and int(o._step_dev) == t
                    seen.append(_check_lr(o, t, tag="replay"))
                    _check_update(o, snap, t, "replay")
                assert len(calls) == 1 and len(set(seen)) >= 4
                o.param_groups[0]["lr"] *= 0.2
                base = o.param_groups[0]["lr"]
                t += 1
                snap = _snap(o)
                step(bn.next_batch())
                assert len(calls) == 1, "a changed base rate must not re-capture a scheduled step"
                _check_lr(o, t, base=base, tag="replay after lr * 0.2")
                _check_update(o, snap, t, "replay after lr * 0.2")
                sched2 = dict(SCHED, total_steps=40)
                o.param_groups[0]["lr_schedule"] = dict(o.param_groups[0]["lr_schedule"], total_steps=40)
                t += 1
                step(bn.next_batch())
                assert len(calls) == 2, "a changed schedule must re-capture"
                _check_lr(o, t, base=base, sched=sched2, tag="replay after the schedule changed")
                t += 1
                step(bn.next_batch())
                assert len(calls) == 2
                _check_lr(o, t, base=base, sched=sched2, tag="replay")
            finally:
                GraphedTrainStep._capture = orig
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        _free()


def test_no_decay_1d_and_a_callable_apply_per_parameter():
    try:
        bn = Bench(lr_schedule=SCHED, param_options="no_decay_1d")
        o, model = bn.opt, bn.model
        bn.eager()
        assert o._seg_tab is not None and 2 <= o._seg_tab[0].numel() <= 2048
        ends = o._seg_tab[0].tolist()
        assert ends == sorted(set(ends)) and ends[-1] == o.flat_p.numel()
        opts = {n: (1.0, 0.0) for n, p in model.named_parameters() if p.ndim <= 1}
        assert opts and len(opts) < len(list(model.parameters()))
        snap = _snap(o)
        bn.eager()
        _check_lr(o, 2, tag="no_decay_1d")
        _check_update(o, snap, 2, "no_decay_1d", opts, model)
        print(f"no_decay_1d: {len(ends)} segments for {len(SS.flat_layout(model, o))} tensors in the flat buffer")
        _free()

        # the encoder: the down block of every level of the nested U-Net (model.0, model.1.submodule.0, ...)
        picked = {n for n, _ in bn.model.named_parameters() if re.match(r"model\.(1\.submodule\.)*0\.", n)}
        assert 10 < len(picked) < len(list(bn.model.parameters())) // 2
        bn = Bench(lr_schedule=SCHED, param_options=lambda n, p: dict(lr_scale=0.1) if n in picked else None)
        o, model = bn.opt, bn.model
        bn.eager()
        snap = _snap(o)
        bn.eager()
        _check_update(o, snap, 2, "callable", {n: (0.1, WD) for n in picked}, model)
    finally:
        _free()


def test_loose_prompts_follow_the_global_schedule_with_their_own_count():
    """static_prompts=False, abeta [1, 0], [0, 1], [1, 1], [0, 0]: a prompt without a gradient is not stepped, so its
    bias-correction count falls behind the global one -- its update is coma_adamw's at the GLOBAL last_lr, its own count and,
    under "no_decay_1d", its own decay."""
    try:
        bn = Bench(static=False, lr_schedule=SCHED, param_options="no_decay_1d")
        o, model = bn.opt, bn.model
        prompts = [model.pos_dynamic_prompt, model.neg_dynamic_prompt]
        counts, lag = [0, 0], False
        for t in (1, 2, 3, 4):
            before = []
            for p in prompts:
                st = o.state.get(p) or {}
                before.append((p.detach().clone().view(-1), st["exp_avg"].clone().view(-1) if st else torch.zeros_like(p).view(-1),
                               st["exp_avg_sq"].clone().view(-1) if st else torch.zeros_like(p).view(-1)))
            bn.eager()
            _check_lr(o, t, tag="loose")
            for j, p in enumerate(prompts):
                assert id(p) not in o._flat_ids
                if p.grad is None:
                    assert torch.equal(p.detach().view(-1), before[j][0])
                    continue
                counts[j] += 1
                lag = lag or counts[j] < t
                pp, mm, vv = (x.clone() for x in before[j])
                wd = 0.0 if p.ndim <= 1 else WD
                _adamw(pp, p.grad.float().contiguous().view(-1), mm, vv, float(o.last_lr), wd, counts[j])
                assert torch.equal(p.detach().view(-1), pp), f"prompt {j}, step {t}"
                assert torch.equal(o.state[p]["exp_avg"].view(-1), mm) and torch.equal(o.state[p]["exp_avg_sq"].view(-1), vv)
                assert o.state[p]["step"] == counts[j]
        assert lag and o._flat_step == 4
    finally:
        _free()


def test_composition_with_window_clip_average_and_slices():
    """grad_acc_batch = 2, a clip, ema_decay = 0.9 beside the schedule: last_lr moves on applied updates only.  Then, without
    the window, one step taken over three slices (cut at 16-byte chunk boundaries, as the data-parallel buckets are; advance
    on the first, the loose parameters on a call of their own) is bitwise one whole launch on copies."""
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss
    try:
        bn = Bench(lr_schedule=SCHED, param_options="no_decay_1d", grad_acc_batch=2, max_grad_norm=1e-3, ema_decay=0.9)
        o = bn.opt
        bn.eager()
        assert o.pending == 1 and o._flat_step == 0 and float(o.last_lr) == 0.0
        bn.eager()
        assert o.pending == 0 and o._flat_step == 1
        first = _check_lr(o, 1, tag="window")
        keep_e = o.flat_ema.clone()
        bn.eager()
        assert o.pending == 1 and float(o.last_lr) == first and torch.equal(o.flat_ema, keep_e)
        bn.eager()
        assert _check_lr(o, 2, tag="window") != first and float(o.last_grad_norm) > 1e-3
        assert not torch.equal(o.flat_ema, keep_e)
        _free()

        bn = Bench(lr_schedule=SCHED, param_options="no_decay_1d", ema_decay=0.9)
        o = bn.opt
        bn.eager()
        o.zero_grad()
        losses, _ = forward_loss(bn.model, bn.crit, bn.next_batch())
        losses[0].backward()
        ops.SidePrep.join()
        n = o.flat_p.numel()
        cuts = [0, 4 * 257, (n // 3) // 4 * 4, n]
        p, m, v, e = (t.clone() for t in (o.flat_p, o.flat_m, o.flat_v, o.flat_ema))
        for i, (a, c) in enumerate(zip(cuts, cuts[1:])):
            o.step_shards([(a, c - a)], advance=i == 0, loose=False)
        o.step_shards([], advance=False, loose=True)
        assert o._flat_step == 2
        _check_lr(o, 2, tag="slices")
        o._update(p, o.flat_g, m, v, e, o._flat_step, o._step_dev, flat_off=0)
        for nm, a, b in zip("pmve", (o.flat_p, o.flat_m, o.flat_v, o.flat_ema), (p, m, v, e)):
            assert torch.equal(a, b), f"flat_{nm}: three slices differ from one launch"
    finally:
        _free()


def test_checkpoint_resumes_the_schedule(tmp_path):
    """The state after two steps into a fresh optimizer that was built with ANOTHER schedule: the file's schedule and options
    win; the layout it builds holds bitwise the uninterrupted run's parameters and moments after update 2; and the third step is
    update 3 of the plan at the uninterrupted run's rate, p, m, v bitwise coma_adamw's on that restored state (the gradients of
    two runs differ in their last bits -- the backward's atomics -- so the two runs' third steps are not compared with each other
    beyond that)."""
    from coma_unet_amd import checkpoint
    try:
        bn = Bench(lr_schedule=SCHED, param_options="no_decay_1d")
        bn.eager()
        bn.eager()
        files = checkpoint.save_checkpoint(str(tmp_path), 1, bn.model, bn.opt, torch.tensor(1.0), None)
        raw = torch.load(files[0], map_location="cpu", weights_only=True)
        grp = raw["optimizer_state_dict"]["param_groups"][0]
        assert grp["lr_schedule"] == bn.opt._schedule().to_dict() and len(grp["param_options"]) == len(grp["params"])
        keep = _snap(bn.opt)
        bn.eager()
        want = _check_lr(bn.opt, 3, tag="uninterrupted")

        b2 = Bench(lr_schedule=dict(warmup_steps=50), param_options=None)
        assert checkpoint.load_checkpoint(files[0], b2.model, b2.opt, None) == 2
        o = b2.opt
        assert o._schedule().to_dict() == grp["lr_schedule"] and o.param_groups[0]["param_options"][:3] == [tuple(x) for x in grp["param_options"][:3]]
        assert o.current_lr() == LP.lr_ref(SCHED, LR, 3)
        b2.k = 2
        opts = {n: (1.0, 0.0) for n, p in b2.model.named_parameters() if p.ndim <= 1}
        snap = b2.first_step(3, "resumed", opts)             # builds the layout from the parked state and takes update 3
        for nm, a, b in zip("pmv", snap, keep):
            assert torch.equal(a, b), f"flat_{nm} restored from the file is not the uninterrupted run's after update 2"
        assert snap[1].any() and snap[2].any()
        assert o._flat_step == 3 and int(o._step_dev) == 3 and float(o.last_lr) == want
        assert o._seg_tab is not None
        snap = _snap(o)
        b2.eager()
        _check_lr(o, 4, tag="resumed")
        _check_update(o, snap, 4, "resumed", opts, b2.model)
    finally:
        _free()


def _loader(n_batches, B, abetas, seed0=0, triplet=True):
    """The loaders of tests/test_train_loop_gpu.py: samples in the reference's layout."""
    from coma_unet_amd.synthetic import make_batch
    out, lookup = [], {}
    for i in range(n_batches):
        b = make_batch(B, S, seed=seed0 + i)
        ab = torch.tensor(abetas[i], dtype=torch.float32)
        cov = b["covars"].clone()
        cov[:, 0, 0] = ab
        paths = [f"/data/xnat/adni/{seed0 + i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP/analysis/rnu.nii" for j in range(B)]
        for j, p in enumerate(paths):
            lookup[f"{seed0 + i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP"] = b["roi_pred_dicts"][j]
        item = (b["mri"], b["tau"], b["roi"], (ab, cov), paths)
        out.append((item, item, item) if triplet else item)
    return out, lookup


def test_train_dp_runs_the_schedule_under_one_capture(tmp_path, monkeypatch, caplog):
    """Two epochs of four batches, graph-replayed: one capture; the epoch's log line carries current_lr() of the plan; the
    checkpoint on disk reloads into a fresh optimizer with schedule, options and count."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import checkpoint, train_loop
    from coma_unet_amd.train import GraphedTrainStep, make_optimizer
    try:
        train, lk = _loader(4, 2, [[1, 0], [0, 1], [1, 1], [0, 0]], seed0=40)
        torch.manual_seed(11)
        m = cu.build_model(volume_shape=S, static_prompts=True).cuda()
        m.set_save_attn(None)
        m.train(True)
        seen, calls = {}, []
        orig_opt, orig_cap = train_loop.make_optimizer, GraphedTrainStep._capture

        def spy_opt(*a, **kw):
            seen["opt"] = orig_opt(*a, **kw)
            return seen["opt"]

        def counted(self):
            calls.append(1)
            return orig_cap(self)
        monkeypatch.setattr(train_loop, "make_optimizer", spy_opt)
        monkeypatch.setattr(GraphedTrainStep, "_capture", counted)
        sched = LP.STEP_SCHED_LOOP
        with caplog.at_level(logging.INFO):
            losses = A.train_dp(m, cu.build_reference_criterion(), train, None, 2, LR, save_path=str(tmp_path), cuda_id=0,
                                roi_vecs_dict=lk, lr_schedule=sched, param_options="no_decay_1d")
        o = seen["opt"]
        assert len(losses) == 2 and o.scheduled and o._flat_step == 8 and int(o._step_dev) == 8
        assert len(calls) == 1, f"{len(calls)} captures"
        assert o._seg_tab is not None
        _check_lr(o, 8, sched=sched, tag="train_dp")
        logged = [float(x) for x in re.findall(r"lr (\d\.\d+e[-+]\d+)", caplog.text)]
        assert len(logged) == 2
        for got, k in zip(logged, (4, 8)):
            assert abs(got - LR * LP.schedule(sched).factor(k)) <= 1e-9 * LR, (got, k)
        m2 = cu.build_model(volume_shape=S, static_prompts=True).cuda()
        o2 = make_optimizer(m2, 5e-4)
        path = os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth")
        assert checkpoint.load_checkpoint(path, m2, o2, None) == 2
        assert o2.scheduled and o2._schedule() == LP.schedule(sched) and o2.param_groups[0]["lr"] == LR
        assert o2.param_groups[0]["param_options"] == o.param_groups[0]["param_options"]
        assert {int(st["step"]) for st in o2.state.values()} == {8}          # parked until the layout exists: the count resumes
    finally:
        _free()
