"""FusedAdamW(grad_acc_batch, max_grad_norm) through the training step: eager, graph-replayed (GraphedTrainStep's two
graphs), mixed, flush(), clip-only, parameters outside the flat buffer, and train_dp.

The reference needs no second model: the product leaves every micro-batch's own gradient in `flat_g`, which is cloned after
each micro-batch and fed to the fp64 window of tests/_grad_accum_plan.py; `flat_acc`, `flat_p`, `flat_m`, `flat_v` and
`last_grad_norm` must then meet the helper's bounds (derived from the kernel source, not measured).

Clipping: a window with max_grad_norm = 1e30 reports the norm, the next one runs with half of that.  At lr = 1e-3 the norm of
this model's gradient falls from one window to the next by more than a factor of two (measured: 301 -> 135 over the first two
windows), so "half of the last norm" does not reliably bite: it is kept as one case (checked against the helper whichever way
the coefficient falls), and a further window with 1 / 64 of the first norm is the one that is asserted to bite."""
import gc
import os

import pytest
import torch

import _grad_accum_plan as GP
import _nonconv_plan as NP
import _step_state as SS
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

MODE = "fp32-direct"
LR = 1e-3
HP = (LR,) + NP.ADAMW_HP[1:]
assert NP.ADAMW_HP[1:] == (0.9, 0.999, 1e-8, 1e-2)        # FusedAdamW's defaults


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _set(opt, K, mx):
    opt.param_groups[0]["grad_acc_batch"] = K
    opt.param_groups[0]["max_grad_norm"] = mx


class Bench:
    """A model that took the two plain steps the flat layout needs, and the fp64 mirror of its optimizer state."""

    def __init__(self):
        import coma_unet_amd as cu
        from coma_unet_amd.train import make_optimizer, train_step
        self.model = SS.fresh_model(MODE)
        self.crit = cu.build_reference_criterion()
        self.opt = make_optimizer(self.model, LR)
        for k in (1, 2):
            train_step(self.model, self.crit, self.opt, SS.batch(MODE, k))
        assert self.opt.built and self.opt._flat_step == 2 and self.opt.flat_acc is None and not self.opt.windowed
        self.mirror()

    def mirror(self):
        o = self.opt
        z = lambda: torch.zeros(o.flat_p.numel(), dtype=torch.float64, device="cuda")
        self.p0 = o.flat_p.double().clone()
        self.st = dict(p=self.p0.clone(), m=o.flat_m.double().clone(), v=o.flat_v.double().clone(), bp=z(), bm=z(), bv=z())
        self.t = o._flat_step

    def eager(self, b):
        from coma_unet_amd.train import train_step
        train_step(self.model, self.crit, self.opt, b)

    def window(self, steps, max_norm, K=None, flush=False, tag=""):
        """`steps`: [(callable, batch)] -- the window's micro-batches.  Checks the accumulator after every one, that the
        parameters stay put until the last, and the update against the helper.  -> the helper's window."""
        o = self.opt
        K = K or len(steps)
        before = o.flat_p.clone()
        step0 = o._flat_step
        gs = []
        for i, (fn, b) in enumerate(steps):
            fn(b)
            gs.append(o.flat_g.clone())
            if K > 1:
                A, bd = GP.accumulate(gs)[-1]
                if i == 0:
                    assert torch.equal(o.flat_acc, gs[0])
                else:
                    R.check_elementwise(o.flat_acc, A, bd, f"{tag} flat_acc after micro-batch {i + 1}")
            if i < K - 1:
                assert torch.equal(o.flat_p, before), f"{tag}: parameters moved at micro-batch {i + 1} of {K}"
                assert o.pending == i + 1 and o._flat_step == step0 and int(o._step_dev) == step0 and int(o._acc_dev) == i + 1
        if flush:
            with pytest.raises(RuntimeError, match=r"flush\(\)"):
                o.state_dict()
            o.flush()
        self.t += 1
        w = GP.window(self.st, gs, self.t, max_norm=max_norm, hp=HP)
        assert o.pending == 0 and o._flat_step == self.t and int(o._step_dev) == self.t
        if K > 1:
            assert int(o._acc_dev) == 0
        st = self.st
        r = dict(m=R.check_elementwise(o.flat_m, st["m"], st["bm"], f"{tag} m"),
                 v=R.check_elementwise(o.flat_v, st["v"], st["bv"], f"{tag} v"),
                 upd=R.check_elementwise(o.flat_p.double() - self.p0, st["p"] - self.p0, st["bp"], f"{tag} p - p0"))
        assert not torch.equal(o.flat_p, before)
        if max_norm is None:
            assert o.last_grad_norm is None
        else:
            got = float(o.last_grad_norm)
            assert abs(got - w["norm"]) <= w["b_norm"], (tag, got, w["norm"], w["b_norm"])
        print(f"{tag}: update {self.t}, count {len(gs)}, norm {w['norm']:.6g}, c {w['c']:.4g}; worst ratios {r}")
        return w


def _flat_index(bench):
    return next(i for i, p in enumerate(bench.opt.param_groups[0]["params"]) if id(p) in bench.opt._flat_ids)


BITE = 64.0        # max_grad_norm = first norm / BITE: bites unless the gradient norm collapsed 64-fold within two updates


def test_eager_windows_accumulate_then_clip():
    """K = 3: max_grad_norm 1e30 (the clip cannot bite), then half the norm the first window reported, then 1 / 64 of it."""
    try:
        bn = Bench()
        o = bn.opt
        i = _flat_index(bn)
        s0 = float(o.state_dict()["state"][i]["step"])
        _set(o, 3, 1e30)
        w1 = bn.window([(bn.eager, SS.batch(MODE, k)) for k in (3, 4, 5)], 1e30, tag="eager window 1")
        assert w1["c"] == 1.0
        half = float(o.last_grad_norm) / 2
        _set(o, 3, half)
        bn.window([(bn.eager, SS.batch(MODE, k)) for k in (6, 7, 8)], half, tag="eager window 2")
        assert float(o.state_dict()["state"][i]["step"]) == s0 + 2 and o.pending == 0
        _set(o, 3, 2 * half / BITE)
        w3 = bn.window([(bn.eager, SS.batch(MODE, k)) for k in (9, 10, 11)], 2 * half / BITE, tag="eager window 3")
        assert w3["c"] < 0.75, "the third window's clip must bite"
        assert float(o.state_dict()["state"][i]["step"]) == s0 + 3 and o.pending == 0
    finally:
        _free()


def test_graphed_windows_recapture_and_mix_with_eager():
    """The same two windows through GraphedTrainStep: the micro-batch graph twice and the applying graph once per window;
    the change of max_grad_norm recaptures both graphs; the second window's middle micro-batch runs eagerly."""
    from coma_unet_amd.train import GraphedTrainStep
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            bn = Bench()
            o = bn.opt
            _set(o, 3, 1e30)
            step = GraphedTrainStep(bn.model, bn.crit, o, SS.batch(MODE, 3), prewarmed=True)
            assert step.micro_graph is not None and o.pending == 0 and o._flat_step == 2 and int(o._acc_dev) == 0
            graphs = (step.micro_graph, step.graph)
            replay = lambda b: step(b)
            bn.window([(replay, SS.batch(MODE, k)) for k in (3, 4, 5)], 1e30, tag="graph window 1")
            assert (step.micro_graph, step.graph) == graphs
            half = float(o.last_grad_norm) / 2
            _set(o, 3, half)
            bn.window([(replay, SS.batch(MODE, 6)), (bn.eager, SS.batch(MODE, 7)), (replay, SS.batch(MODE, 8))], half,
                      tag="graph window 2 (mixed)")
            assert step.micro_graph is not graphs[0] and step.graph is not graphs[1], "no recapture after max_grad_norm changed"
            bite = 2 * half / BITE
            _set(o, 3, bite)
            w3 = bn.window([(replay, SS.batch(MODE, 9)), (bn.eager, SS.batch(MODE, 10)), (replay, SS.batch(MODE, 11))], bite,
                           tag="graph window 3 (mixed)")
            assert w3["c"] < 0.75, "the third window's clip must bite"
            # a replayed micro-batch, then an eager flush of the window it opened
            w4 = bn.window([(replay, SS.batch(MODE, 12))], bite, K=3, flush=True, tag="graph micro-batch + flush")
            assert w4["s"] == w4["c"] < 0.75
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        _free()


def test_flush_applies_the_mean_of_an_open_window():
    """Two micro-batches of a K = 3 window, then flush(): the mean of two gradients; state_dict() before it raises."""
    try:
        bn = Bench()
        _set(bn.opt, 3, None)
        w = bn.window([(bn.eager, SS.batch(MODE, k)) for k in (3, 4)], None, K=3, flush=True, tag="flush")
        assert w["s"] == 0.5
        bn.opt.flush()                                   # nothing pending: no-op
        assert bn.opt._flat_step == bn.t and bn.opt.pending == 0
    finally:
        _free()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_clip_only(graph):
    """K = 1 with clipping: one graph as before.  max_grad_norm 1e30: flat_p is bitwise what coma_adamw makes of the same
    flat_g; then half the reported norm: within the helper's bounds."""
    from coma_unet_amd import ops
    from coma_unet_amd.train import GraphedTrainStep
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            bn = Bench()
            o = bn.opt
            _set(o, 1, 1e30)
            if graph:
                step = GraphedTrainStep(bn.model, bn.crit, o, SS.batch(MODE, 3), prewarmed=True)
                assert step.micro_graph is None and o._flat_step == 2 and o.pending == 0
                fn = lambda b: step(b)
            else:
                fn = bn.eager
            p, m, v = o.flat_p.clone(), o.flat_m.clone(), o.flat_v.clone()
            w = bn.window([(fn, SS.batch(MODE, 3))], 1e30, tag=f"clip-only {'graph' if graph else 'eager'} 1e30")
            assert w["c"] == 1.0 and o.flat_acc is None
            ops.adamw_(p, o.flat_g.clone(), m, v, LR, 0.9, 0.999, 1e-8, 1e-2, o._flat_step, o._step_dev)    # (device step count, as the product)
            assert torch.equal(o.flat_p, p) and torch.equal(o.flat_m, m) and torch.equal(o.flat_v, v)
            half = float(o.last_grad_norm) / 2
            _set(o, 1, half)
            g0 = step.graph if graph else None
            bn.window([(fn, SS.batch(MODE, 4))], half, tag=f"clip-only {'graph' if graph else 'eager'} half")
            assert not graph or step.graph is not g0
            _set(o, 1, 2 * half / BITE)
            w = bn.window([(fn, SS.batch(MODE, 5))], 2 * half / BITE, tag=f"clip-only {'graph' if graph else 'eager'} 1/64")
            assert w["c"] < 0.75, "the clip must bite"
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        _free()


def test_parameters_outside_the_flat_buffer():
    """static_prompts=False, K = 2, abeta [1, 1] then [0, 0]: each dynamic prompt receives a gradient in one micro-batch
    only, is updated with half of it, and both count in the clipped norm."""
    import coma_unet_amd as cu
    from coma_unet_amd.train import make_optimizer, train_step
    try:
        torch.manual_seed(SS.SEED)
        model = cu.build_model(volume_shape=(32, 32, 32), static_prompts=False, compute_dtype=torch.float32, conv_algo=1).cuda()
        model.set_save_attn(None)
        model.train(True)
        crit = cu.build_reference_criterion()
        opt = make_optimizer(model, LR)
        for k in (1, 2):
            train_step(model, crit, opt, SS.batch(MODE, k))
        prompts = [model.pos_dynamic_prompt, model.neg_dynamic_prompt]
        assert all(id(p) not in opt._flat_ids for p in prompts)
        _set(opt, 2, 1e30)
        # one window to learn the norm, then one with a clip that bites (1 / 64 of that norm: see the module docstring)
        mirrors = None
        for max_norm in (1e30, None):
            if max_norm is None:
                max_norm = float(opt.last_grad_norm) / BITE
                _set(opt, 2, max_norm)
            flat_st = dict(p=opt.flat_p.double().clone(), m=opt.flat_m.double().clone(), v=opt.flat_v.double().clone())
            z = lambda t: torch.zeros(t.numel(), dtype=torch.float64, device="cuda")
            mirrors = []
            for p in prompts:
                s = opt.state.get(p) or {}
                mirrors.append(dict(p=p.detach().double().reshape(-1).clone(),
                                    m=s["exp_avg"].double().reshape(-1).clone() if s else z(p),
                                    v=s["exp_avg_sq"].double().reshape(-1).clone() if s else z(p),
                                    bp=z(p), bm=z(p), bv=z(p), t=int(s["step"]) if s else 0))
            gs, loose = [], [[], []]
            for k in (3, 4):                                   # ABETA entries [1, 1] and [0, 0]
                train_step(model, crit, opt, SS.batch(MODE, k))
                gs.append(opt.flat_g.clone())
                for j, p in enumerate(prompts):
                    loose[j].append(None if p.grad is None else p.grad.detach().float().reshape(-1).clone())
            assert [[g is not None for g in l] for l in loose] == [[True, False], [False, True]]
            # the window's total sum of squares: flat accumulator + both prompts' (each a single, exactly assigned gradient)
            A, b = GP.accumulate(gs)[-1]
            tot, rel = GP.sumsq(A, b)
            ex = [next(g for g in l if g is not None).double() for l in loose]
            ex_tot = sum(float((e * e).sum()) for e in ex)
            total = tot + ex_tot
            sc = GP.scale(total, (tot * rel + ex_tot * (sum(e.numel() for e in ex) + 2) * GP.U64) / total, 2, max_norm)
            got = float(opt.last_grad_norm)
            assert abs(got - sc["norm"]) <= sc["b_norm"], (got, sc["norm"], sc["b_norm"])
            print(f"loose window: norm {got:.6g}; the prompts hold {ex_tot / total:.3g} of the squared norm, bound {sc['b_norm']:.3g}")
            assert ex_tot > 0
            # in fp32 the norm cannot show so small a share: the fp64 sum the optimizer handed to the kernel can
            assert abs(float(opt._extra_dev) - ex_tot) <= (sum(e.numel() for e in ex) + 2) * GP.U64 * ex_tot
            if ex_tot / total > 1e-5:       # (visible beyond the fp32 rounding of the norm: leaving them out must show)
                assert abs(got - tot ** 0.5 / 2) > 4 * sc["b_norm"], "the prompts' gradients must count in the norm"
            for j, (p, mr) in enumerate(zip(prompts, mirrors)):
                p_before, m_before = mr["p"].clone(), mr["m"].clone()
                GP.apply(mr, ex[j], torch.zeros_like(ex[j]), sc, mr["t"] + 1, hp=HP)
                s = opt.state[p]
                assert int(s["step"]) == mr["t"] + 1
                R.check_elementwise(s["exp_avg"].reshape(-1), mr["m"], mr["bm"], f"prompt {j} m")
                R.check_elementwise(s["exp_avg_sq"].reshape(-1), mr["v"], mr["bv"], f"prompt {j} v")
                R.check_elementwise(p.detach().double().reshape(-1) - p_before, mr["p"] - p_before, mr["bp"], f"prompt {j} update")
                # half the gradient (times the clip coefficient) is what reached the first moment
                b1 = NP.f32(0.9)
                moved = mr["m"] - b1 * m_before                     # (a difference of fp64 numbers: exact to 2^-52 of |m|)
                assert float((moved - (1 - b1) * ex[j] * sc["c"] / 2).abs().max()) <= 1e-12 * float(mr["m"].abs().max())
            assert opt.pending == 0 and not opt._loose_live
            assert all(float(a.abs().max()) == 0.0 for a in opt._loose_acc.values())
        assert sc["c"] < 0.75
    finally:
        _free()


S = (32, 32, 32)


def _loader(n_batches, B, abetas, seed0=0):
    """The training loader of tests/test_train_loop_gpu.py: (anchor, pos, neg) triplets in the reference's sample layout."""
    from coma_unet_amd.synthetic import make_batch
    out, lookup = [], {}
    for i in range(n_batches):
        b = make_batch(B, S, seed=seed0 + i)
        ab = torch.tensor(abetas[i], dtype=torch.float32)
        cov = b["covars"].clone()
        cov[:, 0, 0] = ab
        paths = [f"/data/xnat/adni/{i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP/analysis/rnu.nii" for j in range(B)]
        for j, p in enumerate(paths):
            lookup[f"{i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP"] = b["roi_pred_dicts"][j]
        item = (b["mri"], b["tau"], b["roi"], (ab, cov), paths)
        out.append((item, item, item))
    return out, lookup


def test_train_dp_accumulates_flushes_and_checkpoints(tmp_path, monkeypatch):
    """grad_acc_batch=2 over 3 batches per epoch: one full window and one flushed at the end of the epoch."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd.train import make_optimizer
    try:
        train, lookup = _loader(3, 2, [[1, 0], [0, 1], [1, 1]], seed0=70)
        torch.manual_seed(11)
        m = cu.build_model(volume_shape=S).cuda()
        m.set_save_attn(None)
        m.train(True)
        seen = {}
        orig = make_optimizer

        def spy(*a, **kw):
            seen["opt"] = orig(*a, **kw)
            return seen["opt"]

        from coma_unet_amd import train_loop
        monkeypatch.setattr(train_loop, "make_optimizer", spy)
        losses = A.train_dp(m, cu.build_reference_criterion(), train, None, 1, 1e-3, save_path=str(tmp_path), cuda_id=0,
                            roi_vecs_dict=lookup, graph=False, grad_acc_batch=2, max_grad_norm=5.0)
        opt = seen["opt"]
        assert len(losses) == 1 and opt.pending == 0 and opt._flat_step == 2 and int(opt._step_dev) == 2 and int(opt._acc_dev) == 0
        assert float(opt.last_grad_norm) > 0
        raw = torch.load(os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth"), map_location="cpu", weights_only=True)
        pg = raw["optimizer_state_dict"]["param_groups"][0]
        assert pg["grad_acc_batch"] == 2 and pg["max_grad_norm"] == 5.0
        assert float(raw["optimizer_state_dict"]["state"][0]["step"]) == 2.0
        fresh = make_optimizer(m, 1e-3)
        fresh.load_state_dict(raw["optimizer_state_dict"])
        assert fresh.param_groups[0]["grad_acc_batch"] == 2 and fresh.param_groups[0]["max_grad_norm"] == 5.0
    finally:
        _free()
