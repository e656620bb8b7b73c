"""FusedAdamW(ema_decay, ema_warmup) through the training step at 32^3, B = 2: eager, graph-replayed, under an accumulation
window, slice by slice, swapped under the model, through a checkpoint and through train_dp.

The reference needs no second optimizer: after every update the product's own parameters (`flat_p`, the kernel's p') feed the
fp64 recurrence of tests/_ema_plan.py, and `flat_ema` must stay within the bound the helper counts from the kernel source."""
import gc
import os

import pytest
import torch

import _ema_plan as EP
import _nonconv_plan as NP
import _step_state as SS
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

MODE = "fp32-direct"
LR = 1e-3
S = (32, 32, 32)


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


class Track:
    """The fp64 recurrence beside an optimizer's flat average."""

    def __init__(self, e0):
        self.st = EP.ema_init(e0.detach().reshape(-1))

    def update(self, p_new, got, decay, warm, t, tag):
        d = EP.ema_update(self.st, p_new.detach().reshape(-1), decay, warm, t)
        ratio = R.check_elementwise(got.detach().reshape(-1), self.st["e"], self.st["b"], tag)
        print(f"{tag}: update {t}, d_t {d:.6g}, worst ratio {ratio:.3g}")
        return d


class Bench:
    """A static-prompts model that took `steps` eager steps with the average on, and the recurrence that followed them."""

    def __init__(self, decay=0.9, warm=False, steps=2, **kw):
        import coma_unet_amd as cu
        from coma_unet_amd.train import make_optimizer
        self.model = SS.fresh_model(MODE)
        self.crit = cu.build_reference_criterion()
        self.opt = make_optimizer(self.model, LR, ema_decay=decay, ema_warmup=warm, **kw)
        self.decay, self.warm, self.t = decay, warm, 0
        p0 = {n: p.detach().clone() for n, p in self.model.named_parameters()}
        self.k = 0
        self.track = None
        for _ in range(steps):
            self.eager()
            if self.track is None:            # the layout exists now: e_0 = the parameters before the first update
                o = self.opt
                e0 = torch.zeros_like(o.flat_p)
                for n, off, k in SS.flat_layout(self.model, o):
                    e0[off:off + k] = p0[n].reshape(-1)
                self.track = Track(e0)
            self.moved("warm-up step")

    def next_batch(self):
        self.k += 1
        return SS.batch(MODE, self.k)

    def eager(self, b=None):
        from coma_unet_amd.train import train_step
        train_step(self.model, self.crit, self.opt, b if b is not None else self.next_batch())

    def moved(self, tag):
        """An update was applied: the average must follow the recurrence."""
        self.t += 1
        assert self.opt._flat_step == self.t and int(self.opt._step_dev) == self.t
        return self.track.update(self.opt.flat_p, self.opt.flat_ema, self.decay, self.warm, self.t, tag)


def test_eager_recurrence_flat_buffer_and_loose_prompts():
    """static_prompts=False, four eager steps at ema_decay=0.9 (abeta [1, 0], [0, 1], [1, 1], [0, 0]: the third and fourth
    steps leave one prompt without a gradient, whose average must then stay put)."""
    import coma_unet_amd as cu
    from coma_unet_amd.train import make_optimizer, train_step
    try:
        torch.manual_seed(SS.SEED)
        model = cu.build_model(volume_shape=S, static_prompts=False, compute_dtype=torch.float32, conv_algo=1).cuda()
        model.set_save_attn(None)
        model.train(True)
        crit = cu.build_reference_criterion()
        opt = make_optimizer(model, LR, ema_decay=0.9)
        assert opt.flat_ema is None and opt.averaging
        prompts = [model.pos_dynamic_prompt, model.neg_dynamic_prompt]
        p0 = {n: p.detach().clone() for n, p in model.named_parameters()}
        loose = [Track(p) for p in prompts]                     # (their averages start at the value of their first step)
        stepped, last = [0, 0], [None, None]
        flat = None
        for k in (1, 2, 3, 4):
            train_step(model, crit, opt, SS.batch(MODE, k))
            if flat is None:
                e0 = torch.zeros_like(opt.flat_p)
                for n, off, kk in SS.flat_layout(model, opt):
                    e0[off:off + kk] = p0[n].reshape(-1)
                flat = Track(e0)
                assert all(id(p) not in opt._flat_ids for p in prompts)
            flat.update(opt.flat_p, opt.flat_ema, 0.9, False, k, f"flat step {k}")
            for j, p in enumerate(prompts):
                if p.grad is not None:
                    stepped[j] += 1
                    loose[j].update(p, opt._loose_ema[p], 0.9, False, stepped[j], f"prompt {j} step {k}")
                else:
                    assert torch.equal(opt._loose_ema[p], last[j]), f"prompt {j} had no gradient at step {k}: its average moved"
                last[j] = opt._loose_ema[p].clone()
        assert stepped == [3, 3] and opt._flat_step == 4
        assert not torch.equal(opt.flat_ema, opt.flat_p)
        # parameters that never receive a gradient have no average; the serialised average carries their current value
        sd = opt.ema_state_dict(model)
        none = [n for n, p in model.named_parameters() if id(p) not in opt._flat_ids and p not in opt._loose_ema]
        assert none and all(torch.equal(sd[n], dict(model.named_parameters())[n].detach()) for n in none)
        assert list(sd) == list(model.state_dict())
        # state_dict() stays torch.optim.AdamW-shaped
        osd = opt.state_dict()
        assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in osd["state"].values())
        assert osd["param_groups"][0]["ema_decay"] == 0.9 and osd["param_groups"][0]["ema_warmup"] is False
    finally:
        _free()


def test_graphed_recurrence_with_warmup_and_recapture():
    """Two eager steps, then five replays of one captured step on changing batches with warm-up on: d_t = (1 + t) / (10 + t)
    moves with the DEVICE step count (2/11, 3/12 eager; 4/13 .. 8/17 < 0.9 replayed).  Changing ema_decay re-captures once
    and the next update uses the new value."""
    from coma_unet_amd.train import GraphedTrainStep
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            bn = Bench(decay=0.9, warm=True)
            o = bn.opt
            step = GraphedTrainStep(bn.model, bn.crit, o, bn.next_batch(), prewarmed=True)
            bn.k -= 1                                              # (the capture executed nothing: that batch is still to come)
            assert o._flat_step == 2 and int(o._step_dev) == 2 and step.micro_graph is None
            graph = step.graph
            ds = []
            for _ in range(5):
                before = o.flat_ema.clone()
                step(bn.next_batch())
                ds.append(bn.moved("replay"))
                assert not torch.equal(o.flat_ema, before)
            assert step.graph is graph, "a replay without a changed option must not re-capture"
            assert ds == [(1 + t) / (10 + t) for t in (3, 4, 5, 6, 7)]
            o.param_groups[0]["ema_decay"] = 0.25
            bn.decay = 0.25
            step(bn.next_batch())
            assert step.graph is not graph, "no re-capture after ema_decay changed"
            graph = step.graph
            assert bn.moved("replay after ema_decay changed") == 0.25
            step(bn.next_batch())
            assert step.graph is graph and bn.moved("replay") == 0.25
            o.param_groups[0]["ema_warmup"] = False
            step(bn.next_batch())
            assert step.graph is not graph
            bn.warm = False
            bn.moved("replay after ema_warmup changed")
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    finally:
        _free()


def test_average_moves_on_the_applying_update_only():
    """grad_acc_batch=2: a micro-batch step leaves flat_ema bitwise alone; the applying step and flush() move it."""
    try:
        bn = Bench(decay=0.9)
        o = bn.opt
        o.param_groups[0]["grad_acc_batch"] = 2
        keep = o.flat_ema.clone()
        bn.eager()
        assert o.pending == 1 and torch.equal(o.flat_ema, keep) and o._flat_step == 2
        bn.eager()
        assert o.pending == 0 and not torch.equal(o.flat_ema, keep)
        bn.moved("applying step")
        keep = o.flat_ema.clone()
        bn.eager()
        assert o.pending == 1 and torch.equal(o.flat_ema, keep)
        with pytest.raises(RuntimeError, match=r"flush\(\)"):
            o.swap_ema()
        o.flush()
        assert o.pending == 0 and not torch.equal(o.flat_ema, keep)
        bn.moved("flush()")
        o.param_groups[0]["max_grad_norm"] = 1e-3               # with a clip that bites: still the kernel's own p'
        bn.eager()
        bn.eager()
        assert float(o.last_grad_norm) > 1e-3
        bn.moved("applying step, clipped")
    finally:
        _free()


def _eval(model, b):
    was = model.training
    model.eval()
    model.set_training(False)
    try:
        with torch.no_grad():
            return model(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"]).float().clone()
    finally:
        model.train(was)
        model.set_training(was)


def test_swap_context_puts_the_average_under_the_model():
    import coma_unet_amd as cu
    try:
        bn = Bench(decay=0.9, steps=3)
        o, model = bn.opt, bn.model
        b = SS.batch(MODE, 9)
        p_keep, e_keep = o.flat_p.clone(), o.flat_ema.clone()
        ptrs = [p.data_ptr() for p in model.parameters()]
        y_iter = _eval(model, b)
        twin = SS.fresh_model(MODE)
        twin.load_state_dict(o.ema_state_dict(model))
        y_twin = _eval(twin, b)
        pred = cu.Predictor(model, b, graph=True)
        y_pred_iter = pred().float().clone()
        with o.ema_weights() as inside:
            assert inside is o
            assert torch.equal(o.flat_p, e_keep) and torch.equal(o.flat_ema, p_keep)
            for n, off, k in SS.flat_layout(model, o):
                assert torch.equal(dict(model.named_parameters())[n].detach().reshape(-1), e_keep[off:off + k]), n
            assert [p.data_ptr() for p in model.parameters()] == ptrs, "the swap must be by content"
            y_in = _eval(model, b)
            with pytest.raises(RuntimeError, match="swapped in"):
                o.step()
            with pytest.raises(RuntimeError, match="swapped in"):
                o.state_dict()
            # the serialised average is the same whichever side is in
            for (n, a), (_, c) in zip(o.ema_state_dict(model).items(), twin.state_dict().items()):
                assert torch.equal(a, c), n
            pred.refresh()
            y_pred_in = pred().float().clone()
        pred.refresh()
        y_pred_out = pred().float().clone()
        assert torch.equal(o.flat_p, p_keep) and torch.equal(o.flat_ema, e_keep)
        print(f"eval under the average vs a model loaded from ema_state_dict {rel(y_in, y_twin):.3e}; average vs iterate "
              f"{rel(y_in, y_iter):.3e}; predictor inside {rel(y_pred_in, y_in):.3e}, outside {rel(y_pred_out, y_iter):.3e}")
        # two eval forwards of one set of weights: 1e-5 (test_predictor_gpu.test_model_state_untouched); "different" must
        # stand clear of it (10 x, as test_refresh_picks_up_new_running_statistics)
        assert rel(y_in, y_twin) <= 1e-5
        assert rel(y_in, y_iter) > 1e-4
        assert rel(y_pred_iter, y_iter) <= 1e-5 and rel(y_pred_in, y_in) <= 1e-5 and rel(y_pred_out, y_iter) <= 1e-5
        bn.eager()                                                # and training goes on
        bn.moved("step after the context")
    finally:
        _free()


def _same(got, ref, gscale, what, rtol=5e-3):
    """test_model_gpu._same_step: tensor by tensor to rtol, except tensors whose gradient is rounding noise (|g| <= 1e-6 of the
    largest: Adam turns the fp32 atomics' order into a step of ~lr there)."""
    gmax = max(gscale.values())
    worst = (0.0, "")
    for n, r in ref.items():
        if n not in gscale or float(r.abs().max()) == 0 or gscale[n] <= 1e-6 * gmax:
            continue
        worst = max(worst, (rel(got[n], r), n))
    assert worst[0] < rtol, (what, worst)


def test_checkpoint_carries_the_average(tmp_path):
    """Three steps, save; two more steps uninterrupted against load-into-fresh + two steps: parameters and averages agree to
    what test_resume_into_fresh_optimizer_matches_uninterrupted_run allows for parameters.  The five reference keys are
    unchanged, the file loads with weights_only=True, and a file written without the option leaves the average to start at
    the loaded parameters."""
    import coma_unet_amd as cu
    from coma_unet_amd import checkpoint
    from coma_unet_amd.train import make_optimizer, train_step
    try:
        bn = Bench(decay=0.9, warm=True, steps=3)
        o, model = bn.opt, bn.model
        files = checkpoint.save_checkpoint(str(tmp_path), 3, model, o, torch.tensor(1.0), None, checkpoint_iter=5)
        raw = torch.load(files[0], map_location="cpu", weights_only=True)
        assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "ema_state_dict"}
        assert list(raw["ema_state_dict"]) == list(raw["model_state_dict"])
        assert set(raw["optimizer_state_dict"]) == {"state", "param_groups"}
        assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in raw["optimizer_state_dict"]["state"].values())
        moved = [n for n, _p in model.named_parameters() if not torch.equal(raw["ema_state_dict"][n], raw["model_state_dict"][n])]
        assert len(moved) > 10
        for k, v in raw["model_state_dict"].items():              # buffers (BatchNorm statistics) are not averaged
            if k not in dict(model.named_parameters()):
                assert torch.equal(raw["ema_state_dict"][k], v), k
        for k in (4, 5):
            bn.eager(SS.batch(MODE, k))
            bn.moved(f"uninterrupted step {k}")
        ref_p = {n: p.detach().clone() for n, p in model.named_parameters()}
        ref_e = {n: v.clone() for n, v in o.ema_state_dict(model).items() if n in ref_p}
        gscale = {n: (float(p.grad.abs().max()) if p.grad is not None else 0.0) for n, p in model.named_parameters()}

        torch.manual_seed(99)                                     # different weights: everything must come from the file
        m2 = cu.build_model(volume_shape=S, static_prompts=True, **SS.MODES[MODE][0]).cuda()
        m2.set_save_attn(None)
        m2.train(True)
        o2 = make_optimizer(m2, LR, ema_decay=0.9, ema_warmup=True)
        assert checkpoint.load_checkpoint(files[0], m2, o2, None) == 4
        assert not o2.built and o2.flat_ema is None                # parked until the layout exists
        for (n, a), (_, c) in zip(o2.ema_state_dict(m2).items(), raw["ema_state_dict"].items()):
            assert torch.equal(a.cpu(), c), n
        crit = cu.build_reference_criterion()
        for k in (4, 5):
            train_step(m2, crit, o2, SS.batch(MODE, k))
        assert o2._flat_step == 5 and not o2._ema_parked
        _same({n: p.detach() for n, p in m2.named_parameters()}, ref_p, gscale, "parameters")
        _same(o2.ema_state_dict(m2), ref_e, gscale, "averages")

        # a checkpoint written without the option: the average starts at the loaded parameters
        m3 = SS.fresh_model(MODE)
        o3 = make_optimizer(m3, LR)
        for k in (1, 2):
            train_step(m3, crit, o3, SS.batch(MODE, k))
        assert o3.flat_ema is None and not o3._loose_ema
        d3 = tmp_path / "plain"
        f3 = checkpoint.save_checkpoint(str(d3), 2, m3, o3, torch.tensor(1.0), None)
        raw3 = torch.load(f3[0], map_location="cpu", weights_only=True)
        assert set(raw3) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss"}
        m4 = SS.fresh_model(MODE)
        o4 = make_optimizer(m4, LR, ema_decay=0.5)
        checkpoint.load_checkpoint(f3[0], m4, o4, None)
        assert o4.averaging and o4.param_groups[0]["ema_decay"] == 0.5
        loaded = {n: p.detach().clone() for n, p in m4.named_parameters()}
        train_step(m4, crit, o4, SS.batch(MODE, 3))
        e0 = torch.zeros_like(o4.flat_p)
        for n, off, k in SS.flat_layout(m4, o4):
            e0[off:off + k] = loaded[n].reshape(-1)
        assert o4._flat_step == 3
        Track(e0).update(o4.flat_p, o4.flat_ema, 0.5, False, 3, "first step after a checkpoint without an average")
        # ... and into an optimizer whose layout (and average) already exists
        train_step(m4, crit, o4, SS.batch(MODE, 4))
        checkpoint.load_checkpoint(f3[0], m4, o4, None)
        assert torch.equal(o4.flat_ema, o4.flat_p)
    finally:
        _free()


def test_sharded_exchange_raises_and_slices_follow_the_recurrence():
    from coma_unet_amd import ops
    from coma_unet_amd.data_parallel import GradReducer
    from coma_unet_amd.train import forward_loss, train_step
    try:
        bn = Bench(decay=0.9)
        o = bn.opt
        # a world-size-1 GradReducer step
        red = GradReducer(o, overlap=False)
        assert red.world == 1
        train_step(bn.model, bn.crit, o, bn.next_batch(), red)
        bn.moved("GradReducer, one rank")
        # the step taken slice by slice as the slices' gradients arrive (GradReducer.reduce_flat_and_step): slices that start
        # off 16-byte alignment, an empty one, the loose parameters last; bitwise one whole launch on copies
        o.zero_grad()
        losses, _ = forward_loss(bn.model, bn.crit, bn.next_batch())
        losses[0].backward()
        ops.SidePrep.join()
        n = o.flat_p.numel()
        cuts = [0, 1027, 1027, n // 3 + 1, n - 5, n]
        spans = [(a, c - a) for a, c in zip(cuts, cuts[1:])]
        p, g, m, v, e = (t.clone() for t in (o.flat_p, o.flat_g, o.flat_m, o.flat_v, o.flat_ema))
        for i, sp in enumerate(spans):
            o.step_shards([sp], advance=i == 0, loose=False)
        o.step_shards([], advance=False, loose=True)
        bn.moved("slice by slice")
        # every element was stepped exactly once: the first moment against ONE whole launch on copies.  Not bitwise -- the
        # slices off 16-byte alignment take the kernel's scalar loop, and the compiler contracts the multiply-adds of the two
        # loops differently -- but within twice _nonconv_plan.adamw_step's bound of m (4 roundings over the mass
        # b1 |m| + (1 - b1) |g|, u each, doubled there); an element skipped or stepped twice is off by ~(1 - b1) |g|
        m_old = m.clone()
        ops.adamw_ema_(p, g, m, v, e, 0.9, False, LR, 0.9, 0.999, 1e-8, 1e-2, o._flat_step, o._step_dev)
        mass = NP.f32(0.9) * m_old.double().abs() + (1 - NP.f32(0.9)) * g.double().abs()
        R.check_elementwise(o.flat_m, m.double(), 2 * 2 * 4 * NP.U_F32 * mass, "first moment, slices against one launch")
        assert float((m.double() - m_old.double()).abs().max()) > 1e3 * float((2 * 2 * 4 * NP.U_F32 * mass).max())
        # a sharded exchange: refused before anything is launched
        o.shard_exchange = object()
        keep = o.flat_ema.clone()
        with pytest.raises(ValueError, match="sharded"):
            train_step(bn.model, bn.crit, o, bn.next_batch())
        with pytest.raises(ValueError, match="sharded"):
            o.step_shards([(0, 8)])
        o.shard_exchange = None
        assert torch.equal(o.flat_ema, keep) and o._flat_step == bn.t
    finally:
        _free()


def test_option_off_allocates_nothing_and_adds_no_key():
    import coma_unet_amd as cu
    from coma_unet_amd import checkpoint
    from coma_unet_amd.train import GraphedTrainStep, make_optimizer, train_step
    try:
        model = SS.fresh_model(MODE)
        crit = cu.build_reference_criterion()
        opt = make_optimizer(model, LR)
        for k in (1, 2):
            train_step(model, crit, opt, SS.batch(MODE, k))
        assert opt.flat_ema is None and not opt._loose_ema and not opt._ema_parked and not opt.averaging
        ck = checkpoint.checkpoint_dict(0, model, opt, torch.tensor(0.0))
        assert "ema_state_dict" not in ck and set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss"}
        with pytest.raises(RuntimeError, match="ema_decay"):
            opt.swap_ema()
        # switched on later: the average starts at the parameters of that moment, allocated outside the capture
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            step = GraphedTrainStep(model, crit, opt, SS.batch(MODE, 3), prewarmed=True)
            assert opt.flat_ema is None
            step(SS.batch(MODE, 3))
            opt.param_groups[0]["ema_decay"] = 0.5
            start = opt.flat_p.clone()
            step(SS.batch(MODE, 4))
            assert opt._flat_step == 4
            Track(start).update(opt.flat_p, opt.flat_ema, 0.5, False, 4, "first replay after the option was switched on")
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
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


@pytest.mark.parametrize("ema_eval", [True, False], ids=["ema_eval", "iterate_eval"])
def test_train_dp_evaluates_under_the_average_and_checkpoints_it(tmp_path, monkeypatch, ema_eval):
    """One epoch of three batches with ema_decay=0.9: the validation pass sees the averaged weights (ema_eval) or the iterate,
    a predictor passed through is refreshed inside and after, and the checkpoint carries the average."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import train_loop
    try:
        train, lk1 = _loader(3, 2, [[1, 0], [0, 1], [1, 1]], seed0=70)
        val, lk2 = _loader(1, 2, [[1, 0]], seed0=90, triplet=False)
        torch.manual_seed(11)
        m = cu.build_model(volume_shape=S).cuda()
        m.set_save_attn(None)
        m.train(True)
        seen = {}
        orig_opt, orig_test = train_loop.make_optimizer, train_loop.contrastive_test

        def spy_opt(*a, **kw):
            seen["opt"] = orig_opt(*a, **kw)
            return seen["opt"]

        class FakePredictor:
            log = []

            def refresh(self):
                self.log.append(seen["opt"]._ema_in)

            def fits(self, mri):
                return False

        def spy_test(model, *a, **kw):
            o = seen["opt"]
            seen["in"] = o._ema_in
            seen["predictor"] = kw.get("predictor")
            seen["flat_p"] = o.flat_p.clone()
            return orig_test(model, *a, **kw)

        monkeypatch.setattr(train_loop, "make_optimizer", spy_opt)
        monkeypatch.setattr(train_loop, "contrastive_test", spy_test)
        fake = FakePredictor()
        losses = A.train_dp(m, cu.build_reference_criterion(), train, val, 1, 1e-3, save_path=str(tmp_path), cuda_id=0,
                            roi_vecs_dict={**lk1, **lk2}, graph=False, ema_decay=0.9, ema_warmup=True, ema_eval=ema_eval,
                            predictor=fake)
        o = seen["opt"]
        assert len(losses) == 1 and o.averaging and o.param_groups[0]["ema_warmup"] is True and o._flat_step == 3
        assert seen["in"] is ema_eval and not o._ema_in
        assert seen["predictor"] is fake
        assert fake.log == ([True, False] if ema_eval else [])
        assert torch.equal(seen["flat_p"], o.flat_ema if ema_eval else o.flat_p)
        assert not torch.equal(o.flat_ema, o.flat_p) and m.training
        raw = torch.load(os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth"), map_location="cpu",
                         weights_only=True)
        assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "scheduler_state_dict", "ema_state_dict"}
        for n, off, k in SS.flat_layout(m, o):
            assert torch.equal(raw["ema_state_dict"][n].reshape(-1), o.flat_ema[off:off + k].cpu()), n
            assert torch.equal(raw["model_state_dict"][n].reshape(-1), o.flat_p[off:off + k].cpu()), n
    finally:
        _free()
