"""What the training step carries from one step to the next -- the flat gradient buffer behind the sparse zero_grad,
ops.GradSink, ops.ZeroArena, the ops.PrepAhead plan and its persistent buffers, ops.SidePrep, ops.WgradSide, the captured
graph's static inputs and device-side step counter -- under weights and batches that change every step.

Every measured step is compared, tensor by tensor, with a stateless evaluation of the same (weights, batch) on a model that
never took a step (tests/_step_state.py).  The same kernels run on both sides: kernel numerics are pinned elsewhere
(test_production_shapes_gpu.py, test_ops_gpu.py); a difference here is state that leaked from another step.  Bounds and
their measurement: _step_state.TOL, profiles/step_state_noise.txt.
"""
import pytest
import torch

import _step_state as ss

pytestmark = pytest.mark.gpu


def _clean(out):
    for k, bad in out:
        assert not bad, (k, bad[:10])


@pytest.mark.parametrize("mode", list(ss.MODES))
def test_eager_steps_carry_nothing(mode):
    """Default switches (write-through, sparse zero_grad, arena, PrepAhead, WgradSide), eager steps."""
    met = [ss.check_power(mode, k) for k in ss.MEASURED]
    assert all(met) or mode not in ss.POWER_MET, met
    _, out = ss.trajectory(mode)
    _clean(out)


@pytest.mark.parametrize("mode", ["bf16-auto", "fp32-direct"])
def test_graph_replay_carries_nothing(mode):
    """GraphedTrainStep captured after the warm-up steps: the weights are perturbed outside the graph, the batch goes through
    the static input buffers, the step counter lives on the device."""
    run, out = ss.trajectory(mode, graph=True)
    _clean(out)
    assert run.opt._flat_step == ss.MEASURED[-1]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_side_prep_carries_nothing(graph):
    """ops.SidePrep's persistent per-layer weight buffers (opt-in), on the deterministic direct kernels."""
    from coma_unet_amd import ops
    try:
        with ss.switches(SidePrep=True):
            _, out = ss.trajectory("fp32-direct", graph=graph)
            torch.cuda.synchronize()
    finally:
        ops.SidePrep._bufs.clear()
    _clean(out)


def _poison(run):
    """NaN into every gradient slot zero_grad() skips and every persistent preparation buffer."""
    from coma_unet_amd import ops
    opt = run.opt
    n = 0
    for p in opt._flat_params:
        if id(p) in opt._zero_big:
            p.grad.fill_(float("nan"))
            n += 1
    assert n == len(opt._zero_big) > 0
    bufs = []
    for plan in run.model.__dict__.get("_prep_ahead_plans", {}).values():
        if isinstance(plan, list):
            for e in plan:
                r, bm, wk = e["bufs"] if e["bufs"] is not None else (None, None, None)
                bufs += [r, bm] + list(wk or ())
    if ops.SidePrep.enabled:
        for ent in ops.SidePrep._bufs.values():
            bufs += [ent[1], ent[2]]
    bufs = [t for t in bufs if t is not None]
    assert len(bufs) >= 60, len(bufs)
    for t in bufs:
        t.fill_(float("nan"))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_poisoned_slots_and_buffers_are_rewritten(graph):
    """The sparse zero_grad rests on every backward kernel overwriting its whole slot, the persistent preparation buffers on
    being refilled before they are read: with NaN in all of them before each step, the gradients must still be finite and
    the reference's."""
    run, out = ss.trajectory("bf16-auto", graph=graph, before=_poison)
    assert bool(torch.isfinite(run.opt.flat_g).all())
    _clean(out)


def test_sparse_zero_falls_back_when_a_big_tensor_is_not_written():
    """A large master that gets no gradient after the table was built: its slot (which zero_grad skipped) is cleared before
    the update reads it, its first moment only decays, and zero_grad goes back to full clears."""
    mode = "fp32-direct"
    run = ss.Run(mode, lr=1e-5)          # (lr > 0: the update must really run on the cleared slot)
    opt = run.opt
    assert opt._zero_tab is not None
    name, p = next((n, p) for n, p in run.model.named_parameters() if id(p) in opt._zero_big and n.endswith("merge.conv.weight"))
    off, k = opt._offsets[id(p)]
    assert k >= (1 << 16) and float(opt.flat_g[off:off + k].abs().max()) > 0
    m_old = opt.flat_m[off:off + k].clone()
    assert float(m_old.abs().max()) > 0
    p.requires_grad_(False)
    try:
        run.take(4, same_weights=False)
    finally:
        p.requires_grad_(True)
    assert float(opt.flat_g[off:off + k].abs().max()) == 0.0, name
    b1 = opt.param_groups[0]["betas"][0]
    # m <- b1 * m + (1 - b1) * 0: one fp32 multiply (a fused form of it rounds once more: a few ulp)
    assert torch.allclose(opt.flat_m[off:off + k], m_old * b1, rtol=1e-6, atol=0.0)
    assert opt.sparse_zero is False and opt._zero_tab is None and not opt._zero_big
    for step in (5, 6):
        ss.perturb(run.model, step)
        ref_g, ref_l = ss.reference_at(mode, run.model, ss.batch(mode, step))
        from coma_unet_amd.train import train_step
        losses, _ = train_step(run.model, run.crit, opt, ss.batch(mode, step))
        torch.cuda.synchronize()
        bad = ss.compare(mode, ss.grads_of(run.model), ref_g, float(losses[0]), ref_l)
        assert not bad, (step, bad[:10])


@pytest.mark.parametrize("mode", ["fp32-direct", "bf16-auto"])
def test_arena_exhaustion_falls_back_to_fresh_zeros(mode):
    """A 1 MB arena: most takers get None and fall back to fresh zeros / the library's own memsets, in the middle of a step
    whose other takers hold arena slices (the direct kernels for a bound with power, bf16 for the MFMA kernels' scratch)."""
    from coma_unet_amd import ops
    run = ss.Run(mode)
    key = torch.cuda.current_device()
    big, nbytes = ops.ZeroArena._arenas[key], ops.ZeroArena.nbytes
    try:
        ops.ZeroArena.nbytes = 1 << 20
        small = ops.ZeroArena._arenas[key] = ops.ZeroArena(torch.device("cuda", key))
        ops.ZeroArena.nbytes = nbytes
        for k in (4, 5):
            ref_g, ref_l = ss.reference(mode, k)
            got_g, got_l = run.take(k)
            bad = ss.compare(mode, got_g, ref_g, got_l, ref_l)
            assert not bad, (k, bad[:10])
        assert small.missed > 0 and small.buf.numel() == 1 << 20
    finally:
        ops.ZeroArena.nbytes = nbytes
        ops.ZeroArena._arenas[key] = big


# -- the comparison has teeth: host-level mutations of one step must be reported ---------------------------------------
def test_harness_reports_a_skipped_gradient_clear(monkeypatch):
    from coma_unet_amd import ops
    from coma_unet_amd.optim import FusedAdamW
    mode = "fp32-direct"
    run = ss.Run(mode)
    ref_g, ref_l = ss.reference(mode, 4)

    def no_clear(self, set_to_none=True):
        ops.GradSink.begin_step()          # (the step's bookkeeping, without the clear of the flat buffer)

    monkeypatch.setattr(FusedAdamW, "zero_grad", no_clear)
    got_g, got_l = run.take(4)
    monkeypatch.undo()
    bad = ss.compare(mode, got_g, ref_g, got_l, ref_l)
    print("skipped clear:", len(bad), bad[:8])
    assert bad and all(n != "loss" for n, _, _ in bad)
    ref_g, ref_l = ss.reference(mode, 5)         # and the next, unpatched, step is clean again
    got_g, got_l = run.take(5)
    assert not ss.compare(mode, got_g, ref_g, got_l, ref_l)


def test_harness_reports_unrefreshed_weight_buffers(monkeypatch):
    from coma_unet_amd import ops
    mode = "fp32-direct"
    run = ss.Run(mode)
    ref_g, ref_l = ss.reference(mode, 4)
    real = ops._prep_fwd

    def stale(master, r, transposed, fwd_dtype, dgrad_dtype, bufs=None):
        if bufs is None:
            return real(master, r, transposed, fwd_dtype, dgrad_dtype)
        _, _, rr, meta = real(master, r, transposed, fwd_dtype, dgrad_dtype)     # (fresh weights, thrown away)
        return bufs[0], bufs[1], rr, meta                                          # the persistent ones, as step 3 left them

    monkeypatch.setattr(ops, "_prep_fwd", stale)
    got_g, got_l = run.take(4)
    monkeypatch.undo()
    bad = ss.compare(mode, got_g, ref_g, got_l, ref_l)
    print("stale weights:", len(bad), bad[:8])
    assert len(bad) > 50 and any(n == "loss" for n, _, _ in bad)
