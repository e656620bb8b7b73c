"""Harness of tests/test_step_state_gpu.py: a training trajectory whose step k is a pure function of (weights_k, batch_k),
a stateless reference for that step, and a per-tensor comparison of the two.

The stateful run keeps everything the product carries from one step to the next (flat gradient buffer with the sparse
zero_grad, ops.GradSink, ops.ZeroArena, the ops.PrepAhead plan and its persistent buffers, ops.WgradSide, a captured graph).
The reference runs the SAME kernels on a model that has never taken a step, with all of that switched off: whatever differs
beyond the reference's own repeat spread was carried over from another step.  Every step sees other weights (`perturb`) and
another batch (`batch`), so a stale value is not a fresh one.  The learning rate is 0: AdamW leaves the weights alone and
`perturb` alone decides them.
"""
import contextlib
import copy
import zlib

import torch

SEED = 4
A = 0.1                      # relative size of a perturbation
WARMUP = 3                   # step 1 builds the flat layout and records the PrepAhead plan, the sinks are live from step 2,
                             # the sparse zero_grad table is in force from step 3's zero_grad
MEASURED = (4, 5, 6, 7)
ABETA = ([1, 0], [0, 1], [1, 1], [0, 0])       # step k takes ABETA[(k - 1) % 4]: each prompt meets a step without its class

MODES = {          # name -> (build_model keywords, volume)
    "fp32-direct": (dict(compute_dtype=torch.float32, conv_algo=1), (32, 32, 32)),
    "fp32-auto": (dict(compute_dtype=torch.float32, conv_algo=0), (32, 32, 32)),
    "bf16-auto": (dict(compute_dtype=torch.bfloat16, conv_algo=0), (32, 32, 32)),      # what bench.py runs
    "split": (dict(compute_dtype=torch.float32, conv_algo=4), (32, 32, 32)),
    # the wide split's stride-2 / transposed kernels are first picked at 64^3 (test_split_wide_mode_gpu.py)
    "split-wide": (dict(compute_dtype=torch.float32, conv_algo=5), (64, 64, 64)),
}

# Bounds: the stateless reference's own repeat spread (five evaluations of one (weights, batch), every pair compared in the
# form of `bound`, worst tensor of the class over the four measured steps; the worst of all recorded runs, since the
# merge-order noise of the atomics is heavy-tailed and five repeats undersample it) times 4, rounded up to two digits.
# Measured by profiles/step_state_noise.py; the spreads, these constants and the power figures: profiles/step_state_noise.txt.
# fp32-direct starts from the 1e-3 per tensor of test_write_through_gradients_equal_autograd_accumulation and the 1e-5 on
# the loss of the side-stream tests; its measured spread (2e-6) does not ask for more.  The loss is one fp32 number: no loss
# bound below 8 ulp (9.6e-7).
TOL = {
    "fp32-direct": {"conv": 1e-3, "scalar": 1e-3, "prompt": 1e-3, "loss": 1e-5},
    "fp32-auto": {"conv": 0.11, "scalar": 0.84, "prompt": 0.011, "loss": 9.6e-7},
    "bf16-auto": {"conv": 3.3, "scalar": 83.0, "prompt": 0.6, "loss": 9.8e-4},
    "split": {"conv": 0.039, "scalar": 0.43, "prompt": 0.033, "loss": 9.6e-7},
    "split-wide": {"conv": 0.028, "scalar": 0.18, "prompt": 0.019, "loss": 9.6e-7},
}
# Power (consecutive reference steps at least 4 bounds apart on all but 5 % of the tensors / 0.1 % of the elements) is met by
# the reference alone on the direct kernels only.  The other modes' ill-conditioned scalars (PReLU slopes, the one-channel
# gate norms: repeat spread 4e-2 .. 20) put class `scalar`'s bound beyond the distance of two unrelated gradients, so 24-49 %
# of the TENSORS (0.001-0.004 % of the elements) are weak in the fp32 MFMA / split modes, and with bf16 storage every class
# is (78 % of the tensors, 99.97 % of the elements): there the comparison sees non-finite or grossly wrong values only.  The
# tests print the figures for every mode and assert the condition where it is met.
POWER_MET = ("fp32-direct",)
FLOOR = 1e-6                 # absolute part of a bound: tol * FLOOR * gmax * sqrt(numel)
POWER = 4.0                  # consecutive reference steps must lie at least POWER bounds apart
POWER_MAX_TENSORS, POWER_MAX_ELEMENTS = 0.05, 0.001


def tensor_class(name):
    """conv: convolution masters and biases; prompt: the learned prompts; scalar: norm affine parameters, PReLU slopes,
    routing weights and biases, the final linear head."""
    if "prompt" in name:
        return "prompt"
    if ".routing." not in name and (name.endswith("conv.weight") or name.endswith("conv.bias")):
        return "conv"
    return "scalar"


# ------------------------------------------------------------------------------------------------------------------
# models, perturbations, batches (all cached for the module: nothing here is ever written to again)
# ------------------------------------------------------------------------------------------------------------------
_templates, _factors, _batches = {}, {}, {}


def _template(mode):
    import coma_unet_amd as cu
    kw, S = MODES[mode]
    if mode not in _templates:
        torch.manual_seed(SEED)
        _templates[mode] = cu.build_model(volume_shape=S, static_prompts=True, **kw)
    return _templates[mode]


def fresh_model(mode):
    """A model that has never run, with the weights of SEED (a copy of a template that is itself never used)."""
    m = copy.deepcopy(_template(mode)).cuda()
    m.set_save_attn(None)
    m.train(True)
    return m


def perturb(model, k):
    """p *= 1 + A * u in place (the optimizer's flat-buffer views survive), u uniform in [-1, 1) drawn on the CPU from a
    generator seeded by crc32(name) + k."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            key = (name, tuple(p.shape), k)
            u = _factors.get(key)
            if u is None:
                g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + k)
                u = _factors[key] = (torch.rand(p.shape, generator=g) * 2.0 - 1.0).to(p.device)
            p.data.mul_(1.0 + A * u)


def batch(mode, k):
    """Batch of step k: its own seed, abeta flags forced through ABETA, priors as the (B, 36, 2) device tensor."""
    from coma_unet_amd.synthetic import make_batch
    S = MODES[mode][1]
    if (S, k) not in _batches:
        b = make_batch(2, S, seed=100 + k)
        b["covars"][:, 0, 0] = torch.tensor(ABETA[(k - 1) % 4], dtype=b["covars"].dtype)
        gb = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in b.items()}
        gb["roi_pred_dicts"] = _template(mode)._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        _batches[(S, k)] = gb
    return _batches[(S, k)]


@contextlib.contextmanager
def switches(**kw):
    """Set ops.<Class>.enabled for PrepAhead / SidePrep / WgradSide / ZeroArena, restore on exit."""
    from coma_unet_amd import ops
    was = {n: getattr(ops, n).enabled for n in kw}
    try:
        for n, v in kw.items():
            getattr(ops, n).enabled = v
        yield
    finally:
        for n, v in was.items():
            getattr(ops, n).enabled = v


def ops_counts():
    from coma_unet_amd import ops
    return ops.WgradSide.launched


def grads_of(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


# ------------------------------------------------------------------------------------------------------------------
# the stateless reference
# ------------------------------------------------------------------------------------------------------------------
_refs, _ref_params = {}, {}


def stateless(model, b):
    """One zero_grad, forward_loss, backward on a model that never stepped: no flat buffer (the optimizer is never built),
    no sinks, no arena, no plan, one stream."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss, make_optimizer
    with switches(PrepAhead=False, SidePrep=False, WgradSide=False, ZeroArena=False):
        opt = make_optimizer(model, 0.0, write_through=False)
        opt.zero_grad()
        losses, _ = forward_loss(model, cu.build_reference_criterion(), b)
        losses[0].backward()
        ops.SidePrep.join()
        torch.cuda.synchronize()
        assert not opt.built
    return grads_of(model), float(losses[0])


def reference(mode, k, weights=None):
    """(gradients, loss) of step k from a fresh model with perturb 1..k applied; cached per (mode, k).  `weights`: the
    stateful run's parameters at that step -- they must be the very same numbers."""
    if (mode, k) not in _refs:
        m = fresh_model(mode)
        for j in range(1, k + 1):
            perturb(m, j)
        _ref_params.setdefault((MODES[mode][1], k), {n: p.detach().clone() for n, p in m.named_parameters()})
        _refs[(mode, k)] = stateless(m, batch(mode, k))
    g, loss = _refs[(mode, k)]
    if weights is not None:
        params = _ref_params[(MODES[mode][1], k)]
        for n, p in weights:
            assert torch.equal(p.detach(), params[n]), f"step {k}: parameter {n} of the stateful run is not the reference's"
    return g, loss


def reference_at(mode, model, b):
    """Uncached: the stateless step of a fresh model that is given `model`'s current weights (for runs whose weights moved)."""
    m = fresh_model(mode)
    with torch.no_grad():
        for (n, p), (_, q) in zip(m.named_parameters(), model.named_parameters()):
            p.data.copy_(q.data)
    return stateless(m, b)


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def _norms(ts):
    return torch.stack(torch._foreach_norm([t.reshape(-1).float() for t in ts])).double().cpu()


def distances(got, ref):
    """Per tensor with a gradient: (name, numel, |got - ref|, |ref|), and gmax = the largest reference gradient magnitude."""
    names = [n for n in ref if ref[n] is not None]
    for n in ref:
        assert (got[n] is None) == (ref[n] is None), f"{n}: gradient {'missing' if got[n] is None else 'unexpected'}"
    d = _norms(torch._foreach_sub([got[n].reshape(-1).float() for n in names], [ref[n].reshape(-1).float() for n in names]))
    r = _norms([ref[n] for n in names])
    gmax = float(torch.stack([ref[n].abs().max() for n in names]).max())
    return [(n, ref[n].numel(), float(d[i]), float(r[i])) for i, n in enumerate(names)], gmax


def flat_layout(model, opt):
    """[(name, offset, numel)] of the optimizer's flat buffers."""
    return [(n,) + tuple(opt._offsets[id(p)]) for n, p in model.named_parameters() if id(p) in opt._offsets]


def flat_slices(layout, flat):
    """{name: slice} of a copy of a flat buffer: the per-tensor view `compare` takes."""
    return {n: flat[off:off + k] for n, off, k in layout}


def bound(tol, numel, rnorm, gmax):
    return tol * rnorm + tol * FLOOR * gmax * numel ** 0.5


def compare(mode, got, ref, loss=None, ref_loss=None):
    """List of mismatches (empty: the step carried nothing): (name, |got - ref|, bound) for every tensor beyond its bound,
    no tensor excluded, plus the loss."""
    tol = TOL[mode]
    dist, gmax = distances(got, ref)
    bad = []
    for n, numel, d, r in dist:
        b = bound(tol[tensor_class(n)], numel, r, gmax)
        if not d <= b:          # (a NaN is a mismatch)
            bad.append((n, d, b))
    if loss is not None and not abs(loss - ref_loss) <= tol["loss"] * abs(ref_loss):
        bad.append(("loss", abs(loss - ref_loss), tol["loss"] * abs(ref_loss)))
    return bad


def power(mode, ref, prev):
    """Tensors whose reference gradients of two consecutive steps lie closer than POWER bounds: a value left over from the
    previous step would pass there.  -> (names, share of the tensors, share of the elements, names of the tensors whose
    gradient is exactly zero in both steps).  The last group is not counted as weak: those are the convolution biases in
    front of a mean-removing normalisation, whose gradient the kernels return as exact zeros (layers.Config,
    zero_bias_grad_under_norm) -- a value left over from the previous step IS the fresh value there, and anything else in
    such a slot is beyond the absolute part of its bound."""
    tol = TOL[mode]
    dist, gmax = distances(prev, ref)
    zero = [n for n, numel, d, r in dist if d == 0.0 and r == 0.0]
    weak = [(n, numel) for n, numel, d, r in dist
            if n not in zero and not d >= POWER * bound(tol[tensor_class(n)], numel, r, gmax)]
    total = sum(numel for _, numel, _, _ in dist)
    return [n for n, _ in weak], len(weak) / len(dist), sum(k for _, k in weak) / total, zero


def check_power(mode, k):
    weak, share_t, share_e, zero = power(mode, reference(mode, k)[0], reference(mode, k - 1)[0])
    print(f"{mode} step {k}: {len(weak)} tensors ({share_t:.1%} of the tensors, {share_e:.4%} of the elements) move less than "
          f"{POWER:g} bounds from step {k - 1}: {weak}; exactly zero in both steps: {len(zero)}")
    return share_t <= POWER_MAX_TENSORS and share_e <= POWER_MAX_ELEMENTS


# ------------------------------------------------------------------------------------------------------------------
# the stateful run
# ------------------------------------------------------------------------------------------------------------------
class Run:
    """Default switches unless the caller changed them: write-through, sparse zero_grad, arena, PrepAhead, WgradSide."""

    def __init__(self, mode, graph=False, lr=0.0):
        import coma_unet_amd as cu
        from coma_unet_amd import ops
        from coma_unet_amd.train import GraphedTrainStep, make_optimizer, train_step
        self.mode, self.graph = mode, graph
        self.model = fresh_model(mode)
        self.opt = make_optimizer(self.model, lr)
        self.crit = cu.build_reference_criterion()
        for k in range(1, WARMUP + 1):
            perturb(self.model, k)
            train_step(self.model, self.crit, self.opt, batch(mode, k))
        self.step = None
        self.capture_counts = None
        self.prep_ahead_used = 0       # layers served from the up-front preparation over the measured steps
        self.wgrad_side_launched = 0   # weight gradients sent to the side stream over the measured steps
        if graph:
            n = (ops.PrepAhead.used, ops.WgradSide.launched)
            self.step = GraphedTrainStep(self.model, self.crit, self.opt, batch(mode, WARMUP), prewarmed=True)
            self.capture_counts = (ops.PrepAhead.used - n[0], ops.WgradSide.launched - n[1])

    def take(self, k, before=None, same_weights=True):
        """Step k -> (gradients, loss).  `before(run)` runs between the perturbation and the step.  Asserts that the weights
        are the reference's (unless the run has moved them itself) and that every mechanism that is switched on was live in
        this step (under graph replay the host-side counters move at capture only)."""
        from coma_unet_amd import ops
        from coma_unet_amd.train import train_step
        perturb(self.model, k)
        if same_weights:
            reference(self.mode, k, self.weights())
        if before is not None:
            before(self)
        n = (ops.PrepAhead.used, ops.WgradSide.launched)
        arena = ops.ZeroArena._arenas.get(torch.cuda.current_device()) if ops.ZeroArena.enabled else None
        if arena is not None and not self.graph:
            arena.peak = 0
        if self.graph:
            losses, _ = self.step(batch(self.mode, k))
        else:
            losses, _ = train_step(self.model, self.crit, self.opt, batch(self.mode, k))
        torch.cuda.synchronize()
        used, launched = (ops.PrepAhead.used - n[0], ops.WgradSide.launched - n[1]) if not self.graph else self.capture_counts
        opt = self.opt
        if opt.write_through and opt.sparse_zero:
            assert opt._zero_tab is not None and len(opt._zero_big) > 0, "the sparse zero_grad table is not in force"
        if ops.PrepAhead.enabled and not ops.SidePrep.enabled:
            plans = [p for p in self.model.__dict__.get("_prep_ahead_plans", {}).values() if isinstance(p, list)]
            assert len(plans) == 1 and used == len(plans[0]) >= 40, f"PrepAhead served {used} layers of {[len(p) for p in plans]}"
            self.prep_ahead_used += used
        if ops.SidePrep.enabled:
            assert len(ops.SidePrep._bufs) > 40
        if ops.WgradSide.enabled and opt.write_through:
            assert launched > 0, "WgradSide launched no weight gradient"
            self.wgrad_side_launched += launched
        if arena is not None:
            assert arena.peak > 0, "the zeroed arena was not used"
        assert int(opt._step_dev) == opt._flat_step == k, (int(opt._step_dev), opt._flat_step, k)
        return grads_of(self.model), float(losses[0])

    def weights(self):
        return list(self.model.named_parameters())


def trajectory(mode, graph=False, before=None, steps=MEASURED):
    """The standard test body: warm up, then every measured step against its reference.  -> list of (k, mismatches)."""
    for k in steps:
        reference(mode, k)
    run = Run(mode, graph=graph)
    out = []
    for k in steps:
        ref_g, ref_l = reference(mode, k)
        got_g, got_l = run.take(k, before)
        bad = compare(mode, got_g, ref_g, got_l, ref_l)
        print(f"{mode}{' graph' if graph else ''} step {k}: loss {got_l:.6f} vs {ref_l:.6f}; {len(bad)} mismatches {bad[:8]}")
        out.append((k, bad))
    # the thresholds of test_weight_preparation_ahead_equals_inline / test_side_stream_weight_gradients_equal_one_stream: they
    # hold for a run of steps (one step serves every layer of the plan and launches as many weight gradients beside the
    # chain as the model has layers with one).  A replay moves no host-side counter: `take` checked the capture's own.
    from coma_unet_amd import ops
    if not graph and len(steps) > 1:
        if ops.PrepAhead.enabled and not ops.SidePrep.enabled:
            assert run.prep_ahead_used >= 60, run.prep_ahead_used
        if ops.WgradSide.enabled:
            assert run.wgrad_side_launched >= 40, run.wgrad_side_launched
    return run, out
