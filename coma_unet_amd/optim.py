"""Fused AdamW on flat fp32 buffers (torch.optim.AdamW semantics; the reference builds
``torch.optim.AdamW(model.parameters(), lr)``, attn_unet_data_parallel.py:736).

Parameters that receive a gradient in the first step are packed into ONE flat parameter
buffer and ONE flat gradient buffer (``p.data`` / ``p.grad`` become views), so a step is a
single HBM-bound kernel launch and the data-parallel gradient exchange can all-reduce
contiguous buckets of the same buffer.  Parameters whose gradient is ``None`` are skipped
exactly as torch does (no decay, no moment update, no step count): the reference model has
~75 such tensors ("aux model heads never used in forward").

``grad_acc_batch=K`` / ``max_grad_norm``: gradient accumulation over K micro-batches and global-norm clipping inside the
step's own kernels (``ops.grad_accum_`` / ``ops.adamw_ex_``), replay-safe.  The gradient applied is the MEAN over the
window's micro-batches (the ``(loss / K).backward()`` idiom; the reference's commented-out ``grad_acc_batch`` lines,
attn_unet_data_parallel.py:887-890, do not divide -- the mean keeps ``lr`` comparable across K).

``ema_decay=d`` / ``ema_warmup``: an exponential moving average of the weights, moved by the update's own kernel
(``ops.adamw_ema_``: the parameter is in registers there already) into ``flat_ema``, a buffer with ``flat_p``'s layout;
``swap_ema()`` / ``ema_weights()`` exchange parameters and average by content (``ops.swap_f32_``), so that every view and every
captured graph keeps its address; ``ema_state_dict`` / ``load_ema_state_dict`` serialise it.  With the option off nothing of it
exists.

``lr_schedule`` / ``param_options``: the update's kernel forms its own learning rate -- a base rate held in device memory
times warm-up and decay factors (``LRSchedule``) evaluated at the device update count -- and takes ``lr_scale`` /
``weight_decay`` per parameter from a device table of segments of the flat buffer (``ops.adamw_sched_``).  A replayed graph
walks through the schedule and a plateau scheduler's change of ``param_groups[0]["lr"]`` needs no new capture.  With both
options off nothing of it exists and the launches are the ones above.
"""
from __future__ import annotations

import math

import torch

from . import ops


NO_EXCHANGE = ("grad_acc_batch > 1 / max_grad_norm are not supported under a data-parallel gradient exchange (sharded steps, "
               "GradReducer, StreamedGradExchange): the exchange of an accumulated gradient and the clip of a sharded one are "
               "not implemented")


def _check_window_opts(grad_acc_batch, max_grad_norm):
    if isinstance(grad_acc_batch, bool) or int(grad_acc_batch) != grad_acc_batch or int(grad_acc_batch) < 1:
        raise ValueError(f"grad_acc_batch must be an integer >= 1, got {grad_acc_batch!r}")
    if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
        raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm!r}")


NO_EMA_SHARDED = ("ema_decay is not supported under a sharded gradient exchange (StreamedGradExchange(sharded=True)): each rank "
                  "updates only its own slices of the parameters there, and the averages of the other slices are not gathered")
EMA_IN = "the averaged weights are swapped in (swap_ema() / ema_weights()): swap them out before {}"


def _check_ema_opts(ema_decay, ema_warmup):
    if ema_decay is not None:
        if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or lie strictly inside (0, 1), got {ema_decay!r}")
    if not isinstance(ema_warmup, (bool, int)) or ema_warmup not in (0, 1):
        raise ValueError(f"ema_warmup must be a bool, got {ema_warmup!r}")


class LRSchedule:
    """Per-update learning-rate factor: linear warm-up (torch's ``LinearLR(start_factor=warmup_start,
    total_iters=warmup_steps)``), then one of ``constant``, ``cosine`` (``CosineAnnealingLR``'s closed form with
    ``eta_min = min_ratio * base``, held at ``min_ratio`` from ``total_steps`` on), ``linear`` (down to ``min_ratio`` over
    ``total_steps``) or ``step`` (``StepLR(step_size, gamma)``), counted from the end of the warm-up.  ``factor(s)`` is the
    factor of the update that follows ``s`` applied updates (torch's convention: ``scheduler.step()`` behind
    ``optimizer.step()``); the kernel (coma_adamw_sched) evaluates the same definition in fp32 on the device."""

    KINDS = ops.SCHED_KINDS

    def __init__(self, warmup_steps=0, warmup_start=1.0 / 3.0, decay="constant", total_steps=None, min_ratio=0.0,
                 step_size=None, gamma=0.1):
        def whole(x):
            return not isinstance(x, bool) and isinstance(x, int)

        def real(x):
            return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)
        if not whole(warmup_steps) or warmup_steps < 0 or warmup_steps >= 2 ** 31:
            raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}")
        if not real(warmup_start) or not 0.0 < warmup_start <= 1.0:
            raise ValueError(f"warmup_start must lie inside (0, 1], got {warmup_start!r}")
        if decay not in self.KINDS:
            raise ValueError(f"decay must be one of {self.KINDS}, got {decay!r}")
        if decay in ("cosine", "linear"):
            if not whole(total_steps) or total_steps < 1 or total_steps >= 2 ** 31:
                raise ValueError(f"decay={decay!r} needs total_steps, an integer >= 1, got {total_steps!r}")
        elif total_steps is not None and (not whole(total_steps) or total_steps < 1 or total_steps >= 2 ** 31):
            raise ValueError(f"total_steps must be None or an integer >= 1, got {total_steps!r}")
        if not real(min_ratio) or not 0.0 <= min_ratio <= 1.0:
            raise ValueError(f"min_ratio must lie inside [0, 1], got {min_ratio!r}")
        if decay == "step":
            if not whole(step_size) or step_size < 1 or step_size >= 2 ** 31:
                raise ValueError(f"decay='step' needs step_size, an integer >= 1, got {step_size!r}")
        elif step_size is not None and (not whole(step_size) or step_size < 1 or step_size >= 2 ** 31):
            raise ValueError(f"step_size must be None or an integer >= 1, got {step_size!r}")
        if not real(gamma) or not 0.0 < gamma <= 1.0:
            raise ValueError(f"gamma must lie inside (0, 1], got {gamma!r}")
        self.warmup_steps, self.warmup_start, self.decay = warmup_steps, float(warmup_start), decay
        self.total_steps, self.min_ratio, self.step_size, self.gamma = total_steps, float(min_ratio), step_size, float(gamma)

    def factor(self, s):
        """warm(s) * decay(u) in Python floats: the definition (the only place the formula lives on the host)."""
        s = max(int(s), 0)
        Wm, f0, T, r = self.warmup_steps, self.warmup_start, self.total_steps, self.min_ratio
        warm = f0 + (1.0 - f0) * min(s, Wm) / Wm if Wm > 0 else 1.0
        u = max(s - Wm, 0)
        if self.decay != "step" and T is not None:
            u = min(u, T)
        if self.decay == "cosine":
            dec = r + (1.0 - r) * (1.0 + math.cos(math.pi * u / T)) / 2.0
        elif self.decay == "linear":
            dec = 1.0 - (1.0 - r) * u / T
        elif self.decay == "step":
            dec = self.gamma ** (u // self.step_size)
        else:
            dec = 1.0
        return warm * dec

    def kernel_args(self):
        """(kind, warmup_steps, warmup_start, total_steps, min_ratio, step_size, gamma) as ops.adamw_sched_ takes them."""
        return (self.KINDS.index(self.decay), self.warmup_steps, self.warmup_start, self.total_steps or 1, self.min_ratio,
                self.step_size or 1, self.gamma)

    def to_dict(self):
        return dict(warmup_steps=self.warmup_steps, warmup_start=self.warmup_start, decay=self.decay,
                    total_steps=self.total_steps, min_ratio=self.min_ratio, step_size=self.step_size, gamma=self.gamma)

    @classmethod
    def from_dict(cls, d):
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "LRSchedule(" + ", ".join(f"{k}={v!r}" for k, v in self.to_dict().items()) + ")"


def _as_schedule_dict(lr_schedule):
    """None, an LRSchedule or a dict of its arguments -> None or the validated plain dict kept in param_groups[0]."""
    if lr_schedule is None:
        return None
    if isinstance(lr_schedule, LRSchedule):
        return lr_schedule.to_dict()
    if isinstance(lr_schedule, dict):
        try:
            return LRSchedule(**lr_schedule).to_dict()
        except TypeError as e:
            raise ValueError(f"lr_schedule: {e}") from None
    raise ValueError(f"lr_schedule must be None, an LRSchedule or a dict of its arguments, got {lr_schedule!r}")


def _check_option(lr_scale, weight_decay, who=""):
    ok = lambda x: not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and x >= 0.0
    if not ok(lr_scale):
        raise ValueError(f"param_options{who}: lr_scale must be a finite number >= 0, got {lr_scale!r}")
    if weight_decay is not None and not ok(weight_decay):
        raise ValueError(f"param_options{who}: weight_decay must be None or a finite number >= 0, got {weight_decay!r}")
    return (float(lr_scale), None if weight_decay is None else float(weight_decay))


def resolve_param_options(param_options, named_params):
    """param_options -> None or the list of (lr_scale, weight_decay) pairs, aligned with `named_params` ([(name, param)]),
    that param_groups[0] keeps; weight_decay None: the group's.  "no_decay_1d": weight decay 0 for every parameter with
    ndim <= 1 (biases, norm scales, PReLU slopes, the learned prompts); a callable (name, param) -> dict(lr_scale=1.0,
    weight_decay=None) (or None for the defaults); a ready list of pairs is checked and passed through."""
    named_params = list(named_params)
    if param_options is None:
        return None
    if isinstance(param_options, str):
        if param_options != "no_decay_1d":
            raise ValueError(f'param_options: the one preset is "no_decay_1d", got {param_options!r}')
        return [(1.0, 0.0 if p.ndim <= 1 else None) for _, p in named_params]
    if callable(param_options):
        out = []
        for name, p in named_params:
            d = param_options(name, p) or {}
            if not isinstance(d, dict) or set(d) - {"lr_scale", "weight_decay"}:
                raise ValueError(f"param_options({name!r}) must return a dict with lr_scale / weight_decay, got {d!r}")
            out.append(_check_option(d.get("lr_scale", 1.0), d.get("weight_decay"), f"({name!r})"))
        return out
    if isinstance(param_options, (list, tuple)):
        if len(param_options) != len(named_params) or any(not isinstance(o, (list, tuple)) or len(o) != 2 for o in param_options):
            raise ValueError(f"param_options: a list needs one (lr_scale, weight_decay) pair per parameter "
                             f"({len(named_params)}), got {len(param_options)} entries")
        return [_check_option(a, b, f"[{i}]") for i, (a, b) in enumerate(param_options)]
    raise ValueError(f'param_options must be None, "no_decay_1d", a callable or a list of pairs, got {param_options!r}')


def build_segments(numels, options, weight_decay, total=None, cap=ops.MAX_SEGS):
    """The segment table of coma_adamw_sched for tensors of `numels` elements laid out back to back, with `options`
    [(lr_scale, weight_decay or None)] beside them: -> (seg_end, seg_lr_scale, seg_wd) as lists, seg_end strictly ascending.
    Neighbours with equal options are one segment, empty tensors none; the last segment reaches `total` (the flat buffer's
    padding belongs to it).  ValueError above `cap` segments (the kernel's)."""
    ends, scales, wds = [], [], []
    pos = 0
    for k, (scale, wd) in zip(numels, options):
        if k == 0:
            continue
        pos += int(k)
        opt = (float(scale), float(weight_decay if wd is None else wd))
        if ends and (scales[-1], wds[-1]) == opt:
            ends[-1] = pos
        else:
            ends.append(pos); scales.append(opt[0]); wds.append(opt[1])
    if ends and total is not None:
        assert total >= pos
        ends[-1] = int(total)
    if len(ends) > cap:
        raise ValueError(f"param_options: {len(ends)} segments of the flat buffer differ from their neighbours, the kernel "
                         f"takes at most {cap}: give neighbouring parameters equal options")
    return ends, scales, wds


def check_no_exchange(optimizer, reducer):
    """ValueError when a gradient exchange meets an optimizer that accumulates or clips."""
    if reducer is not None and getattr(optimizer, "windowed", False):
        raise ValueError(NO_EXCHANGE)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, dynamic=(), write_through=False,
                 pad_to=1, grad_acc_batch=1, max_grad_norm=None, ema_decay=None, ema_warmup=False, lr_schedule=None,
                 param_options=None, param_names=None):
        """grad_acc_batch=K > 1: ``step()`` means "this micro-batch's backward is done" -- it adds the flat gradient to a flat
        fp32 accumulator and the K-th call (or ``flush()``) applies ONE update with the MEAN of the window's gradients.
        max_grad_norm: clip that mean gradient to this global 2-norm first (``torch.nn.utils.clip_grad_norm_``; the
        unclipped norm is left in ``last_grad_norm``, a device float).  Both live in ``param_groups[0]``.
        ema_decay=d: every applied update also moves an exponential moving average of the weights, e += (1 - d_t)(p - e),
        inside the update's own kernel (``ops.adamw_ema_``); d_t = d, or min(d, (1 + t) / (10 + t)) with ema_warmup (t: the
        update count).  The average starts at the parameters' values when the option is switched on.  ``swap_ema()`` /
        ``ema_weights()`` put it under the model, ``ema_state_dict`` / ``load_ema_state_dict`` serialise it.  Both options
        live in ``param_groups[0]`` too.
        lr_schedule (None, an LRSchedule or a dict of its arguments) / param_options (None, "no_decay_1d", a callable
        (name, param) -> dict(lr_scale=1.0, weight_decay=None), or a list of such pairs; param_names: the names the callable
        sees, default the parameters' positions): either one switches the update to coma_adamw_sched, which forms
        lr_t = lr * warm * decay on the device from the update count and takes lr_t * lr_scale and weight_decay per
        parameter.  ``param_groups[0]`` keeps them as plain data -- the schedule's dict, a list of (lr_scale, weight_decay)
        aligned with ``params`` -- so ``state_dict()`` carries them; ``param_groups[0]["lr"]`` stays the BASE rate, the one a
        plateau scheduler acts on (``sync_lr()``), ``last_lr`` is the device float the kernel wrote and ``current_lr()`` the
        host's value for logging."""
        _check_window_opts(grad_acc_batch, max_grad_norm)
        _check_ema_opts(ema_decay, ema_warmup)
        params = list(params)
        assert not params or not isinstance(params[0], dict), "one parameter group (the reference uses one)"
        names = list(param_names) if param_names is not None else [str(i) for i in range(len(params))]
        if len(names) != len(params):
            raise ValueError(f"param_names: {len(names)} names for {len(params)} parameters")
        lr_schedule = _as_schedule_dict(lr_schedule)
        param_options = resolve_param_options(param_options, zip(names, params))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_acc_batch=int(grad_acc_batch),
                        max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                        ema_decay=None if ema_decay is None else float(ema_decay), ema_warmup=bool(ema_warmup))
        if lr_schedule is not None or param_options is not None:      # (without the options the group has the keys it had)
            defaults.update(lr_schedule=lr_schedule, param_options=param_options)
        super().__init__(params, defaults)
        assert len(self.param_groups) == 1, "one parameter group (the reference uses one)"
        self._dynamic = {id(p) for p in dynamic}   # may or may not get a gradient, step to step
        self.flat_p = self.flat_g = self.flat_m = self.flat_v = None
        self._flat_params = []
        self._flat_step = 0
        # write_through: backward kernels store parameter gradients straight into the flat buffer's slots
        # (ops.GradSink) -- no per-parameter AccumulateGrad launch.  Off when a GradReducer drives its
        # all-reduce from post-accumulate-grad hooks (those do not fire for sunk gradients).
        self.write_through = write_through
        self.pad_to = max(1, int(pad_to))   # flat buffers padded to a multiple of this (the world size, for sharded steps)
        # set by data_parallel.StreamedGradExchange(sharded=True): each rank then steps only its own sub-slices of the moment
        # buffers, and state_dict() must re-assemble them first (a COLLECTIVE: every rank calls state_dict())
        self.shard_exchange = None
        # sparse zero_grad (write-through only): the backward kernels overwrite ("=") the gradient slots of the large
        # tensors every step, so zero_grad() only has to clear what lies between them -- one small launch instead of a
        # memset of the whole buffer (647 MB, ~90 us).  Built from what the previous step's kernels actually wrote and
        # checked again at every step (a tensor that was NOT written after all is zeroed before the update reads it).
        self._zero_tab = None          # (device int64 [n, 2] table, n, longest range)
        self._zero_big = ()            # ids of the parameters zero_grad() skips
        self.sparse_zero = True
        # accumulation window / clipping (allocated on first use; none of it exists on the default path)
        self.flat_acc = None           # fp32 accumulator with flat_g's layout (grad_acc_batch > 1)
        self._acc_dev = None           # device int32: micro-batches in the open window (a captured step keeps counting under replay)
        self._pending = 0              # its host copy
        self._partials = None          # device fp64 [ops.ACC_PARTIALS]: per-block sums of squares of the gradient to clip
        self._extra_dev = None         # device fp64: squared norm of the gradients outside the flat buffer
        self._norm_dev = None          # device fp32: what coma_adamw_ex wrote (the unclipped norm of the mean gradient)
        self._loose_acc = {}           # parameter outside the flat buffer -> its fp32 accumulator (all zeros between windows)
        self._loose_live = set()       # ids of those that received a gradient in the open window
        self.last_grad_norm = None
        # weight EMA (ema_decay; allocated by _ensure_ema, none of it exists on the default path)
        self.flat_ema = None           # the average of flat_p, same layout
        self._loose_ema = {}           # parameter outside the flat buffer -> its average (flat fp32), from its first step on
        self._ema_parked = {}          # parameter -> average loaded before the flat layout existed (load_ema_state_dict)
        self._ema_in = False           # swap_ema(): the parameters hold the average, flat_ema / _loose_ema the iterate
        # learning-rate schedule / parameter options (allocated by _ensure_sched; none of it exists on the default path)
        self._lr_dev = None            # device fp32: the base rate the kernel reads
        self._lr_host = None           # its host shadow (sync_lr)
        self.last_lr = None            # device fp32: the rate coma_adamw_sched formed for the last update (before any lr_scale)
        self._seg_tab = None           # (seg_end int64, seg_lr_scale fp32, seg_wd fp32) on the device, or None: uniform
        self._seg_key = None           # what the table was built from: (copy of the options list, weight decay)
        self._index = None             # id(parameter) -> position in the group (_param_index)

    # -- layout -------------------------------------------------------------------------
    def _build(self):
        ps = [p for p in self.param_groups[0]["params"] if p.grad is not None and id(p) not in self._dynamic]
        assert ps, "no parameter has a gradient"
        dev = ps[0].device
        n = sum(p.numel() for p in ps)
        n = (n + self.pad_to - 1) // self.pad_to * self.pad_to
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        self._offsets = {}
        for p in ps:
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.data.reshape(-1))
            self.flat_g[off:off + k].copy_(p.grad.reshape(-1))
            p.data = self.flat_p[off:off + k].view(p.shape)
            p.grad = self.flat_g[off:off + k].view(p.shape)
            self._offsets[id(p)] = (off, k)
            p._coma_sink = bool(self.write_through)
            off += k
        self._flat_params = ps
        self._flat_ids = {id(p) for p in ps}
        # a state_dict loaded BEFORE the layout existed (the reference's resume order: fresh optimizer ->
        # load_state_dict -> train, validation.py:276-281, attn_unet_data_parallel.py:729-733) parked its moments in
        # self.state[p]: move them into the flat buffers and carry the step count over
        for p in ps:
            st = self.state.pop(p, None)
            if st:
                off, k = self._offsets[id(p)]
                self.flat_m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.flat_v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                self._flat_step = max(self._flat_step, int(st["step"]))
        self._step_dev = torch.full((1,), self._flat_step, dtype=torch.int32, device=dev)
        self._ensure_ema()
        self._ensure_sched()

    @property
    def built(self):
        return self.flat_p is not None

    def set_write_through(self, on: bool):
        self.write_through = bool(on)
        for p in self._flat_params:
            p._coma_sink = self.write_through

    def zero_grad(self, set_to_none=True):
        ops.GradSink.begin_step()
        for p in self.param_groups[0]["params"]:
            if self.built and id(p) in self._flat_ids:
                continue
            p.grad = None
        if self.built:
            if self._zero_tab is not None and self.write_through and self.sparse_zero:
                tab, n, longest = self._zero_tab
                from ._lib import lib, check, stream
                check(lib.coma_zero_ranges(self.flat_g.data_ptr(), tab.data_ptr(), n, longest, stream()), "coma_zero_ranges")
            else:
                self.flat_g.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        self.step_shards(None)

    @torch.no_grad()
    def step_shards(self, shards, advance=True, loose=True):
        """One AdamW step.  shards=None: the whole flat buffer (one launch).  shards=[(offset, length)]: only those slices
        of it -- the data-parallel step with a reduce-scattered gradient updates this rank's slices and all-gathers the
        parameters afterwards (data_parallel.StreamedGradExchange); the moments of the other slices are never touched here
        (they live, up to date, on the ranks that own them).  A step may also be taken slice by slice as the slices'
        gradients arrive (GradReducer.reduce_flat_and_step): advance=True on the first call only (the step count moves
        once), loose=True on one call only (parameters outside the flat buffer)."""
        averaging = self.averaging
        if averaging and self.shard_exchange is not None:
            raise ValueError(NO_EMA_SHARDED)
        if self._ema_in:
            raise RuntimeError(EMA_IN.format("step()"))
        if self.windowed:         # grad_acc_batch > 1 or max_grad_norm: the step goes through the window
            if shards is not None or not (advance and loose) or self.shard_exchange is not None:
                raise ValueError(NO_EXCHANGE)
            ops.SidePrep.join()
            return self._micro_step()
        ops.SidePrep.join()       # the side stream's expert-gradient scatters land in the flat gradient buffer
        if not self.built:
            self._build()
        self._ensure_ema()
        self._ensure_sched()
        if advance:
            self._flat_step += 1
            self._step_dev += 1            # device-side copy: a captured step keeps counting under graph replay
            self._sparse_zero_bookkeeping()
        for off, k in ([(0, self.flat_p.numel())] if shards is None else shards):
            if k > 0:                      # (elementwise: the average moves slice by slice with the parameters)
                sl = slice(off, off + k)
                self._update(self.flat_p[sl], self.flat_g[sl], self.flat_m[sl], self.flat_v[sl],
                             self.flat_ema[sl] if averaging else None, self._flat_step, self._step_dev, flat_off=off)
        if not loose:
            return
        # backward is over: every slice of the step's zeroed arena is dead -- ONE memset clears them.  Behind the AdamW launch,
        # not in front of it: with ~170 MB of freshly dirtied lines ahead of it the 2.7 GB AdamW sweep measured 1.10 ms
        # instead of 0.85 ms.
        ops.ZeroArena.end_step()
        for p in self.param_groups[0]["params"]:
            if id(p) in self._flat_ids or p.grad is None:
                continue
            st = self._loose_state(p)
            self._update(p.data.view(-1), p.grad.float().contiguous().view(-1), st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1),
                         self._loose_average(p) if averaging else None, st["step"], loose=p)

    def _update(self, p, g, m, v, average, step, step_dev=None, window=None, flat_off=None, loose=None):
        """One update of the flat fp32 (p, g, m, v) and, where there is one, of `average`, at update count `step` / the device
        int32 `step_dev`.  window: ops.adamw_ex_'s (count_dev, partials, n_partials, extra_sumsq, max_norm, norm_out), or None
        outside an accumulation window.  flat_off: (p, g, m, v) are the flat buffers from this element on; loose: they are
        those of this parameter outside the flat buffer (only the scheduled path looks at either).  The one place that picks
        the kernel; the default step stays on coma_adamw."""
        grp = self.param_groups[0]
        if self.scheduled:
            # all three variants in one entry point.  A slice of the flat buffer reads the segment table at its own offset;
            # a loose parameter has its own options and bias-correction count, and the schedule's count is the global one
            b1, b2 = grp["betas"]
            scale, wd, segs = 1.0, grp["weight_decay"], None
            if loose is not None:
                scale, wd = self._option_of(loose)
            elif self._seg_tab is not None:
                segs = self._seg_tab
            d, w = self._ema_opts() if average is not None else (0.0, False)
            ops.adamw_sched_(p, g, m, v, self._lr_dev, self._schedule().kernel_args(), b1, b2, grp["eps"], wd, step, step_dev,
                             self._flat_step, self._step_dev, scale, segs, flat_off or 0,
                             self.last_lr if loose is None else None, average, d, w, *(window or ()))
            return
        hp = (float(grp["lr"]), *grp["betas"], grp["eps"], grp["weight_decay"])
        if average is not None:
            ops.adamw_ema_(p, g, m, v, average, *self._ema_opts(), *hp, step, step_dev, *(window or ()))
        elif window is not None:
            ops.adamw_ex_(p, g, m, v, *hp, step, step_dev, *window)
        else:
            ops.adamw_(p, g, m, v, *hp, step, step_dev)

    def _loose_state(self, p):
        """The moments of a parameter outside the flat buffer, created at its first update, with the count of this one."""
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
        st["step"] += 1
        return st

    # -- accumulation window and clipping ----------------------------------------------
    def _window_opts(self):
        g = self.param_groups[0]
        K, mx = g.get("grad_acc_batch", 1), g.get("max_grad_norm")
        _check_window_opts(K, mx)
        return int(K), (None if mx is None else float(mx))

    @property
    def windowed(self):
        """Either new option is on: step() goes through coma_grad_accum / coma_adamw_ex instead of coma_adamw."""
        K, mx = self._window_opts()
        return K > 1 or mx is not None

    @property
    def pending(self):
        """Micro-batches in the open window (0: the last step() or flush() applied an update)."""
        return self._pending

    def _ensure_window_buffers(self):
        """The window's device state, allocated outside any graph capture (a counter created under capture would be
        re-created, not advanced, by every replay)."""
        K, mx = self._window_opts()
        dev = self.flat_g.device
        if K > 1 and self.flat_acc is None:
            self.flat_acc = torch.zeros_like(self.flat_g)
        if self._acc_dev is None:
            self._acc_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        if mx is not None and self._partials is None:
            self._partials = torch.zeros(ops.ACC_PARTIALS, dtype=torch.float64, device=dev)
            self._extra_dev = torch.zeros(1, dtype=torch.float64, device=dev)
            self._norm_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def _micro_step(self):
        """This micro-batch's backward is done: into the window; the grad_acc_batch-th one applies the update."""
        K, mx = self._window_opts()
        if not self.built:
            self._build()
        self._ensure_window_buffers()
        self._ensure_ema()
        self._ensure_sched()
        self._sparse_zero_bookkeeping()
        apply = self._pending + 1 >= K
        nb = None
        if K > 1:
            # flat_g keeps this micro-batch's own gradient; the partials of the K-th launch are those of the finished sum
            nb = ops.grad_accum_(self.flat_acc, self.flat_g, self._acc_dev, self._partials if (apply and mx is not None) else None)
            self._acc_dev += 1
            for p in self.param_groups[0]["params"]:
                if id(p) in self._flat_ids or p.grad is None:
                    continue
                acc = self._loose_acc.get(p)
                if acc is None:
                    acc = self._loose_acc[p] = torch.zeros_like(p, dtype=torch.float32).view(-1)
                acc.add_(p.grad.float().reshape(-1))        # (0 + g is exact: the window's first gradient is assigned)
                self._loose_live.add(id(p))
        self._pending += 1
        if apply:
            self._apply(K, mx, nb)
        else:
            ops.ZeroArena.end_step()

    def flush(self):
        """Apply an open window of fewer than grad_acc_batch micro-batches (the mean over those it holds).  No-op when
        nothing is pending."""
        if self._pending == 0:
            return
        if self._ema_in:
            raise RuntimeError(EMA_IN.format("flush()"))
        K, mx = self._window_opts()
        self._ensure_ema()
        self._ensure_sched()
        with torch.no_grad():
            self._apply(K, mx, None)

    def _apply(self, K, mx, nb):
        g = self.param_groups[0]
        acc_mode = K > 1
        src = self.flat_acc if acc_mode else self.flat_g
        count_dev = self._acc_dev if acc_mode else None
        if acc_mode:
            loose_src = [(p, self._loose_acc[p]) for p in g["params"] if id(p) in self._loose_live]
        else:
            loose_src = [(p, p.grad.float().contiguous().view(-1)) for p in g["params"]
                         if id(p) not in self._flat_ids and p.grad is not None]
        partials, n_part, extra, norm_out = None, 0, None, None
        if mx is not None:
            if nb is None:                 # flush(), or no accumulation: a norm-only pass over the gradient source
                nb = ops.grad_accum_(None, src, None, self._partials)
            partials, n_part, norm_out = self._partials, nb, self._norm_dev
            if loose_src:
                self._extra_dev.copy_(torch.stack([a.double().pow(2).sum() for _, a in loose_src]).sum().view(1))
                extra = self._extra_dev
        self._flat_step += 1
        self._step_dev += 1                # once per applied update (torch's step count under the usual accumulation idiom)
        averaging = self.averaging         # the average moves here, on the applying update, never on a micro-batch
        window = (count_dev, partials, n_part, extra, mx or 0.0)
        self._update(self.flat_p, src, self.flat_m, self.flat_v, self.flat_ema if averaging else None, self._flat_step,
                     self._step_dev, window + (norm_out,), flat_off=0)
        ops.ZeroArena.end_step()           # (behind the sweep, as in step_shards)
        for p, a in loose_src:
            st = self._loose_state(p)
            self._update(p.data.view(-1), a, st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1),
                         self._loose_average(p) if averaging else None, st["step"], None, window + (None,), loose=p)
        if acc_mode:
            self._acc_dev.zero_()
            for _, a in loose_src:
                a.zero_()
            self._loose_live.clear()
        self._pending = 0
        self.last_grad_norm = norm_out

    # -- learning-rate schedule and parameter options ---------------------------------------
    @property
    def scheduled(self):
        """lr_schedule or param_options is set: every update goes through coma_adamw_sched."""
        g = self.param_groups[0]
        return g.get("lr_schedule") is not None or g.get("param_options") is not None

    def _schedule(self):
        d = self.param_groups[0].get("lr_schedule")
        return LRSchedule() if d is None else LRSchedule.from_dict(d)

    def _option_of(self, p):
        """(lr_scale, weight_decay) of one parameter of the group."""
        g = self.param_groups[0]
        opts = g.get("param_options")
        if opts is None:
            return 1.0, g["weight_decay"]
        scale, wd = opts[self._param_index()[id(p)]]
        return float(scale), float(g["weight_decay"] if wd is None else wd)

    def _param_index(self):
        """id(parameter) -> its position in the group (the group's parameter list never changes)."""
        if self._index is None:
            self._index = {id(p): i for i, p in enumerate(self.param_groups[0]["params"])}
        return self._index

    def _ensure_sched(self):
        """The device state of the scheduled path -- base rate, last_lr, segment table -- allocated outside any graph capture
        (GraphedTrainStep._capture calls this first), and the base rate brought up to date (sync_lr)."""
        if not self.built or not self.scheduled:
            return
        g = self.param_groups[0]
        dev = self.flat_p.device
        if self._lr_dev is None:
            self._lr_host = float(g["lr"])
            self._lr_dev = torch.full((1,), self._lr_host, dtype=torch.float32, device=dev)
            self.last_lr = torch.zeros(1, dtype=torch.float32, device=dev)
        opts = g.get("param_options")
        # (compared by value against a copy: the list may be edited in place; no tuple is built while nothing changed)
        same = (opts is None and self._seg_key is None) or \
            (opts is not None and self._seg_key is not None and self._seg_key[1] == g["weight_decay"] and self._seg_key[0] == opts)
        if not same:
            if opts is not None:
                opts[:] = [tuple(o) for o in opts]          # (pairs that came as lists would never compare equal to the copy)
            self._seg_key = None if opts is None else (list(opts), float(g["weight_decay"]))
            self._seg_tab = None
            if opts is not None:
                if len(opts) != len(g["params"]):
                    raise ValueError(f"param_options: {len(opts)} entries for {len(g['params'])} parameters")
                index = self._param_index()
                ends, scales, wds = build_segments([p.numel() for p in self._flat_params],
                                                   [opts[index[id(p)]] for p in self._flat_params], g["weight_decay"],
                                                   total=self.flat_p.numel())
                self._seg_tab = (torch.tensor(ends, dtype=torch.int64, device=dev),
                                 torch.tensor(scales, dtype=torch.float32, device=dev),
                                 torch.tensor(wds, dtype=torch.float32, device=dev))
        self.sync_lr()

    def sync_lr(self):
        """param_groups[0]["lr"] -> the device float the kernel reads, when it differs from what is there (a plateau
        scheduler moved it).  Never inside a capture: step() calls it when not capturing, GraphedTrainStep before a replay."""
        if self._lr_dev is None or torch.cuda.is_current_stream_capturing():
            return
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_host:
            self._lr_dev.fill_(lr)
            self._lr_host = lr

    def current_lr(self):
        """The host's value of the rate of the NEXT update, lr * factor(applied updates): for logging, no device read."""
        count = self._flat_step
        if not self.built:                # (a loaded state waits in self.state until the layout exists: _build takes its count)
            count = max([count] + [int(st["step"]) for st in self.state.values() if st])
        return float(self.param_groups[0]["lr"]) * self._schedule().factor(count)

    # -- weight EMA ------------------------------------------------------------------------
    def _ema_opts(self):
        g = self.param_groups[0]
        d, w = g.get("ema_decay"), g.get("ema_warmup", False)
        _check_ema_opts(d, w)
        return (None if d is None else float(d)), bool(w)

    @property
    def averaging(self):
        """ema_decay is set: every applied update goes through coma_adamw_ema."""
        return self._ema_opts()[0] is not None

    def _ensure_ema(self):
        """The average of the flat buffer, allocated and started at the parameters' values (e_0 = p_0) outside any graph
        capture: when the layout is built, or at the first step after the option was switched on.  Averages that
        load_ema_state_dict parked before the layout existed move in here."""
        if not self.built or not self.averaging:
            return
        if self.flat_ema is None:
            self.flat_ema = self.flat_p.clone()
        for p, t in list(self._ema_parked.items()):
            t = t.to(self.flat_p.device).float().reshape(-1)
            if id(p) in self._flat_ids:
                off, k = self._offsets[id(p)]
                self.flat_ema[off:off + k].copy_(t)
            elif id(p) in self._dynamic:          # (a parameter that never receives a gradient has no average)
                self._loose_ema[p] = t.clone()
        self._ema_parked.clear()

    def _loose_average(self, p):
        """The average of a parameter outside the flat buffer: starts at its value when it is first stepped."""
        e = self._loose_ema.get(p)
        if e is None:
            e = self._loose_ema[p] = p.data.detach().float().reshape(-1).clone()
        return e

    def reset_ema(self):
        """Restart the average from the parameters' current values."""
        if self._ema_in:
            raise RuntimeError(EMA_IN.format("reset_ema()"))
        self._ema_parked.clear()
        self._loose_ema.clear()
        if self.flat_ema is not None:
            self.flat_ema.copy_(self.flat_p)

    @torch.no_grad()
    def swap_ema(self):
        """Exchange parameters and average BY CONTENT (coma_swap_f32 on the flat buffers and on every parameter outside them
        that has an average): `p.data`, the flat views and the addresses a captured graph holds all stay where they are.
        Call it again to swap back.  While the average is in, step(), flush() and state_dict() raise RuntimeError."""
        if not self.averaging:
            raise RuntimeError("swap_ema(): this optimizer keeps no average (ema_decay is None)")
        if self._pending:
            raise RuntimeError(f"swap_ema(): {self._pending} micro-batch(es) of an open accumulation window -- call flush() first")
        self._ensure_ema()
        if self.flat_ema is not None:         # (before the first step the average IS the parameters: nothing to move)
            ops.swap_f32_(self.flat_p, self.flat_ema)
        for p, e in self._loose_ema.items():
            ops.swap_f32_(p.data.view(-1), e)
        self._ema_in = not self._ema_in

    def ema_weights(self):
        """``with optimizer.ema_weights():`` -- the model computes with the averaged weights inside, with the iterate again
        after it (also when the body raises)."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.swap_ema()
            try:
                yield self
            finally:
                self.swap_ema()
        return scope()

    def _average_of(self, p):
        """The average of parameter p as a tensor of its shape, or None where there is none."""
        if self.built and id(p) in self._flat_ids and self.flat_ema is not None:
            off, k = self._offsets[id(p)]
            return (self.flat_p if self._ema_in else self.flat_ema)[off:off + k].view(p.shape)
        if p in self._loose_ema:
            return (p.data if self._ema_in else self._loose_ema[p]).view(p.shape)
        if p in self._ema_parked:
            return self._ema_parked[p].view(p.shape)
        return None

    @torch.no_grad()
    def ema_state_dict(self, model):
        """``model.state_dict()`` with the averaged values where an average exists; everything else -- parameters that never
        received a gradient and all buffers, BatchNorm running statistics included -- as it is now
        (``AveragedModel(use_buffers=False)``).  Loads into a model with ``load_state_dict``."""
        if not self.averaging:
            raise RuntimeError("ema_state_dict(): this optimizer keeps no average (ema_decay is None)")
        self._ensure_ema()
        sd = model.state_dict()
        for name, p in model.named_parameters():
            avg = self._average_of(p)
            if name in sd and avg is not None:
                sd[name] = avg.detach().to(sd[name].dtype).clone()
        return sd

    @torch.no_grad()
    def load_ema_state_dict(self, model, sd):
        """Restore the averages from an ``ema_state_dict``.  Before the flat layout exists they wait, like the moments of
        load_state_dict, and _build() moves them in."""
        if self._ema_in:
            raise RuntimeError(EMA_IN.format("load_ema_state_dict()"))
        for name, p in model.named_parameters():
            if name in sd:
                self._ema_parked[p] = sd[name].detach().to(p.device).float().clone()
        self._ensure_ema()

    def _sparse_zero_bookkeeping(self):
        """After a backward: (1) any large tensor zero_grad() skipped that the kernels did NOT overwrite this step still
        holds last step's gradient -- clear it now, before the update reads it, and go back to full clears; (2) otherwise
        (re)build the table of what zero_grad() has to clear from what this step's kernels wrote."""
        if not (self.write_through and self.sparse_zero):
            self._zero_tab, self._zero_big = None, ()
            return
        written = ops.GradSink.written
        if self._zero_tab is not None:
            missing = [p for p in self._flat_params if id(p) in self._zero_big and id(p) not in written]
            if missing:
                for p in missing:
                    p.grad.zero_()
                self._zero_tab, self._zero_big, self.sparse_zero = None, (), False
            return
        big = [p for p in self._flat_params if id(p) in written and p.numel() >= (1 << 16)]
        if not big:
            return
        ranges, pos = [], 0
        for p in big:                                   # (flat order == _flat_params order)
            off, k = self._offsets[id(p)]
            if off > pos:
                ranges.append((pos, off - pos))
            pos = off + k
        n = self.flat_g.numel()
        if n > pos:
            ranges.append((pos, n - pos))
        if sum(r[1] for r in ranges) * 4 > n:           # not worth a table: most of the buffer needs clearing anyway
            return
        tab = torch.tensor(ranges if ranges else [(0, 0)], dtype=torch.int64, device=self.flat_g.device)
        self._zero_tab = (tab, len(ranges), max([r[1] for r in ranges], default=0))
        self._zero_big = {id(p) for p in big}

    # -- torch.optim.AdamW-compatible checkpoint format (attn_unet_data_parallel.py:946-952) ----
    def state_dict(self):
        """torch.optim.AdamW's format.  Under a sharded exchange the moments of this rank's sub-slices are current and the
        others stopped at the last unsharded step: they are all-gathered first (every rank must call state_dict(), like any
        collective; afterwards every rank holds the full, identical state)."""
        if self._ema_in:
            raise RuntimeError(EMA_IN.format("state_dict()"))
        if self._pending:
            raise RuntimeError(f"FusedAdamW.state_dict(): {self._pending} micro-batch(es) of an open accumulation window are "
                               "not applied yet -- call flush() first")
        if self.shard_exchange is not None and self.built:
            self.shard_exchange.gather_state()
        params = self.param_groups[0]["params"]
        state = {}
        for i, p in enumerate(params):
            if self.built and id(p) in self._flat_ids:
                off, k = self._offsets[id(p)]
                state[i] = {"step": torch.tensor(float(self._flat_step)),
                            "exp_avg": self.flat_m[off:off + k].view(p.shape).clone(),
                            "exp_avg_sq": self.flat_v[off:off + k].view(p.shape).clone()}
            elif p in self.state and self.state[p]:
                st = self.state[p]
                state[i] = {"step": torch.tensor(float(st["step"])), "exp_avg": st["exp_avg"].clone(),
                            "exp_avg_sq": st["exp_avg_sq"].clone()}
        pg = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        pg["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [pg]}

    def load_state_dict(self, sd):
        params = self.param_groups[0]["params"]
        # (a file written without an average does not switch off the one this optimizer was built with)
        skip = ("params", "ema_decay", "ema_warmup") if sd["param_groups"][0].get("ema_decay") is None else ("params",)
        # (nor does one written without a schedule or without parameter options switch off what this one has)
        skip += tuple(k for k in ("lr_schedule", "param_options") if sd["param_groups"][0].get(k) is None)
        for k, v in sd["param_groups"][0].items():
            if k not in skip:
                self.param_groups[0][k] = v
        # the flat layout exists only after the first backward: until then the moments wait in self.state[p]
        # (per-parameter AdamW entries) and _build() moves them into the flat buffers
        for i, st in sd["state"].items():
            p = params[int(i)]
            if self.built and id(p) in self._flat_ids:
                off, k = self._offsets[id(p)]
                self.flat_m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.flat_v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                self._flat_step = int(st["step"])
                self._step_dev.fill_(self._flat_step)
            else:
                self.state[p] = {"step": int(st["step"]), "exp_avg": st["exp_avg"].to(p.device).float().clone(),
                                 "exp_avg_sq": st["exp_avg_sq"].to(p.device).float().clone()}
        if self.built:      # parameters inside the flat buffer share one step count
            self._step_dev.fill_(self._flat_step)
        g = self.param_groups[0]
        if g.get("lr_schedule") is not None:
            g["lr_schedule"] = _as_schedule_dict(g["lr_schedule"])
        if g.get("param_options") is not None:
            g["param_options"] = resolve_param_options([tuple(o) for o in g["param_options"]], [(str(i), p) for i, p in enumerate(params)])
