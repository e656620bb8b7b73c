"""End-to-end parity of the HIP model + losses + train step against the CPU oracle
(BASELINE configs C1 32^3 and a C2-shaped 64^3 run) and against the committed golden fixture.

Tolerances: forward/loss vs the fp32 oracle <= 1e-3 rel-L2 (north_star's bound; measured ~1e-5).
Gradients are compared with the fp64 oracle: through ~45 conv+norm layers at batch 2 the
backward pass is ill-conditioned in fp32 -- the fp32 CPU oracle itself is 2e-3..5e-2 away from
its own fp64 run (worst at the 4^3 bottom levels) -- so the bound per tensor is
max(2e-2, 4 x the fp32 CPU oracle's own error) on every gradient that is not rounding noise.
"""
import copy
import os

import numpy as np
import pytest
import torch

import _step_state as ss      # the per-tensor comparison of the step-state tests

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    n = b.norm()
    return float((a - b).norm() / n) if n > 0 else float((a - b).norm())


def _pair(shape, seed, dtype=torch.float32, **kw):
    import coma_unet_amd as cu
    from oracle.coma_oracle import build_reference_model
    torch.manual_seed(seed)
    om = build_reference_model(volume_shape=shape)
    om.set_save_attn(None)
    om.train(True)
    gm = cu.build_model(volume_shape=shape, compute_dtype=dtype, **kw).cuda()
    gm.load_state_dict(om.state_dict(), strict=True)
    gm.set_save_attn(None)
    gm.train(True)
    return om, gm


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def test_state_dict_keys_match_oracle():
    om, gm = _pair((32, 32, 32), 0)
    assert list(om.state_dict().keys()) == list(gm.state_dict().keys())
    assert [n for n, _ in om.named_parameters()] == [n for n, _ in gm.named_parameters()]


@pytest.mark.parametrize("B", [1, 2])
def test_c1_forward_loss_backward_vs_oracle_and_golden(B):
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    S = (32, 32, 32)
    om, gm = _pair(S, 100 + B)          # same seeds as oracle/make_golden.py
    b = make_batch(B, S, seed=7 + B)
    gold = np.load(os.path.join(GOLD, "model32_oracle.npz"))
    # GPU
    losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(b))
    losses[0].backward()
    assert rel(outs[0], torch.from_numpy(gold[f"b{B}_out"])) < 1e-3
    assert rel(outs[1][-1], torch.from_numpy(gold[f"b{B}_proj4"])) < 1e-3
    assert abs(float(losses[0]) - float(gold[f"b{B}_total"])) / float(gold[f"b{B}_total"]) < 1e-4
    assert rel(losses[1], torch.from_numpy(gold[f"b{B}_gen"])) < 1e-4
    n_none = sum(p.grad is None for p in gm.parameters())
    assert n_none == int(gold[f"b{B}_n_grad_none"])
    # fp64 oracle for the gradients
    o64 = copy.deepcopy(om).double()
    res = o64(b["mri"].double(), b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"].double())
    tot = train_step_loss(res, b["tau"].double(), b["roi"].double(), b["covars"], build_reference_criterion())[0]
    tot.backward()
    assert rel(outs[0], res[0]) < 1e-4
    # the fp32 CPU oracle's own distance from fp64 is the yardstick for "as accurate as the reference"
    r32 = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
    train_step_loss(r32, b["tau"], b["roi"], b["covars"], build_reference_criterion())[0].backward()
    o32g = dict(om.named_parameters())
    og = dict(o64.named_parameters())
    worst = worst_cpu = 0.0
    for n, p in gm.named_parameters():
        r = og[n].grad
        assert (p.grad is None) == (r is None), n
        if r is None or float(r.norm()) < 1e-4 * max(1.0, float(og[n].norm())):
            continue   # conv biases in front of a norm: mathematically zero, rounding noise in both
        e, e_cpu = rel(p.grad, r), rel(o32g[n].grad, r)
        worst, worst_cpu = max(worst, e), max(worst_cpu, e_cpu)
        assert e < max(3e-2, 4.0 * e_cpu), (n, e, e_cpu)   # (3e-2: one-channel norm scalars at the 4^3 level, batch 2, with the
                                                            #  fp32 MFMA kernels' summation order; 128^3 gradients: test_baseline_configs_gpu, 2e-2)
    print(f"worst relative gradient error vs fp64 oracle: HIP fp32 {worst:.2e}, CPU fp32 oracle {worst_cpu:.2e}")


def test_eval_mode_uses_double_updated_running_stats():
    """The reference runs the U-Net twice per forward (attn_unet_data_parallel.py:664,666): BN running
    stats move twice.  One folded update must leave the same buffers and the same eval output."""
    from coma_unet_amd.synthetic import make_batch
    S = (32, 32, 32)
    om, gm = _pair(S, 5)
    b = make_batch(2, S, seed=11)
    gb = _gpu_batch(b)
    with torch.no_grad():
        om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        gm(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    osd, gsd = om.state_dict(), gm.state_dict()
    for k in osd:
        if "running_" in k:
            assert rel(gsd[k], osd[k]) < 1e-4, k
        if "num_batches_tracked" in k:
            assert int(gsd[k]) == int(osd[k]) == (2 if k.startswith("model.") else 1), k
    om.eval(), gm.eval()
    with torch.no_grad():
        eo = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        eg = gm(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    assert eg.shape == eo.shape and rel(eg, eo) < 1e-3


def test_bf16_storage_error_is_measured():
    """bf16 activations: report the measured error instead of claiming the fp32 bound."""
    from coma_unet_amd.synthetic import make_batch
    S = (32, 32, 32)
    om, gm = _pair(S, 9, dtype=torch.bfloat16)
    b = make_batch(2, S, seed=13)
    gb = _gpu_batch(b)
    with torch.no_grad():
        oo = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        go = gm(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    e = rel(go[0].float(), oo[0])
    mae = float((go[0].float().cpu() - oo[0]).abs().mean())
    print(f"bf16 forward rel-L2 {e:.3e}, voxel MAE {mae:.3e}")
    assert e < 1e-1


def test_train_steps_follow_oracle():
    """Three AdamW steps on the same batch: losses must track the CPU oracle + torch.optim.AdamW."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    S = (32, 32, 32)
    om, gm = _pair(S, 21)
    b = make_batch(2, S, seed=17)
    gb = _gpu_batch(b)
    oopt = torch.optim.AdamW(om.parameters(), 1e-3)
    gopt = make_optimizer(gm, 1e-3)
    ocrit, gcrit = build_reference_criterion(), cu.build_reference_criterion()
    ol, gl = [], []
    for _ in range(3):
        oopt.zero_grad()
        res = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        tot = train_step_loss(res, b["tau"], b["roi"], b["covars"], ocrit)[0]
        tot.backward()
        oopt.step()
        ol.append(float(tot))
        losses, _ = train_step(gm, gcrit, gopt, gb)
        gl.append(float(losses[0]))
    print("oracle losses", ol, "gpu losses", gl)
    assert abs(gl[0] - ol[0]) / ol[0] < 1e-4
    for a, r in zip(gl[1:], ol[1:]):
        assert abs(a - r) / r < 5e-2     # Adam's first steps are sign-like: noise-level grads flip +-lr


def test_c2_shape_64cubed_batch4_properties():
    """C2-shaped run (64^3, batch 4): oracle forward parity + size-independent properties."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    S = (64, 64, 64)
    om, gm = _pair(S, 31)
    b = make_batch(4, S, seed=19)
    gb = _gpu_batch(b)
    losses, outs = forward_loss(gm, cu.build_reference_criterion(), gb)
    with torch.no_grad():
        oo = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
    assert rel(outs[0], oo[0]) < 1e-3
    assert float(outs[0].min()) >= 0.0                         # final ReLU
    assert [tuple(p.shape) for p in outs[1]] == [(4, 64 ** 3), (4, 32 ** 3), (4, 16 ** 3), (4, 8 ** 3), (4, 4 ** 3)]
    assert tuple(outs[2].shape) == (4, 1, 1, 1, 2048)
    # per-sample independence of the loss vector: permuting the batch permutes it
    losses[0].backward()
    perm = [2, 0, 3, 1]
    gb2 = {k: (v[perm] if torch.is_tensor(v) else [v[i] for i in perm]) for k, v in gb.items()}
    gm.zero_grad()
    losses2, _ = forward_loss(gm, cu.build_reference_criterion(), gb2)
    # BatchNorm couples samples only through order-independent batch statistics
    assert rel(losses2[1], losses[1][perm]) < 1e-4


def test_rccl_reducer_path_single_rank():
    """The RCCL code path (bucket hooks, async all-reduce on the process group's stream, join before the
    optimizer) with a 1-rank group: reductions are identities, so the losses must equal the plain step's."""
    import torch.distributed as dist
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer
    from coma_unet_amd.data_parallel import GradReducer, broadcast_module
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29571", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    try:
        S = (32, 32, 32)
        b = _gpu_batch(make_batch(2, S, seed=23))
        losses = []
        for use_reducer in (False, True):
            torch.manual_seed(3)
            gm = cu.build_model(volume_shape=S, static_prompts=True).cuda()
            gm.set_save_attn(None)
            gm.train(True)
            opt = make_optimizer(gm, 1e-3)
            red = None
            if use_reducer:
                broadcast_module(gm)
                red = GradReducer(opt, bucket_bytes=8 << 20)
                red.world = 2          # force the multi-rank code path on the 1-rank group
            crit = cu.build_reference_criterion()
            ls = [float(train_step(gm, crit, opt, b, red)[0][0]) for _ in range(4)]
            if use_reducer:
                assert red._buckets is not None and len(red._buckets) > 4 and len(red._hooks) > 100
            losses.append(ls)
        torch.cuda.synchronize()
        print("plain", losses[0], "reduced", losses[1])
        for a, r in zip(losses[1], losses[0]):
            assert abs(a - r) <= 5e-3 * abs(r)    # fp32 atomics in the weight-gradient / split-K merges are order-dependent:
                                                  # Adam at lr 1e-3 turns that into ~1e-3 run-to-run noise by steps 3-4
        # graph-replayed forward+backward followed by the flat all-reduce + AdamW (bench.py's N > 1 mode)
        from coma_unet_amd.train import GraphedTrainStep
        torch.manual_seed(3)
        gm = cu.build_model(volume_shape=S, static_prompts=True).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        opt = make_optimizer(gm, 1e-3)
        broadcast_module(gm)
        red = GradReducer(opt, bucket_bytes=8 << 20)
        red.world = 2
        gb = dict(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        step = GraphedTrainStep(gm, cu.build_reference_criterion(), opt, gb, warmup=2, reducer=red)
        ls = [float(step()[0][0]) for _ in range(2)]
        print("graph+reduce", ls)
        for a, r in zip(ls, losses[0][2:]):
            assert abs(a - r) <= 5e-3 * abs(r)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("sharded", [False, True])
def test_capi_rccl_exchange_eager_and_in_graph_single_rank(sharded):
    """The C-ABI RCCL path (coma_comm_init / coma_allreduce_sum_f32 / reduce_scatter + all_gather on a side HIP stream,
    launched from the gradient sink while backward is still running) with a 1-rank communicator: the reductions are
    identities, so eager and hipGraph-captured steps -- the graph then CONTAINS the collectives, the fork / join and the
    (sharded) optimizer step -- must follow the plain single-GPU trajectory."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    from coma_unet_amd.data_parallel import StreamedGradExchange
    from coma_unet_amd.rccl_comm import RcclComm
    S = (32, 32, 32)
    b = make_batch(2, S, seed=61)
    comm = RcclComm()
    assert comm.world == 1 and comm.rank == 0
    t = torch.arange(10, dtype=torch.float32, device="cuda")
    comm.all_reduce_(t), comm.broadcast_(t)
    r = torch.empty(10, device="cuda")
    comm.reduce_scatter(t, r), comm.all_gather(r, t)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.arange(10, dtype=torch.float32))

    def run(mode):
        torch.manual_seed(4)
        gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=torch.bfloat16).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        gb = _gpu_batch(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        opt = make_optimizer(gm, 1e-5)
        crit = cu.build_reference_criterion()
        ex = StreamedGradExchange(opt, comm, bucket_bytes=8 << 20, sharded=sharded) if mode != "plain" else None
        if mode == "graph":
            step = GraphedTrainStep(gm, crit, opt, gb, warmup=2, reducer=ex)
            assert step.in_graph
            ls = [float(step()[0][0]) for _ in range(3)]
        else:
            ls = [float(train_step(gm, crit, opt, gb, ex)[0][0]) for _ in range(5)][2:]
        if ex is not None:
            assert ex._buckets is not None and len(ex._buckets) > 4 and all(ex._launched)
            assert ex.early >= len(ex._buckets) // 2, (ex.early, len(ex._buckets))      # most buckets left before backward ended
        torch.cuda.synchronize()
        return ls, opt._flat_step

    plain, n0 = run("plain")
    eager, n1 = run("eager")
    graph, n2 = run("graph")
    print("plain", plain, "capi eager", eager, "capi graph", graph)
    assert n0 == n1 == n2 == 5
    for a, g_, r_ in zip(eager, graph, plain):
        assert abs(a - r_) <= 2e-2 * abs(r_) and abs(g_ - r_) <= 2e-2 * abs(r_)
    comm.close()


def test_graphed_step_matches_eager_steps():
    """The hipGraph-captured step (bench.py's one-GPU launch mode) must walk the same loss trajectory as eager steps.
    Learning rate 1e-5: at 1e-3 two runs of the SAME mode already differ by ~3-8 % after two steps (bf16 + fp32-atomic
    merge order, turned into sign-level update noise by Adam on near-zero gradients -- measured eager-vs-eager spread
    33.7 .. 35.9), which would only test the noise.  That the captured optimizer step really moves the parameters is
    checked at the end; that lr = 0 leaves them alone, in test_checkpoint_roundtrip_and_plateau_scheduler."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    S = (32, 32, 32)
    b = make_batch(2, S, seed=29)
    traj, moved = [], []
    for graphed in (False, True):
        torch.manual_seed(4)
        gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=torch.bfloat16).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        p0 = {n: p.detach().clone() for n, p in gm.named_parameters()}
        gb = _gpu_batch(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        opt = make_optimizer(gm, 1e-5)
        crit = cu.build_reference_criterion()
        if graphed:
            step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)       # 2 eager warm-up steps inside
            ls = [float(step()[0][0]) for _ in range(3)]
        else:
            ls = [float(train_step(gm, crit, opt, gb)[0][0]) for _ in range(5)][2:]
        traj.append(ls)
        torch.cuda.synchronize()
        moved.append(sum(float((p.detach() - p0[n]).abs().sum()) for n, p in gm.named_parameters()))
    print("eager", traj[0], "graph", traj[1], "moved", moved)
    for a, r in zip(traj[1], traj[0]):
        assert abs(a - r) <= 2e-2 * abs(r)
    assert moved[1] > 0 and abs(moved[1] - moved[0]) <= 0.1 * moved[0]     # 5 AdamW steps of size ~lr each, both modes


def test_write_through_gradients_equal_autograd_accumulation():
    """ops.GradSink: gradients written by the kernels into the optimizer's flat buffer must equal the ones
    autograd accumulates when write-through is off (same kernels; fp32 path, atomics-free comparison bound)."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer
    S = (32, 32, 32)
    b = make_batch(2, S, seed=31)
    grads, nbt = [], []
    for wt in (False, True):
        torch.manual_seed(5)
        # conv_algo=1: the direct kernels (no split-K / replica atomics in the forward pass), so that the two runs differ by
        # the gradient plumbing under test only -- with the fp32 MFMA kernels' order-dependent merges an ill-conditioned
        # scalar (a PReLU slope at the 4^3 level) moves by several per cent from run to run in EITHER mode
        gm = cu.build_model(volume_shape=S, static_prompts=True, conv_algo=1).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        gb = _gpu_batch(b)
        opt = make_optimizer(gm, 0.0, write_through=wt)     # lr 0, weight decay acts on lr too: parameters stay put
        crit = cu.build_reference_criterion()
        for _ in range(3):                                  # step 1 builds the flat layout; sinks are live from step 2
            train_step(gm, crit, opt, gb)
        assert opt.built and all(getattr(p, "_coma_sink", False) == wt for p in opt._flat_params)
        grads.append({n: p.grad.detach().clone() for n, p in gm.named_parameters() if p.grad is not None})
        nbt.append({n: int(v) for n, v in gm.state_dict().items() if n.endswith("num_batches_tracked")})
    assert grads[0].keys() == grads[1].keys()
    worst = max((rel(grads[1][n], grads[0][n]), n) for n in grads[0] if float(grads[0][n].abs().max()) > 1e-6)
    print("write-through vs accumulate, worst:", worst)
    assert worst[0] <= 1e-3, worst      # wgrad atomics order differs run to run
    assert nbt[0] == nbt[1] and any(v == 6 for v in nbt[0].values()) and any(v == 3 for v in nbt[0].values())


def test_side_stream_weight_preparation_equals_one_stream():
    """ops.SidePrep: routing, expert mix / re-layout and the expert-gradient scatter on a second HIP stream (eager, and as
    a parallel branch of the captured graph) must give the gradients and parameters of the one-stream order -- compared
    on the deterministic direct kernels (conv_algo=1), where any missing stream dependency shows as a mismatch."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    S = (32, 32, 32)
    b = make_batch(2, S, seed=33)
    res = {}
    was = ops.SidePrep.enabled
    try:
        for mode in ("one-stream", "side", "side-graph"):
            ops.SidePrep.enabled = mode != "one-stream"
            torch.manual_seed(9)
            gm = cu.build_model(volume_shape=S, static_prompts=True, conv_algo=1).cuda()
            gm.set_save_attn(None)
            gm.train(True)
            gb = _gpu_batch(b)
            gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
            opt = make_optimizer(gm, 0.0)        # lr 0 (weight decay acts through lr too): every step sees the same parameters
            crit = cu.build_reference_criterion()
            losses = []
            if mode == "side-graph":
                step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)        # 2 eager warm-up steps, then replays
                for _ in range(2):
                    losses.append(float(step()[0][0]))
            else:
                for _ in range(4):
                    losses.append(float(train_step(gm, crit, opt, gb)[0][0]))
            torch.cuda.synchronize()
            if mode != "one-stream":
                assert len(ops.SidePrep._bufs) > 40
            res[mode] = (losses, opt.flat_g.clone(), opt.flat_p.clone())
            layout = ss.flat_layout(gm, opt)
    finally:
        ops.SidePrep.enabled = was
    ref_l, ref_g, ref_p = res["one-stream"]
    for mode in ("side", "side-graph"):
        l, g, p_ = res[mode]
        print(mode, l, "vs", ref_l)
        for a in l:
            assert abs(a - ref_l[0]) <= 1e-5 * abs(ref_l[0]), (mode, l, ref_l)
        assert rel(g, ref_g) < 5e-3 and torch.equal(p_, ref_p), (mode, rel(g, ref_g))      # (norm / loss reductions use fp32 atomics)
        # tensor by tensor (a norm over the whole buffer does not see a small tensor that is entirely wrong)
        bad = ss.compare("fp32-direct", ss.flat_slices(layout, g), ss.flat_slices(layout, ref_g))
        assert not bad, (mode, bad[:10])


def test_side_stream_weight_gradients_equal_one_stream():
    """ops.WgradSide: weight gradients, expert scatters and routing backward on the second HIP stream (eager, as a parallel
    branch of the captured graph, and under a bare ``loss.backward()`` whose caller reads the gradients right away) must
    give the gradients and parameters of the one-stream order -- on the deterministic direct kernels (conv_algo=1), where a
    missing stream dependency or a buffer handed out too early shows as a mismatch."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, forward_loss, make_optimizer, GraphedTrainStep
    S = (32, 32, 32)
    b = make_batch(2, S, seed=35)
    res = {}
    was = ops.WgradSide.enabled
    try:
        for mode in ("one-stream", "side", "side-graph", "side-bare"):
            ops.WgradSide.enabled = mode != "one-stream"
            n0 = ops.WgradSide.launched
            torch.manual_seed(9)
            gm = cu.build_model(volume_shape=S, static_prompts=True, conv_algo=1).cuda()
            gm.set_save_attn(None)
            gm.train(True)
            gb = _gpu_batch(b)
            gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
            opt = make_optimizer(gm, 0.0)        # lr 0 (weight decay acts through lr too): every step sees the same parameters
            crit = cu.build_reference_criterion()
            losses = []
            if mode == "side-graph":
                step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)        # 2 eager warm-up steps, then replays
                for _ in range(2):
                    losses.append(float(step()[0][0]))
                g = opt.flat_g.clone()
            elif mode == "side-bare":
                for _ in range(2):
                    train_step(gm, crit, opt, gb)
                opt.zero_grad()
                ls, _ = forward_loss(gm, crit, gb)
                ls[0].backward()
                g = opt.flat_g.clone()       # on the current stream, right behind backward(): the join was queued by the pass
                assert not ops.WgradSide.dirty and not ops.WgradSide.keep
                losses = [float(ls[0])]
            else:
                for _ in range(4):
                    losses.append(float(train_step(gm, crit, opt, gb)[0][0]))
                g = opt.flat_g.clone()
            torch.cuda.synchronize()
            used = ops.WgradSide.launched - n0
            assert (used == 0) if mode == "one-stream" else (used >= 40), (mode, used)
            res[mode] = (losses, g, opt.flat_p.clone())
            layout = ss.flat_layout(gm, opt)
    finally:
        ops.WgradSide.enabled = was
    ref_l, ref_g, ref_p = res["one-stream"]
    for mode in ("side", "side-graph", "side-bare"):
        l, g, p_ = res[mode]
        print(mode, l, "vs", ref_l)
        for a in l:
            assert abs(a - ref_l[0]) <= 1e-5 * abs(ref_l[0]), (mode, l, ref_l)
        assert rel(g, ref_g) < 5e-3 and torch.equal(p_, ref_p), (mode, rel(g, ref_g))      # (norm / loss reductions use fp32 atomics)
        bad = ss.compare("fp32-direct", ss.flat_slices(layout, g), ss.flat_slices(layout, ref_g))      # tensor by tensor
        assert not bad, (mode, bad[:10])


def test_weight_preparation_ahead_equals_inline():
    """ops.PrepAhead: every layer's routing + expert mix at the start of the forward, on two streams beside each other
    (eager, and as parallel branches of the captured graph), must give the losses, gradients and parameters of the in-line
    order -- on the deterministic direct kernels (conv_algo=1).  The first forward of a configuration records the plan; a
    second forward while a backward is still outstanding falls back to the in-line preparation."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, forward_loss, make_optimizer, GraphedTrainStep
    S = (32, 32, 32)
    b = make_batch(2, S, seed=39)
    res = {}
    was = ops.PrepAhead.enabled
    try:
        for mode in ("inline", "ahead", "ahead-graph"):
            ops.PrepAhead.enabled = mode != "inline"
            n0 = ops.PrepAhead.used
            torch.manual_seed(9)
            gm = cu.build_model(volume_shape=S, static_prompts=True, conv_algo=1).cuda()
            gm.set_save_attn(None)
            gm.train(True)
            gb = _gpu_batch(b)
            gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
            opt = make_optimizer(gm, 0.0)        # lr 0 (weight decay acts through lr too): every step sees the same parameters
            crit = cu.build_reference_criterion()
            losses = []
            if mode == "ahead-graph":
                step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)        # eager step 1 records, step 2 prepares ahead; then replays
                for _ in range(2):
                    losses.append(float(step()[0][0]))
            else:
                for _ in range(4):
                    losses.append(float(train_step(gm, crit, opt, gb)[0][0]))
            torch.cuda.synchronize()
            used = ops.PrepAhead.used - n0
            assert (used == 0) if mode == "inline" else (used >= 60), (mode, used)
            res[mode] = (losses, opt.flat_g.clone(), opt.flat_p.clone())
            layout = ss.flat_layout(gm, opt)
            if mode == "ahead":
                # a second forward before the backward of the first: the persistent buffers are still needed -> in-line
                opt.zero_grad()
                l1, _ = forward_loss(gm, crit, gb)
                n1 = ops.PrepAhead.used
                with torch.no_grad():
                    forward_loss(gm, crit, gb)
                assert ops.PrepAhead.used == n1 and ops.PrepAhead.live > 0
                l1[0].backward()
                torch.cuda.synchronize()
                assert rel(opt.flat_g, res[mode][1]) < 5e-3
                opt.zero_grad()          # (layers whose output the loss never reaches see no backward: the step boundary resets the count)
                assert ops.PrepAhead.live == 0
    finally:
        ops.PrepAhead.enabled = was
    ref_l, ref_g, ref_p = res["inline"]
    for mode in ("ahead", "ahead-graph"):
        l, g, p_ = res[mode]
        print(mode, l, "vs", ref_l)
        for a in l:
            assert abs(a - ref_l[0]) <= 1e-5 * abs(ref_l[0]), (mode, l, ref_l)
        assert rel(g, ref_g) < 5e-3 and torch.equal(p_, ref_p), (mode, rel(g, ref_g))      # (norm / loss reductions use fp32 atomics)
        bad = ss.compare("fp32-direct", ss.flat_slices(layout, g), ss.flat_slices(layout, ref_g))      # tensor by tensor
        assert not bad, (mode, bad[:10])


def _grad_scale(model):
    return {n: (float(p.grad.abs().max()) if p.grad is not None else 0.0) for n, p in model.named_parameters()}


def _same_step(model, ref_params, ref_gscale, rtol=5e-3):
    """Parameters after 'one more step from the same state' in two runs must agree to rtol -- except tensors whose gradient
    is rounding noise or exactly zero depending on the run (the projection heads' BatchNorm behind an RnC loss that is
    identically zero at batch 2: |g| <= 1e-6 of the largest gradient): Adam turns such a gradient into a step of ~lr in a
    direction the fp32 atomics' order decides, or into no step at all."""
    gmax = max(ref_gscale.values())
    worst = (0.0, "")
    for n, p in model.named_parameters():
        r = ref_params[n]
        if float(r.abs().max()) == 0 or ref_gscale[n] <= 1e-6 * gmax:
            continue
        worst = max(worst, (rel(p, r), n))
    assert worst[0] < rtol, worst


def test_checkpoint_roundtrip_and_plateau_scheduler(tmp_path):
    """ReduceLROnPlateau drives FusedAdamW (eager and graph-replayed: a learning-rate change re-captures),
    and a checkpoint in the reference's format (attn_unet_data_parallel.py:943-955) restores model, moments, step count
    and scheduler so that the resumed run takes the same next step."""
    import coma_unet_amd as cu
    from coma_unet_amd import checkpoint
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    from torch.optim.lr_scheduler import ReduceLROnPlateau
    S = (32, 32, 32)
    b = make_batch(2, S, seed=41)

    def fresh():
        torch.manual_seed(6)
        gm = cu.build_model(volume_shape=S, static_prompts=True).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        gb = _gpu_batch(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        opt = make_optimizer(gm, 1e-3)
        return gm, gb, opt, ReduceLROnPlateau(opt, "min", patience=0, factor=0.5)

    gm, gb, opt, sched = fresh()
    crit = cu.build_reference_criterion()
    for _ in range(3):
        loss = train_step(gm, crit, opt, gb)[0][0]
    sched.step(1.0)
    sched.step(2.0)                       # no improvement with patience 0 -> lr halves
    assert abs(opt.param_groups[0]["lr"] - 5e-4) < 1e-12
    files = checkpoint.save_checkpoint(str(tmp_path), 7, gm, opt, loss, sched, checkpoint_iter=7)
    assert [os.path.basename(f) for f in files] == ["checkpoint_latest_epoch.pth", "checkpoint_epoch_7.pth"]
    raw = torch.load(files[0], map_location="cpu", weights_only=True)
    assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "scheduler_state_dict"}
    assert set(raw["optimizer_state_dict"]) == {"state", "param_groups"} and raw["optimizer_state_dict"]["param_groups"][0]["lr"] == 5e-4
    st0 = raw["optimizer_state_dict"]["state"][0]
    assert set(st0) == {"step", "exp_avg", "exp_avg_sq"} and float(st0["step"]) == 3.0
    next_loss = float(train_step(gm, crit, opt, gb)[0][0])            # step 4 of the original run (lr 5e-4)
    after4 = {n: p.detach().clone() for n, p in gm.named_parameters()}
    gscale4 = _grad_scale(gm)

    gm2, gb2, opt2, sched2 = fresh()
    for _ in range(2):                     # the flat optimizer layout exists after the first steps; then restore
        train_step(gm2, crit, opt2, gb2)
    assert checkpoint.load_checkpoint(files[0], gm2, opt2, sched2) == 8
    assert opt2.param_groups[0]["lr"] == 5e-4 and sched2.state_dict()["best"] == sched.state_dict()["best"]
    l2 = float(train_step(gm2, crit, opt2, gb2)[0][0])
    assert abs(l2 - next_loss) <= 1e-3 * abs(next_loss)
    _same_step(gm2, after4, gscale4)          # same step from the same state (atomics order differs run to run)

    # graph replay follows a scheduler change by re-capturing
    gm3, gb3, opt3, sched3 = fresh()
    g = GraphedTrainStep(gm3, crit, opt3, gb3, warmup=2)
    g()
    opt3.param_groups[0]["lr"] = 0.0       # a step with lr 0 must leave the parameters where they are
    before = {n: p.detach().clone() for n, p in gm3.named_parameters()}
    g()
    assert g._captured_hyper[0] == 0.0
    assert all(torch.equal(p, before[n]) for n, p in gm3.named_parameters())


def test_resume_into_fresh_optimizer_matches_uninterrupted_run(tmp_path):
    """The reference's resume order (validation.py:276-281, attn_unet_data_parallel.py:729-733): build a FRESH model and
    optimizer, load_state_dict both, then train.  The first resumed step must equal step N+1 of the uninterrupted run:
    Adam moments and the step count (bias correction) have to survive a load that happens before the flat layout exists.
    Also loads a stock torch.optim.AdamW state_dict the same way."""
    import coma_unet_amd as cu
    from coma_unet_amd import checkpoint
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer
    S = (32, 32, 32)
    b = make_batch(2, S, seed=43)

    def fresh(seed):
        torch.manual_seed(seed)
        gm = cu.build_model(volume_shape=S, static_prompts=True).cuda()
        gm.set_save_attn(None)
        gm.train(True)
        gb = _gpu_batch(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        return gm, gb, make_optimizer(gm, 1e-3)

    crit = cu.build_reference_criterion()
    gm, gb, opt = fresh(6)
    for _ in range(3):
        loss = train_step(gm, crit, opt, gb)[0][0]
    files = checkpoint.save_checkpoint(str(tmp_path), 3, gm, opt, loss, None, checkpoint_iter=5)
    sd_opt = opt.state_dict()
    m_norm = float(opt.flat_m.norm())
    l4 = float(train_step(gm, crit, opt, gb)[0][0])                      # step 4, uninterrupted
    after4 = {n: p.detach().clone() for n, p in gm.named_parameters()}
    gscale4 = _grad_scale(gm)

    gm2, gb2, opt2 = fresh(99)                                           # different init: everything must come from the file
    checkpoint.load_checkpoint(files[0], gm2, opt2, None)                # BEFORE any step: no flat layout yet
    assert not opt2.built
    l4b = float(train_step(gm2, crit, opt2, gb2)[0][0])
    assert opt2.built and opt2._flat_step == 4 and int(opt2._step_dev) == 4
    assert not any(opt2.state[p] for p in opt2._flat_params if p in opt2.state)      # no dead fp32 clones left behind
    assert abs(l4b - l4) <= 1e-3 * abs(l4)
    _same_step(gm2, after4, gscale4)   # with zeroed moments / step = 1 the first Adam step is ~lr everywhere: > 1e-1 on small tensors
    assert abs(float(opt2.state_dict()["state"][0]["step"]) - 4.0) == 0

    # a stock torch.optim.AdamW state_dict (same param order) loads into a fresh FusedAdamW the same way
    gm3, gb3, opt3 = fresh(6)
    ref_opt = torch.optim.AdamW(gm3.parameters(), 1e-3)
    ref_opt.load_state_dict(sd_opt)
    opt3.load_state_dict(ref_opt.state_dict())
    train_step(gm3, crit, opt3, gb3)
    assert opt3._flat_step == 4
    # moments after one more step: m4 = b1 m3 + (1-b1) g, so |m4| stays within a factor of the saved |m3| (not ~ (1-b1)|g| of a cold start)
    assert float(opt3.flat_m.norm()) > 0.5 * m_norm


def test_return_branches_embeddings_decoder_ds_save_attn():
    """The return contracts the training loop never takes (attn_unet_data_parallel.py:147-148, 225-227, 687-691):
    embeddings_out -> (out, projected, final, encoder features), decoder_ds -> (out, projected, final, []),
    save_attn -> the gate also returns its coefficients (and the layer still returns the gated features).
    Outputs must equal the default branch's (same weights, same inputs) and the oracle's shapes."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from oracle.coma_oracle import build_reference_model
    S = (32, 32, 32)
    b = make_batch(2, S, seed=71)
    gb = _gpu_batch(b)
    torch.manual_seed(9)
    base = cu.build_model(volume_shape=S).cuda()
    base.set_save_attn(None)
    base.train(True)
    sd = base.state_dict()
    with torch.no_grad():
        ref = base(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    assert len(ref) == 3

    def variant(**kw):
        m = cu.build_model(volume_shape=S, **kw).cuda()
        m.load_state_dict(sd)
        m.set_save_attn(None)
        m.train(True)
        return m

    with torch.no_grad():
        emb = variant(embeddings_out=True)
        o = emb(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
        assert len(o) == 4 and rel(o[0], ref[0]) < 1e-5 and rel(o[2], ref[2]) < 1e-5
        assert [tuple(e.shape) for e in o[3]] == [(2, 32, 32, 32, 32), (2, 64, 16, 16, 16), (2, 128, 8, 8, 8), (2, 256, 4, 4, 4), (2, 512, 2, 2, 2)]
        emb.train(False)        # eval + embeddings_out still returns the 4-tuple (:672-673 only short-cuts without embeddings_out)
        emb.set_training(False)
        assert len(emb(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])) == 4
        dds = variant(decoder_ds=True)
        o = dds(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
        assert len(o) == 4 and o[3] == [] and rel(o[0], ref[0]) < 1e-5 and dds.decoder_ds
        sa = variant()
        sa.set_save_attn("/nonexistent/attention_dump_dir")       # not None: the gates return (att, psi); nothing is written to disk here
        o = sa(gb["mri"], gb["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=gb["roi"])
        assert len(o) == 3 and rel(o[0], ref[0]) < 1e-5
        gate = sa.model[1].attention
        assert gate.save_attn is not None
        g = torch.randn((2, 32, 32, 32, 32), device="cuda")
        x = torch.randn((2, 32, 32, 32, 32), device="cuda")
        att, psi = gate(g=g, x=x)
        assert tuple(psi.shape) == (2, 32, 32, 32, 1) and rel(att, x * psi) < 1e-5 and 0.0 < float(psi.min()) and float(psi.max()) < 1.0
    # the oracle takes the same branches with the same tuple lengths
    om = build_reference_model(volume_shape=S, embeddings_out=True)
    om.set_save_attn(None)
    with torch.no_grad():
        oo = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
    assert len(oo) == 4 and [tuple(e.shape) for e in oo[3]] == [(2, 32, 32, 32, 32), (2, 64, 16, 16, 16), (2, 128, 8, 8, 8), (2, 256, 4, 4, 4), (2, 512, 2, 2, 2)]


def test_noncubic_volume_odd_batch():
    """Shapes the tiling has to cope with beyond the cubes of the BASELINE configs: a 32 x 48 x 64 volume, batch 3 --
    fp32 forward + loss against the oracle, then bf16 eager and graph-replayed train steps (finite, decreasing)."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss, train_step, make_optimizer, GraphedTrainStep
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    S, B = (32, 48, 64), 3
    om, gm = _pair(S, 77)
    b = make_batch(B, S, seed=17)
    with torch.no_grad():
        losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(b))
        ref = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        ref_total = train_step_loss(ref, b["tau"], b["roi"], b["covars"], build_reference_criterion())[0]
    assert rel(outs[0], ref[0]) < 1e-3
    assert abs(float(losses[0]) - float(ref_total)) <= 1e-3 * abs(float(ref_total))
    torch.manual_seed(8)
    gb16 = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=torch.bfloat16).cuda()
    gb16.set_save_attn(None)
    gb16.train(True)
    gb = _gpu_batch(b)
    gb["roi_pred_dicts"] = gb16._priors(b["roi_pred_dicts"], B, torch.device("cuda"))
    opt = make_optimizer(gb16, 1e-3)
    crit = cu.build_reference_criterion()
    l0 = float(train_step(gb16, crit, opt, gb)[0][0])
    step = GraphedTrainStep(gb16, crit, opt, gb, warmup=2)
    ls = [float(step()[0][0]) for _ in range(4)]
    assert all(np.isfinite(v) for v in [l0] + ls) and ls[-1] < l0
