"""Prefetcher(smoothing=...) and train_dp(smooth_tau=...): the tau target -- and nothing else -- is smoothed, in front of the
augmentation warp, for training and validation batches alike; without the option nothing is imported and nothing changes.
32^3, batch 2, the model built as tests/test_augment_train_gpu.py builds it (conv_algo=1: the deterministic kernels, as every
bitwise comparison of two runs in this suite uses)."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = (32, 32, 32)


def _samples():
    """The three-sample input of test_input_pipeline.py::test_prefetcher_yields_prepared_samples."""
    rng = np.random.default_rng(3)
    samples = []
    for i in range(3):
        shp = (24 + 2 * i, 20, 22)
        samples.append({"mri": rng.random(shp).astype(np.float32), "tau": rng.random(shp).astype(np.float32),
                        "roi": (rng.random(shp) > 0.5).astype(np.float32), "spacing": (1.0, 1.0, 1.0), "id": i})
    return samples


def test_prefetcher_smooths_tau_only():
    from coma_unet_amd import input_pipeline as P
    from coma_unet_amd.smooth import GaussianSmooth3D
    samples = _samples()
    plain = list(P.Prefetcher(samples))
    got = list(P.Prefetcher(samples, smoothing=True))
    torch.cuda.synchronize()
    assert [g["id"] for g in got] == [0, 1, 2]
    ref = GaussianSmooth3D.reference()
    for g, p in zip(got, plain):
        assert torch.equal(g["mri"], p["mri"]) and torch.equal(g["roi"], p["roi"])
        assert g["tau"].shape == p["tau"].shape and torch.equal(g["tau"], ref(p["tau"]))
        assert not torch.equal(g["tau"], p["tau"])
    # a dict and an instance are taken too; resize=False goes through nan_to_num and the plain launch
    inst = GaussianSmooth3D.from_fwhm(2, (2, 2, 2))
    for spec, twin in ((dict(sigma=0.8, axes=("z", "y", "x"), boundary="nearest"), GaussianSmooth3D(0.8, ("z", "y", "x"), boundary="nearest")),
                       (inst, inst)):
        for resize in (True, False):
            got = list(P.Prefetcher(samples, smoothing=spec, resize=resize))
            base = list(P.Prefetcher(samples, resize=resize))
            torch.cuda.synchronize()
            for g, p in zip(got, base):
                assert torch.equal(g["mri"], p["mri"]) and torch.equal(g["roi"], p["roi"]) and torch.equal(g["tau"], twin(p["tau"]))


def test_prefetcher_warps_the_smoothed_tau():
    from coma_unet_amd import input_pipeline as P
    from coma_unet_amd.augment import Augment3D
    from coma_unet_amd.smooth import GaussianSmooth3D
    kw = dict(rotate_deg=8.0, scale=(0.95, 1.05), translate_vox=2.0, seed=17)
    samples = _samples()
    aug, twin, other = Augment3D(**kw), Augment3D(**kw), Augment3D(**kw)     # (all three draw the same transforms in the same order)
    got = list(P.Prefetcher(samples, smoothing=True, augment=aug))
    plain = list(P.Prefetcher(samples))
    torch.cuda.synchronize()
    ref = GaussianSmooth3D.reference()
    for g, p in zip(got, plain):
        want = twin(p["mri"], ref(p["tau"]), p["roi"])
        unsmoothed = other(p["mri"], p["tau"], p["roi"])
        torch.cuda.synchronize()
        for k, w in zip(("mri", "tau", "roi"), want):
            assert torch.equal(g[k], w), k
        assert not torch.equal(g["tau"], unsmoothed[1])


def _loader(n_batches, B, abetas, seed0=0, triplet=False, tau_map=None):
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
        tau = b["tau"] if tau_map is None else tau_map(b["tau"])
        item = (b["mri"], tau, b["roi"], (ab, cov), paths)
        out.append((item, item, item) if triplet else item)
    return out, lookup


def _model(seed=0, **kw):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    m = cu.build_model(volume_shape=S, **kw).cuda()
    m.set_save_attn(None)
    m.train(True)
    return m


class _Spy:
    """Records the tau of every training step and of every evaluation batch, and the loss of every training batch."""

    def __enter__(self):
        from coma_unet_amd import train_loop as TL
        self.TL, self.train_tau, self.eval_tau, self.losses = TL, [], [], []
        self.step, self.stats = TL.train_step, TL.M.eval_stats

        def step(model, criterion, optimizer, batch, *a, **k):
            self.train_tau.append(batch["tau"].clone())
            r = self.step(model, criterion, optimizer, batch, *a, **k)
            self.losses.append(float(r[0][0]))
            return r

        def stats(pred, tau, *a, **k):
            if tau.size(0) > 1:              # (the whole batch: contrastive_test's own call, not the per-sample correlation ones)
                self.eval_tau.append(tau.clone())
            return self.stats(pred, tau, *a, **k)

        TL.train_step, TL.M.eval_stats = step, stats
        return self

    def __exit__(self, *exc):
        self.TL.train_step, self.TL.M.eval_stats = self.step, self.stats


def _same_bits(res_a, res_b):
    """Two contrastive_test results, entry by entry, bit for bit (NaN equal to NaN): the comparison
    test_augment_train_gpu.py::test_augmentation_never_touches_evaluation applies to an untouched run."""
    for cls_a, cls_b in zip(res_a, res_b):
        for k, (x, y) in enumerate(zip(cls_a, cls_b)):
            x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)
            y = np.asarray(y.detach().cpu() if torch.is_tensor(y) else y, dtype=np.float64)
            assert np.array_equal(x, y, equal_nan=True), (k, x, y)


def test_train_dp_smooths_training_and_validation_tau():
    """Four runs of one epoch (two training batches, one validation batch): the option absent, smooth_tau=None, smooth_tau=True,
    and the option absent on loaders whose tau was smoothed beforehand.

    Equality of two runs is judged the way test_augment_train_gpu.py::test_augmentation_never_touches_evaluation judges an
    untouched run: a fixed model (lr 0, frozen BatchNorm) on the deterministic direct kernels (conv_algo=1), the metrics of the
    validation pass inside train_dp bit for bit.  The training losses are then two evaluations of the same model on the same
    data; they are held to 1e-5 relative, the loss bound of the direct kernels in tests/_step_state.py (TOL["fp32-direct"],
    measured repeat spread 2e-6): the loss and norm kernels behind them are not pinned to be bitwise repeatable."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import train_loop as TL
    from coma_unet_amd.smooth import GaussianSmooth3D
    ref = GaussianSmooth3D.reference()
    pre = lambda t: ref(t.cuda().contiguous()).cpu()
    runs, orig = {}, TL.contrastive_test
    for name, kw, tau_map in (("absent", {}, None), ("none", {"smooth_tau": None}, None), ("on", {"smooth_tau": True}, None),
                              ("pre", {}, pre)):
        train, lk1 = _loader(2, 2, [[1, 0], [0, 1]], seed0=70, triplet=True, tau_map=tau_map)
        val, lk2 = _loader(1, 2, [[1, 0]], seed0=90, tau_map=tau_map)
        saved, rec = None, []
        if name == "none":
            saved = sys.modules.pop("coma_unet_amd.smooth")
        TL.contrastive_test = lambda *a, _r=rec, **k: (_r.append(orig(*a, **k)), _r[-1])[1]
        try:
            with _Spy() as spy:
                losses = A.train_dp(_model(11, conv_algo=1), cu.build_reference_criterion(), train, val, 1, 0.0, save_path="", cuda_id=0,
                                    roi_vecs_dict={**lk1, **lk2}, fold_id=3, val_iter=1, graph=False, freeze_bn=True, **kw)
            if name == "none":
                assert "coma_unet_amd.smooth" not in sys.modules            # nothing imported without the option
        finally:
            TL.contrastive_test = orig
            if saved is not None:
                sys.modules["coma_unet_amd.smooth"] = saved
        assert len(spy.train_tau) == 2 and len(spy.eval_tau) == 1 and len(losses) == 1 and len(rec) == 1
        runs[name] = (losses, spy.losses, spy.train_tau, spy.eval_tau, train, val, rec[0])
    print({k: (v[0], v[1]) for k, v in runs.items()})
    # what reached the criterion and the evaluation: the smoothed target, bit for bit; untouched without the option
    _, _, t_on, e_on, train, val, _ = runs["on"]
    for got, item in zip(t_on, train):
        assert torch.equal(got, ref(item[0][1].cuda())) and not torch.equal(got.cpu(), item[0][1])
    assert torch.equal(e_on[0], ref(val[0][1].cuda())) and not torch.equal(e_on[0].cpu(), val[0][1])
    for name in ("absent", "none"):
        assert all(torch.equal(got.cpu(), item[0][1]) for got, item in zip(runs[name][2], runs[name][4]))
        assert torch.equal(runs[name][3][0].cpu(), runs[name][5][0][1])
    # None is the run without the option; the option is the run on smoothed data; and it is not a no-op
    for a, b in (("none", "absent"), ("on", "pre")):
        _same_bits(runs[a][6], runs[b][6])
        worst = max(abs(x - y) / abs(y) for x, y in zip(runs[a][0] + runs[a][1], runs[b][0] + runs[b][1]))
        print(f"{a} vs {b}: worst relative difference of the training losses {worst:.2e} (bound 1e-5)")
        assert worst <= 1e-5
    assert all(abs(a - b) > 1e-3 * abs(b) for a, b in zip(runs["on"][1], runs["absent"][1]))
    assert float(runs["on"][6][0][0]) != float(runs["absent"][6][0][0])                 # the validation MAE moved too


def test_graphed_loop_with_smooth_tau_matches_eager():
    """graph=True: the smoothing runs in front of the graph load, the replayed steps see the smoothed target.  Per-batch losses
    against the all-eager run, with the tolerance test_train_loop_gpu.py uses between the two loops (2e-2 relative, lr 1e-5)."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import train as T
    from coma_unet_amd import train_loop as TL
    train, lookup = _loader(4, 2, [[1, 0], [0, 1], [1, 1], [0, 0]], seed0=120, triplet=True)
    runs = {}
    for mode in (False, True):
        m = _model(21, static_prompts=True, compute_dtype=torch.bfloat16)
        losses, kinds = [], []
        step, call = TL.train_step, T.GraphedTrainStep.__call__

        def eager(*a, **k):
            r = step(*a, **k)
            losses.append(float(r[0][0])), kinds.append("eager")
            return r

        def replay(this, *a, **k):
            r = call(this, *a, **k)
            losses.append(float(r[0][0])), kinds.append("graph")
            return r

        TL.train_step, T.GraphedTrainStep.__call__ = eager, replay
        try:
            A.train_dp(m, cu.build_reference_criterion(), train, None, 1, 1e-5, save_path="", cuda_id=0, roi_vecs_dict=lookup,
                       fold_id=0, graph=mode, optimizer=T.make_optimizer(m, 1e-5), smooth_tau=True)
        finally:
            TL.train_step, T.GraphedTrainStep.__call__ = step, call
        runs[mode] = (losses, kinds)
    (le, ke), (lg, kg) = runs[False], runs[True]
    assert ke == ["eager"] * 4 and kg == ["eager"] * 2 + ["graph"] * 2
    print("eager:", le, "\ngraph:", lg)
    for a, b in zip(lg, le):
        assert np.isfinite(a) and abs(a - b) <= 2e-2 * abs(b), (lg, le)
