"""train_dp(augment=...) and Prefetcher(augment=...): 32^3, batch 2, the model built as tests/test_train_loop_gpu.py builds it.
Augmentation reaches every training batch (eager and graph-replayed alike, a fresh transform per batch), never the
evaluation passes, and its generator state travels through the checkpoint."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = (32, 32, 32)
AUG = dict(rotate_deg=8.0, scale=(0.95, 1.05), translate_vox=2.0, elastic_grid=(4, 4, 4), elastic_sigma_vox=1.0, mri_scale=(0.9, 1.1),
           mri_shift=(-0.05, 0.05), mri_gamma=(0.9, 1.1), noise_sigma=(0.0, 0.02), seed=17)


def _loader(n_batches, B, abetas, seed0=0, triplet=False):
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
        out.append((item, item, item) if triplet else item)
    return out, lookup


def _model(seed=0, **kw):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    m = cu.build_model(volume_shape=S, **kw).cuda()
    m.set_save_attn(None)
    m.train(True)
    return m


def _recorder(**kw):
    from coma_unet_amd.augment import Augment3D

    class Rec(Augment3D):
        """Keeps what every call drew."""

        def __init__(self, **k):
            super().__init__(**k)
            self.drawn = []

        def sample_params(self, B, shape=(128, 128, 128)):
            r = super().sample_params(B, shape)
            self.drawn.append((r[0].copy(), None if r[1] is None else r[1].copy()))
            return r

    return Rec(**{**AUG, **kw})


class _BatchLosses:
    """Records the loss of every training batch, whichever way train_dp ran it (train_step or a GraphedTrainStep replay)."""

    def __enter__(self):
        from coma_unet_amd import train as T, train_loop as TL
        self.T, self.TL, self.losses, self.kinds = T, TL, [], []
        self.step, self.call = TL.train_step, T.GraphedTrainStep.__call__

        def step(*a, **k):
            r = self.step(*a, **k)
            self.losses.append(float(r[0][0])), self.kinds.append("eager")
            return r

        def call(this, *a, **k):
            r = self.call(this, *a, **k)
            self.losses.append(float(r[0][0])), self.kinds.append("graph")
            return r

        TL.train_step, T.GraphedTrainStep.__call__ = step, call
        return self

    def __exit__(self, *exc):
        self.TL.train_step, self.T.GraphedTrainStep.__call__ = self.step, self.call


def test_train_dp_eager_with_augment():
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    train, lookup = _loader(3, 2, [[1, 0], [0, 1], [1, 1]], seed0=70, triplet=True)
    runs = {}
    for name, aug in (("plain", None), ("aug", _recorder()), ("dict", dict(AUG))):
        kw = {} if aug is None else {"augment": aug}
        runs[name] = A.train_dp(_model(11), cu.build_reference_criterion(), train, None, 2, 1e-3, save_path="", cuda_id=0,
                                roi_vecs_dict=lookup, fold_id=3, graph=False, **kw)
        if name == "aug":
            assert aug.calls == 6 and len(aug.drawn) == 6
            assert all(not np.array_equal(aug.drawn[0][0], d[0]) for d in aug.drawn[1:])        # a fresh transform per batch
    print("epoch losses:", runs)
    assert all(len(v) == 2 and np.all(np.isfinite(v)) for v in runs.values())
    assert all(abs(a - p) > 1e-6 * abs(p) for a, p in zip(runs["aug"], runs["plain"]))
    assert all(abs(a - p) > 1e-6 * abs(p) for a, p in zip(runs["dict"], runs["plain"]))         # a dict of arguments augments too


def test_augmentation_never_touches_evaluation(tmp_path):
    """A fixed model (lr 0, frozen BatchNorm): the validation pass inside train_dp gives bitwise the metrics of a run without
    augment, the augmenter ran once per TRAINING batch, and only checkpoints of an augmenting run carry its state.
    The model runs on the deterministic direct kernels (conv_algo=1), as every bitwise comparison of two forwards in this suite
    does: the default kernels merge the deep layers' split-K partials with fp32 atomics, and two evaluations of the SAME model
    on the SAME data then differ in the last bit (measured here: MAE 0.25130627 vs 0.25130624), augmentation or not."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import train_loop as TL
    train, lk1 = _loader(3, 2, [[1, 0], [0, 1], [1, 1]], seed0=70, triplet=True)
    val, lk2 = _loader(2, 2, [[1, 0], [0, 0]], seed0=90)
    lookup = {**lk1, **lk2}
    seen, orig = {}, TL.contrastive_test
    try:
        for name, aug in (("plain", None), ("aug", _recorder())):
            rec = []
            TL.contrastive_test = lambda *a, _r=rec, **k: (_r.append(orig(*a, **k)), _r[-1])[1]
            kw = {} if aug is None else {"augment": aug}
            d = str(tmp_path / name)
            A.train_dp(_model(11, conv_algo=1), cu.build_reference_criterion(), train, val, 1, 0.0, save_path=d, cuda_id=0, roi_vecs_dict=lookup,
                       fold_id=3, val_iter=1, graph=False, freeze_bn=True, **kw)
            seen[name] = rec
            raw = torch.load(os.path.join(d, "checkpoints", "checkpoint_latest_epoch.pth"), map_location="cpu", weights_only=True)
            assert ("augment_state" in raw) == (aug is not None)
            if aug is not None:
                assert aug.calls == 3 and raw["augment_state"]["calls"] == 3
    finally:
        TL.contrastive_test = orig
    assert len(seen["plain"]) == len(seen["aug"]) == 1
    for cls_p, cls_a in zip(seen["plain"][0], seen["aug"][0]):
        for k, (p, a) in enumerate(zip(cls_p, cls_a)):
            p = np.asarray(p.detach().cpu() if torch.is_tensor(p) else p, dtype=np.float64)
            a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
            assert np.array_equal(p, a, equal_nan=True), (k, p, a)


def test_train_dp_graphed_loop_with_augment_matches_eager():
    """graph=True: batches 1-2 eager, capture on the third, later batches loaded into the graph's static inputs and replayed --
    each with its own transform.  Per-batch losses against the all-eager run of the same augmenter seed, with the tolerance
    test_train_loop_gpu.py uses between the graphed and the eager loop (2e-2 relative, lr 1e-5)."""
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import train as T
    train, lookup = _loader(5, 2, [[1, 0], [0, 1], [1, 1], [0, 0], [1, 0]], seed0=120, triplet=True)
    runs = {}
    for mode in (False, True):
        m = _model(21, static_prompts=True, compute_dtype=torch.bfloat16)
        aug = _recorder()
        with _BatchLosses() as rec:
            A.train_dp(m, cu.build_reference_criterion(), train, None, 2, 1e-5, save_path="", cuda_id=0, roi_vecs_dict=lookup,
                       fold_id=0, graph=mode, optimizer=T.make_optimizer(m, 1e-5), augment=aug)
        runs[mode] = (rec.losses, rec.kinds, aug.drawn)
    (le, ke, de), (lg, kg, dg) = runs[False], runs[True]
    assert ke == ["eager"] * 10 and kg == ["eager"] * 2 + ["graph"] * 8          # captured on the third batch, replayed since
    assert len(de) == len(dg) == 10
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(de, dg))
    assert all(not np.array_equal(dg[2][0], d[0]) for d in dg[3:])                # a fresh transform per replay
    print("eager:", le, "\ngraph:", lg)
    for a, b in zip(lg, le):
        assert np.isfinite(a) and abs(a - b) <= 2e-2 * abs(b), (lg, le)


def test_resume_continues_the_parameter_stream(tmp_path):
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd import checkpoint
    from coma_unet_amd.train import make_optimizer
    from torch.optim.lr_scheduler import ReduceLROnPlateau
    train, lookup = _loader(2, 2, [[1, 0], [0, 1]], seed0=70, triplet=True)
    common = dict(save_path=str(tmp_path), cuda_id=0, roi_vecs_dict=lookup, fold_id=3, graph=False)
    whole = _recorder()
    A.train_dp(_model(11), cu.build_reference_criterion(), train, None, 2, 1e-4, **{**common, "save_path": ""}, augment=whole)
    first = _recorder()
    A.train_dp(_model(11), cu.build_reference_criterion(), train, None, 1, 1e-4, **common, augment=first)
    ck = os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth")
    m2 = _model(12)
    opt2 = make_optimizer(m2, 1e-4)
    sch2 = ReduceLROnPlateau(opt2, "min", patience=5)
    rest = _recorder(seed=999)                        # another seed: everything must come from the file
    start = checkpoint.load_checkpoint(ck, m2, opt2, sch2, augment=rest)
    assert start == 1 and rest.calls == 2 and rest.seed == AUG["seed"]
    m2.train(True)
    A.train_dp(m2, cu.build_reference_criterion(), train, None, 2, 1e-4, **{**common, "save_path": ""}, from_checkpoint=True,
               optimizer=opt2, scheduler=sch2, start_epoch=start, augment=rest)
    assert len(whole.drawn) == 4 and len(first.drawn) == 2 and len(rest.drawn) == 2
    for a, b in zip(whole.drawn, first.drawn + rest.drawn):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the same through train_dp's own kwarg
    raw = torch.load(ck, map_location="cpu", weights_only=True)
    again = _recorder(seed=5)
    A.train_dp(m2, cu.build_reference_criterion(), train, None, 2, 1e-4, **{**common, "save_path": ""}, from_checkpoint=True,
               optimizer=opt2, scheduler=sch2, start_epoch=1, augment=again, augment_state=raw["augment_state"])
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(whole.drawn[2:], again.drawn))


def test_prefetcher_augments_each_prepared_sample():
    from coma_unet_amd import input_pipeline as P
    rng = np.random.default_rng(3)
    samples = []
    for i in range(2):
        shp = (24 + 2 * i, 20, 22)
        samples.append({"mri": rng.random(shp).astype(np.float32), "tau": rng.random(shp).astype(np.float32),
                        "roi": (rng.random(shp) > 0.3).astype(np.float32) * 17, "spacing": (1.0, 1.0, 1.0), "id": i})
    aug, twin = _recorder(), _recorder()
    got = list(P.Prefetcher(samples, augment=aug))
    plain = list(P.Prefetcher(samples))
    torch.cuda.synchronize()
    assert [g["id"] for g in got] == [0, 1] and aug.calls == 2
    for g, p, (params, disp) in zip(got, plain, aug.drawn):
        want = twin(p["mri"], p["tau"], p["roi"], params=params, disp=disp)
        torch.cuda.synchronize()
        for k, w in zip(("mri", "tau", "roi"), want):
            assert g[k].shape == p[k].shape and torch.equal(g[k], w), k
        assert not torch.equal(g["tau"], p["tau"])
        assert not g["mri"][g["roi"] == 0].any()
