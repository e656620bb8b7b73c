"""On-device 3-D augmentation for the training path (build-side: the reference's dataset code only resamples).

One kernel launch (``coma_augment_warp``, csrc/augment.hip) warps the MRI, the tau target and the ROI label volume of every
sample of a batch by the SAME per-sample transform: an affine map (rotation about the volume centre, anisotropic scale,
translation, optional flips) plus an optional smooth elastic displacement, trilinear for MRI and tau, nearest-neighbour for
the labels; the MRI additionally takes an intensity map (scale, shift, gamma), additive Gaussian noise from a counter-based
generator, and stays exactly 0 wherever the warped ROI is 0 (the reference's ``mri[roi == 0] = 0``).  The normative
semantics are in include/coma_unet.h and DESIGN.md section 4 "Augmentation".

Everything random is drawn on the host from one ``numpy`` generator (``sample_params``), so a run is reproducible from
``seed`` and resumable from ``state_dict()``; the device only sees a (B, 16) parameter table and the control grid.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr

NPARAM = 16
MAX_GRID = 8                       # control points per axis the kernel stages in LDS
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0], dtype=np.float32)
_MASK64 = (1 << 64) - 1


def _three(v, name):
    a = np.atleast_1d(np.asarray(v, dtype=np.float64))
    if a.shape == (1,):
        a = np.repeat(a, 3)
    if a.shape != (3,):
        raise ValueError(f"{name}: a scalar or three values (z, y, x) expected, got {v!r}")
    return a


def matrix(rotate_deg_zyx=(0.0, 0.0, 0.0), scale_zyx=(1.0, 1.0, 1.0), translate_zyx=(0.0, 0.0, 0.0), flips=(False, False, False),
           shape=(128, 128, 128)):
    """The deterministic composition: a (3, 4) float64 matrix A in (z, y, x) order that maps an OUTPUT voxel index o to the
    SOURCE voxel index  s = c + R diag(1 / scale) F (o - c) + t,  c = (shape - 1) / 2.

    rotate_deg_zyx: angles about the z, y and x axis; R = Rz Ry Rx.  scale_zyx > 1 magnifies the content along that axis.
    translate_zyx: in voxels, added to the source index (the centre of the output shows source voxel c + t).
    flips: per axis, mirror about the centre.  Zero angles, unit scales, no flips and no translation give the exact
    identity; flips with integer translations give exact signed permutation matrices."""
    az, ay, ax = (math.radians(float(a)) for a in _three(rotate_deg_zyx, "rotate_deg_zyx"))
    sc, t = _three(scale_zyx, "scale_zyx"), _three(translate_zyx, "translate_zyx")
    if not np.all(np.isfinite(sc)) or np.any(sc <= 0):
        raise ValueError(f"scale_zyx must be positive, got {scale_zyx!r}")
    f = np.array([-1.0 if bool(b) else 1.0 for b in flips])
    if f.shape != (3,) or len(shape) != 3:
        raise ValueError("flips and shape take three entries (z, y, x)")
    cz_, sz_, cy_, sy_, cx_, sx_ = math.cos(az), math.sin(az), math.cos(ay), math.sin(ay), math.cos(ax), math.sin(ax)
    Rz = np.array([[1, 0, 0], [0, cz_, -sz_], [0, sz_, cz_]], dtype=np.float64)       # about z: turns the (y, x) plane
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]], dtype=np.float64)       # about y: the (z, x) plane
    Rx = np.array([[cx_, -sx_, 0], [sx_, cx_, 0], [0, 0, 1]], dtype=np.float64)       # about x: the (z, y) plane
    M = (Rz @ Ry @ Rx) @ np.diag(1.0 / sc) @ np.diag(f)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    A = np.empty((3, 4), dtype=np.float64)
    A[:, :3] = M
    A[:, 3] = c - M @ c + t
    return A + 0.0                 # (-0.0 -> 0.0)


def pack_params(A, mri_scale=1.0, mri_shift=0.0, mri_gamma=1.0, noise_sigma=0.0):
    """One row of the kernel's parameter table from a (3, 4) matrix and the four intensity parameters."""
    row = np.empty(NPARAM, dtype=np.float32)
    row[:12] = np.asarray(A, dtype=np.float64).reshape(12)
    row[12:] = (mri_scale, mri_shift, mri_gamma, noise_sigma)
    return row


def _upload(a, dev):
    """Host table -> device on the current stream, through a pinned copy of its own (torch's caching host allocator keeps the block
    alive until the stream has read it; the caller's array is free to change at once)."""
    return torch.from_numpy(np.array(a, dtype=np.float32)).pin_memory().to(dev, non_blocking=True)


def _view(t, D, H, W, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"augment: {name} must be an fp32 device tensor (there is no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"augment: {name} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    if t.dim() < 3 or tuple(t.shape[-3:]) != (D, H, W):
        raise ValueError(f"augment: {name} has shape {tuple(t.shape)}, expected (..., {D}, {H}, {W})")
    return t


def warp(mri, tau, roi, params, disp=None, seed=0, out=None):
    """The kernel as it is: ALWAYS one launch of ``coma_augment_warp`` on the current stream.  mri / tau / roi: contiguous fp32
    device tensors of equal shape whose last three dimensions are (D, H, W); everything in front is the batch.  params:
    (B, 16) fp32 (device tensor or numpy); disp: None or (B, 3, gz, gy, gx) fp32, 2..8 points per axis; out: optional
    (mri, tau, roi) buffers of the input shapes, disjoint from the inputs.  Returns the three outputs."""
    if not torch.is_tensor(mri) or mri.dim() < 3:
        raise ValueError("augment: volumes of at least three dimensions expected")
    D, H, W = (int(s) for s in mri.shape[-3:])
    for t, name in ((mri, "mri"), (tau, "tau"), (roi, "roi")):
        _view(t, D, H, W, name)
    if not (mri.numel() == tau.numel() == roi.numel()) or mri.numel() == 0:
        raise ValueError(f"augment: mri / tau / roi differ in size: {tuple(mri.shape)}, {tuple(tau.shape)}, {tuple(roi.shape)}")
    B = mri.numel() // (D * H * W)
    dev = mri.device
    if out is None:
        out = (torch.empty_like(mri), torch.empty_like(tau), torch.empty_like(roi))
    if len(out) != 3:
        raise ValueError("augment: out= takes three buffers (mri, tau, roi)")
    for o, i, name in zip(out, (mri, tau, roi), ("out[0]", "out[1]", "out[2]")):
        _view(o, D, H, W, name)
        if o.numel() != i.numel() or o.device != dev:
            raise ValueError(f"augment: {name} does not match its input: {tuple(o.shape)} vs {tuple(i.shape)}")
    if not torch.is_tensor(params):
        params = _upload(params, dev)
    if params.dtype != torch.float32 or tuple(params.shape) != (B, NPARAM) or not params.is_contiguous() or params.device != dev:
        raise ValueError(f"augment: params must be a contiguous ({B}, {NPARAM}) fp32 table on {dev}, got {tuple(params.shape)}")
    g = (0, 0, 0)
    if disp is not None:
        if not torch.is_tensor(disp):
            disp = _upload(disp, dev)
        if disp.dtype != torch.float32 or disp.dim() != 5 or tuple(disp.shape[:2]) != (B, 3) or not disp.is_contiguous() \
                or disp.device != dev:
            raise ValueError(f"augment: disp must be a contiguous ({B}, 3, gz, gy, gx) fp32 grid on {dev}, got {tuple(disp.shape)}")
        g = tuple(int(s) for s in disp.shape[2:])
        if min(g) < 2 or max(g) > MAX_GRID:
            raise ValueError(f"augment: control grid {g}: 2..{MAX_GRID} points per axis")
    check(lib.coma_augment_warp(ptr(mri), ptr(tau), ptr(roi), ptr(out[0]), ptr(out[1]), ptr(out[2]), B, D, H, W, ptr(params),
                                ptr(disp), g[0], g[1], g[2], int(seed) & _MASK64, L.stream()), "coma_augment_warp")
    return tuple(out)


class Augment3D:
    """Random spatial + intensity augmentation of a (mri, tau, roi) batch on the device, one kernel launch per batch.

    Spatial (identical for mri / tau / roi of a sample):
      rotate_deg:   a scalar or (z, y, x): each angle uniform in [-r, r] degrees, about the volume centre;
      scale:        (lo, hi): each axis uniform in [lo, hi] (> 1 magnifies);
      translate_vox: a scalar or (z, y, x): each shift uniform in [-t, t] voxels;
      flip_axes:    the axes (0 = z, 1 = y, 2 = x) that MAY flip, each with probability 1/2.  Empty by default: the model's
                    learned prompts and the FreeSurfer labels are lateralised (left and right structures carry different
                    ids), so a mirrored sample shows anatomy under the wrong labels -- enable a flip only for an axis
                    along which neither matters;
      elastic_grid / elastic_sigma_vox: a (gz, gy, gx) control grid (2..8 points per axis) of N(0, sigma^2) displacements
                    in voxels, interpolated trilinearly over the volume; None / 0: no elastic part.
    Intensity (MRI only; tau is the regression target and is only resampled): mri_scale, mri_shift, mri_gamma, noise_sigma,
      each a (lo, hi) range drawn uniformly per sample.
    p: the probability that a sample is augmented at all; otherwise it gets the exact identity.

    Draw order (one ``np.random.default_rng(seed)`` stream; EVERY draw below happens for every sample, whatever ``p`` decides and
    whichever ranges are degenerate, so the position in the stream depends only on the number of samples drawn so far): per
    sample b = 0 .. B-1:  u_p;  rotation z, y, x;  scale z, y, x;  translation z, y, x;  one flip coin per entry of
    flip_axes, in the given order;  mri_scale;  mri_shift;  mri_gamma;  noise_sigma;  then, with an elastic grid, the
    (3, gz, gy, gx) normal displacements of that sample.  The noise kernel's seed of the n-th ``__call__`` is derived from
    (seed, n), not from the stream."""

    def __init__(self, rotate_deg=10.0, scale=(0.9, 1.1), translate_vox=4.0, flip_axes=(), elastic_grid=None, elastic_sigma_vox=0.0,
                 mri_scale=(1.0, 1.0), mri_shift=(0.0, 0.0), mri_gamma=(1.0, 1.0), noise_sigma=(0.0, 0.0), p=1.0, seed=0):
        self.rotate_deg = _three(rotate_deg, "rotate_deg")
        self.translate_vox = _three(translate_vox, "translate_vox")
        if np.any(self.rotate_deg < 0) or np.any(self.translate_vox < 0):
            raise ValueError("rotate_deg / translate_vox are half-widths: >= 0")
        self.scale = self._range(scale, "scale", positive=True)
        self.flip_axes = tuple(int(a) for a in flip_axes)
        if any(a not in (0, 1, 2) for a in self.flip_axes) or len(set(self.flip_axes)) != len(self.flip_axes):
            raise ValueError(f"flip_axes: distinct axes out of (0, 1, 2) expected, got {flip_axes!r}")
        self.elastic_grid = None
        self.elastic_sigma_vox = float(elastic_sigma_vox)
        if elastic_grid is not None and self.elastic_sigma_vox > 0:
            g = tuple(int(v) for v in elastic_grid)
            if len(g) != 3 or min(g) < 2 or max(g) > MAX_GRID:
                raise ValueError(f"elastic_grid {elastic_grid!r}: three extents of 2..{MAX_GRID} control points")
            self.elastic_grid = g
        elif self.elastic_sigma_vox < 0:
            raise ValueError("elastic_sigma_vox must be >= 0")
        self.mri_scale = self._range(mri_scale, "mri_scale")
        self.mri_shift = self._range(mri_shift, "mri_shift")
        self.mri_gamma = self._range(mri_gamma, "mri_gamma", positive=True)
        self.noise_sigma = self._range(noise_sigma, "noise_sigma")
        if self.noise_sigma[0] < 0:
            raise ValueError("noise_sigma must be >= 0")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"p={p!r} is not a probability")
        self.p = float(p)
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.calls = 0
        self.last_params = None          # what the latest __call__ applied (params, disp): for logs and tests

    @staticmethod
    def _range(v, name, positive=False):
        lo, hi = (float(x) for x in v)
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi) or (positive and lo <= 0):
            raise ValueError(f"{name}={v!r}: a finite (lo, hi) range with lo <= hi{' and lo > 0' if positive else ''} expected")
        return lo, hi

    # -- sampling ---------------------------------------------------------------------------------------------------
    def sample_params(self, B, shape=(128, 128, 128)):
        """-> (params (B, 16) float32 numpy, disp (B, 3, gz, gy, gx) float32 numpy or None) for volumes of ``shape``."""
        rng = self.rng
        params = np.empty((B, NPARAM), dtype=np.float32)
        disp = None if self.elastic_grid is None else np.zeros((B, 3) + self.elastic_grid, dtype=np.float32)
        for b in range(B):
            on = rng.random() < self.p
            rot = rng.uniform(-self.rotate_deg, self.rotate_deg)
            sc = rng.uniform(self.scale[0], self.scale[1], 3)
            tr = rng.uniform(-self.translate_vox, self.translate_vox)
            flips = [False, False, False]
            for a in self.flip_axes:
                flips[a] = bool(rng.random() < 0.5)
            inten = [rng.uniform(*r) for r in (self.mri_scale, self.mri_shift, self.mri_gamma, self.noise_sigma)]
            d = None if disp is None else rng.normal(0.0, self.elastic_sigma_vox, (3,) + self.elastic_grid)
            if on:
                params[b] = pack_params(matrix(rot, sc, tr, flips, shape), *inten)
                if d is not None:
                    disp[b] = d
            else:
                params[b] = IDENTITY
        return params, disp

    @staticmethod
    def is_identity(params, disp=None):
        params = params.detach().cpu().numpy() if torch.is_tensor(params) else np.asarray(params)
        if disp is not None:
            disp = disp.detach().cpu().numpy() if torch.is_tensor(disp) else np.asarray(disp)
            if np.any(disp != 0):
                return False
        return bool(np.all(params == IDENTITY[None]))

    # -- application ------------------------------------------------------------------------------------------------
    def __call__(self, mri, tau, roi, params=None, disp=None, out=None):
        """Augment one batch.  mri / tau / roi: fp32 device tensors in the shapes the training step takes ((B, 1, D, H, W), or
        (1, D, H, W) from the Prefetcher): the last three dimensions of ``mri`` are the volume, everything in front is the
        batch.  params / disp: apply THIS transform (see ``sample_params`` / ``pack_params``) instead of drawing one.
        out: (mri, tau, roi) buffers to write into (e.g. a GraphedTrainStep's static ``batch`` tensors).
        Returns (mri, tau, roi) in the input shapes.  A batch whose parameters are all the identity launches no kernel and
        returns its inputs (copied into ``out`` when that is given)."""
        if not torch.is_tensor(mri) or mri.dim() < 3:
            raise ValueError("augment: volumes of at least three dimensions expected")
        D, H, W = (int(s) for s in mri.shape[-3:])
        B = mri.numel() // max(D * H * W, 1)
        if params is None:
            params, disp = self.sample_params(B, (D, H, W))
        self.last_params = (params, disp)
        n = self.calls
        self.calls += 1
        if not torch.is_tensor(params) and self.is_identity(params, disp):
            if out is None:
                return mri, tau, roi
            for o, i in zip(out, (mri, tau, roi)):
                o.copy_(i.reshape(o.shape))
            return tuple(out)
        if disp is not None and not torch.is_tensor(disp) and not np.any(disp):
            disp = None
        seed = (self.seed * 0x9E3779B97F4A7C15 + n * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & _MASK64
        return warp(mri, tau, roi, params, disp, seed, out)

    # -- resumable state --------------------------------------------------------------------------------------------
    def state_dict(self):
        """The generator's position (plain ints / strings / dicts: loads under ``torch.load(weights_only=True)``)."""
        return {"seed": self.seed, "calls": self.calls, "bit_generator": _plain(self.rng.bit_generator.state)}

    def load_state_dict(self, state):
        self.seed, self.calls = int(state["seed"]), int(state["calls"])
        self.rng = np.random.default_rng(self.seed)
        self.rng.bit_generator.state = state["bit_generator"]


def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (np.integer,)):
        return int(o)
    return o


def as_augmenter(spec, rank=0):
    """train_dp's ``augment=``: an Augment3D is used as it is; a dict is its keyword arguments, with ``seed`` offset by the
    data-parallel rank so that the replicas draw different transforms."""
    if spec is None or isinstance(spec, Augment3D):
        return spec
    if isinstance(spec, dict):
        kw = dict(spec)
        kw["seed"] = int(kw.get("seed", 0)) + int(rank)
        return Augment3D(**kw)
    raise TypeError(f"augment= takes an Augment3D, a dict of its arguments or None, got {type(spec).__name__}")
