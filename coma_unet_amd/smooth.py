"""Gaussian smoothing of the tau-PET target on the device (the reference's ``-smoothing`` flag).

What the reference computes (``validation.py:690`` / ``validation_combined_dataset.py:356`` -> ``smoothing=True`` ->
``VolumeDataset.py:138-140``): MONAI's ``GaussianSmooth()`` over the tau target of every sample, training and test sets alike,
after the 2 mm resample and ``nan_to_num`` and before the skull masking of the MRI.

* ``GaussianSmooth()`` defaults to ``sigma = 1.0``, ``approx = "erf"``; it builds
  ``GaussianFilter(img.ndim - 1, sigma, approx="erf", truncated=4.0)`` and applies it to ``img.unsqueeze(0)``.
* The 1-D taps (MONAI ``gaussian_1d``, NOT normalised): ``tail = int(max(sigma * truncated, 0.5) + 0.5)``,
  ``x = -tail .. tail``, ``t = 0.70710678 / |sigma|``, ``w = clamp(0.5 * (erf(t (x + 0.5)) - erf(t (x - 0.5))), min=0)``;
  for sigma = 1: 9 taps that sum to 0.99999320.
* ``separable_filtering`` correlates axis by axis with zero padding.
* Kept as upstream: the reference calls ``smoothing(tau_tensor.squeeze(0))`` on a ``(1, D, H, W)`` tensor.  MONAI is
  channel-first, so D becomes the channel axis and the filter is 2-D: every z-slice (dim 0 of the ``sitk.GetArrayFromImage``
  layout) is smoothed in-plane over (y, x), nothing along z.  ``GaussianSmooth3D.reference()`` is that preset.  (The dead helper
  ``monai_spatial_transforms``, ``VolumeDataset.py:301-307``, would have been the 3-D variant.)
* The unused nibabel loader (``data_util.py:109-110``) calls ``smooth_image(fwhm=2, mode='nearest')``: scipy's
  ``gaussian_filter`` with ``sigma_vox = fwhm / voxel_mm / sqrt(8 ln 2)`` per axis, radius ``int(4 sigma + 0.5)``, sampled
  taps normalised to 1, edge replication.  ``GaussianSmooth3D.from_fwhm`` is that preset.

Parity status: MONAI is not installed here, so the ``erf`` preset restates the formulas above and is "unpinned against MONAI
itself", as the resampler is against SimpleITK; the ``sampled`` mode is pinned against scipy (tests/test_smooth_cpu.py).

One kernel launch per call (``coma_gauss_smooth3d``, csrc/smooth.hip); the arithmetic contract is in include/coma_unet.h.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import lib, check, ptr

MAX_RADIUS = 8                     # COMA_SMOOTH_MAX_RADIUS
SMALL_RADIUS = 4                   # COMA_SMOOTH_SMALL_RADIUS
ZEROS, NEAREST = 0, 1
_BOUNDARY = {"zeros": ZEROS, "nearest": NEAREST}
_AXES = ("z", "y", "x")


def tile(radius=SMALL_RADIUS, z_filtered=True):
    """(tz, ty, tx): the tile of outputs one block owns in a launch whose largest radius is ``radius``."""
    t = [C.c_int32(), C.c_int32(), C.c_int32()]
    lib.coma_gauss_smooth3d_tile(int(radius), int(bool(z_filtered)), *(C.byref(v) for v in t))
    return tuple(int(v.value) for v in t)


TILE = tile()                      # (8, 8, 32): the largest tile; tests size their shapes from it
TILE_LARGE_RADIUS = tile(MAX_RADIUS, True)


def gaussian_taps(sigma, truncated=4.0, approx="erf"):
    """The 1-D taps as an fp64 numpy array.  ``"erf"``: MONAI's ``gaussian_1d(approx="erf")`` (not normalised);
    ``"sampled"``: scipy's ``_gaussian_kernel1d`` (radius int(truncated * sigma + 0.5), normalised to 1)."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be positive and finite, got {sigma!r}")
    truncated = float(truncated)
    if not (math.isfinite(truncated) and truncated > 0):
        raise ValueError(f"truncated must be positive and finite, got {truncated!r}")
    if approx == "erf":
        tail = int(max(sigma * truncated, 0.5) + 0.5)
        x = np.arange(-tail, tail + 1, dtype=np.float64)
        t = 0.70710678 / abs(sigma)
        w = np.array([0.5 * (math.erf(t * (v + 0.5)) - math.erf(t * (v - 0.5))) for v in x], dtype=np.float64)
        return np.clip(w, 0.0, None)
    if approx == "sampled":
        radius = int(truncated * sigma + 0.5)
        x = np.arange(-radius, radius + 1, dtype=np.float64)
        w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        return w / w.sum()
    raise ValueError(f"approx must be 'erf' or 'sampled', got {approx!r}")


def smooth(vol, taps_zyx, boundary=ZEROS, out=None):
    """The kernel as it is: ALWAYS one launch on the current stream.  vol: contiguous fp32 device tensor whose last three
    dimensions are (D, H, W), everything in front is the batch.  taps_zyx: per axis an array of fp32 weights or None."""
    D, H, W = (int(s) for s in vol.shape[-3:])
    B = vol.numel() // (D * H * W)
    if out is None:
        out = torch.empty_like(vol)
    t = [None if w is None else np.ascontiguousarray(w, dtype=np.float32) for w in taps_zyx]
    a = [(None, 0) if w is None else (w.ctypes.data, int(w.size)) for w in t]
    check(lib.coma_gauss_smooth3d(ptr(vol), ptr(out), B, D, H, W, a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1], int(boundary),
                                  None, 0, 0, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0, L.stream()), "coma_gauss_smooth3d")
    return out


class GaussianSmooth3D:
    """Separable Gaussian filter over the ``axes`` of fp32 device volumes, one kernel launch per call.

    sigma: a scalar or one value per entry of ``axes``, in voxels.  axes: a subset of ("z", "y", "x"); the others are
    left alone.  approx / truncated: see ``gaussian_taps``.  boundary: "zeros" (MONAI) or "nearest" (edge replication).
    The taps are computed once in fp64 and rounded once to fp32."""

    def __init__(self, sigma=1.0, axes=("y", "x"), approx="erf", boundary="zeros", truncated=4.0):
        axes = tuple(axes)
        if any(a not in _AXES for a in axes) or len(set(axes)) != len(axes):
            raise ValueError(f"axes: distinct entries out of {_AXES} expected, got {axes!r}")
        sig = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
        if sig.shape == (1,):
            sig = np.repeat(sig, len(axes))
        if sig.shape != (len(axes),):
            raise ValueError(f"sigma: a scalar or one value per axis of {axes!r} expected, got {sigma!r}")
        if boundary not in _BOUNDARY:
            raise ValueError(f"boundary must be one of {tuple(_BOUNDARY)}, got {boundary!r}")
        self.axes, self.approx, self.boundary, self.truncated = axes, approx, boundary, float(truncated)
        self.sigma = {a: float(s) for a, s in zip(axes, sig)}
        self.taps64 = {a: gaussian_taps(self.sigma[a], truncated, approx) for a in axes}
        for a, w in self.taps64.items():
            if w.size // 2 > MAX_RADIUS:
                raise ValueError(f"axis {a}: sigma {self.sigma[a]} at truncation {truncated} needs radius {w.size // 2} > {MAX_RADIUS}")
        self.taps = tuple(None if a not in axes else self.taps64[a].astype(np.float32) for a in _AXES)      # (z, y, x)

    @classmethod
    def reference(cls):
        """What the reference's ``-smoothing`` computes: sigma 1, erf taps, zero padding, in-plane (y, x) only."""
        return cls(sigma=1.0, axes=("y", "x"), approx="erf", boundary="zeros", truncated=4.0)

    @classmethod
    def from_fwhm(cls, fwhm_mm, spacing_xyz, boundary="nearest"):
        """The nibabel / scipy preset (``smooth_image(fwhm=...)``): all three axes, sampled taps normalised to 1."""
        sx, sy, sz = (float(v) for v in spacing_xyz)
        k = math.sqrt(8.0 * math.log(2.0))
        return cls(sigma=tuple(float(fwhm_mm) / s / k for s in (sz, sy, sx)), axes=_AXES, approx="sampled", boundary=boundary)

    @property
    def radius(self):
        return max((w.size // 2 for w in self.taps64.values()), default=0)

    @staticmethod
    def _volume(vol):
        if not torch.is_tensor(vol) or vol.dtype != torch.float32:
            raise ValueError(f"smooth: an fp32 tensor expected, got {getattr(vol, 'dtype', type(vol).__name__)}")
        if not vol.is_contiguous():
            raise ValueError(f"smooth: the volume must be contiguous, got strides {tuple(vol.stride())} for shape {tuple(vol.shape)}")
        ok = vol.dim() in (3, 4) or (vol.dim() == 5 and vol.shape[1] == 1)
        if not ok or vol.numel() == 0:
            raise ValueError(f"smooth: (D, H, W), (B, D, H, W) or (B, 1, D, H, W) expected, got {tuple(vol.shape)}")
        if not vol.is_cuda:
            raise ValueError("smooth: a device tensor expected (there is no CPU path)")
        return vol

    def __call__(self, vol, out=None):
        """vol: (D, H, W), (1, D, H, W), (B, D, H, W) or (B, 1, D, H, W) fp32 device tensor; returns the same shape."""
        self._volume(vol)
        if out is not None:
            if self._volume(out).shape != vol.shape or out.device != vol.device:
                raise ValueError(f"smooth: out has shape {tuple(out.shape)}, expected {tuple(vol.shape)}")
        return smooth(vol, self.taps, _BOUNDARY[self.boundary], out)

    def resampled(self, src, spacing_xyz, new_spacing, default_value=0.0, nan_to_num=True, size_xyz=None):
        """``self(resample_nearest(src, ...))`` in ONE launch, bit for bit, without the resampled volume: src is a raw
        (Z, Y, X) fp32 device volume; returns the smoothed (Zo, Yo, Xo) volume on the new grid."""
        from .input_pipeline import out_size
        self._volume(src)
        if src.dim() != 3:
            raise ValueError(f"smooth: a raw (Z, Y, X) volume expected, got {tuple(src.shape)}")
        Dz, Hy, Wx = (int(s) for s in src.shape)
        Wo, Ho, Do = size_xyz if size_xyz is not None else out_size((Wx, Hy, Dz), spacing_xyz, new_spacing)
        out = torch.empty((Do, Ho, Wo), dtype=torch.float32, device=src.device)
        a = [(None, 0) if w is None else (w.ctypes.data, int(w.size)) for w in self.taps]
        check(lib.coma_gauss_smooth3d(None, ptr(out), 1, Do, Ho, Wo, a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1],
                                      _BOUNDARY[self.boundary], ptr(src), Dz, Hy, Wx, float(spacing_xyz[2]), float(spacing_xyz[1]),
                                      float(spacing_xyz[0]), float(new_spacing[2]), float(new_spacing[1]), float(new_spacing[0]),
                                      float(default_value), int(bool(nan_to_num)), L.stream()), "coma_gauss_smooth3d")
        return out


def as_smoother(spec):
    """``smoothing=`` / ``smooth_tau=``: None stays None, True is the reference preset, a dict is GaussianSmooth3D's keyword
    arguments, an instance is used as it is."""
    if spec is None or isinstance(spec, GaussianSmooth3D):
        return spec
    if spec is True:
        return GaussianSmooth3D.reference()
    if isinstance(spec, dict):
        return GaussianSmooth3D(**spec)
    raise TypeError(f"smoothing takes None, True, a dict of GaussianSmooth3D's arguments or an instance, got {spec!r}")
