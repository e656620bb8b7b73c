"""Generates tests/golden/roi_losses_ref.npz from the REFERENCE's own criterions.py (not collected by pytest).

    python tests/make_roi_loss_golden.py <directory of the reference checkout>

The reference file is imported at run time, as oracle/make_golden.py does: two empty stand-in modules named `data_util`
and `VolumeDataset` go into sys.modules first (the file uses them only in code that is not exercised), and `roi` is handed
over as a torch.Tensor subclass whose get_device() answers "cpu", which lets the UNMODIFIED RoiRSE.forward
(`torch.ones(..., device=roi.get_device())`) run on the CPU.  Nothing of the reference's text is copied.

Contents, for B = 1, 2, 3 at (B, 1, 5, 6, 7) in fp64 (inputs from _roi_loss_plan.golden_inputs: multiples of 1/64 in
[0, 4), exactly representable in bf16; labels from the 36 ROI ids, 0, 2 and 4999; weights 225 / 100 / 7.5):
  in{B}_pred, in{B}_gt, in{B}_roi, weights, roi_ids
  {rse,rrmse}{B}_{mean,sum}            the reference class's loss for reduction "mean" / "sum"
  {rse,rrmse}{B}_grad_{mean,sum}       d loss / d pred
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _roi_loss_plan as P  # noqa: E402
from coma_unet_amd.roi_tables import ROI_INDICES  # noqa: E402


def import_reference_criterions(ref_dir):
    for name in ("data_util", "VolumeDataset"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, ref_dir)
    import criterions as ref  # noqa: the reference's own file
    sys.path.pop(0)
    return ref


class CpuRoi(torch.Tensor):
    def get_device(self):
        return "cpu"


def main(ref_dir):
    ref = import_reference_criterions(ref_dir)
    w = P.mixed_weights(len(ROI_INDICES))
    out = dict(weights=w.numpy(), roi_ids=np.asarray(ROI_INDICES, dtype=np.int32))
    for B in P.GOLDEN_B:
        pred, gt, roi = P.golden_inputs(B, ROI_INDICES)
        out.update({f"in{B}_pred": pred.numpy(), f"in{B}_gt": gt.numpy(), f"in{B}_roi": roi.numpy()})
        for name, cls, kind in (("rse", ref.RoiRSE, P.RSE), ("rrmse", ref.RoiRRMSE, P.RRMSE)):
            for red in ("mean", "sum"):
                p = pred.clone().requires_grad_(True)
                loss = cls(w, ROI_INDICES, reduction=red)(p, gt, roi.as_subclass(CpuRoi))
                loss.backward()
                out[f"{name}{B}_{red}"] = np.asarray(float(loss))
                out[f"{name}{B}_grad_{red}"] = p.grad.numpy()
                mine = P.loss64(kind, pred, gt, roi, ROI_INDICES, w)
                mine = mine.mean() if red == "mean" else mine.sum()
                print(f"{name} B={B} {red}: reference {float(loss):.17g}  restatement {float(mine):.17g}")
    path = os.path.join(HERE, "golden", "roi_losses_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
