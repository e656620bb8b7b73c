"""The expert scatter (coma_weight_prep_bwd, 27 taps, E = 8, batch 2) per layer shape of the benched model, for a
rocprofv3 --kernel-trace run: every shape is ITERS launches in the order of SHAPES, so the trace splits by position.
COMA_WPREP_BWD_SPLIT=0 / 1 forces the serial / the expert-split form; profiles/wprep_bwd_table.py makes the table.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python profiles/microbench_wprep_bwd.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coma_unet_amd import ops  # noqa: E402

ITERS = 12
E, B = 8, 2
# (cin, cout, transposed), blocks of 256 pairs: 1 .. 1024
SHAPES = [(3, 16, False), (16, 16, False), (16, 32, False), (32, 32, False), (64, 32, False), (64, 64, False), (128, 64, False),
          (64, 128, True), (128, 128, False), (256, 128, False), (256, 256, False), (512, 512, False)]

if __name__ == "__main__":
    for cin, cout, tr in SHAPES:
        master = torch.randn((E, cin, cout, 3, 3, 3) if tr else (E, cout, cin, 3, 3, 3), device="cuda") * 0.05
        r = torch.rand((B, E), device="cuda")
        _, _, rr, meta = ops._prep_fwd(master, r, tr, torch.bfloat16, torch.bfloat16)
        dwk = torch.randn((B, 27, cout, cin), device="cuda")
        for _ in range(ITERS):
            ops._prep_bwd(dwk, master, rr, meta, None)
        torch.cuda.synchronize()
