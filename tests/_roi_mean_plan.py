"""Shared by test_roi_mean_cpu.py, test_roi_mean_kernels_gpu.py and test_roi_mean_step_gpu.py: the fp64 restatement of the
ROI-mean loss, a plain-Python mirror of the launch arithmetic of csrc/roi_mean.hip, the cases / label patterns / tables, the
input construction, and the bounds counted from the kernel source.

The restatement is plain torch on whatever device its inputs live on and shares no code with the kernels.  It is written
literally: for each table slot a `roi == idx` mask and sum(mask * x) / count_nonzero(mask), as RoiCorrMetric.acc_roi_corr
does (attn_unet_data_parallel.py:49-60); a region without voxels is skipped, a later copy of a duplicated id owns no voxel,
and the gradient comes from autograd.
"""
import functools

import torch

from _roi_loss_plan import U_F32, U_BF16, U_F64, CASES, OTHER_LABELS, case_layout, cdiv, vec4_ok, vol  # noqa: F401

MSE, L1, HUBER = 0, 1, 2
KINDS = {"mse": MSE, "l1": L1, "huber": HUBER}
DELTA = 0.15                 # the huber cases' delta: the offsets below put regions on both sides of it
DELTA32 = float(torch.tensor(DELTA, dtype=torch.float32))   # what the C ABI's `float delta` holds: the restatement's default

# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic of csrc/roi_mean.hip (test_roi_mean_cpu.py searches the source for the constants)
# ---------------------------------------------------------------------------------------------------------------------
THREADS = 256
RM_BLOCKS = 512              # roi_mean_partial_k: one block per 256 * 8 voxels, capped
RM_PER_BLOCK = 256 * 8
RM_WAVE_VOX = 256            # voxels one wave handles per trip (4 per lane, on both paths)
RM_SLOTS = 64
RM_REC = 3 * RM_SLOTS        # doubles per block record
FIN_PARTS = 16               # roi_mean_finalize_k: 16 x 64 threads, part p adds records p, p + 16, ...
BWD_CAP = 8192


def fwd_blocks(V):
    return max(1, min(cdiv(V, RM_PER_BLOCK), RM_BLOCKS))


def ws_bytes(B):
    return B * RM_BLOCKS * RM_REC * 8


def fwd_trips(V):
    """Trips of the forward loop the busiest wave makes: a trip of the whole grid covers blocks * 4 waves * 256 voxels."""
    return cdiv(V, fwd_blocks(V) * 4 * RM_WAVE_VOX)


def bwd_blocks(V, vec):
    return max(1, min(cdiv(cdiv(V, 4) if vec else V, THREADS), BWD_CAP))


def finalize_trips(V):
    return cdiv(fwd_blocks(V), FIN_PARTS)


# ---------------------------------------------------------------------------------------------------------------------
# tables and label patterns
# ---------------------------------------------------------------------------------------------------------------------
TABLES = ("roi36", "randw", "one", "wide64")
PATTERNS = ("blocks", "random", "single", "none", "absent", "fractional")
NONE_LABELS = (0.0, 2.0, 3000.0, 4998.0)       # in no table below
BIG_ID, DUP_SLOT = 4999, 50                    # wide64: an id past the kernels' 4096-entry label table; slot 50 repeats slot 3's id

# (pattern, table) pairs every small case runs, and the ones the `cap` case runs
COMBOS = [("blocks", "roi36"), ("random", "roi36"), ("single", "roi36"), ("none", "roi36"), ("absent", "roi36"),
          ("fractional", "roi36"), ("blocks", "randw"), ("random", "randw"), ("absent", "randw"), ("random", "one"),
          ("single", "one"), ("none", "one"), ("blocks", "wide64"), ("random", "wide64"), ("fractional", "wide64")]
CAP_COMBOS = [("blocks", "roi36"), ("random", "wide64"), ("absent", "randw")]


def case_combos():
    """-> [(case, pattern, table)]"""
    out = []
    for c in CASES:
        out += [(c, p, t) for p, t in (CAP_COMBOS if c[0] == "cap" else COMBOS)]
    return out


def table(name):
    """-> ids (list of int), weights (fp64 tensor)"""
    from coma_unet_amd.roi_tables import ROI_INDICES
    if name == "roi36":
        return list(ROI_INDICES), torch.full((36,), 225.0, dtype=torch.float64)
    if name == "randw":
        g = torch.Generator().manual_seed(77)
        w = 0.5 + 300.0 * torch.rand(36, generator=g, dtype=torch.float64)
        w[4], w[30] = 0.0, 0.0
        return list(ROI_INDICES), w
    if name == "one":
        return [ROI_INDICES[5]], torch.tensor([2.5], dtype=torch.float64)
    assert name == "wide64"
    ids = list(ROI_INDICES) + [BIG_ID] + [3 + i for i in range(27)]          # 36 + 1 + 27 = 64; 3..29 holds 17 and 18 again
    ids[DUP_SLOT] = ids[3]
    g = torch.Generator().manual_seed(78)
    return ids, 1.0 + 9.0 * torch.rand(64, generator=g, dtype=torch.float64)


def slot_volume(roi, ids):
    """slot of every voxel by roi_lut_slot's rules: exact label values only, the first occurrence of an id wins; -1: none."""
    slot = torch.full(roi.shape, -1, dtype=torch.int64, device=roi.device)
    for r in reversed(range(len(ids))):
        slot[roi == float(ids[r])] = r
    return slot


def _labels(pattern, dims, B, ids, gen, blocks_roi):
    from coma_unet_amd.roi_tables import ROI_INDICES
    shape = (B,) + tuple(dims)
    pool36 = [float(i) for i in ROI_INDICES]
    draw = lambda pool: torch.tensor(pool, dtype=torch.float32)[torch.randint(0, len(pool), shape, generator=gen)]
    if pattern == "blocks":
        return blocks_roi.clone()
    if pattern == "random":
        return draw(pool36 + [float(i) for i in OTHER_LABELS])
    if pattern == "single":
        return torch.full(shape, float(ids[0]), dtype=torch.float32)
    if pattern == "none":
        return draw(list(NONE_LABELS))
    if pattern == "absent":                    # every third id of the 36 never occurs ...
        gone = pool36[2::3]
        lab = draw([v for v in pool36 if v not in gone] + [float(i) for i in OTHER_LABELS])
        lab[1].view(-1)[vol(dims) // 2] = gone[1]          # ... but for ONE voxel of sample 1: a region of exactly one voxel
        return lab
    assert pattern == "fractional"
    lab = draw(pool36 + [float(i) for i in OTHER_LABELS])
    half = torch.rand(shape, generator=gen) < 0.15
    return torch.where(half, lab + 0.5, lab)


@functools.lru_cache(maxsize=4)
def _batch(dims, B):
    from coma_unet_amd.synthetic import make_batch
    b = make_batch(B, dims, seed=101)
    return b["tau"][:, 0].double(), b["roi"][:, 0].clone()


@functools.lru_cache(maxsize=8)
def make_inputs(case, pattern, tab):
    """-> pred, gt (fp64), roi (fp32), each (B, D, H, W, 1) on the CPU, ids, weights (fp64); shared, never modified.
    gt is make_batch's tau; pred = gt + o_{b, r(v)} + 0.05 noise with |o| in [0.05, 0.11] or [0.19, 0.3], a random sign, and
    noise uniform in [-0.5, 0.5): every present region has 0.025 <= |d_r| <= 0.135 or 0.165 <= |d_r| before the inputs are
    rounded, so neither the "l1" sign nor the huber branch (delta 0.15) can flip under rounding.  (A voxel in no region gets
    no offset.)"""
    name, dims, B, _ = case
    ids, w = table(tab)
    gen = torch.Generator().manual_seed(1000 * PATTERNS.index(pattern) + 10 * TABLES.index(tab) + len(name))
    gt, blocks_roi = _batch(tuple(dims), B)
    lab = _labels(pattern, dims, B, ids, gen, blocks_roi)
    slot = slot_volume(lab, ids)
    n = len(ids)
    u = torch.rand((B, n), generator=gen, dtype=torch.float64)
    mag = torch.where(u < 0.5, 0.05 + 0.12 * u, 0.19 + 0.22 * (u - 0.5))
    sign = torch.where(torch.rand((B, n), generator=gen) < 0.5, -1.0, 1.0).double()
    o = torch.cat([mag * sign, torch.zeros(B, 1, dtype=torch.float64)], dim=1)          # column n: "no region"
    off = torch.gather(o, 1, torch.where(slot >= 0, slot, n).reshape(B, -1)).reshape(slot.shape)
    noise = torch.rand(slot.shape, generator=gen, dtype=torch.float64) - 0.5
    pred = gt + off + 0.05 * noise
    return pred.unsqueeze(-1), gt.unsqueeze(-1), lab.unsqueeze(-1), ids, w


# ---------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def _flat(t):
    return t.double().reshape(t.shape[0], -1)


def region_sums64(pred, gt, roi, ids):
    """-> count, sum pred, sum gt: (B, n_roi) fp64 each; differentiable in `pred`."""
    p, g, r = _flat(pred), _flat(gt), roi.reshape(roi.shape[0], -1)
    cnt, sp, sg, seen = [], [], [], set()
    for idx in ids:
        mask = (r == idx).double() if idx not in seen else torch.zeros_like(p)
        seen.add(idx)
        cnt.append(torch.count_nonzero(mask, dim=1).double())
        sp.append(torch.sum(mask * p, dim=1))
        sg.append(torch.sum(mask * g, dim=1))
    return torch.stack(cnt, 1), torch.stack(sp, 1), torch.stack(sg, 1)


def region_means64(pred, gt, roi, ids):
    """-> count, mean pred, mean gt: (B, n_roi) fp64 each (means 0 where count is 0); differentiable in `pred`."""
    cnt, sp, sg = region_sums64(pred, gt, roi, ids)
    safe = torch.where(cnt > 0, cnt, torch.ones_like(cnt))
    return cnt, sp / safe, sg / safe


def phi64(kind, pm, gm, delta):
    if kind == MSE:
        return torch.square(pm - gm)
    if kind == L1:
        return torch.abs(pm - gm)
    return torch.nn.functional.huber_loss(pm, gm, reduction="none", delta=delta)


def loss64(kind, pred, gt, roi, ids, w, delta=DELTA32):
    """per-sample loss (B,) in fp64, differentiable in `pred`: absent regions skipped; 0 where nothing is present."""
    cnt, pm, gm = region_means64(pred, gt, roi, ids)
    here = (cnt > 0).double()
    wd = w.double().to(cnt.device).view(1, -1) * here
    num = torch.sum(wd * phi64(kind, pm, gm, delta), dim=1)
    den = torch.sum(wd, dim=1)
    live = den != 0
    return torch.where(live, num / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(num))


def loss_coef_grad64(kind, pred, gt, roi, ids, w, gout, delta=DELTA32):
    """-> loss (B,), coef (B, n_roi) by the closed form w phi'(d) / (n sum w), d (sum_b gout_b loss_b) / d pred by AUTOGRAD on
    the restatement, and (count, d) per region."""
    p = pred.detach().double().clone().requires_grad_(True)
    l = loss64(kind, p, gt, roi, ids, w, delta)
    (l * gout.double().reshape(-1)).sum().backward()
    cnt, pm, gm = region_means64(pred.detach(), gt, roi, ids)
    d = pm - gm
    here = cnt > 0
    wd = w.double().to(cnt.device).view(1, -1) * here
    den = wd.sum(1, keepdim=True)
    if kind == MSE:
        dphi = 2.0 * d
    elif kind == L1:
        dphi = torch.sign(d)
    else:
        dphi = torch.where(d.abs() < delta, d, delta * torch.sign(d))
    coef = torch.where(here & (den != 0), wd * dphi / (torch.where(here, cnt, torch.ones_like(cnt)) * torch.where(den != 0, den, torch.ones_like(den))),
                       torch.zeros_like(d))
    return l.detach(), coef, p.grad, (cnt, torch.where(here, d, torch.zeros_like(d)))


def closed_grad64(coef, gout, roi, ids):
    """the backward kernel's closed form: gout_b coef[b][slot] per voxel, 0 in no region"""
    B, n = coef.shape
    slot = slot_volume(roi, ids).reshape(B, -1)
    c = torch.cat([coef * gout.double().view(B, 1), torch.zeros(B, 1, dtype=torch.float64, device=coef.device)], dim=1)
    return torch.gather(c, 1, torch.where(slot >= 0, slot, n)).reshape(roi.shape)


def amplification(pred, gt, roi, ids):
    """max over present regions of (|mean pred| + |mean gt|) / |d|: what the fp64 roundings of the two means are amplified
    by in d = mean pred - mean gt (1 when nothing is present)."""
    cnt, pm, gm = region_means64(pred, gt, roi, ids)
    here = cnt > 0
    a = torch.where(here, (pm.abs() + gm.abs()) / torch.where(here, (pm - gm).abs(), torch.ones_like(pm)), torch.ones_like(pm))
    return float(a.max())


# ---------------------------------------------------------------------------------------------------------------------
# bounds, counted from csrc/roi_mean.hip.  Every sum, the means, d, phi, the weighted sums and the quotients are fp64; pred /
# gt convert to double exactly.  The longest chain of additions behind a region sum (sum_chain): 3 (a lane's 4 voxels) + 6
# (the segmented scan) + the run sums a wave's owner lane adds, at most one per voxel of its trips + 3 (waves) + records / 16
# (part) + 15 (parts); additions of an exact zero are exact, so a sum of n values never takes more than n - 1 inexact ones.
# Each is within 2^-53 of the L1 mass so far; REF_CHAIN more are allowed for the restatement's own torch.sum.
# d = mean pred - mean gt amplifies the two means' errors by amp = (|mean pred| + |mean gt|) / |d| (P.amplification, from the
# restatement); phi = d^2 doubles that.  The weighted sums over <= 64 slots and the quotients add 64 + 10 roundings of
# non-negative terms (weights >= 0).
#   loss   one cast to fp32: 2^-24 (taken twice, as the existing ROI-loss tests do: 2 u) + the fp64 terms
#   coef   w phi'(d) / (n sum w): the same fp64 terms, one cast: 2 u
#   dpred  gout * coef in fp32: the stored coef (1) and the product (1) -> within 4 u; bf16 adds the store's rounding
#   stats  the sums themselves: held to V 2^-53 relative to the value, the figure the kernels were specified with.  For the
#          cases past one block sum_chain + REF_CHAIN <= V (test_roi_mean_cpu.py asserts it); for the 210-voxel cases the
#          worst-case count is 209 + REF_CHAIN > V, so there the check asks for more than the count guarantees on adversarial
#          data.  (Measured: 0 -- sums of a few thousand fp32 values of one magnitude are exact in fp64.)
# ---------------------------------------------------------------------------------------------------------------------
LOSS_REL = 1e-6              # ceilings that must hold besides the counted bounds
K_CAST = 2                   # 2 u for the one fp32 cast of loss / coef
K_GRAD = 4
REF_CHAIN = 32
AMP_MAX = 400.0              # the amplification the ceilings are checked at; the inputs stay under it (CPU test)


def sum_chain(V):
    return min(3 + 6 + min(V, fwd_trips(V) * RM_WAVE_VOX) + 3 + finalize_trips(V) + FIN_PARTS - 1, V - 1)


def f64_terms(V, amp):
    return ((sum_chain(V) + REF_CHAIN) * 2.0 * (1.0 + amp) + 74) * U_F64


def scalar_bound(V, amp):
    """relative bound of loss[b] and of a non-zero coef[b][r]"""
    return K_CAST * U_F32 + f64_terms(V, amp)


def grad_bound(V, amp, dtype):
    return (U_BF16 if dtype == torch.bfloat16 else 0.0) + K_GRAD * U_F32 + f64_terms(V, amp)


def stats_bound(V):
    return V * U_F64
