"""Shared by test_nonconv_sizes_gpu.py and test_nonconv_sizes_cpu.py: plain-Python mirrors of the launch arithmetic of the
streaming kernels (csrc/elementwise.hip, metrics.hip, norm.hip, norm_common.h, gate.hip), the shapes at which each kernel
is run past one block / one chunk / one pass of its grid-stride loop, and fp64 restatements of the operations.

The restatements are plain torch on whatever device the inputs live on and share no code with the kernels; the CPU module
checks each of them against an independent source (torch.optim.AdamW, torch.nn.functional, the oracles, the golden file).
"""
import numpy as np
import torch

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
U_F64 = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic (the constants are searched for in the .hip sources by test_nonconv_sizes_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
THREADS = 256
EW_CAP = 8192              # ew_grid (elementwise.hip), resample_nn_k's grid (metrics.hip)
LOSS_BLOCKS = 512          # loss_partial_k: one block per 256 * 8 voxels, capped
LOSS_PER_BLOCK = 256 * 8
LOSS_FINALIZE_LANES = 64   # loss_finalize_k / colsum_finalize_k: k += 64
EVAL_CAP = 1024            # eval_stats_k: one block per 256 * 16 voxels, capped
EVAL_PER_BLOCK = 256 * 16
ZERO_GX, ZERO_GY = 64, 1024
ROWS_CAP = 1024            # make_rows: at most 1024 / G chunks of rows
ROWS_PER_STEP = 16         # make_rows: a chunk is at least 16 steps of ry rows
NORM_BLOCKS = 4096         # ew_blocks (norm.hip): COMA_NORM_BLOCKS default
NORM_UNR = 4
GATE_MID_CAP = 1024        # gate_mid_fwd_k / gate_apply_bwd_k: 1024 / B blocks of 2 * (256 / cv) voxels
GATE_APPLY_CAP = 4096      # gate_apply_fwd_k (4 items per thread), gate_mid_bwd_apply_k (2 items per thread)

EW_PASS = EW_CAP * THREADS                  # elements one pass of an ew_grid launch covers: 2 097 152


def cdiv(a, b):
    return -(-a // b)


def ew_grid(total):
    return max(1, min(cdiv(total, THREADS), EW_CAP))


def passes(total, blocks, per_block=THREADS):
    """Trips of the grid-stride loop the busiest thread makes."""
    return cdiv(total, blocks * per_block)


def loss_blocks(V):
    return max(1, min(cdiv(V, LOSS_PER_BLOCK), LOSS_BLOCKS))


def eval_blocks(V):
    return max(1, min(cdiv(V, EVAL_PER_BLOCK), EVAL_CAP))


def zero_grid(n, max_len):
    return max(1, min(cdiv(max_len, THREADS), ZERO_GX)), min(n, ZERO_GY)


def make_rows(R_, C, G, vec):
    """make_rows of norm_common.h -> dict(cv, cvp, ry, nchunks, ch)."""
    cv = C // vec
    cvp = 1
    while cvp < cv:
        cvp <<= 1
    cvp = min(cvp, 256)
    ry = 256 // cvp
    nch = max(1, min(cdiv(R_, ry * ROWS_PER_STEP), max(1, ROWS_CAP // G)))
    return dict(cv=cv, cvp=cvp, ry=ry, nchunks=nch, ch=cdiv(R_, nch))


def ew_blocks(total, per_thread):
    return max(1, min(cdiv(total, THREADS * per_thread), NORM_BLOCKS))


def apply_blocks(total, cv, per_thread):
    nb = ew_blocks(total, per_thread)
    if 0 < cv <= 256 and 256 % cv == 0:
        return nb
    while nb > 1 and (nb * 256) % cv != 0:
        nb -= 1
    return nb


def gate_blocks(items, per_block, cap):
    return max(1, min(cdiv(items, per_block), cap))


def vol(dims):
    return dims[0] * dims[1] * dims[2]


# ---------------------------------------------------------------------------------------------------------------------
# the cases (smallest shapes that cross each boundary; test_nonconv_sizes_cpu.py asserts that they do)
# ---------------------------------------------------------------------------------------------------------------------
# ew3_k: (name, dims, C, channels of the wider output buffer, channel offset of the slice, vector width)
EW3_CASES = [("vec4", (63, 65, 65), 32, 36, 0, 4), ("vec1", (41, 41, 41), 32, 34, 1, 1)]
# gate_mul_*_k: (name, dims, C, wider buffer, offset, vec)
GATE_MUL_CASES = [("c256", (31, 33, 33), 256, 260, 0, 4), ("c32", (63, 65, 65), 32, 36, 0, 4),
                  ("c32_even", (64, 64, 65), 32, 32, 0, 4), ("c32_vec1", (41, 41, 41), 32, 34, 1, 1)]
# cast_copy_k / batch_sum_k: (name, dims, C)
CAST_CASES = [("c1", (128, 128, 129), 1), ("c3", (89, 89, 89), 3)]
BATCH_SUM_B = 3
# roi paint / losses: (name, dims, B)
LOSS_CASES = [("mid", (32, 33, 35), 3), ("big", (128, 128, 129), 3)]
# eval_stats_k: (name, dims, B)
EVAL_CASES = [("blocks", (27, 28, 29), 3), ("cap", (128, 128, 257), 1)]
# adamw_k: (name, n, element offset of the slices into 16-byte aligned buffers)
ADAMW_CASES = [("vec4", 8389635, 0), ("scalar", 2098179, 1)]
ADAMW_HP = (1e-3, 0.9, 0.999, 1e-8, 1e-2)       # lr, beta1, beta2, eps, weight decay
# NormAct / GateFused over the apply caps: (dims, B, C[, F])
NORM_BIG = ((81, 81, 81), 1, 32)
GATE_BIG = [("vec4", (81, 81, 81), 1, 32, 16, 4), ("vec1", (51, 51, 51), 1, 32, 16, 1)]
# resample_nn_k: the case added to tests/test_input_pipeline.py (input shape, spacing) -> 130 x 128 x 128 outputs
RESAMPLE_CASE = ((65, 64, 64), (4.0, 4.0, 4.0))

NORM_ACTS = ["none", "relu", "prelu", "leaky", "sigmoid", "prelu_relu"]      # (L.ACT_* codes)


def norm_f32_vec(C, ld):
    return 4 if (C % 4 == 0 and ld % 4 == 0) else 1


def norm_f32_rows(batch=2):
    """fp32 twins of _synthetic_norm_rows (test_production_shapes_gpu.py): per (C, mode) 5 chunks with the last one 3 rows
    short, and past the 1024 / G cap with a ragged last chunk.  -> (V, C, ld, mode, act, affine, rows per group)."""
    out = []
    acts = ["prelu", "relu", "leaky", "sigmoid", "prelu_relu", "none", "prelu"]
    for i, C in enumerate((1, 3, 16, 32, 96)):
        ld = C if C % 4 == 0 else (C + 7) // 8 * 8
        vec = norm_f32_vec(C, ld)
        for mode, G in (("batch", 1), ("instance", batch)):
            per = make_rows(1, C, G, vec)["ry"] * ROWS_PER_STEP
            cap = max(1, ROWS_CAP // G)
            for Rg in (5 * per - 3, cap * (per + 4) - 3):
                V = Rg if G == batch else cdiv(Rg, batch)
                act = acts[(i + len(out)) % len(acts)]
                out.append((V, C, ld, mode, act, mode == "batch", V if G == batch else V * batch))
    return out


def colsum_rows(batch=2):
    """spatial mean (instance rows) and conv bias gradient (batch or per-sample rows): more than 64 chunks below the cap
    with a ragged last chunk, and past the 1024 / G cap.  -> (what, dtype, C, ld, V)."""
    out = []
    for dt in ("f32", "bf16"):
        for C, ld in ((5, 8), (32, 40)):
            vec = (8 if dt == "bf16" else 4) if C % 8 == 0 else 1
            for what, G in (("mean", batch), ("bias", 1), ("bias_ps", batch)):
                per = make_rows(1, C, G, vec)["ry"] * ROWS_PER_STEP
                cap = max(1, ROWS_CAP // G)
                for Rg in (70 * per - 3, cap * (per + 4) - 3):
                    out.append((what, dt, C, ld, Rg if G == batch else cdiv(Rg, batch)))
    return out


def zero_ranges_table(seed=0):
    """1100 ranges (more than grid y) over a flat buffer: gaps of 1..3 sentinel cells between them, zero-length ranges, odd
    offsets, and one range longer than one pass of grid x (64 * 256).  -> (int64 table [n, 2], buffer length, longest)."""
    rng = np.random.default_rng(seed)
    rows, off = [], 3
    for i in range(1100):
        ln = 50001 if i == 7 else (0 if i % 9 == 0 else int(rng.integers(1, 41)))
        rows.append((off, ln))
        off += ln + int(rng.integers(1, 4))
    tab = torch.tensor(rows, dtype=torch.int64)
    return tab, off + 5, int(tab[:, 1].max())


# ---------------------------------------------------------------------------------------------------------------------
# fp64 restatements
# ---------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def adamw_init(p0):
    """state of adamw_step: p, m, v and the running error bounds of each."""
    z = lambda: torch.zeros_like(p0, dtype=torch.float64)
    return dict(p=p0.double().clone(), m=z(), v=z(), bp=z(), bm=z(), bv=z())


def adamw_bias_terms(b1, b2, t, pow_ulps=2.0):
    """bias corrections in double and the relative error of the kernel's fp32 versions.
    The kernel forms bc = 1 - powf(beta, t): powf is within `pow_ulps` ulp (one ulp <= 2 u |value|), the subtraction rounds
    once -- an absolute error that the small 1 - beta^t divides: eps(bc) = pow_ulps 2 u beta^t / (1 - beta^t) + u.
    -> (bc1, bc2, eps(bc1), eps(sqrt(bc2)))."""
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    e1 = pow_ulps * 2 * U_F32 * b1 ** t / bc1 + U_F32
    e2 = 0.5 * (pow_ulps * 2 * U_F32 * b2 ** t / bc2 + U_F32) + U_F32           # sqrtf: half the relative error + its rounding
    return bc1, bc2, e1, e2


def adamw_step(st, g, t, hp=ADAMW_HP):
    """One AdamW step (torch.optim.AdamW: decoupled decay, bias-corrected, eps outside sqrt(v_hat)) in fp64 with the
    float32-rounded hyper-parameters, in place on `st`; the bounds bp / bm / bv follow the recurrence of the errors of
    adamw_k's fp32 arithmetic (u = 2^-24 per rounding, counted from the source: adamw_body in csrc/elementwise.hip):
      m = b1 m + (1 - b1) g ............ 4 roundings over the mass b1 |m| + (1 - b1) |g|, the old error shrinks by b1
      v = b2 v + (1 - b2) g g .......... 5 roundings, all terms positive
      denom = sqrtf(v) / bc2s + eps .... sqrtf, division, sum: 3 roundings, + half of v's relative error, + eps(bc2s)
      s = (lr / bc1) (m / denom) ....... 3 roundings + eps(bc1) + m's and denom's errors
      p = p (1 - lr wd) - s ............ 3 roundings relative to |p| (the decay factor's two, the product), 1 of the result
    -> dict of the step's terms for the report: the share of the bias-correction term in the bound of the update."""
    lr, b1, b2, eps, wd = (f32(x) for x in hp)
    u = U_F32
    g = g.double()
    p, m, v = st["p"], st["m"], st["v"]
    st["bm"] = b1 * st["bm"] + 2 * 4 * u * (b1 * m.abs() + (1 - b1) * g.abs())
    m.mul_(b1).add_((1 - b1) * g)
    st["bv"] = b2 * st["bv"] + 2 * 5 * u * (b2 * v + (1 - b2) * g * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    bc1, bc2, e1, e2 = adamw_bias_terms(b1, b2, t)
    root = v.sqrt() / bc2 ** 0.5
    denom = root + eps
    rel_v = st["bv"] / (2 * v).clamp_min(1e-300)
    b_denom = root * (rel_v + 2 * u) + u * denom
    s = (lr / bc1) * m / denom
    b_s = (lr / bc1) * st["bm"] / denom + s.abs() * (b_denom / denom + 3 * u)
    b_bias = s.abs() * (e1 + root * e2 / denom)                     # the 1 - powf(beta, t) terms alone
    st["bp"] = st["bp"] + 3 * u * p.abs() + b_s + b_bias
    p.mul_(1 - lr * wd).sub_(s)
    st["bp"] = st["bp"] + u * p.abs()
    return dict(bias_share=float((b_bias / st["bp"].clamp_min(1e-300)).max()), e_bc1=e1, e_bc2s=e2)


def roi_slots(roi, ids):
    """slot of every label of `roi` in the id list (first occurrence wins), -1 where it is none of them."""
    slot = torch.full(roi.shape, -1, dtype=torch.int64, device=roi.device)
    for i in reversed(range(len(ids))):
        slot[roi == float(ids[i])] = i
    return slot


def paint_ref(roi, x, prior, ids, abeta, pos, neg):
    """cat((selected prompt, saliency, suvr)) of the ROI painting: roi, x (B, D, H, W, 1), prior (B, n, 2) {suvr, saliency},
    pos / neg (D, H, W).  -> (B, D, H, W, 3) in the precision of the inputs (the values are copied, never computed)."""
    B = roi.shape[0]
    slot = roi_slots(roi[..., 0], ids)
    live = (slot >= 0) & ~(x[..., 0].float() < f32(1e-4))
    pr = prior.to(pos.dtype)
    b_idx = torch.arange(B, device=roi.device).view(B, 1, 1, 1).expand_as(slot)
    zero = torch.zeros((), dtype=pos.dtype, device=roi.device)
    suvr = torch.where(live, pr[b_idx, slot.clamp_min(0), 0], zero)
    sal = torch.where(live, pr[b_idx, slot.clamp_min(0), 1], zero)
    prompt = torch.stack([pos if float(abeta[b]) == 1.0 else neg for b in range(B)])
    return torch.stack((prompt, sal, suvr), dim=-1)


def roi_mse_ref(pred, gt, roi, ids, w):
    """per-sample loss mean(mask) * mean((pred - gt)^2) with mask = w[slot] on the ROI voxels, in fp64 (B, D, H, W, 1 inputs).
    -> loss (B,), mask_mean (B,), mean (pred - gt)^2 (B,)."""
    slot = roi_slots(roi[..., 0], ids)
    mask = torch.where(slot >= 0, w.double()[slot.clamp_min(0)], torch.zeros((), dtype=torch.float64, device=roi.device))
    mm = mask.mean(dim=(1, 2, 3))
    ms = ((pred.double() - gt.double()) ** 2)[..., 0].mean(dim=(1, 2, 3))
    return mm * ms, mm, ms


def eval_stats_ref(pred, gt, roi, ids):
    """(B, n + 1, 8) table of coma_eval_stats in fp64 and the L1 mass of the terms of every entry (for the bound).
    k: 0 count, 1 sum |d|, 2 sum d^2, 3 sum g, 4 sum g^2, 5 sum p, 6 sum |d / g| over the non-NaN entries, 7 their count;
    the last bin is the whole volume, whose slots 6 / 7 take |(g - p) / g| where |g| > 1e-8."""
    p, g = pred.double()[..., 0], gt.double()[..., 0]
    B, n = p.shape[0], len(ids)
    d = p - g
    slot = roi_slots(roi[..., 0], ids)
    r = (d / g).abs()
    ok = ~torch.isnan(r)
    r0 = torch.where(ok, r, torch.zeros_like(r))
    okg = g.abs() > float(np.float32(1e-8))
    rg = torch.where(okg, ((g - p) / torch.where(okg, g, torch.ones_like(g))).abs(), torch.zeros_like(g))
    one = torch.ones_like(d)
    terms = [one, d.abs(), d * d, g, g * g, p, r0, ok.double()]
    gterms = terms[:6] + [rg, okg.double()]
    out = torch.zeros((B, n + 1, 8), dtype=torch.float64, device=p.device)
    mass = torch.zeros_like(out)
    flat = slot.reshape(B, -1)
    bins = torch.arange(n, device=p.device)
    T = torch.stack([t.reshape(B, -1) for t in terms], 1)                 # (B, 8, N)
    big = torch.isinf(T)
    Tf = torch.where(big, torch.zeros_like(T), T)                        # (an inf term makes its bin inf: counted apart)
    for c0 in range(0, flat.shape[1], 1 << 18):                          # one-hot products in chunks: no contended scatter
        hot = (flat[:, c0:c0 + (1 << 18), None] == bins).double()        # (B, chunk, n); slot -1 is in no bin
        out[:, :n] += torch.matmul(Tf[:, :, c0:c0 + (1 << 18)], hot).transpose(1, 2)
        mass[:, :n] += torch.matmul(Tf[:, :, c0:c0 + (1 << 18)].abs(), hot).transpose(1, 2)
        ninf = torch.matmul(big[:, :, c0:c0 + (1 << 18)].double(), hot).transpose(1, 2)
        out[:, :n] = torch.where(ninf > 0, torch.full_like(ninf, float("inf")), out[:, :n])
    mass[:, :n] = torch.where(torch.isinf(out[:, :n]), out[:, :n], mass[:, :n])
    for k in range(8):
        out[:, n, k] = gterms[k].reshape(B, -1).sum(1)
        mass[:, n, k] = gterms[k].reshape(B, -1).abs().sum(1)
    return out, mass


def act64(z, act, a):
    """-> (act(z), d act / dz, d act / d slope, jump of d act / dz at z = 0)."""
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    pos = z > 0
    if act == "none":
        return z, one, zero, 0.0
    if act == "relu":
        return torch.where(pos, z, zero), pos.double(), zero, 1.0
    if act == "prelu":
        return torch.where(pos, z, a * z), torch.where(pos, one, a * one), torch.where(pos, zero, z), abs(1.0 - a)
    if act == "leaky":
        return torch.where(pos, z, 0.01 * z), torch.where(pos, one, 0.01 * one), zero, 0.99
    if act == "sigmoid":
        s = torch.sigmoid(z)
        return s, s * (1 - s), zero, 0.0
    if act == "prelu_relu":
        live = (~pos) & (a * z > 0)
        y = torch.where(pos, z, torch.where(live, a * z, zero))
        return y, torch.where(pos, one, torch.where(live, a * one, zero)), torch.where(live, z, zero), max(1.0, abs(a))
    raise ValueError(act)


def norm_act64(x, dy, mode, act, gamma=None, beta=None, slope=None, eps=1e-5, momentum=0.1):
    """BatchNorm3d(train) / InstanceNorm3d + activation on channels-last x (B, D, H, W, C), forward and backward written out
    in fp64 (no autograd).  -> dict(y, dx, dgamma, dbeta, dslope, running_mean, running_var) and what the bounds need:
    mag_y / mag_dx (L1 mass of the terms behind one element, as oracle.fp64_ref.norm_act_ref), mass (L1 mass of the terms of
    the three parameter sums), z, and kink = |dy| rstd |gamma| * the jump of the activation's slope at z = 0."""
    x, dy = x.double(), dy.double()
    C = x.shape[4]
    red = (0, 1, 2, 3) if mode == "batch" else (1, 2, 3)
    n = x.numel() // C // (1 if mode == "batch" else x.shape[0])
    mu = x.mean(red, keepdim=True)
    var = ((x - mu) ** 2).mean(red, keepdim=True)
    rstd = (var + eps).rsqrt()
    ga = gamma.double().view(1, 1, 1, 1, C) if gamma is not None else torch.ones((1, 1, 1, 1, C), dtype=torch.float64, device=x.device)
    be = beta.double().view(1, 1, 1, 1, C) if beta is not None else torch.zeros_like(ga)
    a = float(slope) if slope is not None else 0.25
    xhat = (x - mu) * rstd
    z = xhat * ga + be
    y, da, ds, jump = act64(z, act, a)
    dz = dy * da
    s1 = dz.mean(red, keepdim=True)
    s2 = (dz * xhat).mean(red, keepdim=True)
    dx = rstd * ga * (dz - s1 - xhat * s2)
    xmag = (x.abs() + mu.abs()) * rstd
    out = dict(y=y, dx=dx, z=z, mag_y=ga.abs() * xmag + be.abs(),
               mag_dx=ga.abs() * rstd * (dz.abs() + dz.abs().mean(red, keepdim=True) + xmag * (dz * xhat).abs().mean(red, keepdim=True)),
               kink=dy.abs() * rstd * ga.abs() * jump,
               dgamma=(dz * xhat).sum((0, 1, 2, 3)), dbeta=dz.sum((0, 1, 2, 3)), dslope=(dy * ds).sum().reshape(1),
               mass=dict(dgamma=(dz * xhat).abs().sum((0, 1, 2, 3)), dbeta=dz.abs().sum((0, 1, 2, 3)),
                         dslope=(dy * ds).abs().sum().reshape(1)))
    if mode == "batch":
        out["running_mean"] = momentum * mu.reshape(C)
        out["running_var"] = (1 - momentum) + momentum * var.reshape(C) * n / max(1, n - 1)
    return out


def _bn_cols(t, eps):
    """training BatchNorm statistics of the columns of t (rows, C) -> mean, rstd, xhat."""
    mu = t.mean(0, keepdim=True)
    var = ((t - mu) ** 2).mean(0, keepdim=True)
    rstd = (var + eps).rsqrt()
    return mu, rstd, (t - mu) * rstd


def gate64(x, g1raw, x1raw, P, datt, eps=1e-5):
    """The attention gate behind its W_g / W_x convolutions, forward and backward written out in fp64 (csrc/gate.hip):
        s = relu(BN_g(g1raw) + BN_x(x1raw));  psi = sigmoid(BN_psi(w . s + b));  att = x psi
    x (B, D, H, W, C), g1raw / x1raw (B, D, H, W, F), P: gam_g, bet_g, gam_x, bet_x (F), w (F), b (1), gam_p, bet_p (1).
    -> dict of the outputs, the gradients, and A_* = L1 mass of the terms behind one element of each (first-order
    propagation of the operands' magnitudes through the same formulas), kink_* = what one flipped relu mask moves."""
    C, F_ = x.shape[-1], g1raw.shape[-1]
    shp = x.shape
    X, G1, X1, DA = (t.double().reshape(-1, t.shape[-1]) for t in (x, g1raw, x1raw, datt))
    q = {k: v.double().reshape(1, -1) for k, v in P.items()}
    mg, rg, gh = _bn_cols(G1, eps)
    mx, rx, xh = _bn_cols(X1, eps)
    t = gh * q["gam_g"] + q["bet_g"] + xh * q["gam_x"] + q["bet_x"]
    A_t = (G1.abs() + mg.abs()) * rg * q["gam_g"].abs() + q["bet_g"].abs() + (X1.abs() + mx.abs()) * rx * q["gam_x"].abs() + q["bet_x"].abs()
    s = t.clamp_min(0)
    pr = (s * q["w"]).sum(1, keepdim=True) + q["b"]
    A_pr = (A_t * q["w"].abs()).sum(1, keepdim=True) + q["b"].abs()
    mp, rp, zh = _bn_cols(pr, eps)
    zp = zh * q["gam_p"] + q["bet_p"]
    A_z = q["gam_p"].abs() * rp * (A_pr + mp.abs() + zh.abs() * (A_pr ** 2).mean().sqrt()) + q["bet_p"].abs()
    psi = torch.sigmoid(zp)
    A_psi = 0.25 * A_z + psi                                   # (sigmoid' <= 1 / 4; + the sigmoid's own roundings)
    att = X * psi
    # backward
    dx = DA * psi
    dpsi = (DA * X).sum(1, keepdim=True)
    A_dpsi = (DA * X).abs().sum(1, keepdim=True)
    sg = psi * (1 - psi)
    dzp = dpsi * sg
    A_dzp = A_dpsi * sg + dpsi.abs() * A_psi                   # (|d(psi (1 - psi))| <= |d psi|)
    n1, n2 = dzp.mean(), (dzp * zh).mean()
    cp = q["gam_p"] * rp
    dpr = cp * (dzp - n1 - zh * n2)
    A_dpr = cp.abs() * (A_dzp + A_dzp.mean() + zh.abs() * (A_dzp * zh.abs()).mean())
    live = (s > 0).double()
    d = dpr * q["w"] * live
    A_d = A_dpr * q["w"].abs() * live
    out = dict(att=att.reshape(shp), psi=psi.reshape(*shp[:4], 1), A_psi=A_psi.reshape(*shp[:4], 1), dx=dx.reshape(shp),
               A_att=(X.abs() * A_psi).reshape(shp),
               A_dx=(DA.abs() * A_psi).reshape(shp), t=t, A_t=A_t,
               dw=(dpr * s).sum(0), m_dw=(A_dpr * s.abs()).sum(0), dgam_p=(dzp * zh).sum().reshape(1), dbet_p=dzp.sum().reshape(1),
               m_dgam_p=(A_dzp * zh.abs()).sum().reshape(1), m_dbet_p=A_dzp.sum().reshape(1))
    for name, hat, r_, gam in (("g", gh, rg, q["gam_g"]), ("x", xh, rx, q["gam_x"])):
        a_, b_ = d.mean(0, keepdim=True), (d * hat).mean(0, keepdim=True)
        c_ = r_ * gam
        out["d" + name + "1"] = (c_ * (d - a_ - hat * b_)).reshape(g1raw.shape)
        out["A_d" + name + "1"] = (c_.abs() * (A_d + A_d.mean(0, keepdim=True) + hat.abs() * (A_d * hat.abs()).mean(0, keepdim=True))).reshape(g1raw.shape)
        out["kink_d" + name + "1"] = (c_.abs() * (dpr * q["w"]).abs()).reshape(g1raw.shape)
        out["dgam_" + name], out["dbet_" + name] = (d * hat).sum(0), d.sum(0)
        out["m_dgam_" + name], out["m_dbet_" + name] = (A_d * hat.abs()).sum(0), A_d.sum(0)
    n = X.shape[0]
    for name, mu_, r_ in (("g", mg, rg), ("x", mx, rx), ("p", mp, rp)):
        var = 1.0 / r_ ** 2 - eps
        out["rm_" + name] = 0.1 * mu_.reshape(-1)
        out["rv_" + name] = 0.9 + 0.1 * var.reshape(-1) * n / max(1, n - 1)
    return out
