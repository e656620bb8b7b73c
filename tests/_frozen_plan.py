"""Shared by test_frozen_bn_cpu.py and test_frozen_bn_kernels_gpu.py: plain-Python mirrors of the launch arithmetic of the
frozen-BatchNorm kernels (csrc/norm.hip: norm_act_bwd_frozen_k; csrc/gate.hip: gate_frozen_fwd_k / gate_frozen_bwd_k), the
shapes they are run at, and fp64 restatements of the frozen BatchNorm + activation and of the frozen attention gate.

A BatchNorm is frozen when a train-mode model normalises with the running statistics: with m = running_mean and
r = rsqrt(running_var + eps) it is the per-channel affine map xhat = (x - m) r, z = gamma xhat + beta.  The restatements are
plain torch without autograd and share no code with the kernels; the CPU module checks them against torch autograd.
"""
import torch

import _nonconv_plan as NP

# sup |sigmoid''| = 1 / (6 sqrt 3) < 0.0963: what an error of z moves the sigmoid's derivative by
SIG_LIP = 0.0963
K_Z = 8        # fp32 roundings behind z = fma((x - m) r, gamma, beta): r from running_var (add, rsqrt within 2 ulp: 3), the
               # difference, two products / the fma (3), a margin of 2


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def frozen_vec(dtype, C, lds, sums):
    """pick_vec8 over x, dy and dx: 8 bf16 channels (16 bytes) where C and every pitch allow and no parameter sum is wanted
    (with the sums the kernel is 4 wide at most, as the training backward's sums pass), else 4, else 1."""
    if dtype == "bf16" and not sums and C % 8 == 0 and all(ld % 8 == 0 for ld in lds):
        return 8
    return 4 if C % 4 == 0 and all(ld % 4 == 0 for ld in lds) else 1


def frozen_norm_plan(rows, C, vec, dtype):
    """norm_act_bwd_frozen_k: make_rows(batch) -> blocks = row chunks, trips of the row loop of the busiest thread (one
    trip = a burst of 8 (bf16) / 2 (fp32) rows per thread, ry rows apart), whether the last chunk is short and whether a
    burst ends inside a chunk (masked rows)."""
    r = NP.make_rows(rows, C, 1, vec)
    burst = 8 if dtype == "bf16" else 2
    per_thread = NP.cdiv(r["ch"], r["ry"])
    last = rows - (r["nchunks"] - 1) * r["ch"]
    return dict(blocks=r["nchunks"], ch=r["ch"], ry=r["ry"], cv=r["cv"], cvp=r["cvp"], trips=NP.cdiv(per_thread, burst),
                ragged_last=last != r["ch"], ragged_rows=r["ch"] % r["ry"] != 0 or last % r["ry"] != 0,
                masked_burst=per_thread % 2 != 0 or NP.cdiv(last, r["ry"]) % 2 != 0)


# NormAct frozen, bf16 twins (B = 2): (V, C, pitch of x, activation) -- 16-byte vectors at C = 8 and 32 and, through a pitch of
# 12 channels, 8-byte ones; each with several row chunks, several bursts per thread and a short last chunk
FROZEN_BF16 = [(10238, 8, 16, "prelu"), (3583, 32, 40, "relu"), (2501, 8, 12, "leaky")]
# every activation with and without parameter gradients at one small fp32 shape: (V, C, pitch)
FROZEN_ACT_SHAPE = (4099, 12, 16)

# GateFrozen: (name, dims, B, C, F, dtype, vector width of the backward)
GATE_FROZEN = [("vec4", (81, 81, 81), 1, 32, 16, "f32", 4), ("vec1", (51, 51, 51), 1, 32, 16, "f32", 1),
               ("wide", (5, 6, 7), 2, 256, 128, "f32", 4), ("bf16", (41, 41, 41), 2, 64, 32, "bf16", 4)]
GATE_FROZEN_CAP = 2048        # gate_frozen_fwd_k / gate_frozen_bwd_k: at most 2048 / B blocks per sample
GATE_FROZEN_U = 2             # voxels per lane group and trip


def gate_frozen_plan(V, B, C, F_, vec):
    """gate_frozen_fwd_k (vec up to 8 on bf16) / gate_frozen_bwd_k (vec <= 4): cv = max(C, F) / vec lanes per voxel, a block
    holds 256 / cv voxel slots and strides over its sample's voxels with the grid, two voxels per slot and trip."""
    cv = max(C, F_) // vec
    vpb = 256 // cv
    nb = NP.gate_blocks(V, vpb * GATE_FROZEN_U, max(1, GATE_FROZEN_CAP // B))
    per_trip = nb * vpb * GATE_FROZEN_U
    return dict(cv=cv, vpb=vpb, blocks=nb, trips=NP.cdiv(V, per_trip), ragged=V % per_trip != 0,
                half_live=0 < V % per_trip <= nb * vpb or V % (nb * vpb) != 0)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 restatements
# ---------------------------------------------------------------------------------------------------------------------
def norm_frozen64(x, dy, act, rmean, rvar, gamma=None, beta=None, slope=None, eps=1e-5):
    """Frozen BatchNorm3d + activation on channels-last x (B, D, H, W, C), forward and backward written out in fp64:
        xhat = (x - m) r     z = gamma xhat + beta     y = act(z)
        dz = dy act'(z)      dx = dz gamma r           dgamma = sum dz xhat     dbeta = sum dz     dslope = sum dy dact/dslope
    -> dict(y, dx, dgamma, dbeta, dslope, z) and what the bounds need: mag_y (L1 mass of the terms behind z), mag_dx (of the
    terms behind dx, with what z's error moves a sigmoid's derivative by), mass (of the three sums), kink = |dy| r |gamma| *
    the jump of the activation's slope at z = 0 (what the element moves by when the kernel takes the other branch) and
    kink_mass(near) = what the three sums move by when the elements of the mask `near` do."""
    x, dy = x.double(), dy.double()
    C = x.shape[4]
    v = lambda t, d: (t.double() if t is not None else torch.full((C,), d, dtype=torch.float64, device=x.device)).view(1, 1, 1, 1, C)
    m, r = v(rmean, 0.0), (v(rvar, 1.0) + eps).rsqrt()
    ga, be = v(gamma, 1.0), v(beta, 0.0)
    a = float(slope) if slope is not None else 0.25
    xhat = (x - m) * r
    z = xhat * ga + be
    y, da, ds, jump = NP.act64(z, act, a)
    dz = dy * da
    dx = dz * ga * r
    xmag = (x.abs() + m.abs()) * r
    mag_y = ga.abs() * xmag + be.abs()
    da_mag = da.abs() + (SIG_LIP * mag_y if act == "sigmoid" else 0.0)
    dz_mag = dy.abs() * da_mag
    red = (0, 1, 2, 3)
    live = (ds != 0).double()
    out = dict(y=y, dx=dx, z=z, mag_y=mag_y, mag_dx=dz_mag * ga.abs() * r, kink=dy.abs() * r * ga.abs() * jump,
               dgamma=(dz * xhat).sum(red), dbeta=dz.sum(red), dslope=(dy * ds).sum().reshape(1),
               mass=dict(dgamma=(dz_mag * xmag).sum(red), dbeta=dz_mag.sum(red), dslope=(dy.abs() * mag_y * live).sum().reshape(1)))

    def kink_mass(near):
        k = near * dy.abs() * jump
        return dict(dgamma=(k * xhat.abs()).sum(red), dbeta=k.sum(red), dslope=(near * dy.abs() * mag_y).sum().reshape(1))

    out["kink_mass"] = kink_mass
    return out


def gate_frozen64(x, g1raw, x1raw, P, S, datt, eps=1e-5):
    """The attention gate behind its W_g / W_x convolutions with all three BatchNorms frozen, forward and backward written
    out in fp64:
        t = gam_g ghat + bet_g + gam_x x1hat + bet_x     s = relu(t)     pr = w . s + b
        zhat = (pr - m_p) r_p     psi = sigmoid(gam_p zhat + bet_p)      att = x psi
        dx = datt psi     dpsi = sum_c datt x     dzp = dpsi psi (1 - psi)
        dgam_p = sum dzp zhat     dbet_p = sum dzp     dpr = dzp gam_p r_p     db = sum dpr
        dw_f = sum dpr s_f        d_f = dpr w_f [t_f > 0]
        dg1_f = d_f gam_g,f r_g,f      dx1_f = d_f gam_x,f r_x,f
        dgam_g,f = sum d_f ghat_f      dbet_g,f = sum d_f     (and the same for x)
    x (B, D, H, W, C), g1raw / x1raw (B, D, H, W, F); P: gam_g, bet_g, gam_x, bet_x, w (F), b, gam_p, bet_p (1);
    S: rm_g, rv_g, rm_x, rv_x (F), rm_p, rv_p (1).  -> dict of the outputs, the gradients, A_* = L1 mass of the terms behind
    one element of each, m_* = L1 mass of the terms of each sum, kink_* = what one flipped relu mask moves an element by and
    near_mass(near) = what the sums move by when the relu masks of `near` (rows, F) flip."""
    shp, fs = x.shape, g1raw.shape
    X, G1, X1, DA = (t.double().reshape(-1, t.shape[-1]) for t in (x, g1raw, x1raw, datt))
    q = {k: v.double().reshape(1, -1) for k, v in {**P, **S}.items()}
    rg, rx, rp = (q["rv_g"] + eps).rsqrt(), (q["rv_x"] + eps).rsqrt(), (q["rv_p"] + eps).rsqrt()
    gh, xh = (G1 - q["rm_g"]) * rg, (X1 - q["rm_x"]) * rx
    A_gh, A_xh = (G1.abs() + q["rm_g"].abs()) * rg, (X1.abs() + q["rm_x"].abs()) * rx
    t = gh * q["gam_g"] + q["bet_g"] + xh * q["gam_x"] + q["bet_x"]
    A_t = A_gh * q["gam_g"].abs() + q["bet_g"].abs() + A_xh * q["gam_x"].abs() + q["bet_x"].abs()
    live = (t > 0).double()
    s = t * live
    pr = (s * q["w"]).sum(1, keepdim=True) + q["b"]
    A_pr = (A_t * live * q["w"].abs()).sum(1, keepdim=True) + q["b"].abs()
    zh = (pr - q["rm_p"]) * rp
    A_zh = (A_pr + q["rm_p"].abs()) * rp
    zp = zh * q["gam_p"] + q["bet_p"]
    A_z = q["gam_p"].abs() * A_zh + q["bet_p"].abs()
    psi = torch.sigmoid(zp)
    A_psi = 0.25 * A_z + psi                                   # (sigmoid' <= 1 / 4; + the sigmoid's own roundings)
    dpsi = (DA * X).sum(1, keepdim=True)
    A_dpsi = (DA * X).abs().sum(1, keepdim=True)
    sg = psi * (1 - psi)
    dzp = dpsi * sg
    A_dzp = A_dpsi * sg + dpsi.abs() * A_psi                   # (|d(psi (1 - psi))| <= |d psi|)
    cp = q["gam_p"] * rp
    dpr = dzp * cp
    A_dpr = A_dzp * cp.abs()
    d = dpr * q["w"] * live
    A_d = A_dpr * q["w"].abs() * live
    flip = (dpr * q["w"]).abs()
    out = dict(att=(X * psi).reshape(shp), psi=psi.reshape(*shp[:4], 1), A_psi=A_psi.reshape(*shp[:4], 1),
               A_att=(X.abs() * A_psi).reshape(shp), dx=(DA * psi).reshape(shp), A_dx=(DA.abs() * A_psi).reshape(shp), t=t, A_t=A_t,
               dw=(dpr * s).sum(0), m_dw=(A_dpr * s.abs() + dpr.abs() * A_t * live).sum(0),
               db=dpr.sum().reshape(1), m_db=A_dpr.sum().reshape(1),
               dgam_p=(dzp * zh).sum().reshape(1), m_dgam_p=(A_dzp * zh.abs() + dzp.abs() * A_zh).sum().reshape(1),
               dbet_p=dzp.sum().reshape(1), m_dbet_p=A_dzp.sum().reshape(1))
    hats = {"g": (gh, A_gh, q["gam_g"] * rg), "x": (xh, A_xh, q["gam_x"] * rx)}
    for name, (hat, A_hat, c_) in hats.items():
        out["d" + name + "1"] = (d * c_).reshape(fs)
        out["A_d" + name + "1"] = (A_d * c_.abs()).reshape(fs)
        out["kink_d" + name + "1"] = (flip * c_.abs()).reshape(fs)
        out["dgam_" + name], out["dbet_" + name] = (d * hat).sum(0), d.sum(0)
        out["m_dgam_" + name], out["m_dbet_" + name] = (A_d * hat.abs() + d.abs() * A_hat).sum(0), A_d.sum(0)

    def near_mass(near):
        k = near * flip
        o = dict(dw=(near * dpr.abs() * A_t).sum(0), db=torch.zeros(1, dtype=torch.float64, device=X.device),
                 dgam_p=torch.zeros(1, dtype=torch.float64, device=X.device), dbet_p=torch.zeros(1, dtype=torch.float64, device=X.device))
        for name, (hat, _A, _c) in hats.items():
            o["dgam_" + name], o["dbet_" + name] = (k * hat.abs()).sum(0), k.sum(0)
        return o

    out["near_mass"] = near_mass
    return out
