"""fp64 references that run at the full production size, and the per-element error bound the bf16 kernels are held to.

Test infrastructure only: the product never imports this module.

Convolutions are written as a sum over taps of fp64 GEMMs on shifted views of channels-last volumes (B, D, H, W, C),
with weights in the library's kernel layout wk[Bw, taps, Cout, Cin] (Bw = 1: shared, Bw = B: per-sample CondConv
weights; tap = (kz * k + ky) * k + kx).  The output grid is cut into slabs along D so peak memory stays bounded.  Every
call can also return the magnitude tensor A = |x| (*) |w| + |b| -- the same operation on absolute values -- that the
per-element bound needs.  It is plain torch on whatever device the inputs live on and shares no code with the kernels.
"""
import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8          # unit roundoff of bf16 (8 significant bits, round to nearest)
U_F32 = 2.0 ** -24

_SLAB_ELEMS = 1 << 26       # fp64 elements of one gathered operand slab (512 MB)


def _chunks(n, per):
    per = max(1, per)
    return [(a, min(n, a + per)) for a in range(0, n, per)]


def _gather(x, wt, stride, pad, out_dhw, bias=None):
    """out[b, o] = bias[b] + sum_t xpad[b, o * stride + t] @ wt[b, t]^T;  x (B, D, H, W, C), wt (Bw, k^3, N, C)."""
    B, C = x.shape[0], x.shape[4]
    Bw, T, N = wt.shape[0], wt.shape[1], wt.shape[2]
    k = round(T ** (1.0 / 3.0))
    Do, Ho, Wo = out_dhw
    xp = F.pad(x, (0, 0, pad, pad + k, pad, pad + k, pad, pad + k)) if pad or k > 1 else x
    out = torch.empty((B, Do, Ho, Wo, N), dtype=x.dtype, device=x.device)
    per = _SLAB_ELEMS // max(1, B * Ho * Wo * max(C, N))
    w_t = wt.transpose(2, 3)                       # (Bw, T, C, N)
    for d0, d1 in _chunks(Do, per):
        acc = torch.zeros((B, d1 - d0, Ho, Wo, N), dtype=x.dtype, device=x.device)
        if bias is not None:
            acc += bias.view(bias.shape[0] if bias.dim() == 2 else 1, 1, 1, 1, N)
        for t in range(T):
            tz, ty, tx = t // (k * k), (t // k) % k, t % k
            z0 = d0 * stride + tz
            xs = xp[:, z0:z0 + (d1 - d0 - 1) * stride + 1:stride, ty:ty + (Ho - 1) * stride + 1:stride,
                    tx:tx + (Wo - 1) * stride + 1:stride, :]
            a = xs.reshape(B, -1, C)
            acc += torch.matmul(a, w_t[:, t] if Bw == B else w_t[0, t]).view_as(acc)
        out[:, d0:d1] = acc
    return out


def _scatter(x, wt, stride, pad, out_dhw):
    """out[b, i * stride - pad + t] += x[b, i] @ wt[b, t]^T (the adjoint of _gather);  x (B, D, H, W, C)."""
    B, D, H, W, C = x.shape
    Bw, T, N = wt.shape[0], wt.shape[1], wt.shape[2]
    k = round(T ** (1.0 / 3.0))
    Do, Ho, Wo = out_dhw
    ext = lambda n, no: max((n - 1) * stride + k, no + pad)
    yp = torch.zeros((B, ext(D, Do), ext(H, Ho), ext(W, Wo), N), dtype=x.dtype, device=x.device)
    w_t = wt.transpose(2, 3)
    per = _SLAB_ELEMS // max(1, B * H * W * max(C, N))
    for d0, d1 in _chunks(D, per):
        a = x[:, d0:d1].reshape(B, -1, C)
        for t in range(T):
            tz, ty, tx = t // (k * k), (t // k) % k, t % k
            z0 = d0 * stride + tz
            v = torch.matmul(a, w_t[:, t] if Bw == B else w_t[0, t]).view(B, d1 - d0, H, W, N)
            yp[:, z0:z0 + (d1 - d0 - 1) * stride + 1:stride, ty:ty + (H - 1) * stride + 1:stride,
               tx:tx + (W - 1) * stride + 1:stride, :] += v
    return yp[:, pad:pad + Do, pad:pad + Ho, pad:pad + Wo].contiguous()


def _pair(a, g, stride, pad, a_is_coarse_gathered, per_sample, T):
    """dw[b, t] = sum over pairs.  conv: a = dy (N at output grid), g = x gathered: dw[t] = dy^T @ xpad_shift[t].
    transposed (a_is_coarse_gathered=False): a = x (coarse), g = dy gathered at fine positions: dw[t] = gshift[t]^T @ x."""
    B = a.shape[0]
    k = round(T ** (1.0 / 3.0))
    Do, Ho, Wo = a.shape[1:4]
    Na, Ng = a.shape[4], g.shape[4]
    gp = F.pad(g, (0, 0, pad, pad + k, pad, pad + k, pad, pad + k))
    out = torch.zeros((B, T, Na, Ng) if a_is_coarse_gathered else (B, T, Ng, Na), dtype=a.dtype, device=a.device)
    per = _SLAB_ELEMS // max(1, B * Ho * Wo * max(Na, Ng))
    for d0, d1 in _chunks(Do, per):
        # one GEMM per (sample, z-plane), summed after: a single GEMM with K = 2M voxels and tiny M, N is very slow
        aa = a[:, d0:d1].reshape(B * (d1 - d0), Ho * Wo, Na)
        for t in range(T):
            tz, ty, tx = t // (k * k), (t // k) % k, t % k
            z0 = d0 * stride + tz
            gs = gp[:, z0:z0 + (d1 - d0 - 1) * stride + 1:stride, ty:ty + (Ho - 1) * stride + 1:stride,
                    tx:tx + (Wo - 1) * stride + 1:stride, :].reshape(B * (d1 - d0), Ho * Wo, Ng)
            if a_is_coarse_gathered:
                p_ = torch.matmul(aa.transpose(1, 2), gs)
            else:
                p_ = torch.matmul(gs.transpose(1, 2), aa)
            out[:, t] += p_.view(B, d1 - d0, *p_.shape[1:]).sum(1)
    return out if per_sample else out.sum(0, keepdim=True)


def out_grid(dhw, k, stride, transposed):
    if transposed:
        return tuple(n * stride for n in dhw)
    p = (k - 1) // 2
    return tuple((n + 2 * p - k) // stride + 1 for n in dhw)


def conv_fwd(x, wk, bias, k, stride, transposed, mag=True):
    """y = conv3d / conv_transpose3d (padding (k-1)/2, output_padding stride-1) of channels-last x with kernel-layout
    weights wk [Bw, k^3, Cout, Cin] and bias (Cout,) / (B, Cout) / None.  -> (y, A) with A = |x| (*) |wk| + |bias|
    (None when mag=False)."""
    p = (k - 1) // 2
    og = out_grid(x.shape[1:4], k, stride, transposed)
    run = (lambda xx, ww, bb: _scatter(xx, ww, stride, p, og) + (0 if bb is None else bb.view(bb.shape[0] if bb.dim() == 2 else 1, 1, 1, 1, -1))) \
        if transposed else (lambda xx, ww, bb: _gather(xx, ww, stride, p, og, bb))
    y = run(x, wk, bias)
    A = run(x.abs(), wk.abs(), None if bias is None else bias.abs()) if mag else None
    return y, A


def conv_dgrad(dy, wk, x_dhw, k, stride, transposed, mag=True):
    """dx of conv_fwd for upstream gradient dy (channels-last), kernel-layout wk [Bw, k^3, Cout, Cin]. -> (dx, A)."""
    p = (k - 1) // 2
    wT = wk.transpose(2, 3)                      # (Bw, T, Cin, Cout)
    run = (lambda g, w: _gather(g, w, stride, p, x_dhw)) if transposed else (lambda g, w: _scatter(g, w, stride, p, x_dhw))
    dx = run(dy, wT)
    return dx, (run(dy.abs(), wT.abs()) if mag else None)


def conv_wgrad(x, dy, k, stride, transposed, per_sample, mag=True):
    """dwk [Bw, k^3, Cout, Cin] of conv_fwd (summed over the batch unless per_sample). -> (dw, A)."""
    p, T = (k - 1) // 2, k ** 3
    if transposed:
        run = lambda xx, gg: _pair(xx, gg, stride, p, False, per_sample, T)
    else:
        run = lambda xx, gg: _pair(gg, xx, stride, p, True, per_sample, T)
    dw = run(x, dy)
    return dw, (run(x.abs(), dy.abs()) if mag else None)


# ---------------------------------------------------------------------------------------------------------------------
# error checks
# ---------------------------------------------------------------------------------------------------------------------
def elem_bound(ref, A, K, u_out=U_BF16, base=None):
    """Worst-case bound of an output rounded once to a format of unit roundoff u_out, computed from bf16-exact operands
    with fp32 accumulation over K terms in ANY order (split-K atomics included):
        |got - ref| <= u_out |ref| + 2 K 2^-24 A  (+ |base| u_out for an accumulate epilogue)."""
    b = u_out * ref.abs() + (2.0 * K * U_F32) * A
    if base is not None:
        b = b + u_out * base.abs()
    return b


def slab_rel_l2(got, ref, dims):
    """max over slabs of rel-L2; a slab is one index of the leading `dims` axes (e.g. 2: (sample, z-plane) of a
    channels-last volume, (sample, tap) of a kernel-layout weight gradient).  An all-zero reference slab must be matched
    exactly (inf otherwise)."""
    g = got.double().reshape(*ref.shape[:dims], -1)
    r = ref.double().reshape(*ref.shape[:dims], -1)
    num = (g - r).norm(dim=-1)
    den = r.norm(dim=-1)
    q = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))
    return float(q.max())


def check_elementwise(got, ref, bound, what=""):
    """-> max |got - ref| / bound; asserts <= 1 (and that got is finite) with the worst element in the message."""
    g = got.detach().double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{what}: element {idx} off by {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}"
                             f" (ref {float(ref.reshape(-1)[i]):.4e}, got {float(g.reshape(-1)[i]):.4e}); worst ratio {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# normalisation + activation, attention gate
# ---------------------------------------------------------------------------------------------------------------------
def act_ref(z, act, slope=None):
    if act == "none":
        return z
    if act == "relu":
        return F.relu(z)
    if act == "prelu":
        return F.prelu(z, slope)
    if act == "leaky":
        return F.leaky_relu(z, 0.01)
    if act == "sigmoid":
        return torch.sigmoid(z)
    if act == "prelu_relu":
        return F.relu(F.prelu(z, slope))
    raise ValueError(act)


def _bn(x, red, gamma, beta, eps, rm=None, rv=None, momentum=0.1):
    """Normalisation over the axes `red` of a channels-first fp64 tensor in plain torch arithmetic (no library kernel);
    rm / rv (BatchNorm running statistics, unbiased variance) are updated in place."""
    C = x.shape[1]
    mu = x.mean(red, keepdim=True)
    var = ((x - mu) ** 2).mean(red, keepdim=True)
    if rm is not None:
        n = x.numel() // C
        with torch.no_grad():
            rm.mul_(1 - momentum).add_(momentum * mu.reshape(C))
            rv.mul_(1 - momentum).add_(momentum * var.reshape(C) * n / max(1, n - 1))
    z = (x - mu) * torch.rsqrt(var + eps)
    if gamma is not None:
        z = z * gamma.view(1, C, 1, 1, 1)
    if beta is not None:
        z = z + beta.view(1, C, 1, 1, 1)
    return z


def norm_act_ref(x, dy, mode, act, gamma=None, beta=None, slope=None, eps=1e-5, momentum=0.1):
    """fp64 BatchNorm(train) / InstanceNorm + activation on channels-last x (B, D, H, W, C), forward and backward by
    autograd.  -> dict(y, dx, dgamma, dbeta, dslope, running_mean, running_var, mag_y, mag_dx).  mag_*: magnitudes
    of the terms each output is computed from (|gamma| (|x| + |mean|) rstd + |beta|; |gamma| rstd (|dz| + mean |dz| +
    (|x| + |mean|) rstd mean |dz xhat|)), dz_mass: L1 mass of the terms of dgamma / dbeta / dslope."""
    C = x.shape[4]
    xe = x.permute(0, 4, 1, 2, 3).double().clone().requires_grad_(True)
    ps = [None if t is None else t.double().clone().requires_grad_(True) for t in (gamma, beta, slope)]
    rm = torch.zeros(C, dtype=torch.float64, device=x.device)
    rv = torch.ones(C, dtype=torch.float64, device=x.device)
    red = (0, 2, 3, 4) if mode == "batch" else (2, 3, 4)
    z = _bn(xe, red, ps[0], ps[1], eps, rm if mode == "batch" else None, rv if mode == "batch" else None, momentum)
    zd = z.detach().requires_grad_(True)
    y = act_ref(zd, act, ps[2])
    dye = dy.permute(0, 4, 1, 2, 3).double()
    dz = torch.autograd.grad(y, [zd] + ([ps[2]] if ps[2] is not None else []), dye)
    dslope = dz[1] if ps[2] is not None else None
    dz = dz[0]
    z.backward(dz)
    with torch.no_grad():
        mu = xe.mean(red, keepdim=True)
        rstd = (xe.var(red, unbiased=False, keepdim=True) + eps).rsqrt()
        xhat = (xe - mu) * rstd
        xmag = (xe.abs() + mu.abs()) * rstd          # (x - mean) * rstd is formed from these two terms
        gm = ps[0].view(1, C, 1, 1, 1).abs() if ps[0] is not None else 1.0
        bm = ps[1].view(1, C, 1, 1, 1).abs() if ps[1] is not None else 0.0
        mag_y = gm * xmag + bm
        mag_dx = gm * rstd * (dz.abs() + dz.abs().mean(red, keepdim=True) + xmag * (dz * xhat).abs().mean(red, keepdim=True))
        cred = (0, 2, 3, 4)
        dz_mass = {"dgamma": (dz * xhat).abs().sum(cred), "dbeta": dz.abs().sum(cred),
                   "dslope": (dye * zd).abs().sum().reshape(1)}
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    return dict(y=cl(y.detach()), dx=cl(xe.grad), dgamma=None if ps[0] is None else ps[0].grad,
                dbeta=None if ps[1] is None else ps[1].grad, dslope=dslope,
                running_mean=rm, running_var=rv, mag_y=cl(mag_y), mag_dx=cl(mag_dx), dz_mass=dz_mass)


def gate_ref(P, g, x, rm=None, momentum=0.1, eps=1e-5):
    """fp64 attention gate of MONAI's AttentionBlock in training mode (channels-first g, x (B, C, D, H, W)):
        psi = sigmoid(BN_psi(W_psi relu(BN_g(W_g g) + BN_x(W_x x))));  att = x * psi.
    P: {parameter name of ObservableAttentionBlock: fp64 tensor}; rm: {"W_g" | "W_x" | "psi": [running mean, var]},
    updated in place.  -> (att, psi)."""
    def cbn(name, t):
        w = P[f"{name}.0.conv.weight"]
        y = torch.einsum("bcdhw,oc->bodhw", t, w.reshape(w.shape[0], w.shape[1]))
        b = P.get(f"{name}.0.conv.bias")
        if b is not None:
            y = y + b.view(1, -1, 1, 1, 1)
        r = rm[name] if rm is not None else [None, None]
        return _bn(y, (0, 2, 3, 4), P[f"{name}.1.weight"], P[f"{name}.1.bias"], eps, r[0], r[1], momentum)

    s = F.relu(cbn("W_g", g) + cbn("W_x", x))
    psi = torch.sigmoid(cbn("psi", s))
    return x * psi, psi
