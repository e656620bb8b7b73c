"""Shared by the inference tests: the eval-mode attention gate as plain fp64 torch (F.conv3d + F.batch_norm(training=False)),
and the random BatchNorm state the tests put into a gate block.  (oracle/fp64_ref.gate_ref is the training-mode gate.)"""
import torch
import torch.nn.functional as F


def randomize_gate(block, seed):
    """gamma in [0.5, 1.5], beta in [-0.3, 0.3], running means in +-0.5, running variances in [0.5, 2]."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda t, lo, hi: t.copy_((torch.rand(t.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).to(t.dtype))
    with torch.no_grad():
        for bn in (block.W_g[1], block.W_x[1], block.psi[1]):
            u(bn.weight, 0.5, 1.5), u(bn.bias, -0.3, 0.3), u(bn.running_mean, -0.5, 0.5), u(bn.running_var, 0.5, 2.0)


def gate_eval_ref64(block, g, x):
    """g, x: (B, C, D, H, W).  Returns (att (B, C, D, H, W), psi (B, 1, D, H, W)) in fp64 on the CPU."""
    d = lambda t: None if t is None else t.detach().double().cpu()
    g, x = d(g), d(x)

    def conv_bn(seq, t):
        c, bn = seq[0].conv, seq[1]
        return F.batch_norm(F.conv3d(t, d(c.weight), d(c.bias)), d(bn.running_mean), d(bn.running_var), d(bn.weight),
                            d(bn.bias), training=False, eps=bn.eps)
    s = torch.relu(conv_bn(block.W_g, g) + conv_bn(block.W_x, x))
    psi = torch.sigmoid(conv_bn(block.psi, s))
    return x * psi, psi


def folded_gate64(fold, wg, wx, g, x):
    """The gate from fold_gate's tables alone (plus the bare convolution weights), in the tables' dtype."""
    F_ = fold["scale_g"].numel()
    v = lambda t: t.reshape(1, F_, 1, 1, 1)
    s = torch.relu(v(fold["scale_g"]) * F.conv3d(g, wg) + v(fold["scale_x"]) * F.conv3d(x, wx) + v(fold["shift"]))
    psi = torch.sigmoid(fold["psi_ab"][0] * (s * v(fold["w_psi"])).sum(1, keepdim=True) + fold["psi_ab"][1])
    return x * psi, psi
