"""Helpers of the front training tests (test_front_train_host.py, test_gpu_batchnorm_train.py, test_gpu_grouper_bwd.py,
test_gpu_front_train.py): float64 references of the new kernels with componentwise bounds, fp32 emulations of their arithmetic with the
faults the host test plants, and the float64 restatement of the Compressor's front in TRAINING mode with its bf16 twin.  Training-mode
BatchNorm is restated here: oracle/ldt_oracle.batch_norm_eval is eval-only.  None of a bound is taken from what a kernel returned.

Bounds, counted from the kernels' operation order (csrc/batchnorm.hip, csrc/grouper_bwd.hip); u = 2^-24, v = 2^-53:
  bn_stats      mean: the float64 sum of M fp32 values (M v sum|x| / M) and one rounding.  rstd: the float64 mean of (x - mean)^2 moves the
                variance by at most (M + 8) v of 2 mean (x - mean)^2, which 1 / sqrt carries as rstd^3 / 2, plus one rounding.  The running
                buffers: the float64 blend and one rounding.
  bn_relu_fwd   xhat = (x - mean) * rstd: two roundings; pre = fma(gamma, xhat, beta): one; bf16 output: 2^-8 on top.
  bn_relu_bwd   the mask is a SELECTION: the reference takes it as an argument (default: the forward's fp32 arithmetic restated, whose sign is
                exact).  dbeta: one rounding + the float64 sum.  dgamma: the same + 2 u per term for the fp32 xhat.  dx: the two column means
                (one rounding each on top of their sums' bounds), the subtraction, the fma, gamma * rstd and the final product.
  maxpool_*     exact: torch.equal.
  group_normalize_bwd   d = g - anchor is fp32 in the kernel (u |d|); inv carries kernel_checks.group_reference's rho (the statistics kernel's
                allowance), the mean tol1 / n_el, sigma rho / inv; every sum is float64 with one rounding.
"""
import torch

import kernel_checks as kc
from kernel_checks import SLACK, U8, U24

U53 = 2.0 ** -53
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# (M, C): the smallest M and an odd width; the tiny fixture's M; a row tail and a width that is no multiple of 4; MiniPointnet's width;
# past the shipped 65 536 rows (137 workgroups of rows: partials across workgroups)
BN_CASES = [(2, 5), (384, 64), (4101, 131), (512, 256), (70000, 128)]
# (B, n, S, k, D)
GNB_CASES = [(1, 5, 1, 2, 3), (3, 64, 8, 16, 64), (2, 300, 7, 12, 128), (2, 2048, 32, 128, 128)]


# ------------------------------------------------------------------------------------------------- training-mode BatchNorm + ReLU
def bn_case(M, C, seed=None, zero_var_col=None, big_row=None):
    """-> dict(x, dy, gamma, beta, running_mean, running_var) fp32.  zero_var_col: that column of x holds one value; big_row: that row's dy
    is 2^20 times the others'."""
    g = torch.Generator().manual_seed(7000 + 31 * M + C if seed is None else seed)
    x = torch.randn(M, C, generator=g) * (0.5 + torch.rand(C, generator=g) * 2) + torch.randn(C, generator=g)
    if zero_var_col is not None:
        x[:, zero_var_col] = 0.3713
    dy = torch.randn(M, C, generator=g)
    if big_row is not None:
        dy[big_row] *= 2.0 ** 20
    return {"x": x, "dy": dy, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.3,
            "running_mean": torch.randn(C, generator=g) * 0.1, "running_var": torch.rand(C, generator=g) + 0.5}


def bn_stats_ref(x, running_mean=None, running_var=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """float64 -> ({mean, rstd, running_mean, running_var}, the same keys' bounds)."""
    M = x.shape[0]
    x64 = x.double()
    mean = x64.mean(0)
    dev2 = ((x64 - mean) ** 2).mean(0)
    rstd = 1 / torch.sqrt(dev2 + eps)
    d_mean = M * U53 * x64.abs().mean(0)
    d_var = (M + 8) * U53 * 2 * dev2 + 2 * d_mean * (x64 - mean).abs().mean(0)
    ref = {"mean": mean, "rstd": rstd}
    tol = {"mean": (mean.abs() * U24 + d_mean) * SLACK, "rstd": (rstd * U24 + 0.5 * rstd ** 3 * d_var) * SLACK}
    if running_mean is not None:
        rm = (1 - momentum) * running_mean.double() + momentum * mean
        ref["running_mean"], tol["running_mean"] = rm, (rm.abs() * U24 + momentum * d_mean + 4 * U53 * (running_mean.double().abs() + mean.abs())) * SLACK
    if running_var is not None:
        unb = dev2 * M / (M - 1)
        rv = (1 - momentum) * running_var.double() + momentum * unb
        ref["running_var"], tol["running_var"] = rv, (rv.abs() * U24 + momentum * d_var * M / (M - 1) + 4 * U53 * rv.abs()) * SLACK
    return ref, tol


def bn_pre_fp32(x, stats, gamma, beta):
    """The forward's fp32 arithmetic restated: xhat = fl(fl(x - mean) * rstd) in fp32; pre = fma(gamma, xhat, beta), formed in float64 from the
    exact product (its sign is the fma's) -> (xhat fp32, pre float64)."""
    xh = (x - stats[0]) * stats[1]
    return xh, gamma.double() * xh.double() + beta.double()


def bn_relu_fwd_ref(x, stats, gamma, beta, out_bf16):
    """float64 from the fp32 operands -> (y, tol)."""
    xh = (x.double() - stats[0].double()) * stats[1].double()
    gx = gamma.double() * xh
    pre = gx + beta.double()
    tol = 2 * U24 * gx.abs() + U24 * pre.abs()
    y = pre.clamp_min(0)
    if out_bf16:
        tol = tol + U8 * (y + tol)
    return y, tol * SLACK


def bn_relu_bwd_ref(dy, x, stats, gamma, beta, mask=None):
    """float64 -> ((dx, dgamma, dbeta), their bounds).  mask: the selection y > 0 to differentiate at (default: the forward's own)."""
    M = x.shape[0]
    if mask is None:
        mask = bn_pre_fp32(x, stats, gamma, beta)[1] > 0
    rstd, ga = stats[1].double(), gamma.double()
    xh = (x.double() - stats[0].double()) * rstd
    dyh = dy.double() * mask
    dbeta, dgamma = dyh.sum(0), (dyh * xh).sum(0)
    tol_db = (dbeta.abs() * U24 + M * U53 * dyh.abs().sum(0)) * SLACK
    tol_dg = (dgamma.abs() * U24 + (2 * U24 + M * U53) * (dyh * xh).abs().sum(0)) * SLACK
    mb, mg = dbeta / M, dgamma / M
    d_mb, d_mg = tol_db / M + U24 * mb.abs(), tol_dg / M + U24 * mg.abs()
    t1 = dyh - mb
    t = t1 - xh * mg
    a = ga * rstd
    dx = a * t
    tol_dx = a.abs() * (U24 * t1.abs() + d_mb + xh.abs() * d_mg + mg.abs() * 2 * U24 * xh.abs() + U24 * t.abs()) + 2 * U24 * dx.abs()
    return (dx, dgamma, dbeta), (tol_dx * SLACK, tol_dg, tol_db)


BN_FAULTS = ("unbiased variance in rstd", "biased variance in running_var", "xhat dgamma / M dropped", "mask from dy", "fp32 running sums")


def bn_emulate(c, fault=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """The three kernels' arithmetic on the CPU (float64 sums rounded once, fp32 rows) with one of BN_FAULTS planted -> dict(mean, rstd,
    running_mean, running_var, y (fp32), dx, dgamma, dbeta)."""
    assert fault is None or fault in BN_FAULTS
    x, dy, ga, be = c["x"], c["dy"], c["gamma"], c["beta"]
    M = x.shape[0]
    if fault == "fp32 running sums":
        s = torch.zeros(x.shape[1])
        for r in range(M):
            s = s + x[r]
        mean64 = (s / M).double()
    else:
        mean64 = x.double().sum(0) / M
    a = ((x.double() - mean64) ** 2).sum(0)
    var = a / (M - 1 if fault == "unbiased variance in rstd" else M)
    stats = torch.stack([mean64.float(), (1 / torch.sqrt(var + eps)).float()])
    unb = a / (M if fault == "biased variance in running_var" else M - 1)
    out = {"mean": stats[0], "rstd": stats[1],
           "running_mean": ((1 - momentum) * c["running_mean"].double() + momentum * mean64).float(),
           "running_var": ((1 - momentum) * c["running_var"].double() + momentum * unb).float()}
    xh, pre = bn_pre_fp32(x, stats, ga, be)
    out["y"] = pre.float().clamp_min(0)
    mask = (dy > 0) if fault == "mask from dy" else (pre > 0)
    dyh = torch.where(mask, dy, torch.zeros_like(dy))
    db64, dg64 = dyh.double().sum(0), (dyh.double() * xh.double()).sum(0)
    mb, mg = (db64 / M).float(), (dg64 / M).float()
    if fault == "xhat dgamma / M dropped":
        mg = torch.zeros_like(mg)
    t = ((dyh - mb).double() - xh.double() * mg.double()).float()
    out.update({"dx": (ga * stats[1]) * t, "dgamma": dg64.float(), "dbeta": db64.float(), "stats": stats})
    return out


def worst_ratio(got, ref, tol):
    """max err / tol over one output without asserting (the planted faults)."""
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


# ------------------------------------------------------------------------------------------------- the max with its arg-max
def maxpool_case(G, n, C, seed, bf16=False):
    """Values with planted ties (an equal maximum in two rows: the first wins), positive ones, and cells whose every row is <= 0 (ReLU
    outputs: exactly 0) -> x [G n, C]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(G, n, C, generator=g).clamp_min(0)               # ReLU outputs: about half the cells are 0, ties at 0 everywhere
    if n > 1:
        top = x.max(1).values + 1.0
        x[:, n - 1, ::3] = top[:, ::3]                                # a positive tie: the same maximum in the last row and ...
        x[:, 0, ::6] = top[:, ::6]                                    # ... (every other one of them) in the first
        x[:, :, 1::7] = 0.0                                           # all-zero cells
    if bf16:
        x = x.bfloat16().float()
    return x.reshape(G * n, C)


def maxpool_argmax_ref(x, G, n, last_wins=False):
    x3 = x.double().view(G, n, -1)
    out = x3.max(1).values
    hit = x3 == out[:, None, :]
    if last_wins:
        arg = n - 1 - hit.flip(1).int().argmax(1)
    else:
        arg = hit.int().argmax(1)
    return out.float(), arg.int()


def maxpool_relu_bwd_ref(d_out, out, arg, n):
    G, C = out.shape
    dz = torch.zeros(G, n, C, dtype=d_out.dtype)
    dz.scatter_(1, arg.long()[:, None, :], torch.where(out > 0, d_out, torch.zeros_like(d_out))[:, None, :])
    return dz.view(G * n, C)


# ------------------------------------------------------------------------------------------------- the 'anchor' grouping's backward
def gnb_case(B, n, S, k, D, seed=None, bf16=False):
    """Crafted operands: every centre is among its own neighbours (slot 0), point `all` sits in every group (slot 1), point `none` in no
    group and is no centre -> dict(feat, xyz, fi, ki, alpha, dU [B S k, 2 D + 3], all, none)."""
    g = torch.Generator().manual_seed(9000 + 17 * n + D if seed is None else seed)
    feat = torch.randn(B, n, D, generator=g) * 0.7 * (1 + torch.arange(B).float()[:, None, None] * 0.5)
    xyz = torch.randn(B, n, 3, generator=g) * 0.4
    p_all, p_none = 1 % n, n - 1
    fi = torch.stack([torch.randperm(n - 1, generator=g)[:S] for _ in range(B)])                  # distinct centres, never `none`
    ki = torch.randint(0, n - 1, (B, S, k), generator=g)
    ki[:, :, 0] = fi
    if k > 1:
        ki[:, :, 1] = p_all
    alpha = torch.rand(D + 3, generator=g) + 0.5
    dU = torch.randn(B * S * k, 2 * D + 3, generator=g)
    if bf16:
        dU = dU.bfloat16()
    return dict(feat=feat, xyz=xyz, fi=fi.int(), ki=ki.int(), alpha=alpha, dU=dU, all=p_all, none=p_none, B=B, n=n, S=S, k=k, D=D)


def group_forward64(feat, xyz, fi, ki, alpha, beta):
    """U [B, S, k, 2 D + 3] of LocalGrouper ('anchor', layers.py:297-315) in the operands' dtype, differentiable."""
    G = torch.cat([kc._take(feat, ki.long()), kc._take(xyz, ki.long())], -1)
    anchor = torch.cat([kc._take(feat, fi.long()), kc._take(xyz, fi.long())], -1)[:, :, None]
    d = G - anchor
    B = feat.shape[0]
    std = torch.std(d.reshape(B, -1), dim=-1)[:, None, None, None]
    un = alpha * (d / (std + kc.EPS_STD)) + beta
    D = feat.shape[2]
    return torch.cat([un, anchor[..., :D].expand(-1, -1, ki.shape[2], -1)], -1)


GNB_FAULTS = ("anchor's -sum_j dd dropped", "P term dropped", "biased sigma")


def group_normalize_bwd_ref(c, fault=None):
    """float64 of the formulas in include/ldt_hip.h -> ((dalpha, dbeta, dfeat), their bounds).  fault: one of GNB_FAULTS planted (then the
    bounds are meaningless)."""
    assert fault is None or fault in GNB_FAULTS
    feat, xyz, fi, ki, alpha = c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"]
    B, n, D = feat.shape
    S, k = ki.shape[1], ki.shape[2]
    D3, n_el = D + 3, S * k * (D + 3)
    gr = kc.group_reference(feat, xyz, fi, ki, alpha, torch.zeros(D3))
    dU = c["dU"].double().view(B, S, k, -1)
    f, x, fl, kl = feat.double(), xyz.double(), fi.long(), ki.long()
    d = torch.cat([kc._take(f, kl), kc._take(x, kl)], -1) - torch.cat([kc._take(f, fl), kc._take(x, fl)], -1)[:, :, None]
    red = lambda t: t.sum((1, 2, 3))
    m = red(d) / n_el
    var = red((d - m[:, None, None, None]) ** 2) / (n_el if fault == "biased sigma" else n_el - 1)
    sigma = var.sqrt()
    inv = 1 / (sigma + kc.EPS_STD)
    rho = gr["rho"]
    u1 = dU[..., :D3]
    al = alpha.double()
    s_a, abs_a = (u1 * d).sum((1, 2)), (u1 * d).abs().sum((1, 2))                                   # [B, D3]
    dbeta = u1.sum((0, 1, 2))
    tol_dbeta = (dbeta.abs() * U24 + B * S * k * U53 * u1.abs().sum((0, 1, 2))) * SLACK
    dalpha = (inv[:, None] * s_a).sum(0)
    d_sa = (U24 + S * k * U53) * abs_a
    tol_dalpha = (dalpha.abs() * U24 + (inv[:, None] * (rho[:, None] * s_a.abs() + d_sa)).sum(0)) * SLACK
    P = (al * s_a).sum(1)
    d_P = (al.abs() * d_sa).sum(1) + D3 * U53 * (al * s_a).abs().sum(1)
    q = al * u1
    iv, mm = inv[:, None, None, None], m[:, None, None, None]
    cB = torch.where(sigma > 0, P * inv ** 2 / ((n_el - 1) * sigma), torch.zeros_like(P))
    if fault == "P term dropped":
        cB = torch.zeros_like(cB)
    d_cB = torch.where(sigma > 0, cB.abs() * (2 * rho + rho / (inv * sigma).clamp_min(1e-300)) + d_P * inv ** 2 / ((n_el - 1) * sigma), torch.zeros_like(P))
    dd = q * iv - cB[:, None, None, None] * (d - mm)
    tol_dd = ((q * iv).abs() * rho[:, None, None, None] + d_cB[:, None, None, None] * (d - mm).abs()
              + cB.abs()[:, None, None, None] * (U24 * d.abs() + (gr["tol1"] / n_el)[:, None, None, None]) + 4 * U53 * ((q * iv).abs() + (cB[:, None, None, None] * (d - mm)).abs()))
    u2 = dU[..., D3:D3 + D]
    dfeat, tol, mag = torch.zeros(B, n, D, dtype=torch.float64), torch.zeros(B, n, D, dtype=torch.float64), torch.zeros(B, n, D, dtype=torch.float64)
    for b in range(B):
        idx = kl[b].reshape(-1)
        dfeat[b].index_add_(0, idx, dd[b, ..., :D].reshape(-1, D))
        tol[b].index_add_(0, idx, tol_dd[b, ..., :D].reshape(-1, D))
        mag[b].index_add_(0, idx, dd[b, ..., :D].abs().reshape(-1, D))
        back = u2[b].sum(1) if fault == "anchor's -sum_j dd dropped" else u2[b].sum(1) - dd[b, ..., :D].sum(1)
        dfeat[b].index_add_(0, fl[b], back)
        tol[b].index_add_(0, fl[b], tol_dd[b, ..., :D].sum(1))
        mag[b].index_add_(0, fl[b], dd[b, ..., :D].abs().sum(1) + u2[b].abs().sum(1))
    tol_dfeat = (tol + U24 * dfeat.abs() + (S + k + 2) * U53 * mag) * SLACK
    return (dalpha, dbeta, dfeat), (tol_dalpha, tol_dbeta, tol_dfeat)


# ------------------------------------------------------------------------------------------------- the front, restated (Network.py:189-198)
class _Round(torch.autograd.Function):
    """bf16 rounding of a GEMM operand, forward and backward (the twin: the device's GEMMs round their operands in both directions)."""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().to(g.dtype)


def _lin(x, w, b, twin):
    """x [rows, K] @ w [N, K]^T + b; twin: both operands rounded to bf16, and the gradient arriving at the product too."""
    if twin:
        return _Round.apply(x) @ _Round.apply(w).t() + b
    return x @ w.t() + b


def _bn_train(x, gamma, beta, eps=BN_EPS):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return gamma * ((x - mean) / torch.sqrt(var + eps)) + beta, mean, var


def _relu_sel(pre, mask):
    """ReLU at a pinned selection (mask None: its own) -> (y, the mask)."""
    if mask is None:
        mask = pre.detach() > 0
    return pre * mask.to(pre.dtype), mask


def _max_sel(h, arg, dim=1):
    """max over `dim` at a pinned arg-max (None: its own, the first index on equal values) -> (values, arg)."""
    if arg is None:
        top = h.detach().max(dim, keepdim=True).values
        arg = (h.detach() == top).int().argmax(dim)
    return torch.gather(h, dim, arg.long().unsqueeze(dim)).squeeze(dim), arg


FRONT_SELECTIONS = ("mask1", "mask2", "mask3", "arg", "pmask1", "pmask2", "parg")


def w2(sd, name):
    w = sd[name]
    return w.reshape(w.shape[0], -1)


def front(sd, cfg, cloud, fps_idx, knn_idx, sel=None, twin=False):
    """The Compressor's front in TRAINING mode from a state_dict (dtype: its own), token-major: cloud [B, N, 3] (already normalised when
    cfg.norm_input) with the device's (or the oracle's) fps_idx / knn_idx -> (tokens [B, T, D] before ActNorm, pos [B, p_dim],
    the selections it ran at, {bn prefix: (batch mean, biased batch variance, rows)}).  sel: a dict of FRONT_SELECTIONS to pin (missing or None
    entries: its own).  twin: the three PreExtraction GEMMs on bf16-rounded operands (the fp32 linears stay fp32, as on the device)."""
    sel = dict(sel or {})
    B, N, _ = cloud.shape
    D, T = cfg.hidden_dim, cfg.z_scales
    k = knn_idx.shape[2]
    feat = (cloud.reshape(B * N, 3) @ w2(sd, "input.weight").t() + sd["input.bias"]).view(B, N, D)
    U = group_forward64(feat, cloud, fps_idx, knn_idx, sd["group.affine_alpha"].reshape(-1), sd["group.affine_beta"].reshape(-1))
    if twin:
        U = U + (U.detach().bfloat16().to(U.dtype) - U.detach())                                   # the grouped rows are stored as bf16
    U = U.reshape(B * T * k, -1)
    ex, bns, out = "group.extraction.", {}, {}
    z1 = _lin(U, w2(sd, ex + "transfer.net.0.weight"), sd[ex + "transfer.net.0.bias"], twin)
    p1, mu, var = _bn_train(z1, sd[ex + "transfer.net.1.weight"], sd[ex + "transfer.net.1.bias"])
    bns[ex + "transfer.net.1"] = (mu.detach(), var.detach(), z1.shape[0])
    h1, out["mask1"] = _relu_sel(p1, sel.get("mask1"))
    z2 = _lin(h1, w2(sd, ex + "operation.0.net1.0.weight"), sd[ex + "operation.0.net1.0.bias"], twin)
    p2, mu, var = _bn_train(z2, sd[ex + "operation.0.net1.1.weight"], sd[ex + "operation.0.net1.1.bias"])
    bns[ex + "operation.0.net1.1"] = (mu.detach(), var.detach(), z2.shape[0])
    r, out["mask2"] = _relu_sel(p2, sel.get("mask2"))
    z3 = _lin(r, w2(sd, ex + "operation.0.net2.0.weight"), sd[ex + "operation.0.net2.0.bias"], twin) + h1
    # max_j ReLU(z3_j) = ReLU(max_j z3_j): the same function and the same gradient (a cell whose every row is <= 0 passes none either way);
    # in this order the arg-max is a selection among distinct values and the last ReLU's mask has one cell per (group, channel)
    top, out["arg"] = _max_sel(z3.view(B * T, k, D), sel.get("arg"))
    tok, out["mask3"] = _relu_sel(top, sel.get("mask3"))
    pe = "pos_embedding."
    ctr = kc._take(cloud, fps_idx.long()).reshape(B * T, 3)
    y1 = ctr @ w2(sd, pe + "conv1.weight").t() + sd[pe + "conv1.bias"]
    q1, mu, var = _bn_train(y1, sd[pe + "bn1.weight"], sd[pe + "bn1.bias"])
    bns[pe + "bn1"] = (mu.detach(), var.detach(), y1.shape[0])
    a1, out["pmask1"] = _relu_sel(q1, sel.get("pmask1"))
    y2 = a1 @ w2(sd, pe + "conv2.weight").t() + sd[pe + "conv2.bias"]
    q2, mu, var = _bn_train(y2, sd[pe + "bn2.weight"], sd[pe + "bn2.bias"])
    bns[pe + "bn2"] = (mu.detach(), var.detach(), y2.shape[0])
    a2, out["pmask2"] = _relu_sel(q2, sel.get("pmask2"))
    pool, out["parg"] = _max_sel(a2.view(B, T, -1), sel.get("parg"))
    pos = pool @ sd[pe + "fc.weight"].t() + sd[pe + "fc.bias"]
    return tok.view(B, T, D), pos, out, bns


# Parameters of the front whose gradient is analytically ZERO in training mode: a bias in front of a BatchNorm, and affine_beta and the input
# conv's bias, each of which shifts every row of some columns of U by one constant (the bias cancels in g - anchor and stays in the anchor
# columns) that the transfer conv's BatchNorm removes.  Both sides hold rounding noise there; the tests bound it against the live gradient
# next to it instead of comparing noise with noise.
FRONT_DEAD = {"group.extraction.transfer.net.0.bias": "group.extraction.transfer.net.0.weight",
              "group.extraction.operation.0.net1.0.bias": "group.extraction.operation.0.net1.0.weight",
              "pos_embedding.conv1.bias": "pos_embedding.conv1.weight", "pos_embedding.conv2.bias": "pos_embedding.conv2.weight",
              "group.affine_beta": "group.affine_alpha", "input.bias": "input.weight"}


def front_names(sd):
    return [k for k in sd if k.split(".")[0] in ("input", "group", "pos_embedding") and sd[k].is_floating_point()
            and not k.endswith(("running_mean", "running_var"))]


def front_step(init, cfg, cloud, fps_idx, knn_idx, d_tokens, d_pos, dtype, sel=None, twin=False):
    """front + autograd of <d_tokens, tokens> + <d_pos, pos> on a copy of the weights -> ({name: grad}, tokens, pos, selections, bns)."""
    names = front_names(init)
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    tok, pos, s, bns = front(sd, cfg, cloud.to(dtype), fps_idx, knn_idx, sel, twin)
    torch.autograd.backward([tok, pos], [d_tokens.to(dtype), d_pos.to(dtype)])
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in zip(names, leaves)}
    return grads, tok.detach(), pos.detach(), s, bns


def whole_step(init, cfg, names, cloud, fps_idx, knn_idx, post_noise, target, dtype, kl_weight, sel=None, twin=False, d_set=None, keep_mask=None):
    """front -> encoder -> top_down -> kl_weight * cat(kls).mean() + CD_loss('l1') + autograd on a copy of the weights (names: every
    trained parameter) -> ({name: grad, 'd_tokens', 'd_pos', 'd_set'}, (loss, kl_loss, rec_loss), tokens, pos, selections, bns).  twin: the
    front's GEMM operands rounded to bf16 and the rest under torch.autocast("cpu", bfloat16), as encoder_train_checks.chain_step's twin.
    d_set: the gradient with respect to the set to start the reconstruction path from, in place of this run's own."""
    import decoder_train_checks as dc
    import encoder_train_checks as ec
    import topdown_train_checks as tc
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    tok, pos, s, bns = front(sd, cfg, cloud.to(dtype), fps_idx, knn_idx, sel, twin)
    tok.retain_grad(); pos.retain_grad()
    nz = [t.detach().to(dtype) for t in post_noise]
    with torch.autocast("cpu", torch.bfloat16, enabled=twin):
        outs = ec.encoder(sd, cfg, tok, pos)
        pts, all_eps, kls = tc.top_down(sd, cfg, outs, nz, keep_mask=keep_mask)
    pts.retain_grad()
    kl_loss = torch.cat([k.to(dtype) for k in kls], dim=1).mean()
    rec_loss = dc.cd_loss_torch(pts.to(dtype), target.to(dtype), "l1")
    if d_set is None:
        (kl_weight * kl_loss + rec_loss).backward()
        d_own = pts.grad
    else:
        (d_own,) = torch.autograd.grad(rec_loss, pts, retain_graph=True)
        torch.autograd.backward([pts, kl_weight * kl_loss], [d_set.to(pts.dtype), torch.ones((), dtype=kl_loss.dtype)])
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in zip(names, leaves)}
    grads["d_tokens"], grads["d_pos"], grads["d_set"] = tok.grad, pos.grad, d_own
    losses = (float((kl_weight * kl_loss + rec_loss).detach()), float(kl_loss.detach()), float(rec_loss.detach()))
    return grads, losses, tok.detach(), pos.detach(), s, bns


def running_after(init, bns, momentum=BN_MOMENTUM):
    """The four BatchNorms' buffers after one training step, float64, as nn.BatchNorm1d updates them."""
    out = {}
    for p, (mu, var, rows) in bns.items():
        out[p + ".running_mean"] = (1 - momentum) * init[p + ".running_mean"].double() + momentum * mu.double()
        out[p + ".running_var"] = (1 - momentum) * init[p + ".running_var"].double() + momentum * var.double() * rows / (rows - 1)
        out[p + ".num_batches_tracked"] = init[p + ".num_batches_tracked"] + 1
    return out


def selection_shares(a, b):
    """-> {selection: share of cells on which a and b disagree}."""
    return {k: float((a[k] != b[k]).double().mean()) for k in FRONT_SELECTIONS}
