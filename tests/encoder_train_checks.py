"""Helpers of the encoder training tests (test_encoder_train_host.py, test_gpu_actnorm_bwd.py, test_gpu_encoder_train.py,
tools/gen_encoder_train_golden.py): the float64 reference of the ActNorm backward with componentwise bounds, an fp32 emulation of the
kernel's arithmetic with the faults the host test plants, and the float64 restatement of the encoder from the oracle's pieces with its
bf16 twin.  None of a bound is taken from what a kernel returned.

ActNorm backward (csrc/actnorm.hip, ldt_actnorm_bwd), counted from the kernel's operation order:
  dx[b][i] = fl(dz[b][i] * expf(-log_scale[i])): the negation is exact, expf is within LIBM["expf"] ulp of its result, the product is one
    rounding; the bound allows two roundings plus the libm constant, relative to |dz exp(-log_scale)|.
  dshift[i] = -sum_b dx[b][i]: the kernel adds the fp32 values it stored, in float64, and rounds once: one final rounding of |dshift| plus
    the summed bounds of the terms, plus B float64 roundings of the running sum (2^-53 each, of at most sum_b |dx|).
  dlog_scale[i] = -sum_b dz[b][i] z[b][i]: each product of two fp32 factors is exact in float64 (24 + 24 bits), so a term carries no bound
    of its own: one final rounding of |dlog_scale| plus the float64 roundings of the running sum.

The encoder (ldt_amd/compressor_train.py: EncoderTrainStep): `encoder` restates Network.py:200-205 with O.act_norm, O.residual_block
(y = the raw x, c = pos) and O.final_layer; `encoder_step` differentiates <d_enc_out, enc_out>; `chain_step` puts it in front of
topdown_train_checks.top_down with the stage-1 loss.  autocast=True is the bf16 twin of the project's yardstick (DESIGN.md sections 4.11 /
4.15)."""
import torch

import kernel_checks as kc
from kernel_checks import LIBM, SLACK, U24, ULP32

U53 = 2.0 ** -53
# (B, per_sample): one sample and an odd width; the tiny fixture's 8 tokens x 64; the shipped 32 x 128 at B 16; a width that is no multiple
# of 4 (the scalar form, with a tail behind the last full group of 16 columns); the 'set' form (per_sample = C) past one workgroup's 512 rows
# (two stages: 2 and 10 partials, the last one partial)
ANB_CASES = [(1, 5), (3, 8 * 64), (16, 32 * 128), (2, 4101), (700, 64), (5000, 64)]
ANB_ROWS = 512                     # csrc/actnorm.hip: rows per workgroup; more rows take the second stage


def actnorm_case(B, per, ls_max=1.0, seed=None, big_sample=None):
    """-> dict(x, shift, log_scale, z, dz), fp32: x the forward's input, z = (x - shift) * exp(-log_scale) as fp32 torch forms it (what the
    tape holds), log_scale uniform in [-ls_max, ls_max] with both ends present.  big_sample: that sample's dz is 2^20 times the others'."""
    g = torch.Generator().manual_seed(1000 * B + per if seed is None else seed)
    x = torch.randn(B, per, generator=g) * 1.5 + 0.3
    shift = torch.randn(per, generator=g) * 0.5
    ls = (torch.rand(per, generator=g) * 2 - 1) * ls_max
    ls[0], ls[-1] = ls_max, -ls_max
    dz = torch.randn(B, per, generator=g)
    if big_sample is not None:
        dz[big_sample] *= 2.0 ** 20
    z = (x - shift) * torch.exp(-ls)
    return {"x": x, "shift": shift, "log_scale": ls, "z": z, "dz": dz}


def actnorm_bwd_ref(dz, z, log_scale):
    """float64 -> ((dx, dshift, dlog_scale), (tol_dx, tol_dshift, tol_dlog_scale)): the bounds of the module text."""
    B = dz.shape[0]
    dz64, z64, e = dz.double(), z.double(), torch.exp(-log_scale.double())
    dx = dz64 * e
    dshift = -dx.sum(0)
    dls = -(dz64 * z64).sum(0)
    tol_dx = dx.abs() * (2 * U24 + LIBM["expf"] * ULP32) * SLACK
    tol_dshift = (dshift.abs() * U24 + tol_dx.sum(0) + B * U53 * dx.abs().sum(0)) * SLACK
    tol_dls = (dls.abs() * U24 + B * U53 * (dz64 * z64).abs().sum(0)) * SLACK
    return (dx, dshift, dls), (tol_dx, tol_dshift, tol_dls)


ANB_FAULTS = ("wrong sign on dshift", "x instead of z in dlog_scale", "exp(+log_scale)", "last sample dropped from the sums",
              "fp32 running sums")


def actnorm_bwd_emulate(dz, z, log_scale, x=None, fault=None):
    """The kernel's arithmetic on the CPU: fp32 expf and product, float64 sums rounded once -> (dx, dshift, dlog_scale) fp32, with one of
    ANB_FAULTS planted (x: the forward's input, for the fault that reads it)."""
    assert fault is None or fault in ANB_FAULTS
    e = torch.exp(log_scale if fault == "exp(+log_scale)" else -log_scale)
    dx = dz * e
    other = x if fault == "x instead of z in dlog_scale" else z
    n = dz.shape[0] - 1 if fault == "last sample dropped from the sums" and dz.shape[0] > 1 else dz.shape[0]
    if fault == "fp32 running sums":
        s, t = torch.zeros_like(dx[0]), torch.zeros_like(dx[0])
        for b in range(n):
            s = s + dx[b]
            t = t + dz[b] * other[b]
        dshift, dls = -s, -t
    else:
        dshift = (-dx[:n].double().sum(0)).float()
        dls = (-(dz[:n].double() * other[:n].double()).sum(0)).float()
    if fault == "wrong sign on dshift":
        dshift = -dshift
    return dx, dshift, dls


def actnorm_worst(got, ref, tol, what):
    """max err / tol over the three outputs, each held per element (kernel_checks.assert_elementwise) -> (dx, dshift, dlog_scale) ratios."""
    return tuple(kc.assert_elementwise(g, r, t, "%s %s" % (what, n)) for g, r, t, n in zip(got, ref, tol, ("dx", "dshift", "dlog_scale")))


def actnorm_ratio(got, ref, tol):
    """max err / tol over the three outputs without asserting (the planted faults)."""
    out = 0.0
    for g, r, t in zip(got, ref, tol):
        err = (g.double() - r).abs()
        out = max(out, float(torch.where(err == 0, torch.zeros_like(err), err / t).max()))
    return out


# ---- the encoder: the float64 restatement and its bf16 twin
def encoder(sd, cfg, tokens, pos):
    """Network.py:200-205 from the oracle's pieces, token-major: tokens [B, T, C] before ActNorm, pos [B, p_dim] -> the n_layers stage
    outputs [B, T, C]."""
    from oracle import ldt_oracle as O
    nk = getattr(cfg, "norm", "layer_norm")
    x = tokens
    if getattr(cfg, "ActNorm", True) is not None:
        x = O.act_norm(sd, "conv_in", x)
    outs = []
    for i in range(cfg.n_layers):
        for j in range(cfg.encoder_layers):
            x = O.residual_block(sd, "encoder.%d.atts.%d" % (i, j), x, x, pos, cfg.num_heads, norm=nk)     # y = the raw x (quirk Q2)
        outs.append(O.final_layer(sd, "encoder.%d.conv_out" % i, x, pos, norm=nk))
    return outs


def _leaves(init, names, dtype):
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()}
    return sd, [sd[n].requires_grad_(True) for n in names]


def encoder_step(init, ccfg, names, tokens, pos, d_enc_out, dtype, autocast=False):
    """encoder + autograd of sum_i <d_enc_out[i], enc_out[i]> on a copy of the weights -> ({name: grad, 'd_tokens', 'd_pos'}, enc_out)."""
    sd, leaves = _leaves(init, names, dtype)
    tk = tokens.detach().clone().to(dtype).requires_grad_(True)
    ps = pos.detach().clone().to(dtype).requires_grad_(True)
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        outs = encoder(sd, ccfg, tk, ps)
    torch.autograd.backward(outs, [d.detach().to(o.dtype) for d, o in zip(d_enc_out, outs)])
    grads = {n: p.grad for n, p in zip(names, leaves)}
    grads["d_tokens"], grads["d_pos"] = tk.grad, ps.grad
    return grads, [o.detach() for o in outs]


def chain_step(init, ccfg, names, tokens, pos, post_noise, target, dtype, kl_weight, autocast=False, d_set=None, keep_mask=None):
    """encoder -> top_down -> kl_weight * cat(kls).mean() + CD_loss('l1') + autograd on a copy of the weights (names: the encoder's and the
    top-down parameters) -> ({name: grad, 'd_enc_out.i', 'd_tokens', 'd_pos', 'd_set': d rec_loss / d set}, (loss, kl_loss, rec_loss), set,
    all_eps, enc_out).  d_set: the gradient with respect to the set to start the reconstruction path from, in place of this run's own."""
    import decoder_train_checks as dc
    import topdown_train_checks as tc
    sd, leaves = _leaves(init, names, dtype)
    tk = tokens.detach().clone().to(dtype).requires_grad_(True)
    ps = pos.detach().clone().to(dtype).requires_grad_(True)
    nz = [t.detach().to(dtype) for t in post_noise]
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        outs = encoder(sd, ccfg, tk, ps)
        for o in outs:
            o.retain_grad()
        pts, all_eps, kls = tc.top_down(sd, ccfg, outs, nz, keep_mask=keep_mask)
    pts.retain_grad()
    kl_loss = torch.cat([k.to(dtype) for k in kls], dim=1).mean()
    rec_loss = dc.cd_loss_torch(pts.to(dtype), target.to(dtype), "l1")
    if d_set is None:
        (kl_weight * kl_loss + rec_loss).backward()
        d_own = pts.grad
    else:
        (d_own,) = torch.autograd.grad(rec_loss, pts, retain_graph=True)
        torch.autograd.backward([pts, kl_weight * kl_loss], [d_set.to(pts.dtype), torch.ones((), dtype=kl_loss.dtype)])
    grads = {n: p.grad for n, p in zip(names, leaves)}
    grads.update({"d_enc_out.%d" % i: o.grad for i, o in enumerate(outs)})
    grads["d_tokens"], grads["d_pos"], grads["d_set"] = tk.grad, ps.grad, d_own
    losses = (float((kl_weight * kl_loss + rec_loss).detach()), float(kl_loss.detach()), float(rec_loss.detach()))
    return grads, losses, pts.detach(), all_eps.detach(), [o.detach() for o in outs]


def perturb_actnorm(sd, seed=77):
    """ActNorm away from its init() state (shift = log_scale = 0: the identity): shift 0.1 randn, log_scale 0.2 randn from a seeded
    generator, written into the state_dict in place -> (shift, log_scale)."""
    g = torch.Generator().manual_seed(seed)
    sh, ls = sd["conv_in.shift"], sd["conv_in.log_scale"]
    sd["conv_in.shift"] = (0.1 * torch.randn(sh.shape, generator=g)).to(sh.dtype)
    sd["conv_in.log_scale"] = (0.2 * torch.randn(ls.shape, generator=g)).to(ls.dtype)
    return sd["conv_in.shift"], sd["conv_in.log_scale"]
