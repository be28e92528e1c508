"""Helpers of the top-down training kernel tests (test_topdown_train_host.py, test_gpu_attention_bwd_wide.py, test_gpu_reparam_kl_bwd.py):
float64 references with componentwise bounds, and fp32 emulations of the kernels' arithmetic with the faults the host test plants.  None
of a bound is taken from what a kernel returned.

Attention backward on a long key axis (csrc/attention_bwd.hip, ldt_attention_bwd_wide)
  kernel_checks.attn_bwd_ref at head width 32 with P and dS rounded, plus, when there is more than one chunk of CHUNK keys:
  * on dQ, the one fp32 sum of the chunks' partials: (chunks - 1) 2^-24 scale times the sum of the partials' magnitudes, itself at most
    |dS| |K|;
  * on all three outputs, the extra roundings of L.  The direct form takes L = m + ln(sum).  The chunked form takes
    L = M + ln sum_c s_c exp(m_c - M): per chunk one subtraction (its rounding moves the term by at most |m_c - M| exp(m_c - M) 2^-24 <=
    2^-24 / e of the total), one expf (LIBM_ABS, of a value <= 1), one product; then chunks - 1 additions, each rounding at most the
    total.  The argument of the logarithm is therefore off by at most E_L = (chunks + 3) 2^-24 + LIBM_ABS relative, and so is L in
    absolute terms.  L enters every P = exp(s - L) as a relative error E_L, and through P every dS: E_L scale |dS| |K| on dQ,
    E_L scale |dS|^T |Q| on dK, E_L P^T |dO| on dV.
Backward of the posterior draw and the KL term (csrc/eval_loss.hip, ldt_reparam_kl_bwd)
  the reference is float64 autograd over the reference's own expressions (Network.py:12-29, 221-224); the kernel's closed form rounds, per
  element: lv / 2 and expf (EXP_ROUNDINGS on s, relative), the product s n (1), eps's fused multiply-add (1 on |eps|), g's (1 on |g|),
  the halving (exact), dlv's fused multiply-add (1 on |dlv|): counted in `reparam_kl_bwd_ref`."""
import torch

import kernel_checks as kc
from kernel_checks import LIBM_ABS, SLACK, U24, attn_bwd_ref

CHUNK = 256                        # LDT_ATTN_BWD_WIDE_CHUNK
# (B, H, Nq, Nk) at head width 32: decoder_train_checks.LONG_SHAPES mirrored
WIDE_SHAPES = [(1, 2, 8, 16), (2, 2, 32, 296), (1, 4, 72, 552), (1, 1, 32, 2048)]
UNDERFLOW_SHAPE = (1, 2, 24, 520)  # chunk 1's scores at least 40 above chunk 0's


def wide_case(B, H, Nq, Nk, seed=None):
    """-> (q bf16 [B Nq, H 32], kv bf16 [B Nk, 2 H 32] = K | V, dO bf16 [B, H, Nq, 32])"""
    import cross_bwd_checks as cb
    return cb.cross_case(B, H, Nq, Nk, 32, False, seed)


def underflow_case(seed=None):
    """UNDERFLOW_SHAPE with every query pulled towards one direction u per head and the keys of chunk 1 (256 .. 511) pushed along u, the
    others against it: every score of chunk 1 is at least 40 above every score of chunk 0, so exp(m_0 - M) contributes nothing that fp32
    holds next to chunk 1's sum (exp(-40) < 2^-57).  -> (q, kv, dO, the least margin in float64)."""
    import narrow_bwd_checks as nb
    B, H, Nq, Nk = UNDERFLOW_SHAPE
    q, kv, do = wide_case(B, H, Nq, Nk, seed)
    C = H * 32
    g = torch.Generator().manual_seed(77)
    u = torch.nn.functional.normalize(torch.randn(H, 32, generator=g), dim=-1)
    q4 = q.float().view(B, Nq, H, 32) * 0.25 + 8.0 * u
    k4 = kv[:, :C].float().view(B, Nk, H, 32) * 0.25
    sign = torch.full((Nk,), -1.0)
    sign[CHUNK:2 * CHUNK] = 1.0
    k4 = k4 + (24.0 * sign)[None, :, None, None] * u
    q, kv = nb.bf(q4.reshape(B * Nq, C)), torch.cat([nb.bf(k4.reshape(B * Nk, C)), kv[:, C:]], 1)
    s = nb.scores64(q, kv, B, H, Nq, Nk, 32)
    margin = float((s[..., CHUNK:2 * CHUNK].min(-1).values - torch.cat([s[..., :CHUNK], s[..., 2 * CHUNK:]], -1).max(-1).values).min())
    return q, kv, do, margin


def score_err(q, kv, B, H, Nq, Nk):
    """A bound [B, H, Nq] on the error of any fp32 logit of a query row: the MFMA sum of 32 products (C_ACC 32 2^-24 |q| . |k|), the scale
    and one more rounding (2 x 2^-24 |s|), at the row's largest."""
    import narrow_bwd_checks as nb
    C = H * 32
    qk = nb.heads(q.double().abs(), B, H, Nq, 32) @ nb.heads(kv[:, :C].double().abs(), B, H, Nk, 32).transpose(-1, -2) * 32 ** -0.5
    return (kc.C_ACC * 32 * U24 * qk.max(-1).values + 2 * U24 * nb.scores64(q, kv, B, H, Nq, Nk, 32).abs().max(-1).values) * SLACK


def lse_err(q, kv, B, H, Nq, Nk, keys, chunks):
    """A bound [B, H, Nq] on the kernels' L = max + ln(sum) against float64: the logits' error (it moves L by at most itself), the sum of
    `keys` exponentials as the kernel adds them (keys / 16 per lane, then 4 shuffle steps, each rounding at most the total; expf LIBM_ABS
    each of a value <= 1), logf (LIBM_ABS), the last addition (2^-24 |L|), and the chunked combination's E_L of the module docstring."""
    import narrow_bwd_checks as nb
    L = torch.logsumexp(nb.scores64(q, kv, B, H, Nq, Nk, 32), -1)
    e_l = ((chunks + 3) * U24 + LIBM_ABS) if chunks > 1 else 0.0
    return (score_err(q, kv, B, H, Nq, Nk) + (-(-keys // 16) + 4) * U24 + 2 * LIBM_ABS + U24 * L.abs() + e_l) * SLACK


def wide_ref(q, kv, o, do, B, H, Nq, Nk, chunk=CHUNK):
    """-> (references, bounds) of dq [B, H, Nq, 32], dk, dv [B, H, Nk, 32]: attn_bwd_ref plus the terms of the module docstring."""
    Dh, C = 32, H * 32
    q, kv, o, do = q.cpu(), kv.cpu(), o.cpu(), do.cpu()
    ref, tol = attn_bwd_ref(q, kv[:, :C], kv[:, C:], o, do, B, H, Nq, Nk, Dh, True)
    chunks = -(-Nk // chunk)
    if chunks > 1:
        q4, k4, v4 = kc.heads(q, B, Nq, H, Dh), kc.heads(kv[:, :C], B, Nk, H, Dh), kc.heads(kv[:, C:], B, Nk, H, Dh)
        o6, g6, sc = o.double(), do.double(), Dh ** -0.5
        P = torch.softmax(q4 @ k4.transpose(-1, -2) * sc, -1)
        dS = P * (g6 @ v4.transpose(-1, -2) - (g6 * o6).sum(-1, keepdim=True))
        e_l = ((chunks + 3) * U24 + LIBM_ABS) * SLACK
        tol = dict(tol)
        tol["dq"] = tol["dq"] + ((chunks - 1) * U24 + e_l) * sc * (dS.abs() @ k4.abs())
        tol["dk"] = tol["dk"] + e_l * sc * (dS.abs().transpose(-1, -2) @ q4.abs())
        tol["dv"] = tol["dv"] + e_l * (P.transpose(-1, -2) @ g6.abs())
    return ref, tol


def wide_check(got, q, kv, o, do, B, H, Nq, Nk, what):
    """got: {'dq' rows [B Nq, H 32], 'dk', 'dv' rows [B Nk, H 32]} -> {name: worst err / tol}; fails naming the output."""
    import narrow_bwd_checks as nb
    ref, tol = wide_ref(q, kv, o, do, B, H, Nq, Nk)
    n = {"dq": Nq, "dk": Nk, "dv": Nk}
    return {nm: kc.assert_elementwise(nb.heads(got[nm].cpu(), B, H, n[nm], 32), ref[nm], tol[nm], "%s %s" % (what, nm)) for nm in ("dq", "dk", "dv")}


WIDE_FAULTS = ("a chunk's partial dropped from dq", "chunk sums combined without exp(m_c - M)", "partials added unscaled")


def wide_emulate(q, kv, o, do, B, H, Nq, Nk, chunk=CHUNK, fault=None):
    """The kernels' arithmetic in fp32: each chunk's (maximum, sum), combined in chunk order into L; dQ summed per chunk of keys and the
    partials added in chunk order; dK / dV whole -> bf16 rows like narrow_bwd_checks.emulate, and L [B, H, Nq, 1] fp32."""
    import narrow_bwd_checks as nb
    assert fault is None or fault in WIDE_FAULTS
    Dh, C = 32, H * 32
    bf = nb.bf
    q4, k, v = nb.heads(q.float(), B, H, Nq, Dh), nb.heads(kv[:, :C].float(), B, H, Nk, Dh), nb.heads(kv[:, C:].float(), B, H, Nk, Dh)
    g32, o32 = do.float(), o.float()
    sc = float(torch.tensor(float(Dh)).rsqrt())
    s = q4 @ k.transpose(-1, -2) * sc
    chunks = -(-Nk // chunk)
    cut = [(c * chunk, min((c + 1) * chunk, Nk)) for c in range(chunks)]
    m_c = [s[..., lo:hi].max(-1, keepdim=True).values for lo, hi in cut]
    s_c = [torch.exp(s[..., lo:hi] - m).sum(-1, keepdim=True) for (lo, hi), m in zip(cut, m_c)]
    M = torch.stack(m_c).max(0).values
    tot = torch.zeros_like(M)
    for m, sm in zip(m_c, s_c):
        tot = tot + (sm if fault == "chunk sums combined without exp(m_c - M)" else sm * torch.exp(m - M))
    L = M + torch.log(tot)
    P = torch.exp(s - L)
    dS = P * (g32 @ v.transpose(-1, -2) - (g32 * o32).sum(-1, keepdim=True))
    P, dS = bf(P).float(), bf(dS).float()
    dq = torch.zeros(B, H, Nq, Dh)
    for c, (lo, hi) in enumerate(cut):
        if not (fault == "a chunk's partial dropped from dq" and c == chunks // 2):
            dq = dq + dS[..., lo:hi] @ k[:, :, lo:hi]
    out = {"dq": dq * (1.0 if fault == "partials added unscaled" else sc), "dk": dS.transpose(-1, -2) @ q4 * sc, "dv": P.transpose(-1, -2) @ g32}
    return {nm: bf(z).permute(0, 2, 1, 3).reshape(-1, C) for nm, z in out.items()}, L


# ---- backward of the posterior draw and the KL term
LOG_SQRT_2PI = 0.9189385332        # the constant as the reference writes it (Network.py:13, 18)
EXP_ROUNDINGS = 4                  # s = expf(lv / 2): the halving is exact, expf within a few ulp
# (rows, z): 16-byte form, scalar form (z odd), the shipped rows x z
RKB_SHAPES = [(24, 40), (7, 5), (512, 20)]


def rkb_case(rows, z, lo=-6.0, hi=10.0, seed=None):
    """-> (post fp32 [rows, 2 z] = mu | logvar, noise [rows, z], d_eps [rows, z]).  The first row's logvar holds elements below lo, above
    hi and exactly on both bounds; the rest spread over [lo - 2, hi + 2] so that both sides of the clamp occur everywhere."""
    g = torch.Generator().manual_seed(31 * rows + z if seed is None else seed)
    post = torch.randn(rows, 2 * z, generator=g)
    post[:, z:] = post[:, z:] * 3.0 + 1.0
    edge = torch.tensor([lo - 1.5, hi + 0.75, lo, hi, lo + 0.5])
    post[0, z:z + min(z, 5)] = edge[:min(z, 5)]
    post[-1, z:z + min(z, 5)] = edge.flip(0)[:min(z, 5)]
    return post, torch.randn(rows, z, generator=g), torch.randn(rows, z, generator=g) * 0.01


def kl_terms(eps, mu, lv):
    """The reference's log q(z) - log p(z) per element (Network.py:12-19 log_p_var_normal / log_p_normal, :223-224)."""
    logqz = -0.5 * (eps - mu) ** 2 / torch.exp(lv) - 0.5 * lv - LOG_SQRT_2PI
    logpz = -0.5 * eps ** 2 - LOG_SQRT_2PI
    return logqz - logpz


def reparam_kl_bwd_autograd(post, noise, d_eps, kl_scale, lo, hi):
    """float64 autograd of  (eps * d_eps).sum() + kl_scale * kl.sum()  over the reference's expressions: mu, logvar = post.chunk(2, dim=1)
    (Network.py:76), logvar.clamp(lo, hi) (:219), eps = mu + exp(logvar / 2) * noise (:26-29) -> dpost float64 [rows, 2 z]."""
    p = post.double().clone().requires_grad_(True)
    z = p.shape[1] // 2
    mu, lv = p[:, :z], p[:, z:].clamp(lo, hi)
    eps = mu + torch.exp(lv / 2) * noise.double()
    (g,) = torch.autograd.grad((eps * d_eps.double()).sum() + kl_scale * kl_terms(eps, mu, lv).sum(), p)
    return g


RKB_FAULTS = ("clamp mask ignored", "-kl_scale / 2 dropped", "KL term on d_eps dropped")


def reparam_kl_bwd_closed(post, noise, d_eps, kl_scale, lo, hi, dt=torch.float64, fault=None):
    """The kernel's closed form in dtype dt.  dt float64: -> (dpost, bound).  dt float32: the kernel's arithmetic with one of RKB_FAULTS
    planted -> dpost alone."""
    assert fault is None or fault in RKB_FAULTS
    z = post.shape[1] // 2
    mu, raw, n, de = post[:, :z].to(dt), post[:, z:].to(dt), noise.to(dt), d_eps.to(dt)
    ks = torch.tensor(float(kl_scale), dtype=torch.float32).to(dt)      # the entry point takes it as a float
    lv = raw.clamp(lo, hi)
    sn = torch.exp(lv / 2) * n
    eps = mu + sn
    g = de + (0.0 if fault == "KL term on d_eps dropped" else ks) * eps
    dlv = g * (sn / 2) - (0.0 if fault == "-kl_scale / 2 dropped" else ks / 2)
    live = torch.ones_like(raw, dtype=torch.bool) if fault == "clamp mask ignored" else (raw >= lo) & (raw <= hi)
    out = torch.cat([g, torch.where(live, dlv, torch.zeros_like(dlv))], 1)
    if dt != torch.float64:
        return out
    e_sn = (EXP_ROUNDINGS + 1) * U24 * sn.abs()
    e_eps = e_sn + U24 * eps.abs()
    e_g = ks.abs() * e_eps + U24 * g.abs()
    e_dlv = e_g * (sn / 2).abs() + g.abs() * e_sn / 2 + U24 * dlv.abs()
    return out, torch.cat([e_g, torch.where(live, e_dlv, torch.zeros_like(e_dlv))], 1) * SLACK


# ---- the whole top-down step: the float64 restatement and its bf16 twin (test_gpu_topdown_train.py, tools/gen_topdown_train_golden.py)
def top_down(sd, cfg, enc_out, post_noise, keep_mask=None):
    """Compressor.top_down (Network.py:208-233) from the oracle's pieces, token-major: enc_out n_layers tensors [B, T, C] in bottom-up order,
    post_noise n_layers tensors [B, T, z] in consumption order -> (set [B, N, 3], all_eps [B, T, n_layers z], kls: n_layers tensors [B, T, z])."""
    from oracle import ldt_oracle as O
    L, z, H = cfg.n_layers, cfg.z_dim, cfg.num_heads
    act, nk = getattr(cfg, "decoder_act", None), getattr(cfg, "norm", "layer_norm")
    o = O.initial_set(sd, enc_out[0].shape[0], keep_mask=keep_mask)
    all_eps, kls = [], []
    for j in range(L):
        blk = "decoder.%d" % (L - 1 - j)
        xj = enc_out[-j - 1]
        p = O.residual_block(sd, blk + ".att", xj, o if j != 0 else xj, None, H, act=act, norm=nk)        # compute_posterior, :61-78
        post = O.linear(sd, blk + ".prior.1", torch.nn.functional.silu(p))
        mu, lv = post[..., :z], post[..., z:].clamp(cfg.min_sigma, 10.)
        eps = mu + torch.exp(lv / 2.) * post_noise[j]                                                     # :26-29
        kls.append(kl_terms(eps, mu, lv))                                                                 # :222-224
        o = O.decoder_block(sd, blk, o, eps, H, None, act=act, norm=nk)                                   # :225
        all_eps.append(eps)
    return O.linear(sd, "output", o), torch.cat(all_eps, dim=-1), kls


def oracle_step(init, ccfg, names, enc_out, post_noise, target, dtype, kl_weight, keep_mask=None, autocast=False, d_set=None, rec=True):
    """top_down + kl_weight * cat(kls).mean() + CD_loss('l1') + autograd on a copy of the weights -> ({name: grad, 'd_enc_out.i': grad,
    'd_set': d rec_loss / d set}, (loss, kl_loss, rec_loss), set, all_eps, (sd, leaves)).  d_set: the gradient with respect to the set to
    start the reconstruction path from, in place of this run's own; rec False: the KL path alone (d_set = 0)."""
    import decoder_train_checks as dc
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in init.items()}
    leaves = [sd[n].requires_grad_(True) for n in names]
    xs = [t.detach().clone().to(dtype).requires_grad_(True) for t in enc_out]
    nz = [t.detach().to(dtype) for t in post_noise]
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        pts, all_eps, kls = top_down(sd, ccfg, xs, nz, keep_mask=keep_mask)
    pts.retain_grad()
    kl_loss = torch.cat([k.to(dtype) for k in kls], dim=1).mean()
    rec_loss = dc.cd_loss_torch(pts.to(dtype), target.to(dtype), "l1")
    if d_set is None and rec:
        (kl_weight * kl_loss + rec_loss).backward()
        d_own = pts.grad
    else:
        (d_own,) = torch.autograd.grad(rec_loss, pts, retain_graph=True)
        start = torch.zeros_like(pts) if not rec else d_set.to(pts.dtype)
        torch.autograd.backward([pts, kl_weight * kl_loss], [start, torch.ones((), dtype=kl_loss.dtype)])
    grads = {n: p.grad for n, p in zip(names, leaves)}
    grads.update({"d_enc_out.%d" % i: x.grad for i, x in enumerate(xs)})
    grads["d_set"] = d_own
    return grads, (float(kl_weight * kl_loss + rec_loss), float(kl_loss), float(rec_loss)), pts.detach(), all_eps.detach(), (sd, leaves)
