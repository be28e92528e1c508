"""GPU (-m gpu): the backward and optimizer kernels of a Score training step (csrc/score_bwd.hip, attention_bwd.hip, optim.hip), each
alone, per element.

Every kernel is compared with float64 computed from the very bf16 / fp32 inputs the kernel read, with kernel_checks.assert_elementwise
and a bound built from the operands the way kernel_checks.gemm_tol is.  The references and bounds live in kernel_checks.py (its "Score
training step" section states each next to its expression): tests/test_gpu_train_tape.py holds every call of a whole backward to the same
ones.  Each test prints its largest err / tol (run with -s); DESIGN.md section 4.11 records them."""
import math

import pytest
import torch

import kernel_checks as kc
from kernel_checks import U24, attn_bwd_ref

pytestmark = pytest.mark.gpu


def bf(t):
    return t.to(torch.bfloat16)


def report(name, ratio):
    print("train-kernel %-34s max err/tol %.3f" % (name, ratio))
    return ratio


# ------------------------------------------------------------------------------------------------ transposing cast
@pytest.mark.parametrize("R,C", [(16, 120), (200, 128), (72, 4096)])
@pytest.mark.parametrize("src_bf16", [False, True])
def test_transpose_cast_is_exact_and_zero_pads(R, C, src_bf16):
    from ldt_amd import ops
    g = torch.Generator().manual_seed(R * 7 + C)
    src = torch.randn(R, C, generator=g)
    src = bf(src) if src_bf16 else src
    Rp = ops.pad64(R)
    want = kc.transpose_cast_want(src, Rp)
    big = torch.full((C + 2, Rp + 64), 7.0, dtype=torch.bfloat16, device="cuda")       # guard band around the destination view
    out = ops.transpose_cast_bf16(src.cuda(), out=big[1:C + 1, :Rp])
    assert out.shape == (C, Rp) and torch.equal(out.cpu(), want)
    assert bool((big[0] == 7).all()) and bool((big[C + 1] == 7).all()) and bool((big[:, Rp:] == 7).all())
    assert torch.equal(ops.transpose_cast_bf16(src.cuda()).cpu(), want)              # a fresh destination, default padding
    # a strided source view (columns of a wider matrix)
    wide = torch.randn(R, C + 8, generator=g)
    wide = bf(wide) if src_bf16 else wide
    assert torch.equal(ops.transpose_cast_bf16(wide.cuda()[:, 8:]).cpu()[:, :R], bf(wide[:, 8:]).t())


# ------------------------------------------------------------------------------------------------ column sum, wgrad / dgrad through the route
@pytest.mark.parametrize("M,C", [(16, 128), (200, 128), (200, 120)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_colsum(M, C, dt):
    from ldt_amd import ops
    g = torch.Generator().manual_seed(M + C)
    dy = torch.randn(M, C, generator=g).to(dt)
    out = ops.colsum(dy.cuda())
    ref, tol = kc.colsum_ref(dy)
    report("colsum %dx%d %s" % (M, C, dt), kc.assert_elementwise(out.cpu(), ref, tol, "colsum"))
    assert torch.equal(ops.colsum(dy.cuda()), out)


@pytest.mark.parametrize("M,N,K", [(16, 128, 128), (200, 128, 120), (200, 512, 128)])
def test_wgrad_and_dgrad_through_the_nt_route(M, N, K):
    """dW = dY^T X contracts over the M tokens (16: one padded K-tile of the GEMM; 200: four, the last partial), dX = dY W over N."""
    from ldt_amd import ops
    g = torch.Generator().manual_seed(M * N + K)
    dy, x, w = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / N ** 0.5
    dw = ops.wgrad(dy.cuda(), x.cuda())
    assert dw.shape == (N, K) and dw.dtype == torch.float32
    ref, tol = kc.wgrad_ref(dy, x)
    report("wgrad M%d N%d K%d" % (M, N, K), kc.assert_elementwise(dw.cpu(), ref, tol, "wgrad"))
    dyb = bf(dy)
    w_t = ops.transpose_cast_bf16(w.cuda())                                          # [K, pad64(N)]
    assert w_t.shape == (K, ops.pad64(N))
    dx = ops.dgrad(dyb.cuda(), w_t)
    wt = bf(w).t().contiguous()                                                      # [K, N]
    ref, tol = kc.dgrad_ref(dyb, wt)
    report("dgrad M%d N%d K%d" % (M, N, K), kc.assert_elementwise(dx.cpu(), ref, tol, "dgrad"))


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate backward
def ln_case(M, C, rps, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 1.7 + offset * 1.7 + torch.randn(M, 1, generator=g) * 0.3
    dy = torch.randn(M, C, generator=g)
    scale = torch.randn(M // rps, C, generator=g) * 0.3
    dx0 = torch.randn(M, C, generator=g)                                             # the residual-stream gradient dx is added into
    return x, dy, scale, dx0


@pytest.mark.parametrize("M,rps,offset", [(16, 8, 0.0), (200, 8, 0.0), (200, 200, 0.0), (200, 8, 10.0)])
def test_layernorm_modulate_bwd(M, rps, offset):
    """offset 10: every row's mean^2 / variance is ~100 — x - mean cancels a digit, which the bound carries as |mean| / std."""
    from ldt_amd import ops
    C = 128
    x, dy, scale, dx0 = ln_case(M, C, rps, M + rps + int(offset), offset)
    dx = dx0.clone().cuda()
    dsh, dsc = ops.layernorm_modulate_bwd(x.cuda(), dy.cuda(), dx, scale=scale.cuda(), mod_sample_stride=C, rows_per_sample=rps)
    ref, tol, (mean, var) = kc.layernorm_modulate_bwd_ref(x, dy, scale, rps, dx0)
    if offset:
        assert 50 < float((mean ** 2 / var).min())
    r = kc.assert_elementwise(dx.cpu(), ref["dx"], tol["dx"], "layernorm_modulate_bwd dx")
    S = M // rps
    r = max(r, kc.assert_elementwise(dsh.cpu(), ref["dshift"], tol["dshift"], "layernorm_modulate_bwd dshift"),
            kc.assert_elementwise(dsc.cpu(), ref["dscale"], tol["dscale"], "layernorm_modulate_bwd dscale"))
    report("layernorm_modulate_bwd M%d rps%d off%g" % (M, rps, offset), r)
    wide = torch.full((S, 6 * C), 7.0, device="cuda")                               # dshift / dscale into column blocks of wider rows
    dx3 = dx0.clone().cuda()
    ops.layernorm_modulate_bwd(x.cuda(), dy.cuda(), dx3, scale=scale.cuda(), mod_sample_stride=C, rows_per_sample=rps,
                               dshift=wide[:, :C], dscale=wide[:, C:2 * C])
    assert torch.equal(wide[:, :C], dsh) and torch.equal(wide[:, C:2 * C], dsc) and bool((wide[:, 2 * C:] == 7).all()) and torch.equal(dx3, dx)
    # no modulation outputs, a second time: the same dx bits
    dx2 = dx0.clone().cuda()
    assert ops.layernorm_modulate_bwd(x.cuda(), dy.cuda(), dx2, scale=scale.cuda(), mod_sample_stride=C, rows_per_sample=rps,
                                      want_mod=False) == (None, None)
    assert torch.equal(dx2, dx)


# ------------------------------------------------------------------------------------------------ GELU, gate, SiLU, loss, embedding
@pytest.mark.parametrize("M", [16, 200])
@pytest.mark.parametrize("dh_dt", [torch.float32, torch.bfloat16])
def test_gelu_bwd(M, dh_dt):
    from ldt_amd import ops
    C = 128
    g = torch.Generator().manual_seed(M)
    u = bf(torch.randn(M, C, generator=g) * 2.5)
    u[0, :8] = bf(torch.tensor([-12.0, -6.0, -3.0, -0.0, 0.0, 3.0, 6.0, 12.0]))
    dh = torch.randn(M, C, generator=g).to(dh_dt)
    out = ops.gelu_bwd(u.cuda(), dh.cuda())
    ref, tol = kc.gelu_bwd_ref(u, dh)
    report("gelu_bwd M%d %s" % (M, dh_dt), kc.assert_elementwise(out.cpu(), ref, tol, "gelu_bwd"))


@pytest.mark.parametrize("M,rps", [(16, 8), (200, 8), (200, 200)])
@pytest.mark.parametrize("a_dt", [torch.float32, torch.bfloat16])
def test_gate_residual_bwd(M, rps, a_dt):
    from ldt_amd import ops
    C = 128
    g = torch.Generator().manual_seed(M + rps)
    dy, a = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g).to(a_dt)
    mod = torch.randn(M // rps, 6 * C, generator=g)                                   # the gate is a column block of the modulation rows
    gate = mod[:, 2 * C:3 * C]
    da, dg = ops.gate_residual_bwd(dy.cuda(), mod.cuda()[:, 2 * C:3 * C], a.cuda(), rows_per_sample=rps)
    S = M // rps
    ref, tol = kc.gate_residual_bwd_ref(dy, gate, a, rps)
    r = kc.assert_elementwise(da.cpu(), ref["da"], tol["da"], "gate_residual_bwd da")
    r = max(r, kc.assert_elementwise(dg.cpu(), ref["dgate"], tol["dgate"], "gate_residual_bwd dgate"))
    report("gate_residual_bwd M%d rps%d %s" % (M, rps, a_dt), r)
    da2, none = ops.gate_residual_bwd(dy.cuda(), mod.cuda()[:, 2 * C:3 * C], None, rows_per_sample=rps)
    assert none is None and torch.equal(da2, da)
    wide = torch.full((S, 6 * C), 7.0, device="cuda")                               # dgate written into a column block of wider rows
    ops.gate_residual_bwd(dy.cuda(), mod.cuda()[:, 2 * C:3 * C], a.cuda(), rows_per_sample=rps, dgate=wide[:, 2 * C:3 * C])
    assert torch.equal(wide[:, 2 * C:3 * C], dg) and bool((wide[:, :2 * C] == 7).all()) and bool((wide[:, 3 * C:] == 7).all())


def test_silu_bwd():
    from ldt_amd import ops
    g = torch.Generator().manual_seed(3)
    c, dy = torch.randn(200, 128, generator=g) * 3, torch.randn(200, 128, generator=g)
    c[0, :4] = torch.tensor([-30.0, -0.0, 0.0, 30.0])
    out = ops.silu_bwd(c.cuda(), dy.cuda())
    ref, tol = kc.silu_bwd_ref(c, dy)
    report("silu_bwd", kc.assert_elementwise(out.cpu(), ref["dc"], tol["dc"], "silu_bwd"))
    out2, act = ops.silu_bwd(c.cuda(), dy.cuda(), want_act=True)                      # + SiLU(c), the next Linear's wgrad operand
    assert torch.equal(out2, out)
    kc.assert_elementwise(act.cpu(), ref["act"], tol["act"], "silu_bwd act")


@pytest.mark.parametrize("B,T", [(2, 8), (25, 8), (1, 200)])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_dsm_loss_bwd(B, T, l1, weighted):
    from ldt_amd import ops
    C = 128
    g = torch.Generator().manual_seed(B * T + l1)
    eta, params = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    params[0, 0, :4] = eta[0, 0, :4]                                                  # d = 0: the l1 gradient is 0 there
    w = torch.rand(B, generator=g) + 0.5 if weighted else None
    out = ops.dsm_loss_bwd(eta.cuda(), params.cuda(), None if w is None else w.cuda(), l1=l1)
    ref, tol = kc.dsm_loss_bwd_ref(eta, params, w, l1)
    report("dsm_loss_bwd B%d T%d l1=%d w=%d" % (B, T, l1, weighted), kc.assert_elementwise(out.cpu(), ref, tol, "dsm_loss_bwd"))


def test_embedding_grad():
    from ldt_amd import ops
    g = torch.Generator().manual_seed(11)
    B, D, K = 8, 128, 4
    dc = torch.randn(B, D, generator=g)
    label = torch.tensor([2, 0, 2, 1, 0, 2, 2, 0])                                    # class 3 has no sample: a zero row
    out = ops.embedding_grad(dc.cuda(), label.cuda(), K)
    ref, tol = kc.embedding_grad_ref(dc, label, K)
    report("embedding_grad", kc.assert_elementwise(out.cpu(), ref, tol, "embedding_grad"))
    assert float(out[3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ attention backward
def attn_case(B, H, N, seed, large_logit=False):
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    qkv = torch.randn(B * N, 3 * C, generator=g)
    if large_logit:                                                                   # s[i, (7 i + 3) % N] ~ 12 |k|^2 / 8 ~ 96: exp overflows without the max
        q = qkv[:, :C].view(B, N, H, 64)
        k = qkv[:, C:2 * C].view(B, N, H, 64)
        q += 12.0 * k[:, (7 * torch.arange(N) + 3) % N]
    return bf(qkv), bf(torch.randn(B, H, N, 64, generator=g))


@pytest.mark.parametrize("B,H,N,large", [(2, 2, 8, False), (1, 2, 72, False), (1, 1, 256, False), (1, 2, 72, True)])
def test_attention_bwd(B, H, N, large):
    """(1, 2, 72): one full 64-key stretch plus a partial one (and a partial 32-column step of the kernel's loop).  large: one logit per row
    is ~96, far above the others, so a backward that skipped the recomputed row maximum would overflow."""
    from ldt_amd import ops
    C = H * 64
    qkv, do = attn_case(B, H, N, B * 100 + H * 10 + N + large, large)
    qkv_d, do_d = qkv.cuda(), do.cuda()
    q, k, v = qkv_d[:, :C], qkv_d[:, C:2 * C], qkv_d[:, 2 * C:]
    o = ops.attention_fwd(q, k, v, B, H, N, N, 64)                                    # the saved forward output, as training keeps it
    dq, dk, dv = ops.attention_bwd(q, k, v, o, do_d, B, H, N)
    ref, tol = attn_bwd_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o.cpu(), do, B, H, N, N)
    if large:
        s = (qkv[:, :C].double().view(B, N, H, 64).permute(0, 2, 1, 3) @ qkv[:, C:2 * C].double().view(B, N, H, 64).permute(0, 2, 3, 1)) / 8
        assert float(s.amax(-1).min()) > 40 and float(s.amax(-1).max()) > 89      # past fp32 exp's range
    hd = lambda z: z.cpu().view(B, N, H, 64).permute(0, 2, 1, 3)
    r = max(kc.assert_elementwise(hd(got), ref[nm], tol[nm], "attention_bwd " + nm) for nm, got in (("dq", dq), ("dk", dk), ("dv", dv)))
    report("attention_bwd B%d H%d N%d large=%d" % (B, H, N, large), r)
    dq2, dk2, dv2 = ops.attention_bwd(q, k, v, o, do_d, B, H, N)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)     # fixed order: the same bits


def test_attention_bwd_q1_probe():
    """Quirk Q1: dO is the raw [B][H][N][Dh] buffer.  A gradient in the single row [b][h][n] must reach dV only in head h of sample b —
    a kernel that read dO as (B, N, H, Dh) rows would spread it over other heads or tokens' heads."""
    from ldt_amd import ops
    B, H, N = 2, 2, 8
    C = H * 64
    qkv, _ = attn_case(B, H, N, 5)
    qkv_d = qkv.cuda()
    q, k, v = qkv_d[:, :C], qkv_d[:, C:2 * C], qkv_d[:, 2 * C:]
    o = ops.attention_fwd(q, k, v, B, H, N, N, 64)
    for b, h, n in ((1, 0, 5), (0, 1, 2)):
        do = torch.zeros(B, H, N, 64, dtype=torch.bfloat16, device="cuda")
        do[b, h, n] = 1.0
        dq, dk, dv = ops.attention_bwd(q, k, v, o, do, B, H, N)
        inside = torch.zeros(B, N, H, 64, dtype=torch.bool, device="cuda")
        inside[b, :, h] = True
        dv4 = dv.reshape(B, N, H, 64)
        assert float(dv4[~inside].abs().max()) == 0.0 and bool((dv4[inside] != 0).all())
        dq4, dk4 = dq.reshape(B, N, H, 64), dk.reshape(B, N, H, 64)
        assert float(dk4[~inside].abs().max()) == 0.0
        only_row = torch.zeros_like(inside)
        only_row[b, n, h] = True
        assert float(dq4[~only_row].abs().max()) == 0.0 and float(dq4[only_row].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("n", [1000, 70001, 3_000_000])
def test_sumsq_and_clip_factor(n):
    """1000: four partials; 70001: 274, an odd tail; 3e6: more elements than 1024 partials x 256 lanes cover in one pass."""
    from ldt_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 0.01
    ref = float((x.double() ** 2).sum())
    for max_norm in (0.0, 0.5, 100.0):
        out = ops.sumsq(x.cuda(), max_norm=max_norm).cpu()
        # bound: float64 partials of exact squares, one rounding to fp32; the root and the factor: two more each
        assert abs(float(out[0]) - ref) <= 2 * U24 * ref
        assert abs(float(out[1]) - math.sqrt(ref)) <= 3 * U24 * math.sqrt(ref)
        want = min(1.0, max_norm / (math.sqrt(ref) + 1e-6)) if max_norm > 0 else 1.0
        assert abs(float(out[2]) - want) <= 6 * U24 * want
        assert torch.equal(ops.sumsq(x.cuda(), max_norm=max_norm).cpu(), out)
    assert float(ops.sumsq(x.cuda(), max_norm=100.0)[2]) == 1.0


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("clip", [0.37, 1.0])
def test_adam_ema_step_against_torch_adam(weight_decay, clip):
    """Three steps of torch.optim.Adam + the reference's EMA lines (tools/utils.py:49-62) on the CPU against ldt_adam_ema_step, fed the same
    gradients and the same state.  The CPU side runs in float64 from the device's fp32 state: the bound's 2^-24 |p| term is the rounding of the
    STORED fp32 value against an exact result (against an fp32 torch run a second 2^-24 |p|, that run's own rounding, would have to be
    allowed: two fp32 evaluations of p + d differ by a whole ulp whenever p + d sits near a rounding boundary).  Each step starts from the
    device's own previous state, so every step is judged by the one-step bound.
    Bound (the issue's): 2^-24 |p| + 8 x 2 x 2^-24 |delta p|: eight roundings in the update chain, doubled because the device's sqrt and
    divide need not be correctly rounded; exp_avg and exp_avg_sq likewise with their own step deltas; the EMA by propagation from the
    parameter's bound (stated at the check)."""
    from ldt_amd import ops
    n, lr, b1, b2, eps, decay = 4099, 2e-3, 0.9, 0.999, 1e-8, 0.98
    g = torch.Generator().manual_seed(int(weight_decay * 1000) + int(clip * 100))
    st32 = {"p": torch.randn(n, generator=g), "m": torch.zeros(n), "v": torch.zeros(n), "ema": torch.zeros(n)}
    coef = torch.tensor([clip], dtype=torch.float32)
    worst = 0.0
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g) * (0.1 if step == 2 else 1.0)
        use_clip = clip != 1.0 or step == 2                                            # (a factor of exactly 1 is also passed once)
        # CPU: clip_grad_norm_'s in-place fp32 scaling (one IEEE product: the device's is held to torch.equal below), then in float64
        # torch.optim.Adam and the EMA lines (kernel_checks.adam_ema_ref, which also forms the bound stated above)
        fed = (grad * coef) if use_clip else grad                                    # clip_grad_norm_ ran in fp32: THE gradient Adam is fed
        ref, tol = kc.adam_ema_ref(st32, fed, step, lr, b1, b2, eps, weight_decay, decay, ema_init=step == 1)
        # device
        d = {k: v.clone().cuda() for k, v in st32.items()}
        gd = grad.clone().cuda()
        ops.adam_ema_step_(d["p"], gd, d["m"], d["v"], d["ema"], step, lr, b1, b2, eps, weight_decay, decay, ema_init=step == 1,
                           clip_factor=coef.cuda() if use_clip else None)
        if use_clip:
            assert torch.equal(gd.cpu(), grad * coef)                                  # the gradient is scaled in place
        else:
            assert torch.equal(gd.cpu(), grad)
        for nm, got in (("p", d["p"]), ("exp_avg", d["m"]), ("exp_avg_sq", d["v"])):
            worst = max(worst, kc.assert_elementwise(got.cpu(), ref[nm], tol[nm], "adam_ema_step %s, step %d" % (nm, step)))
        # the EMA is a function of the NEW parameter: ema = ema_old d + (1 - d) p.  On a parameter's first step ema_old = p, so the EMA IS the
        # new parameter: bit-equal to it on the device, and held to the parameter's bound.  After that it inherits p's error with the factor
        # d ema / d p = 1 - d and adds its own rounding plus the roundings of its change (the issue's form, on the EMA's own delta).
        if step == 1:
            assert torch.equal(d["ema"], d["p"])
        worst = max(worst, kc.assert_elementwise(d["ema"].cpu(), ref["ema"], tol["ema"], "adam_ema_step ema, step %d" % step))
        st32 = {"p": d["p"].cpu(), "m": d["m"].cpu(), "v": d["v"].cpu(), "ema": d["ema"].cpu()}
    report("adam_ema_step wd%g clip%g" % (weight_decay, clip), worst)
