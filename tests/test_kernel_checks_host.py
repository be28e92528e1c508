"""CPU: the reference helpers of the fused projection + attention tests (kernel_checks.py) judged without a GPU.

An emulation of the kernels' contract in torch on the CPU — q | k | v = bf16(fp32 accumulation) in two different summation orders (K in
64-blocks, forward and reversed), float32 softmax, P rounded to bf16, O bf16 — must pass every check that test_gpu_fused_attention_exact.py
applies to the HIP kernels, and the same emulation with one planted fault (one key dropped for one query row; heads h and h + 1 swapped in
k; the S | C slice of one 64-column segment taken from the next segment) must FAIL them: the proof that the derived bound is tight enough to
tell a right kernel from a nearly right one."""
import numpy as np
import pytest
import torch

import kernel_checks as kc

DH = 64


def project(x, w, bias, reverse):
    """fp32 accumulation over K in 64-blocks (forward / reversed order) + bias, not yet rounded."""
    blocks = list(range(0, x.shape[1], 64))
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in (reversed(blocks) if reverse else blocks):
        acc = acc + x[:, k0:k0 + 64] @ w[:, k0:k0 + 64].T
    return acc if bias is None else acc + bias


def project_folded(xs, w, S, C, stats, reverse, shift_segment=None):
    """The LN-folded consumer in fp32: rstd acc - rstd mean S + C with (mean, rstd) from the fp32 statistics.  shift_segment = s: the planted
    fault, columns [64 s, 64 s + 64) read the S | C of the next 64-column segment."""
    K = xs.shape[1]
    s = stats.sum(0)
    mean = s[:, 0:1] / K
    rstd = torch.rsqrt((s[:, 1:2] / K - mean * mean).clamp_min(0) + 1e-6)
    if shift_segment is not None:
        S, C = S.clone(), C.clone()
        a = shift_segment * 64
        S[a:a + 64], C[a:a + 64] = S[a + 64:a + 128].clone(), C[a + 64:a + 128].clone()
    return rstd * project(xs, w, None, reverse) - rstd * mean * S + C


def attend(q, k, v, B, H, Nq, Nk, drop=None, swap_k_heads=None):
    """bf16 q | k | v rows -> O [B, H, Nq, DH] bf16: float32 scores and softmax, P to bf16, fp32 P V.  drop = (b, h, i, j): key j is missing
    for query i of head (b, h); swap_k_heads = h: k of heads h and h + 1 exchanged."""
    sp = lambda z, n: z.float().reshape(B, n, H, DH).permute(0, 2, 1, 3)
    kk = sp(k, Nk)
    if swap_k_heads is not None:
        kk = kk.clone()
        kk[:, [swap_k_heads, swap_k_heads + 1]] = kk[:, [swap_k_heads + 1, swap_k_heads]]
    s = sp(q, Nq) @ kk.transpose(-1, -2) * DH ** -0.5
    if drop is not None:
        s[drop] = float("-inf")
    return (s.softmax(-1).bfloat16().float() @ sp(v, Nk)).bfloat16()


def randn_case(B, T, H, K, seed, xscale=1.0):
    g = torch.Generator().manual_seed(seed)
    C = H * DH
    x = (torch.randn(B * T, K, generator=g) * xscale).bfloat16().float()
    w = (torch.randn(3 * C, K, generator=g) / K ** 0.5).bfloat16().float()
    bias = 0.1 * torch.randn(3 * C, generator=g)
    return x, w, bias


def folded_case(B, T, H, K, granule, seed, scale=0.5):
    """xs with a row mean that is not small and differs from row to row (what is the same for every key cancels in the softmax); W, S, C at half of _consumer_bound's scale: at full scale the q, k of K = 1024 (magnitude ~1.7,
    accumulation bound 2^-19 of three terms) take tol / base to 9.5 somewhere, beyond the cap of 8."""
    g = torch.Generator().manual_seed(seed)
    C = H * DH
    xs = torch.randn(B * T, K, generator=g) * 1.2 + 0.4
    w = (scale * torch.randn(3 * C, K, generator=g) / K ** 0.5).bfloat16().float()
    S, Cc = scale * torch.randn(3 * C, generator=g), scale * torch.randn(3 * C, generator=g)
    xs = (xs + 0.6 * torch.randn(B * T, 1, generator=g)).bfloat16().float()
    t = xs.double().view(B * T, K // granule, granule)
    stats = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()
    return xs, w, S, Cc, stats


def split(y, C):
    return y[:, :C], y[:, C:2 * C], y[:, 2 * C:]


def check_c(out, pre, acc, B, H, T, what, kv=None, Nk=None):
    ref, tol, ratio, amb = kc.fused_attention_tol(pre, acc, B, H, T, DH, kv=kv, Nk=Nk)
    kc.assert_ratio_caps(ratio, what)
    return kc.assert_elementwise(out.reshape(-1, DH), ref.reshape(-1, DH), tol.reshape(-1, DH), what)


# ------------------------------------------------------------------------------------------------------------- the helpers themselves
def test_ambiguous_ulp_marks_exactly_the_neighbourhood_of_a_rounding_boundary():
    ulp = 2.0 ** -7                                                   # of [1, 2)
    pre = torch.tensor([1.0 + 0.5 * ulp, 1.0 + 0.5 * ulp + 1e-6, 1.0 + 0.5 * ulp - 1e-4, 1.0 + 3 * ulp, 1.0 + 1e-7, 1.0 - 0.25 * ulp + 1e-7, -(2.0 + ulp), 0.75], dtype=torch.float64)
    e = kc.ambiguous_ulp(pre, torch.full_like(pre, 1e-5))
    assert [bool(v) for v in e > 0] == [True, True, False, False, False, True, True, False]
    b = lambda v: 1e-5 + kc.U24 * v
    want = [ulp + b(float(pre[0])), 0.5 * ulp + b(float(pre[5])), 2 * ulp + b(2.0 + ulp)]          # (one ulp of the binade, plus b)
    assert [float(e[0]), float(e[5]), float(e[6])] == pytest.approx(want, rel=1e-12)
    assert torch.equal(kc.bf16_round(torch.tensor([1.0 + 0.75 * ulp], dtype=torch.float64)), torch.tensor([1.0 + ulp], dtype=torch.float64))


@pytest.mark.parametrize("K,std,top", [(128, 0.51, 3.25), (320, 0.74, 4.25), (1024, 1.28, 6.38)])
def test_exact_projection_probe_is_exact_in_any_order_and_of_ordinary_sharpness(K, std, top):
    x, w, bias, y = kc.exact_projection_probe(512, 768, K, 1)
    assert abs(float(y.std()) - std) < 0.1 * std and float(y.abs().max()) <= top + 1.0 and 0.85 <= float((y != 0).double().mean()) <= 0.99
    for reverse in (False, True):
        assert torch.equal(project(x, w, bias, reverse).bfloat16().double(), y)


def test_rounding_flips_between_summation_orders_stay_inside_the_ambiguous_mask():
    """What fused_attention_tol rests on: wherever bf16(fp32 accumulation) differs from bf16_round(float64), the element is marked ambiguous
    and differs by no more than the mask carries (one ulp, or many where cancellation leaves a value below its accumulation error); and the two orders do differ somewhere (otherwise this test shows nothing)."""
    x, w, bias = randn_case(8, 32, 4, 1024, 5)
    pre = x.double() @ w.double().T + bias.double()
    e = kc.ambiguous_ulp(pre, kc.gemm_acc_err(x, w, bias, 1024))
    r = kc.bf16_round(pre)
    ys = [project(x, w, bias, rev).bfloat16().double() for rev in (False, True)]
    assert not torch.equal(ys[0], ys[1])
    for y in ys:
        assert bool(((y - r).abs() <= e).all()) and int((y != r).sum()) > 0
    assert 0.05 < float((e > 0).double().mean()) < 0.2


# ------------------------------------------------------------------------------------------------------------- the emulation passes (a), (b), (c)
SELF = [(4, 32, 4, 320), (4, 32, 4, 1024), (2, 256, 4, 128), (2, 256, 4, 1024)]      # B, T, H, K


@pytest.mark.parametrize("B,T,H,K", SELF)
def test_emulation_passes_the_exact_projection_probe_at_the_plain_attention_bound(B, T, H, K):
    C = H * DH
    x, w, bias, y = kc.exact_projection_probe(B * T, 3 * C, K, 7)
    ref, vmax = kc.attention_ref64(*split(y, C), B, H, T, T, DH)
    for reverse in (False, True):
        qkv = project(x, w, bias, reverse).bfloat16()
        assert torch.equal(qkv.double(), y)
        kc.assert_elementwise(attend(*split(qkv, C), B, H, T, T).reshape(-1, DH), ref.reshape(-1, DH), kc.attention_base_tol(ref, vmax).reshape(-1, DH), "exact probe")


@pytest.mark.parametrize("T,cross", [(32, False), (256, False), (32, True)])
def test_emulation_passes_the_gather_probe_at_tolerance_zero(T, cross):
    B, H = 2, 2
    C = H * DH
    x, w, kv, want = kc.gather_projection_probe(B, H, T, T, DH, 3, cross=cross)
    for bias in (None, torch.zeros(w.shape[0])):
        y = project(x, w, bias, False).bfloat16()
        q, k, v = (y, kv[:, :C].bfloat16(), kv[:, C:].bfloat16()) if cross else split(y, C)
        kc.assert_elementwise(attend(q, k, v, B, H, T, T).reshape(-1, DH), want.double().reshape(-1, DH), 0.0, "gather probe")


@pytest.mark.parametrize("B,T,H,K", SELF)
def test_emulation_passes_the_two_stage_bound_in_both_orders(B, T, H, K):
    x, w, bias = randn_case(B, T, H, K, B + T + K)
    pre = x.double() @ w.double().T + bias.double()
    acc = kc.gemm_acc_err(x, w, bias, K)
    for reverse in (False, True):
        out = attend(*split(project(x, w, bias, reverse).bfloat16(), H * DH), B, H, T, T)
        assert check_c(out, pre, acc, B, H, T, "plain T %d K %d" % (T, K)) <= 1.0


@pytest.mark.parametrize("B,T,H,K,granule", [(4, 32, 4, 512, 32), (4, 32, 4, 1024, 32), (2, 256, 4, 256, 256), (2, 256, 4, 1024, 256)])
def test_emulation_of_the_folded_form_passes_the_two_stage_bound(B, T, H, K, granule):
    xs, w, S, Cc, stats = folded_case(B, T, H, K, granule, T + K)
    pre, acc = kc.consumer_pre64(xs, w, S, Cc, stats, K)
    for reverse in (False, True):
        out = attend(*split(project_folded(xs, w, S, Cc, stats, reverse).bfloat16(), H * DH), B, H, T, T)
        assert check_c(out, pre, acc, B, H, T, "folded T %d K %d" % (T, K)) <= 1.0


def test_emulation_of_the_cross_form_passes_the_two_stage_bound():
    B, T, H, K = 4, 32, 4, 1024
    C = H * DH
    x, w, bias = randn_case(B, T, H, K, 11)
    w, bias = w[:C], bias[:C]
    kv = (torch.randn(B * T, 2 * C, generator=torch.Generator().manual_seed(12)) * 1.5).bfloat16()
    pre = x.double() @ w.double().T + bias.double()
    out = attend(project(x, w, bias, True).bfloat16(), kv[:, :C], kv[:, C:], B, H, T, T)
    assert check_c(out, pre, kc.gemm_acc_err(x, w, bias, K), B, H, T, "cross", kv=(kv[:, :C], kv[:, C:]), Nk=T) <= 1.0


# ------------------------------------------------------------------------------------------------------------- planted faults must fail
@pytest.mark.parametrize("B,T,H,K", [(4, 32, 4, 320), (2, 256, 4, 1024)])
def test_planted_dropped_key_and_swapped_heads_fail_every_check(B, T, H, K):
    C = H * DH
    # (c) randn data: the key with the largest weight of head (1, 2) dropped for that one query row; k of heads 1 and 2 exchanged
    x, w, bias = randn_case(B, T, H, K, B + T + K)
    pre = x.double() @ w.double().T + bias.double()
    acc = kc.gemm_acc_err(x, w, bias, K)
    qkv = split(project(x, w, bias, False).bfloat16(), C)
    r = split(kc.bf16_round(pre), C)
    p = (kc.heads(r[0], B, T, H, DH) @ kc.heads(r[1], B, T, H, DH).transpose(-1, -2) * DH ** -0.5).softmax(-1)[1, 2]
    i, j = divmod(int(p.argmax()), T)
    check_c(attend(*qkv, B, H, T, T), pre, acc, B, H, T, "no fault")
    with pytest.raises(AssertionError, match="ONE ROW"):
        check_c(attend(*qkv, B, H, T, T, drop=(1, 2, i, j)), pre, acc, B, H, T, "dropped key (randn)")
    with pytest.raises(AssertionError, match="outside the bound"):
        check_c(attend(*qkv, B, H, T, T, swap_k_heads=1), pre, acc, B, H, T, "swapped heads (randn)")
    # (a) exact-projection probe at the plain bound
    x, w, bias, y = kc.exact_projection_probe(B * T, 3 * C, K, 7)
    ref, vmax = kc.attention_ref64(*split(y, C), B, H, T, T, DH)
    p = (kc.heads(y[:, :C], B, T, H, DH) @ kc.heads(y[:, C:2 * C], B, T, H, DH).transpose(-1, -2) * DH ** -0.5).softmax(-1)[1, 2]
    i, j = divmod(int(p.argmax()), T)
    qkv = split(project(x, w, bias, False).bfloat16(), C)
    for kw in (dict(drop=(1, 2, i, j)), dict(swap_k_heads=1)):
        with pytest.raises(AssertionError, match="outside the bound"):
            kc.assert_elementwise(attend(*qkv, B, H, T, T, **kw).reshape(-1, DH), ref.reshape(-1, DH), kc.attention_base_tol(ref, vmax).reshape(-1, DH), "exact probe")
    # (b) gather probe at tolerance 0: the gathered key of query 5 dropped; heads exchanged
    x, w, _, want = kc.gather_projection_probe(B, H, T, T, DH, 3)
    qkv = split(project(x, w, None, False).bfloat16(), C)
    for kw in (dict(drop=(1, 2, 5, int(kc.attention_pi(T, T, salt=13 * (1 * H + 2))[5]))), dict(swap_k_heads=1)):
        with pytest.raises(AssertionError, match="outside the bound"):
            kc.assert_elementwise(attend(*qkv, B, H, T, T, **kw).reshape(-1, DH), want.double().reshape(-1, DH), 0.0, "gather probe")


@pytest.mark.parametrize("B,T,H,K,granule,segment", [(4, 32, 4, 512, 32, 1), (2, 256, 4, 1024, 256, 9)])
def test_planted_shifted_fold_segment_fails(B, T, H, K, granule, segment):
    """The folded form reading the S | C slice of the next 64-column segment for one segment (q of head 1; v of head 1)."""
    xs, w, S, Cc, stats = folded_case(B, T, H, K, granule, T + K)
    pre, acc = kc.consumer_pre64(xs, w, S, Cc, stats, K)
    out = attend(*split(project_folded(xs, w, S, Cc, stats, False, shift_segment=segment).bfloat16(), H * DH), B, H, T, T)
    with pytest.raises(AssertionError, match="outside the bound"):
        check_c(out, pre, acc, B, H, T, "shifted S | C segment")


# ============================================================================================================= grouped rows + the fused grouper
# An emulation of csrc/grouper_mlp.hip's contract: fp32 statistics and normalisation, bf16 at U, h1, r and out, fp32 accumulation in two k
# orders, 32-row tiles (k = 8 / 16: 4 / 2 groups per tile with a ragged last tile, k = 32 m: m tiles combined by a max onto a zeroed buffer),
# writing into a guarded buffer like the GPU module's.  FAULTS are the ways such a kernel goes subtly wrong.
FAULTS = ("drop_one", "stale_inv", "xyz_zero", "swap_l2", "ragged_store", "no_zero")
bf = lambda t: t.float().bfloat16().float()


def mm16(a, w, rev):
    """fp32 accumulation over K in 16-steps (the MFMA k-step), forward or reversed."""
    steps = list(range(0, a.shape[-1], 16))
    acc = torch.zeros(*a.shape[:-1], w.shape[0])
    for k0 in (reversed(steps) if rev else steps):
        acc = acc + a[..., k0:k0 + 16] @ w[:, k0:k0 + 16].T
    return acc


def emulate_rows(c, mode="anchor", stale=False, wrong_mean=False):
    """ldt_group_normalize in fp32 -> (U bf16-valued float [B S k, 2D+3], sums float64 [2B])."""
    B, S, k, D = c["B"], c["S"], c["k"], c["D"]
    fi, ki = c["fi"].long(), c["ki"].long()
    G = torch.cat([kc._take(c["feat"], ki), kc._take(c["xyz"], ki)], -1)
    anc = kc._take(c["feat"], fi)
    if mode == "anchor":
        org = torch.cat([anc, kc._take(c["xyz"], fi)], -1)[:, :, None]
    else:
        org = torch.zeros(B, S, 1, D + 3)
        for j in range(k):
            org = org + G[:, :, j:j + 1]
        org = org / float(k)
        if wrong_mean:
            org = org.roll(1, 1)
    d = G - org
    s1, s2 = d.double().sum((1, 2, 3)), (d.double() ** 2).sum((1, 2, 3))
    cnt = float(S * k * (D + 3))
    var = ((s2 - cnt * (s1 / cnt) ** 2) / (cnt - 1)).clamp_min(0)
    inv = (1.0 / (var.sqrt().float() + torch.tensor(1e-5)))[:, None, None, None]
    if stale:
        inv = inv[[0] * B]
    u = torch.cat([c["alpha"] * (d * inv) + c["beta"], anc[:, :, None].expand(-1, -1, k, -1)], -1)
    return bf(u).reshape(B * S * k, -1), torch.stack([s1, s2], 1).reshape(-1)


def emulate_grouper(c, W, rev=False, fault=None, fill=float("nan")):
    """-> (big, out view [B S, 128]) of kc.guarded, filled like the GPU module fills it."""
    B, S, k = c["B"], c["S"], c["k"]
    w1, b1, w2, b2, w3, b3 = W
    u, _ = emulate_rows(c, stale=fault == "stale_inv")
    u = u.reshape(B, S, k, -1).clone()
    if fault == "xyz_zero":
        u[..., 128:131] = 0
    if fault == "swap_l2":                                          # two k-slots of one layer-2 fragment (k-step 3, channel block 1) exchanged
        w2 = w2.clone()
        w2[32:64, [50, 53]] = w2[32:64, [53, 50]]
    h1 = bf(torch.relu(mm16(u, w1, rev) + b1))
    r = bf(torch.relu(mm16(h1, w2, rev) + b2))
    o = mm16(r, w3, rev) + b3 + h1                                  # [B, S, k, 128]
    if fault == "drop_one":                                         # the neighbour that decides channel 0 of group (0, 0) never enters the max
        o[0, 0, int(o[0, 0, :, 0].argmax())] = float("-inf")
    big, out = kc.guarded(B * S, 128, fill, "cpu")
    flat = big[4096:]                                               # rows addressed from the view's start, like the kernel's pointer
    if k > 32:
        if fault != "no_zero":
            out.zero_()
        for t in range(k // 32):                                    # the tiles of a group meet in memory
            out.copy_(torch.maximum(out, bf(torch.relu(o[:, :, 32 * t:32 * t + 32].amax(2))).reshape(B * S, 128)))
    else:
        res = bf(torch.relu(o.amax(2)))
        out.copy_(res.reshape(B * S, 128))
        gpt = 32 // k
        if fault == "ragged_store" and S % gpt:                     # the repeated last group of the ragged tile is stored after group S - 1
            for b in range(B):
                flat[(b * S + S) * 128:(b * S + S + 1) * 128] = res[b, S - 1]
    return big, out


def wimg_of(W):
    from ldt_amd.compressor import _grouper_fragment_image
    return _grouper_fragment_image(W[0], W[2], W[4])


def staged(c, W):
    g = kc.group_reference(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"], stats_rel=kc.U24)
    st = emulate_rows(c)[1].reshape(-1, 2)
    assert bool(((st[:, 0] - g["s1"]).abs() <= g["tol1"]).all()) and bool(((st[:, 1] - g["s2"]).abs() <= g["tol2"]).all())
    return kc.grouper_staged_reference(g, *W)


def probe_a(c0, variant, fault=None, rev=False):
    """-> (got, want, slot) of probe (a) on the emulation; `want` from the emulation of ldt_group_normalize (never faulty)."""
    w1, sel, sgn, alpha = kc.grouper_selection_probe(variant)
    c = kc.plant_winners(dict(c0, alpha=alpha, beta=torch.zeros(131)), sel, sgn, alpha)
    z = torch.zeros(128)
    _, got = emulate_grouper(c, (w1, z, torch.zeros(128, 128), z, torch.zeros(128, 128), z), rev=rev, fault=fault)
    U, _ = emulate_rows(c)
    want, slot = kc.grouper_selection_expected(U, c["B"], c["S"], c["k"], sel, sgn)
    return got, want, slot, sel


def probe_b(c0, fault=None, rev=False):
    feat, beta, W, o = kc.grouper_integer_probe(c0["B"], c0["n"], 5)
    c = dict(c0, feat=feat, alpha=torch.zeros(131), beta=beta)
    _, got = emulate_grouper(c, W, rev=rev, fault=fault)
    return got, kc._take(o, c["fi"].long()).reshape(-1, 128)


GROUPER_SHAPES = [(3, 300, 7, 8), (2, 512, 5, 64)]                  # 4 groups per tile with a ragged last tile; two tiles per group


@pytest.mark.parametrize("mode,D,k", [("anchor", 128, 16), ("anchor", 64, 5), ("anchor", 20, 8), ("center", 128, 8), ("center", 32, 5)])
def test_group_rows_emulation_passes_and_a_stale_inv_or_wrong_mean_fails(mode, D, k):
    # (the degenerate cloud belongs to 'anchor' mode, where d == 0 exactly; around a group MEAN a cloud without spread leaves only the mean's
    # own fp32 rounding, multiplied by 1 / 1e-5: nothing there can be pinned)
    c = kc.grouper_case(3, 200, 6, k, 3, D=D, degenerate=1 if mode == "anchor" else None)
    ref = kc.group_reference(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"], mode)
    U, st = emulate_rows(c, mode)
    res = kc.check_group_rows(U.bfloat16(), st, ref, D, "rows")
    assert res["pinned"] >= 0.98 and res["stat"] <= 1.0
    if mode == "anchor":
        assert torch.equal(U.reshape(3, -1, 2 * D + 3)[1, :, :D + 3], bf(c["beta"]).expand(6 * k, -1))  # the degenerate cloud: bf16(beta)
    with pytest.raises(AssertionError, match="outside their interval"):
        kc.check_group_rows(emulate_rows(c, mode, stale=True)[0].bfloat16(), st, ref, D, "stale inv")
    if mode == "center":
        with pytest.raises(AssertionError):
            U2, st2 = emulate_rows(c, mode, wrong_mean=True)
            kc.check_group_rows(U2.bfloat16(), st2, ref, D, "mean of the neighbouring group")


@pytest.mark.parametrize("B,n,S,k", GROUPER_SHAPES)
def test_grouper_emulation_passes_a_b_c_in_both_orders(B, n, S, k):
    c = kc.grouper_case(B, n, S, k, 1)
    W = kc.grouper_weights(2)
    sr = staged(c, W)
    for rev in (False, True):
        big, out = emulate_grouper(c, W, rev=rev)
        mism = kc.check_grouper(out, sr, "emulation (c) rev %d" % rev)
        kc.assert_guard_intact(big, out.numel(), "emulation")
        assert mism < 0.01
        slots = set()
        for v in range(3):
            got, want, slot, sel = probe_a(c, v, rev=rev)
            assert torch.equal(got.double(), want)
            slots |= set(slot[:, sel < 131].flatten().tolist())
        assert slots == set(range(k))                               # every register position decided some output
        got, want = probe_b(c, rev=rev)
        assert torch.equal(got.double(), want)
    assert wimg_of(W).numel() == 132 * 512                          # the image the GPU module builds from the same panels


def old_test_passes(c, W, got):
    """What test_fused_grouper_vs_oracle_and_chain asks: rel-MSE < 1e-4 against an fp32 evaluation, < 1e-5 and fewer than 25 % of the elements
    different against the (clean) chain."""
    w1, b1, w2, b2, w3, b3 = [t.double() for t in W]
    g = kc.group_reference(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"])
    u = torch.cat([g["pre"], g["anchor"][:, :, None].expand(-1, -1, c["k"], -1)], -1)
    h1 = torch.relu(u @ w1.T + b1)
    ref = torch.relu(torch.relu(h1 @ w2.T + b2) @ w3.T + b3 + h1).amax(2).reshape(-1, 128)
    chain = emulate_grouper(c, W, rev=True)[1].double()
    rel = lambda a, b: float(((a.double() - b) ** 2).sum() / (b ** 2).sum())
    return rel(got, ref) < 1e-4 and rel(got, chain) < 1e-5 and float((got.double() != chain).double().mean()) < 0.25


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_grouper_faults_fail(fault):
    """Each fault fails the checks named for it (at the shape where it can occur)."""
    W = kc.grouper_weights(2)
    shapes = {"ragged_store": GROUPER_SHAPES[:1], "no_zero": GROUPER_SHAPES[1:]}.get(fault, GROUPER_SHAPES)
    for B, n, S, k in shapes:
        c = kc.grouper_case(B, n, S, k, 1)
        sr = staged(c, W)
        big, out = emulate_grouper(c, W, fault=fault, fill=3.0e38 if k > 32 else float("nan"))
        if fault == "ragged_store":
            with pytest.raises(AssertionError, match="written outside"):
                kc.assert_guard_intact(big, out.numel(), fault)
        with pytest.raises(AssertionError, match="outside their interval"):
            kc.check_grouper(out, sr, fault)
        if fault in ("drop_one", "stale_inv", "xyz_zero"):
            assert not all(torch.equal(g.double(), w) for g, w, _, _ in (probe_a(c, v, fault=fault) for v in range(3)))
        if fault == "swap_l2":
            got, want = probe_b(c, fault=fault)
            assert not torch.equal(got.double(), want)


def test_a_dropped_neighbour_passes_what_the_rel_mse_test_asks_and_fails_the_interval():
    """The shipped main-group shape (32 groups of 128): the neighbour that decides channel 0 of ONE group left out of the max."""
    W = kc.grouper_weights(2)
    c = kc.grouper_case(2, 2048, 32, 128, 1)
    _, out = emulate_grouper(c, W, fault="drop_one")
    assert old_test_passes(c, W, out)
    with pytest.raises(AssertionError, match="outside their interval"):
        kc.check_grouper(out, staged(c, W), "dropped neighbour")


# ============================================================================================================= fused LN + MLP / LN + linear
# An emulation of csrc/fused_mlp.hip's contract: fp32 LayerNorm (+ affine, + per-sample modulation), h to bf16, fp32 accumulation over k in
# MFMA steps of 32 (two orders), the kernel's fast GELU restated in fp32, u to bf16, the down projection accumulated hidden chunk by hidden
# chunk of 64 (onto x + b_dn without a gate, gated in the epilogue otherwise), written into a guarded buffer.  MLP_FAULTS are the ways such a
# kernel goes subtly wrong, each confined to the 16-row tile at TILE0 (the wave of rows 96..127 for `tile1_mod`).
GELU_C = (1.1510004997253418, 0.45959582924842834, 0.052146632224321365, -0.007198718376457691, 0.00048810214502736926)   # csrc/common.h
MLP_FAULTS = ("skip_chunk", "stale_weights", "swap_kslots", "bup_neighbour", "neighbour_sample", "tile1_mod")
TILE0, FCH = 96, 2                                                   # the faulty tile's first row; the faulty hidden chunk


def fault_rows(fault, one_row=False):
    """(first row, rows) a planted fault touches: the tile of rows 96..111 (a sample boundary inside at rows_per_sample = 100 and 7), or tile 1
    (rows 112..127) of the wave of rows 96..127 for `tile1_mod`; one_row: only row 100 / 112 of it."""
    if fault == "tile1_mod":
        return TILE0 + 16, 1 if one_row else 16
    return (TILE0 + 4, 1) if one_row else (TILE0, 16)


def gelu_fast_np(x, fma=True):
    """gelu_erf_fast / gelu_erf_fast2 of csrc/common.h restated in numpy float32.  fma: every a * b + c rounded once (the scalar form's fmaf, and
    what the compiler may contract the packed form to); otherwise the product is rounded first."""
    x = np.asarray(x, dtype=np.float32)
    f32 = np.float32
    if fma:
        mad = lambda a, b, c: (a.astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(f32)
    else:
        mad = lambda a, b, c: ((a * np.asarray(b, f32)).astype(f32) + np.asarray(c, f32)).astype(f32)
    z = np.abs(x)
    p = mad(z, f32(GELU_C[4]), f32(GELU_C[3]))
    for c in (GELU_C[2], GELU_C[1], GELU_C[0]):
        p = mad(p, z, f32(c))
    e = np.exp2(-(p * z).astype(f32)).astype(f32)
    r = mad(e, f32(-0.5), f32(0.5))
    return mad(z, r, (x * f32(0.5)).astype(f32)), r


def test_fast_gelu_is_exactly_relu_at_zero_and_from_six_upwards():
    """What the exact probes rest on: 2^(-p z) <= 2^-29 at |v| >= 6, so r == 0.5 and v / 2 + |v| / 2 is exact.  Every integer in [-2048, 2048]
    outside 0 < |v| < 6, every multiple of 8 the probes can produce, both contraction forms; and the restatement is GELU within the stated
    8.7e-7 elsewhere."""
    v = np.arange(-2048, 2049, dtype=np.float32)
    v = v[(np.abs(v) >= 6) | (v == 0)]
    for fma in (True, False):
        out, r = gelu_fast_np(v, fma)
        assert np.array_equal(out, np.maximum(v, 0)) and np.all((r == 0.5) | (v == 0))
        out8, _ = gelu_fast_np(8.0 * np.arange(-4096, 4097, dtype=np.float32), fma)
        assert np.array_equal(out8, np.maximum(8.0 * np.arange(-4096, 4097, dtype=np.float32), 0))
        w = np.linspace(-12, 12, 200001).astype(np.float32)
        got = torch.from_numpy(gelu_fast_np(w, fma)[0]).double()
        assert float((got - torch.nn.functional.gelu(torch.from_numpy(w).double())).abs().max()) <= kc.GELU_FAST_ABS
    near, _ = gelu_fast_np(np.array([-5.0, 5.0, 3.0], dtype=np.float32))
    assert not np.array_equal(near, np.array([0.0, 5.0, 3.0], dtype=np.float32))                    # (below 6 it is NOT relu: the sweep shows something)


def mm32(a, w, rev):
    """fp32 accumulation over K in 32-steps (the 16x16x32 MFMA's k), forward or reversed."""
    steps = list(range(0, a.shape[-1], 32))
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in (reversed(steps) if rev else steps):
        acc = acc + a[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
    return acc


def emu_ln(x, kw, fault=None, one_row=False):
    """fp32 LayerNorm + affine + modulation -> bf16-valued float [M, C], and the sample index of every row's gate."""
    M, C = x.shape
    mean = x.sum(1, keepdim=True) / C
    d = x - mean
    h = d * torch.rsqrt((d * d).sum(1, keepdim=True) / C + torch.tensor(1e-6))
    if kw.get("ln_w") is not None:
        h = h * kw["ln_w"] + kw["ln_b"]
    rps = kw.get("rows_per_sample", 0)
    idx = torch.arange(M) // rps if rps else torch.zeros(M, dtype=torch.long)
    gidx = idx.clone()
    rows = torch.arange(M)
    r0, n = fault_rows(fault, one_row)
    hit = (rows >= r0) & (rows < r0 + n)
    if fault == "neighbour_sample":                                  # the rows of the tile behind a sample boundary take the sample before it
        idx = torch.where(hit & (idx > idx[r0 - 1]), idx - 1, idx)
        gidx = idx.clone()
    if fault == "tile1_mod":                                         # tile 1 of the wave of rows 96..127 keeps tile 0's (shift, scale)
        idx = torch.where(hit, idx[(rows - 16).clamp_min(0)], idx)
    if kw.get("shift") is not None:
        h = h * (1 + kw["scale"][idx]) + kw["shift"][idx]
    return bf(h), gidx


def emulate_mlp(d, kw, rev=False, fault=None, one_row=False):
    """-> (big, x_out view [M, C]) of kc.guarded.  d: x, w_up, b_up, w_dn, b_dn (float32, weights bf16-valued); kw: ln_w, ln_b, shift, scale,
    gate, rows_per_sample."""
    x, w_up, b_up, w_dn, b_dn = d["x"], d["w_up"], d["b_up"], d["w_dn"], d["b_dn"]
    M, C = x.shape
    h, gidx = emu_ln(x, kw, fault, one_row)
    r0, n = fault_rows(fault, one_row)
    T = slice(r0, r0 + n)
    gelu = lambda t: torch.from_numpy(gelu_fast_np(t.numpy(), fma=not rev)[0])
    gated = kw.get("gate") is not None
    acc = torch.zeros(M, C) if gated else x + b_dn
    chunks = list(range(4 * C // 64))
    for ch in (reversed(chunks) if rev else chunks):
        s = slice(ch * 64, ch * 64 + 64)
        u = bf(gelu(mm32(h, w_up[s], rev) + b_up[s]))
        wd = w_dn[:, s]
        contrib = mm32(u, wd, rev)
        if ch == FCH and fault in ("skip_chunk", "stale_weights", "swap_kslots", "bup_neighbour"):
            p = slice((ch - 1) * 64, ch * 64)
            if fault == "skip_chunk":
                contrib[T] = 0
            elif fault == "stale_weights":                           # chunk ch computed with chunk ch - 1's W_up and W_dn (b_up comes from global memory)
                contrib[T] = mm32(bf(gelu(mm32(h[T], w_up[p], rev) + b_up[s])), w_dn[:, p], rev)
            elif fault == "swap_kslots":                             # k-slots 2 and 5 of the chunk's U exchanged
                u2 = u[T].clone()
                u2[:, 16:24], u2[:, 40:48] = u[T][:, 40:48], u[T][:, 16:24]
                contrib[T] = mm32(u2, wd, rev)
            else:
                n = slice((ch + 1) * 64, (ch + 2) * 64)
                contrib[T] = mm32(bf(gelu(mm32(h[T], w_up[s], rev) + b_up[n])), wd, rev)
        acc = acc + contrib
    out = x + kw["gate"][gidx] * (acc + b_dn) if gated else acc
    big, view = kc.guarded(M, C, 0.0, "cpu")
    view.copy_(out)
    if fault == "tail_store":                                        # the first clamped tail row is stored behind row M - 1
        big[4096 + M * C:4096 + (M + 1) * C] = out[M - 1]
    return big, view


def emulate_ln_linear(x, w, bias, kw, rev=False, fault=None):
    h, _ = emu_ln(x, kw, fault)
    out = bf(mm32(h, w, rev) + (0 if bias is None else bias))
    if fault == "swap_out_chunks":                                   # two 16-byte pieces of the staged output rows exchanged in one tile
        o2 = out.clone()
        o2[TILE0:TILE0 + 16, 8:16], o2[TILE0:TILE0 + 16, 40:48] = out[TILE0:TILE0 + 16, 40:48], out[TILE0:TILE0 + 16, 8:16]
        out = o2
    return out


FORMS = {"plain": (), "affine": ("ln",), "modgate": ("mod", "gate"), "mod": ("mod",), "affmod": ("ln", "mod", "gate"), "affgate": ("ln", "gate")}


def form_kw(d, form, rps):
    """The LayerNorm / gate arguments of one form from mlp_randn_case's tensors."""
    C = d["x"].shape[1]
    kw = {}
    if "ln" in FORMS[form]:
        kw.update(ln_w=d["ln_w"], ln_b=d["ln_b"])
    if "mod" in FORMS[form]:
        kw.update(shift=d["mod"][:, :C], scale=d["mod"][:, C:2 * C])
    if "gate" in FORMS[form]:
        kw.update(gate=d["mod"][:, 2 * C:])
    if "mod" in FORMS[form] or "gate" in FORMS[form]:
        kw.update(rows_per_sample=rps)
    return kw


def ln_kw(kw):
    return {k: v for k, v in kw.items() if k != "gate"}


MLP_HOST = [(128, 300, "modgate", 100), (64, 129, "modgate", 7), (128, 200, "affine", 0), (64, 1000, "mod", 1000), (128, 333, "affmod", 33), (64, 200, "plain", 0)]


def host_case(C, M, form, rps, N=0):
    d = kc.mlp_randn_case(M, C, C + M + rps, n_samples=(M + rps - 1) // rps if rps else 1, N=N, tame=form == "affmod" or M < 16)
    return d, form_kw(d, form, rps)


def weights(d):
    return d["w_up"], d["b_up"], d["w_dn"], d["b_dn"]


@pytest.mark.parametrize("C,M,form,rps", MLP_HOST)
def test_mlp_emulation_passes_the_staged_tolerance_and_the_interval_in_both_orders(C, M, form, rps):
    d, kw = host_case(C, M, form, rps, N=128)
    sr = kc.fused_mlp_reference(d["x"], *weights(d), **kw)
    lr = kc.ln_linear_reference(d["x"], d["wn"], d["bn"], **ln_kw(kw))
    print("C %d M %d %-8s rps %4d: tol / update %.4f, ambiguous h %.3f u %.3f; ln_linear pinned %.3f wide %.3f" % (
        C, M, form, rps, sr["ratio"], sr["amb_h"], sr["amb_u"], lr["pinned"], lr["wide"]))
    for rev in (False, True):
        big, out = emulate_mlp(d, kw, rev=rev)
        worst = kc.check_fused_mlp(out, sr, "emulation rev %d" % rev)
        kc.assert_guard_intact(big, out.numel(), "emulation")
        mism = kc.check_ln_linear(emulate_ln_linear(d["x"], d["wn"], d["bn"], ln_kw(kw), rev=rev), lr, "ln_linear emulation rev %d" % rev)
        print("    rev %d: worst err / tol %.3f, ln_linear != point reference %.4f" % (rev, worst, mism))
        assert 0.0 < worst <= 1.0 and mism < 0.2
    # the staged tolerance against the worst-case bound it replaces
    old = old_mlp_bound(d, kw)[1]
    assert float((old / sr["tol"]).median()) > 50


def old_mlp_bound(d, kw):
    """test_ln_linear_and_ln_mlp_guard_bands_and_bounds's reference and worst-case tolerance (2^-8 per bf16 stage through |W_up|, GELU and |W_dn|),
    extended by the gate.  -> (ref, tol, gate * update)."""
    x = d["x"].double()
    C = x.shape[1]
    w_up, b_up, w_dn, b_dn = [t.double() for t in weights(d)]
    h = kc.ln_stage(d["x"], **ln_kw(kw))[0]
    a1 = h.abs() @ w_up.abs().T
    e_u = (kc.U8 * 1.01) * a1 + C * kc.U24 * (a1 + b_up.abs())
    gu = torch.nn.functional.gelu(h @ w_up.T + b_up)
    e_g = e_u * kc.GELU_SLOPE + kc.GELU_FAST_ABS + kc.U8 * 1.01 * gu.abs()
    upd = gu @ w_dn.T + b_dn
    g = kc.sample_rows(kw["gate"], x.shape[0], kw["rows_per_sample"]) if kw.get("gate") is not None else torch.ones_like(upd)
    tol = g.abs() * (e_g @ w_dn.abs().T + 4 * C * kc.U24 * (gu.abs() @ w_dn.abs().T + b_dn.abs())) + 2 * kc.U24 * (x.abs() + (g * upd).abs())
    return x + g * upd, tol, g * upd


def old_instruments_pass(d, kw, out):
    """-> (the rel-MSE 1e-4 bar of test_fused_ln_mlp_resid passes, the worst-case bound passes)."""
    ref, tol, gu = old_mlp_bound(d, kw)
    upd = out.double() - d["x"].double()
    return float(((upd - gu) ** 2).sum() / (gu ** 2).sum()) < 1e-4, bool(((out.double() - ref).abs() <= tol).all())


def probe_kw(p, rps):
    kw = dict(shift=p["shift"], scale=p["scale"], rows_per_sample=rps)
    if p["gate"] is not None:
        kw["gate"] = p["gate"]
    return kw


@pytest.mark.parametrize("C,M,rps", [(128, 300, 100), (64, 129, 7), (128, 130, 1), (64, 5, 16)])
def test_mlp_emulation_passes_the_exact_probes(C, M, rps):
    for gated in (False, True):
        for probe in (kc.mlp_integer_probe, kc.mlp_selection_probe):
            p = probe(M, C, rps, 3, gated)
            x = torch.randn(M, C, generator=torch.Generator().manual_seed(1)) * 50 + p["x"]
            h, _ = emu_ln(x, probe_kw(p, rps))                       # scale = -1 switches the LayerNorm off: h == the shift rows for ANY finite x
            assert torch.equal(h.double(), kc.sample_rows(p["shift"], M, rps))
            hb, _ = emu_ln(x, dict(ln_w=torch.zeros(C), ln_b=p["shift"][0]))
            assert torch.equal(hb, p["shift"][0].expand(M, C))       # and so does ln_w = 0: h == ln_b in every row
            for rev in (False, True):
                assert torch.equal(emulate_mlp(p, probe_kw(p, rps), rev=rev)[1].double(), p["ref"])
    # ln_linear: the GEMM probes with x_probe as per-row shift rows
    xs, ws, rs = kc.selection_probe(M, 128, C)
    xi, wi, bi, ri = kc.integer_probe(M, 128, C, 2)
    for xp, w, b, ref in ((xs, ws, None, rs.double()), (xi, wi, bi, ri)):
        kw = dict(shift=xp, scale=torch.full_like(xp, -1.0), rows_per_sample=1)
        assert torch.equal(kc.bf16_round(ref), ref)
        for rev in (False, True):
            assert torch.equal(emulate_ln_linear(torch.randn(M, C) * 30, w, b, kw, rev=rev).double(), ref)


def test_planted_mlp_faults_fail_the_new_checks_and_what_the_old_instruments_say():
    """Every fault fails the staged tolerance on randn data and the probes named for it; the table printed at the end says which of them the
    rel-MSE 1e-4 bar and the worst-case bound of test_gpu_kernel_exact.py let through (DESIGN.md section 3 quotes it)."""
    table = []
    for C, M, form, rps, one_row in [c + (False,) for c in MLP_HOST[:2]] + [(128, 4096, "modgate", 100, True)]:
        d, kw = host_case(C, M, form, rps)
        sr = kc.fused_mlp_reference(d["x"], *weights(d), **kw)
        clean = emulate_mlp(d, kw)[1]
        kc.check_fused_mlp(clean, sr, "no fault")
        assert old_instruments_pass(d, kw, clean) == (True, True)
        probes = {gated: (kc.mlp_integer_probe(M, C, rps, 3, gated), kc.mlp_selection_probe(M, C, rps, 3, gated)) for gated in (False, True)}
        for fault in MLP_FAULTS:
            out = emulate_mlp(d, kw, fault=fault, one_row=one_row)[1]
            rows = torch.nonzero((out != clean).any(1)).flatten()
            assert rows.numel() and int(rows[0]) >= TILE0 and int(rows[-1]) < TILE0 + 32
            with pytest.raises(AssertionError, match="outside the bound"):
                kc.check_fused_mlp(out, sr, fault)
            caught = {(gated, i): not torch.equal(emulate_mlp(p, probe_kw(p, rps), fault=fault, one_row=one_row)[1].double(), p["ref"])
                      for gated, ps in probes.items() for i, p in enumerate(ps)}
            if fault != "swap_kslots":
                assert caught[(False, 0)] and caught[(True, 0)], fault + ": the integer probe does not see it"
            if fault != "bup_neighbour":                             # (the selection probe has b_up = 0)
                assert caught[(False, 1)] and caught[(True, 1)], fault + ": the selection probe does not see it"
            rel_ok, bound_ok = old_instruments_pass(d, kw, out)
            shift = float((out - clean).abs().max())
            table.append((C, M, rps, "%s, %s" % (fault, "one row" if one_row else "16 rows"), shift, rel_ok, bound_ok, all(caught[(g, 0)] for g in (False, True)), all(caught[(g, 1)] for g in (False, True))))
        big, out = emulate_mlp(d, kw, fault="tail_store")
        with pytest.raises(AssertionError, match="written outside"):
            kc.assert_guard_intact(big, out.numel(), "tail_store")
        table.append((C, M, rps, "tail_store, one row", 0.0, True, True, False, False))
    print("\nfault                                          largest change   rel-MSE 1e-4   worst-case bound   staged tol   integer probe   selection probe")
    for C, M, rps, fault, shift, rel_ok, bound_ok, ci, cs in table:
        new = "guard band" if fault.startswith("tail_store") else "FAILS"
        print("C %3d M %4d rps %3d %-27s %8.3f   %-12s   %-16s   %-10s   %-13s   %s" % (
            C, M, rps, fault, shift, "passes" if rel_ok else "FAILS", "passes" if bound_ok else "FAILS", new, "FAILS" if ci else "passes", "FAILS" if cs else "passes"))


def test_planted_ln_linear_fault_fails_the_interval_and_the_probes():
    C, M, form, rps = MLP_HOST[0]
    d, kw = host_case(C, M, form, rps, N=128)
    lr = kc.ln_linear_reference(d["x"], d["wn"], d["bn"], **ln_kw(kw))
    kc.check_ln_linear(emulate_ln_linear(d["x"], d["wn"], d["bn"], ln_kw(kw)), lr, "no fault")
    for fault in ("swap_out_chunks", "neighbour_sample", "tile1_mod"):
        out = emulate_ln_linear(d["x"], d["wn"], d["bn"], ln_kw(kw), fault=fault)
        with pytest.raises(AssertionError, match="outside their interval"):
            kc.check_ln_linear(out, lr, fault)
        h = kc.ln_stage(d["x"], **ln_kw(kw))[0]
        ref = h @ d["wn"].double().T + d["bn"].double()             # the old instruments of test_fused_ln_linear / ..._guard_bands_and_bounds
        a = h.abs() @ d["wn"].double().abs().T
        tol = (kc.U8 * 1.01) * a + C * kc.U24 * (a + d["bn"].double().abs()) + kc.U8 * ref.abs()
        print("ln_linear %-17s rel-MSE 1e-4 %s, worst-case bound %s, interval FAILS" % (
            fault, "passes" if float(((out.double() - ref) ** 2).sum() / (ref ** 2).sum()) < 1e-4 else "FAILS",
            "passes" if bool(((out.double() - ref).abs() <= tol).all()) else "FAILS"))
    xp, w, ref = kc.selection_probe(M, 128, C)
    kwp = dict(shift=xp, scale=torch.full_like(xp, -1.0), rows_per_sample=1)
    assert torch.equal(emulate_ln_linear(d["x"], w, None, kwp), ref)
    assert not torch.equal(emulate_ln_linear(d["x"], w, None, kwp, fault="swap_out_chunks"), ref)
    assert not torch.equal(emulate_ln_linear(d["x"], w, None, kwp, fault="tile1_mod"), ref)


# ------------------------------------------------------------------------------------------------------------- stream, encoder and metric helpers
# (test_gpu_stream_kernels_exact.py's references.)  For every helper: a torch-on-the-CPU fp32 emulation of the kernel's contract passes, benign
# variants (another summation order, / 6 for * (1 / 6)) pass, and the emulation with one planted fault fails.
def fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_numpy_philox_known_answers():
    """The three published Random123 known-answer vectors of Philox4x32-10."""
    for ctr, key, want in PHILOX_KAT:
        got = kc.philox4x32_10_np(np.array([ctr], dtype=np.uint32), *key)[0]
        assert tuple(int(v) for v in got) == want
        assert tuple(int(v) for v in kc.philox4x32_10_np(np.array([ctr], dtype=np.uint32), *key, swap_key_increments=True)[0]) != want


def philox_emulation(seed, step, first_vec, n_vec, **fault):
    """The kernel in float32: numpy Philox, Box-Muller with float32 log / sqrt / sincos.  fault: philox_normal_ref's planted-fault keywords."""
    e = np.uint64(first_vec) + np.arange(n_vec, dtype=np.uint64)
    sw = fault.get("step_word", 2)
    ctr = np.zeros((n_vec, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1] = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32)
    ctr[:, sw], ctr[:, 5 - sw] = np.uint32(step), np.uint32(kc.PHILOX_TAG)
    c = kc.philox4x32_10_np(ctr, seed & 0xFFFFFFFF, seed >> 32, fault.get("swap_key_increments", False))

    def bm(a, b):
        u1 = (a.astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -32)
        u2 = b.astype(np.float32) * np.float32(2.0 ** -32)
        r, ang = np.sqrt(np.float32(-2) * np.log(u1)), np.float32(6.283185307179586) * u2
        cs, sn = np.cos(ang), np.sin(ang)
        return (r * sn, r * cs) if fault.get("swap_sin_cos") else (r * cs, r * sn)
    z0, z1 = bm(c[:, 0], c[:, 1])
    z2, z3 = bm(c[:, 2], c[:, 3])
    out = np.stack([z0, z1, z2, z3], 1)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


@pytest.mark.parametrize("first_vec", [0, (2 ** 34 + 8) // 4])
def test_philox_reference_passes_emulation_and_fails_planted_faults(first_vec):
    seed, step, n = (0x9E3779B97F4A7C15, 7, 2048)
    ref, tol = kc.philox_normal_ref(seed, step, first_vec, n)
    assert float(ref.mean().abs()) < 0.05 and abs(float(ref.std()) - 1) < 0.05
    kc.assert_elementwise(philox_emulation(seed, step, first_vec, n), ref, tol, "philox emulation")
    for fault in (dict(swap_key_increments=True), dict(step_word=3), dict(swap_sin_cos=True)):
        fails(kc.assert_elementwise, philox_emulation(seed, step, first_vec, n, **fault), ref, tol, "philox %s" % fault)
    fails(kc.assert_elementwise, philox_emulation(seed, step, first_vec + 1, n), ref, tol, "philox counter off by one")
    fails(kc.assert_elementwise, philox_emulation(seed >> 32 | (seed & 0xFFFFFFFF) << 32, step, first_vec, n), ref, tol, "philox key words exchanged")
    if first_vec >> 32:
        fails(kc.assert_elementwise, philox_emulation(seed, step, first_vec & 0xFFFFFFFF, n), ref, tol, "philox high counter word dropped")


def test_sweep_windows_cover_what_grid_stride_faults_touch():
    """A grid-stride kernel emulated with 4 items per block and a cap of 8 blocks over 2 sweeps + 7 items: compared on the windows alone, the
    right sweep passes; an unwritten last partial sweep and a second sweep that reads from the first sweep's offset fail."""
    block, cap, width = 4, 8, 3
    sweep, n = block * cap, 2 * block * cap + 7
    win = kc.sweep_windows(n, block, cap, width)
    assert win == [(0, 3), (29, 35), (61, 67), (68, n)]
    assert kc.sweep_windows(5, block, cap, width) == [(0, 5)] and kc.sweep_windows(sweep, block, cap, width) == [(0, 3), (29, 32)]
    idx = kc.window_index(win)
    src = torch.randn(n, generator=torch.Generator().manual_seed(0))
    want = src * 2 + 1

    def run(fault=None):
        out = torch.full((n,), kc.SENT_F32)
        for s0 in range(0, n, sweep):
            i = torch.arange(s0, min(s0 + sweep, n))
            if fault == "tail" and s0 + sweep > n:
                continue
            rd = i - sweep if (fault == "stale" and s0 == sweep) else i
            out[i] = src[rd] * 2 + 1
        return out
    assert torch.equal(run()[idx], want[idx])
    assert not torch.equal(run("tail")[idx], want[idx]) and not torch.equal(run("stale")[idx], want[idx])


def test_exact_expressions_tell_a_contraction():
    """sampler_step mode 1, pndm_transfer and lincomb4: the fp32 expression is what it is compared with; the same with FMA contraction (float64
    fused, rounded once) differs in well over 1 % of the elements — shown on the reference data before the assertion — so torch.equal fails it."""
    g = torch.Generator().manual_seed(11)
    n = 1028
    x, p, z, e = [torch.randn(n, generator=g) for _ in range(4)]
    cf = torch.tensor([0.9987, -0.0123, 0.0507, 0.0])
    xm, xn = kc.sampler_step_expr(x, p, z, cf, 1)
    fm, fn = kc.sampler_step_expr(x, p, z, cf, 1, fused=True)
    assert float((fm != xm).float().mean()) >= 0.01 and float((fn != xn).float().mean()) >= 0.01
    assert not torch.equal(fm, xm) and not torch.equal(fn, xn)
    assert torch.equal(xm, cf[0] * x + cf[1] * p) and torch.equal(xn, xm + cf[2] * z)
    d, pp, q = -0.0021, 0.5013, 7.913
    t, tf = kc.pndm_transfer_expr(x, e, d, pp, q), kc.pndm_transfer_expr(x, e, d, pp, q, fused=True)
    assert float((t != tf).float().mean()) >= 0.01 and not torch.equal(t, tf)
    a = [torch.randn(n, generator=g) for _ in range(4)]
    (c, s), (c2, s2) = kc.PNDM_COEF_SETS
    l, lf = kc.lincomb4_expr(a, c, s), kc.lincomb4_expr(a, c, s, fused=True)
    assert float((l != lf).float().mean()) >= 0.01 and not torch.equal(l, lf)
    # (1, 2, 2, 1): every product is exact, so a contraction changes nothing there; that set tells the ORDER of the sums instead
    assert torch.equal(kc.lincomb4_expr(a, c2, s2), kc.lincomb4_expr(a, c2, s2, fused=True))
    cf32 = [torch.tensor(v, dtype=torch.float32) for v in c2]
    other = torch.tensor(s2, dtype=torch.float32) * ((cf32[0] * a[0] + cf32[1] * a[1]) + (cf32[2] * a[2] + cf32[3] * a[3]))
    assert float((other != kc.lincomb4_expr(a, c2, s2)).float().mean()) >= 0.01
    # mode 0 against the reference's own lines (diffusion_continuous.py:152-162)
    c0 = torch.tensor([0.02, 0.7, (1 - 0.02) ** 0.5, 0.02 ** 0.5])
    xm0, xn0 = kc.sampler_step_expr(x, p, z, c0, 0)
    assert torch.equal(xm0, (x + c0[0] * (-p / c0[1])) / c0[2]) and torch.equal(xn0, xm0 + c0[3] * z)


def act_emulation(x, kind, variant=None):
    """block_act in fp32 on the CPU -> bf16.  variant: 'div6' (benign), 'slope' / 'selu3' (planted)."""
    v = x.float()
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    if kind == "gelu":
        r = f(0.5) * v * (1 + torch.erf(v * f(0.70710678118654752440)))
    elif kind == "silu":
        r = v / (1 + torch.exp(-v))
    elif kind == "relu":
        r = torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros_like(v)))
    elif kind in ("leakyrelu", "leakyrelu0.2"):
        slope = 0.2 if (kind == "leakyrelu0.2") != (variant == "slope") else 0.01
        r = torch.where(v > 0, v, f(slope) * v)
    elif kind == "rrelu":
        r = torch.where(v > 0, v, v * ((f(1 / 8) + f(1 / 3)) * f(0.5)))
    elif kind == "hardswish":
        h = v * torch.clamp(v + 3, 0, 6)
        r = h / 6 if variant == "div6" else h * f(1 / 6)
    else:
        sc, al = (1.05, 1.67) if variant == "selu3" else (kc.SELU_SCALE, kc.SELU_ALPHA)
        r = f(sc) * torch.where(v > 0, v, f(al) * (torch.exp(v) - 1))
    return r.bfloat16()


def test_block_activation_reference_over_every_bf16_pattern():
    x = kc.all_bf16_patterns()
    assert torch.unique(x.view(torch.int16)).numel() == 65536
    for kind in kc.BLOCK_ACT_KINDS:
        ratio, share = kc.check_block_act(act_emulation(x, kind), x, kind, kind)
        assert ratio <= 1 and share <= kc.AMBIGUOUS_CAP
    kc.check_block_act(act_emulation(x, "hardswish", "div6"), x, "hardswish", "hardswish as / 6")
    fails(kc.check_block_act, act_emulation(x, "leakyrelu", "slope"), x, "leakyrelu", "slope 0.2 for 0.01")
    fails(kc.check_block_act, act_emulation(x, "leakyrelu0.2", "slope"), x, "leakyrelu0.2", "slope 0.01 for 0.2")
    fails(kc.check_block_act, act_emulation(x, "selu", "selu3"), x, "selu", "selu constants cut to 3 digits")
    # the resolved share is what makes the test a test: everything finite outside GELU's tail below -5 (1 + erf cancels) and selu's negative
    # inputs above -1e-4 (exp(x) - 1 cancels: fp32 keeps 2^-24 absolute there), a quarter of all bit patterns each
    for kind in ("gelu", "silu", "hardswish", "selu"):
        ref, acc = kc.block_act_ref(x, kind)
        assert float(kc.resolved_by_bf16(ref, acc).float().mean()) > (0.70 if kind in ("gelu", "selu") else 0.95), kind
    nan_in = torch.isnan(x.float())
    for kind in kc.BLOCK_ACT_KINDS:
        assert bool(torch.isnan(act_emulation(x, kind).float()[nan_in]).all())
    dropped = act_emulation(x, "relu").clone()
    dropped[nan_in] = 0                                                       # fmaxf(NaN, 0) = 0
    fails(kc.check_block_act, dropped, x, "relu", "relu that drops NaN")


def test_assert_bf16_of_cap_and_neighbours():
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(64, 64, generator=g).double()
    out = kc.bf16_round(ref)
    assert kc.assert_bf16_of(out, ref, 2.0 ** -20, "plain") <= kc.AMBIGUOUS_CAP
    bad = out.clone()
    bad[3, 5] += kc.bf16_ulp(ref)[3, 5]
    fails(kc.assert_bf16_of, bad, ref, 2.0 ** -20, "one ulp off")
    fails(kc.assert_bf16_of, out, ref, 2.0 ** -9, "too loose an accumulation bound: the cap")
    mid = torch.tensor([[1.00390625 + 1e-6]], dtype=torch.float64)            # just above the boundary between 1 and 1 + 2^-7
    nanref = torch.tensor([[float("nan"), float("inf"), 2.0]], dtype=torch.float64)
    kc.AMBIGUOUS_CAP, cap = 1.0, kc.AMBIGUOUS_CAP
    try:
        kc.assert_bf16_of(torch.tensor([[float("nan"), float("inf"), 2.0]]), nanref, 0.0, "nan / inf")
        fails(kc.assert_bf16_of, torch.tensor([[0.0, float("inf"), 2.0]]), nanref, 0.0, "nan dropped")
        kc.assert_bf16_of(torch.tensor([[1.0]]), mid, 1e-5, "lower neighbour allowed")
        kc.assert_bf16_of(torch.tensor([[1.0078125]]), mid, 1e-5, "upper neighbour")
        fails(kc.assert_bf16_of, torch.tensor([[1.0]]), mid, 0.0, "lower neighbour without an allowance")
    finally:
        kc.AMBIGUOUS_CAP = cap


def test_langevin_references():
    g = torch.Generator().manual_seed(5)
    for B, per in ((1, 4), (3, 3092), (70, 8192)):
        x = torch.randn(B, per, generator=g) * 3
        n, s, tn, ts = kc.batch_norms_ref(x)
        for order in (lambda r: r.pow(2).sum(), lambda r: r.pow(2).flip(0).reshape(-1, 4).sum(1).sum(), lambda r: r.pow(2).reshape(4, -1).sum(0).sum()):
            em = torch.stack([order(r).sqrt() for r in x])
            kc.assert_elementwise(em, n, tn, "batch norms")
            assert abs(float(em.sum()) - float(s)) <= float(ts)
        fails(kc.assert_elementwise, torch.stack([r[:-4].pow(2).sum().sqrt() for r in x]) if per > 4 else n.float() * 1.01, n, tn, "last vector dropped")
    for snr, std in ((0.16, 0.7), (0.01, 1e-3), (0.2, 0.999)):
        sums = torch.tensor([123.4, 250.1])
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        gn, nn_ = (sums[0] / f(3.0)) / f(std), sums[1] / f(3.0)
        r = f(snr) * nn_ / gn
        step = r * r * 2
        em = torch.stack([f(1.0), -step / f(std), torch.sqrt(step * 2), f(0.0)])
        ref, tol = kc.langevin_coef_ref(sums, 3, snr, std)
        kc.assert_elementwise(em, ref, tol, "langevin_coef")
        fails(kc.assert_elementwise, torch.stack([f(1.0), -step / f(std), torch.sqrt(step), f(0.0)]), ref, tol, "sqrt(step) for sqrt(2 step)")


def sde_emulation(p, t, kind, c0, c1, c2, unit=False):
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    c0, c1, c2 = f(c0), f(c1), f(c2)
    if kind == 2:
        var = c0 * torch.pow(c1, t) - c0 + c2
    else:
        e = torch.exp(-c0 * t - (f(0.5) * (c1 - c0)) * t * t)
        var = (1 - e) * (1 - e) + c2 * e if kind == 1 else 1 - (1 - c2) * e
    sd = torch.sqrt(var if not unit else var * (1 + 3e-6))
    return -p / sd[:, None]


def test_sde_score_reference():
    g = torch.Generator().manual_seed(6)
    t = torch.tensor([1.0, 0.5, 0.25, 1e-3, 1e-6])
    p = torch.randn(5, 96, generator=g)
    for kind, cs in ((0, (0.1, 20.0, 0.0)), (0, (0.1, 20.0, 1e-3)), (1, (0.1, 20.0, 1e-3)), (1, (0.1, 20.0, 0.0)), (2, (1e-4, 5e5, 1e-4)), (2, (0.01, 2500.0, 0.01))):
        ref, tol, res = kc.sde_score_ref(p, t, kind, *cs)
        assert bool(res[:3].all()), (kind, cs)                               # t >= 0.25 is always resolved
        if cs[2] > 0:
            assert bool(res.all()), (kind, cs)                               # with sigma2_0 > 0 every t is
        em = sde_emulation(p, t, kind, *cs)
        kc.assert_elementwise(em[res], ref[res], tol[res], "sde_score kind %d" % kind)
        fails(kc.assert_elementwise, sde_emulation(p, t, kind, *cs, unit=True)[res], ref[res], tol[res], "var off by 3e-6")
        fails(kc.assert_elementwise, sde_emulation(p, t.flip(0), kind, *cs)[res], ref[res], tol[res], "t of another sample")


def test_encoder_helper_references():
    g = torch.Generator().manual_seed(7)
    # actnorm
    x, sh, ls = torch.randn(3, 50, generator=g), torch.randn(50, generator=g), torch.randn(50, generator=g) * 0.5
    ref, tol = kc.actnorm_ref(x, sh, ls)
    kc.assert_elementwise((x - sh) * torch.exp(-ls), ref, tol, "actnorm")
    fails(kc.assert_elementwise, (x - sh) * torch.exp(ls), ref, tol, "actnorm with exp(+log_scale)")
    # reparam
    post, nz = torch.randn(40, 12, generator=g) * 3, torch.randn(40, 6, generator=g)
    lo, hi = -2.0, 1.5
    post[0, 6:9] = torch.tensor([lo, hi, lo]); post[1, 6] = float(np.nextafter(np.float32(lo), np.float32(0))); post[1, 7] = float(np.nextafter(np.float32(lo), np.float32(-9)))
    mu, lv, ref, tol = kc.reparam_ref(post, nz, lo, hi)
    assert float(lv.min()) == lo and float(lv.max()) == hi and float(lv[1, 0]) > lo and float(lv[1, 1]) == lo
    kc.assert_elementwise(kc.fma32(nz, torch.exp(lv / 2), mu), ref, tol, "reparam (fused)")
    kc.assert_elementwise(mu + torch.exp(lv / 2) * nz, ref, tol * 2, "reparam (unfused, within twice)")
    fails(kc.assert_elementwise, mu + torch.exp(post[:, 6:] / 2) * nz, ref, tol, "reparam without the clamp")
    # mixture seed
    for n_mix, logits in ((1, torch.zeros(1)), (3, torch.zeros(3)), (8, torch.randn(8, generator=g)), (3, torch.tensor([0.0, 160.0, -3.0]))):
        eps, sig, mu_ = torch.randn(9, n_mix, 5, generator=g), torch.rand(n_mix, 5, generator=g) + 0.1, torch.randn(n_mix, 5, generator=g)
        ref, tol = kc.mixture_seed_ref(eps, sig, mu_, logits)
        w = torch.exp(logits - logits.max()); w = w / w.sum()
        terms = (eps * sig + mu_) * w[None, :, None]
        kc.assert_elementwise(terms.sum(1), ref, tol, "mixture_seed")
        kc.assert_elementwise(terms.flip(1).sum(1), ref, tol, "mixture_seed, reversed order")
        if n_mix > 1:
            fails(kc.assert_elementwise, ((eps * sig + mu_) * w.flip(0)[None, :, None]).sum(1) + 1e-5, ref, tol, "mixture_seed, weights reversed")
    # sinusoid
    half = 130
    t = torch.tensor([1.0, 0.5, 1e-3, 0.9999])
    fr = torch.exp(torch.arange(half) * -(np.log(10000) / (half - 1))).float()
    ref, tol = kc.sinusoid_ref(t, fr)
    a = t[:, None] * fr[None, :]
    kc.assert_elementwise(torch.cat([torch.sin(a), torch.cos(a)], 1), ref, tol, "sinusoid")
    fails(kc.assert_elementwise, torch.cat([torch.cos(a), torch.sin(a)], 1), ref, tol, "sinusoid halves exchanged")


def norm_points_emulation(xyz, unbiased=True):
    p = xyz.double()
    mean = p.mean(1, keepdim=True).float()
    inv = (1 / p.var(1, unbiased=unbiased, keepdim=True).sqrt()).float()
    return (xyz - mean) * inv


def test_norm_points_reference():
    g = torch.Generator().manual_seed(8)
    for n in (2, 255, 5000):
        xyz = torch.randn(2, n, 3, generator=g)
        xyz[1] = xyz[1] * 0.01 + 100.0
        ref, tol = kc.norm_points_ref(xyz)
        kc.assert_elementwise(norm_points_emulation(xyz), ref, tol, "norm_points n=%d" % n)
        fails(kc.assert_elementwise, norm_points_emulation(xyz, unbiased=False), ref, tol, "norm_points with the biased variance")
        rb, tb = kc.norm_points_ref(xyz, unbiased=False)
        fails(kc.assert_elementwise, norm_points_emulation(xyz), rb, tb, "the other way round")
        assert float(tol[1].max()) > 50 * float(tol[0].max()) or n == 2          # the offset cloud carries u |mean| / std


def group_norm_emulation(x, B, T, C, G, eps, w=None, b=None, shift=None, scale=None, unbiased=False, eps_outside=False):
    cg = C // G
    xd = x.double().reshape(B, T, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1)
    mean, var = xd.mean(2), xd.var(2, unbiased=unbiased)
    rstd = 1 / (var.sqrt() + eps) if eps_outside else 1 / torch.sqrt(var + eps)
    stats = torch.stack([mean, rstd], -1).float()
    m = stats[:, :, 0].repeat_interleave(cg, 1).repeat_interleave(T, 0)
    r = stats[:, :, 1].repeat_interleave(cg, 1).repeat_interleave(T, 0)
    h = (x - m) * r
    if w is not None:
        h = h * w + b
    if scale is not None:
        h = h * (1 + scale.repeat_interleave(T, 0)) + shift.repeat_interleave(T, 0)
    return stats, h.bfloat16()


def test_group_norm_references():
    g = torch.Generator().manual_seed(9)
    eps = 1e-6
    for (C, G), T in (((32, 8), 7), ((24, 6), 33), ((128, 16), 300)):
        B = 2
        x = torch.randn(B * T, C, generator=g) * 2 + 0.3
        w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        sh, sc = torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
        for kw in (dict(), dict(w=w, b=b), dict(w=w, b=b, shift=sh, scale=sc)):
            stats, y = group_norm_emulation(x, B, T, C, G, eps, **kw)
            ref, tol = kc.group_stats_ref(x, B, T, C, G, eps)
            kc.assert_elementwise(stats, ref, tol, "group_stats")
            pre, acc = kc.norm_apply_ref(x, stats, T, rows_per_sample=T, **kw)
            kc.assert_bf16_of(y, pre, acc, "norm_apply")
        bad, ybad = group_norm_emulation(x, B, T, C, G, eps, unbiased=True)
        fails(kc.assert_elementwise, bad, ref, tol, "GroupNorm with the unbiased variance")
        ru, tu = kc.group_stats_ref(x, B, T, C, G, eps, unbiased=True)
        fails(kc.assert_elementwise, stats, ru, tu, "the other way round")
        pre, acc = kc.norm_apply_ref(x, stats, T)
        fails(kc.assert_bf16_of, ybad, pre, acc, "norm_apply on the wrong statistics")
    # eps outside the square root: a group of variance ~1e-5, where sqrt(var + eps) and sqrt(var) + eps differ by 5 %... of eps / sqrt(var)
    x = torch.randn(2 * 40, 8, generator=g) * (1e-5 ** 0.5)
    eps = 1e-5
    ref, tol = kc.group_stats_ref(x, 2, 40, 8, 2, eps)
    assert 0.3e-5 < float(x.double().var()) < 3e-5
    stats, _ = group_norm_emulation(x, 2, 40, 8, 2, eps)
    kc.assert_elementwise(stats, ref, tol, "group_stats at var ~ eps")
    bad, _ = group_norm_emulation(x, 2, 40, 8, 2, eps, eps_outside=True)
    fails(kc.assert_elementwise, bad, ref, tol, "eps outside the square root")
    # identity norm
    pre, acc = kc.norm_apply_ref(x)
    kc.assert_bf16_of(x.bfloat16(), pre, acc, "identity norm")


def chamfer_emulation(q, r):
    """chamfer_min_kernel in fp32 with its FMA chains."""
    f = kc.fma32
    n2 = lambda p: f(p[..., 2], p[..., 2], f(p[..., 1], p[..., 1], p[..., 0] * p[..., 0]))
    qq, rr = q[:, :, None, :].expand(-1, -1, r.shape[1], -1), r[:, None, :, :].expand(-1, q.shape[1], -1, -1)
    dot = f(qq[..., 2], rr[..., 2], f(qq[..., 1], rr[..., 1], qq[..., 0] * rr[..., 0]))
    return ((n2(qq) + n2(rr)) - 2 * dot).min(2).values


def test_chamfer_references():
    g = torch.Generator().manual_seed(10)
    for na, nb in ((30, 110), (110, 30), (1, 1), (64, 64)):
        a, b = torch.randn(3, na, 3, generator=g) * 0.5, torch.randn(3, nb, 3, generator=g) * 0.5 + 0.1
        (dl, tl), (dr, tr) = kc.chamfer_ref(a, b)
        el, er = chamfer_emulation(b, a), chamfer_emulation(a, b)
        kc.assert_elementwise(el, dl, tl, "chamfer dl"); kc.assert_elementwise(er, dr, tr, "chamfer dr")
        if na == nb and na > 1:
            fails(kc.assert_elementwise, er, dl, tl, "dl and dr exchanged")
    x, y = torch.randn(2, 70, 3, generator=g) * 0.5, torch.randn(3, 45, 3, generator=g) * 0.5
    ref, tol = kc.chamfer_pairwise_ref(x, y)
    em = torch.stack([torch.stack([chamfer_emulation(y[r:r + 1], x[s:s + 1]).mean() + chamfer_emulation(x[s:s + 1], y[r:r + 1]).mean() for r in range(3)]) for s in range(2)])
    kc.assert_elementwise(em, ref, tol, "chamfer_pairwise")
    fails(kc.assert_elementwise, em.flip(1), ref, tol, "chamfer_pairwise with the reference clouds reversed")
    drop = torch.stack([torch.stack([chamfer_emulation(y[r:r + 1], x[s:s + 1, :64]).mean() + chamfer_emulation(x[s:s + 1], y[r:r + 1]).mean() for r in range(3)]) for s in range(2)])
    fails(kc.assert_elementwise, drop, ref, tol, "chamfer_pairwise that loses the last chunk of one cloud")


def test_maxpool_expression_and_stride_fault():
    g = torch.Generator().manual_seed(12)
    G, n, C, ld = 6, 5, 8, 12
    big = torch.randn(G * n, ld, generator=g)
    view = big[:, :C]
    big[7, 3] = float("nan"); big[10:15, 2] = float("-inf")
    want = kc.maxpool_expr(view, G, n)
    assert bool(torch.isnan(want[1, 3])) and float(want[2, 2]) == float("-inf")
    dense = big.reshape(-1)[:G * n * C].reshape(G * n, C)                      # the planted fault: ld = C on the strided storage
    got = kc.maxpool_expr(dense, G, n)
    same = lambda a, b: bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    assert same(kc.maxpool_expr(view.contiguous(), G, n), want) and not same(got, want)
    fmax = torch.where(torch.isnan(view), torch.full_like(view, float("-inf")), view).reshape(G, n, C).max(1).values      # fmaxf drops NaN
    assert not same(fmax, want)


def test_nan_fixed_kernels_are_under_no_isa_signature():
    """maxpool_kernel and block_act_kernel changed how they select (NaN propagates): neither is one of the hand-counted kernels whose
    disassembly csrc/isa_signatures.json pins, so there is no signature to re-audit."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldt_amd", "csrc", "isa_signatures.json")
    names = " ".join(json.load(open(path))["kernels"])
    assert "maxpool" not in names and "block_act" not in names
