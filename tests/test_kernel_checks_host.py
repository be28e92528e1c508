"""CPU: the reference helpers of the fused projection + attention tests (kernel_checks.py) judged without a GPU.

An emulation of the kernels' contract in torch on the CPU — q | k | v = bf16(fp32 accumulation) in two different summation orders (K in
64-blocks, forward and reversed), float32 softmax, P rounded to bf16, O bf16 — must pass every check that test_gpu_fused_attention_exact.py
applies to the HIP kernels, and the same emulation with one planted fault (one key dropped for one query row; heads h and h + 1 swapped in
k; the S | C slice of one 64-column segment taken from the next segment) must FAIL them: the proof that the derived bound is tight enough to
tell a right kernel from a nearly right one."""
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
