"""Per-element checks and exact probes for the MFMA kernels (used by test_gpu_kernel_exact.py, test_gpu_fused_attention_exact.py and
test_gpu_kernels.py).

A bf16 output's rel-MSE bar has to sit above the output rounding (~1.3e-6), so it passes hundreds of entirely wrong elements in a large
output.  The checks here are componentwise: a bound derived from the operands in float64 (gemm_tol + assert_elementwise), and operands
built so that the result is exact in fp32 accumulation of any order and after bf16 rounding (the probe generators), compared with
torch.equal.  Everything works on whatever device its arguments live on; nothing here needs a GPU to import."""
import torch

U24 = 2.0 ** -24          # fp32 unit round-off
U8 = 2.0 ** -8            # bf16 unit round-off (half an ulp, relative)
# constant of the accumulation term of gemm_tol.  1 is the textbook worst case (K sequential fp32 additions); the measured errors of the
# MFMA kernels sit far below it (blocked summation, random signs): at 1 the worst fp32-output err / tol over every row of
# test_gpu_kernel_exact.py's route table on the MI355X was 0.031 (the K = 64 rows; 0.002 at K = 704), so the constant was halved four times,
# to where that ratio is ~0.5.  The bf16-output ratios sit at 0.98-0.995 for any constant: their bound is the output rounding itself,
# 2^-8 |ref|, which an element near a power of two attains ("What a rel-MSE cannot see").
C_ACC = 1.0 / 16
GELU_SLOPE = 1.13         # max |d gelu / dx| (1.1289 at x = sqrt(2))
GELU_FAST_ABS = 1e-6      # csrc/common.h: gelu_erf_fast is within 8.7e-7 of GELU


def _tile_report(bad, r, c):
    """Where the violations of a 2-D mask sit: one row / one column / the smallest aligned tile that holds them all."""
    rows = torch.nonzero(bad.any(1)).flatten()
    cols = torch.nonzero(bad.any(0)).flatten()
    n = int(bad.sum())
    r0, r1, c0, c1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    where = "rows %d..%d x cols %d..%d" % (r0, r1, c0, c1)
    if r0 == r1:
        return "all in ONE ROW %d (cols %d..%d, %d of %d in that span)" % (r0, c0, c1, n, c1 - c0 + 1)
    if c0 == c1:
        return "all in ONE COLUMN %d (rows %d..%d, %d of %d in that span)" % (c0, r0, r1, n, r1 - r0 + 1)
    for t in (16, 64, 128, 256):
        if r0 // t == r1 // t and c0 // t == c1 // t:
            h = min(bad.shape[0], (r0 // t + 1) * t) - r0 // t * t
            w = min(bad.shape[1], (c0 // t + 1) * t) - c0 // t * t
            return "all inside ONE %d x %d tile (%d, %d): %d of its %d elements; %s" % (t, t, r0 // t, c0 // t, n, h * w, where)
    return "spread over %d rows and %d columns; %s" % (rows.numel(), cols.numel(), where)


def assert_elementwise(out, ref64, tol, what):
    """Fails if any |out - ref64| > tol (tol: a scalar or a tensor like ref64; NaN / inf in `out` violate).  The message names the worst
    element's (row, col) in the 2-D view [-1, last dim], its 256 / 128 / 64 / 16 tile coordinates, how many elements violate and whether they
    fill one tile, one row or one column.  -> max(err / tol) on success."""
    assert tuple(out.shape) == tuple(ref64.shape), "%s: shape %s vs reference %s" % (what, tuple(out.shape), tuple(ref64.shape))
    ref64 = ref64.to(out.device).double()
    tol = tol.to(out.device).double().expand_as(ref64) if torch.is_tensor(tol) else torch.full_like(ref64, float(tol))
    err = (out.double() - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)       # (err > 0 at tol == 0 -> inf: a violation)
    bad = ~(err <= tol)                                                    # NaN compares false: counted
    if bool(bad.any()):
        C = ref64.shape[-1] if ref64.dim() else 1
        b2, r2 = bad.reshape(-1, C), torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).reshape(-1, C)
        i = int(torch.where(b2, r2, torch.full_like(r2, -1.0)).argmax())
        r, c = i // C, i % C
        tiles = ", ".join("%d: (%d, %d) + (%d, %d)" % (t, r // t, c // t, r % t, c % t) for t in (256, 128, 64, 16))
        raise AssertionError(
            "%s: %d of %d elements outside the bound.  Worst at (row %d, col %d): got %r, want %r, |err| %.4g = %.3g x tol %.4g.  "
            "Tile (index) + (offset) at %s.  Violations: %s"
            % (what, int(bad.sum()), bad.numel(), r, c, float(out.reshape(-1, C)[r, c]), float(ref64.reshape(-1, C)[r, c]),
               float(err.reshape(-1, C)[r, c]), float(r2[r, c]), float(tol.reshape(-1, C)[r, c]), tiles, _tile_report(b2, r, c)))
    return float(ratio.max()) if ratio.numel() else 0.0


def gemm_acc_err(x, w, bias, K, c=None):
    """float64 [M, N]: c * K * 2^-24 * (|x| @ |w|^T + |bias|), the componentwise bound on fp32 accumulation in any order."""
    a = x.double().abs() @ w.double().abs().T
    if bias is not None:
        a = a + bias.double().abs()
    return a * ((C_ACC if c is None else c) * K * U24)


def gemm_tol(x, w, bias, K, out_dtype, gelu=False, ref=None, c=None):
    """Componentwise tolerance of out = epi(x @ w^T + bias) against its float64 reference, from the operands (float64 throughout):
    the accumulation bound gemm_acc_err, scaled by GELU's largest slope plus the fast form's stated distance from GELU when `gelu`,
    plus the bf16 rounding 2^-8 |ref| for a bf16 output.  ref: the float64 reference AFTER the epilogue (computed here when None)."""
    acc = gemm_acc_err(x, w, bias, K, c)
    if ref is None:
        ref = x.double() @ w.double().T
        if bias is not None:
            ref = ref + bias.double()
        if gelu:
            ref = torch.nn.functional.gelu(ref)
    if gelu:
        acc = acc * GELU_SLOPE + GELU_FAST_ABS
    if out_dtype == torch.bfloat16:
        return acc * (1 + U8) + U8 * ref.double().abs()
    return acc + U24 * ref.double().abs()                                  # (the final fp32 rounding of the stored value)


def bf16_ulp(ref64):
    """One bf16 ulp at |ref64| (2^-7 relative to the binade's lower edge), float64."""
    a = ref64.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ------------------------------------------------------------------------------------------------------------- probes
def selection_probe(M, N, K):
    """x [M, K] one-hot rows (column (7 m + 3) % K, value +1 / -1 by row parity), w [N, K] asymmetric bf16-exact integers: x @ w^T is a signed
    gather of w, exact in bf16 and fp32.  -> (x, w, ref) float32 on the CPU."""
    m = torch.arange(M)
    km = (m * 7 + 3) % K
    sign = (1 - 2 * (m % 2)).float()
    x = torch.zeros(M, K)
    x[m, km] = sign
    n = torch.arange(N)
    w = (((n[:, None] * 131 + torch.arange(K)[None, :] * 17) % 251) - 125).float()
    assert torch.equal(w.bfloat16().float(), w)
    ref = (w[:, km].T * sign[:, None]).contiguous()
    return x, w, ref


def integer_probe(M, N, K, seed, max_abs=256, with_bias=True, density=0.125, device="cpu"):
    """x [M, K], w [N, K] in {-2..2}, about `density` dense, bias integer in {-3..3}: every partial sum of x @ w^T + bias is an integer below
    2^24 and every result an integer of magnitude <= max_abs <= 256 — exact in fp32 accumulation of any order and after bf16 rounding.  Both
    properties are CHECKED on the float64 result and the density lowered until they hold.  The draw is on the CPU (seeded torch.Generator);
    the float64 check runs on `device`.  -> (x, w, bias, ref float64 on `device`), x / w / bias float32 on the CPU."""
    assert max_abs <= 256
    g = torch.Generator().manual_seed(seed)
    for _ in range(8):
        def draw(r, c):
            v = torch.randint(1, 3, (r, c), generator=g).float() * (1 - 2 * torch.randint(0, 2, (r, c), generator=g)).float()
            return v * (torch.rand(r, c, generator=g) < density).float()
        x, w = draw(M, K), draw(N, K)
        bias = torch.randint(-3, 4, (N,), generator=g).float() if with_bias else None
        xd, wd = x.to(device).double(), w.to(device).double()
        ref = xd @ wd.T
        worst_partial = float((xd.abs() @ wd.abs().T).max()) + 3
        if bias is not None:
            ref = ref + bias.to(device).double()
        if worst_partial < 2 ** 24 and float(ref.abs().max()) <= max_abs and bool((ref == ref.round()).all()):
            return x, w, bias, ref
        density *= 0.7
    raise AssertionError("integer_probe: no density gives |result| <= %d at M=%d N=%d K=%d" % (max_abs, M, N, K))


def attention_pi(Nq, Nk, salt=0):
    """Key index each query gathers: even queries walk the first and last key of every 64-key tile (and key Nk - 1), odd ones a stride."""
    edges = sorted({e for t in range(0, Nk, 64) for e in (t, min(t + 63, Nk - 1))})
    i = torch.arange(Nq) + salt
    e = torch.tensor(edges)[(i // 2) % len(edges)]
    return torch.where(i % 2 == 0, e, (i * 37 + 11) % Nk)


def attention_gather_probe(B, H, Nq, Nk, dh, seed, key_salt=False):
    """Q [B, Nq, H dh], K, V [B, Nk, H dh] (bf16-exact float32) such that query i of head (b, h) scores at least 40 above every other key at key
    pi(i): K[j] carries the +1 / -1 code of the bits of j in the first 11 channels of each head, Q[i] = 160 x the code of pi(i) — a one-bit
    difference costs 2 * 160 / sqrt(dh) >= 40 in score, so every other weight is below e^-40 and O[b, h, i] == V[b, pi(i), head h] to the bit
    (V has magnitudes in [2^-6, 4]: the leftovers cannot move a last bit).  key_salt: head (b, h) codes j ^ m(b, h) instead of j on both sides
    (m below the largest power of two <= Nk, different for neighbouring heads): the scores are the same, but k of another head now selects
    key pi(i) ^ m ^ m' — without it K is the same in every head and a kernel that mixes up the heads of k goes unseen.
    -> (q, k, v, want [B, H, Nq, dh])."""
    assert Nk <= 2048 and dh >= 11 and 2 * 160 / dh ** 0.5 >= 40
    g = torch.Generator().manual_seed(seed)
    C = H * dh
    code = lambda j: (1 - 2 * ((j[:, None] >> torch.arange(11)[None, :]) & 1)).float()            # [n, 11] of +1 / -1
    q = torch.zeros(B, Nq, C); k = torch.zeros(B, Nk, C)
    mag = torch.exp2(torch.randint(-6, 2, (B, Nk, C), generator=g).float()) * (1 + torch.randint(0, 128, (B, Nk, C), generator=g).float() / 128)
    v = mag * (1 - 2 * torch.randint(0, 2, (B, Nk, C), generator=g)).float()
    assert torch.equal(v.bfloat16().float(), v) and float(v.abs().min()) >= 2.0 ** -6 and float(v.abs().max()) <= 4.0
    want = torch.empty(B, H, Nq, dh)
    for b in range(B):
        for h in range(H):
            pi = attention_pi(Nq, Nk, salt=13 * (b * H + h))
            m = (5 + 3 * (b * H + h)) % (1 << (Nk.bit_length() - 1)) if key_salt and Nk >= 4 else 0
            k[b, :, h * dh:h * dh + 11] = code(torch.arange(Nk) ^ m)
            q[b, :, h * dh:h * dh + 11] = 160.0 * code(pi ^ m)
            want[b, h] = v[b, pi, h * dh:(h + 1) * dh]
            # the construction's claim, checked: the gap to the runner-up in score
            s = (q[b, :, h * dh:(h + 1) * dh].double() @ k[b, :, h * dh:(h + 1) * dh].double().T) * dh ** -0.5
            top = s.gather(1, pi[:, None])
            s.scatter_(1, pi[:, None], float("-inf"))
            assert Nk == 1 or float((top - s.max(1, keepdim=True).values).min()) >= 40.0
    return q, k, v, want


# ------------------------------------------------------------------------------------------------------------- fused projection + attention
# (test_gpu_fused_attention_exact.py; validated without a GPU, planted faults included, by test_kernel_checks_host.py)
def bf16_round(x64):
    """float64 -> the bf16 value (as float64) a kernel stores: fp32, then round-to-nearest-even to bf16.  (The double rounding can differ from a
    direct one only within 2^-24 |x| of a rounding boundary, which ambiguous_ulp counts as ambiguous anyway.)"""
    return x64.float().bfloat16().double()


def ambiguous_ulp(pre, acc):
    """float64 like pre: how far bf16(an fp32 accumulation within acc + 2^-24 |pre| =: b of pre) can lie from bf16_round(pre).  0 where `pre` is
    further than b from every bf16 rounding boundary (the midpoint of two neighbouring bf16 values; just above a power of two the lower
    neighbour sits half an ulp away, so that boundary a quarter): both round to the same value.  Elsewhere half an ulp at |pre| + half an ulp
    at |pre| + b + b: one ulp to within 2^-10 in the ordinary case b << ulp, and still a bound where cancellation leaves |pre| below its own
    accumulation error (there the two can differ by many ulps)."""
    a = pre.double().abs()
    b = acc.double() + U24 * a
    ulp = bf16_ulp(a)
    frac = a / ulp - torch.floor(a / ulp)
    dist = torch.minimum((frac - 0.5).abs() * ulp, a - torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -126)))) + ulp / 4)
    return (0.5 * ulp + 0.5 * bf16_ulp(a + b) + b) * (dist <= b).double()


def heads(z, B, n, H, dh):
    """[B * n, H * dh] rows -> float64 [B, H, n, dh]."""
    return z.double().reshape(B, n, H, dh).permute(0, 2, 1, 3)


def attention_ref64(q, k, v, B, H, Nq, Nk, dh):
    """float64 softmax(q k^T / sqrt(dh)) v -> (O [B, H, Nq, dh], max_j |v_j| [B, H, 1, dh])."""
    p = (heads(q, B, Nq, H, dh) @ heads(k, B, Nk, H, dh).transpose(-1, -2) * dh ** -0.5).softmax(-1)
    vv = heads(v, B, Nk, H, dh)
    return (p @ vv).contiguous(), vv.abs().amax(2, keepdim=True)


def attention_base_tol(ref, vmax):
    """The bound of test_attention_bound_vs_float64 on exact bf16 inputs: 2^-8 |ref| (bf16 output) + 2^-8 max_j |v_j| (P rounded to bf16)."""
    return U8 * ref.abs() + U8 * vmax


def exact_projection_probe(M, N, K, seed, with_bias=True, device="cpu"):
    """integer_probe operands with w and the bias scaled by 2^-3: every x w^T + bias is an integer <= 256 times 2^-3, exact in fp32
    accumulation of any order and in bf16 (checked on the float64 result), of ordinary softmax sharpness (standard deviation 0.5 .. 1.3 for
    K = 128 .. 1024).  -> (x, w, bias, y float64 on `device`): the q | k | v a kernel computes internally are `y` to the bit."""
    x, w, bias, ref = integer_probe(M, N, K, seed, with_bias=with_bias, device=device)
    w, y = w / 8, ref / 8
    bias = None if bias is None else bias / 8
    assert torch.equal(w.bfloat16().float(), w) and torch.equal(x.bfloat16().float(), x)
    assert bool((y * 8 == (y * 8).round()).all()) and float(y.abs().max()) <= 32.0 and torch.equal(bf16_round(y), y)
    return x, w, bias, y


def gather_projection_probe(B, H, Nq, Nk, dh, seed, cross=False):
    """attention_gather_probe through the projection: self form X = [Q | K | V] rows (K_gemm = 3 H dh) and W = the 3 H dh identity; cross form
    X = Q, W = the H dh identity and kv = [K | V] rows of the condition.  x w^T reproduces Q, K, V to the bit, so O == want at tolerance 0
    (with no bias or an all-zero one).  -> (x, w, kv or None, want [B, H, Nq, dh]) float32 on the CPU."""
    q, k, v, want = attention_gather_probe(B, H, Nq, Nk, dh, seed, key_salt=True)
    C = H * dh
    if cross:
        return q.reshape(B * Nq, C), torch.eye(C), torch.cat([k, v], -1).reshape(B * Nk, 2 * C), want
    assert Nq == Nk
    return torch.cat([q, k, v], -1).reshape(B * Nq, 3 * C), torch.eye(3 * C), None, want


def consumer_pre64(xs, w, S, C, stats, K, mm=None, mm_abs=None):
    """The LN-folded consumer's algebra in float64 from the fp32 row statistics stats [parts, M, 2] (as test_gpu_kernel_exact._consumer_bound):
    pre = rstd (xs w^T) - rstd mean S + C and its accumulation bound: fp32 accumulation, plus mean, variance (a difference of two fp32 terms)
    and rsqrt in fp32, 2^-19 relative on every term they scale.  mm / mm_abs: xs w^T and |xs| |w|^T when already computed.  -> (pre, acc)."""
    s = stats.double().sum(0)
    mean = s[:, 0:1] / K
    rstd = 1 / torch.sqrt((s[:, 1:2] / K - mean * mean).clamp_min(0) + 1e-6)
    mm = xs.double() @ w.double().T if mm is None else mm
    mm_abs = xs.double().abs() @ w.double().abs().T if mm_abs is None else mm_abs
    t1, t2, t3 = rstd * mm, rstd * mean * S.double(), C.double()
    return t1 - t2 + t3, rstd * mm_abs * (C_ACC * K * U24) + 2.0 ** -19 * (t1.abs() + t2.abs() + t3.abs())


def fused_attention_tol(pre, acc, B, H, Nq, dh, kv=None, Nk=None, chunk=8):
    """Two-stage float64 reference of `projection -> bf16 -> attention` and its componentwise tolerance, all from the reference.
    pre float64 [B Nq, 3 H dh] = the projection ([B Nq, H dh] = q alone with kv = (k, v) rows [B Nk, H dh] given exactly), acc = its
    accumulation bound.  r = bf16_round(pre); the kernel's q | k | v can differ from r by at most e = ambiguous_ulp(pre, acc).  Per query row
    d_i = max_j (e_q |k|^T + |q| e_k^T + e_q e_k^T)_ij / sqrt(dh) bounds the change of every score, so every softmax weight moves by at most a
    factor e^(+-2 d_i) and
        |O - O_ref| <= e^(2 d_i) (2^-8 |O_ref| + 2^-8 max_j |v_j|) + (e^(2 d_i) - 1) (p |v|)_i + e^(2 d_i) (p e_v)_i.
    -> (O_ref [B, H, Nq, dh], tol, tol / base with base = the first term at d = 0, ambiguous fraction).  Samples are processed `chunk` at a time."""
    C = H * dh
    r, e = bf16_round(pre), ambiguous_ulp(pre, acc)
    if kv is None:
        Nk = Nq
        parts = [(r[:, i * C:(i + 1) * C], e[:, i * C:(i + 1) * C]) for i in range(3)]
    else:
        parts = [(r, e)] + [(t.double(), torch.zeros_like(t, dtype=torch.float64)) for t in kv]
    refs, tols, ratios = [], [], []
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        (q, eq), (k, ek), (v, ev) = [(heads(t[b0 * n:(b0 + nb) * n], nb, n, H, dh), heads(u[b0 * n:(b0 + nb) * n], nb, n, H, dh))
                                     for (t, u), n in zip(parts, (Nq, Nk, Nk))]
        kt, ekt = k.transpose(-1, -2), ek.transpose(-1, -2)
        d = ((eq @ kt.abs() + q.abs() @ ekt + eq @ ekt) * dh ** -0.5).amax(-1, keepdim=True)
        p = (q @ kt * dh ** -0.5).softmax(-1)
        ref = p @ v
        base = attention_base_tol(ref, v.abs().amax(2, keepdim=True))
        g = torch.exp(2 * d)
        tol = g * base + (g - 1) * (p @ v.abs()) + g * (p @ ev)
        refs.append(ref); tols.append(tol); ratios.append(tol / base)
    return torch.cat(refs).contiguous(), torch.cat(tols).contiguous(), torch.cat(ratios), float((e > 0).double().mean())


RATIO_MEDIAN_CAP, RATIO_MAX_CAP = 3.0, 8.0


def assert_ratio_caps(ratio, what):
    """The condition that keeps fused_attention_tol honest: the allowance for rounding flips may widen the plain attention bound by a median
    factor of at most 3 and nowhere by more than 8; a case beyond that needs smaller inputs, not a wider cap.  -> (median, max)."""
    med, mx = float(ratio.median()), float(ratio.max())
    assert med <= RATIO_MEDIAN_CAP and mx <= RATIO_MAX_CAP, "%s: tol / base median %.2f (cap %g), max %.2f (cap %g)" % (what, med, RATIO_MEDIAN_CAP, mx, RATIO_MAX_CAP)
    return med, mx
