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


# ------------------------------------------------------------------------------------------------------------- grouped rows + the fused grouper
# (test_gpu_grouper_exact.py; validated without a GPU, planted faults included, by test_kernel_checks_host.py)
#
# A worst-case componentwise bound is useless through the grouper's three bf16 stages: 2^-8 per stage through |W1|, |W2|, |W3| is ~3 |ref|.
# What the kernels owe instead is an INTERVAL: a float64 reference that rounds where the kernel rounds (U, h1, r, out), an allowance for what
# fp32 arithmetic can move before each rounding, and — because rounding is monotone — lo = bf16(pre - a) <= out <= bf16(pre + a) = hi.  Where
# lo == hi (most elements) the output is pinned to the bit; elsewhere exactly the neighbouring values are allowed.
FX_HALF_STEP = 2.0 ** -21          # csrc/common.h: every wave's fp64 partial enters the per-cloud sums rounded to 2^-20 fixed point
EPS_STD = float(torch.tensor(1e-5, dtype=torch.float32))       # the 1e-5f the kernels add to the standard deviation


def _take(t, idx):
    """t [B, n, C], idx [B, ...] -> [B, ..., C]."""
    B = t.shape[0]
    return torch.gather(t, 1, idx.reshape(B, -1, 1).expand(-1, -1, t.shape[-1])).reshape(*idx.shape, t.shape[-1])


def grouper_case(B, n, S, k, seed, D=128, fscale=0.7, degenerate=None, plant=True):
    """Crafted inputs of the grouping kernels (no FPS / kNN): features N(0, fscale^2) x (1 + b / 2) (every cloud its own scale), xyz N(0, 0.4^2),
    seeded random indices with planted cases: point 0 and point n - 1 as neighbours and as anchors, a repeated neighbour in group S // 2, the
    anchor inside its own neighbour set in the even groups only.  degenerate = b: every neighbour of cloud b is its group's anchor (d == 0).
    -> dict of CPU tensors (fi, ki int32)."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, n, D, generator=g) * fscale * (1 + torch.arange(B).float()[:, None, None] * 0.5)
    xyz = torch.randn(B, n, 3, generator=g) * 0.4
    fi = torch.randint(0, n, (B, S), generator=g)
    ki = torch.randint(0, n, (B, S, k), generator=g)
    if plant:
        ki = torch.where(ki == fi[:, :, None], (ki + 1) % n, ki)                  # no anchor in its own set ...
        ki[:, ::2, k // 2] = fi[:, ::2]                                           # ... except in the even groups
        fi[0, S - 1] = n - 1; fi[B - 1, 0] = 0
        ki[0, 0, 0] = 0; ki[0, 0, k - 1] = n - 1; ki[B - 1, S - 1, k - 1] = 0; ki[B - 1, S - 1, 0] = n - 1
        ki[:, S // 2, 1] = ki[:, S // 2, 0]
        if k > 4:
            ki[:, S // 2, k - 1] = ki[:, S // 2, 0]
    if degenerate is not None:
        ki[degenerate] = fi[degenerate][:, None]
    alpha = torch.rand(D + 3, generator=g) + 0.5
    beta = torch.randn(D + 3, generator=g) * 0.2
    return dict(feat=feat, xyz=xyz, fi=fi.int(), ki=ki.int(), alpha=alpha, beta=beta, B=B, n=n, S=S, k=k, D=D)


def grouper_weights(seed, D=128):
    """PreExtraction panels of ordinary scale: bf16-exact N(0, 1 / K) weights, N(0, 0.2^2) biases.  -> (w1 [D, 2D+3], b1, w2, b2, w3, b3)."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.bfloat16().float()
    w1 = bf(torch.randn(D, 2 * D + 3, generator=g) / (2 * D + 3) ** 0.5)
    w2, w3 = bf(torch.randn(D, D, generator=g) / D ** 0.5), bf(torch.randn(D, D, generator=g) / D ** 0.5)
    b1, b2, b3 = [torch.randn(D, generator=g) * 0.2 for _ in range(3)]
    return w1, b1, w2, b2, w3, b3


def group_reference(feat, xyz, fi, ki, alpha, beta, mode="anchor", stats_rel=None):
    """float64 reference of ldt_group_normalize from the fp32 operands, with what the kernels' arithmetic may move (all from the reference):
      d      = g - origin (origin: the anchor's [feature | xyz], or in 'center' mode the mean of the group's k rows);
      s1, s2 = per-cloud sums of d and d^2, tol1 / tol2 their tolerance.  Vector statistics kernels ('anchor', D = 64 / 128): a lane forms fp32
               partial sums over its ceil(k / rows in flight) rows x 5 terms =: m, everything after is fp64: m 2^-24 (sum |d|, sum d^2).  Scalar
               kernel (any other D, and 'center'): only d itself is rounded to fp32, 2^-24 per element (twice that on its square); in 'center'
               mode d also carries the fp32 mean of k terms, k 2^-24 mean_j |g_j|.  Every wave's partial enters as 2^-20 fixed point: half a
               step per wave on top (the kernels' own format, stated in csrc/common.h);
      inv    = 1 / (sqrt(var) + 1e-5f), rho = its relative allowance: the statistics tolerance carried through var and sqrt, plus the fp32 cast,
               add and divide;
      pre    = alpha (d inv) + beta and a = its allowance: the subtraction, two multiplies and the statistics on the first term, the final add
               on the sum (an FMA contraction only removes roundings).
    stats_rel: the caller has ASSERTED the kernel's sums of this very case to lie within stats_rel (sum |d|, sum d^2) of s1, s2 (2^-24 in part
    (c) of the grouper tests: half a rounding on inv, so that a stays at the 8 x 2^-24 (|alpha d inv| + |beta|) the staged reference was
    designed with); tol1 / tol2 and rho are then that instead of the worst case of the summation.
    -> dict(pre, a [B, S, k, D + 3], anchor [B, S, D], s1, s2, tol1, tol2, inv, rho [B])."""
    B, n, D = feat.shape
    S, k = ki.shape[1], ki.shape[2]
    f, x, fi, ki = feat.double(), xyz.double(), fi.long(), ki.long()
    G = torch.cat([_take(f, ki), _take(x, ki)], -1)
    anchor = _take(f, fi)
    if mode == "anchor":
        d = G - torch.cat([anchor, _take(x, fi)], -1)[:, :, None]
        dd = U24 * d.abs()
    else:
        d = G - G.mean(2, keepdim=True)
        dd = U24 * d.abs() + (k * U24) * G.abs().mean(2, keepdim=True)
    red = lambda t: t.sum((1, 2, 3))
    s1, s2, cnt = red(d), red(d * d), float(S * k * (D + 3))
    if mode == "anchor" and D in (64, 128):
        m = -(-k // (64 // (D // 4))) * 5
        tol1, tol2 = m * U24 * red(d.abs()), m * U24 * red(d * d)
        waves = min((S + 3) // 4, 64) * 4
    else:
        tol1, tol2 = red(dd), red(2 * d.abs() * dd + dd * dd)
        waves = min((S * k + 3) // 4, 256) * 4
    if stats_rel is not None:
        tol1, tol2 = stats_rel * red(d.abs()), stats_rel * red(d * d)
    tol1 = tol1 + 2.0 ** -40 * red(d.abs()) + waves * FX_HALF_STEP
    tol2 = tol2 + 2.0 ** -40 * red(d * d) + waves * FX_HALF_STEP
    var = ((s2 - s1 * s1 / cnt) / (cnt - 1)).clamp_min(0)
    dvar = (tol2 + (2 * s1.abs() * tol1 + tol1 * tol1) / cnt) / (cnt - 1)
    std = var.sqrt()
    dstd = torch.maximum((var + dvar).sqrt() - std, std - (var - dvar).clamp_min(0).sqrt())
    inv = 1 / (std + EPS_STD)
    rho = dstd * inv + 3 * U24
    iv, rh = inv[:, None, None, None], rho[:, None, None, None]
    al, be = alpha.double(), beta.double()
    t1 = al * (d * iv)
    pre = t1 + be
    a_t1 = al.abs() * iv * dd + t1.abs() * (rh + 2 * U24)
    a = (a_t1 + U24 * (pre.abs() + a_t1)) * (1 + 2.0 ** -10)
    return dict(pre=pre, a=a, anchor=anchor, s1=s1, s2=s2, tol1=tol1, tol2=tol2, inv=inv, rho=rho)


def _grouper_coords(row, col, k, S, slot=None):
    """Where an element of a grouped tensor sits in the fused grouper: cloud / group, neighbour slot -> 32-row tile, tile row, and the layer-3
    accumulator (half, register) that holds it; channel -> 32-channel block and lane."""
    if slot is None:                                                       # a per-neighbour row index
        g, j = row // k, row % k
    else:
        g, j = row, slot
    gpt = 1 if k >= 32 else 32 // k
    tj = j % 32 if gpt == 1 else (g % S % gpt) * k + j
    return "cloud %d group %d neighbour slot %d (tile %d row %d: half %d register %d), channel block %d lane %d" % (
        g // S, g % S, j, j // 32 if gpt == 1 else (g % S) // gpt, tj, (tj >> 2) & 1, 4 * (tj >> 3) + (tj & 3), col // 32, col % 32)


def _tile_report_groups(bad, k, S, per_neighbour):
    """The (group, neighbour slot, 32-channel block) view of a violation mask [rows, C]: rows are neighbour rows (group k + slot) or groups."""
    rows = torch.nonzero(bad.any(1)).flatten()
    grp = torch.unique(rows // k if per_neighbour else rows)
    blocks = torch.unique(torch.nonzero(bad.any(0)).flatten() // 32).tolist()
    s = "%d group(s) %s of %d cloud(s), 32-channel blocks %s" % (grp.numel(), grp[:8].tolist(), torch.unique(grp // S).numel(), blocks)
    if per_neighbour:
        s += ", neighbour slots %s" % torch.unique(rows % k)[:16].tolist()
    return s


def assert_interval(out, lo, hi, what, k=None, S=None, slot=None):
    """Fails unless lo <= out <= hi everywhere (NaN violates).  out / lo / hi [rows, C].  With k and S the message also gives the element's
    coordinates in the fused grouper (rows = neighbour rows, or groups when `slot` = the reference's arg-max neighbour per element is given)."""
    assert tuple(out.shape) == tuple(lo.shape) == tuple(hi.shape), "%s: shape %s vs reference %s" % (what, tuple(out.shape), tuple(lo.shape))
    o = out.double()
    lo, hi = lo.to(o.device), hi.to(o.device)
    bad = ~((o >= lo) & (o <= hi))
    if bool(bad.any()):
        C = o.shape[1]
        far = torch.where(bad, torch.nan_to_num(torch.maximum(lo - o, o - hi), nan=float("inf")), torch.full_like(o, -1.0))
        i = int(far.argmax())
        r, c = i // C, i % C
        msg = "%s: %d of %d elements outside their interval.  Worst at (row %d, col %d): got %r, want [%r, %r].  Violations: %s" % (
            what, int(bad.sum()), bad.numel(), r, c, float(o[r, c]), float(lo[r, c]), float(hi[r, c]), _tile_report(bad, r, c))
        if k is not None:
            msg += "; %s; worst: %s" % (_tile_report_groups(bad, k, S, slot is None), _grouper_coords(r, c, k, S, None if slot is None else int(slot[r, c])))
        raise AssertionError(msg)


PINNED_MIN_ROWS = 0.98


def check_group_rows(U, stats, ref, D, what):
    """ldt_group_normalize's U [B S k, ldu] bf16 and fp64 sums [2B] against group_reference: the sums within tol1 / tol2; the normalised columns
    inside [bf16(pre - a), bf16(pre + a)], at least 98 % of them pinned (a condition on the reference: a case below it needs tamer inputs);
    the anchor columns == bf16(feat[anchor]) and the padding == 0, bit for bit.  -> dict(pinned, stat = worst err / tol of the sums)."""
    B, S, k = ref["pre"].shape[:3]
    st = stats.double().reshape(B, 2).to(ref["s1"].device)
    e1, e2 = (st[:, 0] - ref["s1"]).abs(), (st[:, 1] - ref["s2"]).abs()
    assert bool((e1 <= ref["tol1"]).all()) and bool((e2 <= ref["tol2"]).all()), "%s: sums %s vs %s / %s: err %s / %s, tol %s / %s" % (
        what, st.tolist(), ref["s1"].tolist(), ref["s2"].tolist(), e1.tolist(), e2.tolist(), ref["tol1"].tolist(), ref["tol2"].tolist())
    lo, hi = bf16_round(ref["pre"] - ref["a"]).reshape(-1, D + 3), bf16_round(ref["pre"] + ref["a"]).reshape(-1, D + 3)
    pinned = float((lo == hi).double().mean())
    assert pinned >= PINNED_MIN_ROWS, "%s: only %.4f of the normalised elements are pinned by the reference (needs %.2f)" % (what, pinned, PINNED_MIN_ROWS)
    assert_interval(U[:, :D + 3], lo, hi, what + ": normalised columns", k=k, S=S)
    want = ref["anchor"].float().bfloat16()[:, :, None, :].expand(-1, -1, k, -1).reshape(-1, D).to(U.device)
    assert torch.equal(U[:, D + 3:2 * D + 3], want), what + ": anchor columns differ from bf16(feat[anchor])"
    assert bool((U[:, 2 * D + 3:].float() == 0).all()), what + ": K padding not zero"
    return dict(pinned=pinned, stat=float(torch.maximum(e1 / ref["tol1"], e2 / ref["tol2"]).max()))


PINNED_MIN, WIDE_MAX = 0.6, 0.15


def grouper_staged_reference(g, w1, b1, w2, b2, w3, b3):
    """Staged float64 reference of grouping + PreExtraction + neighbour max from g = group_reference(..., 'anchor'): bf16 where the kernels round
    (U, h1, r, out), every stage carrying the allowance e for elements whose rounding an fp32 accumulation can flip (ambiguous_ulp; zero where
    the pre-activation is below -acc: ReLU gives exactly 0 on both sides), propagated through |W| of the next layer together with that layer's
    fp32 accumulation bound C_ACC K 2^-24 (|x| |W|^T + |b|) (K = 259, 128, and 160 for layer 3 with its residual k-steps).  The result keeps
    the allowance PER NEIGHBOUR: lo = bf16(relu(max_j (p3 - a3))), hi = bf16(relu(max_j (p3 + a3))).
    -> dict(lo, hi, ref [B S, 128], slot = arg-max neighbour of the point reference, pinned = share with lo == hi, wide = share whose interval
    exceeds 2 bf16 ulps)."""
    c = C_ACC
    B, S, k = g["pre"].shape[:3]
    dv = g["pre"].device
    W1, W2, W3 = w1.double().to(dv), w2.double().to(dv), w3.double().to(dv)
    B1, B2, B3 = b1.double().to(dv), b2.double().to(dv), b3.double().to(dv)
    los, his, refs, slots = [], [], [], []
    for b in range(B):                                                      # one cloud at a time: the per-neighbour float64 tensors are large
        anc = g["anchor"][b][:, None, :].expand(-1, k, -1)
        pu = torch.cat([g["pre"][b], anc], -1)
        au = torch.cat([g["a"][b], torch.zeros_like(anc)], -1)
        ru, eu = bf16_round(pu), ambiguous_ulp(pu, au)
        p1 = ru @ W1.T + B1
        a1 = eu @ W1.abs().T + c * W1.shape[1] * U24 * (ru.abs() @ W1.abs().T + B1.abs())
        p1r = torch.relu(p1)
        r1, e1 = bf16_round(p1r), ambiguous_ulp(p1r, a1) * (p1 > -a1)
        p2 = r1 @ W2.T + B2
        a2 = e1 @ W2.abs().T + c * W2.shape[1] * U24 * (r1.abs() @ W2.abs().T + B2.abs())
        p2r = torch.relu(p2)
        r2, e2 = bf16_round(p2r), ambiguous_ulp(p2r, a2) * (p2 > -a2)
        p3 = r2 @ W3.T + B3 + r1
        a3 = e2 @ W3.abs().T + e1 + c * (W3.shape[1] + 32) * U24 * (r2.abs() @ W3.abs().T + B3.abs() + r1)
        a3 = a3 + U24 * p3.abs()
        los.append(bf16_round(torch.relu((p3 - a3).amax(1))))
        his.append(bf16_round(torch.relu((p3 + a3).amax(1))))
        m, j = p3.max(1)
        refs.append(bf16_round(torch.relu(m))); slots.append(j)
    lo, hi, ref, slot = torch.cat(los), torch.cat(his), torch.cat(refs), torch.cat(slots)
    wide = (hi - lo) > 2 * bf16_ulp(hi.clamp_min(2.0 ** -126))
    return dict(lo=lo, hi=hi, ref=ref, slot=slot, pinned=float((lo == hi).double().mean()), wide=float(wide.double().mean()), k=k, S=S)


def check_grouper(out, sr, what):
    """The fused grouper's (or the five-kernel chain's) fp32 [B S, 128] against grouper_staged_reference: the two conditions on the reference
    (pinned share >= 0.6, wide-interval share <= 0.15: a case outside needs tamer inputs, not wider caps), then the interval per element.
    -> share of elements that differ from the point reference at all."""
    assert sr["pinned"] >= PINNED_MIN and sr["wide"] <= WIDE_MAX, "%s: pinned share %.3f (needs %.2f), wide-interval share %.3f (cap %.2f)" % (
        what, sr["pinned"], PINNED_MIN, sr["wide"], WIDE_MAX)
    assert_interval(out, sr["lo"], sr["hi"], what, k=sr["k"], S=sr["S"], slot=sr["slot"])
    return float((out.double() != sr["ref"].to(out.device)).double().mean())


# probe (a): one signed unit per W1 row, everything after layer 1 switched off: out[g][c] = max_j relu(+-U[j][sel(c)])
def grouper_selection_probe(variant, D=128):
    """-> (w1 [D, 2D+3] with row c = sgn(c) at column sel(c) = (c + D variant) mod (2D + 3): three variants walk all 259 inputs, every layer-1
    k-step — the three xyz slots of step 16 and the anchor steps included —, sel [D], sgn [D], alpha [D + 3] = +-2^p)."""
    c = torch.arange(D)
    sel = (c + D * variant) % (2 * D + 3)
    sgn = (1 - 2 * ((c + variant) % 2)).float()
    w1 = torch.zeros(D, 2 * D + 3)
    w1[c, sel] = sgn
    i = torch.arange(D + 3)
    alpha = torch.exp2(((i % 3) - 1).float()) * torch.where(i % 5 == 0, -1.0, 1.0)
    return w1, sel, sgn, alpha


def plant_winners(case, sel, sgn, alpha):
    """A copy of `case` (distinct points for every (group, slot) and every anchor: needs S (k + 1) <= n) in which neighbour slot (c + s) mod k of
    group s decides output channel c of probe (a): its value in input column sel(c) is moved 40 cloud scales from the anchor's, towards the
    sign that survives alpha, W1's sign and the ReLU.  Every slot 0..k-1 — each in-lane max position, both halves, every tile — then decides
    some output of every group (asserted by the caller on the reference's arg-max)."""
    B, n, S, k, D = case["B"], case["n"], case["S"], case["k"], case["D"]
    assert S * (k + 1) <= n
    g = torch.Generator().manual_seed(1000 + S * k)
    out = dict(case)
    feat, xyz = case["feat"].clone(), case["xyz"].clone()
    fi, ki = torch.empty(B, S, dtype=torch.long), torch.empty(B, S, k, dtype=torch.long)
    for b in range(B):
        perm = torch.randperm(n, generator=g)
        perm = torch.cat([torch.tensor([0, n - 1]), perm[(perm != 0) & (perm != n - 1)]])        # point 0 anchors group 0, point n - 1 is its slot 0
        fi[b] = perm[torch.arange(S) * (k + 1)]
        ki[b] = perm[(torch.arange(S)[:, None] * (k + 1) + 1 + torch.arange(k)[None, :])]
        for c in range(D):
            col = int(sel[c])
            if col >= D + 3:
                continue                                                                          # an anchor column: the same on every slot
            s = torch.arange(S)
            p, a = ki[b, s, (c + s) % k], fi[b]
            push = 40.0 * (1 + b / 2) * float(torch.sign(sgn[c] * alpha[col]))
            if col < D:
                feat[b, p, col] = feat[b, a, col] + push
            else:
                xyz[b, p, col - D] = xyz[b, a, col - D] + push
    out.update(feat=feat, xyz=xyz, fi=fi.int(), ki=ki.int())
    return out


def grouper_selection_expected(U, B, S, k, sel, sgn):
    """out of probe (a) from the grouped rows U [B S k, >= 259] (ops.group_normalize on the same inputs): float64 [B S, 128] and the arg-max slot."""
    u = U[:, :sel.numel() * 2 + 3].double().reshape(B * S, k, -1)[:, :, sel.to(U.device)] * sgn.double().to(U.device)
    m, j = torch.relu(u).max(1)
    return m, j


# probe (b): integers all the way
def grouper_integer_probe(B, n, seed, D=128, device="cpu"):
    """alpha = 0, beta / features / weights / biases small integers (integer_probe's {-2..2}, sparse — W2 and W3 {-1, 0, 1} and denser; biases {-3..3}): U = [beta | feat[anchor]],
    and h1, r, out are integers of magnitude <= 256 with every partial sum an integer far below 2^24 — exact in fp32 accumulation of any order
    and after each bf16 rounding, through all three layers and the residual.  CHECKED on the float64 result over every point as a possible
    anchor; densities lowered until it holds.  -> (feat [B, n, D], beta, (w1, b1, w2, b2, w3, b3), o float64 [B, n, D] on `device`: the output
    of a group is o[b, anchor])."""
    g = torch.Generator().manual_seed(seed)
    density = 0.1                      # W2 (+-1) at 1.5 x, W3 (+-1) at 1 x: two k-slots of a 32-row fragment then differ in some row in all but ~1e-3 of the pairs
    for _ in range(10):
        def draw(r, c, dens, top=3):
            v = torch.randint(1, top, (r, c), generator=g).float() * (1 - 2 * torch.randint(0, 2, (r, c), generator=g)).float()
            return v * (torch.rand(r, c, generator=g) < dens).float()
        feat = draw(B * n, D, 0.3).reshape(B, n, D)
        beta = draw(1, D + 3, 0.5).reshape(-1)
        w1, w2, w3 = draw(D, 2 * D + 3, 0.06), draw(D, D, 1.5 * density, 2), draw(D, D, density, 2)
        b1, b2, b3 = [torch.randint(-3, 4, (D,), generator=g).float() for _ in range(3)]
        W1, W2, W3 = w1.to(device).double(), w2.to(device).double(), w3.to(device).double()
        u = torch.cat([beta.to(device).double().expand(B * n, -1), feat.to(device).double().reshape(B * n, D)], -1)
        h1 = torch.relu(u @ W1.T + b1.to(device).double())
        r = torch.relu(h1 @ W2.T + b2.to(device).double())
        o = torch.relu(r @ W3.T + b3.to(device).double() + h1)
        partial = max(float((u.abs() @ W1.abs().T).max()), float((h1 @ W2.abs().T).max()), float((r @ W3.abs().T + h1).max())) + 3
        ok = all(float(t.max()) <= 256 and bool((t == t.round()).all()) and torch.equal(bf16_round(t), t) for t in (h1, r, o))
        if ok and partial < 2 ** 24 and float((o > 0).double().mean()) > 0.2 and float((r > 0).double().mean()) > 0.2:
            return feat, beta, (w1, b1, w2, b2, w3, b3), o.reshape(B, n, D)
        density *= 0.9
    raise AssertionError("grouper_integer_probe: no density keeps h1, r and out within 256")


def guarded(rows, cols, fill, device, guard=4096):
    """-> (big, view): a contiguous fp32 [rows, cols] view (16-byte aligned) in the middle of a buffer whose `guard` elements on either side hold a
    sentinel, the view itself `fill`."""
    big = torch.full((rows * cols + 2 * guard,), SENT_F32, dtype=torch.float32, device=device)
    view = big[guard:guard + rows * cols].view(rows, cols)
    view.fill_(fill)
    return big, view


SENT_F32 = -1.7014118e38                         # a bit pattern no kernel under test produces


def assert_guard_intact(big, numel, what, guard=4096):
    lo, hi = big[:guard], big[guard + numel:]
    bad = int((lo != SENT_F32).sum()) + int((hi != SENT_F32).sum())
    if bad:
        where = torch.nonzero(torch.cat([lo, hi]) != SENT_F32).flatten()
        raise AssertionError("%s: %d element(s) written outside `out` (first at offset %d of the surround: %s the view)" % (
            what, bad, int(where[0]), "before" if int(where[0]) < guard else "%d after the end of" % (int(where[0]) - guard)))


# ------------------------------------------------------------------------------------------------------------- fused LN + MLP / LN + linear
# (csrc/fused_mlp.hip; test_gpu_fused_mlp_exact.py; validated without a GPU, planted faults included, by test_kernel_checks_host.py)
#
# The worst-case bound of test_ln_linear_and_ln_mlp_guard_bands_and_bounds carries 2^-8 per bf16 stage through |W_up|, GELU and |W_dn|: it is
# several times the update itself.  As for the grouper, the reference here rounds where the kernel rounds (h, u) and allows, per element, only
# what fp32 arithmetic can do to that rounding: nothing, except within the accumulation error of a rounding boundary, where it is one ulp.
LN_ALLOW = 4 * 2.0 ** -20          # fp32 LayerNorm of a normalised value (test_layernorm_modulate_and_cast_pad_guard_bands)
MLP_TOL_CAP = 0.02                 # condition on the reference: median(tol) <= this x median(|gate * update|)
LNLIN_PINNED_MIN, LNLIN_WIDE_MAX = 0.8, 0.05


def sample_rows(t, n, rows_per_sample, row0=0):
    """Per-sample rows t [nS, C] -> float64 [n, C]: row r of the result is t[(row0 + r) // rows_per_sample]."""
    return t.double()[(torch.arange(n, device=t.device) + row0) // rows_per_sample]


def ln_stage(x, ln_w=None, ln_b=None, shift=None, scale=None, rows_per_sample=0, row0=0):
    """Stage h of both kernels in float64: LN(x) (eps 1e-6, biased variance), then * w + b and / or * (1 + scale) + shift (in this order, as
    the kernel; shift / scale [nS, C] per-sample rows taken by (row0 + row) // rows_per_sample).  Allowance a = 4 2^-20 (1 + |h^|) times
    (1 + |w|) and / or (1 + |scale|): what fp32 mean / variance / rsqrt leave on h^, carried through the factors that follow.
    -> (pre, a, r = bf16_round(pre), e = ambiguous_ulp(pre, a))."""
    xd = x.double()
    hhat = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6)
    pre, f = hhat, torch.ones_like(hhat)
    if ln_w is not None:
        w = ln_w.double().to(xd.device)
        pre, f = pre * w + ln_b.double().to(xd.device), f * (1 + w.abs())
    if shift is not None:
        sc = sample_rows(scale.to(xd.device), xd.shape[0], rows_per_sample, row0)
        pre, f = pre * (1 + sc) + sample_rows(shift.to(xd.device), xd.shape[0], rows_per_sample, row0), f * (1 + sc.abs())
    a = LN_ALLOW * (1 + hhat.abs()) * f
    return pre, a, bf16_round(pre), ambiguous_ulp(pre, a)


def fused_mlp_reference(x, w_up, b_up, w_dn, b_dn, ln_w=None, ln_b=None, shift=None, scale=None, gate=None, rows_per_sample=0, row_chunk=16384):
    """Staged float64 reference of ln_mlp_resid_kernel on x [M, C] (fp32), on x's device, `row_chunk` rows at a time:
      h:   pre_h, a_h, r_h, e_h = ln_stage(...)
      u:   p_u = r_h W_up^T + b_up, a_u = e_h |W_up|^T + C_ACC C 2^-24 (|r_h| |W_up|^T + |b_up|); p_g = gelu(p_u), a_g = GELU_SLOPE a_u +
           GELU_FAST_ABS; r_u = bf16_round(p_g), e_u = ambiguous_ulp(p_g, a_g)
      out: upd = r_u W_dn^T + b_dn, ref = x + g upd (g = the gate's per-sample row, 1 without a gate), and, the output being fp32,
           tol = |g| (e_u |W_dn|^T + C_ACC 4C 2^-24 (|r_u| |W_dn|^T + |b_dn|)) + 2 2^-24 (|x| + |g upd|) + 2^-24 |ref|.
    -> dict(ref, tol [M, C], amb_h, amb_u = the shares of h / u elements whose rounding may flip, ratio = median(tol) / median(|g upd|))."""
    dv, (M, C) = x.device, x.shape
    Wu, Bu, Wd, Bd = w_up.double().to(dv), b_up.double().to(dv), w_dn.double().to(dv), b_dn.double().to(dv)
    refs, tols, gus, nh, nu = [], [], [], 0.0, 0.0
    for r0 in range(0, M, row_chunk):
        xs = x[r0:r0 + row_chunk].double()
        _, _, rh, eh = ln_stage(xs, ln_w, ln_b, shift, scale, rows_per_sample, r0)
        ru_abs = rh.abs() @ Wu.abs().T
        pu = rh @ Wu.T + Bu
        au = eh @ Wu.abs().T + C_ACC * C * U24 * (ru_abs + Bu.abs())
        pg = torch.nn.functional.gelu(pu)
        ag = GELU_SLOPE * au + GELU_FAST_ABS
        ru, eu = bf16_round(pg), ambiguous_ulp(pg, ag)
        upd = ru @ Wd.T + Bd
        g = torch.ones_like(xs) if gate is None else sample_rows(gate.to(dv), xs.shape[0], rows_per_sample, r0)
        ref = xs + g * upd
        tol = g.abs() * (eu @ Wd.abs().T + C_ACC * 4 * C * U24 * (ru.abs() @ Wd.abs().T + Bd.abs())) + 2 * U24 * (xs.abs() + (g * upd).abs()) + U24 * ref.abs()
        refs.append(ref); tols.append(tol); gus.append((g * upd).abs())
        nh += float((eh > 0).double().sum()); nu += float((eu > 0).double().sum())
    ref, tol, gu = torch.cat(refs), torch.cat(tols), torch.cat(gus)
    return dict(ref=ref, tol=tol, amb_h=nh / (M * C), amb_u=nu / (M * 4 * C), ratio=float(tol.median() / gu.median()))


def check_fused_mlp(x_out, sr, what):
    """ln_mlp_resid_'s x against fused_mlp_reference: the condition on the reference first (median(tol) <= 0.02 median(|g upd|): a case beyond
    it needs tamer inputs, never a wider cap), then every element.  -> worst err / tol."""
    assert sr["ratio"] <= MLP_TOL_CAP, "%s: median(tol) / median(|update|) = %.4f (cap %g)" % (what, sr["ratio"], MLP_TOL_CAP)
    return assert_elementwise(x_out, sr["ref"], sr["tol"], what)


def ln_linear_reference(x, w, bias=None, ln_w=None, ln_b=None, shift=None, scale=None, rows_per_sample=0, row_chunk=16384):
    """Interval reference of ln_linear_kernel (and of the projection ln_mlp_resid_kernel chains): pre = r_h W^T + b, a = e_h |W|^T +
    C_ACC C 2^-24 (|r_h| |W|^T + |b|), lo = bf16_round(pre - a), hi = bf16_round(pre + a) (rounding is monotone).
    -> dict(lo, hi, ref = bf16_round(pre) [M, N], pinned = share with lo == hi, wide = share whose interval exceeds 2 bf16 ulps)."""
    dv, (M, C) = x.device, x.shape
    W = w.double().to(dv)
    B = torch.zeros(W.shape[0], dtype=torch.float64, device=dv) if bias is None else bias.double().to(dv)
    los, his, refs = [], [], []
    for r0 in range(0, M, row_chunk):
        _, _, rh, eh = ln_stage(x[r0:r0 + row_chunk], ln_w, ln_b, shift, scale, rows_per_sample, r0)
        pre = rh @ W.T + B
        a = eh @ W.abs().T + C_ACC * C * U24 * (rh.abs() @ W.abs().T + B.abs())
        los.append(bf16_round(pre - a)); his.append(bf16_round(pre + a)); refs.append(bf16_round(pre))
    lo, hi, ref = torch.cat(los), torch.cat(his), torch.cat(refs)
    wide = (hi - lo) > 2 * bf16_ulp(torch.maximum(lo.abs(), hi.abs()))
    return dict(lo=lo, hi=hi, ref=ref, pinned=float((lo == hi).double().mean()), wide=float(wide.double().mean()))


def check_ln_linear(out, sr, what):
    """A bf16 [M, N] output against ln_linear_reference: the two conditions on the reference (pinned share >= 0.8, wide-interval share <= 0.05: a
    case outside needs tamer inputs, not wider caps), then the interval per element.  -> share of elements that differ from the point reference."""
    assert sr["pinned"] >= LNLIN_PINNED_MIN and sr["wide"] <= LNLIN_WIDE_MAX, "%s: pinned share %.3f (needs %.2f), wide-interval share %.3f (cap %.2f)" % (
        what, sr["pinned"], LNLIN_PINNED_MIN, sr["wide"], LNLIN_WIDE_MAX)
    assert_interval(out, sr["lo"], sr["hi"], what)
    return float((out.double() != sr["ref"].to(out.device)).double().mean())


def mlp_randn_case(M, C, seed, n_samples=1, N=0, tame=False):
    """The data of the randn checks: x = 2 randn + 0.3, bf16-exact W ~ randn / sqrt(K), b ~ 0.1 randn, an affine pair (w in [1, 2), b ~ 0.2 randn)
    and per-sample modulation rows shift | scale | gate ~ 0.5 randn as one [n_samples, 3C] tensor; with N a next-block projection wn [N, C], bn
    and its own affine pair.  The allowance of h is 4 2^-20 (1 + |h^|) (1 + |w|) (1 + |scale|) against a value that grows with |w| |1 + scale|
    only, so small |w| and scale near -1 unpin outputs: with w in [0.5, 1.5) an affine C = 128 case sits at 79 .. 83 % pinned, astride the
    condition.  tame (where an affine LayerNorm and a modulation meet, and for fewer than 16 rows, where one sample's modulation row decides the
    whole case): w in [2, 3) and modulation ~ 0.25 randn.  -> dict of CPU tensors (weights float32 holding bf16 values)."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.bfloat16().float()
    lo, ms = (2.0, 0.25) if tame else (1.0, 0.5)
    d = dict(x=torch.randn(M, C, generator=g) * 2 + 0.3,
             w_up=bf(torch.randn(4 * C, C, generator=g) / C ** 0.5), b_up=torch.randn(4 * C, generator=g) * 0.1,
             w_dn=bf(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5), b_dn=torch.randn(C, generator=g) * 0.1,
             ln_w=torch.rand(C, generator=g) + lo, ln_b=torch.randn(C, generator=g) * 0.2,
             mod=torch.randn(n_samples, 3 * C, generator=g) * ms)
    if N:
        d.update(wn=bf(torch.randn(N, C, generator=g) / C ** 0.5), bn=torch.randn(N, generator=g) * 0.1,
                 nln_w=torch.rand(C, generator=g) + lo, nln_b=torch.randn(C, generator=g) * 0.2)
    return d


# exact probes.  Two facts carry them (both asserted on the host, test_kernel_checks_host.py): (1) the LayerNorm can be switched off from the
# outside: with scale = -1 the kernel computes h^ * 0 + shift == shift for any finite x (per sample, or per row with rows_per_sample = 1), and with
# ln_w = 0 h == ln_b in every row; (2) gelu_erf_fast / gelu_erf_fast2 are exactly relu at 0 and at every |v| >= 6.
def probe_gates(n_samples, C, g):
    """Gates from {1, -1, 2, -2, 1/2} per (sample, channel)."""
    return torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[torch.randint(0, 5, (n_samples, C), generator=g)]


def _sparse_ints(g, r, c, density, top=3):
    v = torch.randint(1, top, (r, c), generator=g).float() * (1 - 2 * torch.randint(0, 2, (r, c), generator=g)).float()
    return v * (torch.rand(r, c, generator=g) < density).float()


def mlp_integer_probe(M, C, rows_per_sample, seed, gated, device="cpu"):
    """Integers through the whole MLP.  h = the shift rows = 8 x sparse {-2..2} per sample (scale = -1 switches the LayerNorm off), W_up sparse
    {-2..2}, b_up = 8 x {-3..3}: every hidden pre-activation is a multiple of 8, i.e. 0 or at least 8 in magnitude, where the kernel's GELU is
    exactly relu; u is then a multiple of 8 up to 2048 (bf16-exact).  W_dn sparse {-2..2}, b_dn {-3..3}, x sparse {-2..2}, gates from
    {+-1, +-2, 1/2}: every partial sum is a multiple of 1/2 far below 2^24, exact in fp32 in any order, with or without FMA contraction.  All
    of that is CHECKED on the float64 result, and the densities lowered until it holds.
    -> dict(x, shift, scale, gate (None when not `gated`), w_up, b_up, w_dn, b_dn: float32 CPU tensors; ref: float64 [M, C] on `device`)."""
    g = torch.Generator().manual_seed(seed)
    nS = (M + rows_per_sample - 1) // rows_per_sample
    density = 0.25
    for _ in range(10):
        shift = 8 * _sparse_ints(g, nS, C, 0.4)
        w_up, b_up = _sparse_ints(g, 4 * C, C, density), 8 * torch.randint(-3, 4, (4 * C,), generator=g).float()
        w_dn, b_dn = _sparse_ints(g, C, 4 * C, density), torch.randint(-3, 4, (C,), generator=g).float()
        x = _sparse_ints(g, M, C, 0.5)
        gate = probe_gates(nS, C, g) if gated else None
        dd = lambda t: t.double().to(device)
        h = sample_rows(dd(shift), M, rows_per_sample)
        pu = h @ dd(w_up).T + dd(b_up)
        u = torch.relu(pu)
        upd = u @ dd(w_dn).T + dd(b_dn)
        gg = sample_rows(dd(gate), M, rows_per_sample) if gated else torch.ones_like(upd)
        ref = dd(x) + gg * upd
        partial = float((dd(x).abs() + gg.abs() * (u @ dd(w_dn).abs().T + dd(b_dn).abs())).max())
        partial_u = float((h.abs() @ dd(w_up).abs().T + dd(b_up).abs()).max())
        ok = torch.equal(bf16_round(h), h) and torch.equal(bf16_round(u), u) and bool((pu == 8 * (pu / 8).round()).all()) and float(u.max()) <= 2048
        ok = ok and bool((2 * ref == (2 * ref).round()).all()) and max(partial, partial_u) < 2 ** 22 and torch.equal(ref.float().double(), ref)
        if ok and float((u > 0).double().mean()) > 0.2 and float((upd != 0).double().mean()) > 0.5:
            return dict(x=x, shift=shift, scale=torch.full_like(shift, -1.0), gate=gate, w_up=w_up, b_up=b_up, w_dn=w_dn, b_dn=b_dn, ref=ref)
        density *= 0.8
    raise AssertionError("mlp_integer_probe: no density keeps every stage exact at M=%d C=%d" % (M, C))


def mlp_selection_probe(M, C, rows_per_sample, seed, gated, device="cpu"):
    """A signed gather through the MLP.  h = the shift rows = 8 (1 + (37 c + 101 s) mod 255): multiples of 8 in [8, 2040], distinct over the
    channels of a sample and, for one channel, over any 255 consecutive samples.  W_up is a signed one-hot: hidden unit j reads channel
    sel(j) = (37 j + j // C) mod C with sign -1 when j % 4 == 3 (every channel is read with sign +1 by some unit), b_up = 0: u[j] =
    relu(+-h[sel(j)]).  W_dn sums a few hidden units: unit j enters output j % C with weight 1 + j // C and output (7 j + 1 + j // C) mod C
    with weight -(5 + j % 3), so no unit's column of W_dn is zero and no two units have the same one (checked): a hidden unit read from the wrong k-slot, chunk or row
    changes the result.  x sparse {-2..2}, b_dn {-3..3}, gates from {+-1, +-2, 1/2}; exactness checked as in mlp_integer_probe.
    -> the same dict as mlp_integer_probe."""
    g = torch.Generator().manual_seed(seed)
    nS = (M + rows_per_sample - 1) // rows_per_sample
    c, s, j = torch.arange(C), torch.arange(nS), torch.arange(4 * C)
    shift = 8.0 * (1 + (37 * c[None, :] + 101 * s[:, None]) % 255).float()
    sel, sgn = (37 * j + j // C) % C, torch.where(j % 4 == 3, -1.0, 1.0)
    w_up = torch.zeros(4 * C, C)
    w_up[j, sel] = sgn
    w_dn = torch.zeros(C, 4 * C)
    w_dn[j % C, j] += (1 + j // C).float()
    w_dn[(7 * j + 1 + j // C) % C, j] -= (5 + j % 3).float()
    assert torch.unique(w_dn.T, dim=0).shape[0] == 4 * C and bool((w_dn != 0).any(0).all())
    assert all(bool((sgn[sel == ch] > 0).any()) for ch in range(C))
    b_dn = torch.randint(-3, 4, (C,), generator=g).float()
    x = _sparse_ints(g, M, C, 0.5)
    gate = probe_gates(nS, C, g) if gated else None
    dd = lambda t: t.double().to(device)
    h = sample_rows(dd(shift), M, rows_per_sample)
    u = torch.relu(h @ dd(w_up).T)
    upd = u @ dd(w_dn).T + dd(b_dn)
    gg = sample_rows(dd(gate), M, rows_per_sample) if gated else torch.ones_like(upd)
    ref = dd(x) + gg * upd
    assert torch.equal(bf16_round(h), h) and torch.equal(bf16_round(u), u) and float(h.min()) >= 8 and float(h.max()) <= 2040
    assert float((dd(x).abs() + gg.abs() * (u @ dd(w_dn).abs().T + dd(b_dn).abs())).max()) < 2 ** 22 and torch.equal(ref.float().double(), ref)
    return dict(x=x, shift=shift, scale=torch.full_like(shift, -1.0), gate=gate, w_up=w_up, b_up=torch.zeros(4 * C), w_dn=w_dn, b_dn=b_dn, ref=ref)


# ------------------------------------------------------------------------------------------------------------- stream, encoder and metric helpers
# (csrc/elementwise.hip, samplers.hip, metrics.hip, pointops.hip, actnorm.hip, eval_loss.hip's reparam; test_gpu_stream_kernels_exact.py; validated without a
# GPU, planted faults included, by test_kernel_checks_host.py)
#
# Three kinds of check.  EXACT: kernels that promise the reference's operation order (`fp contract(off)`), copies, casts and selections are
# held to torch.equal with the expression evaluated in fp32 by torch on the CPU.  PHILOX: the normal stream against a numpy Philox4x32-10 +
# Box-Muller (philox_normal_ref).  BOUNDED: everything else against float64, the tolerance derived from the kernel's stated arithmetic: every
# fp32 rounding 2^-24 relative (U24), every libm call LIBM[name] ulps of its result (one ulp <= 2^-23 relative, ULP32).
ULP32 = 2.0 ** -23
# No libm error bound for this device is written in the project, so none was assumed: every constant started at 1 ulp, the worst err / tol of the
# classes that call the function was measured on the MI355X against float64, and the constant is the next power of two at or above that
# ratio (cap 4; the measured ratios: DESIGN.md section 3 and test_gpu_stream_kernels_exact.py::test_zz_margins).  Measured at 1 ulp: expf 0.19-0.997
# (actnorm, reparam, mixture_seed, the score kernels, silu, selu), powf 0.49 (sde_score kind 2), logf + sincosf 0.77 (the Philox stream), sinf /
# cosf 0.61 (sinusoid), erff 0.34 (GELU): every constant stays at 1.
LIBM = {"expf": 1.0, "logf": 1.0, "sincosf": 1.0, "powf": 1.0, "erff": 1.0}
SLACK = 1 + 2.0 ** -10            # second-order terms of the first-order bounds below

PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
PHILOX_TAG = 0x4C445421           # the constant fourth counter word of csrc/samplers.hip


def philox4x32_10_np(ctr, k0, k1, swap_key_increments=False):
    """Philox4x32-10 (Salmon et al. 2011) as csrc/common.h states it: ctr uint32 [n, 4], key (k0, k1) -> uint32 [n, 4].  swap_key_increments:
    the planted fault of the host tests (the two Weyl constants exchanged)."""
    import numpy as np
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    w0, w1 = (PHILOX_W1, PHILOX_W0) if swap_key_increments else (PHILOX_W0, PHILOX_W1)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & mask, n2, p0 & mask]
        k0, k1 = (k0 + w0) & 0xFFFFFFFF, (k1 + w1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def box_muller_ref(a, b, swap_sin_cos=False):
    """csrc/common.h box_muller on uint32 arrays: u1 = ((float)a + 1) 2^-32, u2 = (float)b 2^-32 and the angle 6.2831855f u2 formed in float32
    (those roundings are defined), log / sqrt / sin / cos in float64 on the float32 values.  -> (z0 = r cos, z1 = r sin, relative tolerance):
    logf's error is halved by the square root, which is correctly rounded like the product; sincosf's enters in full."""
    import numpy as np
    u1 = (a.astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -32)
    u2 = b.astype(np.float32) * np.float32(2.0 ** -32)
    ang = (np.float32(6.283185307179586) * u2).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    cs, sn = np.cos(ang), np.sin(ang)
    if swap_sin_cos:
        cs, sn = sn, cs
    rel = ((0.5 * LIBM["logf"] + LIBM["sincosf"]) * ULP32 + 2 * U24) * SLACK
    return r * cs, r * sn, rel


def philox_normal_ref(seed, step, first_vec, n_vec, swap_key_increments=False, step_word=2, swap_sin_cos=False):
    """The normal stream of ldt_philox_normal / ldt_sampler_step(noise = NULL): float64 [n_vec, 4] and its tolerance [n_vec, 4] for the 4-vectors
    first_vec .. first_vec + n_vec - 1 (vector e = elem_offset / 4 + i holds elements 4 e .. 4 e + 3).  Counter {lo32(e), hi32(e), step,
    0x4C445421}, key = (lo32(seed), hi32(seed)) as csrc/api.hip splits it; lanes (z0, z1) = Box-Muller(c0, c1), (z2, z3) = Box-Muller(c2, c3).
    The keyword arguments plant faults for the host tests (step_word = 3: step and the tag word exchanged)."""
    import numpy as np
    e = np.uint64(int(first_vec)) + np.arange(int(n_vec), dtype=np.uint64)
    ctr = np.zeros((int(n_vec), 4), dtype=np.uint32)
    ctr[:, 0] = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (e >> np.uint64(32)).astype(np.uint32)
    ctr[:, step_word] = np.uint32(int(step) & 0xFFFFFFFF)
    ctr[:, 5 - step_word] = np.uint32(PHILOX_TAG)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10_np(ctr, seed & 0xFFFFFFFF, seed >> 32, swap_key_increments)
    z0, z1, rel = box_muller_ref(c[:, 0], c[:, 1], swap_sin_cos)
    z2, z3, _ = box_muller_ref(c[:, 2], c[:, 3], swap_sin_cos)
    z = torch.from_numpy(np.stack([z0, z1, z2, z3], 1))
    return z, z.abs() * rel


def sweep_windows(n_items, block_items, cap_blocks, width):
    """Where a grid-stride fault shows: [(start, stop), ...] (merged, ascending, inside [0, n_items)) covering the first `width` items, `width`
    items either side of every multiple of the sweep cap_blocks * block_items below n_items, and the last `width` items."""
    sweep = cap_blocks * block_items
    raw = [(0, width), (n_items - width, n_items)] + [(k - width, k + width) for k in range(sweep, n_items, sweep)]
    out = []
    for a, b in sorted((max(a, 0), min(b, n_items)) for a, b in raw):
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def window_index(windows, device="cpu"):
    """The windows of sweep_windows as one int64 index tensor."""
    return torch.cat([torch.arange(a, b, device=device) for a, b in windows])


AMBIGUOUS_CAP = 0.02


def assert_bf16_of(out, ref64, acc, what):
    """out (bf16 or its values) == bf16_round(ref64) bit for bit, except where ref64 lies within acc (+ 2^-24 |ref64|) of a bf16 rounding
    boundary (ambiguous_ulp): there either neighbour is allowed.  NaN in the reference demands NaN, an infinity itself.  At most 2 % of the
    elements may be ambiguous (a condition on the reference: otherwise the test is not testing; choose other inputs).  -> ambiguous share."""
    assert tuple(out.shape) == tuple(ref64.shape), "%s: shape %s vs reference %s" % (what, tuple(out.shape), tuple(ref64.shape))
    o = out.double()
    ref64 = ref64.to(o.device).double()
    acc = acc.to(o.device).double().expand_as(ref64) if torch.is_tensor(acc) else torch.full_like(ref64, float(acc))
    fin = torch.isfinite(ref64)
    want = bf16_round(ref64)
    allow = torch.where(fin, ambiguous_ulp(torch.where(fin, ref64, torch.zeros_like(ref64)), acc), torch.zeros_like(ref64))
    allow = torch.where((ref64 == 0) & (acc == 0), torch.zeros_like(allow), allow)            # an exact zero is 0, not `ambiguous`
    share = float((allow > 0).double().mean()) if allow.numel() else 0.0
    assert share <= AMBIGUOUS_CAP, "%s: %.4f of the elements are within their accumulation error of a rounding boundary (cap %.2f)" % (what, share, AMBIGUOUS_CAP)
    nan = torch.isnan(ref64)
    ok = torch.where(nan, torch.isnan(o), torch.where(fin, (o == want) | ((o - want).abs() <= allow), o == ref64))
    if not bool(ok.all()):
        bad = ~ok
        C = ref64.shape[-1] if ref64.dim() else 1
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %d of %d elements are not bf16(reference) (nor its neighbour where that is allowed).  First at (row %d, col %d): got %r, "
                             "want %r (reference %r, allowance %.3g)" % (what, int(bad.sum()), bad.numel(), i // C, i % C, float(o.reshape(-1)[i]),
                                                                         float(want.reshape(-1)[i]), float(ref64.reshape(-1)[i]), float(allow.reshape(-1)[i])))
    return share


def resolved_by_bf16(ref64, acc):
    """Mask: the fp32 evaluation resolves a bf16 ulp there (acc <= a quarter ulp).  Elsewhere (a cancellation tail such as GELU below -5, where
    1 + erf is a few fp32 ulps) assert_bf16_of cannot apply and the absolute bound acc + bf16 rounding (assert_elementwise) is the check."""
    return torch.isfinite(ref64) & (acc <= 0.25 * bf16_ulp(ref64))


# ---- block activations (elementwise.hip block_act): float64 definition and what the fp32 evaluation may move
BLOCK_ACT_KINDS = {"gelu": 1, "silu": 2, "relu": 3, "leakyrelu": 4, "leakyrelu0.2": 5, "rrelu": 6, "hardswish": 7, "selu": 8}
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
RRELU_EVAL_SLOPE = float((torch.tensor(1.0 / 8.0, dtype=torch.float32) + torch.tensor(1.0 / 3.0, dtype=torch.float32)) * 0.5)
# one select and at most ONE fp32 product: a defined rounding, held bit for bit.  (rrelu too: x (11 / 48) for an 8-bit x lands on or next to a bf16
# rounding boundary for 5 % of all inputs, so a bound that allows either neighbour there would not meet assert_bf16_of's cap.)
EXACT_ACTS = ("relu", "leakyrelu", "leakyrelu0.2", "rrelu")
EXPF_MAX_ARG = 88.72283905206835      # log(FLT_MAX): above it expf is +inf


def block_act_exact(x, kind):
    """relu, the two leaky kinds and eval-mode rrelu in fp32 by torch on the CPU: one select and at most one product, bf16 in and out.  NaN stays NaN."""
    v = x.float()
    if kind == "relu":
        r = torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros_like(v)))
    else:
        slope = {"leakyrelu": 0.01, "leakyrelu0.2": 0.2, "rrelu": RRELU_EVAL_SLOPE}[kind]
        r = torch.where(v > 0, v, torch.tensor(slope, dtype=torch.float32) * v)
    return r.bfloat16()


def block_act_ref(x, kind):
    """float64 definition of block activation `kind` on bf16-exact inputs and acc, what the kernel's fp32 evaluation may differ by (before the
    bf16 rounding).  Infinite inputs follow the kernel's formula in IEEE arithmetic (0 x inf = NaN); NaN gives NaN.
      gelu      0.5 x (1 + erf(x / sqrt 2)): the argument's rounding through erf', erff, the sum's rounding; all three scaled by 0.5 |x| (for x < -5
                the sum cancels to a few ulps of 1: acc then exceeds the result, see resolved_by_bf16), two products
      silu      x / (1 + exp(-x)): expf, the sum, the quotient; exp(-x) = inf above 88.72 gives -0 where the definition is ~1e-37: allowed in full
      hardswish x min(max(x + 3, 0), 6) (1/6): the sum (where the clamp passes it), two products and the constant (as / 6: one fewer); x 6 = inf above 5.67e37
      selu      scale x | scale alpha (exp(x) - 1): expf, the difference (cancelling near 0: absolute 2^-24 exp(x)), two products and constants."""
    v = x.double()
    if kind == "gelu":
        a = v * 0.70710678118654752440
        s = 1 + torch.erf(a)
        ref = 0.5 * v * s
        d_s = a.abs() * U24 * (2 / 3.141592653589793 ** 0.5) * torch.exp(-a * a) * 2 + LIBM["erff"] * ULP32 * torch.erf(a).abs() + U24 * s.abs()
        acc = 0.5 * v.abs() * d_s + 2 * U24 * ref.abs()
    elif kind == "silu":
        e = torch.exp(-v)
        ref = v / (1 + e)
        acc = ref.abs() * ((LIBM["expf"] * ULP32 + U24) * e / (1 + e) + 2 * U24)
        acc = torch.where(-v > EXPF_MAX_ARG, ref.abs(), acc)
    elif kind == "hardswish":
        s3 = v + 3
        ref = v * torch.clamp(s3, 0, 6) / 6
        ref = torch.where(v * 6 > 3.4028234663852886e38, torch.full_like(v, float("inf")), ref)      # the formula's x * 6 overflows fp32
        acc = v.abs() * U24 * torch.where((s3 > 0) & (s3 < 6), s3, torch.zeros_like(s3)) / 6 + 3 * U24 * ref.abs()
    elif kind == "selu":
        e = torch.exp(v)
        ref = torch.where(v > 0, SELU_SCALE * v, SELU_SCALE * SELU_ALPHA * torch.expm1(v))
        neg = SELU_SCALE * SELU_ALPHA * (LIBM["expf"] * ULP32 * e + U24 * (e - 1).abs()) + 4 * U24 * ref.abs()
        acc = torch.where(v > 0, 2 * U24 * ref.abs(), neg)
    else:
        raise KeyError(kind)
    ref = torch.where(torch.isnan(v), v, ref)
    return ref, torch.where(torch.isfinite(ref), acc * SLACK, torch.zeros_like(acc))


# ---- LangevinCorrector (samplers.hip)
def batch_norms_ref(x):
    """ldt_batch_norm_sum on x [B, per]: float64 per-sample L2 norms [B], their sum, and tolerances.  A lane adds k = ceil(per / 1024) groups of
    four squares (4 products, 3 sums inside a group) to its accumulator, then 6 shuffle and 2 LDS tree additions: all terms are positive, so
    (k + 12) 2^-24 relative on the sum of squares (an FMA only removes roundings), halved by the correctly rounded sqrt + its own rounding.
    The batch sum: ceil(B / 64) additions per lane + 6 shuffles on top of the norms' own tolerances."""
    B, per = x.shape
    k = -(-per // 1024)
    n = x.double().pow(2).sum(1).sqrt()
    tn = n * ((k + 12) * 0.5 + 1) * U24 * SLACK
    s = n.sum()
    return n, s, tn, tn.sum() + (-(-B // 64) + 6) * U24 * (s + tn.sum()) * SLACK


def langevin_coef_ref(sums, n_total, snr, std_t):
    """ldt_langevin_coef: float64 {1, -step / std, sqrt(2 step), 0} from the fp32 operands, and tolerances.  grad_norm, noise_norm and r take 5
    fp32 roundings, step = 2 r r then carries 11, -step / std 12, sqrt(2 step) 11 / 2 + 1; 1 and 0 are exact."""
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    s0, s1, snr, std = float(sums[0]), float(sums[1]), f32(snr), f32(std_t)
    r = snr * (s1 / n_total) / ((s0 / n_total) / std)
    step = 2 * r * r
    ref = torch.tensor([1.0, -step / std, (2 * step) ** 0.5, 0.0], dtype=torch.float64)
    return ref, ref.abs() * torch.tensor([0.0, 12.0, 6.5, 0.0], dtype=torch.float64) * U24 * SLACK


# ---- score = -params / sqrt(var(t)) (samplers.hip vpsde_score / sde_score)
def sde_score_ref(params, t, kind, c0, c1, c2):
    """float64 -params / sqrt(var(t)) of SDE family `kind` from the fp32 operands (params [B, ...], t [B], constants as the kernel receives them:
    rounded to fp32), its tolerance, and `resolved` [B]: whether fp32 resolves var at all (var > 2 dvar; at t = 1e-6 with sigma2_0 = 0 it
    does not: var ~ 1e-7 is one ulp of e = exp(..) ~ 1, and nothing but finiteness can be asked there).
    One libm error in e (kinds 0, 1: expf of an argument that itself carries the roundings of a = -c0 t, b = 0.5 (c1 - c0) t t and a - b) or in
    powf (kind 2) is carried through var analytically: kind 0 var = 1 - (1 - c2) e; kind 1 var = (1 - e)^2 + c2 e, where 1 - e keeps e's absolute
    error and cancels at small t; kind 2 var = c0 c1^t - c0 + c2.  Then sqrt (correctly rounded) and the quotient."""
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32).double()
    c0, c1, c2 = f32(c0), f32(c1), f32(c2)
    tb = t.double()
    if kind == 2:
        P = torch.pow(c1, tb)
        var = c0 * P - c0 + c2
        dvar = c0 * P * (LIBM["powf"] * ULP32 + U24) + U24 * (c0 * P - c0).abs() + U24 * var.abs()
    else:
        a, b = -c0 * tb, 0.5 * (c1 - c0) * tb * tb
        e = torch.exp(a - b)
        de = e * (U24 * (a.abs() + 3 * b.abs() + (a - b).abs()) + LIBM["expf"] * ULP32)
        if kind == 1:
            om = 1 - e
            dom = de + U24 * om.abs()
            var = om * om + c2 * e
            dvar = 2 * om.abs() * dom + dom * dom + U24 * om * om + c2 * (de + U24 * e) + U24 * var
        else:
            var = 1 - (1 - c2) * e
            dvar = (1 - c2) * (de + 2 * U24 * e) + U24 * var.abs()
    dvar = dvar * SLACK
    resolved = var > 2 * dvar
    sd = var.clamp_min(0).sqrt()
    lo, hi = (var - dvar).clamp_min(0).sqrt(), (var + dvar).sqrt()
    shape = (-1,) + (1,) * (params.dim() - 1)
    p = params.double()
    ref = -p / sd.reshape(shape)
    rel = torch.where(resolved, torch.maximum(sd / lo - 1, 1 - sd / hi) + 2 * U24, torch.full_like(sd, float("inf")))
    return ref, ref.abs() * rel.reshape(shape) * SLACK, resolved


# ---- encoder helpers (pointops.hip)
def actnorm_ref(x, shift, log_scale):
    """ActNorm (eval): float64 (x - shift) exp(-log_scale) on x [B, per], parameters [per]; one difference, expf, one product."""
    ref = (x.double() - shift.double()) * torch.exp(-log_scale.double())
    return ref, ref.abs() * (2 * U24 + LIBM["expf"] * ULP32) * SLACK


def reparam_ref(post, noise, lo, hi):
    """ldt_reparam: mu, logvar = clamp(post[:, z:], lo, hi) (both selections: exact, compared bit for bit) and float64 eps = mu + exp(logvar / 2)
    noise with its tolerance: logvar / 2 is exact, expf, then ONE fused multiply-add (common.h reparam_eps)."""
    z = post.shape[1] // 2
    mu, lv = post[:, :z].clone(), post[:, z:].clamp(float(torch.tensor(lo, dtype=torch.float32)), float(torch.tensor(hi, dtype=torch.float32)))
    prod = noise.double() * torch.exp(lv.double() / 2)
    ref = mu.double() + prod
    return mu, lv, ref, (prod.abs() * LIBM["expf"] * ULP32 + U24 * ref.abs()) * SLACK


LOG_SQRT_2PI_F32 = float(torch.tensor(0.9189385332, dtype=torch.float32))       # the constant as csrc/eval_loss.hip holds it


def reparam_kl_ref(eps, mu, lv):
    """ldt_reparam_kl's log q(z) and KL per element in float64, on the kernel's own fp32 eps, mu and clamped logvar, with the tolerances of its
    stated operation order (FMA contraction off): d = eps - mu; a = (-0.5 (d d)) / expf(lv); b = 0.5 lv; logqz = (a - b) - c;
    logpz = (-0.5 (eps eps)) - c; kl = logqz - logpz.  With u = 2^-24: a carries d (u, twice through the square), the square (u), expf
    (LIBM ulps = 2 LIBM u) and the division (u); the halvings are exact; each difference rounds once.
    -> (logqz, tol_logqz, kl, tol_kl)."""
    eps, mu, lv = eps.double(), mu.double(), lv.double()
    d = eps - mu
    a = (-0.5 * (d * d)) / torch.exp(lv)
    b = 0.5 * lv
    logqz = (a - b) - LOG_SQRT_2PI_F32
    half_sq = 0.5 * (eps * eps)
    logpz = -half_sq - LOG_SQRT_2PI_F32
    kl = logqz - logpz
    tol_q = SLACK * U24 * ((4 + 2 * LIBM["expf"]) * a.abs() + (a - b).abs() + logqz.abs())
    tol_k = tol_q + SLACK * U24 * (2 * half_sq + logpz.abs() + kl.abs())
    return logqz, tol_q, kl, tol_k


def mixture_seed_ref(eps, sig, mu, logits):
    """InitialSet mixture rows: float64 sum_m (eps[r, m] sig[m] + mu[m]) softmax(logits)[m] and its tolerance.  A weight w_m carries the rounding
    of d_m = logit_m - max (|d_m| 2^-24 through exp), expf, the same for the largest term of the denominator + its n_mix - 1 additions, and the
    quotient; a weight that underflows (d_m < -87) is in error by itself, at most 2^-126.  A term carries product, sum and product with w (an
    FMA removes one), the accumulation n_mix additions."""
    n_mix = logits.numel()
    d = logits.double() - logits.double().max()
    w = torch.softmax(logits.double(), 0)
    rw = d.abs() * U24 + LIBM["expf"] * ULP32
    rw = rw + rw.max() + n_mix * U24
    es = eps.double() * sig.double()
    pre = es + mu.double()                                                  # [rows, n_mix, D]
    wv = w[None, :, None]
    term = pre * wv
    ref = term.sum(1)
    tol = (wv * (es.abs() * U24 + pre.abs() * (2 * U24 + rw[None, :, None])) + 2.0 ** -126 * pre.abs()).sum(1) + n_mix * U24 * term.abs().sum(1)
    return ref, tol * SLACK


def norm_points_ref(xyz, unbiased=True):
    """Compressor.norm_pts: float64 (p - mean) / std per cloud and coordinate (UNBIASED std, torch.std's default, Network.py:170-174) on xyz
    [B, n, 3] and its tolerance.  The kernel sums in fp64 (ceil(n / 256) + 12 additions; var = (q - n mean^2) / (n - 1) cancels, so those
    2^-53 count against q + n mean^2), then rounds mean and 1 / std to fp32 BEFORE use: 2^-24 |mean| / std absolute, 2^-24 relative; the
    difference and the product round once each."""
    p = xyz.double()
    n = p.shape[1]
    mean = p.mean(1, keepdim=True)
    var = p.var(1, unbiased=unbiased, keepdim=True)
    inv = 1 / var.sqrt()
    ref = (p - mean) * inv
    q = (p * p).sum(1, keepdim=True)
    rel64 = 0.5 * (-(-n // 256) + 12) * 2.0 ** -53 * (q + n * mean * mean) / ((n - 1) * var)
    return ref, (U24 * mean.abs() * inv + ref.abs() * (3 * U24 + rel64)) * SLACK


def group_stats_ref(x, B, T, C, G, eps, unbiased=False, eps_outside=False):
    """nn.GroupNorm's statistics (BIASED variance, eps inside the square root) on token-major rows x [B T, C]: float64 [B, G, 2] = (mean,
    1 / sqrt(var + eps)) and its tolerance: fp64 sums (2^-53 per addition against sum |x| and sum x^2, ceil(T cg / 256) + 10 of them), then one
    rounding to fp32 each.  unbiased / eps_outside: the planted faults of the host tests."""
    cg = C // G
    xd = x.double()[:, :C].reshape(B, T, G, cg).permute(0, 2, 1, 3).reshape(B, G, T * cg)
    n = T * cg
    mean = xd.mean(2)
    var = xd.var(2, unbiased=unbiased) if n > 1 else torch.zeros_like(mean)
    e = float(torch.tensor(eps, dtype=torch.float32))
    rstd = 1 / (var.sqrt() + e) if eps_outside else 1 / torch.sqrt(var + e)
    adds = (-(-n // 256) + 10) * 2.0 ** -53
    dvar = adds * ((xd * xd).mean(2) + mean * mean) * 2
    ref = torch.stack([mean, rstd], -1)
    tol = torch.stack([U24 * mean.abs() + adds * xd.abs().mean(2), rstd * (U24 + 0.5 * dvar / (var + e))], -1)
    return ref, tol * SLACK


def norm_apply_ref(x, stats=None, rows_per_stat=1, w=None, b=None, shift=None, scale=None, rows_per_sample=1):
    """ldt_norm_apply before its bf16 rounding, float64 from the fp32 operands (stats [S, G, 2] fp32 as the kernel reads them; None: identity):
    pre = ((x - mean) rstd [w + b]) [(1 + scale) + shift] and acc, what fp32 may move: a rounding per operation (a product-sum pair may fuse:
    never more), the rounding of 1 + scale carried through the product.  x [M, C]; shift / scale [nS, C] by row // rows_per_sample."""
    xd = x.double()
    M, C = xd.shape
    if stats is not None:
        G = stats.shape[1]
        st = stats.double()[torch.arange(M, device=x.device) // rows_per_stat]                   # [M, G, 2]
        mean, rstd = st[:, :, 0].repeat_interleave(C // G, 1), st[:, :, 1].repeat_interleave(C // G, 1)
        pre = (xd - mean) * rstd
        acc = 2 * U24 * pre.abs()
    else:
        pre, acc = xd, torch.zeros_like(xd)
    if w is not None:
        pw = pre * w.double()
        pre = pw + b.double()
        acc = acc * w.double().abs() + U24 * pw.abs() + U24 * pre.abs()
    if scale is not None:
        sc = 1 + sample_rows(scale, M, rows_per_sample)
        ps = pre * sc
        pre2 = ps + sample_rows(shift, M, rows_per_sample)
        acc = acc * sc.abs() + 2 * U24 * ps.abs() + U24 * pre2.abs()
        pre = pre2
    return pre, acc * SLACK


def sinusoid_ref(t, freq):
    """float64 [n, 2 half] = [sin(a) | cos(a)] of the FLOAT32 product a = t f (the kernel's __fmul_rn: a defined rounding) and the tolerance
    LIBM['sincosf'] ulps of each value."""
    a = (t.float()[:, None] * freq.float()[None, :]).double()
    ref = torch.cat([torch.sin(a), torch.cos(a)], 1)
    return ref, ref.abs() * LIBM["sincosf"] * ULP32 * SLACK


# ---- Chamfer (pointops.hip chamfer_min_kernel, metrics.hip chamfer_pairwise_kernel)
CHAMFER_ROUNDINGS = 9


def chamfer_dir_ref(q, r):
    """min_j |q_i - r_j|^2 for q [B, nq, 3] against r [B, nr, 3]: float64 [B, nq] and its tolerance.  The kernels evaluate the reference's expanded
    form (|q|^2 + |r|^2) - 2 q.r: three roundings in each squared norm, one in their sum, three in the dot product (|q.r| <= (|q|^2 + |r|^2) / 2,
    doubled exactly), one in the difference (<= 2 (|q|^2 + |r|^2)): 9 2^-24 (|q|^2 + |r|^2), ABSOLUTE — it does not shrink with the distance.
    A minimum moves by at most the largest perturbation of its candidates: 9 2^-24 (|q_i|^2 + max_j |r_j|^2)."""
    qd, rd = q.double(), r.double()
    ref = torch.cat([(qd[:, i:i + 256, None, :] - rd[:, None, :, :]).pow(2).sum(-1).min(2).values for i in range(0, qd.shape[1], 256)], 1)
    tol = CHAMFER_ROUNDINGS * U24 * (qd.pow(2).sum(-1) + rd.pow(2).sum(-1).max(1, keepdim=True).values) * SLACK
    return ref, tol


def chamfer_ref(a, b):
    """ops.chamfer(a [B, na, 3], b [B, nb, 3]) -> ((dl [B, nb], tol), (dr [B, na], tol)): dl = for every point of b its nearest a."""
    return chamfer_dir_ref(b, a), chamfer_dir_ref(a, b)


def chamfer_pairwise_ref(x, y):
    """ops.chamfer_pairwise(x [S, n, 3], y [R, m, 3]): float64 cd [S, R] = mean_j min_i + mean_i min_j and its tolerance: the per-query bound of
    chamfer_dir_ref through the mean, plus the summation (4 ceil(nq / 1024) additions per lane, 6 shuffles, 2 LDS, the quotient) against the mean
    of the magnitudes, plus the final sum's rounding."""
    S, n = x.shape[:2]
    R, m = y.shape[:2]
    ref, tol = torch.zeros(S, R, dtype=torch.float64, device=x.device), torch.zeros(S, R, dtype=torch.float64, device=x.device)
    for s in range(S):
        for r in range(R):
            for qq, rr in ((y[r:r + 1], x[s:s + 1]), (x[s:s + 1], y[r:r + 1])):
                d, t = chamfer_dir_ref(qq, rr)
                nq = qq.shape[1]
                mean = d.mean()
                tm = t.mean() + (4 * -(-nq // 1024) + 9) * U24 * (d.abs() + t).mean()
                ref[s, r] += mean
                tol[s, r] += tm
    return ref, (tol + U24 * ref.abs()) * SLACK


# ---- the expressions the exact kernels are held to (fp32 by torch on the CPU: every product and sum rounds on its own, as `fp contract(off)`)
def fma32(a, b, c):
    """float32(a b + c) with ONE rounding (the product of two fp32 values is exact in float64): what a contraction to FMA would compute."""
    return (a.double() * b.double() + c.double()).float()


def sampler_step_expr(x, p, z, cf, mode, fused=False):
    """ldt_sampler_step on fp32 tensors with the coefficient row cf [4] -> (x_mean, x_next).  mode 0: score = -p / std, x_mean = (x + beta score) /
    sqrt(1 - beta), x = x_mean + sqrt(beta) z with cf = {beta, std, sqrt(1 - beta), sqrt(beta)}; mode 1: x_mean = A x + B p, x = x_mean + C z.
    fused: the planted fault (mode 1 with A x + B p and x_mean + C z contracted)."""
    if mode == 0:
        xm = (x + cf[0] * (-p / cf[1])) / cf[2]
        return xm, xm + cf[3] * z
    if fused:
        xm = fma32(cf[0], x, cf[1] * p)
        return xm, fma32(cf[2], z, xm)
    xm = cf[0] * x + cf[1] * p
    return xm, xm + cf[2] * z


def pndm_transfer_expr(x, et, d, p, q, fused=False):
    """x + d (p x - q et) with the three scalars as fp32; fused: p x - q et and x + d (..) contracted (the planted fault)."""
    d, p, q = [torch.tensor(float(v), dtype=torch.float32) for v in (d, p, q)]
    if fused:
        return fma32(d, fma32(p, x, -(q * et)), x)
    return x + d * (p * x - q * et)


def lincomb4_expr(a, c, s, fused=False):
    """s (((c0 a0 + c1 a1) + c2 a2) + c3 a3), left to right; fused: every sum contracted with its product (the planted fault)."""
    c = [torch.tensor(float(v), dtype=torch.float32) for v in c]
    s = torch.tensor(float(s), dtype=torch.float32)
    if fused:
        return s * fma32(c[3], a[3], fma32(c[2], a[2], fma32(c[1], a[1], c[0] * a[0])))
    return s * (((c[0] * a[0] + c[1] * a[1]) + c[2] * a[2]) + c[3] * a[3])


PNDM_COEF_SETS = (((55.0, -59.0, 37.0, -9.0), 1 / 24), ((1.0, 2.0, 2.0, 1.0), 1 / 6))


def maxpool_expr(x, G, n):
    """max over the n rows of each group of the row-major view x [G n, C] (any row stride), fp32 [G, C]; NaN propagates (torch.max)."""
    return x.float().reshape(G, n, x.shape[1]).max(1).values


def check_block_act(out, x, kind, what):
    """ldt_block_activation's bf16 `out` for bf16 inputs `x` (any shape): relu and the leaky kinds == block_act_exact; the others == bf16(float64
    definition) where fp32 resolves a bf16 ulp (assert_bf16_of) and within acc + the bf16 rounding elsewhere (assert_elementwise); NaN in ->
    NaN out.  -> (worst err / tol over the unresolved elements, ambiguous share of the resolved ones)."""
    if kind in EXACT_ACTS:
        want = block_act_exact(x, kind).to(out.device)
        same = (out == want) | (torch.isnan(out) & torch.isnan(want))
        assert bool(same.all()), "%s: %d elements differ from the fp32 expression (first at flat index %d)" % (
            what, int((~same).sum()), int(torch.nonzero(~same.reshape(-1))[0]))
        return 0.0, 0.0
    ref, acc = block_act_ref(x.to(out.device), kind)
    res = resolved_by_bf16(ref, acc) | ~torch.isfinite(ref)
    share = assert_bf16_of(out[res].reshape(1, -1), ref[res].reshape(1, -1), acc[res].reshape(1, -1), what)
    ratio = 0.0
    if bool((~res).any()):
        r = ref[~res].reshape(1, -1)
        ratio = assert_elementwise(out[~res].reshape(1, -1), r, acc[~res].reshape(1, -1) * (1 + U8) + U8 * r.abs() + 2.0 ** -133, what + " (cancellation tail)")
    return ratio, share


def all_bf16_patterns():
    """Every bf16 bit pattern once, as a [512, 128] bf16 tensor."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(512, 128)


# ------------------------------------------------------------------------------------------------------------- Score training step
# (csrc/score_bwd.hip, attention_bwd.hip, optim.hip; test_gpu_train_kernels.py holds each kernel alone with these, test_gpu_train_tape.py every call of a
# whole backward on that call's own recorded operands, test_gpu_train_stream_exact.py the stream kernels at width and past their grid caps;
# validated without a GPU, planted faults included, by test_train_tape_host.py and test_train_stream_host.py)
#
# Every function takes the operands the kernel read and returns (float64 reference, componentwise bound), or two dicts of them for a kernel
# with several outputs.  The bounds are built the way gemm_tol is:
#   * an accumulation term C_ACC * n * 2^-24 * sum |terms| for every fp32 sum of n terms (the column sums over rows are carried in float64
#     by the kernels, which leaves the term far from attained);
#   * 2^-8 |value| for every intermediate the kernel rounds to bf16 (P and dS in the attention backward) and for a bf16 output;
#   * 2^-24 |value| per fp32 rounding of the element chain, and a stated absolute allowance where libm's erff / expf / logf enter.
LIBM_ABS = 1e-6          # |erff|, |expf| on [-inf, 0], sigmoid: a few fp32 ulp of a value <= 1 (as GELU_FAST_ABS allows the forward)


def pad64(k):
    return (k + 63) // 64 * 64


def transpose_cast_want(src, rows_pad=None):
    """bf16 [C, rows_pad] the transposing cast owes for src [R, C]: bf16(src)^T, columns R.. zero.  Exact: compared with torch.equal."""
    R, C = src.shape
    want = torch.zeros(C, pad64(R) if rows_pad is None else rows_pad, dtype=torch.bfloat16, device=src.device)
    want[:, :R] = src.to(torch.bfloat16).t()
    return want


def cast_pad_want(src, cols_pad):
    """bf16 [rows, cols_pad] of ldt_cast_pad_bf16: bf16(src), columns cols.. zero.  Exact."""
    want = torch.zeros(src.shape[0], cols_pad, dtype=torch.bfloat16, device=src.device)
    want[:, :src.shape[1]] = src.to(torch.bfloat16)
    return want


def colsum_ref(dy):
    """bound: one fp32 sum of M terms + the stored value's rounding"""
    M = dy.shape[0]
    ref = dy.double().sum(0)
    return ref, C_ACC * M * U24 * dy.double().abs().sum(0) + U24 * ref.abs()


def wgrad_ref(dy, x):
    """dW = dY^T X from the operands the GEMM read (bf16(dy)^T [N, M], bf16(x)^T [K, M]).  bound: gemm_tol over the padded contraction
    length (the pad adds exact zeros)"""
    a, b = dy.to(torch.bfloat16).t().contiguous(), x.to(torch.bfloat16).t().contiguous()
    return a.double() @ b.double().T, gemm_tol(a, b, None, pad64(dy.shape[0]), torch.float32)


def dgrad_ref(dyb, wt, out_dtype=torch.float32):
    """dX = dY W from the bf16 operands dyb [M, N] and wt = W^T [K, N] (N: the contraction as the GEMM runs it, zero padding included)."""
    return dyb.double() @ wt.double().T, gemm_tol(dyb, wt, None, dyb.shape[1], out_dtype)


def sgemm_ref(a, w, bias=None):
    """ldt_sgemm (no activation) against float64.  The bound's factor on 2^-24 (|a| |w|^T + |b|): K + 1 roundings at the worst; these kernels
    add their products one after another, so their error grows like sqrt(K) with a larger constant than the blocked bf16 kernels': hence a
    floor of 8 under C_ACC K (test_gpu_kernel_exact.py::test_sgemm_bound_and_integer_probe).  -> (ref, tol)."""
    K = a.shape[1]
    ref = a.double() @ w.double().T
    absacc = a.double().abs() @ w.double().abs().T
    if bias is not None:
        ref, absacc = ref + bias.double(), absacc + bias.double().abs()
    return ref, min(K + 1, max(C_ACC * K, 8)) * U24 * absacc + U24 * ref.abs()


def layernorm_modulate_bwd_ref(x, dy, scale, rps, dx0):
    """x, dy, dx0 [M, C] fp32, scale [M / rps, C] -> ({'dx', 'dshift', 'dscale'} references, the same of bounds); dx = dx0 + the LayerNorm
    gradient (dx is accumulated into), and the row statistics (mean, var) for a caller that asserts a property of its case."""
    M, C = x.shape
    x6, dy6 = x.double(), dy.double()
    mean, var = x6.mean(1, keepdim=True), x6.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-6)
    xh = (x6 - mean) * rstd
    s1 = 1 + scale.double().repeat_interleave(rps, 0)
    gg = dy6 * s1
    mg, mgx = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    ref_dx = dx0.double() + rstd * (gg - mg - xh * mgx)
    # bound.  Row statistics in fp32: mean = a C-term sum (C_ACC C 2^-24 mean|x|, + its rounding); d = x - mean inherits it, so
    # e_xh = |error of LN(x)| = 2^-24 (4 (1 + |xh|) + (C_ACC C + 2) mean|x| / std); rstd: relative e_r = e_xh(row max) + 2^-24 (C_ACC C + 8).
    # The two row means of g and g xh: C_ACC C 2^-24 mean|.| each (+ mean|g| e_xh).  Element chain: 2^-24 per operation on its magnitude.
    sd = torch.sqrt(var)
    e_xh = U24 * (4 * (1 + xh.abs()) + (C_ACC * C + 2) * x6.abs().mean(1, keepdim=True) / sd)
    e_r = e_xh.amax(1, keepdim=True) + U24 * (C_ACC * C + 8)
    e_mg = U24 * (C_ACC * C + 2) * gg.abs().mean(1, keepdim=True)
    e_mgx = U24 * (C_ACC * C + 2) * (gg * xh).abs().mean(1, keepdim=True) + (gg.abs() * e_xh).mean(1, keepdim=True)
    inner = gg - mg - xh * mgx
    tol_dx = (rstd * (4 * U24 * (gg.abs() + mg.abs() + (xh * mgx).abs()) + e_mg + e_xh * mgx.abs() + xh.abs() * e_mgx)
              + (e_r + 2 * U24) * (rstd * inner).abs() + U24 * ref_dx.abs())
    S = M // rps
    ref_sh = dy6.view(S, rps, C).sum(1)
    ref_sc = (dy6 * xh).view(S, rps, C).sum(1)
    # dshift: float64 sum of fp32 terms, one rounding (+ the issue's accumulation term).  dscale: each term fp32(dy * xh): |dy| e_xh + 2^-24 |dy xh|.
    tol_sh = C_ACC * rps * U24 * dy6.abs().view(S, rps, C).sum(1) + U24 * ref_sh.abs()
    tol_sc = ((dy6.abs() * e_xh + U24 * (dy6 * xh).abs()).view(S, rps, C).sum(1) + C_ACC * rps * U24 * (dy6 * xh).abs().view(S, rps, C).sum(1)
              + U24 * ref_sc.abs())
    return {"dx": ref_dx, "dshift": ref_sh, "dscale": ref_sc}, {"dx": tol_dx, "dshift": tol_sh, "dscale": tol_sc}, (mean, var)


def gelu_bwd_ref(u, dh):
    """bound: bf16 output 2^-8 |ref|; fp32 chain 8 x 2^-24 |ref|; erff and expf absolute accuracy times |dh| (1 + |u|)"""
    import math
    u6 = u.double()
    dgelu = 0.5 * (1 + torch.erf(u6 / math.sqrt(2))) + u6 * torch.exp(-0.5 * u6 * u6) / math.sqrt(2 * math.pi)
    ref = dh.double() * dgelu
    return ref, U8 * ref.abs() + 8 * U24 * ref.abs() + LIBM_ABS * dh.double().abs() * (1 + u6.abs())


def gate_residual_bwd_ref(dy, gate, a, rps):
    """dy [M, C] fp32, gate [M / rps, C] (the column block), a [M, C] or None -> ({'da', 'dgate'} references, bounds).
    bound: da one fp32 product then bf16; dgate float64 sum of fp32 products (2^-24 each) + the accumulation term + its rounding"""
    M, C = dy.shape
    S = M // rps
    ref_da = dy.double() * gate.double().repeat_interleave(rps, 0)
    ref, tol = {"da": ref_da}, {"da": (U8 + U24) * ref_da.abs()}
    if a is not None:
        terms = dy.double() * a.double()
        ref["dgate"] = terms.view(S, rps, C).sum(1)
        tol["dgate"] = (1 + C_ACC * rps) * U24 * terms.abs().view(S, rps, C).sum(1) + U24 * ref["dgate"].abs()
    return ref, tol


def silu_bwd_ref(c, dy):
    """-> ({'dc', 'act'} references, bounds).  bound: fp32 chain 8 x 2^-24 |ref| + the sigmoid's absolute accuracy times |dy| (1 + |c|);
    act = SiLU(c): 4 x 2^-24 |act| + the sigmoid's accuracy times |c|"""
    c6 = c.double()
    sg = torch.sigmoid(c6)
    ref = dy.double() * sg * (1 + c6 * (1 - sg))
    return ({"dc": ref, "act": c6 * sg},
            {"dc": 8 * U24 * ref.abs() + LIBM_ABS * dy.double().abs() * (1 + c6.abs()), "act": 4 * U24 * (c6 * sg).abs() + LIBM_ABS * c6.abs()})


def dsm_loss_bwd_ref(eta, params, w=None, l1=False):
    """Gradient of mean(w |eta - params|^p) by float64 autograd.  bound: four fp32 roundings (d, the factor 2 is exact, the weight, 1 / n and
    its product)"""
    with torch.enable_grad():
        p6 = params.detach().double().requires_grad_(True)
        d = eta.double() - p6
        dist = d.abs() if l1 else d * d
        (dist * (1 if w is None else w.double()[:, None, None])).mean().backward()
    return p6.grad, 4 * U24 * p6.grad.abs()


def embedding_grad_ref(dc, label, K):
    """bound: n_k - 1 sequential fp32 additions of class k's rows, worst case (n_k small: C_ACC's statistics do not apply)"""
    D = dc.shape[1]
    label = label.long()
    ref = torch.zeros(K, D, dtype=torch.float64, device=dc.device).index_add_(0, label, dc.double())
    mag = torch.zeros(K, D, dtype=torch.float64, device=dc.device).index_add_(0, label, dc.double().abs())
    nk = torch.bincount(label, minlength=K).double()[:, None]
    return ref, (nk - 1).clamp_min(0) * U24 * mag


def adam_ema_ref(st32, grad, step, lr, b1, b2, eps, weight_decay, decay, ema_init, moment_rounding=False):
    """One step of torch.optim.Adam + the reference's EMA lines (tools/utils.py:49-62) in float64 from the fp32 state st32 = {'p', 'm', 'v',
    'ema'} ('ema' may be None: no EMA is kept) and the fp32 gradient Adam is FED (after clip_grad_norm_'s in-place scaling).  step: the step
    being taken, from 1; ema_init: the EMA starts as a clone of the updated parameter (a parameter's first step).
    -> ({'p', 'exp_avg', 'exp_avg_sq', 'ema'} float64 references, the same of bounds; no 'ema' without one).
    bound: 2^-24 |value| (the rounding of the STORED fp32 value against an exact result) + 8 x 2 x 2^-24 |value - its previous value|: eight
    roundings in the update chain, doubled because the device's sqrt and divide need not be correctly rounded; for p, exp_avg and
    exp_avg_sq alike, each with its own step delta.  The EMA is a function of the NEW parameter, ema = ema_old d + (1 - d) p: with ema_init
    ema_old = p, so the EMA IS the new parameter and is held to the parameter's bound; otherwise it inherits p's error with the factor
    d ema / d p = 1 - d and adds its own rounding plus the roundings of its change.
    moment_rounding: what `8 roundings relative to |delta p|` omits.  delta p = -step_size m_new / denom, and m_new = m + w1 (g - m) is
    formed from fl(g - m): a rounding of 2^-24 |g - m| that enters m_new scaled by w1, 2^-24 |delta m| — relative to the CHANGE of the
    moment, not to m_new.  From zero state (steps 1-3 of test_adam_ema_step_against_torch_adam) |delta m| <= |m_new| and the eight roundings cover it; from a
    late state m + w1 (g - m) can cancel (g ~ -m (1 - w1) / w1), |m_new| << |delta m|, and the rounding of the difference alone exceeds
    16 x 2^-24 |delta p| (a faithful fp32 emulation leaves the plain bound at 2 of 2,097,411 elements of train_stream_checks.adam_main_case:
    test_train_stream_host.py).  With weight decay the fed gradient g + wd p is itself rounded once, 2^-24 |g'| <= 2^-24 (|g' - m| + |m|),
    which adds w1 2^-24 |g'| <= 2^-24 ((1 + w1) |delta m| + w1 |m_new|).  moment_rounding=True therefore adds to p's bound
    3 x 2^-24 |delta m| step_size / denom (1 + (1 + w1) <= 3; the |m_new| part is one of the eight), with step_size and denom of the float64
    reference; the EMA inherits it through p's bound.  exp_avg_sq is a sum of non-negative terms and cannot cancel."""
    p = torch.nn.Parameter(st32["p"].double())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay)
    if step > 1:
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": st32["m"].double(), "exp_avg_sq": st32["v"].double()}
    p.grad = grad.double()
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == step
    ref = {"p": p.data, "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
    tol = {nm: U24 * ref[nm].abs() + 8 * 2 * U24 * (ref[nm] - st32[old].double()).abs() for nm, old in (("p", "p"), ("exp_avg", "m"), ("exp_avg_sq", "v"))}
    if moment_rounding:
        step_size = lr / (1.0 - b1 ** step)
        denom = ref["exp_avg_sq"].sqrt() / (1.0 - b2 ** step) ** 0.5 + eps
        tol["p"] = tol["p"] + 3 * U24 * (ref["exp_avg"] - st32["m"].double()).abs() * step_size / denom
    if st32.get("ema") is not None:
        ema = p.data.clone() if ema_init else st32["ema"].double()
        ema.mul_(decay).add_(p.data, alpha=1. - decay)
        ref["ema"] = ema
        tol["ema"] = tol["p"] if ema_init else U24 * ema.abs() + 8 * 2 * U24 * (ema - st32["ema"].double()).abs() + (1.0 - decay) * tol["p"]
    return ref, tol


def attn_bwd_ref(q, k, v, o, do, B, H, Nq, Nk, Dh=64, rounded=True):
    """The attention backward in float64 from the bf16 operands: q rows [B Nq, H Dh], k and v rows [B Nk, H Dh], o and do [B, H, Nq, Dh]
    -> (references, componentwise bounds): dq [B, H, Nq, Dh]; dk, dv [B, H, Nk, Dh].  Self-attention: Nq = Nk.
    rounded=True    P and dS are rounded to bf16 before the second products (MFMA operands): the 2^-8 terms on P and dS are present.
                    The kernels for head widths 32 and 64.
    rounded=False   P and dS stay fp32 (per-lane FMAs): the 2^-8 terms are absent.  The kernels for 8 and 16."""
    q, k, v = heads(q, B, Nq, H, Dh), heads(k, B, Nk, H, Dh), heads(v, B, Nk, H, Dh)
    o6, g6 = o.double(), do.double()
    sc = Dh ** -0.5
    s = q @ k.transpose(-1, -2) * sc
    L = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - L)
    D = (g6 * o6).sum(-1, keepdim=True)
    dP = g6 @ v.transpose(-1, -2)
    dS = P * (dP - D)
    ref = {"dq": dS @ k * sc, "dk": dS.transpose(-1, -2) @ q * sc, "dv": P.transpose(-1, -2) @ g6}
    # bound.  s and dP: fp32 MFMA sums of Dh terms (C_ACC Dh 2^-24 |.||.|); the exponent s - L carries that of s twice (L is built from the
    # same sums) + 8 x 2^-24 (|s| + |L|) of its fp32 arithmetic + expf / logf: P's relative error e_arg.  D: a Dh-term fp32 sum.
    # dS in fp32: P e_arg |dP - D| + P (e_dP + e_D) + 2 x 2^-24 |dS|; then rounded to bf16 (u8 = 2^-8) or kept (u8 = 0), and P likewise for
    # dV.  Second products: C_ACC n 2^-24 |.||.| each — dq sums over the Nk keys, dk and dv over the Nq queries — the scale in fp32 (dq, dk),
    # and the bf16 output 2^-8 |ref|.
    u8 = U8 if rounded else 0.0
    acc = C_ACC * Dh * U24
    e_arg = 2 * acc * (q.abs() @ k.abs().transpose(-1, -2)) * sc + 8 * U24 * (s.abs() + L.abs()) + 4 * LIBM_ABS
    e_dP = acc * (g6.abs() @ v.abs().transpose(-1, -2))
    e_D = acc * (g6.abs() * o6.abs()).sum(-1, keepdim=True)
    e_dS = P * e_arg * (dP - D).abs() + P * (e_dP + e_D) + (2 * U24 + u8) * dS.abs()
    e_P = P * e_arg + u8 * P
    acc_k, acc_q = C_ACC * Nk * U24, C_ACC * Nq * U24
    tol = {"dq": sc * (e_dS @ k.abs() + acc_k * (dS.abs() @ k.abs())) + (U8 + 2 * U24) * ref["dq"].abs(),
           "dk": sc * (e_dS.transpose(-1, -2) @ q.abs() + acc_q * (dS.abs().transpose(-1, -2) @ q.abs())) + (U8 + 2 * U24) * ref["dk"].abs(),
           "dv": e_P.transpose(-1, -2) @ g6.abs() + acc_q * (P.transpose(-1, -2) @ g6.abs()) + (U8 + U24) * ref["dv"].abs()}
    return ref, tol
