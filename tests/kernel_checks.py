"""Per-element checks and exact probes for the MFMA kernels (used by test_gpu_kernel_exact.py and test_gpu_kernels.py).

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


def attention_gather_probe(B, H, Nq, Nk, dh, seed):
    """Q [B, Nq, H dh], K, V [B, Nk, H dh] (bf16-exact float32) such that query i of head (b, h) scores at least 40 above every other key at key
    pi(i): K[j] carries the +1 / -1 code of the bits of j in the first 11 channels of each head, Q[i] = 160 x the code of pi(i) — a one-bit
    difference costs 2 * 160 / sqrt(dh) >= 40 in score, so every other weight is below e^-40 and O[b, h, i] == V[b, pi(i), head h] to the bit
    (V has magnitudes in [2^-6, 4]: the leftovers cannot move a last bit).  -> (q, k, v, want [B, H, Nq, dh])."""
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
            k[b, :, h * dh:h * dh + 11] = code(torch.arange(Nk))
            q[b, :, h * dh:h * dh + 11] = 160.0 * code(pi)
            want[b, h] = v[b, pi, h * dh:(h + 1) * dh]
            # the construction's claim, checked: the gap to the runner-up in score
            s = (q[b, :, h * dh:(h + 1) * dh].double() @ k[b, :, h * dh:(h + 1) * dh].double().T) * dh ** -0.5
            top = s.gather(1, pi[:, None])
            s.scatter_(1, pi[:, None], float("-inf"))
            assert Nk == 1 or float((top - s.max(1, keepdim=True).values).min()) >= 40.0
    return q, k, v, want
