"""Helpers of the attention-backward tests (ldt_attention_bwd, _narrow and _cross: csrc/attention_bwd.hip): the self-attention cases at
head widths 8, 16 and 32 of test_train_narrow_host.py, test_gpu_train_narrow_kernels.py and test_gpu_train_narrow_tape.py, and what every
case, one length or two (tests/cross_bwd_checks.py), is prepared and emulated with.

The float64 reference and its componentwise bound are kernel_checks.attn_bwd_ref; `rounds` says which of its two forms holds the kernel of
a head width.  `emulate` is the kernels' arithmetic in fp32 on the CPU, with the faults the host tests plant."""
import torch

import kernel_checks as kc

# (B, H, N, Dh): the smallest shapes at which the kernels can go wrong (one wave per 16 rows, 16 columns per step, 32 in the 32-wide form)
SHAPES = [
    (2, 16, 32, 8),          # the hybrid shape
    (2, 8, 32, 16),
    (1, 1, 1, 8),            # one score
    (2, 3, 8, 8),            # N < 16, H odd
    (2, 3, 5, 16),
    (1, 2, 72, 8),           # partial last 16-block and partial 32-step
    (1, 2, 72, 16),
    (3, 16, 40, 8),
    (1, 2, 300, 16),
    (1, 1, 512, 8),          # the limit
    (2, 4, 33, 32),
    (1, 2, 72, 32),
]
LARGE = [(1, 2, 72, 8), (1, 2, 72, 16), (1, 2, 72, 32)]
CASES = [s + (False,) for s in SHAPES] + [s + (True,) for s in LARGE]


def rounds(Dh):
    """Does the kernel for this head width round P and dS to bf16?  """
    return Dh >= 32


def bf(t):
    return t.to(torch.bfloat16)


def attn_case(B, H, N, Dh, large=False, seed=None):
    """test_gpu_train_kernels.attn_case at head width Dh -> (qkv bf16 [B N, 3 H Dh], dO bf16 [B, H, N, Dh]).  large: one logit per row is
    ~96, far above the others (q += (96 / sqrt(Dh)) k[(7 i + 3) % N]; 12 at Dh 64)."""
    g = torch.Generator().manual_seed(100 * B + 10 * H + N + int(large) + Dh if seed is None else seed)
    C = H * Dh
    qkv = torch.randn(B * N, 3 * C, generator=g)
    if large:
        q = qkv[:, :C].view(B, N, H, Dh)
        k = qkv[:, C:2 * C].view(B, N, H, Dh)
        q += (96.0 / Dh ** 0.5) * k[:, (7 * torch.arange(N) + 3) % N]
    return bf(qkv), bf(torch.randn(B, H, N, Dh, generator=g))


def split(qkv):
    """rows [B N, 3 C] = Q | K | V -> (q [B N, C], kv [B N, 2 C])"""
    C = qkv.shape[1] // 3
    return qkv[:, :C], qkv[:, C:]


def heads(z, B, H, N, Dh):
    """rows [B N, H Dh] -> [B, H, N, Dh]"""
    return z.reshape(B, N, H, Dh).permute(0, 2, 1, 3)


def scores64(q, kv, B, H, Nq, Nk, Dh):
    """q rows [B Nq, H Dh], kv rows [B Nk, 2 H Dh] = K | V -> float64 logits [B, H, Nq, Nk]"""
    C = H * Dh
    return heads(q.double(), B, H, Nq, Dh) @ heads(kv[:, :C].double(), B, H, Nk, Dh).transpose(-1, -2) * Dh ** -0.5


def forward_o(q, kv, B, H, Nq, Nk, Dh):
    """The saved forward output as the kernels form it, on the CPU: bf16(bf16(P) V) -> bf16 [B, H, Nq, Dh]."""
    C = H * Dh
    P = torch.softmax(scores64(q, kv, B, H, Nq, Nk, Dh), -1)
    return bf(bf(P).double() @ heads(kv[:, C:].double(), B, H, Nk, Dh))


def check(got, q, kv, o, do, B, H, Nq, Nk, Dh, what, rounded=None):
    """got: {'dq' rows [B Nq, H Dh], 'dk', 'dv' rows [B Nk, H Dh]} (any device) -> worst err / tol; fails naming the output."""
    C = H * Dh
    kv = kv.cpu()
    ref, tol = kc.attn_bwd_ref(q.cpu(), kv[:, :C], kv[:, C:], o.cpu(), do.cpu(), B, H, Nq, Nk, Dh, rounds(Dh) if rounded is None else rounded)
    n = {"dq": Nq, "dk": Nk, "dv": Nk}
    return max(kc.assert_elementwise(heads(got[nm].cpu(), B, H, n[nm], Dh), ref[nm], tol[nm], "%s %s" % (what, nm)) for nm in ("dq", "dk", "dv"))


FAULTS = ("last key dropped from dq", "last query dropped from dk dv", "scale 1/8", "D not subtracted", "dO permuted", "L of the next head",
          "rows past N not masked", "stats of Nk rows")


def emulate(q, kv, o, do, B, H, Nq, Nk, Dh, rounded, fault=None):
    """The kernels' arithmetic in fp32: fp32 products, fp32 L and D, P and dS rounded to bf16 or not, bf16 outputs.
    -> {'dq' rows [B Nq, H Dh], 'dk', 'dv' rows [B Nk, H Dh]} bf16.  fault: one of FAULTS; "stats of Nk rows": L and D looked up as if the
    statistics buffer held Nk rows per head (the self-attention indexing)."""
    assert fault is None or fault in FAULTS
    C = H * Dh
    q4, k, v = heads(q.float(), B, H, Nq, Dh), heads(kv[:, :C].float(), B, H, Nk, Dh), heads(kv[:, C:].float(), B, H, Nk, Dh)
    o32 = o.float()
    g32 = do.float().reshape(B, Nq, H, Dh).permute(0, 2, 1, 3) if fault == "dO permuted" else do.float()
    sc = 0.125 if fault == "scale 1/8" else float(torch.tensor(float(Dh)).rsqrt())
    L = torch.logsumexp(q4 @ k.transpose(-1, -2) * sc, -1, keepdim=True)
    D = (g32 * o32).sum(-1, keepdim=True)
    if fault == "rows past N not masked":                   # a block of 16 rows whose rows past the end re-read the last one and are NOT given weight 0
        pad = lambda z, n: torch.cat([z, z[:, :, -1:].expand(-1, -1, 16 - n % 16, -1)], 2) if n % 16 else z
        q4, g32, L, D, k, v = pad(q4, Nq), pad(g32, Nq), pad(L, Nq), pad(D, Nq), pad(k, Nk), pad(v, Nk)
    if fault == "stats of Nk rows":
        flat = lambda z: z.reshape(-1)[(torch.arange(B * H)[:, None] * Nk + torch.arange(Nq)[None]).reshape(-1) % (B * H * Nq)].view(B, H, Nq, 1)
        L, D = flat(L), flat(D)
    if fault == "L of the next head":
        L = L.roll(1, 1)
    P = torch.exp(q4 @ k.transpose(-1, -2) * sc - L)
    dS = P * (g32 @ v.transpose(-1, -2) - (0 if fault == "D not subtracted" else D))
    if rounded:
        P, dS = bf(P).float(), bf(dS).float()
    dSq, kq = (dS[..., :-1], k[:, :, :-1]) if fault == "last key dropped from dq" else (dS, k)
    Pk, dSk, qk, gk = (P[:, :, :-1], dS[:, :, :-1], q4[:, :, :-1], g32[:, :, :-1]) if fault == "last query dropped from dk dv" else (P, dS, q4, g32)
    out = {"dq": (dSq @ kq * sc)[:, :, :Nq], "dk": (dSk.transpose(-1, -2) @ qk * sc)[:, :, :Nk], "dv": (Pk.transpose(-1, -2) @ gk)[:, :, :Nk]}
    return {nm: bf(z).permute(0, 2, 1, 3).reshape(-1, C) for nm, z in out.items()}
