"""Helpers of test_train_narrow_host.py, test_gpu_train_narrow_kernels.py and test_gpu_train_narrow_tape.py: the attention backward at head
widths 8, 16 and 32 (ldt_attention_bwd_narrow: csrc/attention_narrow_bwd.hip, and csrc/attention_bwd.hip instantiated at 32).

`attn_bwd_ref` is kernel_checks.attn_bwd_ref with Dh in place of 64: the same float64 reference and the same componentwise bound — the
first-product accumulation term C_ACC Dh 2^-24, the scale Dh^-0.5 — and a switch for the two forms of the second products:
    rounded=True    P and dS are rounded to bf16 before the second products (MFMA operands): the 2^-8 terms on P and dS are present.
                    The 64-wide kernel and its instantiation at 32.  At Dh = 64 this IS kernel_checks.attn_bwd_ref, bit for bit.
    rounded=False   P and dS stay fp32 (per-lane FMAs): the 2^-8 terms are absent.  The kernels for 8 and 16.
`emulate` is the kernel's arithmetic in fp32 on the CPU, with the faults the host test plants."""
import torch

import kernel_checks as kc
from kernel_checks import C_ACC, LIBM_ABS, U8, U24

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


def heads(z, B, H, N, Dh):
    """rows [B N, H Dh] -> [B, H, N, Dh]"""
    return z.reshape(B, N, H, Dh).permute(0, 2, 1, 3)


def scores64(qkv, B, H, N, Dh):
    C = H * Dh
    return heads(qkv[:, :C].double(), B, H, N, Dh) @ heads(qkv[:, C:2 * C].double(), B, H, N, Dh).transpose(-1, -2) * Dh ** -0.5


def forward_o(qkv, B, H, N, Dh):
    """The saved forward output as the kernels form it, on the CPU: bf16(bf16(P) V) -> bf16 [B, H, N, Dh]."""
    C = H * Dh
    P = torch.softmax(scores64(qkv, B, H, N, Dh), -1)
    return bf(bf(P).double() @ heads(qkv[:, 2 * C:].double(), B, H, N, Dh))


def attn_bwd_ref(qkv, o, do, B, H, N, Dh=64, rounded=True):
    """float64 from the bf16 operands: -> dict of references and of componentwise bounds, [B, H, N, Dh] each."""
    C = H * Dh
    hd = lambda z: z.double().view(B, N, H, Dh).permute(0, 2, 1, 3)
    q, k, v = hd(qkv[:, :C]), hd(qkv[:, C:2 * C]), hd(qkv[:, 2 * C:])
    o6, g6 = o.double(), do.double()
    sc = Dh ** -0.5
    s = q @ k.transpose(-1, -2) * sc
    L = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - L)
    D = (g6 * o6).sum(-1, keepdim=True)
    dP = g6 @ v.transpose(-1, -2)
    dS = P * (dP - D)
    ref = {"dq": dS @ k * sc, "dk": dS.transpose(-1, -2) @ q * sc, "dv": P.transpose(-1, -2) @ g6}
    # bound: kernel_checks.attn_bwd_ref's, term by term, with Dh for 64.  s and dP: fp32 MFMA sums of Dh terms; the exponent s - L carries
    # that of s twice + 8 x 2^-24 (|s| + |L|) + expf / logf; D: a Dh-term fp32 sum.  dS in fp32: P e_arg |dP - D| + P (e_dP + e_D) +
    # 2 x 2^-24 |dS|; rounded to bf16 (u8 = 2^-8) or kept (u8 = 0), and P likewise for dV.  Second products: C_ACC N 2^-24 |.||.| each,
    # the scale in fp32 (dq, dk), and the bf16 output 2^-8 |ref|.
    u8 = U8 if rounded else 0.0
    acc = C_ACC * Dh * U24
    e_arg = 2 * acc * (q.abs() @ k.abs().transpose(-1, -2)) * sc + 8 * U24 * (s.abs() + L.abs()) + 4 * LIBM_ABS
    e_dP = acc * (g6.abs() @ v.abs().transpose(-1, -2))
    e_D = acc * (g6.abs() * o6.abs()).sum(-1, keepdim=True)
    e_dS = P * e_arg * (dP - D).abs() + P * (e_dP + e_D) + (2 * U24 + u8) * dS.abs()
    e_P = P * e_arg + u8 * P
    acc2 = C_ACC * N * U24
    tol = {"dq": sc * (e_dS @ k.abs() + acc2 * (dS.abs() @ k.abs())) + (U8 + 2 * U24) * ref["dq"].abs(),
           "dk": sc * (e_dS.transpose(-1, -2) @ q.abs() + acc2 * (dS.abs().transpose(-1, -2) @ q.abs())) + (U8 + 2 * U24) * ref["dk"].abs(),
           "dv": e_P.transpose(-1, -2) @ g6.abs() + acc2 * (P.transpose(-1, -2) @ g6.abs()) + (U8 + U24) * ref["dv"].abs()}
    return ref, tol


def check(got, qkv, o, do, B, H, N, Dh, what, rounded=None):
    """got: {'dq', 'dk', 'dv'} as rows [B N, H Dh] (any device) -> worst err / tol; fails naming the output."""
    ref, tol = attn_bwd_ref(qkv.cpu(), o.cpu(), do.cpu(), B, H, N, Dh, rounds(Dh) if rounded is None else rounded)
    return max(kc.assert_elementwise(heads(got[nm].cpu(), B, H, N, Dh), ref[nm], tol[nm], "%s %s" % (what, nm)) for nm in ("dq", "dk", "dv"))


FAULTS = ("last key dropped from dq", "last query dropped from dk dv", "scale 1/8", "D not subtracted", "dO permuted", "L of the next head",
          "rows past N not masked")


def emulate(qkv, o, do, B, H, N, Dh, rounded, fault=None):
    """The kernels' arithmetic in fp32: fp32 products, fp32 L and D, P and dS rounded to bf16 or not, bf16 outputs.
    -> {'dq', 'dk', 'dv'} bf16 rows [B N, H Dh].  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    C = H * Dh
    hd = lambda z: z.float().view(B, N, H, Dh).permute(0, 2, 1, 3)
    q, k, v = hd(qkv[:, :C]), hd(qkv[:, C:2 * C]), hd(qkv[:, 2 * C:])
    o32 = o.float()
    g32 = do.float().reshape(B, N, H, Dh).permute(0, 2, 1, 3) if fault == "dO permuted" else do.float()
    sc = 0.125 if fault == "scale 1/8" else float(torch.tensor(float(Dh)).rsqrt())
    if fault == "rows past N not masked":                   # a block of 16 rows whose rows >= N re-read the last one and are NOT given weight 0
        pad = lambda z: torch.cat([z, z[:, :, -1:].expand(-1, -1, 16 - N % 16, -1)], 2) if N % 16 else z
        L = torch.logsumexp(q @ k.transpose(-1, -2) * sc, -1, keepdim=True)
        D = (g32 * o32).sum(-1, keepdim=True)
        q, k, v, g32, L, D = pad(q), pad(k), pad(v), pad(g32), pad(L), pad(D)
        s = q @ k.transpose(-1, -2) * sc
    else:
        s = q @ k.transpose(-1, -2) * sc
        L = torch.logsumexp(s, -1, keepdim=True)
        D = (g32 * o32).sum(-1, keepdim=True)
    if fault == "L of the next head":
        L = L.roll(1, 1)
    P = torch.exp(s - L)
    dS = P * (g32 @ v.transpose(-1, -2) - (0 if fault == "D not subtracted" else D))
    if rounded:
        P, dS = bf(P).float(), bf(dS).float()
    dSq, kq = (dS[..., :-1], k[:, :, :-1]) if fault == "last key dropped from dq" else (dS, k)
    Pk, dSk, qk, gk = (P[:, :, :-1], dS[:, :, :-1], q[:, :, :-1], g32[:, :, :-1]) if fault == "last query dropped from dk dv" else (P, dS, q, g32)
    out = {"dq": dSq @ kq * sc, "dk": dSk.transpose(-1, -2) @ qk * sc, "dv": Pk.transpose(-1, -2) @ gk}
    return {nm: bf(z[:, :, :N]).permute(0, 2, 1, 3).reshape(B * N, C) for nm, z in out.items()}
