"""Helpers of test_train_cond_host.py and test_gpu_train_cond_kernels.py: the cross-attention backward (ldt_attention_bwd_cross:
csrc/attention_bwd.hip at head widths 32 and 64, csrc/attention_narrow_bwd.hip at 8 and 16) with Nq queries and Nk keys.

`attn_bwd_cross_ref` is kernel_checks.attn_bwd_ref — through narrow_bwd_checks.attn_bwd_ref, its form with the head width as a parameter —
with the two lengths apart: the same float64 reference, the same componentwise bound term by term, built from kernel_checks' own
constants.  The one place where N enters the bound is the accumulation term of the second products, C_ACC N 2^-24: dQ sums over the Nk
keys, dK and dV over the Nq queries.  At Nq = Nk it IS narrow_bwd_checks.attn_bwd_ref (and at 64 kernel_checks.attn_bwd_ref), bit for
bit: test_train_cond_host.py asserts that, so the bound can be neither restated differently nor loosened here."""
import torch

import kernel_checks as kc
import narrow_bwd_checks as nb
from kernel_checks import C_ACC, LIBM_ABS, U8, U24

# (B, H, Nq, Nk, Dh)
SHAPES = [
    (2, 2, 8, 24, 64),       # one partial query block, partial 32-column step
    (1, 2, 72, 40, 64),      # Nq > Nk
    (1, 1, 40, 72, 32),      # Nq < Nk
    (2, 3, 33, 17, 16),      # ragged on both axes
    (1, 2, 17, 33, 8),
    (1, 1, 1, 1, 64),        # one key
    (1, 2, 16, 1, 8),
    (1, 1, 256, 32, 64),     # the configs[4] key count under the headline query count
]
LARGE = [(1, 2, 72, 40, 64), (2, 3, 33, 17, 16)]          # one logit per row far above the others: the recomputed row maximum is needed
CASES = [s + (False,) for s in SHAPES] + [s + (True,) for s in LARGE]
SQUARE = [(2, 2, 40, 64), (2, 4, 33, 32), (1, 2, 72, 16), (2, 3, 24, 8)]      # (B, H, N, Dh): against ops.attention_bwd, bit for bit
PROBES = [(2, 2, 24, 40, 64), (1, 1, 40, 72, 32), (2, 3, 17, 33, 16), (1, 2, 17, 33, 8), (1, 2, 16, 16, 8)]   # Nq <= Nk: a key per query


def bf(t):
    return t.to(torch.bfloat16)


def heads(z, B, H, N, Dh):
    """rows [B N, H Dh] -> [B, H, N, Dh]"""
    return z.reshape(B, N, H, Dh).permute(0, 2, 1, 3)


def cross_case(B, H, Nq, Nk, Dh, large=False, seed=None):
    """-> (q bf16 [B Nq, H Dh], kv bf16 [B Nk, 2 H Dh] = K | V, dO bf16 [B, H, Nq, Dh]).  large: q += (96 / sqrt(Dh)) k[(7 i + 3) % Nk],
    one logit per row ~96 (narrow_bwd_checks.attn_case's rule with the key index taken modulo Nk)."""
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 7 * Nq + Nk + Dh + int(large) if seed is None else seed)
    C = H * Dh
    q = torch.randn(B * Nq, C, generator=g)
    kv = torch.randn(B * Nk, 2 * C, generator=g)
    if large:
        k4 = kv[:, :C].view(B, Nk, H, Dh)
        q.view(B, Nq, H, Dh).add_((96.0 / Dh ** 0.5) * k4[:, (7 * torch.arange(Nq) + 3) % Nk])
    return bf(q), bf(kv), bf(torch.randn(B, H, Nq, Dh, generator=g))


def scores64(q, kv, B, H, Nq, Nk, Dh):
    C = H * Dh
    return heads(q.double(), B, H, Nq, Dh) @ heads(kv[:, :C].double(), B, H, Nk, Dh).transpose(-1, -2) * Dh ** -0.5


def forward_o(q, kv, B, H, Nq, Nk, Dh):
    """The saved forward output as the kernels form it, on the CPU: bf16(bf16(P) V) -> bf16 [B, H, Nq, Dh]."""
    C = H * Dh
    P = torch.softmax(scores64(q, kv, B, H, Nq, Nk, Dh), -1)
    return bf(bf(P).double() @ heads(kv[:, C:].double(), B, H, Nk, Dh))


def attn_bwd_cross_ref(q, kv, o, do, B, H, Nq, Nk, Dh, rounded):
    """float64 from the bf16 operands -> (references, componentwise bounds): dq [B, H, Nq, Dh]; dk, dv [B, H, Nk, Dh].
    narrow_bwd_checks.attn_bwd_ref line for line; N -> Nk in dq's second product, N -> Nq in dk's and dv's."""
    C = H * Dh
    q, k, v = heads(q.double(), B, H, Nq, Dh), heads(kv[:, :C].double(), B, H, Nk, Dh), heads(kv[:, C:].double(), B, H, Nk, Dh)
    o6, g6 = o.double(), do.double()
    sc = Dh ** -0.5
    s = q @ k.transpose(-1, -2) * sc
    L = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - L)
    D = (g6 * o6).sum(-1, keepdim=True)
    dP = g6 @ v.transpose(-1, -2)
    dS = P * (dP - D)
    ref = {"dq": dS @ k * sc, "dk": dS.transpose(-1, -2) @ q * sc, "dv": P.transpose(-1, -2) @ g6}
    u8 = U8 if rounded else 0.0
    acc = C_ACC * Dh * U24
    e_arg = 2 * acc * (q.abs() @ k.abs().transpose(-1, -2)) * sc + 8 * U24 * (s.abs() + L.abs()) + 4 * LIBM_ABS
    e_dP = acc * (g6.abs() @ v.abs().transpose(-1, -2))
    e_D = acc * (g6.abs() * o6.abs()).sum(-1, keepdim=True)
    e_dS = P * e_arg * (dP - D).abs() + P * (e_dP + e_D) + (2 * U24 + u8) * dS.abs()
    e_P = P * e_arg + u8 * P
    acc_k, acc_q = C_ACC * Nk * U24, C_ACC * Nq * U24              # second products: dq sums over the keys, dk and dv over the queries
    tol = {"dq": sc * (e_dS @ k.abs() + acc_k * (dS.abs() @ k.abs())) + (U8 + 2 * U24) * ref["dq"].abs(),
           "dk": sc * (e_dS.transpose(-1, -2) @ q.abs() + acc_q * (dS.abs().transpose(-1, -2) @ q.abs())) + (U8 + 2 * U24) * ref["dk"].abs(),
           "dv": e_P.transpose(-1, -2) @ g6.abs() + acc_q * (P.transpose(-1, -2) @ g6.abs()) + (U8 + U24) * ref["dv"].abs()}
    return ref, tol


def check(got, q, kv, o, do, B, H, Nq, Nk, Dh, what, rounded=None):
    """got: {'dq' rows [B Nq, H Dh], 'dk', 'dv' rows [B Nk, H Dh]} (any device) -> worst err / tol; fails naming the output."""
    ref, tol = attn_bwd_cross_ref(q.cpu(), kv.cpu(), o.cpu(), do.cpu(), B, H, Nq, Nk, Dh, nb.rounds(Dh) if rounded is None else rounded)
    n = {"dq": Nq, "dk": Nk, "dv": Nk}
    return max(kc.assert_elementwise(heads(got[nm].cpu(), B, H, n[nm], Dh), ref[nm], tol[nm], "%s %s" % (what, nm)) for nm in ("dq", "dk", "dv"))


FAULTS = ("last key dropped from dq", "last query dropped from dk dv", "stats of Nk rows", "D not subtracted")


def emulate(q, kv, o, do, B, H, Nq, Nk, Dh, rounded, fault=None):
    """The kernels' arithmetic in fp32 (narrow_bwd_checks.emulate with two lengths) -> {'dq', 'dk', 'dv'} bf16 rows.  fault: one of FAULTS;
    "stats of Nk rows": L and D looked up as if the statistics buffer held Nk rows per head (the self-attention indexing)."""
    assert fault is None or fault in FAULTS
    C = H * Dh
    q4, k, v = heads(q.float(), B, H, Nq, Dh), heads(kv[:, :C].float(), B, H, Nk, Dh), heads(kv[:, C:].float(), B, H, Nk, Dh)
    o32, g32 = o.float(), do.float()
    sc = float(torch.tensor(float(Dh)).rsqrt())
    s = q4 @ k.transpose(-1, -2) * sc
    L = torch.logsumexp(s, -1, keepdim=True)
    D = (g32 * o32).sum(-1, keepdim=True)
    if fault == "stats of Nk rows":
        flat = lambda z: z.reshape(-1)[(torch.arange(B * H)[:, None] * Nk + torch.arange(Nq)[None]).reshape(-1) % (B * H * Nq)].view(B, H, Nq, 1)
        L, D = flat(L), flat(D)
    P = torch.exp(s - L)
    dS = P * (g32 @ v.transpose(-1, -2) - (0 if fault == "D not subtracted" else D))
    if rounded:
        P, dS = bf(P).float(), bf(dS).float()
    dSq, kq = (dS[..., :-1], k[:, :, :-1]) if fault == "last key dropped from dq" else (dS, k)
    Pk, dSk, qk, gk = (P[:, :, :-1], dS[:, :, :-1], q4[:, :, :-1], g32[:, :, :-1]) if fault == "last query dropped from dk dv" else (P, dS, q4, g32)
    out = {"dq": dSq @ kq * sc, "dk": dSk.transpose(-1, -2) @ qk * sc, "dv": Pk.transpose(-1, -2) @ gk}
    return {nm: bf(z).permute(0, 2, 1, 3).reshape(-1, C) for nm, z in out.items()}


# ---- the exact probe on dV
def selection_probe(B, H, Nq, Nk, Dh, seed):
    """Logits in which query i of every (sample, head) selects key pi(i) alone, pi injective (Nq <= Nk): K rows are distinct +-1 sign
    vectors (the bits of the key's index in the first 8 channels, +1 elsewhere), q_i = A k_pi(i) with A a power of two.  Every product
    is +-A and every logit an exact multiple of A in fp32: the winner's is A Dh, every other at most A (Dh - 2), a lead of
    2 A Dh^-0.5 >= 128 after scaling — exp of minus that is 0 in fp32, so the row sum is exactly 1, L is the maximum, and P is exactly the
    one-hot matrix.  Then dV[pi(i)] = dO[i] and dV of an unselected key is 0, bit for bit.
    -> (q, kv, dO, pi [B, H, Nq] (long), lead)"""
    assert Nq <= Nk <= 256 and Dh >= 8
    g = torch.Generator().manual_seed(seed)
    C = H * Dh
    A = 256.0 if Dh in (8, 16) else 512.0
    lead = 2 * A * Dh ** -0.5
    assert lead >= 110
    bits = ((torch.arange(Nk)[:, None] >> torch.arange(8)[None]) & 1).float() * 2 - 1        # [Nk, 8]
    signs = torch.ones(Nk, Dh)
    signs[:, :8] = bits
    pi = torch.stack([torch.randperm(Nk, generator=g)[:Nq] for _ in range(B * H)]).view(B, H, Nq)
    k4 = signs[None, :, None, :].expand(B, Nk, H, Dh)                                         # the same code book in every head
    q4 = A * signs[pi.permute(0, 2, 1)]                                                       # [B, Nq, H, Dh]
    kv = torch.cat([k4.reshape(B * Nk, C), torch.randn(B * Nk, C, generator=g)], 1)
    return bf(q4.reshape(B * Nq, C)), bf(kv), bf(torch.randn(B, H, Nq, Dh, generator=g)), pi, lead


def selection_expected_dv(do, pi, B, H, Nq, Nk, Dh):
    """dV rows [B Nk, H Dh]: row pi(i) of head h = dO[b, h, i]; unselected keys exactly 0."""
    want = torch.zeros(B, H, Nk, Dh, dtype=do.dtype)
    want.scatter_(2, pi[..., None].expand(B, H, Nq, Dh), do.cpu())
    return want.permute(0, 2, 1, 3).reshape(B * Nk, H * Dh)
