"""Helpers of test_train_cond_host.py and test_gpu_train_cond_kernels.py: the cross-attention backward (ldt_attention_bwd_cross:
csrc/attention_bwd.hip) with Nq queries and Nk keys: the shapes, the operands and the exact probe on dV.  The reference and bound
(kernel_checks.attn_bwd_ref, which takes the two lengths apart: dQ sums over the Nk keys, dK and dV over the Nq queries), `check`, the
CPU forward and the fp32 emulation with its planted faults are the ones of the self-attention tests (tests/narrow_bwd_checks.py)."""
import torch

from narrow_bwd_checks import bf

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
