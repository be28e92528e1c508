"""Helpers of the decoder-training kernel tests (test_decoder_train_host.py, test_gpu_cd_loss.py, test_gpu_attention_bwd_long.py,
test_gpu_rows_gather_sum.py): float64 references with componentwise bounds, and fp32 emulations of the kernels' arithmetic with the
faults the host test plants.  Bounds are built like kernel_checks.gemm_tol: accumulation C_ACC n 2^-24 sum |terms|, 2^-8 per bf16-rounded
intermediate, the output rounding; none of them is taken from what a kernel returned.

Chamfer (csrc/chamfer_loss.hip)
  * an index is checked to be a valid argmin before it is used: d64[idx] <= min d64 + 2 x the distance bound of kernel_checks.chamfer_dir_ref
    (the kernel's own distance is within one bound of d64[idx], and within one bound of the true minimum).  No element is left out.
  * the gradient reference is teacher-forced on the kernel's indices, so a near tie is never a false failure.  Per term the kernel rounds:
    the difference (1), the squared length (two more on the differences' account, three of its own, halved by the root), the root (1), the
    quotient (1), the constant upstream / (B n) (1), and the fused multiply-add into the sum (1): under GRAD_ROUNDINGS = 8 relative to the
    term; each of the k additions into a point's sum rounds at most the sum of the magnitudes: (GRAD_ROUNDINGS + k) 2^-24 sum |terms|.
Attention backward on a long query axis (csrc/attention_bwd.hip, ldt_attention_bwd_long)
  * kernel_checks.attn_bwd_ref at head width 32 with P and dS rounded, plus, on dK and dV, the one fp32 sum of ceil(Nq / chunk) partials:
    (chunks - 1) 2^-24 times the sum of the partials' magnitudes, itself at most |dS|^T |q| (P^T |dO|)."""
import torch

import kernel_checks as kc
from kernel_checks import CHAMFER_ROUNDINGS, SLACK, U24, attn_bwd_ref, chamfer_dir_ref

assert CHAMFER_ROUNDINGS == 9
GRAD_ROUNDINGS = 8
CHUNK = 256                        # LDT_ATTN_BWD_LONG_CHUNK
LOSS_REL = 2 * U24                 # the loss against float64 of the same distances: fp64 sums, one rounding of each term and of the total

# (B, n, m): estimated points, target points
CD_SHAPES = [(2, 72, 200), (1, 64, 64), (3, 1, 5), (1, 300, 1)]
# (B, H, Nq, Nk) at head width 32
LONG_SHAPES = [(1, 2, 16, 8), (2, 2, 296, 32), (1, 4, 552, 72), (1, 1, 2048, 32)]


def cd_case(B, n, m, seed=None):
    g = torch.Generator().manual_seed(1000 * B + 10 * n + m if seed is None else seed)
    return torch.randn(B, n, 3, generator=g), torch.randn(B, m, 3, generator=g) * 1.1 + 0.05


# ---- pure-torch Chamfer (the reference's chamfer_python.distChamfer restated: all pairs, min both ways) and CD_loss, for autograd
def dist_chamfer_torch(a, b):
    """a [B, n, 3], b [B, m, 3] -> (d1 [B, n], d2 [B, m], idx1, idx2) by explicit differences."""
    P = (a[:, :, None, :] - b[:, None, :, :]).pow(2).sum(-1)
    d1, i1 = P.min(2)
    d2, i2 = P.min(1)
    return d1, d2, i1, i2


def cd_loss_torch(esti, shapes, type):
    d1, d2, _, _ = dist_chamfer_torch(esti, shapes)
    return (d1.sqrt().mean() + d2.sqrt().mean()) if type == "l1" else (d1.mean() + d2.mean())


def cd_loss_ref(d1, d2, type):
    """float64 (loss, term1, term2) of the given distances (negative ones, which the expanded form can round to, count as 0 under the root)."""
    a, b = d1.double().reshape(-1), d2.double().reshape(-1)
    t = (a.clamp_min(0).sqrt().mean(), b.clamp_min(0).sqrt().mean()) if type == "l1" else (a.mean(), b.mean())
    return torch.stack([t[0] + t[1], t[0], t[1]])


def assert_valid_argmin(q, r, idx, what):
    """idx [B, nq] (any integer dtype) points, for every query, at a reference point whose float64 distance is within 2 bounds of the minimum."""
    B, nq, nr = q.shape[0], q.shape[1], r.shape[1]
    idx = idx.cpu().long()
    assert tuple(idx.shape) == (B, nq) and int(idx.min()) >= 0 and int(idx.max()) < nr, "%s: an index outside its cloud" % what
    dmin, tol = chamfer_dir_ref(q.cpu(), r.cpu())
    at = (q.cpu().double() - torch.gather(r.cpu().double(), 1, idx[..., None].expand(B, nq, 3))).pow(2).sum(-1)
    bad = ~(at <= dmin + 2 * tol)
    assert not bool(bad.any()), "%s: %d of %d indices are no argmin (worst excess %.3g)" % (what, int(bad.sum()), bad.numel(), float((at - dmin).max()))


CD_FAULTS = ("scattered term dropped", "1 / (B n) of the wrong direction", "idx1 used for the gather", "coincident pair poisons")


def _pair_terms(x1, x2, i_of, j_of, c, l1, dt):
    """terms [B, k, 3] = w (x1[i] - x2[j]) c, w = 1 / |.| (l1; 0 at distance 0) or 2, in dtype dt, and their magnitudes"""
    B = x1.shape[0]
    p = torch.gather(x1.to(dt), 1, i_of[..., None].expand(B, i_of.shape[1], 3))
    r = torch.gather(x2.to(dt), 1, j_of[..., None].expand(B, j_of.shape[1], 3))
    d = p - r
    dd = d.pow(2).sum(-1, keepdim=True)
    if l1:
        w = torch.where(dd == 0, torch.zeros_like(dd), 1.0 / dd.sqrt())
    else:
        w = torch.full_like(dd, 2.0)
    return w * d * c


def cd_grad(x1, x2, idx1, idx2, type, upstream=1.0, dt=torch.float64, fault=None):
    """upstream d CD_loss / d x1 given the nearest-neighbour indices (idx1 [B, n] into x2, idx2 [B, m] into x1).
    dt float64: -> (reference [B, n, 3], bound).  dt float32: the kernel's arithmetic in fp32, with one of CD_FAULTS planted -> the gradient alone."""
    assert fault is None or fault in CD_FAULTS
    x1, x2, idx1, idx2 = x1.cpu(), x2.cpu(), idx1.cpu().long(), idx2.cpu().long()
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    l1 = type == "l1"
    c1, c2 = float(upstream) / (B * n), float(upstream) / (B * m)
    if fault == "1 / (B n) of the wrong direction":
        c1, c2 = c2, c1
    ar_n, ar_m = torch.arange(n).expand(B, n), torch.arange(m).expand(B, m)
    t1 = _pair_terms(x1, x2, ar_n, idx1, c1, l1, dt)                    # point i with its own nearest target
    gi, gj = (idx1[:, :min(n, m)] % n, ar_m[:, :min(n, m)]) if fault == "idx1 used for the gather" else (idx2, ar_m)
    t2 = _pair_terms(x1, x2, gi, gj, c2, l1, dt)                        # target j with its nearest point idx2[j]
    if fault == "scattered term dropped":
        t2 = torch.zeros_like(t2)
    if fault == "coincident pair poisons":                             # the reference's inf * 0
        hit = (torch.gather(x1, 1, idx2[..., None].expand(B, m, 3)) == x2).all(-1)
        t2 = torch.where(hit[..., None], torch.full_like(t2, float("nan")), t2)
    out = t1.clone().scatter_add_(1, gi[..., None].expand_as(t2), t2)
    if dt != torch.float64:
        return out
    mag = t1.abs().scatter_add_(1, gi[..., None].expand_as(t2), t2.abs())
    k = 1 + torch.zeros(B, n, dtype=dt).scatter_add_(1, gi, torch.ones(B, gi.shape[1], dtype=dt))
    return out, (GRAD_ROUNDINGS + k)[..., None] * U24 * mag * SLACK


# ---- attention backward on a long query axis
def long_case(B, H, Nq, Nk, seed=None):
    """-> (q bf16 [B Nq, 128-or-H*32], kv bf16 [B Nk, 2 H 32] = K | V, dO bf16 [B, H, Nq, 32])"""
    import cross_bwd_checks as cb
    return cb.cross_case(B, H, Nq, Nk, 32, False, seed)


def long_ref(q, kv, o, do, B, H, Nq, Nk, chunk=CHUNK):
    """-> (references, bounds) of dq [B, H, Nq, 32], dk, dv [B, H, Nk, 32]: attn_bwd_ref with the partial-sum term added to dk and dv."""
    Dh, C = 32, H * 32
    q, kv, o, do = q.cpu(), kv.cpu(), o.cpu(), do.cpu()
    ref, tol = attn_bwd_ref(q, kv[:, :C], kv[:, C:], o, do, B, H, Nq, Nk, Dh, True)
    chunks = -(-Nq // chunk)
    if chunks > 1:
        q4, k4, v4 = kc.heads(q, B, Nq, H, Dh), kc.heads(kv[:, :C], B, Nk, H, Dh), kc.heads(kv[:, C:], B, Nk, H, Dh)
        o6, g6, sc = o.double(), do.double(), Dh ** -0.5
        P = torch.softmax(q4 @ k4.transpose(-1, -2) * sc, -1)
        dS = P * (g6 @ v4.transpose(-1, -2) - (g6 * o6).sum(-1, keepdim=True))
        tol = dict(tol)
        tol["dk"] = tol["dk"] + (chunks - 1) * U24 * sc * (dS.abs().transpose(-1, -2) @ q4.abs())
        tol["dv"] = tol["dv"] + (chunks - 1) * U24 * (P.transpose(-1, -2) @ g6.abs())
    return ref, tol


def long_check(got, q, kv, o, do, B, H, Nq, Nk, what):
    """got: {'dq' rows [B Nq, H 32], 'dk', 'dv' rows [B Nk, H 32]} -> {name: worst err / tol}; fails naming the output."""
    import narrow_bwd_checks as nb
    ref, tol = long_ref(q, kv, o, do, B, H, Nq, Nk)
    n = {"dq": Nq, "dk": Nk, "dv": Nk}
    return {nm: kc.assert_elementwise(nb.heads(got[nm].cpu(), B, H, n[nm], 32), ref[nm], tol[nm], "%s %s" % (what, nm)) for nm in ("dq", "dk", "dv")}


LONG_FAULTS = ("a chunk's partial dropped from dk", "partials added unscaled", "last chunk reads the first chunk's queries")


def long_emulate(q, kv, o, do, B, H, Nq, Nk, chunk=CHUNK, fault=None):
    """The kernels' arithmetic in fp32 with dK / dV summed per chunk of queries and the partials added in chunk order -> bf16 rows like
    narrow_bwd_checks.emulate."""
    import narrow_bwd_checks as nb
    assert fault is None or fault in LONG_FAULTS
    Dh, C = 32, H * 32
    bf = nb.bf
    q4, k, v = nb.heads(q.float(), B, H, Nq, Dh), nb.heads(kv[:, :C].float(), B, H, Nk, Dh), nb.heads(kv[:, C:].float(), B, H, Nk, Dh)
    g32, o32 = do.float(), o.float()
    sc = float(torch.tensor(float(Dh)).rsqrt())
    s = q4 @ k.transpose(-1, -2) * sc
    P = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    dS = P * (g32 @ v.transpose(-1, -2) - (g32 * o32).sum(-1, keepdim=True))
    P, dS = bf(P).float(), bf(dS).float()
    dk, dv = torch.zeros(B, H, Nk, Dh), torch.zeros(B, H, Nk, Dh)
    chunks = -(-Nq // chunk)
    for c in range(chunks):
        lo, hi = c * chunk, min((c + 1) * chunk, Nq)
        qs = slice(0, hi - lo) if (fault == "last chunk reads the first chunk's queries" and c == chunks - 1 and c > 0) else slice(lo, hi)
        if not (fault == "a chunk's partial dropped from dk" and c == chunks // 2):
            dk = dk + dS[:, :, lo:hi].transpose(-1, -2) @ q4[:, :, qs]
        dv = dv + P[:, :, lo:hi].transpose(-1, -2) @ g32[:, :, lo:hi]
    out = {"dq": dS @ k * sc, "dk": dk * (1.0 if fault == "partials added unscaled" else sc), "dv": dv}
    return {nm: bf(z).permute(0, 2, 1, 3).reshape(-1, C) for nm, z in out.items()}


# ---- prior rows
def rows_gather_sum_ref(dy, src, N):
    """dy [B N, C], src [B, R] -> (float64 [R, C], bound): a sum of k terms in the order of b rounds k - 1 times, each at most the sum of magnitudes."""
    B, R = src.shape
    d3 = dy.cpu().double().view(B, N, -1)
    s = src.cpu().long()
    have = (s >= 0)[..., None]
    rows = torch.gather(d3, 1, s.clamp_min(0)[..., None].expand(B, R, d3.shape[2]))
    rows = torch.where(have, rows, torch.zeros_like(rows))
    k = have.sum(0).double()
    return rows.sum(0), (k - 1).clamp_min(0) * U24 * rows.abs().sum(0) * SLACK


def rows_gather_sum_emulate(dy, src, N, fault=None):
    """fp32, in the order of b.  fault 'wrong sample set': the rows of the samples that do NOT hold the row are summed."""
    B, R = src.shape
    d3 = dy.cpu().float().view(B, N, -1)
    out = torch.zeros(R, d3.shape[2])
    for b in range(B):
        s = src[b].cpu().long()
        have = (s >= 0) if fault is None else (s < 0)
        out = out + torch.where(have[:, None], d3[b][s.clamp_min(0)], torch.zeros(R, d3.shape[2]))
    return out
