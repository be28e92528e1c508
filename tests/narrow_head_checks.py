"""Helpers of test_narrow_heads_host.py and test_gpu_narrow_heads.py: the attention kernel for head dim 8 and 16 (csrc/attention_narrow.hip)
and the Score configs that use it (the reference's hybrid airplane config: hidden 128, 16 heads).  Nothing here needs a GPU to import."""
import argparse
import json
import os

import numpy as np
import torch

import kernel_checks as kc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# B, H, Nq, Nk, dh: the smallest shapes at which the narrow kernel (one wave per 16 queries, 32 keys per step) can go wrong
NARROW = [
    (2, 16, 32, 32, 8), (2, 8, 32, 32, 16),                          # the shipped shape and its 16-wide twin
    (1, 1, 1, 1, 8), (2, 3, 8, 5, 8), (2, 3, 8, 5, 16),              # one element; partial query block and key step; H dh = 24 / 48
    (3, 16, 40, 40, 8), (2, 4, 33, 65, 16),                          # one row / one key past a block edge
    (2, 2, 72, 24, 8),                                               # cross-attention with fewer keys than one step
    (1, 16, 256, 256, 8), (1, 2, 300, 77, 8),                        # the bench token count; ragged both ways
    (1, 2, 40, 600, 16), (1, 2, 40, 600, 8),                         # many key steps: the running-maximum rescale
]
# the route table of tests/test_gpu_kernel_exact.py (ATTN), restated: B, H, Nq, Nk, dh, route (0 streaming, 1 resident, 2 whole-head)
WIDE_ROUTES = [
    (2, 4, 256, 256, 64, 2), (2, 4, 256, 256, 32, 0), (3, 4, 129, 129, 64, 2), (2, 2, 129, 129, 32, 0), (2, 2, 255, 65, 64, 2), (2, 2, 255, 65, 32, 0),
    (2, 4, 300, 77, 32, 0), (2, 2, 300, 77, 64, 0), (1, 4, 2048, 256, 32, 0), (1, 2, 2048, 256, 64, 0), (2, 4, 40, 2048, 32, 0), (1, 2, 40, 256, 64, 1),
    (2, 2, 8, 5, 32, 1), (2, 2, 8, 5, 64, 1), (2, 2, 128, 512, 32, 1)]
ROUTE_NARROW = 3


def probe_fits(Nk, dh):
    """The gather probe codes a key index in min(11, dh) channels."""
    return Nk <= min(2048, 1 << dh)


def narrow_pi(Nq, Nk, salt=0):
    """Key index each query gathers: even queries walk the first and last key of every 16-key group (the kernel's MFMA width; 32-key steps are
    pairs of them) and key Nk - 1, odd ones a stride."""
    edges = sorted({e for t in range(0, Nk, 16) for e in (t, min(t + 15, Nk - 1))})
    i = torch.arange(Nq) + salt
    e = torch.tensor(edges)[(i // 2) % len(edges)]
    return torch.where(i % 2 == 0, e, (i * 37 + 11) % Nk)


def gather_probe(B, H, Nq, Nk, dh, seed):
    """kc.attention_gather_probe for heads narrower than 11 channels: the key index is coded as +1 / -1 in nb = min(11, dh) channels of each
    head (Nk <= 2^nb), Q = 160 x the code of pi(i).  A one-bit difference costs 2 * 160 / sqrt(dh) >= 40 in score (113 at dh = 8, 80 at 16), so
    every other weight is below e^-40 and O[b, h, i] == V[b, pi(i), head h] to the bit.  Head (b, h) codes j ^ m(b, h) on both sides (the
    per-head key salt): a kernel that takes k of another head gathers another key.  -> (q, k, v, want [B, H, Nq, dh], pi [B, H, Nq])."""
    nb = min(11, dh)
    assert Nk <= (1 << nb) and 2 * 160 / dh ** 0.5 >= 40
    g = torch.Generator().manual_seed(seed)
    C = H * dh
    code = lambda j: (1 - 2 * ((j[:, None] >> torch.arange(nb)[None, :]) & 1)).float()             # [n, nb] of +1 / -1
    q = torch.zeros(B, Nq, C); k = torch.zeros(B, Nk, C)
    mag = torch.exp2(torch.randint(-6, 2, (B, Nk, C), generator=g).float()) * (1 + torch.randint(0, 128, (B, Nk, C), generator=g).float() / 128)
    v = mag * (1 - 2 * torch.randint(0, 2, (B, Nk, C), generator=g)).float()
    assert torch.equal(v.bfloat16().float(), v) and float(v.abs().min()) >= 2.0 ** -6 and float(v.abs().max()) <= 4.0
    want = torch.empty(B, H, Nq, dh)
    pis = torch.empty(B, H, Nq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            pi = narrow_pi(Nq, Nk, salt=13 * (b * H + h))
            m = (5 + 3 * (b * H + h)) % (1 << (Nk.bit_length() - 1)) if Nk >= 4 else 0
            k[b, :, h * dh:h * dh + nb] = code(torch.arange(Nk) ^ m)
            q[b, :, h * dh:h * dh + nb] = 160.0 * code(pi ^ m)
            want[b, h] = v[b, pi, h * dh:(h + 1) * dh]
            pis[b, h] = pi
            s = (q[b, :, h * dh:(h + 1) * dh].double() @ k[b, :, h * dh:(h + 1) * dh].double().T) * dh ** -0.5
            top = s.gather(1, pi[:, None])
            s.scatter_(1, pi[:, None], float("-inf"))
            assert Nk == 1 or float((top - s.max(1, keepdim=True).values).min()) >= 40.0          # the construction's claim, checked
    return q, k, v, want, pis


def staircase_case(B, H, Nq, Nk, dh, step, seed, spike_query=5, spike_key=None):
    """Row maxima that grow along the keys (every 32-key step raises every query row's maximum by `step` in log2 units, as
    test_gpu_kernels.py::test_attention_softmax_staircase) and one late key that dominates one query row: the running-maximum rescale runs
    at every step, once by a large jump.  -> bf16-exact float32 q [B, Nq, C], k, v [B, Nk, C]."""
    g = torch.Generator().manual_seed(seed)
    C = H * dh
    q = torch.randn(B, Nq, C, generator=g) * 0.1; k = torch.randn(B, Nk, C, generator=g) * 0.1; v = torch.randn(B, Nk, C, generator=g)
    a = 4.0
    stair = (torch.arange(Nk) // 32).float() * step * 0.6931471805599453 * dh ** 0.5 / a
    spike_key = Nk - 30 if spike_key is None else spike_key
    for h in range(H):
        q[:, :, h * dh] = a
        k[:, :, h * dh] = stair
        q[:, spike_query, h * dh + 1] = 8.0
        k[:, spike_key, h * dh + 1] = 16.0 * dh ** 0.5                  # + 128 in score for that query alone
    r = lambda z: z.bfloat16().float()
    return r(q), r(k), r(v)


def rel_mse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / (b ** 2).sum().clamp_min(1e-300))


def digest(t):
    """float64 [sum, sum of squares, <t, cos(0.37 i)>] of a tensor (as tools/gen_score_train_golden.py)."""
    t = torch.as_tensor(t).detach().double().cpu().reshape(-1)
    return torch.stack([t.sum(), (t * t).sum(), (t * torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64))).sum()])


def digest_matches(t, want):
    """Is `t` the tensor whose digest is `want`?  Two things differ between hosts.  The float64 sums are taken in another order (threads, vector
    width): n 2^-53 of the scale below, nothing.  And the init itself is fp32 arithmetic on the seeded uniform draws (an affine map that one CPU
    code path contracts to an FMA and another does not), so an element is reproducible to one fp32 rounding, 2^-23 |t_i|, not to the bit.  Summed
    with Cauchy-Schwarz: |d sum|, |d projection| <= 2^-23 sum |t_i| <= 2^-23 sqrt(n sum t^2), |d sum of squares| <= 2^-22 sum t^2.  Another draw
    of the weights moves the sum by about sqrt(sum t^2) = that scale / sqrt(n), n <= 65536 here: four decimal digits above the bar."""
    want = want.double()
    n, S = torch.as_tensor(t).numel(), float(want[1])
    bar = torch.tensor([2.0 ** -23 * (n * S) ** 0.5, 2.0 ** -22 * S, 2.0 ** -23 * (n * S) ** 0.5], dtype=torch.float64) + 1e-300
    return bool(((digest(t) - want).abs() <= bar).all())


# ------------------------------------------------------------------------------------------------------------- configs and the golden
def _ns(d):
    ns = argparse.Namespace()
    for key, value in d.items():
        setattr(ns, key, _ns(value) if isinstance(value, dict) else value)
    return ns


def hybrid_cfg(**overrides):
    """The reference's hybrid airplane config (tests/golden/hybrid_airplane_cfg.json: its score / compressor / sde sections; the data, opt and
    common keys the classes read restated beside them) as the Namespace the classes take.  overrides: 'section.key' = value."""
    with open(os.path.join(GOLDEN, "hybrid_airplane_cfg.json")) as f:
        d = json.load(f)
    d["data"] = {"num_categorys": 1, "tr_max_sample_points": 2048, "te_max_sample_points": 2048, "batch_size": 8, "test_batch_size": 8}
    d["opt"] = {"ema_decay": 0.9999, "loss_type": "l2", "discrete": False, "pretrain_path": None, "lr": 1e-4, "warmup_iters": 1000,
                "grad_norm_clip_value": 1.0, "beta1": 0.9, "beta2": 0.999, "weight_decay": 0.0, "alpha": 0.1}
    d["common"] = {"num_points": 2048, "seed": 0}
    d["log"] = {"save_path": ""}
    for dotted, val in overrides.items():
        sect, key = dotted.split(".")
        d[sect][key] = val
    cfg = _ns(d)
    cfg.score.graphconv = False
    return cfg


CAPTURES = {   # name: (seed, heads, tokens, num_categorys, conditioned) — hidden 128, t_dim 128, 2 blocks, B = 3
    "a": (31, 16, 32, 1, False), "b": (32, 8, 40, 1, False), "c": (33, 16, 32, 1, True), "d": (34, 16, 32, 3, False)}
CAP_B = 3


def capture_score_cfg(name):
    seed, heads, tokens, ncat, _ = CAPTURES[name]
    cfg = hybrid_cfg(**{"score.num_heads": heads, "score.z_scale": tokens, "score.num_blocks": 2, "score.num_categorys": ncat})
    return cfg.score, seed


def load_golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, "score_narrow_heads.npz")).items()}


def rebuild_score(name, gold):
    """ldt_amd.Score of capture `name`, its weights drawn from the capture's seed and checked against the stored per-tensor digests."""
    import ldt_amd
    scfg, seed = capture_score_cfg(name)
    torch.manual_seed(seed)
    score = ldt_amd.Score(scfg).eval()
    sd = score.state_dict()
    keys = [k[len(name) + len("::init_digest::"):] for k in gold if k.startswith(name + "::init_digest::")]
    assert sorted(keys) == sorted(sd.keys()), "capture %s: the state_dict's tensors differ from the captured ones" % name
    for k in keys:
        assert digest_matches(sd[k], gold["%s::init_digest::%s" % (name, k)]), "capture %s: %s is not the captured init" % (name, k)
    return score, scfg


def capture_inputs(name, gold):
    """-> dict(x, t, out, label | None, pts_cond | None (B, hidden, S) channels-first, img_cond | None)."""
    get = lambda k: gold.get("%s::%s" % (name, k))
    return dict(x=get("x"), t=get("t"), out=get("out"), label=get("label"), pts_cond=get("pts_cond"), img_cond=get("img_cond"))


def oracle_forward(score, scfg, inp):
    """oracle.ldt_oracle.score_forward (fp32, CPU) on a capture's inputs."""
    from oracle import ldt_oracle as O
    import torch.nn.functional as F
    sd = {k: v.detach().float().cpu() for k, v in score.state_dict().items()}
    lab = None
    if inp["label"] is not None:
        e = sd["LabelEmbedding.label_emb.weight"][inp["label"].long()]
        lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", e)))
    cond = None
    if inp["pts_cond"] is not None:
        cond = (inp["pts_cond"].transpose(1, 2).contiguous(), inp["img_cond"])
    return O.score_forward(sd, scfg, inp["x"], inp["t"], label_emb=lab, condition=cond)
