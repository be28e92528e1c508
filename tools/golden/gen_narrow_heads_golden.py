"""TEST INFRASTRUCTURE ONLY — writes tests/golden/score_narrow_heads.npz: the reference's `Score.forward` with 8- and 16-wide heads, on the CPU.

Runs only where the upstream reference can be imported (through oracle/ref_import.py); the fixture is data, the reference does not travel.

The Score of the reference's hybrid airplane config (tests/golden/hybrid_airplane_cfg.json: hidden 128, t_dim 128, z 120) cut to 2 blocks,
B = 3, four captures (tests/narrow_head_checks.py: CAPTURES):

    a   16 heads (head dim 8), 32 tokens
    b    8 heads (head dim 16), 40 tokens
    c   16 heads, 32 tokens, condition = (pts_cond (3, 128, 24), img_cond (3, 128)): cross-attention on block 0, the image row added to c
    d   16 heads, num_categorys = 3, labels

Stored per capture `n`: `n::init_digest::<tensor>` (digest of every tensor of the initial state_dict: the weights are
`torch.manual_seed(seed); Score(cfg)`, which ldt_amd.Score draws bit for bit — asserted here — so the tests rebuild them from the seed; one copy
is 2.7 MB and a committed file may hold 1 MiB), `n::x`, `n::t`, `n::out` and, where present, `n::label`, `n::pts_cond`, `n::img_cond`.

Asserted at capture: ldt_amd.Score's init equals upstream's, and oracle.ldt_oracle.score_forward in fp32 reproduces every output to
<= 1e-10 rel-MSE.

    python tools/golden/gen_narrow_heads_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_import as R  # noqa: E402
import narrow_head_checks as nh  # noqa: E402


def main():
    R.setup()
    from model.scorenet.score import Score
    import ldt_amd
    torch.set_grad_enabled(False)
    out = {}
    for name, (seed, heads, tokens, ncat, conditioned) in nh.CAPTURES.items():
        scfg, _ = nh.capture_score_cfg(name)
        assert scfg.hidden_size == 128 and scfg.t_dim == 128 and scfg.num_heads == heads and scfg.z_scale == tokens
        torch.manual_seed(seed)
        ref = Score(scfg).eval()
        init = {k: v.clone() for k, v in ref.state_dict().items()}
        torch.manual_seed(seed)
        ours = ldt_amd.Score(scfg).eval()
        osd = ours.state_dict()
        assert osd.keys() == init.keys() and all(torch.equal(osd[k], init[k]) for k in init), "ldt_amd.Score's default init differs from upstream's"
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randn(nh.CAP_B, tokens, scfg.z_dim, generator=g)
        t = torch.rand(nh.CAP_B, generator=g) * 0.9 + 0.05
        label = torch.tensor([2, 0, 1]) if ncat > 1 else None
        cond = None
        if conditioned:
            cond = (torch.randn(nh.CAP_B, scfg.hidden_size, 24, generator=g), torch.randn(nh.CAP_B, scfg.t_dim, generator=g) * 0.5)
        y = ref(x, t, label=label, condition=cond)
        assert y.shape == x.shape and bool(torch.isfinite(y).all())
        inp = dict(x=x, t=t, out=y, label=label, pts_cond=None if cond is None else cond[0], img_cond=None if cond is None else cond[1])
        e = nh.rel_mse(nh.oracle_forward(ours, scfg, inp), y)
        print("capture %s: %2d heads, %d tokens: fp32 oracle vs the reference rel-MSE %.3e, out rms %.4f" % (name, heads, tokens, e, float(y.pow(2).mean().sqrt())))
        assert e <= 1e-10, "the oracle does not reproduce the reference's Score.forward"
        out.update({"%s::init_digest::%s" % (name, k): nh.digest(v) for k, v in init.items()})
        out.update({"%s::%s" % (name, k): v for k, v in inp.items() if v is not None})
    path = os.path.join(nh.GOLDEN, "score_narrow_heads.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
