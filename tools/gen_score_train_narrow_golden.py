"""TEST INFRASTRUCTURE ONLY — writes tests/golden/score_train_narrow.npz: the reference's own Score training step at head widths 8, 16 and
32, captured on the CPU.  Runs only where the upstream reference is present.

It is tools/gen_score_train_golden.py's `run` (the same seeds, draws, spy on clip_grad_norm_, fp32-oracle assertion and bf16 twin) under
other Score sizes; that tool and what it writes are unchanged.  The tiny config with Score hidden 128, t_dim 128, 2 blocks, z = 120,
B = 8 fixed latents, lr 2e-3, warm-up 5, EMA 0.98, clip 1.0, discrete, l2 (tests/train_narrow_checks.py: MODELS holds the overrides, so
that the tests rebuild the very configs):

    a_*   16 heads x 8, T = 32 — the hybrid config's head layout and token count.  The full record of score_train_tiny: 20 iterations of
          `Trainer.update_score(eps, discrete=True)` (idx, loss), init / iteration-0 gradient digests, the tensors of at most 1024 elements
          verbatim (gradient, weights and EMA after iterations 1 and 20, exp_avg after iteration 1), the optimizer state's layout, the bf16
          twin's yardsticks (twin_grad_relmse::*, twin_grad_relmse_all, twin_loss_dev, twin_after20_update_relmse, twin_ema20_update_relmse)
    b_*   8 heads x 16, T = 40, num_categorys 3 with labels: one iteration (digests, idx, loss, cates, the twin's gradient yardsticks)
    c_*   4 heads x 32, T = 24: one iteration

The latents are `torch.randn(8, T, 120, generator=manual_seed(77)) * 0.5` as in that tool: stored for (a) (by `run`), by digest for (b) and
(c), whose tests draw them again.

    python tools/gen_score_train_narrow_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_score_train_golden as G  # noqa: E402
import train_narrow_checks as tn  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from oracle.gen_golden import save  # noqa: E402


def run_model(key, out):
    m = tn.MODELS[key]
    base = G.train_cfg

    def cfg_with_overrides(num_categorys=1):
        return tn.apply_overrides(base(num_categorys), key)

    G.train_cfg = cfg_with_overrides
    try:
        mine = {}
        # (a): tag "" makes `run` keep the whole 20-step record; (b), (c): one iteration under a tag, as its labelled model
        G.run(m["num_categorys"], m["iters"], mine, tag="" if m["iters"] > 1 else "x_")
    finally:
        G.train_cfg = base
    for k, v in mine.items():
        out[key + "_" + (k[2:] if k.startswith("x_") else k)] = v
    if key + "_eps" not in out:
        out[key + "_eps_digest"] = G.digest(tn.latents(key))
    else:
        assert torch.equal(out[key + "_eps"], tn.latents(key))


def main():
    R.setup()
    out = {}
    for key in tn.MODELS:
        run_model(key, out)
    small = [k for k, v in out.items() if torch.is_tensor(v) and v.numel() > G.SMALL and not k.endswith("_eps")]
    assert not small, small
    save("score_train_narrow", **out)


if __name__ == "__main__":
    main()
