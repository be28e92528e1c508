"""Time of one Score training step at production width (hidden 1024, 16 heads, 24 blocks), B = 64, at T = 32 and T = 256 latent tokens:
HIP events around the forward, the backward and the optimizer (one warm-up step, then the median of 7), and the rate against 3 x the
forward's FLOPs (forward + dgrad + wgrad of every GEMM; the attention backward's extra recomputation is not credited).
    python tools/bench_train.py [out.txt] [tokens ...]          # out.txt defaults to profiles/train_step.txt, the committed record
Other Score sizes: --hidden H --t-dim D and comma lists --heads a,b,.. --batch a,b,.. (every combination is timed, heads outermost), e.g. the
hybrid config's Score next to the 2- and 8-head models of the same width (profiles/train_step_narrow.txt):
    python tools/bench_train.py profiles/train_step_narrow.txt 32 --hidden 128 --t-dim 128 --heads 16,2,8 --batch 8,64
A condition of S tokens: --cond S times every combination twice in the same run, first unconditional, then on the embedded ViPC pair
(pts_condition (B, hidden, S), img_condition (B, t_dim)): the even blocks cross-attend to the S condition tokens (ldt_attention_bwd_cross) and
the step forms the gradient with respect to the pair.  BASELINE configs[4]'s share, production width (profiles/train_step_cond.txt):
    python tools/bench_train.py profiles/train_step_cond.txt 32 --batch 32 --cond 32
No speed target is attached to these numbers: the step is the unfused, host-driven form; the follow-up that fuses it starts here."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import ldt_amd  # noqa: E402
from ldt_amd import ops  # noqa: E402
from ldt_amd.train import ScoreTrainStep  # noqa: E402

argv, opts = [], {}
it = iter(sys.argv[1:])
for a in it:
    if a in ("--hidden", "--heads", "--t-dim", "--batch", "--cond"):
        opts[a] = [int(v) for v in next(it).split(",")]
    else:
        argv.append(a)
out_path = argv[0] if argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "train_step.txt")
tokens = [int(a) for a in argv[1:]] or [32, 256]
CALLS = 7
overrides = {k: opts[o][0] for o, k in (("--hidden", "score.hidden_size"), ("--t-dim", "score.t_dim")) if o in opts}
conds = [0] + opts.get("--cond", [])                               # 0: unconditional; S: the same step on a condition of S tokens
runs = [(h, b, T, S) for h in opts.get("--heads", [None]) for b in opts.get("--batch", [64]) for T in tokens for S in conds]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def forward_flops(m, T, S=0):
    D, F, z, nb, M = m.hidden_size, m.Transformer[0].mlp.out.in_channels, m.z_dim, m.num_blocks, B * T
    nx = (nb + 1) // 2 if S else 0                                 # cross-attention blocks: the even ones (score.py:149)
    gemm = 2 * M * (z * D + nb * (D * D + 2 * D * F) + (nb - nx) * 3 * D * D + nx * D * D + D * z) + nx * 2 * B * S * 2 * D * D
    attn = (nb - nx) * 4 * B * T * T * D + nx * 4 * B * T * S * D
    return gemm + attn


for heads, B, T, S in runs:
    cfg = ldt_amd.airplane_config(latent_tokens=T, **dict(overrides, **({} if heads is None else {"score.num_heads": heads})))
    torch.manual_seed(0)
    model = ldt_amd.Score(cfg.score).cuda()
    opt = ldt_amd.AdamEMA(model.parameters(), lr=1e-4, ema_decay=0.9999)
    g = torch.Generator().manual_seed(1)
    x, eta = torch.randn(B, T, model.z_dim, generator=g).cuda(), torch.randn(B, T, model.z_dim, generator=g).cuda()
    t = (torch.rand(B, generator=g) * 0.98 + 0.01).cuda()
    pair = (torch.randn(B, model.hidden_size, S, generator=g).cuda() * 0.5, torch.randn(B, model.t_dim, generator=g).cuda() * 0.5) if S else None
    ms = {"forward": [], "backward": [], "optimizer": []}
    for it in range(CALLS + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        opt.zero_grad()
        step = ScoreTrainStep(model, allow_condition=bool(S))
        ev[0].record()
        params = step.forward(x, t, condition=pair)
        loss, _ = ops.dsm_loss(eta, params)
        ev[1].record()
        step.backward(ops.dsm_loss_bwd(eta, params))
        ev[2].record()
        opt.step(max_norm=1.0)
        model.invalidate_packed()
        ev[3].record()
        torch.cuda.synchronize()
        if it:                                                    # the first step is the warm-up (allocation, panel packing)
            for k, (a, b) in zip(ms, ((0, 1), (1, 2), (2, 3))):
                ms[k].append(ev[a].elapsed_time(ev[b]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    total = sum(med.values())
    fl = forward_flops(model, T, S)
    say("Score training step  B %d  T %d%s  hidden %d  blocks %d  (%d parameters)  loss %.4f%s" % (B, T, "  condition S %d" % S if S else "", model.hidden_size, model.num_blocks,
        sum(p.numel() for p in model.parameters()), float(loss),
        "  heads %d x %d  t_dim %d" % (model.num_heads, model.hidden_size // model.num_heads, model.t_dim) if set(opts) - {"--cond"} else ""))
    say("  forward %8.2f ms   backward %8.2f ms   optimizer %7.2f ms   step %8.2f ms   (median of %d after one warm-up)"
        % (med["forward"], med["backward"], med["optimizer"], total, CALLS))
    say("  forward FLOPs %.3e;  3 x forward / step = %.1f TFLOP/s;  forward alone %.1f TFLOP/s;  peak memory %.2f GB"
        % (fl, 3 * fl / total / 1e9, fl / med["forward"] / 1e9, torch.cuda.max_memory_allocated() / 2 ** 30))
    del model, opt, step, params
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
