"""Time of one encoder + top-down training step of the Compressor at the shipped stage-1 shape (hidden 128, 4 heads of 32, 6 stages x 2
AdaLN blocks, 32 tokens, p_dim 256, 2048 set points), B = 16: HIP events around the encoder forward (ActNorm and the stages), the top-down
forward, the Chamfer loss with its gradient, the interleaved top-down backward, the encoder backward (the stages in reverse, the stacked
adaLN linear, ldt_actnorm_bwd) and the optimizer: one warm-up step, then the median of 7.  The ActNorm backward is timed alone as well, in
both forms of the reference's ActNorm (per token and channel: B samples of T C; 'set': B T rows of C, and a 'set' call long enough for the
second stage).
    python tools/bench_encoder_train.py [out.txt]               # out.txt defaults to profiles/encoder_train_step.txt, the committed record
The tokens and the position condition are seeded draws: the frozen front (input conv, grouper, position embedding) is not part of the step.
No speed target is attached to these numbers: the step is the unfused, host-driven form, and nobody had measured it; the top-down step's
figure (profiles/topdown_train_step.txt) is printed beside it for scale only."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ldt_amd  # noqa: E402
from ldt_amd import losses, ops  # noqa: E402
from ldt_amd.compressor_train import EncoderTrainStep, TopDownTrainStep, encoder_parameters, topdown_parameters  # noqa: E402

CALLS = 7
B, N, T = 16, 2048, 32
TOPDOWN_STEP_MS = 46.78                                            # profiles/topdown_train_step.txt
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "encoder_train_step.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn, calls=CALLS):
    fn()                                                           # warm-up
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


cfg = ldt_amd.airplane_config(latent_tokens=T)
c = cfg.compressor
torch.manual_seed(0)
model = ldt_amd.Compressor(c)
model.init()
model = model.cuda()
params = [p for _, p in encoder_parameters(model) + topdown_parameters(model)]
n_enc = sum(p.numel() for _, p in encoder_parameters(model))
opt = ldt_amd.AdamEMA(params, lr=1e-4, ema_decay=0.)
g = torch.Generator().manual_seed(1)
tokens = torch.randn(B, T, c.hidden_dim, generator=g).cuda()
pos = torch.randn(B, c.p_dim, generator=g).cuda()
post_noise = [torch.randn(B, T, c.z_dim, generator=g).cuda() for _ in range(c.n_layers)]
target = torch.randn(B, N, 3, generator=g)
target = (target / target.norm(dim=-1).amax(1)[:, None, None]).cuda()
kl_scale = 1e-6 / (c.n_layers * B * c.z_dim * T)                   # the shipped kl_weight
keys = ("encoder forward", "top-down forward", "loss", "top-down backward", "encoder backward", "optimizer")
ms = {k: [] for k in keys}
for it in range(CALLS + 1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(keys) + 1)]
    opt.zero_grad()
    enc, top = EncoderTrainStep(model), TopDownTrainStep(model)
    ev[0].record()
    enc_out = enc.forward(tokens, pos)
    ev[1].record()
    pts, _, kls = top.forward(enc_out, post_noise, num_points=N)
    ev[2].record()
    loss, d_set = losses.cd_loss(pts, target, "l1", want_grad=True)
    ev[3].record()
    d_enc = top.backward(d_set, kl_scale)
    ev[4].record()
    enc.backward(d_enc)
    ev[5].record()
    opt.step(max_norm=1.0)
    model.invalidate_packed()
    ev[6].record()
    torch.cuda.synchronize()
    if it:                                                        # the first step is the warm-up (allocation, panel packing)
        for i, k in enumerate(keys):
            ms[k].append(ev[i].elapsed_time(ev[i + 1]))
med = {k: statistics.median(v) for k, v in ms.items()}
say("Compressor encoder + top-down training step  B %d  N %d  T %d  hidden %d  heads %d x %d  stages %d x %d blocks  p_dim %d  (%d encoder of %d trained "
    "parameters)  Chamfer loss %.4f" % (B, N, T, c.hidden_dim, c.num_heads, c.hidden_dim // c.num_heads, c.n_layers, c.encoder_layers, c.p_dim, n_enc,
                                        sum(p.numel() for p in params), float(loss)))
say("  " + "   ".join("%s %.2f ms" % (k, med[k]) for k in keys))
say("  step %.2f ms, of which the encoder's forward + backward %.2f ms   (median of %d after one warm-up)"
    % (sum(med.values()), med["encoder forward"] + med["encoder backward"], CALLS))
say("  for scale only: the top-down step alone (profiles/topdown_train_step.txt) took %.2f ms; no target is set for this step" % TOPDOWN_STEP_MS)
say("  peak memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30))
say("ActNorm backward alone (ldt_actnorm_bwd: dx, dshift, dlog_scale), median of 21:")
for rows, per, what in ((B, T * c.hidden_dim, "per token and channel, the Compressor's"), (B * T, c.hidden_dim, "'set'"),
                        (64 * B * T, c.hidden_dim, "'set', 64 x the rows: two stages")):
    dz, z = torch.randn(rows, per, generator=g).cuda(), torch.randn(rows, per, generator=g).cuda()
    ls = (0.2 * torch.randn(per, generator=g)).cuda()
    dx, ds, dl = torch.empty_like(dz), torch.empty(per, device="cuda"), torch.empty(per, device="cuda")
    t = median_ms(lambda: ops.actnorm_bwd(dz, z, ls, rows, dx=dx, dshift=ds, dlog_scale=dl), 21)
    say("  %6d rows x %4d (%s)   %.4f ms   %.1f GB/s" % (rows, per, what, t, 3 * rows * per * 4 / t / 1e6))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
