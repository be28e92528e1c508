"""Time of one whole training step of the Compressor — front, encoder and top-down half — at the shipped stage-1 shape (hidden 128, 4 heads
of 32, 6 stages x 2 AdaLN blocks, 32 tokens of k = 128 neighbours, p_dim 256, 2048 points), B = 16: HIP events around the front forward
(input conv, FPS / kNN, grouping, the three PreExtraction GEMMs with training-mode BatchNorm, the neighbour max, MiniPointnet), the encoder
forward, the top-down forward, the Chamfer loss with its gradient, the top-down, encoder and front backwards and the optimizer: one warm-up
step, then the median of 7.  The same run times the step with the front frozen (update_encoder's phases) for scale, and the new ENTRY POINTS
alone with the bytes they move (computed from the shapes here) over the time of a whole call: HIP events around the entry point, which
holds its stream-ordered allocation, one to six launches and their launch overhead — entry-point times, not kernel times.
    python tools/bench_front_train.py [out.txt]                 # out.txt defaults to profiles/front_train_step.txt, the committed record
    python tools/bench_front_train.py --kernels-only            # the entry points alone, nothing written: the program of a kernel-trace run
                                                                # of its own (rocprofv3 --kernel-trace --stats -- python ... --kernels-only)
No speed target is attached to these numbers: the step is the unfused, host-driven form, and nobody had measured it."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ldt_amd  # noqa: E402
from ldt_amd import losses, ops  # noqa: E402
from ldt_amd.compressor_train import (EncoderTrainStep, FrontTrainStep, TopDownTrainStep, encoder_parameters, front_parameters,  # noqa: E402
                                      topdown_parameters)

CALLS = 7
B, N, T = 16, 2048, 32
KERNELS_ONLY = "--kernels-only" in sys.argv[1:]
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = None if KERNELS_ONLY else (_pos[0] if _pos else os.path.join(ROOT, "profiles", "front_train_step.txt"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn, calls=21):
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
model = model.cuda().train()
g = torch.Generator().manual_seed(1)
post_noise = [torch.randn(B, T, c.z_dim, generator=g).cuda() for _ in range(c.n_layers)]
target = torch.randn(B, N, 3, generator=g)
target = (target / target.norm(dim=-1).amax(1)[:, None, None]).cuda()
kl_scale = 1e-6 / (c.n_layers * B * c.z_dim * T)                   # the shipped kl_weight


def run(with_front):
    """-> ({phase: median ms}, the last loss).  with_front False: the front runs frozen (Compressor.front, evaluation mode), untimed."""
    lists = (front_parameters(model) if with_front else []) + encoder_parameters(model) + topdown_parameters(model)
    opt = ldt_amd.AdamEMA([p for _, p in lists], lr=1e-4, ema_decay=0.)
    keys = ("front forward", "encoder forward", "top-down forward", "loss", "top-down backward", "encoder backward", "front backward", "optimizer")
    ms = {k: [] for k in keys}
    for it in range(CALLS + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(keys) + 1)]
        opt.zero_grad()
        front, enc, top = FrontTrainStep(model), EncoderTrainStep(model), TopDownTrainStep(model)
        if not with_front:
            model.eval()
            fr = model.front(target)
            tokens, pos = fr["tokens"], fr["pos"]
            model.train()
        ev[0].record()
        if with_front:
            tokens, pos = front.forward(target)
        ev[1].record()
        enc_out = enc.forward(tokens, pos)
        ev[2].record()
        pts, _, kls = top.forward(enc_out, post_noise, num_points=N)
        ev[3].record()
        loss, d_set = losses.cd_loss(pts, target, "l1", want_grad=True)
        ev[4].record()
        d_enc = top.backward(d_set, kl_scale)
        ev[5].record()
        d_tokens, d_pos = enc.backward(d_enc)
        ev[6].record()
        if with_front:
            front.backward(d_tokens, d_pos)
        ev[7].record()
        opt.step(max_norm=1.0)
        model.invalidate_packed()
        ev[8].record()
        torch.cuda.synchronize()
        if it:                                                    # the first step is the warm-up (allocation, panel packing)
            for i, k in enumerate(keys):
                ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    return {k: statistics.median(v) for k, v in ms.items()}, float(loss)


k_nb = N // T * 2
M = B * T * k_nb
say("Compressor whole training step  B %d  N %d  T %d  k %d (M = %d grouped rows)  hidden %d  stages %d x %d blocks  p_dim %d  (%d front of %d parameters)"
    % (B, N, T, k_nb, M, c.hidden_dim, c.n_layers, c.encoder_layers, c.p_dim, sum(p.numel() for _, p in front_parameters(model)),
       sum(p.numel() for p in model.parameters())))
if not KERNELS_ONLY:
    frozen, _ = run(False)
    say("  front frozen (update_encoder's phases):  " + "   ".join("%s %.2f ms" % (k, v) for k, v in frozen.items() if not k.startswith("front")))
    say("    step %.2f ms   (median of %d after one warm-up)" % (sum(v for k, v in frozen.items() if not k.startswith("front")), CALLS))
    med, loss = run(True)
    say("  front trained (update_front's phases):   " + "   ".join("%s %.2f ms" % kv for kv in med.items()))
    say("    step %.2f ms, of which the front's forward + backward %.2f ms   Chamfer loss %.4f   (median of %d after one warm-up)"
        % (sum(med.values()), med["front forward"] + med["front backward"], loss, CALLS))
    say("  no target is set for this step; peak memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30))

D = c.hidden_dim
say("the new entry points alone at the step's shapes, median of 21 whole calls (allocation, every launch and the launch overhead included: entry-point\n"
    "times, not kernel times; bytes from the shapes: what a call must read and write once; the operands stay in the Infinity Cache between calls):")
x = torch.randn(M, D, generator=g).cuda()
dy = torch.randn(M, D, generator=g).cuda()
ga, be = (torch.rand(D, generator=g) + 0.5).cuda(), torch.randn(D, generator=g).cuda()
st = ops.bn_stats(x)
t = median_ms(lambda: ops.bn_stats(x))
say("  ldt_bn_stats          [%d, %d]   %.4f ms   %.0f GB/s (x read twice: %d MB)" % (M, D, t, 2 * M * D * 4 / t / 1e6, 2 * M * D * 4 >> 20))
y = torch.empty((M, D), dtype=torch.bfloat16, device="cuda")
t = median_ms(lambda: ops.bn_relu_fwd(x, st, ga, be, out=y))
say("  ldt_bn_relu_fwd bf16  [%d, %d]   %.4f ms   %.0f GB/s (%d MB)" % (M, D, t, M * D * 6 / t / 1e6, M * D * 6 >> 20))
dx = torch.empty_like(x)
t = median_ms(lambda: ops.bn_relu_bwd(dy, x, st, ga, be, dx=dx))
say("  ldt_bn_relu_bwd       [%d, %d]   %.4f ms   %.0f GB/s (dy, x read twice, dx written: %d MB)" % (M, D, t, 5 * M * D * 4 / t / 1e6, 5 * M * D * 4 >> 20))
G = B * T
z = torch.randn(M, D, generator=g).cuda()
tok, arg = ops.maxpool_argmax(z, G, k_nb, relu=True)
t = median_ms(lambda: ops.maxpool_argmax(z, G, k_nb, relu=True))
say("  ldt_maxpool_argmax    [%d x %d, %d]   %.4f ms   %.0f GB/s (%d MB)" % (G, k_nb, D, t, M * D * 4 / t / 1e6, M * D * 4 >> 20))
d_tok = torch.randn(G, D, generator=g).cuda()
dz = torch.empty_like(z)
t = median_ms(lambda: ops.maxpool_relu_bwd(d_tok, tok, arg, k_nb, dz=dz))
say("  ldt_maxpool_relu_bwd  [%d x %d, %d]   %.4f ms   %.0f GB/s (%d MB written)" % (G, k_nb, D, t, M * D * 4 / t / 1e6, M * D * 4 >> 20))
feat = torch.randn(B, N, D, generator=g).cuda()
pts = target
fi = ops.fps(pts, T)
ki = ops.knn(pts, ops.gather_rows(pts, fi), k_nb)
ld = ops.pad64(2 * D + 3)
dU = torch.randn(M, ld, generator=g).cuda()
al = (torch.rand(D + 3, generator=g) + 0.5).cuda()
index = ops.knn_inverted_index(ki, N)
nbytes = M * (2 * D + 3) * 4 * 2 + M * D * 4 * 2 + B * N * D * 4                    # dU read by the sums and again by the gather; the gathered rows twice; dfeat
t = median_ms(lambda: ops.group_normalize_bwd(dU, feat, pts, fi, ki, al, index=index))
say("  ldt_group_normalize_bwd  B %d n %d S %d k %d D %d   %.4f ms   %.0f GB/s (%d MB; the inverted index built once outside: %.4f ms)"
    % (B, N, T, k_nb, D, t, nbytes / t / 1e6, nbytes >> 20, median_ms(lambda: ops.knn_inverted_index(ki, N))))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
