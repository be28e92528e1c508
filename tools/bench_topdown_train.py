"""Time of one top-down training step of the Compressor at the shipped stage-1 shape (hidden 128, 4 heads of 32, 6 levels, 32 latent tokens,
2048 set points), B = 16: HIP events around the forward, the Chamfer loss with its gradient, the interleaved backward and the optimizer (one
warm-up step, then the median of 7), and the posterior's attention backward alone (ldt_attention_bwd_wide: 32 queries on 2048 keys; row
statistics and dQ per chunk of LDT_ATTN_BWD_WIDE_CHUNK = 256 keys, dK / dV by the key-block kernel).
    python tools/bench_topdown_train.py [out.txt]               # out.txt defaults to profiles/topdown_train_step.txt, the committed record
The chunk length is a source constant.  To compare it with the statistics and dQ as ONE sweep over the keys (one wave per 16 queries walking
all 2048), build a second library with the constant at 8192 and pass it: the attention backward is then timed again in a child process on
that library (dK / dV are the same kernel in both, so the difference is the chunked form's):
    (ldt_amd/csrc/build.sh's command lines into another directory, with -DAB_WIDE_CHUNK=8192 on csrc/attention_bwd.hip) -> libldt_one_sweep.so
    python tools/bench_topdown_train.py out.txt --one-sweep-lib libldt_one_sweep.so
What is timed is the whole call of the entry point.  No speed target is attached to these numbers: the step is the unfused, host-driven
form, and nobody had measured it; the decoder step's figure (profiles/decoder_train_step.txt) is printed beside it for scale only."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ldt_amd  # noqa: E402
from ldt_amd import losses, ops  # noqa: E402
from ldt_amd.compressor_train import TopDownTrainStep, topdown_parameters  # noqa: E402

CALLS = 7
B, N, T = 16, 2048, 32
DECODER_STEP_MS = 37.37                                            # profiles/decoder_train_step.txt
args = sys.argv[1:]
one_sweep_lib = None
if "--one-sweep-lib" in args:
    i = args.index("--one-sweep-lib")
    one_sweep_lib = args[i + 1]
    del args[i:i + 2]
attention_only = "--attention-only" in args
args = [a for a in args if a != "--attention-only"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "topdown_train_step.txt")
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


def attention_backward_ms(H=4, Dh=32):
    g = torch.Generator().manual_seed(2)
    C = H * Dh
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).cuda()
    q, kv, do = bf(B * T, C), bf(B * N, 2 * C), bf(B, H, T, Dh)
    o = ops.attention_fwd(q, kv[:, :C], kv[:, C:], B, H, T, N, Dh)
    # (sized for the shipped chunk: a library built with a longer chunk needs less)
    scratch = torch.empty(ops.attention_bwd_wide_scratch(B, H, T, N), dtype=torch.float32, device="cuda")
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    return median_ms(lambda: ops.attention_bwd_wide(q, kv[:, :C], kv[:, C:], o, do, B, H, T, N, dq_out=dq, dkv_out=dkv, scratch=scratch), 21)


if attention_only:                                                 # the child process on the one-sweep library
    print("%.4f" % attention_backward_ms())
    sys.exit(0)

cfg = ldt_amd.airplane_config(latent_tokens=T)
c = cfg.compressor
torch.manual_seed(0)
model = ldt_amd.Compressor(c)
model.init()
model = model.cuda()
params = [p for _, p in topdown_parameters(model)]
opt = ldt_amd.AdamEMA(params, lr=1e-4, ema_decay=0.)
g = torch.Generator().manual_seed(1)
enc_out = [torch.randn(B, T, c.hidden_dim, generator=g).cuda() for _ in range(c.n_layers)]
post_noise = [torch.randn(B, T, c.z_dim, generator=g).cuda() for _ in range(c.n_layers)]
target = torch.randn(B, N, 3, generator=g)
target = (target / target.norm(dim=-1).amax(1)[:, None, None]).cuda()
kl_scale = 1e-6 / (c.n_layers * B * c.z_dim * T)                   # the shipped kl_weight
ms = {"forward": [], "loss": [], "backward": [], "optimizer": []}
for it in range(CALLS + 1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    opt.zero_grad()
    step = TopDownTrainStep(model)
    ev[0].record()
    pts, _, kls = step.forward(enc_out, post_noise, num_points=N)
    ev[1].record()
    loss, d_set = losses.cd_loss(pts, target, "l1", want_grad=True)
    ev[2].record()
    step.backward(d_set, kl_scale)
    ev[3].record()
    opt.step(max_norm=1.0)
    model.invalidate_packed()
    ev[4].record()
    torch.cuda.synchronize()
    if it:                                                        # the first step is the warm-up (allocation, panel packing)
        for k, i in zip(ms, range(4)):
            ms[k].append(ev[i].elapsed_time(ev[i + 1]))
med = {k: statistics.median(v) for k, v in ms.items()}
say("Compressor top-down training step  B %d  N %d  T %d  hidden %d  heads %d x %d  levels %d  (%d top-down parameters)  Chamfer loss %.4f"
    % (B, N, T, c.hidden_dim, c.num_heads, c.hidden_dim // c.num_heads, c.n_layers, sum(p.numel() for p in params), float(loss)))
say("  forward %7.2f ms   loss + gradient %6.2f ms   backward %7.2f ms   optimizer %6.2f ms   step %7.2f ms   (median of %d after one warm-up)"
    % (med["forward"], med["loss"], med["backward"], med["optimizer"], sum(med.values()), CALLS))
say("  for scale only: the decoder step alone (profiles/decoder_train_step.txt) took %.2f ms; no target is set for this step" % DECODER_STEP_MS)
say("  peak memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30))
chunked = attention_backward_ms()
chunk = ldt_amd._lib.ATTN_BWD_WIDE_CHUNK
say("attention backward alone (ldt_attention_bwd_wide: chunk statistics, row statistics, dQ, dK / dV), B %d, 4 heads x 32, Nq %d, Nk %d, median of 21:" % (B, T, N))
say("  statistics and dQ in chunks of %d keys (%d partials per query block, combined in chunk order)   %.3f ms" % (chunk, -(-N // chunk), chunked))
if one_sweep_lib:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--attention-only"], env=dict(os.environ, LDT_HIP_LIB=os.path.abspath(one_sweep_lib)),
                       capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise SystemExit("the one-sweep run failed:\n" + r.stdout + r.stderr)
    one = float(r.stdout.strip().splitlines()[-1])
    say("  statistics and dQ as one chunk of 8192 (one wave per 16 queries walks every key)             %.3f ms" % one)
    say("  the same dK / dV kernel in both: the chunked form accounts for the difference of %.3f ms (%.2f x the whole call)" % (one - chunked, one / chunked))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
