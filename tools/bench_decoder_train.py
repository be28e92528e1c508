"""Time of one decoder training step of the Compressor at the shipped stage-1 shape (hidden 128, 4 heads of 32, 6 levels, 32 latent tokens,
2048 set points), B = 16: HIP events around the forward, the Chamfer loss with its gradient, the backward and the optimizer (one warm-up
step, then the median of 7), and the attention backward alone (ldt_attention_bwd_long: row statistics, dQ, and dK / dV summed per chunk of
LDT_ATTN_BWD_LONG_CHUNK = 256 queries).
    python tools/bench_decoder_train.py [out.txt]               # out.txt defaults to profiles/decoder_train_step.txt, the committed record
The chunk length is a source constant.  To compare it with dK / dV as ONE sweep over the queries (one wave per 16 keys walking all 2048),
build a second library with the constant at 8192 and pass it: the attention backward is then timed again in a child process on that library
(row statistics and dQ are the same kernels in both, so the difference is the dK / dV form's):
    (ldt_amd/csrc/build.sh's command lines into another directory, with -DAB_CHUNK=8192 on csrc/attention_bwd.hip) -> libldt_one_chunk.so
    python tools/bench_decoder_train.py out.txt --one-chunk-lib libldt_one_chunk.so
What is timed is the whole call of the entry point (statistics + dQ + dK / dV), not the dK / dV kernel alone.
No speed target is attached to these numbers: the step is the unfused, host-driven form."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ldt_amd  # noqa: E402
from ldt_amd import losses, ops  # noqa: E402
from ldt_amd.compressor_train import DecoderTrainStep, decoder_parameters  # noqa: E402

CALLS = 7
B, N, T = 16, 2048, 32
args = sys.argv[1:]
one_chunk_lib = None
if "--one-chunk-lib" in args:
    i = args.index("--one-chunk-lib")
    one_chunk_lib = args[i + 1]
    del args[i:i + 2]
attention_only = "--attention-only" in args
args = [a for a in args if a != "--attention-only"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "decoder_train_step.txt")
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
    q, kv, do = bf(B * N, C), bf(B * T, 2 * C), bf(B, H, N, Dh)
    o = ops.attention_fwd(q, kv[:, :C], kv[:, C:], B, H, N, T, Dh)
    scratch = torch.empty(ops.attention_bwd_long_scratch(B, H, N, T), dtype=torch.float32, device="cuda")
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    return median_ms(lambda: ops.attention_bwd_long(q, kv[:, :C], kv[:, C:], o, do, B, H, N, T, dq_out=dq, dkv_out=dkv, scratch=scratch), 21)


if attention_only:                                                 # the child process on the one-chunk library
    print("%.4f" % attention_backward_ms())
    sys.exit(0)

cfg = ldt_amd.airplane_config(latent_tokens=T)
c = cfg.compressor
torch.manual_seed(0)
model = ldt_amd.Compressor(c)
model.init()
model = model.cuda()
params = [p for _, p in decoder_parameters(model)]
opt = ldt_amd.AdamEMA(params, lr=1e-4, ema_decay=0.)
g = torch.Generator().manual_seed(1)
eps = torch.randn(B, T, c.n_layers * c.z_dim, generator=g).cuda()
target = torch.randn(B, N, 3, generator=g)
target = (target / target.norm(dim=-1).amax(1)[:, None, None]).cuda()
ms = {"forward": [], "loss": [], "backward": [], "optimizer": []}
for it in range(CALLS + 1):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    opt.zero_grad()
    step = DecoderTrainStep(model)
    ev[0].record()
    pts = step.forward(eps, num_points=N)
    ev[1].record()
    loss, d_set = losses.cd_loss(pts, target, "l1", want_grad=True)
    ev[2].record()
    step.backward(d_set)
    ev[3].record()
    opt.step(max_norm=1.0)
    model.invalidate_packed()
    ev[4].record()
    torch.cuda.synchronize()
    if it:                                                        # the first step is the warm-up (allocation, panel packing)
        for k, i in zip(ms, range(4)):
            ms[k].append(ev[i].elapsed_time(ev[i + 1]))
med = {k: statistics.median(v) for k, v in ms.items()}
say("Compressor decoder training step  B %d  N %d  T %d  hidden %d  heads %d x %d  levels %d  (%d decoder-side parameters)  loss %.4f"
    % (B, N, T, c.hidden_dim, c.num_heads, c.hidden_dim // c.num_heads, c.n_layers, sum(p.numel() for p in params), float(loss)))
say("  forward %7.2f ms   loss + gradient %6.2f ms   backward %7.2f ms   optimizer %6.2f ms   step %7.2f ms   (median of %d after one warm-up)"
    % (med["forward"], med["loss"], med["backward"], med["optimizer"], sum(med.values()), CALLS))
say("  peak memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30))
chunked = attention_backward_ms()
say("attention backward alone (ldt_attention_bwd_long: statistics, dQ, dK / dV), B %d, 4 heads x 32, Nq %d, Nk %d, median of 21:" % (B, N, T))
say("  dK / dV in chunks of %d queries (%d partials per key block, added in chunk order)   %.3f ms" % (ldt_amd._lib.ATTN_BWD_LONG_CHUNK, -(-N // ldt_amd._lib.ATTN_BWD_LONG_CHUNK), chunked))
if one_chunk_lib:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--attention-only"], env=dict(os.environ, LDT_HIP_LIB=os.path.abspath(one_chunk_lib)),
                       capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise SystemExit("the one-chunk run failed:\n" + r.stdout + r.stderr)
    one = float(r.stdout.strip().splitlines()[-1])
    say("  dK / dV as one chunk of 8192 (one wave per 16 keys walks every query)               %.3f ms" % one)
    say("  the same statistics and dQ kernels in both: the dK / dV form accounts for the difference of %.3f ms (%.2f x the whole call)" % (one - chunked, one / chunked))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
