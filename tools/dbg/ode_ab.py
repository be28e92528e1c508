"""Probability-flow ODE sampling, `solver="scipy"` against `solver="device"`: child processes alternate on one box; each builds the
production-width Score (hidden 1024 x 24 blocks, seeded) once and samples B = 64 x T = 256 and B = 64 x T = 32 at tol = 1e-3,
ode_eps = 1e-2 from the same seeded noise.  Prints NFE, seconds per call and ms per NFE per solver and shape, the accepted / rejected
step counts and `Score.forward_shared_t`'s own time at the shape (what ms per NFE of the device path can approach at best), and the
rel-MSE between the two solvers' latents.   usage: ode_ab.py [rounds] [calls]      (about 75 s of host-side model init per child)"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
CHILD = r'''
import json, os, sys, time
sys.path.insert(0, %r)
import torch, ldt_amd
solver, calls, dump = sys.argv[1], int(sys.argv[2]), sys.argv[3]
cfg = ldt_amd.airplane_config(latent_tokens=32)
torch.manual_seed(0)
score = ldt_amd.Score(cfg.score); comp = ldt_amd.Compressor(cfg.compressor)
tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
tr.model.eval()
B, z = 64, cfg.score.z_dim
res = {}
for T in (256, 32):
    x1 = torch.randn(B, T, z, generator=torch.Generator().manual_seed(100 + T))
    best, nfe, out = 1e9, 0, None
    for r in range(calls + 1):                                             # the first call warms up (weight packing, workspaces)
        torch.cuda.synchronize()
        out, nfe, secs = tr.SDE.sample_model_ode(tr.score_fn, B, (T, z), 1e-2, 1e-3, noise=x1, device="cuda:0", solver=solver)
        if r:
            best = min(best, secs)
    row = {"nfe": nfe, "seconds": best, "ms_per_nfe": best / nfe * 1e3}
    if solver == "device":
        info = tr.SDE.last_ode
        row.update(accepted=info["accepted"], rejected=info["rejected"], route=info["route"])
        xd = x1.cuda()
        tr.model.forward_shared_t(xd, 0.5)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(10):
            tr.model.forward_shared_t(xd, 0.5)
        e1.record(); torch.cuda.synchronize()
        row["forward_shared_t_ms"] = e0.elapsed_time(e1) / 10
    torch.save(out.cpu(), "%%s_%%s_T%%d.pt" %% (dump, solver, T))
    res["T%%d" %% T] = row
print(json.dumps(res), flush=True)
''' % (ROOT,)
import tempfile
tmp = tempfile.mkdtemp(prefix="ode_ab_")
dump = os.path.join(tmp, "lat")
rows = {"scipy": [], "device": []}
for rnd in range(rounds):
    for solver in ("scipy", "device"):
        out = subprocess.run([sys.executable, "-c", CHILD, solver, str(calls), dump], capture_output=True, text=True)
        try:
            r = json.loads(out.stdout.strip().splitlines()[-1])
        except Exception:
            print(out.stdout[-500:], out.stderr[-1500:]); raise
        rows[solver].append(r)
        for k, v in r.items():
            extra = "" if solver == "scipy" else "  (%d accepted, %d rejected, %s; forward_shared_t alone %.3f ms)" % (
                v["accepted"], v["rejected"], v["route"], v["forward_shared_t_ms"])
            print("round %d B=64 %-4s solver=%-6s: nfe %3d  %.4f s per call  %.3f ms per NFE%s"
                  % (rnd, k, solver, v["nfe"], v["seconds"], v["ms_per_nfe"], extra), flush=True)
import torch
for T in (256, 32):
    a, b = torch.load("%s_scipy_T%d.pt" % (dump, T)).double(), torch.load("%s_device_T%d.pt" % (dump, T)).double()
    k = "T%d" % T
    print("B=64 %-4s: best seconds per call scipy %.4f, device %.4f (x%.2f); rel-MSE device vs scipy %.3e"
          % (k, min(r[k]["seconds"] for r in rows["scipy"]), min(r[k]["seconds"] for r in rows["device"]),
             min(r[k]["seconds"] for r in rows["scipy"]) / min(r[k]["seconds"] for r in rows["device"]),
             float(((a - b) ** 2).sum() / (a ** 2).sum())))
