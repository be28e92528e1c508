"""GPU (-m gpu): parity at the PRODUCTION size — the shipped Score (hidden 1024, 16 heads, 24 blocks, 457 M parameters) at
256 latent tokens, seeded weights, against the CPU oracle:

  * B = 64 teacher-forced forward (M = 16,384 rows): the path bench.py times — persistent 256^2 GEMMs with the LayerNorm
    folded into their epilogues (`gemm_bf16_nt_256_kernel<1,2> / <2,2> / <4,1>`), streaming attention — and the
    LayerNorm-kernel path on the same input;
  * BASELINE config C1 exactly: B = 4, N = 100 ancestral steps with injected noise, through Trainer.sample: per-step
    relative-MSE curve of the latents, final latents, decoded cloud and its Chamfer distance (normalised by the cloud's mean
    squared radius), with the decode bar calibrated by the oracle's own sensitivity (random weights: tests/test_gpu_path.py).

Tolerances (relative MSE |a-b|^2/|b|^2): forward <= 1e-4; every step and the final latents <= 1e-4 (north-star:
"per-step MSE and final Chamfer within a stated fp tolerance").  The oracle passes take ~20 s + ~60 s of CPU."""
import copy

import pytest
import torch

from conftest import host_cores, rel_mse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def full():
    import ldt_amd
    from oracle import ldt_oracle as O
    torch.set_num_threads(host_cores())
    cfg = ldt_amd.airplane_config(latent_tokens=256, sample_N=100)
    assert (cfg.score.hidden_size, cfg.score.num_heads, cfg.score.num_blocks) == (1024, 16, 24)
    torch.manual_seed(0)
    score = ldt_amd.Score(cfg.score)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    sd_s = {k: v.detach().clone() for k, v in score.state_dict().items()}
    sd_c = {k: v.detach().clone() for k, v in comp.state_dict().items()}
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    return dict(cfg=cfg, tr=tr, score=tr.model, comp=tr.compressor, sd_s=sd_s, sd_c=sd_c, O=O)


def test_fullsize_teacher_forced_b64(full):
    O, cfg, score = full["O"], full["cfg"], full["score"]
    B, T, z = 64, 256, cfg.score.z_dim
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, T, z, generator=g)
    t = 0.37
    assert score.can_fold(B, T)                                   # the production decision for this batch
    folded = score.forward_shared_t(x.cuda(), t)
    unfolded = score.forward_shared_t(x.cuda(), t, fold=False)    # LayerNorm kernels instead of the folded epilogues
    per_sample = score(x.cuda(), torch.full((B,), t).cuda())      # per-sample AdaLN rows (the generic / conditioned path)
    with torch.no_grad():
        ref = O.score_forward(full["sd_s"], cfg.score, x, torch.full((B,), t))
    e_f, e_u, e_p = rel_mse(folded.cpu(), ref), rel_mse(unfolded.cpu(), ref), rel_mse(per_sample.cpu(), ref)
    print("full-size B=64 forward rel-MSE vs oracle: folded %.3e, LayerNorm kernels %.3e, per-sample rows %.3e" % (e_f, e_u, e_p))
    assert e_f < 1e-4 and e_u < 1e-4 and e_p < 1e-4
    assert e_f < 4 * max(e_u, 1e-7)                               # folding does not cost accuracy at K = 1024 / 4096, 24 blocks
    # a second time: t at the end of the schedule (AdaLN rows of t = 1e-6), inflated input scale
    x2 = x * 30.0
    with torch.no_grad():
        ref2 = O.score_forward(full["sd_s"], cfg.score, x2[:8], torch.full((8,), 1e-6))
    out2 = score.forward_shared_t(x2.cuda(), 1e-6)
    assert rel_mse(out2[:8].cpu(), ref2) < 1e-4


def test_fullsize_shipped_32_tokens_b64(full, monkeypatch):
    """The shipped YAML's regime at production width: B = 64 shapes x 32 latent tokens = 2048 token rows — every GEMM on the mid-size tile
    kernels (csrc/gemm_mid.hip: 128 x 192 / 128 x 256 / 64 x 128 tiles), resident attention — teacher-forced against the oracle, with the
    LayerNorm kernels (LDT_LN_FOLD_SMALL=0) and with the LayerNorms folded into the GEMM epilogues (row statistics per 32 columns: the
    production decision for this batch since round 4)."""
    O, cfg, score = full["O"], full["cfg"], full["score"]
    B, T, z = 64, 32, cfg.score.z_dim
    g = torch.Generator().manual_seed(33)
    x = torch.randn(B, T, z, generator=g)
    t = 0.61
    monkeypatch.delenv("LDT_LN_FOLD", raising=False)
    monkeypatch.setenv("LDT_LN_FOLD_SMALL", "0")
    assert not score.can_fold(B, T)
    plain = score.forward_shared_t(x.cuda(), t)
    monkeypatch.delenv("LDT_LN_FOLD_SMALL")
    assert score.can_fold(B, T)                                   # the production decision for this batch: folded
    folded = score.forward_shared_t(x.cuda(), t)
    with torch.no_grad():
        ref = O.score_forward(full["sd_s"], cfg.score, x, torch.full((B,), t))
    e_p, e_f = rel_mse(plain.cpu(), ref), rel_mse(folded.cpu(), ref)
    print("full-size B=64 x 32 tokens forward rel-MSE vs oracle: LayerNorm kernels %.3e, small-tile LN folding %.3e" % (e_p, e_f))
    assert e_p < 1e-4 and e_f < 1e-4
    assert e_f < 4 * max(e_p, 1e-7)
    assert not torch.equal(plain, folded)                         # the two paths really are different code


def test_c1_exact_free_running(full):
    """BASELINE configs[0] / SURVEY §8d C1: B=4, T=256, N=100, ancestral, decode included."""
    O, cfg, tr = full["O"], full["cfg"], full["tr"]
    B, N, T, z = 4, 100, 256, cfg.score.z_dim
    x0, noises = O.draw_noises(1234, B, T, z, N)
    rec = []
    with torch.no_grad():
        import time
        t0 = time.time()
        ref_pts, ref_eps = O.trainer_sample(full["sd_s"], full["sd_c"], cfg, x0, noises, record=rec,
                                            progress=lambda i: print("  oracle C1 step %d/%d  %.0f s" % (i + 1, N, time.time() - t0), flush=True)
                                            if (i + 1) % 10 == 0 else None)
        g = torch.Generator().manual_seed(0)
        pert = O.compressor_decode(full["sd_c"], cfg.compressor, ref_eps * (1 + 2 ** -9 * torch.randn(ref_eps.shape, generator=g)))
    traj = []
    pts, eps = tr.sample(B, x0=x0, noise=torch.stack(noises), trajectory=traj)
    xs = traj[0].cpu()
    assert xs.shape == (N, B, T, z)
    curve = [rel_mse(xs[i], rec[i][3]) for i in range(N)]
    r2 = (ref_pts ** 2).sum(-1).mean(1)
    cd = float((O.chamfer_cd(pts.cpu(), ref_pts) / r2).max())
    floor_pts, floor_cd = rel_mse(pert, ref_pts), float((O.chamfer_cd(pert, ref_pts) / r2).max())
    print("C1: per-step max %.3e (last %.3e), final latents %.3e, points %.3e (floor %.3e), Chamfer/r^2 %.3e (floor %.3e)"
          % (max(curve), curve[-1], rel_mse(eps.cpu(), ref_eps), rel_mse(pts.cpu(), ref_pts), floor_pts, cd, floor_cd))
    assert max(curve) < 1e-4, curve
    assert rel_mse(eps.cpu(), ref_eps) < 1e-4
    assert rel_mse(pts.cpu(), ref_pts) < max(2e-3, 4 * floor_pts)
    assert cd < max(2e-3, 4 * floor_cd)
    # the decoder alone on the ORACLE's latents (isolates Compressor.sample at the full 2048-point size)
    dec = tr.compressor.sample((B, cfg.data.tr_max_sample_points), given_eps=ref_eps.cuda())
    assert rel_mse(dec.cpu(), ref_pts) < max(2e-3, 4 * floor_pts)
    g2 = torch.Generator().manual_seed(3)
    zl = torch.randn(B, T, z, generator=g2)                        # N(0,1)-scale latents: the decoder's operating range
    with torch.no_grad():
        ref_dec = O.compressor_decode(full["sd_c"], cfg.compressor, zl)
    assert rel_mse(tr.compressor.sample((B, cfg.data.tr_max_sample_points), given_eps=zl.cuda()).cpu(), ref_dec) < 1e-4


def test_fullsize_teacher_forced_rows_of_1000_step_tables(full):
    """The headline config's own tables (BASELINE configs[1]: N = 1000): the 1000-row AdaLN table (598 MB) and LN-folding table
    (1.38 GB) that `sample_discrete` builds with the 128 x 128 fp32 MFMA tile (N <= 100 takes the skinny tile), addressed at
    rows 0 / 500 / 999 through the step counter exactly as step i of the fused loop does (base + i * stride).  B = 64 x T = 256
    teacher-forced forwards on the LN-folded 256^2 path at latents of the scale the loop has there (rms 1 / 20 / 300), the first 4
    samples against the oracle evaluated at t_i; the AdaLN rows themselves against the oracle's fp32 Linear(SiLU(TimeEmbedding)).
    Reference: diffusion/diffusion_continuous.py:238,243-244 (timesteps), model/layers.py:14-41,214 (rows)."""
    O, cfg, score = full["O"], full["cfg"], full["score"]
    B, T, z, N, nb, D = 64, 256, cfg.score.z_dim, 1000, 4, cfg.score.hidden_size
    ts = torch.linspace(1.0, 1e-6, N)
    _, mod = score.time_table(ts.cuda())
    assert mod.shape == (N, score.n_mod) and score.can_fold(B, T)
    fold = score.fold_table(mod)
    assert fold.shape[0] == N
    g = torch.Generator().manual_seed(1000)
    worst = 0.0
    for row, scale in ((0, 1.0), (500, 20.0), (999, 300.0)):
        t_i = ts[row:row + 1]
        c_ref = O.time_embedding(full["sd_s"], "TimeEmbedding", t_i, cfg.score.t_dim // 4)
        sc_ref = torch.nn.functional.silu(c_ref)
        for l in (0, 11, 23):
            ref_rows = O.linear(full["sd_s"], "Transformer.%d.adaLN.1" % l, sc_ref)
            assert rel_mse(mod[row:row + 1, l * 6 * D:(l + 1) * 6 * D].cpu(), ref_rows) < 1e-10, (row, l)
        assert rel_mse(mod[row:row + 1, -2 * D:].cpu(), O.linear(full["sd_s"], "ln_out.adaLN.1", sc_ref)) < 1e-10
        x = torch.randn(B, T, z, generator=g) * scale
        out = score.forward_table_row(x.cuda(), row, mod, fold)
        out_ln = score.forward_table_row(x.cuda(), row, mod, None)          # the LayerNorm-kernel path on the same rows
        with torch.no_grad():
            ref = O.score_forward(full["sd_s"], cfg.score, x[:nb], t_i.expand(nb))
        e_f, e_u = rel_mse(out[:nb].cpu(), ref), rel_mse(out_ln[:nb].cpu(), ref)
        print("row %d of the 1000-step tables (t = %.6f, |x| ~ %g): folded %.3e, LayerNorm kernels %.3e" % (row, float(t_i), scale, e_f, e_u))
        assert e_f < 1e-4 and e_u < 1e-4, (row, e_f, e_u)
        worst = max(worst, e_f)
    del fold, mod


def test_n1000_free_running_production_width(full):
    """The headline's own LENGTH: N = 1000 free-running ancestral steps at the production width (hidden 1024 x 24 blocks) through
    Trainer.sample with injected x0 / per-step noise against the CPU oracle — T = 32 tokens, B = 2 shapes (about 1.5 min of CPU):
    1000-row tables, step-indexed strides up to 999, a 1000-replay hipGraph, ten times the error accumulation of config C1.
    Per-step relative MSE of the latents (from the loop's trajectory dump) and the final latents <= 1e-4.
    Reference: diffusion/diffusion_continuous.py:152-162,231-258; trainer/Latent_SDE_Trainer.py:143-165."""
    import time
    import ldt_amd
    O, score = full["O"], full["score"]
    B, T, N = 2, 32, 1000
    cfg = ldt_amd.airplane_config(latent_tokens=T, sample_N=N)
    z = cfg.score.z_dim
    torch.manual_seed(4)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    x0, noises = O.draw_noises(4321, B, T, z, N)
    traj = []
    pts, eps = tr.sample(B, x0=x0, noise=torch.stack(noises), trajectory=traj)
    assert traj[0].shape == (N, B, T, z) and pts.shape == (B, cfg.data.tr_max_sample_points, 3)
    sde = O.VPSDE(cfg.sde)
    fn = O.score_fn_from_model(sde, lambda xx, tt: O.score_forward(full["sd_s"], cfg.score, xx, tt))
    rec = []
    t0 = time.time()
    with torch.no_grad():
        ref_eps = O.sample_discrete(sde, fn, x0, noises, N, record=rec,
                                    progress=lambda i: print("  oracle N=1000 step %d  %.0f s" % (i + 1, time.time() - t0), flush=True)
                                    if (i + 1) % 100 == 0 else None)
    xs = traj[0].cpu()
    curve = [rel_mse(xs[i], rec[i][3]) for i in range(N)]
    e_fin = rel_mse(eps.cpu(), ref_eps)
    print("N = 1000 free-running, hidden 1024 x 24 blocks, B = %d, T = %d: per-step max %.3e (step %d), steps 0/499/999 %.3e / %.3e / %.3e, "
          "final latents %.3e (rms %.1f)" % (B, T, max(curve), curve.index(max(curve)), curve[0], curve[499], curve[999], e_fin,
                                             float(ref_eps.pow(2).mean().sqrt())))
    assert max(curve) < 1e-4, (max(curve), curve.index(max(curve)))
    assert e_fin < 1e-4


def test_c1_shape_well_conditioned_fixed_bars(full):
    """End to end at the production width with FIXED bars: config C1's shape (B = 4, T = 256, N = 100, ancestral, decode to 2048
    points) on the well-conditioned fixture of oracle/fixtures.py — the seeded Score with ln_out.ln.weight += pinv(ln_in.weight),
    which keeps the latents at rms 0.1-2 through the reverse SDE (the plain seeded weights inflate them to ~400, where the decoder
    is ill-conditioned in fp32 already) — through Trainer.sample with injected noise against the oracle:
    every step and the final latents <= 1e-4, decoded points <= 1e-3, Chamfer / mean squared radius <= 1e-3.
    Reference: trainer/Latent_SDE_Trainer.py:143-165; diffusion/diffusion_continuous.py:152-162,231-258."""
    import time
    import ldt_amd
    from oracle.fixtures import condition_score_head
    O, cfg = full["O"], full["cfg"]
    B, N, T, z = 4, 100, 256, cfg.score.z_dim
    sd_w = condition_score_head(full["sd_s"])
    score = ldt_amd.Score(cfg.score)
    score.load_state_dict(sd_w, strict=True)
    tr = ldt_amd.Trainer(cfg, score, full["comp"], "cuda:0")
    x0, noises = O.draw_noises(99, B, T, z, N)
    traj = []
    pts, eps = tr.sample(B, x0=x0, noise=torch.stack(noises), trajectory=traj)
    rec = []
    t0 = time.time()
    with torch.no_grad():
        ref_pts, ref_eps = O.trainer_sample(sd_w, full["sd_c"], cfg, x0, noises, record=rec,
                                            progress=lambda i: print("  oracle (well-conditioned C1) step %d/%d  %.0f s" % (i + 1, N, time.time() - t0), flush=True)
                                            if (i + 1) % 10 == 0 else None)
    xs = traj[0].cpu()
    curve = [rel_mse(xs[i], rec[i][3]) for i in range(N)]
    rms = [float(rec[i][3].pow(2).mean().sqrt()) for i in (0, 50, 98, 99)]
    r2 = (ref_pts ** 2).sum(-1).mean(1)
    cd = float((O.chamfer_cd(pts.cpu(), ref_pts) / r2).max())
    e_fin, e_pts = rel_mse(eps.cpu(), ref_eps), rel_mse(pts.cpu(), ref_pts)
    print("well-conditioned C1 (latent rms at steps 0/50/98/99: %.2f / %.2f / %.2f / %.2f): per-step max %.3e, final latents %.3e, "
          "points %.3e, Chamfer / r^2 %.3e" % (rms[0], rms[1], rms[2], rms[3], max(curve), e_fin, e_pts, cd))
    assert max(rms) < 10.0                                          # the fixture does what it is for
    assert max(curve) < 1e-4, (max(curve), curve.index(max(curve)))
    assert e_fin < 1e-4
    assert e_pts < 1e-3 and cd < 1e-3


@pytest.mark.parametrize("tokens", [256, 32])
def test_compressor_fullsize_big_batch_vs_oracle(tokens):
    """BASELINE configs[3] shapes through the big-batch kernels (512 clouds per call: one-wave FPS, kNN candidate select, one-kernel
    grouper with 16 / 128 neighbours, resident attention + out-projection, next-level q in the MLP kernel, streaming 3 <-> C convs):
    the first 4 clouds of the batch carry the oracle's clouds, posterior noise and latents and are compared with its fp32 results —
    FPS indices exactly, latents / reconstruction / decode by relative MSE (bf16 operands: <= 1e-4)."""
    import ldt_amd
    from oracle import ldt_oracle as O
    torch.set_num_threads(host_cores())
    cfg = ldt_amd.airplane_config(latent_tokens=tokens)
    cc = cfg.compressor
    torch.manual_seed(3)
    comp = ldt_amd.Compressor(cc)
    comp.init()
    sd = {k: v.detach().float().clone() for k, v in comp.state_dict().items()}
    comp = comp.cuda()
    B, nb = 512, 4
    g = torch.Generator().manual_seed(tokens)
    pts = torch.randn(B, 2048, 3, generator=g)
    pts = pts - pts.mean(1, keepdim=True)
    pts = pts / pts.norm(dim=-1).amax(1)[:, None, None]
    noise = [torch.randn(B, tokens, cc.z_dim, generator=g) for _ in range(cc.n_layers)]
    with torch.no_grad():
        ref = O.compressor_encode(sd, cc, pts[:nb], [n[:nb] for n in noise])
        ref_dec = O.compressor_decode(sd, cc, ref["all_eps"])
    out = comp(pts.cuda(), post_noise=[n.cuda() for n in noise])
    assert torch.equal(out["fps_idx"][:nb].cpu().long(), ref["fps_idx"].long())
    assert rel_mse(out["all_eps"][:nb].cpu(), ref["all_eps"]) < 1e-4
    assert rel_mse(out["set"][:nb].cpu(), ref["set"]) < 1e-4
    eps_in = out["all_eps"].clone()
    eps_in[:nb] = ref["all_eps"].cuda()
    dec = comp.sample((B, 2048), given_eps=eps_in)
    assert rel_mse(dec[:nb].cpu(), ref_dec) < 1e-4


def test_fullsize_vipc_conditioned_vs_oracle(full):
    """BASELINE configs[4]'s per-GPU share at the PRODUCTION width (hidden 1024, 16 heads, 24 blocks): B = 32 shapes, T = 32 latent
    tokens, S = 32 condition tokens — per-sample AdaLN rows (c = t_emb + img_cond, score.py:135) and cross-attention to the
    point condition on the even blocks (score.py:148-149), synthetic ConditionNet outputs:
      * teacher-forced Score.forward(condition=(pts_cond, img_cond)) on all 32 samples vs the oracle;
      * 25 free-running ancestral steps of the FUSED conditional loop (ldt_cond_args: AdaLN rows rebuilt in C++ every step, cached
        condition K/V) through Trainer.sample with injected noise: every step's latents + the final ones vs the oracle on the first 8
        samples (trajectories are independent per sample).
    Bars: relative MSE <= 1e-4 (bf16 operands)."""
    import ldt_amd
    O, score = full["O"], full["score"]
    B, T, S, N, nb = 32, 32, 32, 25, 8
    cfg = ldt_amd.airplane_config(latent_tokens=T, sample_N=N)
    z, D = cfg.score.z_dim, cfg.score.hidden_size
    g = torch.Generator().manual_seed(5)
    pts_tm = torch.randn(B, S, D, generator=g)                      # token-major [B,S,hidden]; the reference's is (B,hidden,S)
    img = torch.randn(B, cfg.score.t_dim, generator=g)
    cond_dev = (pts_tm.transpose(1, 2).contiguous().cuda(), img.cuda())
    x = torch.randn(B, T, z, generator=g)
    t = torch.rand(B, generator=g) * 0.98 + 0.01
    out = score(x.cuda(), t.cuda(), condition=cond_dev)
    with torch.no_grad():
        ref = O.score_forward(full["sd_s"], cfg.score, x, t, condition=(pts_tm, img))
        ref_uncond = O.score_forward(full["sd_s"], cfg.score, x[:2], t[:2])
    e_fwd = rel_mse(out.cpu(), ref)
    assert rel_mse(ref[:2], ref_uncond) > 1e-3                      # the condition matters at this size too
    torch.manual_seed(4)
    comp = ldt_amd.Compressor(cfg.compressor)                       # a T = 32 compressor (decode only rides along here)
    comp.init()
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    x0, noises = O.draw_noises(77, B, T, z, N)
    traj = []
    pts, eps = tr.sample(B, condition=cond_dev, x0=x0, noise=torch.stack(noises), trajectory=traj)
    assert pts.shape == (B, cfg.data.tr_max_sample_points, 3) and traj[0].shape == (N, B, T, z)
    sde = O.VPSDE(cfg.sde)
    fn = O.score_fn_from_model(sde, lambda xx, tt: O.score_forward(full["sd_s"], cfg.score, xx, tt, condition=(pts_tm[:nb], img[:nb])))
    rec = []
    with torch.no_grad():
        ref_eps = O.sample_discrete(sde, fn, x0[:nb], [n[:nb] for n in noises], N, record=rec)
    xs = traj[0][:, :nb].cpu()
    curve = [rel_mse(xs[i], rec[i][3]) for i in range(N)]
    e_fin = rel_mse(eps[:nb].cpu(), ref_eps)
    print("full-size ViPC share (B=32, T=32, S=32): teacher-forced %.3e; fused conditional loop per-step max %.3e, final %.3e"
          % (e_fwd, max(curve), e_fin))
    assert e_fwd < 1e-4 and max(curve) < 1e-4 and e_fin < 1e-4, (e_fwd, curve, e_fin)


def test_fused_qkv_attention_256_matches_two_kernel_path(tmp_path):
    """QKV projection + self-attention in one launch at the bench shape (csrc/gemm_256.hip, gemm_qkv_attn256_kernel: 256 x 192 tiles = one
    head of one 256-token sample, the whole-head attention loop as the epilogue) against the QKV GEMM + attention kernel pair it replaces
    (LDT_QKV_ATTN256=0): the same seeded forwards at the production width (hidden 1024, 16 heads; 4 blocks) in two child processes —
    B = 64 with batch-shared modulation (blocks >= 1 LN-folded consumer form, block 0 the plain form with bias) and with per-sample times
    (every block the plain form behind the LayerNorm kernel), B = 16 (256 tiles = one per workgroup) — three forwards each (run-to-run
    differences would betray a race in the q | k | v hand-over or a mis-counted wait).  Same operand rounding (q, k, v to bf16) and the same
    attention loop (attn_tile_joint) on both sides: <= 1e-6 relative MSE (identical up to where the two GEMM kernels order their sums).
    This is the whole-model check; the kernel alone is held per element (float64 bounds, exact probes, bit-equality with the two-kernel path
    on exact operands, guard bands) by tests/test_gpu_fused_attention_exact.py."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    child = r'''
import sys, torch
sys.path.insert(0, %r)
import ldt_amd
cfg = ldt_amd.airplane_config(latent_tokens=256, sample_N=10, **{"score.num_blocks": 4})
torch.manual_seed(3)
comp = ldt_amd.Compressor(cfg.compressor); comp.init()
score = ldt_amd.Trainer(cfg, ldt_amd.Score(cfg.score), comp, "cuda:0").model
outs = {}
for B in (64, 16):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 256, cfg.score.z_dim, generator=g).cuda(); t = (torch.rand(B, generator=g) * 0.98 + 0.01).cuda()
    for name, fn in (("shared", lambda: score.forward_shared_t(x, 0.37)), ("per_sample", lambda: score(x, t))):
        ref = None
        for rep in range(3):
            o = fn().float().cpu()
            assert bool(torch.isfinite(o).all())
            if ref is not None: assert torch.equal(ref, o), "run-to-run difference"
            ref = o
        outs["%%s_%%d" %% (name, B)] = ref
    # which path ran: the fused kernel never writes the q | k | v rows of the workspace
    ws = score._workspace(B, 256)
    ws["QKV"].fill_(7.0)
    score.forward_shared_t(x, 0.37)
    torch.cuda.synchronize()
    outs["qkv_untouched_%%d" %% B] = torch.tensor(float(bool((ws["QKV"] == 7.0).all())))
torch.save(outs, sys.argv[1])
''' % ROOT
    res = {}
    for flag in ("1", "0"):
        out = tmp_path / ("qa%s.pt" % flag)
        r = subprocess.run([sys.executable, "-c", child, str(out)], env=dict(os.environ, LDT_QKV_ATTN256=flag), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = torch.load(out)
    for k in sorted(res["1"]):
        if k.startswith("qkv_untouched"):
            assert float(res["1"][k]) == 1.0 and float(res["0"][k]) == 0.0, (k, res["1"][k], res["0"][k])   # the switch did select the two paths
            continue
        e = rel_mse(res["1"][k], res["0"][k])
        print("fused QKV + attention (256 tokens) vs two kernels, %s: rel. MSE %.2e" % (k, e))
        assert e < 1e-6, (k, e)


def test_fused_cross_attention_matches_two_kernel_path(tmp_path):
    """q projection + cross-attention in one launch (csrc/gemm_mid.hip, mid_epilogue_xattn: 32 queries x 32 condition tokens, head dim 64,
    64 x 64 tiles) against the q GEMM + attention kernel pair it replaces (LDT_Q_XATTN=0), same seeded conditional forward at the production
    width (hidden 1024, 16 heads; 4 blocks: two with cross-attention; B = 8 and 32 samples: 64 and 256 workgroups) in two child processes,
    three forwards each (run-to-run differences would betray a race in the K | V staging or the q tile hand-over).  q is rounded to bf16 in
    both paths and the softmax math is the same; the two attention kernels order their sums differently: <= 1e-6 relative MSE.
    This is the whole-model check; the kernel alone is held per element by tests/test_gpu_fused_attention_exact.py."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    child = r'''
import sys, torch
sys.path.insert(0, %r)
import ldt_amd
cfg = ldt_amd.airplane_config(latent_tokens=32, sample_N=10, **{"score.num_blocks": 4})
torch.manual_seed(3)
comp = ldt_amd.Compressor(cfg.compressor); comp.init()
score = ldt_amd.Trainer(cfg, ldt_amd.Score(cfg.score), comp, "cuda:0").model
outs = {}
for B in (8, 32):
    g = torch.Generator().manual_seed(B)
    D = cfg.score.hidden_size
    cond = (torch.randn(B, D, 32, generator=g).cuda(), torch.randn(B, cfg.score.t_dim, generator=g).cuda())
    x = torch.randn(B, 32, cfg.score.z_dim, generator=g).cuda(); t = (torch.rand(B, generator=g) * 0.98 + 0.01).cuda()
    ref = None
    for rep in range(3):
        o = score(x, t, condition=cond).float().cpu()
        assert bool(torch.isfinite(o).all())
        if ref is not None: assert torch.equal(ref, o), "run-to-run difference"
        ref = o
    outs[B] = ref
torch.save(outs, sys.argv[1])
''' % ROOT
    res = {}
    for flag in ("1", "0"):
        out = tmp_path / ("xattn%s.pt" % flag)
        r = subprocess.run([sys.executable, "-c", child, str(out)], env=dict(os.environ, LDT_Q_XATTN=flag), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[flag] = torch.load(out)
    for B in (8, 32):
        e = rel_mse(res["1"][B], res["0"][B])
        print("fused cross-attention vs two kernels, B = %d: rel. MSE %.2e" % (B, e))
        assert e < 1e-6, (B, e)


def test_fullsize_lnfold_massive_activation_and_row_offset_guard(full):
    """LN folding at the production size under hostile residual streams:
      (a) a "massive activation" channel (ln_in bias + 60 on ONE channel: the classic trained-transformer outlier) inflates a
          row's variance, not its mean / std ratio — the folded path stays within 1e-4 of the oracle;
      (b) a COMMON offset (ln_in bias + 6 on every channel: |mean| ~ 6 std) is what the folded form is sensitive to (error x
          (1 + mean^2 / var)): the monitored probe forward reports mean^2 / var > Score.FOLD_MAX_MEAN_RATIO, folding is
          switched off for the model, and sampling through the LayerNorm kernels stays within 1e-4."""
    import warnings
    O, cfg, score = full["O"], full["cfg"], full["score"]
    B, T, z, nb = 64, 256, cfg.score.z_dim, 4
    g = torch.Generator().manual_seed(33)
    x = torch.randn(B, T, z, generator=g)
    bias0 = score.ln_in.bias.detach().clone()
    sd = dict(full["sd_s"])

    def _setb(v):                                                   # in place THROUGH the parameter: bumps its version -> repack
        with torch.no_grad():
            score.ln_in.bias.copy_(v)

    try:
        # (a) one massive channel
        b = bias0.clone(); b[123] += 60.0
        _setb(b); sd["ln_in.bias"] = b.cpu()
        assert score.can_fold(B, T)
        folded = score.forward_shared_t(x.cuda(), 0.5)
        with torch.no_grad():
            ref = O.score_forward(sd, cfg.score, x[:nb], torch.full((nb,), 0.5))
        e_a = rel_mse(folded[:nb].cpu(), ref)
        # (b) common offset
        b = bias0 + 6.0
        _setb(b); sd["ln_in.bias"] = b.cpu()
        _, mod = score.time_table(torch.tensor([0.5], device="cuda"))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ratio = score.fold_probe(x.cuda(), 0, mod, score.fold_table(mod))
        assert ratio > score.FOLD_MAX_MEAN_RATIO and score._fold_disabled and not score.can_fold(B, T) and len(w) == 1
        out = score.forward_shared_t(x.cuda(), 0.5)                 # now on the LayerNorm kernels
        with torch.no_grad():
            ref_b = O.score_forward(sd, cfg.score, x[:nb], torch.full((nb,), 0.5))
        e_b = rel_mse(out[:nb].cpu(), ref_b)
        forced = score.forward_shared_t(x.cuda(), 0.5, fold=True)   # what folding would have cost here
        e_forced = rel_mse(forced[:nb].cpu(), ref_b)
        print("LN-fold robustness at full size: massive channel folded %.2e; common offset (mean^2/var = %.1f): LayerNorm kernels %.2e, "
              "folding forced %.2e" % (e_a, ratio, e_b, e_forced))
        assert e_a < 1e-4 and e_b < 1e-4
    finally:
        _setb(bias0)
        score._fold_disabled = False
        score.packed()
