"""GPU (-m gpu): attention with 8- and 16-wide heads (csrc/attention_narrow.hip, route 3) and the Score configs that need it — the
reference's hybrid airplane config builds its Score with hidden 128 and 16 heads.  Helpers: tests/narrow_head_checks.py.

The kernel alone, per shape of nh.NARROW: an exact gather, a componentwise bound against float64, operands and output inside larger
buffers, and bit-equal repeats.  Then the public classes: Score.forward against the reference's captures (tests/golden/score_narrow_heads.npz),
the cross-attention step, a free-running sample against the oracle's trajectory, and the shipped shape end to end through HybridTrainer.
Before the narrow kernel existed every test here ended in "head dim 8 not built"."""
import copy

import pytest
import torch

import kernel_checks as kc
import narrow_head_checks as nh

pytestmark = pytest.mark.gpu

SENT_BF16 = -1.7014118e38                           # a bit pattern no kernel under test produces
_REF = {}


def dev(x, dt=None):
    return x.to("cuda", dt) if dt else x.to("cuda")


def _ops():
    from ldt_amd import ops
    return ops


def _route(B, H, Nq, Nk, dh):
    from ldt_amd import _lib
    return int(_lib.lib().ldt_attention_route(B, H, Nq, Nk, dh))


def _randn_case(B, H, Nq, Nk, dh):
    """One randn problem per shape, its float64 reference computed once and shared (read-only) by the tests that need it."""
    key = (B, H, Nq, Nk, dh)
    if key not in _REF:
        g = torch.Generator().manual_seed(Nq * 3 + Nk + dh)
        C = H * dh
        q = torch.randn(B * Nq, C, generator=g).bfloat16(); kv = (torch.randn(B * Nk, 2 * C, generator=g) * 1.5).bfloat16()
        ref, vmax = kc.attention_ref64(q, kv[:, :C], kv[:, C:], B, H, Nq, Nk, dh)
        _REF[key] = (q, kv, ref, vmax)
    return _REF[key]


@pytest.mark.parametrize("B,H,Nq,Nk,dh", [s for s in nh.NARROW if nh.probe_fits(s[3], s[4])])   # (600 keys do not fit the 8 code channels of a Dh = 8 head)
def test_narrow_attention_gather_probe(B, H, Nq, Nk, dh):
    """O is an exact gather of V rows: the key each query selects sits on the edges of the 16-key groups and on a stride."""
    assert _route(B, H, Nq, Nk, dh) == nh.ROUTE_NARROW
    q, k, v, want, _ = nh.gather_probe(B, H, Nq, Nk, dh, seed=Nq + Nk)
    C = H * dh
    out = _ops().attention_fwd(dev(q, torch.bfloat16).view(B * Nq, C), dev(k, torch.bfloat16).view(B * Nk, C), dev(v, torch.bfloat16).view(B * Nk, C),
                               B, H, Nq, Nk, dh)
    kc.assert_elementwise(out.reshape(B * H * Nq, dh), want.double().reshape(B * H * Nq, dh), 0.0,
                          "gather probe, narrow attention B %d H %d Nq %d Nk %d Dh %d (row = (b H + h) Nq + query)" % (B, H, Nq, Nk, dh))
    assert torch.equal(out.cpu().float(), want)


@pytest.mark.parametrize("B,H,Nq,Nk,dh", nh.NARROW)
def test_narrow_attention_bound_vs_float64(B, H, Nq, Nk, dh):
    """randn data: |out - ref| <= 2^-8 |ref| (bf16 output) + 2^-8 max_j |v_j| (P rounded to bf16 before P V), per element."""
    assert _route(B, H, Nq, Nk, dh) == nh.ROUTE_NARROW
    q, kv, ref, vmax = _randn_case(B, H, Nq, Nk, dh)
    C = H * dh
    kvd = dev(kv)
    out = _ops().attention_fwd(dev(q), kvd[:, :C], kvd[:, C:], B, H, Nq, Nk, dh)
    assert out.shape == (B, H, Nq, dh)
    r = kc.assert_elementwise(out.reshape(-1, dh), ref.reshape(-1, dh), kc.attention_base_tol(ref, vmax).reshape(-1, dh),
                              "narrow attention B %d H %d Nq %d Nk %d Dh %d" % (B, H, Nq, Nk, dh))
    print("worst err / tol %.3f (narrow attention B %d H %d Nq %d Nk %d Dh %d)" % (r, B, H, Nq, Nk, dh))


@pytest.mark.parametrize("B,H,Nq,Nk,dh", [s for s in nh.NARROW if s[3] == 600])
def test_narrow_attention_growing_maxima_and_late_spike(B, H, Nq, Nk, dh):
    """Row maxima that grow by 3 (log2 units) with every 32-key step and one key, 30 from the end, that dominates query 5: the running
    maximum is rescaled at every step.  The bars of test_gpu_kernels.py::test_attention_softmax_staircase beside the elementwise bound."""
    assert _route(B, H, Nq, Nk, dh) == nh.ROUTE_NARROW
    q, k, v = nh.staircase_case(B, H, Nq, Nk, dh, step=3.0, seed=dh)
    C = H * dh
    ref, vmax = kc.attention_ref64(q.view(B * Nq, C), k.view(B * Nk, C), v.view(B * Nk, C), B, H, Nq, Nk, dh)
    out = _ops().attention_fwd(dev(q, torch.bfloat16).view(B * Nq, C), dev(k, torch.bfloat16).view(B * Nk, C), dev(v, torch.bfloat16).view(B * Nk, C),
                               B, H, Nq, Nk, dh)
    e, m = nh.rel_mse(out.cpu(), ref), float((out.cpu().double() - ref).abs().max())
    r = kc.assert_elementwise(out.reshape(-1, dh), ref.reshape(-1, dh), kc.attention_base_tol(ref, vmax).reshape(-1, dh),
                              "narrow attention, growing maxima, Nk %d Dh %d" % (Nk, dh))
    print("growing maxima + spike Dh %d: rel-MSE %.3e, max abs %.4f, worst err / tol %.3f" % (dh, e, m, r))
    assert e < 2e-5 and m < 0.05


@pytest.mark.parametrize("B,H,Nq,Nk,dh", nh.NARROW)
def test_narrow_attention_layout_and_repeatability(B, H, Nq, Nk, dh):
    """Q, K, V as interiors of NaN-surrounded buffers with ld > H Dh (K and V in one buffer), O inside a sentinel-filled buffer: the result
    equals the dense call bit for bit and the surround is intact; three launches into fresh buffers agree bit for bit."""
    assert _route(B, H, Nq, Nk, dh) == nh.ROUTE_NARROW
    ops = _ops()
    q, kv, _, _ = _randn_case(B, H, Nq, Nk, dh)
    C = H * dh
    qd, kd, vd = dev(q), dev(kv[:, :C].contiguous()), dev(kv[:, C:].contiguous())
    dense = ops.attention_fwd(qd, kd, vd, B, H, Nq, Nk, dh)
    for _ in range(2):
        assert torch.equal(ops.attention_fwd(qd, kd, vd, B, H, Nq, Nk, dh), dense), "narrow attention: two launches differ"
    qb = torch.full((B * Nq, C + 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    qb[:, 64:64 + C] = qd
    kvb = torch.full((B * Nk, 2 * C + 192), float("nan"), dtype=torch.bfloat16, device="cuda")
    kvb[:, 64:64 + C] = kd; kvb[:, 128 + C:128 + 2 * C] = vd
    n = B * H * Nq * dh
    big = torch.full((n + 512,), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    out = big[256:256 + n].view(B, H, Nq, dh)
    ops.attention_fwd(qb[:, 64:64 + C], kvb[:, 64:64 + C], kvb[:, 128 + C:128 + 2 * C], B, H, Nq, Nk, dh, out=out)
    what = "narrow attention B %d H %d Nq %d Nk %d Dh %d in larger buffers" % (B, H, Nq, Nk, dh)
    sent = torch.full((), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    assert bool((big[:256] == sent).all()) and bool((big[256 + n:] == sent).all()), what + ": wrote outside O"
    assert not bool(torch.isnan(out.float()).any()), what + ": NaN from outside an operand reached the result"
    kc.assert_elementwise(out.reshape(-1, dh), dense.double().reshape(-1, dh), 0.0, what + " vs the dense call")


# ------------------------------------------------------------------------------------------------------------- the public classes
@pytest.fixture(scope="module")
def gold():
    return nh.load_golden()


def _forward(score, inp):
    cond = None
    if inp["pts_cond"] is not None:
        cond = (inp["pts_cond"].cuda(), inp["img_cond"].cuda())
    lab = None if inp["label"] is None else inp["label"].cuda()
    return score(inp["x"].cuda(), inp["t"].cuda(), label=lab, condition=cond)


@pytest.mark.parametrize("name", sorted(nh.CAPTURES))
def test_score_forward_against_the_reference(gold, name):
    """The C++ Score forward (LayerNorm blocks; hidden 128 folds nothing) against the reference's own Score.forward."""
    score, _ = nh.rebuild_score(name, gold)
    score = score.cuda()
    inp = nh.capture_inputs(name, gold)
    e = nh.rel_mse(_forward(score, inp).cpu(), inp["out"])
    print("Score.forward capture %s: rel-MSE %.3e against the reference" % (name, e))
    assert e <= 1e-4


def test_cross_attention_step_equals_its_two_kernels(gold):
    """ops.qkv_attention's cross form on block 0 of capture (c): narrow heads take the two-kernel path, so the result is the q GEMM followed
    by ops.attention_fwd on the condition's K | V rows, bit for bit."""
    from ldt_amd import _lib
    ops = _ops()
    score, scfg = nh.rebuild_score("c", gold)
    score = score.cuda()
    inp = nh.capture_inputs("c", gold)
    B, T, D, H = nh.CAP_B, scfg.z_scale, scfg.hidden_size, scfg.num_heads
    kv, S = score.project_condition(inp["pts_cond"].cuda())
    wq, bq, _, _ = score._cross_panels(0)
    assert S == 24 and ops.qkv_attention_route(B, T, D, H, D, cond_tokens=S) == 0
    g = torch.Generator().manual_seed(5)
    x = dev(torch.randn(B * T, D, generator=g), torch.bfloat16)
    got = ops.qkv_attention(x, wq, B, T, H, bias=bq, kv_cond=kv[0], cond_tokens=S)
    qkv = torch.empty(B * T, 3 * D, dtype=torch.bfloat16, device="cuda")
    q = ops.gemm_bf16(x, wq, bq, _lib.EPI_BF16, out=qkv[:, :D])
    want = ops.attention_fwd(q, kv[0][:, :D], kv[0][:, D:], B, H, T, S, D // H)
    assert torch.equal(got, want)
    ref, vmax = kc.attention_ref64(q.cpu(), kv[0][:, :D].cpu(), kv[0][:, D:].cpu(), B, H, T, S, D // H)
    kc.assert_elementwise(got.cpu().reshape(-1, D // H), ref.reshape(-1, D // H), kc.attention_base_tol(ref, vmax).reshape(-1, D // H), "cross step")


@pytest.mark.parametrize("variant", ["group_norm", "unet"])
def test_host_driven_variants_against_the_oracle(variant):
    """_forward_host_blocks (norm: group_norm) and the U-Net variant reach the narrow kernel through ops.attention_fwd; with a point
    condition on the plain stack (cross-attention on block 0)."""
    import ldt_amd
    over = {"score.num_blocks": 2, "score.norm": "group_norm"} if variant == "group_norm" else {"score.num_blocks": 2, "score.unet": True}
    scfg = nh.hybrid_cfg(**over).score
    torch.manual_seed(41)
    score = ldt_amd.Score(scfg).eval()
    g = torch.Generator().manual_seed(42)
    B = 3
    inp = dict(x=torch.randn(B, scfg.z_scale, scfg.z_dim, generator=g), t=torch.rand(B, generator=g) * 0.9 + 0.05, label=None,
               pts_cond=torch.randn(B, scfg.hidden_size, 24, generator=g) if variant == "group_norm" else None,
               img_cond=torch.randn(B, scfg.t_dim, generator=g) * 0.5 if variant == "group_norm" else None)
    with torch.no_grad():
        ref = nh.oracle_forward(score, scfg, inp)
    e = nh.rel_mse(_forward(score.cuda(), inp).cpu(), ref)
    print("host-driven %s, 16 heads of 8: rel-MSE %.3e against the oracle" % (variant, e))
    assert e <= 1e-4


def test_free_running_sample_against_the_oracle_trajectory(gold):
    """Trainer.sample, injected x0 and noise, B = 4 (the step replayed as a captured graph) on capture (a)'s Score: every recorded step and
    the final latents against the oracle's free-running trajectory.  25 steps, not 20: the ancestral predictor divides by sqrt(1 - beta) with
    beta = beta_end / N at t = 1 (diffusion_continuous.py:152-162), which is 0 at N = 20 for the config's beta_end = 20 — the reference's own
    trajectory is inf from its first step there.  25 is the smallest N the project runs (smoke())."""
    import ldt_amd
    from oracle import ldt_oracle as O
    score, scfg = nh.rebuild_score("a", gold)
    cfg = nh.hybrid_cfg(**{"score.num_blocks": 2, "sde.sample_N": 25, "compressor.max_outputs": 256, "compressor.outsize": 256,
                           "data.tr_max_sample_points": 256})
    assert vars(cfg.score) == vars(scfg)
    torch.manual_seed(2)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    B, N = 4, 25
    x0, noises = O.draw_noises(77, B, scfg.z_scale, scfg.z_dim, N)
    sd = {k: v.detach().clone() for k, v in score.state_dict().items()}
    rec = []
    with torch.no_grad():
        sde = O.VPSDE(cfg.sde)
        fn = O.score_fn_from_model(sde, lambda x, t: O.score_forward(sd, scfg, x, t))
        ref = O.sample_discrete(sde, fn, x0, noises, N, record=rec)
    tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
    traj = []
    pts, eps = tr.sample(B, x0=x0, noise=torch.stack(noises), use_graph=1, trajectory=traj)
    errs = [nh.rel_mse(traj[0][i].cpu(), rec[i][3]) for i in range(N)]
    e = nh.rel_mse(eps.cpu(), ref)
    print("free-running 25 steps, 16 heads of 8: per-step rel-MSE max %.3e (last %.3e), final latents %.3e" % (max(errs), errs[-1], e))
    assert max(errs) <= 1e-4 and e <= 1e-4
    assert pts.shape == (B, 256, 3) and bool(torch.isfinite(pts).all())
    eager = tr.sample(B, x0=x0, noise=torch.stack(noises), use_graph=0)[1]
    assert torch.equal(eager, eps)                                       # graph replay == eager launches


def test_shipped_hybrid_config_end_to_end():
    """HybridTrainer built from the reference's hybrid airplane settings (Score 128 / 16 heads / 24 blocks, the Compressor as configured),
    sample_N cut to 25 (at 20 the ancestral step at t = 1 divides by sqrt(1 - 20 / 20) = 0, in the reference too): sample, val_nelbo,
    Trainer.val_loss, bit-equal repeats and one probability-flow ODE call."""
    import ldt_amd
    cfg = nh.hybrid_cfg(**{"sde.sample_N": 25})
    assert (cfg.score.hidden_size, cfg.score.num_heads, cfg.score.num_blocks, cfg.score.t_dim, cfg.score.z_scale, cfg.score.z_dim) == (128, 16, 24, 128, 32, 120)
    torch.manual_seed(0)
    score = ldt_amd.Score(cfg.score)
    comp = ldt_amd.Compressor(cfg.compressor)
    comp.init()
    hy = ldt_amd.HybridTrainer(cfg, score, comp, "cuda:0")
    torch.manual_seed(12)
    pts = hy.sample(4, seed=99)
    assert pts.shape == (4, 2048, 3) and bool(torch.isfinite(pts).all())
    torch.manual_seed(12)
    again = hy.sample(4, seed=99)
    assert torch.equal(again, pts)
    g = torch.Generator().manual_seed(3)
    clouds = torch.randn(4, 2048, 3, generator=g) * 0.3
    data = {"te_points": clouds, "cate_idx": torch.zeros(4, dtype=torch.long)}
    torch.manual_seed(5)
    res = hy.val_nelbo(data, seed=7)
    assert bool(torch.isfinite(res["kl"])) and bool(torch.isfinite(res["score_term"]))
    torch.manual_seed(5)
    assert torch.equal(hy.val_nelbo(data, seed=7)["kl"], res["kl"])
    torch.manual_seed(5)
    loss = ldt_amd.Trainer.val_loss(hy, data, t_index=[10, 400, 700, 999], seed=7)
    assert loss.shape == () and bool(torch.isfinite(loss))
    print("hybrid config: val_nelbo kl %.4f, val_loss %.4f" % (float(res["kl"]), float(loss)))
    c2 = copy.deepcopy(cfg)
    c2.sde.sample_mode, c2.sde.ode_tol = "continuous", 1e-2
    hy2 = ldt_amd.HybridTrainer(c2, score, comp, "cuda:0")
    torch.manual_seed(4)
    p2 = hy2.sample(2)
    assert p2.shape == (2, 2048, 3) and bool(torch.isfinite(p2).all()) and hy2.nfe_count > 0
