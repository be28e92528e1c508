"""GPU (-m gpu): Compressor encoder front end (FPS, kNN, grouping) and Compressor.forward vs oracle / golden.

Index work is exact (FPS index sequence; kNN index sets up to exact-distance ties at the k-th neighbour, which
are compared through their sorted distances).  Floating-point outputs: the bf16 tolerances of test_gpu_path.py."""
import pytest
import torch

from conftest import load_golden, rel_mse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from ldt_amd import ops
    from oracle import ldt_oracle as O
    assert torch.cuda.is_available()
    return ops, O


def unit_clouds(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, n, 3, generator=g)
    p = p - p.mean(1, keepdim=True)
    return p / p.norm(dim=-1).amax(1)[:, None, None]


@pytest.mark.parametrize("B,n,m", [(3, 2048, 256), (2, 2048, 32), (2, 64, 8), (1, 700, 33), (2, 5000, 40), (1, 8, 8)])
def test_fps_exact(mods, B, n, m):
    ops, O = mods
    p = unit_clouds(B, n, n + m)
    ref = O.fps(p, m)
    out = ops.fps(p.cuda(), m)
    assert out.dtype == torch.int32 and torch.equal(out.cpu().long(), ref)


def test_fps_ties_and_start(mods):
    ops, O = mods
    p = torch.zeros(1, 600, 3)
    p[0, 2] = torch.tensor([3., 0, 0]); p[0, 513] = torch.tensor([3., 0, 0])
    assert ops.fps(p.cuda(), 2)[0].tolist() == [0, 513] == O.fps(p, 2)[0].tolist()
    q = torch.tensor([[[0., 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 2, 0]]])
    assert ops.fps(q.cuda(), 4)[0].tolist() == [0, 4, 1, 3]


def test_fps_skip_near_origin(mods):
    """The upstream pointnet2_ops variant: points with |p|^2 <= 1e-3 are never selected and never update their
    distance; ON by default, off = the vendored twin.  GPU == oracle restatement, both switch positions, many clouds at once."""
    ops, O = mods
    g = torch.Generator().manual_seed(4)
    p = torch.randn(6, 700, 3, generator=g) * 0.4
    p[:, 5:300:7] *= 0.02                                   # a band of points inside the 1e-3 ball around the origin
    p[:, 0] = torch.tensor([0.5, 0.1, -0.2])
    assert int(((p ** 2).sum(-1) <= 1e-3).sum()) > 100
    for skip in (False, True):
        ref = O.fps(p, 64, skip_near_origin=skip)
        out = ops.fps(p.cuda(), 64, skip_near_origin=skip)
        assert torch.equal(out.cpu().long(), ref)
    picked = O.gather(p, O.fps(p, 64, skip_near_origin=True))[:, 1:]
    assert float((picked ** 2).sum(-1).min()) > 1e-3       # none of the skipped points was chosen
    assert not torch.equal(O.fps(p, 640), O.fps(p, 640, skip_near_origin=False))          # default = upstream's rule
    assert torch.equal(ops.fps(p.cuda(), 64).cpu().long(), O.fps(p, 64, skip_near_origin=True))         # product default too
    z = torch.zeros(1, 40, 3)                               # every point skipped: the kernel keeps returning index 0
    assert ops.fps(z.cuda(), 5, skip_near_origin=True)[0].tolist() == [0, 0, 0, 0, 0] == O.fps(z, 5, skip_near_origin=True)[0].tolist()


@pytest.mark.parametrize("B,n,S,k", [(2, 2048, 256, 16), (2, 2048, 32, 128), (2, 64, 8, 16), (1, 300, 7, 5), (1, 5000, 10, 64)])
def test_knn_sets(mods, B, n, S, k):
    ops, O = mods
    p = unit_clouds(B, n, S * k)
    cen = O.gather(p, O.fps(p, S))
    ref_d = O.square_distance(cen, p)
    ref_idx = torch.topk(ref_d, k, dim=-1, largest=False, sorted=False)[1]
    idx, dist = ops.knn(p.cuda(), cen.cuda(), k, return_dist=True)
    idx = idx.cpu().long()
    assert float((dist.cpu() - ref_d).abs().max()) < 2e-6                     # same expanded-form distances
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    assert all(len(set(r.tolist())) == k for r in idx.reshape(-1, k))        # k distinct neighbours
    got = torch.gather(ref_d, -1, idx).sort(-1)[0]
    want = torch.gather(ref_d, -1, ref_idx).sort(-1)[0]
    assert torch.allclose(got, want, rtol=1e-5, atol=2e-6)                    # same sets up to k-th-neighbour ties
    same = (idx.sort(-1)[0] == ref_idx.sort(-1)[0]).all(-1).float().mean()
    assert float(same) > 0.98


def test_group_normalize_vs_oracle(mods):
    ops, O = mods
    B, n, D, S, k = 2, 256, 64, 16, 32
    g = torch.Generator().manual_seed(4)
    p = unit_clouds(B, n, 9)
    feat = torch.randn(B, n, D, generator=g)
    alpha = torch.rand(D + 3, generator=g) + 0.5; beta = torch.randn(D + 3, generator=g) * 0.2
    fi = O.fps(p, S); ki = O.knn(k, p, O.gather(p, fi))
    new_feat = O.gather(feat, fi)
    grp = torch.cat([O.gather(feat, ki), O.gather(p, ki)], -1)
    mean = torch.cat([new_feat, O.gather(p, fi)], -1).unsqueeze(-2)
    std = torch.std((grp - mean).reshape(B, -1), dim=-1, keepdim=True)[..., None, None]
    ref = torch.cat([alpha * ((grp - mean) / (std + 1e-5)) + beta, new_feat[:, :, None, :].expand(-1, -1, k, -1)], -1)
    U = ops.group_normalize(feat.cuda(), p.cuda(), fi.int().cuda(), ki.int().cuda(), alpha.cuda(), beta.cuda())
    assert U.shape == (B * S * k, 192)
    assert rel_mse(U[:, :2 * D + 3].float().cpu(), ref.reshape(B * S * k, -1)) < 1e-5
    assert float(U[:, 2 * D + 3:].float().abs().max()) == 0.0               # K padding is zero


def test_small_ops(mods):
    ops, O = mods
    g = torch.Generator().manual_seed(8)
    x = torch.randn(6 * 5, 40, generator=g)
    assert torch.equal(ops.maxpool(x.cuda(), 6, 5).cpu(), x.view(6, 5, 40).max(1)[0])
    xb = x.to(torch.bfloat16)
    assert torch.equal(ops.maxpool(xb.cuda(), 6, 5).cpu(), xb.float().view(6, 5, 40).max(1)[0])
    sh = torch.randn(5 * 40, generator=g); ls = torch.randn(5 * 40, generator=g) * 0.3
    y = ops.actnorm_(x.clone().cuda(), sh.cuda(), ls.cuda(), 6)
    assert rel_mse(y.cpu().view(6, 200), (x.view(6, 200) - sh) * torch.exp(-ls)) < 1e-12
    post = torch.randn(30, 16, generator=g) * 20; nz = torch.randn(30, 8, generator=g)
    out = torch.zeros(30, 24, device="cuda")
    mu, lv = ops.reparam(post.cuda(), nz.cuda(), out[:, 8:16], -30., 10., want_stats=True)
    lvr = post[:, 8:].clamp(-30., 10.)
    assert rel_mse(out[:, 8:16].cpu(), post[:, :8] + torch.exp(lvr / 2.) * nz) < 1e-12
    assert torch.equal(lv.cpu(), lvr) and torch.equal(mu.cpu(), post[:, :8]) and float(out[:, :8].abs().sum()) == 0
    src = torch.randn(2, 9, 4, generator=g); idx = torch.tensor([[8, 0, 3], [1, 1, 7]], dtype=torch.int32)
    assert torch.equal(ops.gather_rows(src.cuda(), idx.cuda()).cpu(), O.gather(src, idx.long()))


def test_chamfer_golden(mods):
    ops, O = mods
    a, _ = load_golden("chamfer")
    dl, dr = ops.chamfer(a["a"].cuda(), a["b"].cuda())
    assert rel_mse(dl.cpu(), a["dl"]) < 1e-10 and rel_mse(dr.cpu(), a["dr"]) < 1e-10


def test_compressor_forward_golden(tiny_cfg):
    """Compressor.forward (encode + reconstruct) with the reference's recorded posterior noise."""
    import ldt_amd
    a, _ = load_golden("compressor_fwd_tiny")
    _, csd = load_golden("trainer_sample_tiny")
    comp = ldt_amd.Compressor(tiny_cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    comp = comp.cuda()
    out = comp(a["pts"].cuda(), post_noise=list(a["post_noise"]), want_stats=True)
    assert torch.equal(out["fps_idx"].cpu().long(), a["fps_idx"].long())
    assert torch.equal(out["knn_idx"].cpu().long().sort(-1)[0], a["knn_idx"].long().sort(-1)[0])
    assert rel_mse(out["tokens"].view(2, 8, -1).cpu(), a["tokens"]) < 1e-4
    mu = torch.stack([p[1] for p in out["posteriors"]]); lv = torch.stack([p[2] for p in out["posteriors"]])
    assert rel_mse(mu.cpu(), a["mu"]) < 1e-3 and rel_mse(lv.cpu(), a["logvar"]) < 1e-3
    assert rel_mse(out["all_eps"].cpu(), a["all_eps"]) < 1e-3
    assert rel_mse(out["set"].cpu(), a["set"]) < 1e-3
    eps2 = comp.encode(a["pts"].cuda(), post_noise=list(a["post_noise"]))
    assert torch.equal(eps2, out["all_eps"])


def test_compressor_forward_near_origin_points_golden(tiny_cfg):
    """Clouds with points inside the |p|^2 <= 1e-3 ball: by default FPS follows upstream pointnet2_ops (never picks them) and the
    encode equals what the reference's Compressor.forward produced with that rule (compressor_fwd_origin.npz); with the
    vendored twin's rule (skip_near_origin off) the centres are the twin's — and different."""
    import ldt_amd
    from ldt_amd import ops
    a, _ = load_golden("compressor_fwd_origin")
    _, csd = load_golden("trainer_sample_tiny")
    comp = ldt_amd.Compressor(tiny_cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    comp = comp.cuda()
    out = comp(a["pts"].cuda(), post_noise=list(a["post_noise"]))
    assert torch.equal(out["fps_idx"].cpu().long(), a["fps_idx"].long())
    assert torch.equal(out["knn_idx"].cpu().long().sort(-1)[0], a["knn_idx"].long().sort(-1)[0])
    assert rel_mse(out["all_eps"].cpu(), a["all_eps"]) < 1e-3 and rel_mse(out["set"].cpu(), a["set"]) < 1e-3
    twin = ops.fps(a["pts"].cuda(), tiny_cfg.compressor.z_scales, skip_near_origin=False).cpu().long()
    assert torch.equal(twin, a["fps_idx_twin"].long()) and not torch.equal(twin, a["fps_idx"].long())


def test_encode_decode_roundtrip_shapes_full_size():
    """Shipped sizes (2048 points, 32 and 256 tokens): encode -> decode runs, finite, deterministic."""
    import ldt_amd
    for T in (32, 256):
        cfg = ldt_amd.airplane_config(latent_tokens=T)
        torch.manual_seed(1)
        comp = ldt_amd.Compressor(cfg.compressor).cuda()
        comp.init()
        pts = unit_clouds(3, 2048, T).cuda()
        torch.manual_seed(2); r1 = comp(pts)
        torch.manual_seed(2); r2 = comp(pts)
        assert r1["all_eps"].shape == (3, T, 120) and r1["set"].shape == (3, 2048, 3)
        assert torch.isfinite(r1["all_eps"]).all() and torch.isfinite(r1["set"]).all()
        assert torch.equal(r1["all_eps"], r2["all_eps"])
        dec = comp.decode(r1["all_eps"], 2048)
        assert rel_mse(dec.cpu(), r1["set"].cpu()) < 1e-6            # decode(all_eps) reproduces the reconstruction


def test_compressor_rng_modes(tiny_cfg):
    """`reference_rng=True` consumes the CPU generator exactly as the reference does — B randperms per InitialSet call
    (quirk Q9, even when every row is kept) then one (B, z, T) randn per level (Network.py:26-29,215-220) — so a seeded run
    equals the run with those draws injected and leaves the generator in the same state.  The default mode keys a
    device-side Philox stream with ONE CPU draw: seeded runs repeat, and explicit noise gives identical results in both."""
    import ldt_amd
    a, _ = load_golden("compressor_fwd_tiny")
    _, csd = load_golden("trainer_sample_tiny")
    comp = ldt_amd.Compressor(tiny_cfg.compressor)
    comp.load_state_dict(csd["c"], strict=True)
    comp = comp.cuda()
    pts = a["pts"].cuda()
    B, T, z, L = pts.shape[0], comp.z_scales, comp.z_dim, comp.n_layers
    comp.reference_rng = True
    torch.manual_seed(42)
    out_ref = comp(pts)["all_eps"]
    state_after = torch.get_rng_state()
    torch.manual_seed(42)
    for _ in range(B):
        torch.randperm(comp.max_outputs)
    noise = [torch.randn((B, z, T)).transpose(1, 2) for _ in range(L)]
    assert torch.equal(torch.get_rng_state(), state_after)
    assert torch.equal(comp(pts, post_noise=noise)["all_eps"], out_ref)
    torch.manual_seed(42)
    comp.sample((B, 64), given_eps=out_ref)
    torch.manual_seed(42)
    for _ in range(B):
        torch.randperm(comp.max_outputs)
    expect_state = torch.get_rng_state()
    torch.manual_seed(42)
    comp.sample((B, 64), given_eps=out_ref)
    assert torch.equal(torch.get_rng_state(), expect_state)
    comp.reference_rng = False
    assert torch.equal(comp(pts, post_noise=noise)["all_eps"], out_ref)          # explicit noise: mode-independent
    torch.manual_seed(7)
    e1 = comp(pts)["all_eps"]
    torch.manual_seed(7)
    e2 = comp(pts)["all_eps"]
    assert torch.equal(e1, e2) and not torch.equal(e1, out_ref) and torch.isfinite(e1).all()
    s0 = torch.get_rng_state()
    comp.sample((B, 64), given_eps=e1)                                          # no idle randperms in the default mode
    assert torch.equal(torch.get_rng_state(), s0)


def cc_gelu(cc):
    import copy
    c = copy.deepcopy(cc)
    c.decoder_act = "gelu"
    return c


def test_compressor_variants_golden(tiny_cfg):
    """`decoder_act` (the decoder blocks' LayerNorm -> activation -> projection path: ldt_block_activation), `ActNorm: ~` and the dead
    `AdaLN: False` flag vs outputs captured from the reference (tests/golden/compressor_variants.npz)."""
    import copy
    import ldt_amd
    from conftest import load_golden, rel_mse
    a, sds = load_golden("compressor_variants")
    cc = copy.deepcopy(tiny_cfg.compressor)
    cc.n_layers, cc.encoder_layers = 2, 1
    for tag, act in (("g", "gelu"), ("l", "leakyrelu0.2"), ("h", "hardswish"), ("r", "anything-else-is-relu")):
        ca = copy.deepcopy(cc); ca.decoder_act = act
        comp = ldt_amd.Compressor(ca)
        comp.load_state_dict(sds["w"], strict=True)
        comp = comp.cuda(); comp.init()
        dec = comp.sample((2, 64), given_eps=a["given_eps"].cuda())
        assert dec.shape == a[tag + "_points"].shape and rel_mse(dec.cpu(), a[tag + "_points"]) < 1e-4, tag
        r = comp(a["pts"].cuda(), post_noise=list(a[tag + "_post_noise"]))
        assert rel_mse(r["all_eps"].cpu(), a[tag + "_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a[tag + "_set"]) < 1e-3, tag
    # the two activations of get_activation (tools/utils.py:104-124) the captured fixture does not hold — SELU and rrelu's eval form —
    # against the oracle (pinned to the reference through the four above): same kernel slot, other constants
    from oracle import ldt_oracle as O
    for act in ("selu", "rrelu"):
        ca = copy.deepcopy(cc); ca.decoder_act = act
        comp = ldt_amd.Compressor(ca)
        comp.load_state_dict(sds["w"], strict=True)
        comp = comp.cuda(); comp.init()
        dec = comp.sample((2, 64), given_eps=a["given_eps"].cuda())
        with torch.no_grad():
            ref = O.compressor_decode({k: v.float() for k, v in sds["w"].items()}, ca, a["given_eps"])
            ref_g = O.compressor_decode({k: v.float() for k, v in sds["w"].items()}, cc_gelu(cc), a["given_eps"])
        assert rel_mse(dec.cpu(), ref) < 1e-4, act
        assert rel_mse(ref, ref_g) > 1e-3, act                                   # the activation matters in this fixture
    cn = copy.deepcopy(cc); cn.ActNorm, cn.AdaLN = None, False
    comp = ldt_amd.Compressor(cn)
    comp.load_state_dict({k: v for k, v in sds["w"].items() if not k.startswith("conv_in.")}, strict=True)
    comp = comp.cuda(); comp.init()
    r = comp(a["pts"].cuda(), post_noise=list(a["n_post_noise"]))
    assert rel_mse(r["all_eps"].cpu(), a["n_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a["n_set"]) < 1e-3


def test_norm_variants_golden(tiny_cfg):
    """`norm: group_norm` / `norm: ~` (tools/utils.py:168-181: ldt_group_stats + ldt_norm_apply instead of the LayerNorm kernels; the Score runs its
    blocks host-driven then) vs outputs captured from the reference: Score forward (plain, with point + image condition), a short sampling loop
    through Trainer.sample vs the oracle, Compressor decode and encode."""
    import copy
    import ldt_amd
    from conftest import load_golden, rel_mse
    from oracle import ldt_oracle as O
    a, sds = load_golden("norm_variants")
    for tag, kind in (("gn", "group_norm"), ("id", None)):
        cfg = copy.deepcopy(tiny_cfg)
        cfg.score.norm = kind
        cfg.compressor.norm = kind
        cfg.compressor.n_layers, cfg.compressor.encoder_layers = 2, 1
        score = ldt_amd.Score(cfg.score)
        score.load_state_dict(sds[tag + "s"], strict=True)
        score = score.cuda()
        out = score(a["x"].cuda(), a["t"].cuda())
        assert rel_mse(out.cpu(), a[tag + "_out"]) < 1e-4, tag
        cond = (a["pts_cond"].transpose(1, 2).contiguous().cuda(), a["img_cond"].cuda())
        out = score(a["x"].cuda(), a["t"].cuda(), condition=cond)
        assert rel_mse(out.cpu(), a[tag + "_out_cond"]) < 1e-4, tag
        comp = ldt_amd.Compressor(cfg.compressor)
        comp.load_state_dict(sds[tag + "c"], strict=True)
        comp = comp.cuda(); comp.init()
        dec = comp.sample((2, 64), given_eps=a["given_eps"].cuda())
        assert rel_mse(dec.cpu(), a[tag + "_points"]) < 1e-4, tag
        r = comp(a["pts"].cuda(), post_noise=list(a[tag + "_post_noise"]))
        assert rel_mse(r["all_eps"].cpu(), a[tag + "_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a[tag + "_set"]) < 1e-3, tag
        # the sampling loop (generic, Python-driven: the fused C++ loop is LayerNorm code) on injected noise vs the oracle
        N = 25                                                                   # (N <= 20 makes beta > 1: the ancestral update is not finite)
        sde_cfg = copy.deepcopy(cfg.sde); sde_cfg.sample_N = N
        B, T, z = 2, cfg.score.z_scale, cfg.score.z_dim
        x0, noises = O.draw_noises(5, B, T, z, N)
        sde = ldt_amd.DiffusionVPSDE(sde_cfg)
        tr = ldt_amd.Trainer(cfg, score, comp, "cuda:0")
        eps = sde.sample_discrete(score_fn=tr.score_fn, num_samples=B, N=N, predictor="ancestral", corrector=None, corrector_steps=1, shape=(T, z),
                                  time_eps=sde_cfg.sample_time_eps, probability_flow=False, denoise=True, snr=0.01, device="cuda:0",
                                  x0=x0, noise=torch.stack(noises))
        osde = O.VPSDE(sde_cfg)
        cs = copy.deepcopy(cfg.score)
        fn = O.score_fn_from_model(osde, lambda xx, tt: O.score_forward(sds[tag + "s"], cs, xx, tt))
        with torch.no_grad():
            ref = O.sample_discrete(osde, fn, x0, noises, N)
        assert bool(torch.isfinite(ref).all()) and rel_mse(eps.cpu(), ref) < 1e-4, tag


def test_compressor_options_golden(tiny_cfg):
    """norm_input + pre_group and the mixture InitialSet (max_outputs None) vs outputs captured from the reference."""
    import copy
    import ldt_amd
    from conftest import load_golden, rel_mse
    a, sds = load_golden("compressor_options")
    cfg = copy.deepcopy(tiny_cfg)
    cfg.compressor.n_layers, cfg.compressor.encoder_layers = 2, 1
    ca = copy.deepcopy(cfg.compressor); ca.norm_input, ca.pre_group = True, True
    ca.max_outputs = ca.outsize = 96
    comp = ldt_amd.Compressor(ca)
    comp.load_state_dict(sds["a"], strict=True)                    # incl. pre_grouper.*: same names, same order as upstream
    comp = comp.cuda(); comp.init()
    r = comp(a["a_pts"].cuda(), post_noise=list(a["a_post_noise"]))
    assert rel_mse(r["all_eps"].cpu(), a["a_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a["a_set"]) < 1e-3
    cb = copy.deepcopy(cfg.compressor); cb.max_outputs = None
    comp = ldt_amd.Compressor(cb)
    comp.load_state_dict(sds["b"], strict=True)
    comp = comp.cuda(); comp.init()
    dec = comp.sample((2, 48), given_eps=a["b_given_eps"].cuda(), seed_eps=a["b_seed_eps"])
    assert dec.shape == a["b_points"].shape and rel_mse(dec.cpu(), a["b_points"]) < 1e-4
    r = comp(a["b_pts"].cuda(), post_noise=list(a["b_post_noise"]), seed_eps=a["b_fwd_seed_eps"])
    assert rel_mse(r["all_eps"].cpu(), a["b_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a["b_set"]) < 1e-3
    # pos_embedding: mlp — every token is modulated by its own AdaLN row (blocks.residual_block per_token)
    cm = copy.deepcopy(cfg.compressor); cm.pos_embedding = "mlp"
    cmod = ldt_amd.Compressor(cm)
    cmod.load_state_dict(sds["c"], strict=True)
    cmod = cmod.cuda(); cmod.init()
    r = cmod(a["c_pts"].cuda(), post_noise=list(a["c_post_noise"]))
    assert rel_mse(r["all_eps"].cpu(), a["c_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a["c_set"]) < 1e-3
    # class_condition: label embedding in the position condition and the (AdaLN) decoder blocks; decode ignores labels
    cl = copy.deepcopy(cfg.compressor); cl.class_condition, cl.num_categorys = True, 5
    cmod = ldt_amd.Compressor(cl)
    cmod.load_state_dict(sds["d"], strict=True)
    cmod = cmod.cuda(); cmod.init()
    r = cmod(a["c_pts"].cuda(), label=a["d_label"].cuda(), post_noise=list(a["d_post_noise"]))
    assert rel_mse(r["all_eps"].cpu(), a["d_all_eps"]) < 1e-3 and rel_mse(r["set"].cpu(), a["d_set"]) < 1e-3
    nolabel = cmod(a["c_pts"].cuda(), post_noise=list(a["d_post_noise"]))
    assert rel_mse(nolabel["all_eps"].cpu(), a["d_all_eps"]) > 1e-3
    assert rel_mse(cmod.sample((2, 64), given_eps=a["b_given_eps"].cuda()).cpu(), a["d_points"]) < 1e-4
    comp.reference_rng = True                                       # the seed rows from a seeded CPU generator, like upstream
    torch.manual_seed(79)
    assert torch.equal(comp.sample((2, 48), given_eps=a["b_given_eps"].cuda()), dec)
    comp.reference_rng = False
    d1 = comp.sample((2, 48), given_eps=a["b_given_eps"].cuda())    # device Philox seed rows: finite, different draw
    assert bool(torch.isfinite(d1).all()) and not torch.equal(d1, dec)


@pytest.mark.parametrize("B,n,S,k", [(2, 512, 24, 32), (17, 256, 40, 16), (1, 64, 3, 32), (3, 512, 7, 16), (2, 2048, 32, 128),
                                     (16, 300, 5, 8), (2, 256, 9, 64)])
def test_fused_grouper_vs_oracle_and_chain(mods, B, n, S, k):
    """The one-kernel grouper (grouping + PreExtraction + neighbour max, D = 128) against the oracle's local_grouper (fp32)
    and against the five-kernel chain it replaces — every tile shape (k = 8 / 16: 4 / 2 groups per MFMA tile, k = 32 m: m tiles
    per group; the shipped encoders use k = 16 and k = 128), both cloud-to-XCD mappings (B < 16: flat), ragged group counts,
    non-trivial BatchNorm statistics."""
    ops, O = mods
    from ldt_amd import compressor as Cm
    D = 128
    torch.manual_seed(100 + B)
    grp = Cm.LocalGrouper(D)
    with torch.no_grad():
        grp.affine_alpha.uniform_(0.5, 1.5); grp.affine_beta.normal_(0, 0.2)
        for bn in (grp.extraction.transfer.net[1], grp.extraction.operation[0].net1[1]):
            bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2)
    sd = {"g." + kk: v.detach().clone() for kk, v in grp.state_dict().items()}
    p = unit_clouds(B, n, 31 + B)
    feat = torch.randn(B, n, D, generator=torch.Generator().manual_seed(B)) * 0.7
    _, ref, fi, ki = O.local_grouper(sd, "g", p, feat, S, k)
    G = grp.cuda().pack()
    assert "wimg" in G
    fused = Cm.run_grouper(G, p.cuda(), feat.cuda(), S, k)
    assert torch.equal(fused[2].cpu().long(), fi.long())
    assert rel_mse(fused[1].view(B, S, D).cpu(), ref) < 1e-4
    try:
        Cm.FUSED_GROUPER = False
        chain = Cm.run_grouper(G, p.cuda(), feat.cuda(), S, k)
    finally:
        Cm.FUSED_GROUPER = True
    # same bf16 operands and roundings, another summation order: equal up to a bf16 ulp on a few elements
    assert rel_mse(fused[1], chain[1]) < 1e-5
    assert float((fused[1] != chain[1]).float().mean()) < 0.25
    # ... and per element: both paths inside the interval of the staged float64 reference (kernel_checks.grouper_staged_reference; the
    # instrument of test_gpu_grouper_exact.py, here on the indices FPS and kNN chose), the kernels' sums within 2^-24 of float64 first
    import kernel_checks as kc
    fd, pd, fid, kid = feat.cuda(), p.cuda(), fused[2], fused[3]
    g = kc.group_reference(fd, pd, fid, kid, G["alpha"], G["beta"], stats_rel=kc.U24)
    st = ops.group_normalize(fd, pd, fid, kid, G["alpha"], G["beta"], return_stats=True)[1].reshape(B, 2)
    assert bool(((st[:, 0] - g["s1"]).abs() <= g["tol1"]).all()) and bool(((st[:, 1] - g["s2"]).abs() <= g["tol2"]).all())
    sr = kc.grouper_staged_reference(g, G["w_pre1"][:, :2 * D + 3].float(), G["b_pre1"], G["w_pre2"][:, :D].float(), G["b_pre2"],
                                     G["w_pre3"][:, :D].float(), G["b_pre3"])
    kc.check_grouper(fused[1], sr, "fused grouper B %d n %d S %d k %d" % (B, n, S, k))
    kc.check_grouper(chain[1], sr, "five-kernel chain B %d n %d S %d k %d" % (B, n, S, k))


@pytest.mark.parametrize("n,S,k,levels", [(2048, 64, 16, 3), (1000, 16, 32, 2), (640, 9, 64, 5), (2048, 8, 16, 40)])
def test_knn_ties_and_crowding(mods, n, S, k, levels):
    """Points on a coarse lattice: masses of exactly equal distances.  The candidate fast path of the kNN select (points at or
    below the k-th smallest per-lane minimum, compacted when there are <= 64) must hand over to the full radix select when
    ties crowd below the threshold, and both must return k distinct neighbours whose sorted distances equal the reference's."""
    ops, O = mods
    g = torch.Generator().manual_seed(n + k)
    p = (torch.randint(0, levels, (2, n, 3), generator=g).float() / levels) - 0.5
    cen = p[:, :S].clone()
    ref_d = O.square_distance(cen, p)
    idx, dist = ops.knn(p.cuda(), cen.cuda(), k, return_dist=True)
    idx = idx.cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    assert all(len(set(r.tolist())) == k for r in idx.reshape(-1, k))
    got = torch.gather(dist.cpu(), -1, idx).sort(-1)[0]
    want = dist.cpu().sort(-1)[0][..., :k]
    assert torch.equal(got, want)                                            # exactly the k smallest distances, ties included
    assert float((dist.cpu() - ref_d).abs().max()) < 2e-6


def test_fps_many_clouds_wave_form(mods):
    """From 512 clouds per call FPS runs one wave per cloud (fps_wave.hip) instead of one 512-thread workgroup: same index sequences
    as the workgroup form (run here on sub-batches), as the oracle on a subset, with ragged point counts, planted ties and both
    settings of skip_near_origin."""
    ops, O = mods
    g = torch.Generator().manual_seed(11)
    for n, m in ((2048, 40), (700, 33), (64, 64)):
        p = torch.randn(520, n, 3, generator=g) * 0.5
        p[:, 5] = p[:, n - 3]                                   # exact duplicates: ties between far-apart indices
        if n > 600:
            p[:, 513] = p[:, 2]
        p[:, 7:40:3] *= 0.01                                    # points inside the 1e-3 ball
        pd = p.cuda()
        for skip in (False, True):
            wave = ops.fps(pd, m, skip_near_origin=skip)
            wg = torch.cat([ops.fps(pd[i:i + 130], m, skip_near_origin=skip) for i in range(0, 520, 130)])
            assert torch.equal(wave, wg)
            assert torch.equal(wave[:6].cpu().long(), O.fps(p[:6], m, skip_near_origin=skip))
