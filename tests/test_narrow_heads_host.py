"""Host checks (no GPU) for the 8- and 16-wide attention heads: the reference's captures against the oracle, the Dh = 8 gather probe and
its planted faults, and the routes the built library reports.  Helpers: tests/narrow_head_checks.py."""
import pytest
import torch

import kernel_checks as kc
import narrow_head_checks as nh


@pytest.fixture(scope="module")
def gold():
    return nh.load_golden()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ldt_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(nh.CAPTURES))
def test_golden_against_the_oracle(gold, name):
    """The weights rebuilt from the seed carry the captured digests, and the fp32 oracle reproduces the reference's Score.forward."""
    score, scfg = nh.rebuild_score(name, gold)
    assert scfg.hidden_size // scfg.num_heads in (8, 16)
    inp = nh.capture_inputs(name, gold)
    assert (inp["pts_cond"] is not None) == nh.CAPTURES[name][4] and (inp["label"] is not None) == (nh.CAPTURES[name][3] > 1)
    with torch.no_grad():
        e = nh.rel_mse(nh.oracle_forward(score, scfg, inp), inp["out"])
    assert e <= 1e-10, e


def test_golden_digest_sees_a_changed_weight(gold):
    import ldt_amd
    scfg, seed = nh.capture_score_cfg("a")
    torch.manual_seed(seed + 1)
    other = ldt_amd.Score(scfg).state_dict()
    k = "Transformer.0.fc_q.weight"
    assert not nh.digest_matches(other[k], gold["a::init_digest::" + k])
    assert nh.digest_matches(other[k], nh.digest(other[k].flip(0).flip(0)))


def test_hybrid_config_is_the_shipped_shape():
    cfg = nh.hybrid_cfg()
    s, c = cfg.score, cfg.compressor
    assert (s.hidden_size, s.num_heads, s.num_blocks, s.t_dim, s.z_scale, s.z_dim) == (128, 16, 24, 128, 32, 120)
    assert (c.hidden_dim, c.num_heads, c.z_scales, c.n_layers * c.z_dim) == (128, 4, 32, 120) and cfg.sde.sde_type == "vpsde"


PROBES = [(2, 16, 32, 32, 8), (2, 3, 8, 5, 8), (2, 2, 72, 24, 8), (1, 16, 256, 256, 8), (1, 2, 300, 77, 8), (2, 4, 33, 65, 16)]


@pytest.mark.parametrize("B,H,Nq,Nk,dh", PROBES)
def test_gather_probe_is_exact_and_sees_planted_faults(B, H, Nq, Nk, dh):
    q, k, v, want, pi = nh.gather_probe(B, H, Nq, Nk, dh, seed=Nq + Nk)
    C = H * dh
    att = lambda kk, vv: kc.bf16_round(kc.attention_ref64(q.view(B * Nq, C), kk.view(B * Nk, C), vv.view(B * Nk, C), B, H, Nq, Nk, dh)[0]).float()
    assert torch.equal(att(k, v), want)                                  # float64 attention == the planted gather
    assert int(pi.min()) >= 0 and int(pi.max()) == Nk - 1
    if H > 1 and Nk >= 4:                                                # the heads of K swapped: another key wins somewhere
        ks = k.view(B, Nk, H, dh).roll(1, 2).reshape(B, Nk, C)
        assert not torch.equal(att(ks, v), want)
    if Nk > 1:                                                           # every key one row late: an off-by-one key index
        assert not torch.equal(att(k.roll(1, 1), v), want)


def test_gather_probe_refuses_more_keys_than_codes():
    assert nh.probe_fits(256, 8) and not nh.probe_fits(600, 8) and nh.probe_fits(600, 16)
    with pytest.raises(AssertionError):
        nh.gather_probe(1, 2, 40, 600, 8, seed=1)


def test_abi_and_routes(lib):
    assert lib.ldt_abi_version() == 26
    for B, H, Nq, Nk, dh in nh.NARROW:
        assert int(lib.ldt_attention_route(B, H, Nq, Nk, dh)) == nh.ROUTE_NARROW, (B, H, Nq, Nk, dh)
    for B, H, Nq, Nk, dh, route in nh.WIDE_ROUTES:
        assert int(lib.ldt_attention_route(B, H, Nq, Nk, dh)) == route, (B, H, Nq, Nk, dh)
    from ldt_amd import ops
    for heads in (16, 8):
        for fold in (0, 32):
            assert ops.qkv_attention_route(64, 32, 128, heads, 128, fold=fold) == 0, (heads, fold)
    assert ops.qkv_attention_route(64, 32, 128, 16, 128, cond_tokens=32) == 0
