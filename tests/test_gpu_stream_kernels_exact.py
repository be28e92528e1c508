"""GPU (-m gpu): the small streaming kernels of csrc/elementwise.hip, samplers.hip, metrics.hip, pointops.hip, actnorm.hip and eval_loss.hip (reparam), each driven
alone and judged per element, at sizes that make every grid-stride loop take a second (and a partial third) pass.

  EXACT    torch.equal with the reference's expression evaluated in fp32 by torch on the CPU (kernel_checks.*_expr): sampler_step modes 0 / 1
           (injected noise, device step counter, x_mean_out, traj), pndm_transfer, lincomb4 (a contraction to FMA would differ in > 1 % of the
           elements: test_kernel_checks_host.py), add_f32, widen_bf16, cast_pad_bf16, maxpool (NaN propagates), gather_rows, reparam's mu / logvar,
           relu / leaky / rrelu over every bf16 bit pattern.
  PHILOX   philox_normal and sampler_step(noise = None) against the numpy Philox4x32-10 + Box-Muller of kernel_checks.philox_normal_ref, on the
           windows where a grid-stride fault shows (kernel_checks.sweep_windows), with a non-zero high counter word.
  BOUNDED  against float64 with a tolerance derived from the kernel's stated arithmetic: batch_norm_sum, langevin_coef, vpsde_score / sde_score,
           actnorm_, reparam's eps, mixture_seed, norm_points, group_stats + norm_apply, sinusoid, chamfer, chamfer_pairwise, and gelu / silu /
           hardswish / selu over every bf16 bit pattern (bf16 of the float64 definition wherever fp32 resolves a bf16 ulp).

Sizes.  A kernel with a 2048-block cap and 4 floats per thread sweeps 2048 x 256 x 4 floats: N_OVER4 = 4 (2 x 524,288 + 259) floats is two sweeps and
a tail that is no multiple of 256; a scalar kernel with a 4096-block cap sweeps 1,048,576 items: N_OVER1 = 2 x 1,048,576 + 259, or one sweep + 259
where two would pass ~35 MB.  Every kernel is also run at its smallest legal size and at a mid size that is no multiple of 256.  The helpers, an
emulation that passes them and the planted faults that fail them are tested without a GPU in test_kernel_checks_host.py."""
import collections
import time

import numpy as np
import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

ops = None
_lib = None
RATIOS = collections.defaultdict(float)          # worst err / tol per class (test_zz_margins)
SHARES = collections.defaultdict(float)          # worst ambiguous share per class of assert_bf16_of
T0 = [None]

SWEEP4 = 2048 * 256                              # 4-wide kernels, 2048-block cap: vectors per sweep
N_OVER4 = 4 * (2 * SWEEP4 + 259)                 # 4,196,340 floats: crosses the 2048-block cap twice, tail of 259 vectors
SWEEP1 = 4096 * 256                              # scalar kernels, 4096-block cap: items per sweep
N_OVER1 = 2 * SWEEP1 + 259                       # 2,097,411 items
N_OVER1_2048 = 2 * 2048 * 256 + 259              # scalar kernels with a 2048-block cap (add_f32): 1,048,835 items


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops, _lib
    assert torch.cuda.is_available()
    from ldt_amd import _lib as lib_, ops as ops_
    ops, _lib = ops_, lib_
    T0[0] = time.time()
    yield
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def dev(x, dt=None):
    return x.to("cuda", dt) if dt else x.to("cuda")


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS[kind], ratio)
    return ratio


def gen(seed):
    return torch.Generator().manual_seed(seed)


def same(a, b):
    """torch.equal that counts NaN == NaN (where the reference has one, so must the kernel)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------------------- exact: the sampler updates
@pytest.mark.parametrize("n", [4, 1028, N_OVER4])                      # N_OVER4: crosses sampler_step's 2048-block cap (2 sweeps + 259 vectors)
@pytest.mark.parametrize("mode", [0, 1])
def test_sampler_step_exact(mode, n):
    """Both modes bit for bit, with injected noise read at noise_step_stride x the DEVICE step counter (= 1), with and without x_mean_out, and
    the trajectory row of that step."""
    g = gen(100 + mode)
    x, p = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    nz = torch.randn(2, n, generator=g)
    coef = torch.tensor([[9.0, 9.0, 9.0, 9.0], [0.0123, 0.731, (1 - 0.0123) ** 0.5, 0.0123 ** 0.5]] if mode == 0 else
                        [[9.0, 9.0, 9.0, 9.0], [0.99871, -0.01234, 0.05071, 0.0]])
    xm, xn = kc.sampler_step_expr(x, p, nz[1], coef[1], mode)
    ctr = torch.tensor([1], dtype=torch.int32, device="cuda")
    dx, dp, dnz, dcoef = dev(x), dev(p), dev(nz), dev(coef)
    xmd = torch.full((n,), kc.SENT_F32, device="cuda")
    traj = torch.full((2, n), kc.SENT_F32, device="cuda")
    out = ops.sampler_step(dx, dp, dcoef, 0, mode, noise=dnz, noise_step_stride=n, x_mean_out=xmd, step_ptr=ctr, traj=traj)
    assert torch.equal(out.cpu(), xn) and torch.equal(xmd.cpu(), xm)
    assert torch.equal(traj[1].cpu(), xn) and bool((traj[0] == kc.SENT_F32).all())
    out2 = ops.sampler_step(dx, dp, dcoef, 0, mode, noise=dnz, noise_step_stride=n, step_ptr=ctr)          # x_mean_out null, no traj
    assert torch.equal(out2.cpu(), xn)
    out3 = ops.sampler_step(dx, dp, dcoef, 1, mode, noise=dnz, noise_step_stride=n)                        # the host step
    assert torch.equal(out3.cpu(), xn)


@pytest.mark.parametrize("n", [4, 1028, N_OVER4])                      # N_OVER4: crosses the 2048-block cap of pndm_transfer / lincomb4
def test_pndm_transfer_and_lincomb4_exact(n):
    g = gen(7)
    x, et = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    d, p, q = -0.0021, 0.5013, 7.913
    want = kc.pndm_transfer_expr(x, et, d, p, q)
    assert torch.equal(ops.pndm_transfer(dev(x), dev(et), d, p, q).cpu(), want)
    a = [torch.randn(n, generator=g) for _ in range(4)]
    da = [dev(t) for t in a]
    for c, s in kc.PNDM_COEF_SETS:
        assert torch.equal(ops.lincomb4(da, c, s).cpu(), kc.lincomb4_expr(a, c, s)), c
    if n == 1028:                                                      # out of place into a guard band
        big, view = kc.guarded(1, n, 0.0, "cuda")
        ops.pndm_transfer(dev(x), dev(et), d, p, q, out=view[0])
        assert torch.equal(view[0].cpu(), want)
        kc.assert_guard_intact(big, n, "pndm_transfer")
        big, view = kc.guarded(1, n, 0.0, "cuda")
        c, s = kc.PNDM_COEF_SETS[0]
        ops.lincomb4(da, c, s, out=view[0])
        assert torch.equal(view[0].cpu(), kc.lincomb4_expr(a, c, s))
        kc.assert_guard_intact(big, n, "lincomb4")


def test_pndm_entries_refuse_bad_arguments():
    x = torch.zeros(8, device="cuda")
    lib = _lib.lib()
    assert lib.ldt_pndm_transfer(x.data_ptr(), x.data_ptr(), 0.0, 0.0, 0.0, x.data_ptr(), 6, None) == -3          # n % 4
    assert lib.ldt_pndm_transfer(x.data_ptr() + 4, x.data_ptr(), 0.0, 0.0, 0.0, x.data_ptr(), 4, None) == -3      # misaligned
    assert lib.ldt_lincomb4(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1.0, 1.0, 1.0, 1.0, 1.0, x.data_ptr(), 8, None) == -1
    with pytest.raises(ValueError):
        ops.pndm_transfer(x, x[:4], 0.0, 0.0, 0.0)
    with pytest.raises(TypeError):
        ops.lincomb4([x, x, x, x.double()], (1, 1, 1, 1), 1.0)
    with pytest.raises(_lib.LdtHipError):
        ops.pndm_transfer(x.cpu(), x.cpu(), 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------- exact: copies, casts, selections
@pytest.mark.parametrize("n", [1, 259, N_OVER1_2048])                  # N_OVER1_2048: crosses add_f32's 2048-block cap (scalar: 524,288 per sweep)
def test_add_f32_exact_and_aliased(n):
    g = gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    da = dev(a)
    assert torch.equal(ops.add_f32(da, dev(b)).cpu(), a + b)
    ops.add_f32(da, dev(b), out=da)                                    # out aliases a
    assert torch.equal(da.cpu(), a + b)


@pytest.mark.parametrize("n", [1, 259, N_OVER1])                       # N_OVER1: crosses widen_bf16's 4096-block cap
def test_widen_bf16_exact(n):
    w = torch.randn(n, generator=gen(n)).bfloat16()
    if n >= 65536:
        w[:65536] = kc.all_bf16_patterns().reshape(-1)
    got = ops.widen_bf16(dev(w)).cpu()
    assert same(got, w.float())


@pytest.mark.parametrize("rows,cols,cols_pad", [(1, 1, 4), (259, 7, 8), (16400, 253, 256)])       # 16,400 x 64 vectors: crosses cast_pad's 2048-block cap
def test_cast_pad_bf16_exact(rows, cols, cols_pad):
    srcbig = torch.randn(rows, cols + 3, generator=gen(rows))
    src = srcbig[:, :cols]                                             # a row-strided source
    guard = 4096
    big = torch.full((rows * cols_pad + 2 * guard,), 7.0, dtype=torch.bfloat16, device="cuda")
    out = big[guard:guard + rows * cols_pad].view(rows, cols_pad)
    ops.cast_pad_bf16(dev(srcbig)[:, :cols], cols_pad, out=out)
    got = out.cpu()
    assert torch.equal(got[:, :cols], src.bfloat16())
    assert bool((got[:, cols:].float() == 0).all())                    # the pad columns
    assert bool((big[:guard].float() == 7.0).all()) and bool((big[guard + rows * cols_pad:].float() == 7.0).all())


MAXPOOL_CASES = [(3, 1, 5, 5), (7, 5, 33, 33), (7, 5, 33, 40), (8200, 2, 128, 128)]               # (G, n, C, ld); 8200 x 128: crosses maxpool's 4096-block cap


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G,n,C,ld", MAXPOOL_CASES)
def test_maxpool_exact(G, n, C, ld, dtype):
    """A row-strided view (ld > C), a group that is all -inf, and NaN: the reference's adaptive_max_pool1d / torch.max propagate it."""
    big = torch.randn(G * n, ld, generator=gen(G + n)).to(dtype)
    big[0:n, 0] = float("-inf")                                        # group 0, column 0: all -inf
    if G > 1:
        big[n, C - 1] = float("nan")                                   # group 1: first row NaN
        big[3 * n - 1, 0] = float("nan")                               # group 2: last row NaN
    view = big[:, :C]
    want = kc.maxpool_expr(view, G, n)
    got = ops.maxpool(dev(big)[:, :C], G, n).cpu()
    assert float(got[0, 0]) == float("-inf")
    if G > 1:
        assert bool(torch.isnan(got[1, C - 1])) and bool(torch.isnan(got[2, 0])), "maxpool dropped a NaN"
    assert same(got, want)


@pytest.mark.parametrize("B,S,C,n", [(1, 1, 1, 1), (2, 37, 7, 50), (2, 4100, 128, 50)])           # 2 x 4100 x 128: crosses gather_rows's 4096-block cap
def test_gather_rows_exact(B, S, C, n):
    g = gen(S)
    src = torch.randn(B, n, C, generator=g)
    idx = torch.randint(0, n, (B, S), generator=g)
    idx[:, 0] = n - 1; idx[:, -1] = 0
    if S > 4:
        idx[:, 1] = idx[:, 2] = n // 2                                 # repeated
    want = torch.gather(src, 1, idx[:, :, None].expand(-1, -1, C))
    assert torch.equal(ops.gather_rows(dev(src), dev(idx.int())).cpu(), want)


@pytest.mark.parametrize("rows,z,ldo", [(1, 1, 1), (37, 7, 12), (52500, 20, 28)])                 # 52,500 x 20: crosses reparam's 4096-block cap
def test_reparam_exact_stats_and_bounded_eps(rows, z, ldo):
    g = gen(rows)
    lo, hi = -4.0, 2.5
    post, nz = torch.randn(rows, 2 * z, generator=g) * 3, torch.randn(rows, z, generator=g)
    up, dn = lambda v: float(np.nextafter(np.float32(v), np.float32(99))), lambda v: float(np.nextafter(np.float32(v), np.float32(-99)))
    edge = torch.tensor([lo, up(lo), dn(lo), hi, dn(hi), up(hi)])      # exactly at, just inside and just outside both clamps
    k = min(edge.numel(), rows * z)
    flat = post[:, z:].clone().reshape(-1); flat[:k] = edge[:k]; post[:, z:] = flat.reshape(rows, z)
    mu, lv, ref, tol = kc.reparam_ref(post, nz, lo, hi)
    big = torch.full((rows, ldo), kc.SENT_F32, device="cuda")
    out = big[:, ldo - z:]
    gmu, glv = ops.reparam(dev(post), dev(nz), out, lo, hi, want_stats=True)
    assert torch.equal(gmu.cpu(), mu) and torch.equal(glv.cpu(), lv)
    note("reparam eps (expf)", kc.assert_elementwise(out.cpu(), ref, tol, "reparam eps"))
    assert bool((big[:, :ldo - z] == kc.SENT_F32).all())
    out2 = torch.empty(rows, z, device="cuda")
    assert ops.reparam(dev(post), dev(nz), out2, lo, hi) == (None, None) and torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------------------- block activations
@pytest.mark.parametrize("kind", sorted(kc.BLOCK_ACT_KINDS))
def test_block_activation_every_bf16_pattern(kind):
    x = kc.all_bf16_patterns()
    out = ops.block_activation_(dev(x.clone()), kc.BLOCK_ACT_KINDS[kind]).cpu()
    assert bool(torch.isnan(out.float()[torch.isnan(x.float())]).all()), "a NaN input must give NaN"
    ratio, share = kc.check_block_act(out, x, kind, kind)
    note("block_activation %s, unresolved tail" % kind, ratio)
    SHARES["block_activation " + kind] = max(SHARES["block_activation " + kind], share)
    want = {"gelu": (float("inf"), float("nan")), "silu": (float("inf"), float("nan")), "relu": (float("inf"), 0.0), "leakyrelu": (float("inf"), -float("inf")),
            "leakyrelu0.2": (float("inf"), -float("inf")), "rrelu": (float("inf"), -float("inf")), "hardswish": (float("inf"), float("nan")),
            "selu": (float("inf"), float(torch.tensor(-kc.SELU_SCALE * kc.SELU_ALPHA).bfloat16()))}[kind]      # the formula in IEEE arithmetic: 0 x inf = NaN
    got = out.reshape(-1)[[0x7F80, 0xFF80]].float()                    # the flat index is the bit pattern: +inf, -inf
    assert same(got, torch.tensor(want)), (kind, got.tolist())


@pytest.mark.parametrize("kind", sorted(kc.BLOCK_ACT_KINDS))
def test_block_activation_strided_over_the_cap(kind):
    """[21,850, 96] in rows of 104: 2,097,600 elements cross block_act's 4096-block cap twice; the 8 spare columns stay untouched."""
    M, C, ld = 21850, 96, 104
    pat = kc.all_bf16_patterns().reshape(-1)
    x = pat[(torch.arange(M * C) * 7 + 3) % 65536].reshape(M, C)
    big = torch.full((M, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    big[:, :C] = dev(x)
    ops.block_activation_(big[:, :C], kc.BLOCK_ACT_KINDS[kind])
    assert bool((big[:, C:].float() == 7.0).all())
    ratio, share = kc.check_block_act(big[:, :C].contiguous(), dev(x), kind, kind + " strided")
    note("block_activation %s, unresolved tail" % kind, ratio)
    SHARES["block_activation " + kind] = max(SHARES["block_activation " + kind], share)


# ------------------------------------------------------------------------------------------------------------- Philox
def _check_stream(out, seed, stream, first_vec, what):
    n_vec = out.numel() // 4
    win = kc.sweep_windows(n_vec, 256, 2048, 256)
    got = out.reshape(n_vec, 4).cpu()
    worst = 0.0
    for a, b in win:
        ref, tol = kc.philox_normal_ref(seed, stream, first_vec + a, b - a)
        worst = max(worst, kc.assert_elementwise(got[a:b], ref, tol, "%s vectors %d..%d" % (what, a, b)))
    return note("philox normal stream (logf, sincosf)", worst)


@pytest.mark.parametrize("elem_offset", [0, 2 ** 34 + 8])              # a counter only (no memory there): the high counter word becomes 4
@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("n", [4, N_OVER4])                            # N_OVER4: crosses philox_normal's 2048-block cap
def test_philox_normal_stream(n, step, elem_offset):
    seed = 0x9E3779B97F4A7C15                                          # both key words non-zero and different
    out = ops.philox_normal((n,), "cuda", seed=seed, step=step, elem_offset=elem_offset)
    _check_stream(out, seed, step, elem_offset // 4, "philox_normal")
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("n", [4, N_OVER4])
def test_sampler_step_draws_the_stream_of_its_id(n):
    """noise = None, coef (1, 0, 1, 0), x = params = 0: x_next = 0 + 1 z is the stream itself, at id step * philox_mul + philox_add = 5 * 3 + 2."""
    seed, off = 0x0123456789ABCDEF, 2 ** 34 + 8
    z = torch.zeros(n, device="cuda")
    coef = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 6, device="cuda")
    ctr = torch.tensor([5], dtype=torch.int32, device="cuda")
    out = ops.sampler_step(z, z, coef, 0, 1, step_ptr=ctr, elem_offset=off, seed=seed, philox_mul=3, philox_add=2)
    _check_stream(out, seed, 17, off // 4, "sampler_step")
    assert torch.equal(out, ops.philox_normal((n,), "cuda", seed=seed, step=17, elem_offset=off))


# ------------------------------------------------------------------------------------------------------------- bounded: Langevin
@pytest.mark.parametrize("B,per", [(1, 4), (3, 4), (70, 4), (1, 3092), (3, 3092), (70, 3092), (1, 245760), (3, 245760), (33, 245760)])
def test_batch_norm_sum_bounded(B, per):
    """(70 x 245,760 floats would be 69 MB: the largest batch at that size is 33, 32 MB.)  B = 70 takes norm_sum's second pass, 245,760 240 per lane."""
    x = torch.randn(B, per, generator=gen(B + per)) * 2
    n, s, tn, ts = kc.batch_norms_ref(x)
    norms, tot = torch.zeros(B, device="cuda"), torch.zeros(1, device="cuda")
    ops.batch_norm_sum(dev(x), B, per, norms, tot)
    note("batch_norm_sum norms", kc.assert_elementwise(norms.cpu(), n, tn, "batch norms"))
    note("batch_norm_sum sum", kc.assert_elementwise(tot.cpu(), s.reshape(1), ts.reshape(1), "norm sum"))


@pytest.mark.parametrize("snr,std", [(0.16, 0.7), (0.01, 1e-3), (0.2, 0.999), (1.0, 0.05)])
def test_langevin_coef_bounded(snr, std):
    sums = torch.tensor([123.4, 250.1])
    out = torch.full((4,), 9.0, device="cuda")
    ops.langevin_coef(dev(sums), 3, snr, std, out)
    ref, tol = kc.langevin_coef_ref(sums, 3, snr, std)
    note("langevin_coef", kc.assert_elementwise(out.cpu(), ref, tol, "langevin_coef"))


SDE_CONSTS = {0: ((0.1, 20.0, 0.0), (0.1, 20.0, 1e-3)), 1: ((0.1, 20.0, 1e-3), (0.1, 20.0, 0.0)), 2: ((1e-4, 5e5, 1e-4), (0.01, 2500.0, 0.01))}


@pytest.mark.parametrize("per", [96, 132108])                          # 132,108 = 4 (2 x 64 x 256 + 259): strides past the 64-block cap, with a tail
@pytest.mark.parametrize("kind", [-1, 0, 1, 2])                        # -1: ldt_vpsde_score
def test_sde_score_bounded(kind, per):
    """Every sample reads its own t.  Where fp32 cannot resolve var (sde_score_ref: t = 1e-6 with sigma2_0 = 0) only a non-NaN result is asked."""
    t = torch.tensor([1.0, 0.5, 0.25, 1e-3, 1e-6])
    p = torch.randn(5, per, generator=gen(per + kind))
    for cs in SDE_CONSTS[max(kind, 0)]:
        ref, tol, res = kc.sde_score_ref(p, t, max(kind, 0), *cs)
        assert bool(res[:3].all()) and (cs[2] == 0 or bool(res.all()))
        got = (ops.vpsde_score(dev(p), dev(t), *cs) if kind < 0 else ops.sde_score(dev(p), dev(t), kind, *cs)).cpu()
        name = "vpsde_score (expf)" if kind < 0 else "sde_score kind %d (%s)" % (kind, "powf" if kind == 2 else "expf")
        note(name, kc.assert_elementwise(got[res], ref[res], tol[res], name))
        assert not bool(torch.isnan(got).any())


# ------------------------------------------------------------------------------------------------------------- bounded: encoder helpers
@pytest.mark.parametrize("B,per", [(1, 1), (3, 259), (5, 209767)])     # 5 x 209,767 = 1,048,835: crosses actnorm's 4096-block cap
def test_actnorm_bounded(B, per):
    g = gen(per)
    x, sh, ls = torch.randn(B, per, generator=g), torch.randn(per, generator=g), torch.randn(per, generator=g) * 0.5
    ref, tol = kc.actnorm_ref(x, sh, ls)
    got = ops.actnorm_(dev(x.clone()), dev(sh), dev(ls), B).cpu()
    note("actnorm (expf)", kc.assert_elementwise(got, ref, tol, "actnorm"))


@pytest.mark.parametrize("n_mix,logits", [(1, [0.0]), (3, [0.5, 0.5, 0.5]), (8, [0.3, -1.0, 2.0, 0.0, 1.5, -2.5, 0.7, 0.1]), (3, [0.0, 160.0, -3.0]), (8, [0.0] * 8)])
def test_mixture_seed_bounded(n_mix, logits):
    g = gen(n_mix)
    rows, D = (8195, 128) if n_mix == 1 else (37, 7)                   # 8,195 x 128 = 1,048,960: crosses mixture_seed's 4096-block cap
    eps, sig, mu = torch.randn(rows, n_mix, D, generator=g), torch.rand(n_mix, D, generator=g) + 0.1, torch.randn(n_mix, D, generator=g)
    lg = torch.tensor(logits)
    ref, tol = kc.mixture_seed_ref(eps, sig, mu, lg)
    got = ops.mixture_seed(dev(eps), dev(sig), dev(mu), dev(lg)).cpu()
    note("mixture_seed (expf)", kc.assert_elementwise(got, ref, tol, "mixture_seed"))


def test_mixture_seed_refuses_nine_components():
    t = torch.zeros(9 * 4, device="cuda")
    assert _lib.lib().ldt_mixture_seed(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 9, 4, 1, t.data_ptr(), None) == -2


@pytest.mark.parametrize("n", [2, 255, 257, 2048, 5000])
def test_norm_points_bounded(n):
    xyz = torch.randn(3, n, 3, generator=gen(n))
    xyz[1] = xyz[1] * 0.01 + 100.0                                     # a cloud far from the origin: the bound carries u |mean| / std
    ref, tol = kc.norm_points_ref(xyz)
    note("norm_points", kc.assert_elementwise(ops.norm_points(dev(xyz)).cpu(), ref, tol, "norm_points"))


@pytest.mark.parametrize("T", [7, 33, 300])                            # 300 x C / G = 600 .. 2,400 values per group: past group_stats's 256 lanes
@pytest.mark.parametrize("C,G", [(32, 8), (24, 6), (128, 16)])
def test_group_stats_and_norm_apply(C, G, T):
    g = gen(C + T)
    B, ldx = 3, C + 4
    xb = torch.randn(B * T, ldx, generator=g) * 2 + 0.3
    x = xb[:, :C]
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    sh, sc = torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
    dx = dev(xb)[:, :C]
    stats = ops.group_stats(dx, B, T, G, 1e-6)
    ref, tol = kc.group_stats_ref(x, B, T, C, G, 1e-6)
    note("group_stats", kc.assert_elementwise(stats.cpu(), ref, tol, "group_stats"))
    st = stats.cpu()
    for kw in (dict(), dict(w=w, b=b), dict(shift=sh, scale=sc), dict(w=w, b=b, shift=sh, scale=sc)):
        dkw = {k: dev(v) for k, v in kw.items()}
        y = ops.norm_apply(dx, stats, T, mod_sample_stride=C, rows_per_sample=T, **dkw)
        pre, acc = kc.norm_apply_ref(x, st, T, rows_per_sample=T, **kw)
        SHARES["norm_apply"] = max(SHARES["norm_apply"], kc.assert_bf16_of(y.cpu(), pre, acc, "norm_apply %s" % sorted(kw)))
    y = ops.norm_apply(dx, None, w=dev(w), b=dev(b))                   # the identity norm
    pre, acc = kc.norm_apply_ref(x, None, w=w, b=b)
    kc.assert_bf16_of(y.cpu(), pre, acc, "identity norm + affine")
    assert torch.equal(ops.norm_apply(dx).cpu(), x.bfloat16())


def test_norm_apply_over_the_cap():
    """M = 1,048,835 rows of C = 4: one vector per row, crosses norm_apply's 4096-block cap (1,048,576 vectors per sweep)."""
    M, C = SWEEP1 + 259, 4
    g = gen(1)
    x = torch.randn(M, C, generator=g)
    stats = torch.stack([torch.randn(M // 5 + 1, 2, generator=g) * 0.1, torch.rand(M // 5 + 1, 2, generator=g) + 0.5], -1)      # [S, G = 2, 2]
    y = ops.norm_apply(dev(x), dev(stats), 5)
    pre, acc = kc.norm_apply_ref(x, stats, 5)
    SHARES["norm_apply"] = max(SHARES["norm_apply"], kc.assert_bf16_of(y.cpu(), pre, acc, "norm_apply over the cap"))


@pytest.mark.parametrize("half", [5, 128, 130])                        # 130: past sinusoid's 128 threads per row, a second pass of 2
def test_sinusoid_bounded(half):
    """Score feeds the SDE time itself, t in [time_eps, 1] (score.py time_embedding / time_table: no scale), and the frequencies are <= 1."""
    t = torch.cat([torch.tensor([1.0, 0.5, 1e-2, 1e-3, 1e-6, 0.9999999]), torch.rand(31, generator=gen(half))])
    fr = torch.exp(torch.arange(half) * -(np.log(10000) / (half - 1))).float()
    ref, tol = kc.sinusoid_ref(t, fr)
    note("sinusoid (sincosf)", kc.assert_elementwise(ops.sinusoid(dev(t), dev(fr)).cpu(), ref, tol, "sinusoid"))


# ------------------------------------------------------------------------------------------------------------- bounded: Chamfer
@pytest.mark.parametrize("na,nb", [(300, 1100), (1100, 300), (1, 1)])
def test_chamfer_bounded(na, nb):
    g = gen(na)
    a, b = dev(torch.randn(3, na, 3, generator=g) * 0.5), dev(torch.randn(3, nb, 3, generator=g) * 0.5 + 0.1)
    (dl, tl), (dr, tr) = kc.chamfer_ref(a, b)
    gl, gr = ops.chamfer(a, b)
    note("chamfer", kc.assert_elementwise(gl, dl, tl, "chamfer dl"))
    note("chamfer", kc.assert_elementwise(gr, dr, tr, "chamfer dr"))


@pytest.mark.parametrize("n,m", [(1030, 2050), (2050, 1030)])          # crosses the 1024-point LDS chunk and the 1024-query sweep, both ways
def test_chamfer_pairwise_bounded(n, m):
    g = gen(n)
    x, y = dev(torch.randn(2, n, 3, generator=g) * 0.5), dev(torch.randn(3, m, 3, generator=g) * 0.5 + 0.1)
    ref, tol = kc.chamfer_pairwise_ref(x, y)
    note("chamfer_pairwise", kc.assert_elementwise(ops.chamfer_pairwise(x, y), ref, tol, "chamfer_pairwise"))


def test_zz_margins():
    """Printed last (DESIGN.md section 3 quotes them): the worst err / tol per class with the libm constants of kernel_checks.LIBM, and the worst
    share of elements that assert_bf16_of had to treat as ambiguous."""
    print("libm constants (ulps): %s" % ", ".join("%s %g" % kv for kv in sorted(kc.LIBM.items())))
    for k in sorted(RATIOS):
        print("worst err / tol, %-52s %.3f" % (k + ":", RATIOS[k]))
    for k in sorted(SHARES):
        print("ambiguous share, %-52s %.5f" % (k + ":", SHARES[k]))
    if T0[0] is not None:
        print("module run time %.1f s" % (time.time() - T0[0]))
    assert all(v <= 1.0 for v in RATIOS.values()) and all(v <= kc.AMBIGUOUS_CAP for v in SHARES.values())
