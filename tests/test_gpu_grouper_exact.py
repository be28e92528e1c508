"""GPU (-m gpu): the grouping kernels (csrc/pointops.hip: group_stats_vec / group_stats / group_mean / group_build, entry ldt_group_normalize) and the one-kernel grouper
(csrc/grouper_mlp.hip) driven alone on CRAFTED indices — no FPS or kNN in the loop — and judged per element.

  (1) ldt_group_normalize: the per-cloud sums against float64 at a tolerance derived from the kernels' summation; every normalised element inside
      [bf16(pre - a), bf16(pre + a)] of a float64 reference (pinned to the bit where the two ends agree: at least 98 % of every case); anchor
      columns, K padding, alpha = 0 and a cloud without spread bit for bit.  Both vector statistics kernels, the scalar one, both modes, k not a
      multiple of the rows in flight, grid-stride loops of the statistics and the build kernel.
  (2) ops.grouper_mlp on every template / mapping of its launcher (ROUTES): (a) a signed selection in W1 with layers 2 and 3 switched off —
      torch.equal with the max over ops.group_normalize's rows, the winning neighbour planted in every slot; (b) integers through all three
      layers and the residual — torch.equal with float64; (c) randn data inside the interval of a staged float64 reference that rounds where the
      kernel rounds; (d) three launches bit-equal, `out` pre-filled (NaN, or a large value where the launcher must zero it) inside a sentinel
      surround that stays intact, and the five-kernel chain inside the same interval.
The helpers, an emulation that passes them and six planted faults that fail them are tested without a GPU in test_kernel_checks_host.py."""
import collections
import time

import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

ops = None
Cm = None
EPI_RELU_BF16 = None
ROWS_SEEN, GROUPER_SEEN, T0 = {}, {}, [None]


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops, Cm, EPI_RELU_BF16
    assert torch.cuda.is_available()
    from ldt_amd import _lib, compressor, ops as _ops
    ops, Cm, EPI_RELU_BF16 = _ops, compressor, _lib.EPI_RELU_BF16
    torch.backends.cuda.matmul.allow_tf32 = False
    T0[0] = time.time()
    yield
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def dev(c):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}


def rows_of(c, mode="anchor", alpha=None, stats=True):
    return ops.group_normalize(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"] if alpha is None else alpha, c["beta"], normalize=mode, return_stats=stats)


# ------------------------------------------------------------------------------------------------------------- (1) statistics and grouped rows
# mode, D, B, n, S, k.  D = 128 / 64 'anchor': the vector statistics kernels (2 / 4 rows in flight per wave); any other D and 'center': the scalar
# one.  S = 300 > 4 x 64 workgroup waves: the statistics kernel's grid-stride loop; S k > 1024 rows: the build kernel's.
GROUP_CASES = [
    ("anchor", 128, 3, 600, 300, 8), ("anchor", 128, 3, 256, 3, 128), ("anchor", 128, 3, 64, 1, 5), ("anchor", 128, 4, 300, 3, 32), ("anchor", 128, 3, 300, 40, 16),
    ("anchor", 64, 3, 600, 300, 5), ("anchor", 64, 3, 256, 3, 128), ("anchor", 64, 3, 128, 1, 16), ("anchor", 64, 3, 256, 40, 32), ("anchor", 64, 3, 200, 3, 8),
    ("anchor", 20, 3, 300, 300, 5), ("anchor", 20, 3, 100, 3, 16), ("anchor", 32, 3, 200, 1, 128), ("anchor", 32, 3, 200, 40, 32), ("anchor", 20, 3, 100, 3, 8),
    ("center", 128, 3, 600, 300, 8), ("center", 128, 3, 256, 3, 128), ("center", 128, 3, 64, 1, 5), ("center", 64, 3, 256, 40, 32), ("center", 20, 3, 100, 3, 16),
]


@pytest.mark.parametrize("mode,D,B,n,S,k", GROUP_CASES)
def test_group_rows_and_statistics(mode, D, B, n, S, k):
    """Clouds of scale 1, 1.5, 2 (...); 'anchor' cases carry one cloud (b = 1) whose every neighbour IS its anchor: d == 0, the variance clamps to 0
    and its normalised columns are bf16(beta) while the others are ordinary.  ('center' has no such cloud: around the group MEAN it leaves the
    mean's own fp32 rounding times 1 / 1e-5, which nothing can pin.)"""
    c = dev(kc.grouper_case(B, n, S, k, 10 * D + k + S, D=D, degenerate=1 if mode == "anchor" else None))
    ref = kc.group_reference(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"], mode)
    U, st = rows_of(c, mode)
    assert U.shape == (B * S * k, ops.pad64(2 * D + 3)) and U.dtype == torch.bfloat16
    what = "%s D %d B %d n %d S %d k %d" % (mode, D, B, n, S, k)
    res = kc.check_group_rows(U, st, ref, D, what)
    ROWS_SEEN[what] = (res["pinned"], res["stat"])
    bb = c["beta"].bfloat16()
    if mode == "anchor":
        assert torch.equal(st.reshape(B, 2)[1], torch.zeros(2, dtype=torch.float64, device="cuda")), what + ": sums of the cloud without spread"
        assert torch.equal(U.view(B, S * k, -1)[1, :, :D + 3], bb.expand(S * k, -1)), what + ": cloud without spread != bf16(beta)"
    U0 = rows_of(c, mode, alpha=torch.zeros_like(c["alpha"]), stats=False)
    assert torch.equal(U0[:, :D + 3], bb.expand(B * S * k, -1)), what + ": alpha = 0 must leave bf16(beta)"
    assert torch.equal(U0[:, D + 3:], U[:, D + 3:])
    U2, st2 = rows_of(c, mode)
    assert torch.equal(U2, U) and torch.equal(st2, st), what + ": two launches differ"


# ------------------------------------------------------------------------------------------------------------- (2) the fused grouper alone
Route = collections.namedtuple("Route", "B n S k note")
ROUTES = [
    # k = 8: template <4>, four groups per 32-row tile; S ragged against it (the last tile repeats group S - 1 and must not store it)
    Route(2, 300, 1, 8, "<4> flat, 1 tile / cloud, 3 of its 4 groups repeats; grid capped at 1 workgroup"),
    Route(2, 300, 3, 8, "<4> flat, ragged"),
    Route(3, 300, 5, 8, "<4> flat, 2 tiles / cloud, ragged"),
    Route(16, 300, 7, 8, "<4> XCD-mapped, 2 clouds per XCD, ragged"),
    # k = 16: template <2>
    Route(15, 256, 7, 16, "<2> flat (the largest flat batch), odd S"),
    Route(17, 256, 9, 16, "<2> XCD-mapped, uneven lists (XCD 0 has 3 clouds, the others 2), odd S"),
    Route(2, 2048, 256, 16, "<2> flat: the shipped 256-token main group"),
    # k = 32: template <1>, one tile per group, plain store
    Route(16, 256, 3, 32, "<1> XCD-mapped, plain store"),
    Route(1, 128, 2, 32, "<1> flat, 2 tiles: the grid cap leaves ONE workgroup (< 8)"),
    Route(2, 2048, 256, 32, "<1> flat: the shipped pre_group shape"),
    # k > 32: tiles of a group meet in memory (atomicMax on a zeroed out)
    Route(2, 640, 9, 64, "<1> flat, 2 tiles per group, atomicMax"),
    Route(3, 704, 5, 128, "<1> flat, 4 tiles per group, atomicMax"),
    Route(2, 2048, 32, 128, "<1> flat: the shipped 32-token main group"),
    # 8 clouds per XCD x 40 tiles = 320 > the 256 waves of an XCD's work list: a wave goes on from cloud cl to cloud cl + 6 or cl + 7 of its list
    Route(64, 1408, 40, 32, "<1> XCD-mapped, a wave's work list crosses clouds (b_prev / inv reload)"),
]
_id = lambda r: "B%d-n%d-S%d-k%d" % r[:4]


def scales_of(r):
    """Feature scale per cloud.  Ordinary routes: 1 + b / 2.  The crossing route: 2.2^(position in the XCD's list mod 4): the clouds a wave visits
    one after the other (6 or 7 list positions apart) differ by 2.2x at least, so a stale `inv` is wrong by that factor."""
    b = torch.arange(r.B).float()
    return 2.2 ** ((b // 8) % 4) * (1 + (b % 8) / 16) if r.B == 64 else 1 + b / 2


def case_of(r, seed=1):
    c = kc.grouper_case(r.B, r.n, r.S, r.k, seed + r.S * r.k + r.B)
    c["feat"] = c["feat"] / (1 + torch.arange(r.B).float()[:, None, None] * 0.5) * scales_of(r)[:, None, None]
    return c


def fused(c, W, wimg=None, out=None):
    w1, b1, w2, b2, w3, b3 = W
    wimg = Cm._grouper_fragment_image(w1.cuda(), w2.cuda(), w3.cuda()) if wimg is None else wimg
    return ops.grouper_mlp(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"], wimg, b1.cuda(), b2.cuda(), b3.cuda(), out=out)


def chain(c, W):
    """The five kernels the fused one replaces (compressor.run_grouper's other branch) on the same crafted indices."""
    w1, b1, w2, b2, w3, b3 = [t.cuda() for t in W]
    U = ops.group_normalize(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"])
    h1 = ops.gemm_bf16(U, Cm._bf16_panel(w1), b1, EPI_RELU_BF16)
    r = ops.gemm_bf16(h1, Cm._bf16_panel(w2), b2, EPI_RELU_BF16)
    h2 = ops.gemm_bf16(r, Cm._bf16_panel(w3), b3, EPI_RELU_BF16, skip=h1)
    return ops.maxpool(h2, c["B"] * c["S"], c["k"])


@pytest.mark.parametrize("r", ROUTES, ids=_id)
def test_neighbour_probe_exact(r):
    """(a) alpha = +-2^p, beta = 0, biases 0, W2 = W3 = 0, W1 row c = +-1 at column sel(c) (three variants walk all 259 inputs): out[g][c] =
    max_j relu(+-U[j][sel(c)]) — exactly, with U from ops.group_normalize on the same inputs (a power-of-two alpha and beta = 0 make the bits
    independent of FMA contraction).  Where the cloud has room (S (k + 1) <= n) the indices are all distinct and slot (c + s) mod k is planted
    as the winner of channel c in group s: the reference's arg-max must cover every slot 0..k-1 — the 15 in-lane maxes, the cross-half exchange
    and each of the k / 32 tiles decide some output."""
    base = case_of(r)
    z, zz = torch.zeros(128), torch.zeros(128, 128)
    slots = set()
    planted = r.S * (r.k + 1) <= r.n
    for v in range(3):
        w1, sel, sgn, alpha = kc.grouper_selection_probe(v)
        c = dict(base, alpha=alpha, beta=torch.zeros(131))
        c = dev(kc.plant_winners(c, sel, sgn, alpha) if planted else c)
        U = rows_of(c, stats=False)
        want, slot = kc.grouper_selection_expected(U, r.B, r.S, r.k, sel, sgn)
        got = fused(c, (w1, z, zz, z, zz, z))
        kc.assert_interval(got, want, want, "neighbour probe %s variant %d (%s)" % (_id(r), v, r.note), k=r.k, S=r.S, slot=slot)
        assert torch.equal(got.double(), want)
        slots |= set(slot[:, (sel < 131).cuda()].flatten().tolist())
        assert float((want > 0).double().mean()) > 0.3
    if planted:
        assert slots == set(range(r.k)), "arg-max slots %s do not cover 0..%d" % (sorted(slots), r.k - 1)


@pytest.mark.parametrize("r", ROUTES, ids=_id)
def test_layer_probe_exact(r):
    """(b) alpha = 0 and integers everywhere (kernel_checks.grouper_integer_probe: every h1, r, out an integer <= 256, checked on the float64
    result): the output of a group is a function of its anchor alone and exact through three layers, the residual MFMA and three bf16 roundings.
    Pins the k permutation of the layer-2 / layer-3 fragment image, the bias layout per block and half, and the identity residual."""
    base = case_of(r)
    feat, beta, W, o = kc.grouper_integer_probe(r.B, r.n, 5 + r.k, device="cuda")
    c = dev(dict(base, feat=feat, alpha=torch.zeros(131), beta=beta))
    want = kc._take(o, c["fi"].long()).reshape(-1, 128)
    got = fused(c, W)
    kc.assert_interval(got, want, want, "layer probe %s (%s)" % (_id(r), r.note), k=r.k, S=r.S, slot=torch.zeros_like(want, dtype=torch.long))
    assert torch.equal(got.double(), want)
    assert torch.equal(chain(c, W).double(), want)                   # the chain is exact on the same integers too


@pytest.mark.parametrize("r", ROUTES, ids=_id)
def test_randn_interval_and_housekeeping(r):
    """(c) + (d).  The staged reference takes `inv` from float64 sums; that the kernels' sums of this very case lie within 2^-24 of them (half a
    rounding of `inv`) is asserted first, on the sums ops.group_normalize returns (the same statistics launch the fused kernel makes)."""
    c = dev(case_of(r))
    W = kc.grouper_weights(2)
    what = "%s (%s)" % (_id(r), r.note)
    g = kc.group_reference(c["feat"], c["xyz"], c["fi"], c["ki"], c["alpha"], c["beta"], stats_rel=kc.U24)
    U, st = rows_of(c)
    st = st.reshape(r.B, 2)
    e1, e2 = (st[:, 0] - g["s1"]).abs() / g["tol1"], (st[:, 1] - g["s2"]).abs() / g["tol2"]
    assert float(e1.max()) <= 1 and float(e2.max()) <= 1, "%s: sums off by %.2f / %.2f x 2^-24 (sum |d|, sum d^2)" % (what, float(e1.max()), float(e2.max()))
    del U
    sr = kc.grouper_staged_reference(g, *W)
    del g
    wimg = Cm._grouper_fragment_image(W[0].cuda(), W[2].cuda(), W[4].cuda())
    rows = r.B * r.S
    fill = float("nan") if r.k <= 32 else 3.0e38                     # k > 32: the launcher's zeroing is what atomicMax relies on
    outs = []
    for _ in range(3):
        big, out = kc.guarded(rows, 128, fill, "cuda")
        assert fused(c, W, wimg, out=out) is out
        kc.assert_guard_intact(big, rows * 128, what)                # the ragged tile's repeated group was not stored anywhere
        outs.append(out)
    mism = kc.check_grouper(outs[0], sr, "fused " + what)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), what + ": launches differ"
    assert torch.equal(fused(c, W, wimg), outs[0])
    ch = chain(c, W)
    mism_chain = kc.check_grouper(ch, sr, "chain " + what)
    GROUPER_SEEN[_id(r)] = (sr["pinned"], sr["wide"], mism, mism_chain, float((ch != outs[0]).double().mean()), float(torch.maximum(e1, e2).max()))


def test_device_float64_reference_matches_cpu():
    """The references above are taken on the device (float64 there is a plain matmul, the CPU needs seconds per case): the same helpers on the CPU
    give the same intervals."""
    c = kc.grouper_case(3, 300, 7, 16, 4, degenerate=1)
    W = kc.grouper_weights(2)
    res, pres = [], []
    for cc in (c, dev(c)):
        g = kc.group_reference(cc["feat"], cc["xyz"], cc["fi"], cc["ki"], cc["alpha"], cc["beta"], stats_rel=kc.U24)
        sr = kc.grouper_staged_reference(g, *W)
        res.append([t.cpu() for t in (kc.bf16_round(g["pre"] - g["a"]), kc.bf16_round(g["pre"] + g["a"]), sr["lo"], sr["hi"], sr["ref"], sr["slot"])])
        pres.append(g["pre"].cpu())
    assert torch.allclose(pres[0], pres[1], rtol=1e-12, atol=1e-14)
    for a, b in zip(*res):
        assert float((a != b).double().mean()) <= 1e-4               # (a float64 sum order can move an end that sits on a rounding boundary)
    o = kc.grouper_integer_probe(2, 200, 9)[3]
    assert torch.equal(kc.grouper_integer_probe(2, 200, 9, device="cuda")[3].cpu(), o)


def test_zz_margins():
    """Printed last (DESIGN.md section 3 quotes them): per case the share of elements the reference pins, the share with an interval wider than
    2 ulps, the share of fused / chain outputs that differ from the point reference at all, fused != chain, and the statistics' err / tol."""
    for what, (pinned, stat) in ROWS_SEEN.items():
        print("rows     %-40s pinned %.4f  sums err / tol %.3f" % (what, pinned, stat))
    for what, v in GROUPER_SEEN.items():
        print("grouper  %-20s pinned %.3f  wide %.3f  fused != ref %.5f  chain != ref %.5f  fused != chain %.5f  sums err / 2^-24 %.3f" % ((what,) + v))
    if T0[0] is not None:
        print("module run time %.1f s" % (time.time() - T0[0]))
    assert all(v[0] >= kc.PINNED_MIN and v[1] <= kc.WIDE_MAX for v in GROUPER_SEEN.values())
