"""GPU (-m gpu): the two narrow-block kernels of csrc/fused_mlp.hip — ln_mlp_resid_kernel (LayerNorm, MLP-up, GELU, MLP-down, gated residual,
optionally the next block's LayerNorm + first projection) and ln_linear_kernel — driven alone and judged per element.

  (1) randn data: ln_mlp_resid_'s x against a float64 reference that rounds where the kernel rounds (h, u) and allows, per element, only what fp32
      arithmetic can do to those roundings (kernel_checks.fused_mlp_reference; the condition median(tol) <= 0.02 median(|update|) is asserted on
      the reference first); ln_linear and the chained projection inside [bf16(pre - a), bf16(pre + a)] (ln_linear_reference; at least 80 % of the
      elements pinned to the bit, at most 5 % with an interval beyond 2 ulps).  The bf16 mirror == a cast of x; the chained projection == ops.ln_linear
      on the updated x, bit for bit; three launches into fresh buffers agree to the bit; x in place inside a NaN surround (ldx > C), the mirror
      (ldxb > C) and both bf16 outputs (ldo > N) inside sentinel surrounds that stay intact, equal to the dense calls.
  (2) exact probes, torch.equal: the LayerNorm switched off from outside (scale = -1: h == the shift rows; ln_w = 0: h == ln_b) and values where the
      kernel's GELU is exactly relu — integers through the whole MLP, a signed gather through W_up with a W_dn whose columns are all different,
      gated and ungated, and the GEMM probes through ln_linear and through the chained projection.
  (3) repeated launches with mirror and chained projection: the digests of x, mirror and projection are the same every time (launch_digests).

What no kernel-level test reached before, and the case that reaches it (CASES below, ids C-form-rps-M):
  rows_per_sample = 1 (per_token: every lane its own modulation row)     128-modgate-1-333, 128-modgate-1-4096, 128-mod-1-129, 64-modgate-1-127, 64-affmod-1-16
  a sample boundary inside a 16-row tile / between a wave's two tiles    rps 7, 16, 33: 128-modgate-7-333, 128-modgate-16-127, 128-modgate-33-333, 64-mod-16-333 ...
  M < 16 and M = 1                                                       128-modgate-7-5, 128-modgate-1-1, 128-plain-0-1, 128-affine-0-5, 64-plain-0-5, 64-modgate-1-1
  more workgroups than fit on the chip at once (> 512)                   128-modgate-100-66085 (517 workgroups, the last one 37 rows)
  an output with ldo > N, ln_linear and the chained projection           every case (test_randn_staged_and_housekeeping, the guarded launches)
  an affine LayerNorm together with a modulation                         128-affmod-7-127, 128-affmod-32-333, 64-affmod-1-16
  an affine LayerNorm with a gate only                                   128-affgate-16-128, 128-affgate-33-333, 64-affgate-100-333
  the same digests launch after launch, mirror and chained projection   test_repeated_launches_same_digests
  the shipped pairs: C = 128 with rows_per_sample = 32 / 256 / 2048      128-modgate-32-4096, 128-modgate-256-4096, 128-modgate-2048-4096 (and rows_per_sample = 1)
The helpers, an emulation that passes them and the planted faults that fail them are tested without a GPU in test_kernel_checks_host.py."""
import collections
import hashlib
import time

import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

ops = None
RATIOS = collections.defaultdict(float)          # worst err / tol per class (test_zz_margins)
SEEN, T0 = {}, [None]


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops
    assert torch.cuda.is_available()
    from ldt_amd import ops as _ops
    ops = _ops
    torch.backends.cuda.matmul.allow_tf32 = False
    T0[0] = time.time()
    yield
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS[kind], ratio)
    return ratio


# form: which of (affine LayerNorm, modulation, gate) the launch carries
FORMS = {"plain": (), "affine": ("ln",), "modgate": ("mod", "gate"), "mod": ("mod",), "affmod": ("ln", "mod", "gate"), "affgate": ("ln", "gate")}
Case = collections.namedtuple("Case", "C form rps M N salt", defaults=(0,))
CASES = [
    # the shipped pairs: the Compressor's d = 128 blocks at 32 / 256 / 2048 tokens per sample, and its per-token form
    Case(128, "modgate", 32, 4096, 384), Case(128, "modgate", 256, 4096, 128), Case(128, "modgate", 2048, 4096, 128),
    Case(128, "modgate", 1, 333, 128), Case(128, "modgate", 1, 4096, 64), Case(128, "mod", 1, 129, 384),
    # sample boundaries inside a tile (7), at every tile (16), between a wave's tiles and inside (33), inside a workgroup (100), none (M)
    Case(128, "modgate", 7, 333, 64), Case(128, "modgate", 16, 127, 128), Case(128, "modgate", 33, 333, 384), Case(128, "mod", 33, 128, 64),
    Case(128, "modgate", 100, 333, 128), Case(128, "modgate", 129, 129, 128),
    # fewer rows than a tile
    Case(128, "modgate", 7, 5, 384), Case(128, "modgate", 1, 1, 384, 1), Case(128, "plain", 0, 1, 384), Case(128, "plain", 0, 16, 128), Case(128, "affine", 0, 5, 384),
    Case(128, "affine", 0, 4096, 128), Case(128, "plain", 0, 129, 64),
    # combinations the launcher accepts and no shipped block uses
    Case(128, "affmod", 7, 127, 128), Case(128, "affmod", 32, 333, 64), Case(128, "affgate", 16, 128, 384), Case(128, "affgate", 33, 333, 128),
    # 517 workgroups (two share a CU: more than 512 do not fit at once); the last one has 37 rows
    Case(128, "modgate", 100, 66085, 64),
    Case(64, "modgate", 32, 4096, 128), Case(64, "modgate", 1, 127, 384), Case(64, "modgate", 7, 129, 64), Case(64, "mod", 16, 333, 128),
    Case(64, "modgate", 33, 128, 384), Case(64, "plain", 0, 5, 384), Case(64, "affine", 0, 333, 64), Case(64, "affmod", 1, 16, 384),
    Case(64, "affgate", 100, 333, 128), Case(64, "modgate", 1, 1, 384, 1), Case(64, "plain", 0, 4096, 64), Case(64, "modgate", 333, 333, 128),
]
# salt: with a single row one ambiguous element of h unpins every output it feeds, and whether the conditions on the references hold is a lottery
# (0.50 .. 1.00 pinned over six draws); the salt picks a draw that meets them — a choice of input, made and asserted before any launch
_id = lambda c: "%d-%s-%d-%d" % c[:4]


def case_data(c):
    """-> CPU tensors of kc.mlp_randn_case for the case (one modulation row per sample)."""
    rps = c.rps or c.M
    return kc.mlp_randn_case(c.M, c.C, 1000 * c.C + 7 * c.M + rps + len(c.form) + 100000 * c.salt, n_samples=(c.M + rps - 1) // rps, N=c.N, tame=c.form == "affmod" or c.M < 16)


def ref_kw(d, form, rps, gate=True):
    """The LayerNorm / gate arguments of the float64 references: views of d's tensors (on whatever device they live)."""
    C = d["x"].shape[1]
    kw = {}
    if "ln" in FORMS[form]:
        kw.update(ln_w=d["ln_w"], ln_b=d["ln_b"])
    if "mod" in FORMS[form]:
        kw.update(shift=d["mod"][:, :C], scale=d["mod"][:, C:2 * C])
    if gate and "gate" in FORMS[form]:
        kw.update(gate=d["mod"][:, 2 * C:])
    if "shift" in kw or "gate" in kw:
        kw.update(rows_per_sample=rps)
    return kw


def launch_kw(kw, stride):
    """... and of the launches: the same views plus their per-sample stride."""
    return dict(kw, mod_sample_stride=stride) if "rows_per_sample" in kw else dict(kw)


def nan_guarded(x):
    """x as the interior of a NaN-filled fp32 buffer (ldx = C + 128) -> (big, interior view)."""
    big = torch.full((x.shape[0] + 16, x.shape[1] + 128), float("nan"), dtype=torch.float32, device=x.device)
    view = big[8:8 + x.shape[0], 64:64 + x.shape[1]]
    view.copy_(x)
    return big, view


def assert_nan_surround(big, view, what):
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[8:8 + view.shape[0], 64:64 + view.shape[1]] = False
    assert bool(torch.isnan(big[mask]).all()), what + ": the surround of x was written"
    assert not bool(torch.isnan(view).any()), what + ": NaN from outside x reached the result"


SENT_BF16 = -1.7014118e38                        # a bit pattern no kernel under test produces


def sent_guarded(M, N):
    """-> (big, interior bf16 [M, N] view with row stride N + 128) filled with the sentinel."""
    big = torch.full((M + 16, N + 128), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    return big, big[8:8 + M, 64:64 + N]


def assert_sent_surround(big, view, what):
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[8:8 + view.shape[0], 64:64 + view.shape[1]] = False
    sent = torch.full((), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    bad = mask & (big != sent)
    if bool(bad.any()):
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d elements outside the output were overwritten, first at big[%d, %d] (interior starts at [8, 64], is %s)" % (
            what, int(bad.sum()), i[0], i[1], tuple(view.shape)))
    assert not bool((view == sent).any()) and not bool(torch.isnan(view.float()).any()), what + ": elements of the output were not written"


def mlp(x, d, kw, **more):
    return ops.ln_mlp_resid_(x, d["w_up_bf"], d["b_up"], d["w_dn_bf"], d["b_dn"], **kw, **more)


def to_dev(d):
    dd = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    for k in ("w_up", "w_dn", "wn"):
        if k in dd:
            dd[k + "_bf"] = dd[k].bfloat16().contiguous()
    return dd


# ------------------------------------------------------------------------------------------------------------- (1) randn data
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_randn_staged_and_housekeeping(c):
    C, M, N, rps = c.C, c.M, c.N, c.rps or c.M
    what = "%s (N %d)" % (_id(c), N)
    d = to_dev(case_data(c))
    rkw = ref_kw(d, c.form, rps)
    kw = launch_kw(rkw, 3 * C)
    lkw_ref = ref_kw(d, c.form, rps, gate=False)                     # ln_linear: the same LayerNorm, no gate
    lkw = launch_kw(lkw_ref, 3 * C)
    # conditions on the references, before any output is looked at (asserted again inside the checks)
    sr = kc.fused_mlp_reference(d["x"], d["w_up"], d["b_up"], d["w_dn"], d["b_dn"], **rkw)
    lr = kc.ln_linear_reference(d["x"], d["wn"], d["bn"], **lkw_ref)
    assert sr["ratio"] <= kc.MLP_TOL_CAP and lr["pinned"] >= kc.LNLIN_PINNED_MIN and lr["wide"] <= kc.LNLIN_WIDE_MAX, (sr["ratio"], lr["pinned"], lr["wide"])

    # ---- ln_mlp_resid_: dense with a dense mirror | in place inside a NaN surround with the mirror inside a sentinel surround | plain
    x1, mirror = d["x"].clone(), torch.empty(M, C, dtype=torch.bfloat16, device="cuda")
    assert mlp(x1, d, kw, x_bf16_out=mirror) is x1
    worst = note("ln_mlp_resid_ C %d %s" % (C, c.form), kc.check_fused_mlp(x1, sr, "ln_mlp_resid_ " + what))
    assert torch.equal(mirror, x1.bfloat16()), what + ": bf16 mirror != a cast of x"
    big, xv = nan_guarded(d["x"])
    mbig, mv = sent_guarded(M, C)
    mlp(xv, d, kw, x_bf16_out=mv)
    assert_nan_surround(big, xv, "ln_mlp_resid_ %s in place with ldx > C" % what)
    assert_sent_surround(mbig, mv, "ln_mlp_resid_ %s mirror with ldxb > C" % what)
    assert torch.equal(xv, x1) and torch.equal(mv, mirror), what + ": strided launch differs from the dense one"
    x3 = d["x"].clone()
    mlp(x3, d, kw)
    assert torch.equal(x3, x1), what + ": launches differ"

    # ---- the chained projection: affine next-LN, and modulated where the case is modulated
    nexts = [("affine", dict(ln_w=d["nln_w"], ln_b=d["nln_b"]))]
    if "mod" in FORMS[c.form]:
        nexts.append(("modulated", dict(shift=rkw["shift"], scale=rkw["scale"], rows_per_sample=rps)))
    for name, nref in nexts:
        nkw = launch_kw(nref, 3 * C)
        x2 = d["x"].clone()
        _, qn = mlp(x2, d, kw, next_linear=dict(w=d["wn_bf"], bias=d["bn"], **nkw))
        assert torch.equal(x2, x1), "%s: x of the chained launch (%s next-LN) differs" % (what, name)
        alone = ops.ln_linear(x1, d["wn_bf"], d["bn"], **nkw)
        assert torch.equal(qn, alone), "%s: chained projection (%s next-LN) != ops.ln_linear on the updated x" % (what, name)
        nr = kc.ln_linear_reference(x1, d["wn"], d["bn"], **nref)
        kc.check_ln_linear(alone, nr, "ops.ln_linear on the updated x, %s next-LN, %s" % (name, what))
        obig, ov = sent_guarded(M, N)
        big, xv = nan_guarded(d["x"])
        _, q2 = mlp(xv, d, kw, next_linear=dict(w=d["wn_bf"], bias=d["bn"], out=ov, **nkw))
        assert q2 is ov
        assert_sent_surround(obig, ov, "chained projection %s with ldo > N" % what)
        assert_nan_surround(big, xv, "chained launch %s in place with ldx > C" % what)
        assert torch.equal(ov, qn) and torch.equal(xv, x1), what + ": strided chained launch differs from the dense one"

    # ---- ln_linear on x itself
    outs = [ops.ln_linear(d["x"], d["wn_bf"], d["bn"], **lkw) for _ in range(3)]
    assert outs[0].shape == (M, N) and outs[0].dtype == torch.bfloat16
    mism = kc.check_ln_linear(outs[0], lr, "ln_linear " + what)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), what + ": ln_linear launches differ"
    obig, ov = sent_guarded(M, N)
    big, xv = nan_guarded(d["x"])
    assert ops.ln_linear(xv, d["wn_bf"], d["bn"], out=ov, **lkw) is ov
    assert_sent_surround(obig, ov, "ln_linear %s with ldo > N" % what)
    assert_nan_surround(big, xv, "ln_linear %s with ldx > C" % what)
    assert torch.equal(ov, outs[0]), what + ": strided ln_linear differs from the dense one"
    assert torch.equal(ops.ln_linear(d["x"], d["wn_bf"], None, **lkw), ops.ln_linear(d["x"], d["wn_bf"], torch.zeros_like(d["bn"]), **lkw))
    SEEN[_id(c)] = (sr["ratio"], sr["amb_h"], sr["amb_u"], worst, lr["pinned"], lr["wide"], mism)


# ------------------------------------------------------------------------------------------------------------- (2) exact probes
def probe_dev(p):
    dd = to_dev(p)
    return dd, dict(shift=dd["shift"], scale=dd["scale"], mod_sample_stride=p["shift"].shape[1], **({"gate": dd["gate"]} if p["gate"] is not None else {}))


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_probes_exact(c):
    """The MLP probes with the case's M and rows_per_sample (gated and ungated whatever the case's form: the probes bring their own modulation), x in
    place inside a NaN surround; each launch also chains a GEMM probe through the next block's projection, whose LayerNorm is switched off the same
    way (per-row shift rows with scale = -1, or ln_w = 0 and ln_b = one probe row).  Then the GEMM probes through ops.ln_linear."""
    C, M, N, rps = c.C, c.M, c.N, c.rps or c.M
    xs, ws, rs = kc.selection_probe(M, N, C)
    xi, wi, bi, ri = kc.integer_probe(M, N, C, 3 + M, device="cuda")
    gemm = [("selection", xs.cuda(), ws.cuda().bfloat16(), None, rs.cuda().double()), ("integer", xi.cuda(), wi.cuda().bfloat16(), bi.cuda(), ri)]
    minus = torch.full((M, C), -1.0, device="cuda")
    for gated in (False, True):
        for pi, probe in enumerate((kc.mlp_integer_probe, kc.mlp_selection_probe)):
            p = probe(M, C, rps, 11 + M + rps, gated, device="cuda")
            d, kw = probe_dev(p)
            kw["rows_per_sample"] = rps
            what = "%s probe %s %s" % (probe.__name__, _id(c), "gated" if gated else "ungated")
            name, xp, wp, bp, rp = gemm[pi]
            big, xv = nan_guarded(d["x"])
            mirror = torch.empty(M, C, dtype=torch.bfloat16, device="cuda")
            _, q = mlp(xv, d, kw, x_bf16_out=mirror, next_linear=dict(w=wp, bias=bp, shift=xp, scale=minus, mod_sample_stride=C, rows_per_sample=1))
            assert_nan_surround(big, xv, what)
            kc.assert_elementwise(xv, p["ref"], 0.0, what)
            assert torch.equal(xv.double(), p["ref"]) and torch.equal(mirror, xv.bfloat16())
            kc.assert_elementwise(q, rp, 0.0, "%s: chained %s probe" % (what, name))
            assert torch.equal(q.double(), rp)
            x2 = d["x"].clone()                                      # the other switch: ln_w = 0, every row of the next h is ln_b = probe row M // 2
            _, q = mlp(x2, d, kw, next_linear=dict(w=wp, bias=bp, ln_w=torch.zeros(C, device="cuda"), ln_b=xp[M // 2].contiguous()))
            assert torch.equal(x2, xv) and torch.equal(q.double(), rp[M // 2].expand(M, -1)), what + ": chained projection with ln_w = 0"
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(M)).cuda() * 40 + 3          # any finite x
    for name, xp, wp, bp, rp in gemm:
        q = ops.ln_linear(x, wp, bp, shift=xp, scale=minus, mod_sample_stride=C, rows_per_sample=1)
        kc.assert_elementwise(q, rp, 0.0, "ln_linear %s probe %s" % (name, _id(c)))
        assert torch.equal(q.double(), rp)
        q = ops.ln_linear(x, wp, bp, ln_w=torch.zeros(C, device="cuda"), ln_b=xp[M // 2].contiguous())
        assert torch.equal(q.double(), rp[M // 2].expand(M, -1)), "ln_linear %s probe %s with ln_w = 0" % (name, _id(c))


# ------------------------------------------------------------------------------------------------------------- (3) launch digests
def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def launch_digests():
    """One gated and one ungated randn case (with mirror and chained projection) and the gated integer probe -> {name: sha256}."""
    out = {}
    for c in (Case(128, "modgate", 33, 333, 128), Case(64, "affine", 0, 1000, 64)):
        d = to_dev(case_data(c))
        rps = c.rps or c.M
        kw = launch_kw(ref_kw(d, c.form, rps), 3 * c.C)
        for rep in range(3):
            x, mirror = d["x"].clone(), torch.empty(c.M, c.C, dtype=torch.bfloat16, device="cuda")
            _, q = mlp(x, d, kw, x_bf16_out=mirror, next_linear=dict(w=d["wn_bf"], bias=d["bn"], ln_w=d["nln_w"], ln_b=d["nln_b"]))
            cur = {"%s x" % _id(c): _digest(x), "%s mirror" % _id(c): _digest(mirror), "%s next" % _id(c): _digest(q)}
            assert rep == 0 or all(out[k] == v for k, v in cur.items()), "run-to-run difference"
            out.update(cur)
    p = kc.mlp_integer_probe(333, 128, 33, 5, True, device="cuda")
    d, kw = probe_dev(p)
    x = d["x"].clone()
    mlp(x, d, dict(kw, rows_per_sample=33))
    assert torch.equal(x.double(), p["ref"])
    out["integer probe"] = _digest(x)
    return out


def test_repeated_launches_same_digests():
    """launch_digests() asserts inside: three launches with mirror and chained projection give identical digests, and the gated integer probe is
    exact.  The digests themselves are what two builds of the library are compared by (a kernel refactor must reproduce every one)."""
    d = launch_digests()
    assert len(d) == 7 and all(len(v) == 64 for v in d.values())


def test_zz_margins():
    """Printed last (DESIGN.md section 3 quotes them): per case the conditions on the references and the worst err / tol; per class the worst err / tol."""
    for what, v in SEEN.items():
        print("case %-24s tol / update %.4f  ambiguous h %.3f u %.3f  worst err / tol %.3f | ln_linear pinned %.3f  wide %.3f  != point reference %.5f" % ((what,) + v))
    for k in sorted(RATIOS):
        print("worst err / tol, %-32s %.3f" % (k + ":", RATIOS[k]))
    if SEEN:
        col = lambda i: [v[i] for v in SEEN.values()]
        print("ranges: tol / update %.4f .. %.4f, pinned %.3f .. %.3f, wide %.3f .. %.3f, ln_linear != point reference %.5f .. %.5f" % (
            min(col(0)), max(col(0)), min(col(4)), max(col(4)), min(col(5)), max(col(5)), min(col(6)), max(col(6))))
    if T0[0] is not None:
        print("module run time %.1f s" % (time.time() - T0[0]))
    assert all(v <= 1.0 for v in RATIOS.values())
