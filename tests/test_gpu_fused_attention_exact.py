"""GPU (-m gpu): the three kernels that project q | k | v and attend in one launch, driven alone and judged per element.

They run only inside the Score forward, where tests/test_gpu_fullsize.py compares the whole model's output after four blocks (rel-MSE
1e-6, fused against unfused, both our own kernels).  ops.qkv_attention launches exactly what the forward launches (the forward calls the
same function), so here every form (ROWS: pinned to what ops.qkv_attention_route reports, asserted before every launch, with the
neighbours of each shape rule that must NOT take a fused form) is held to
  (1) torch.equal on a softmax that gathers one key, fed through an identity projection (plain forms, no bias / all-zero bias);
  (2) the plain attention bound 2^-8 |ref| + 2^-8 max_j |v_j| on operands whose projection is exact in fp32 and bf16, plus bit-equality of
      the 256-token form with GEMM + attention kernel on the same operands;
  (3) a two-stage float64 reference on randn data with a derived allowance for bf16 rounding flips of q | k | v (kernel_checks.
      fused_attention_tol; the only possible check of the LN-folded forms), the step-indexed S | C fetch included;
  (4) bit-equality of three launches into fresh buffers, and of operands / outputs embedded in NaN / sentinel surrounds with the dense call,
      the q | k | v workspace untouched.
The helpers, and that they fail a planted dropped key, swapped heads and a shifted S | C segment, are tested without a GPU in
test_kernel_checks_host.py."""
import collections
import time

import pytest
import torch

import kernel_checks as kc

pytestmark = pytest.mark.gpu

ops = None
EPI_BF16 = None
DH = 64
RATIOS = collections.defaultdict(float)          # worst err / tol per class of check
WIDEN = {}                                       # case -> (ambiguous fraction, median, max of tol / base)
SENT_BF16 = -1.7014118e38                        # a bit pattern no kernel under test produces


@pytest.fixture(scope="module", autouse=True)
def _mods():
    global ops, EPI_BF16
    assert torch.cuda.is_available()
    from ldt_amd import _lib, ops as _ops
    ops, EPI_BF16 = _ops, _lib.EPI_BF16
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()                     # the float64 references of the B = 64, T = 256 rows are GBs: freed between rows


def dev(x, dt=None):
    return x.to("cuda", dt) if dt else x.to("cuda")


def note(kind, ratio):
    RATIOS[kind] = max(RATIOS[kind], ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------- route table
SELF32, SELF256, CROSS = 1, 2, 3
FORM = {0: "two kernels", SELF32: "32-token self", SELF256: "256-token self", CROSS: "32 x 32 cross"}
Row = collections.namedtuple("Row", "B T S hidden heads K fold wgs route kvpad")


def _row(tag, B, T, hidden, heads, K, route, S=0, fold=0, wgs=0, kvpad=False):
    return pytest.param(Row(B, T, S, hidden, heads, K, fold, wgs, route, kvpad), id="%s-B%d-T%d-D%d-K%d%s%s%s" % (
        tag, B, T, hidden, K, "-fold%d" % fold if fold else "", "-wgs%d" % wgs if wgs else "", "-kvpad" if kvpad else ""))


ROWS = [
    # 256-token form: (sample, head) tiles of 256 x 192 on the persistent kernel, taken from 5/8 of the workgroups up
    _row("s256", 64, 256, 1024, 16, 1024, SELF256),                       # the bench shape: 1024 tiles, four per workgroup
    _row("s256", 16, 256, 1024, 16, 1024, SELF256),                       # 256 tiles: one each
    _row("s256", 17, 256, 1024, 16, 128, SELF256),                        # 272: sixteen workgroups take a second tile; K = 128: the plain minimum
    _row("s256", 10, 256, 1024, 16, 256, SELF256),                        # 160 tiles = exactly 5/8: taken, grid < CUs
    _row("s256", 9, 256, 1024, 16, 1024, 0),
    _row("s256", 8, 256, 1024, 16, 1024, SELF256, wgs=128),               # taken under a sub-batch stream's cap
    _row("s256", 8, 256, 1024, 16, 1024, 0),                              # ... and not without it
    _row("s256", 40, 256, 256, 4, 256, SELF256),                          # tn = 4 < 8: group_m = 1 order; 160 tiles
    _row("s256", 64, 256, 256, 4, 1024, SELF256),
    _row("s256", 64, 255, 1024, 16, 1024, 0),
    _row("s256", 64, 256, 1024, 32, 1024, 0),                             # head dim 32
    _row("s256", 64, 256, 1024, 16, 64, 0),                               # K below the plain minimum
    _row("s256", 64, 256, 1024, 16, 1024, SELF256, fold=256),             # four statistics parts
    _row("s256", 17, 256, 1024, 16, 512, SELF256, fold=256),
    _row("s256", 40, 256, 256, 4, 256, SELF256, fold=256),                # the folded minimum: one part
    _row("s256", 8, 256, 1024, 16, 768, SELF256, fold=256, wgs=128),
    _row("s256", 9, 256, 1024, 16, 1024, 0, fold=256),
    _row("s256", 64, 256, 1024, 16, 1280, 0, fold=256),                   # more than four parts
    # 32-token self form: 128 x 192 tiles (four samples x one head) of the mid-size tile kernel, at most two rounds of workgroups
    _row("s32", 4, 32, 1024, 16, 1024, SELF32),                           # one row tile
    _row("s32", 64, 32, 1024, 16, 1024, SELF32),                          # the shipped batch
    _row("s32", 128, 32, 1024, 16, 320, SELF32),                          # 512 workgroups: the two-round limit; K = NS + 2 tiles: the minimum
    _row("s32", 132, 32, 1024, 16, 1024, 0),
    _row("s32", 6, 32, 1024, 16, 1024, 0),                                # M % 128
    _row("s32", 64, 32, 256, 4, 320, SELF32),
    _row("s32", 64, 32, 256, 4, 256, 0),                                  # K below NS + 2 tiles
    _row("s32", 64, 32, 1024, 16, 1024, SELF32, fold=32),
    _row("s32", 64, 32, 256, 4, 512, SELF32, fold=32),
    _row("s32", 4, 32, 1024, 16, 512, SELF32, fold=32),
    _row("s32", 132, 32, 1024, 16, 1024, 0, fold=32),
    _row("s32", 64, 32, 1024, 16, 1024, 0, fold=256),                     # statistics per 256 columns are not this kernel's
    # cross form: 64 x 64 tiles (two samples x one head), 48 .. 2 x CUs workgroups
    _row("x32", 6, 32, 1024, 16, 1024, CROSS, S=32),                      # 48 workgroups: the minimum
    _row("x32", 4, 32, 1024, 16, 1024, 0, S=32),
    _row("x32", 8, 32, 1024, 16, 128, CROSS, S=32),
    _row("x32", 32, 32, 1024, 16, 1024, CROSS, S=32, kvpad=True),         # K | V in padded rows with a padded batch stride
    _row("x32", 64, 32, 1024, 16, 1024, CROSS, S=32),                     # 512: the maximum
    _row("x32", 66, 32, 1024, 16, 1024, 0, S=32),
    _row("x32", 64, 32, 1024, 16, 1024, 0, S=64),
]
TAKEN = [p for p in ROWS if p.values[0].route]
PLAIN = [p for p in TAKEN if not p.values[0].fold]


def check_route(r):
    got = ops.qkv_attention_route(r.B, r.T, r.hidden, r.heads, r.K, cond_tokens=r.S, fold=r.fold, max_wgs=r.wgs)
    assert got == r.route, "%s runs '%s', the table says '%s': this shape no longer tests the kernel it was chosen for" % (r, FORM[got], FORM[r.route])


@pytest.mark.parametrize("r", ROWS)
def test_route_table(r):
    check_route(r)


def test_route_table_reaches_every_form_and_every_neighbour():
    rows = [p.values[0] for p in ROWS]
    assert {(r.route, bool(r.fold)) for r in rows if r.route} == {(SELF32, False), (SELF32, True), (SELF256, False), (SELF256, True), (CROSS, False)}
    off = {(r.B, r.T, r.S, r.hidden, r.heads, r.K, r.fold, r.wgs) for r in rows if not r.route}
    for want in [(9, 256, 0, 1024, 16, 1024, 0, 0), (64, 255, 0, 1024, 16, 1024, 0, 0), (64, 256, 0, 1024, 32, 1024, 0, 0),     # 5/8 rule, tokens, head dim
                 (132, 32, 0, 1024, 16, 1024, 0, 0), (6, 32, 0, 1024, 16, 1024, 0, 0), (64, 32, 0, 256, 4, 256, 0, 0),          # two rounds, M % 128, K tiles
                 (4, 32, 32, 1024, 16, 1024, 0, 0), (66, 32, 32, 1024, 16, 1024, 0, 0)]:                                         # 48 .. 512 workgroups
        assert want in off, want
    edges = {(r.route, r.B, r.K, r.fold) for r in rows}
    for want in [(SELF256, 10, 256, 0), (SELF256, 17, 128, 0), (SELF256, 40, 256, 256), (SELF256, 64, 1024, 256), (SELF32, 128, 320, 0), (SELF32, 4, 1024, 0),
                 (SELF32, 64, 512, 32), (SELF32, 64, 1024, 32), (CROSS, 6, 1024, 0), (CROSS, 64, 1024, 0), (CROSS, 8, 128, 0)]:
        assert want in edges, want


# ------------------------------------------------------------------------------------------------------------- launching
def kv_operand(r, kv):
    """The condition's K | V rows [B S, 2 hidden] bf16 as the product passes them (ld = 2 hidden) or, kvpad, inside NaN-padded rows with a
    NaN tail per sample (row stride 2 hidden + 128, S + 3 rows per sample).  -> keyword arguments of ops.qkv_attention."""
    if kv is None:
        return {}
    kv = dev(kv, torch.bfloat16)
    if not r.kvpad:
        return dict(kv_cond=kv)
    big = torch.full((r.B, r.S + 3, 2 * r.hidden + 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    big[:, :r.S, 64:64 + 2 * r.hidden] = kv.view(r.B, r.S, 2 * r.hidden)
    return dict(kv_cond=big.view(r.B * (r.S + 3), -1)[:, 64:64 + 2 * r.hidden], kv_batch_stride=big.stride(0))


def launch3(r, x, w, bias=None, kv=None, **fold):
    """Three launches into fresh buffers (the mid kernel's epilogue hazard once showed as run-to-run differences): all equal, the q | k | v
    workspace untouched.  -> O [B, H, T, DH]."""
    check_route(r)
    kw = dict(fold, **kv_operand(r, kv))
    outs = []
    for i in range(3):
        qkv = torch.full((r.B * r.T, 3 * r.hidden), SENT_BF16, dtype=torch.bfloat16, device="cuda")
        out = torch.full((r.B, r.heads, r.T, r.hidden // r.heads), SENT_BF16, dtype=torch.bfloat16, device="cuda")
        ops.qkv_attention(x, w, r.B, r.T, r.heads, bias=bias, cond_tokens=r.S, max_wgs=r.wgs, out=out, qkv=qkv, **kw)
        assert bool((qkv == SENT_BF16).all()), "%s: the fused form wrote to the q | k | v workspace" % (r,)
        outs.append(out)
    for i in (1, 2):
        assert torch.equal(outs[0], outs[i]), "%s: launch %d differs from launch 0 in %d elements" % (r, i, int((outs[0] != outs[i]).sum()))
    return outs[0]


def flat(t):
    return t.reshape(-1, t.shape[-1])


# ------------------------------------------------------------------------------------------------------------- (1) gather probe, tolerance 0
@pytest.mark.parametrize("r", PLAIN)
def test_gather_probe_through_the_projection(r):
    """X = [Q | K | V] rows of attention_gather_probe (keys salted per head) and W = the identity (K_gemm = 3 hidden; cross: X = Q, W = I, K | V
    cached): O == V[pi] to the bit, without a bias and with an all-zero one (both pointer paths of the epilogue).  The row's own K does not
    enter (the projection's K is 3 hidden / hidden here); its B, width and workgroup cap do."""
    cross = r.route == CROSS
    x, w, kv, want = kc.gather_projection_probe(r.B, r.heads, r.T, r.S if cross else r.T, DH, r.B + r.T, cross=cross)
    g = r._replace(K=w.shape[1])
    if ops.qkv_attention_route(g.B, g.T, g.hidden, g.heads, g.K, cond_tokens=g.S, max_wgs=g.wgs) != r.route:
        pytest.fail("%s: at K = %d the gather probe no longer runs the row's form" % (r, g.K))
    xd, wd = dev(x, torch.bfloat16), dev(w, torch.bfloat16)
    for bias in (None, torch.zeros(w.shape[0], device="cuda")):
        out = launch3(g, xd, wd, bias, kv)
        kc.assert_elementwise(flat(out), flat(want).double(), 0.0, "gather probe%s, %s" % (" + zero bias" if bias is not None else "", r))


# ------------------------------------------------------------------------------------------------------------- (2) exact projection
@pytest.mark.parametrize("r", PLAIN)
def test_exact_projection_probe(r):
    """Operands whose q | k | v are known to the bit (integers / 8): the fused output meets the plain attention bound against float64 with no
    allowance for the projection.  On the same operands the GEMM + attention kernel pair reproduces q | k | v exactly, and the 256-token form
    (the same attn_tile_joint loop on identical inputs) equals its O bit for bit."""
    cross = r.route == CROSS
    C, M = r.hidden, r.B * r.T
    N = C if cross else 3 * C
    x, w, bias, y = kc.exact_projection_probe(M, N, r.K, r.B * 7 + r.K, device="cuda")
    xd, wd, bd = dev(x, torch.bfloat16), dev(w, torch.bfloat16), dev(bias)
    if cross:
        kv = (torch.randn(r.B * r.S, 2 * C, generator=torch.Generator().manual_seed(r.B)) * 1.5).bfloat16()
        k64, v64 = dev(kv[:, :C]).double(), dev(kv[:, C:]).double()
        q64 = y
    else:
        kv = None
        q64, k64, v64 = y[:, :C], y[:, C:2 * C], y[:, 2 * C:]
    Nk = r.S if cross else r.T
    out = launch3(r, xd, wd, bd, kv)
    ref, vmax = kc.attention_ref64(q64, k64, v64, r.B, r.heads, r.T, Nk, DH)
    ratio = kc.assert_elementwise(flat(out), flat(ref), flat(kc.attention_base_tol(ref, vmax)), "exact projection probe, %s" % (r,))
    print("worst err / tol %.3f (exact projection, %s)" % (note("fused %s, exact projection" % FORM[r.route], ratio), FORM[r.route]))
    del ref
    # the two-kernel path on the same operands
    assert ops.gemm_route(EPI_BF16, M, N, r.K, max_wgs=r.wgs).family != "none"
    from ldt_amd import _lib
    assert int(_lib.lib().ldt_attention_route(r.B, r.heads, r.T, Nk, DH)) == (2 if r.T == 256 else 1)
    qkv = ops.gemm_bf16(xd, wd, bd, EPI_BF16)
    assert torch.equal(qkv.double(), y), "GEMM: q | k | v of the exact probe differ from the known values in %d elements" % int((qkv.double() != y).sum())
    if cross:
        kvd = dev(kv)
        two = ops.attention_fwd(qkv, kvd[:, :C], kvd[:, C:], r.B, r.heads, r.T, Nk, DH)
    else:
        two = ops.attention_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], r.B, r.heads, r.T, Nk, DH)
    if r.route == SELF256:
        kc.assert_elementwise(flat(out), flat(two).double(), 0.0, "fused 256-token form vs GEMM + whole-head attention kernel, %s" % (r,))
    else:
        print("fused vs two kernels: %d of %d elements differ (%s)" % (int((out != two).sum()), out.numel(), FORM[r.route]))


# ------------------------------------------------------------------------------------------------------------- (3) randn data, two-stage bound
def mm64(a, b):
    return dev(a).double() @ dev(b).double().T


def randn_case(r, device="cuda"):
    """Operands of row r and the float64 projection with its accumulation bound, everything but the draw on `device`.  Plain: X ~ N(0, 1),
    W ~ N(0, 1 / K), bias 0.1 N(0, 1).  Folded: xs with a row mean that is not small (* 1.2 + 0.4 as _consumer_bound) and differs from row to
    row (+ 0.6 N(0, 1) per row: with one common mean the term r mu S is nearly the same for every key, and what is the same for every key —
    a wrong S or C of the k segment — cancels in the softmax: rstd mean has a spread of 0.5 instead of 0.05), statistics given exactly in fp32, random S | C at half scale like W (at full scale tol / base passes its cap of 8 at K = 1024: test_kernel_checks_host.
    folded_case), laid out as the forward's table [steps][S (3 hidden) | C (3 hidden) | ...] and read at step 2 of 3 (the others NaN)."""
    g = torch.Generator().manual_seed(r.B * 11 + r.T + r.K + r.fold)
    C, M = r.hidden, r.B * r.T
    N = C if r.route == CROSS else 3 * C
    to = lambda t, dt=None: t.to(device, dt) if dt else t.to(device)
    if not r.fold:
        x = torch.randn(M, r.K, generator=g).bfloat16().float()
        w = (torch.randn(N, r.K, generator=g) / r.K ** 0.5).bfloat16().float()
        bias = 0.1 * torch.randn(N, generator=g)
        kv = (torch.randn(r.B * r.S, 2 * C, generator=g) * 1.5).bfloat16() if r.route == CROSS else None
        xd, wd = to(x).double(), to(w).double()
        pre = xd @ wd.T + to(bias).double()
        acc = (xd.abs() @ wd.abs().T + to(bias).double().abs()) * (kc.C_ACC * r.K * kc.U24)
        return dict(x=x, w=w, bias=bias, kv=kv, pre=pre, acc=acc)
    xs = torch.randn(M, r.K, generator=g) * 1.2 + 0.4
    w = (0.5 * torch.randn(N, r.K, generator=g) / r.K ** 0.5).bfloat16().float()
    S, Cc = 0.5 * torch.randn(N, generator=g), 0.5 * torch.randn(N, generator=g)
    xs = (xs + 0.6 * torch.randn(M, 1, generator=g)).bfloat16().float()
    t = to(xs).double().view(M, r.K // r.fold, r.fold)
    stats = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()          # [K / granule, M, 2]
    xd, wd = to(xs).double(), to(w).double()
    pre, acc = kc.consumer_pre64(xs, w, to(S), to(Cc), stats, r.K, mm=xd @ wd.T, mm_abs=xd.abs() @ wd.abs().T)
    stride = 2 * N + 64
    table = torch.full((3, stride), float("nan"))
    table[2, :N], table[2, N:2 * N] = S, Cc
    return dict(x=xs, w=w, stats=stats, table=table, stride=stride, pre=pre, acc=acc, kv=None, bias=None)


def reference(r, p):
    C = r.hidden
    kv = None if p["kv"] is None else (p["kv"][:, :C].to(p["pre"].device), p["kv"][:, C:].to(p["pre"].device))
    ref, tol, ratio, amb = kc.fused_attention_tol(p["pre"], p["acc"], r.B, r.heads, r.T, DH, kv=kv, Nk=r.S or None)
    med, mx = kc.assert_ratio_caps(ratio, str(r))
    return ref, tol, (amb, med, mx)


@pytest.mark.parametrize("r", TAKEN)
def test_randn_two_stage_bound_vs_float64(r):
    """The contract — q | k | v = bf16(fp32 accumulation), attention with P rounded to bf16, O bf16 — against float64 attention of the
    bf16-rounded float64 projection, with kernel_checks.fused_attention_tol's allowance for the elements whose rounding depends on the
    summation order.  Nothing in the bound is read from the kernel; its widening over the plain attention bound is capped (median 3, max 8)."""
    t0 = time.time()
    p = randn_case(r)
    N = p["w"].shape[0]
    xd, wd = dev(p["x"], torch.bfloat16), dev(p["w"], torch.bfloat16)
    if r.fold:
        table = dev(p["table"])
        step = torch.tensor([2], dtype=torch.int32, device="cuda")
        out = launch3(r, xd, wd, stats=p["stats"], fold_s=table[0, :N], fold_c=table[0, N:2 * N], fold_step_stride=p["stride"], step_ptr=step)
    else:
        out = launch3(r, xd, wd, dev(p["bias"]), p["kv"])
    ref, tol, widen = reference(r, p)
    kind = "fused %s%s, randn" % (FORM[r.route], ", folded" if r.fold else "")
    ratio = note(kind, kc.assert_elementwise(flat(out), flat(ref), flat(tol), "%s, %s" % (kind, r)))
    WIDEN[str(r)] = widen
    print("worst err / tol %.3f; ambiguous %.1f %%, tol / base median %.2f max %.2f; %.1f s (%s)" % ((ratio, 100 * widen[0]) + widen[1:] + (time.time() - t0, kind)))


# ------------------------------------------------------------------------------------------------------------- the two-kernel path of the entry
@pytest.mark.parametrize("r", [_row("s256", 9, 256, 1024, 16, 1024, 0), _row("x32", 4, 32, 1024, 16, 1024, 0, S=32), _row("s32", 6, 32, 1024, 16, 1024, 0),
                               _row("s256", 9, 256, 1024, 16, 1024, 0, fold=256)])
def test_route_zero_is_gemm_plus_attention_kernel(r):
    """Where no fused form takes the shape the entry runs the GEMM into the workspace and the attention kernel: equal to the two ops calls."""
    check_route(r)
    p = randn_case(r._replace(route=CROSS if r.S else 0))
    C, M = r.hidden, r.B * r.T
    N = p["w"].shape[0]
    xd, wd = dev(p["x"], torch.bfloat16), dev(p["w"], torch.bfloat16)
    qkv = torch.full((M, 3 * C), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    if r.fold:
        table = dev(p["table"])
        step = torch.tensor([2], dtype=torch.int32, device="cuda")
        out = ops.qkv_attention(xd, wd, r.B, r.T, r.heads, stats=p["stats"], fold_s=table[0, :N], fold_c=table[0, N:2 * N], fold_step_stride=p["stride"],
                                step_ptr=step, qkv=qkv)
        want = ops.gemm_lnfold(xd, wd, p["stats"], table[2, :N].contiguous(), table[2, N:2 * N].contiguous())
    else:
        kvd = None if p["kv"] is None else dev(p["kv"])
        out = ops.qkv_attention(xd, wd, r.B, r.T, r.heads, bias=dev(p["bias"]), kv_cond=kvd, cond_tokens=r.S, qkv=qkv)
        want = ops.gemm_bf16(xd, wd, dev(p["bias"]), EPI_BF16)
    assert torch.equal(qkv[:, :N], want) and (N == 3 * C or bool((qkv[:, N:] == SENT_BF16).all()))
    k, v = (kvd[:, :C], kvd[:, C:]) if r.S else (want[:, C:2 * C], want[:, 2 * C:])
    assert torch.equal(out, ops.attention_fwd(want[:, :C], k, v, r.B, r.heads, r.T, r.S or r.T, C // r.heads))


# ------------------------------------------------------------------------------------------------------------- guard bands
def embed(t, top=8, left=64, bottom=8, right=64):
    big = torch.full((t.shape[0] + top + bottom, t.shape[1] + left + right), float("nan"), dtype=t.dtype, device=t.device)
    big[top:top + t.shape[0], left:left + t.shape[1]] = t
    return big[top:top + t.shape[0], left:left + t.shape[1]]


@pytest.mark.parametrize("r", [_row("s256", 17, 256, 1024, 16, 512, SELF256), _row("s256", 17, 256, 1024, 16, 512, SELF256, fold=256),
                               _row("s32", 64, 32, 256, 4, 512, SELF32), _row("s32", 64, 32, 256, 4, 512, SELF32, fold=32),
                               _row("x32", 32, 32, 1024, 16, 1024, CROSS, S=32, kvpad=True)])
def test_leading_dims_and_guard_bands(r):
    """X and W as interiors of NaN-surrounded buffers (ldx > K, ldw > K), the cross form's K | V inside NaN-padded rows, O as the interior of a
    sentinel-filled buffer, the q | k | v workspace filled with a sentinel: the result equals the dense call bit for bit, no sentinel outside O
    is touched, the workspace is untouched (q | k | v never reach HBM) and no NaN gets in."""
    p = randn_case(r)
    N = p["w"].shape[0]
    xd, wd = dev(p["x"], torch.bfloat16), dev(p["w"], torch.bfloat16)
    kw = {}
    if r.fold:
        table = dev(p["table"])
        kw = dict(stats=p["stats"], fold_s=table[0, :N], fold_c=table[0, N:2 * N], fold_step_stride=p["stride"], step_ptr=torch.tensor([2], dtype=torch.int32, device="cuda"))
    bias = None if r.fold else dev(p["bias"])
    dense = launch3(r._replace(kvpad=False), xd, wd, bias, p["kv"], **kw)
    n = dense.numel()
    big = torch.full((n + 512,), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    out = big[256:256 + n].view_as(dense)
    qkv = torch.full((r.B * r.T, 3 * r.hidden), SENT_BF16, dtype=torch.bfloat16, device="cuda")
    check_route(r)
    ops.qkv_attention(embed(xd), embed(wd), r.B, r.T, r.heads, bias=bias, cond_tokens=r.S, max_wgs=r.wgs, out=out, qkv=qkv, **dict(kw, **kv_operand(r, p["kv"])))
    what = "%s in larger buffers" % (r,)
    assert bool((big[:256] == SENT_BF16).all()) and bool((big[256 + n:] == SENT_BF16).all()), what + ": wrote outside O"
    assert bool((qkv == SENT_BF16).all()), what + ": wrote to the q | k | v workspace"
    assert not bool(torch.isnan(out.float()).any()), what + ": NaN from outside an operand reached the result"
    kc.assert_elementwise(flat(out), flat(dense).double(), 0.0, what + " vs the dense call")


def test_zz_margins():
    """Printed last: the worst err / tol per class of check and how far the rounding-flip allowance widened the plain attention bound
    (DESIGN.md section 3 quotes them).  A ratio above 1 fails its own test; a class at 0.05 would mean its bound is too loose to be worth having."""
    for kind in sorted(RATIOS):
        print("margin  %-50s worst err / tol %.3f" % (kind, RATIOS[kind]))
    if WIDEN:
        print("tol / base over %d randn cases: ambiguous %.1f .. %.1f %%, medians %.2f .. %.2f, maxima %.2f .. %.2f" % (
            len(WIDEN), 100 * min(v[0] for v in WIDEN.values()), 100 * max(v[0] for v in WIDEN.values()), min(v[1] for v in WIDEN.values()),
            max(v[1] for v in WIDEN.values()), min(v[2] for v in WIDEN.values()), max(v[2] for v in WIDEN.values())))
    assert all(v <= 1.0 for v in RATIOS.values())
