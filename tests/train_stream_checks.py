"""The Score-training stream kernels (csrc/score_bwd.hip, csrc/optim.hip) at width and past their grid caps: the case lists, an fp32 CPU
emulation of every kernel in the kernel's own order, and the faults planted on it.  Imported by test_train_stream_host.py (CPU: the faithful
emulation is inside the reference's bound at every case, every planted fault is caught) and test_gpu_train_stream_exact.py (-m gpu: the
kernels themselves on the same cases, judged by the same check functions).

References and bounds are kernel_checks' (layernorm_modulate_bwd_ref, gelu_bwd_ref, gate_residual_bwd_ref, silu_bwd_ref, dsm_loss_bwd_ref,
colsum_ref, embedding_grad_ref, transpose_cast_want, adam_ema_ref); nothing here holds a tolerance of its own.

Layout of a case.  Every 2-D operand is a column block `blk(buf, at)` of a wider buffer, `at` = (first row, first column, rows, columns): the
buffers travel to the device whole and the views are formed there, so a kernel sees row strides that differ from C and from each other.  A
destination is the interior of a buffer filled with kernel_checks.SENT_F32 (-2^127, exact in bf16 too): `assert_outside_unchanged` compares
every bit outside the destination with the buffer before the call, and an element the kernel owes but never wrote still holds the sentinel,
which no bound admits.

An emulation takes its geometry as arguments — the row strides through the views, `sweep` (threads of a capped grid), `slices` (row
slices of a column reduction), `rows_per_wg` (rows per workgroup of the LayerNorm row kernel) — and `fault`, one of

  first_sweep     a grid-stride loop that does not loop: elements past the first sweep stay unwritten
  ld_is_C         every row operand addressed with row stride C instead of its own
  skip_row_tail   the last, partial group of rows_per_wg rows is not processed
  drop_slices     slices 8-15 of a column reduction are dropped (their rows are neither summed nor, in the gate kernel, written)
  tail_lane       the column guard of the last pass is `c <= C`: lane C % 64 reads, and writes, one column further
  frozen_sample   the loss backward takes its sample index once, at the start of the thread's first sweep
  lerp_form       Adam's first moment by at::lerp's first form where the weight selects the second
  ema_absent      the EMA is written although none was passed (into the buffer the caller hands over as a guard)
  skip_blocks     the label-embedding gradient covers the first 256 columns only

`faults_of(...)` of each family lists the ones that can show at a case (ld_is_C needs ld != C, drop_slices more than 8 rows per sample, ...).
lerp_form is special: both forms are correct interpolations that differ by at most 2^-24 |g - m|, one sixteenth of what adam_ema_ref allows
for the change, so no bound separates them.  The kernel spells every operation of exp_avg and exp_avg_sq out (`fp contract(off)`, explicit
fmaf, IEEE product and difference), so those two buffers are held bit for bit to the emulation as well (fma32x is an exact fused
multiply-add), and that comparison is what catches it."""
import functools

import numpy as np
import torch

import kernel_checks as kc

SENT = kc.SENT_F32
WAVE = 64
ROWS_PER_WG = 4                    # ln_mod_bwd_rows_kernel: one wave per row, 256 threads
RED_COLS, RED_SLICES = 64, 16      # column reductions of score_bwd.hip
EMB_BLOCK = 256                    # embedding_grad_kernel: columns per block
SWEEP_4096 = 4096 * 256            # gelu_bwd, adam_ema_step: threads of the capped grid
SWEEP_2048 = 2048 * 256            # silu_bwd, dsm_loss_bwd
TAIL = 259                         # elements past the last full sweep: no multiple of 64 or 256
GELU_EDGES = (-12.0, -6.0, -3.0, -0.0, 0.0, 3.0, 6.0, 12.0)
SILU_EDGES = (-30.0, -0.0, 0.0, 30.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- views and guard bands
def blk(buf, at):
    r0, c0, M, C = at
    return buf[r0:r0 + M, c0:c0 + C]


def restride(v, ld=None, cols=None):
    """The 2-D view v re-addressed from its first element with row stride `ld` and `cols` columns (defaults: its own)."""
    return v.as_strided((v.shape[0], v.shape[1] if cols is None else cols), (v.stride(0) if ld is None else ld, 1), v.storage_offset())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_outside_unchanged(before, after, ats, what):
    """Every bit of the 2-D (or flat, with ats = [(start, stop)]) buffer `after` outside the destination blocks `ats` is the bit of `before`."""
    before, after = before.cpu(), after.cpu()
    keep = torch.ones(before.shape, dtype=torch.bool)
    for at in ats:
        if before.dim() == 1:
            keep[at[0]:at[1]] = False
        else:
            keep[at[0]:at[0] + at[2], at[1]:at[1] + at[3]] = False
    bad = (_bits(before) != _bits(after)) & keep
    if bool(bad.any()):
        raise AssertionError("%s: %d element(s) outside the destination changed, first at %s" % (what, int(bad.sum()), torch.nonzero(bad)[0].tolist()))


def sentinel(rows, cols, dtype=torch.float32):
    return torch.full((rows, cols), SENT, dtype=dtype)


class Worst:
    """max err / tol over the assert_elementwise calls of one check."""
    def __init__(self):
        self.r = 0.0

    def __call__(self, out, ref, tol, what):
        self.r = max(self.r, kc.assert_elementwise(out.cpu(), ref, tol, what))


# ------------------------------------------------------------------------------------------------------------- arithmetic of the kernels
def fma32x(a, b, c):
    """float32 fma(a, b, c), exactly: the product of two fp32 values is exact in float64, the sum is rounded to odd there (TwoSum gives the
    sign of what the float64 sum dropped), and 53 >= 2 x 24 + 2 bits make the final rounding to fp32 the single rounding of the exact value."""
    a, b, c = [np.asarray(t, dtype=np.float64) for t in (a, b, c)]
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return torch.from_numpy(s.astype(np.float32))


def lane_sum(v):
    """fp32 [M, C] -> [M, 1]: wave_sum of per-lane partial sums over c = lane, lane + 64, ... (a lane past C adds nothing), the xor butterfly
    32, 16, ..., 1 — after which every lane holds the same bits."""
    M, C = v.shape
    passes = -(-C // WAVE)
    pad = torch.zeros(M, passes * WAVE, dtype=torch.float32)
    pad[:, :C] = v
    pad = pad.view(M, passes, WAVE)
    s = torch.zeros(M, WAVE, dtype=torch.float32)
    for p in range(passes):
        s = s + pad[:, p]
    lane = torch.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, :1].clone()


def slice_sum(terms, slices=RED_SLICES, fault=None):
    """fp32 terms [S, rows, C] -> float64 [S, C]: slice k sums rows k, k + slices, ... front to back in float64, the slices are added in index
    order (slices_sum_fixed)."""
    S, rows, C = terms.shape
    t64 = terms.double()
    tot = torch.zeros(S, C, dtype=torch.float64)
    for k in range(slices // 2 if fault == "drop_slices" else slices):
        acc = torch.zeros(S, C, dtype=torch.float64)
        for t in range(k, rows, slices):
            acc = acc + t64[:, t]
        tot = tot + acc
    return tot


def _written_rows(rows, slices, fault):
    """Rows of a sample that a column kernel's slices visit."""
    t = torch.arange(rows)
    return t[(t % slices) < slices // 2] if fault == "drop_slices" else t


def _col_count(C, fault):
    return C + 1 if fault == "tail_lane" else C


# ------------------------------------------------------------------------------------------------------------- LayerNorm + modulate, gate
LN_GATE_SHAPES = ((21, 7, 1024), (34, 17, 120), (5, 1, 40))        # (M, rows_per_sample, C)
LN_OFFSET_CASE = (21, 7, 1024, 10.0)


@functools.lru_cache(maxsize=None)
def ln_gate_case(M, rps, C, offset=0.0):
    """x, dy, dx and a, da as column blocks of five buffers with five row strides, dx and da inside sentinel, scale / gate blocks 1 / 2 of
    [S, 6 C] modulation rows, dshift / dscale / dgate blocks 0 / 1 / 2 of a sentinel [S, 6 C]."""
    g = gen(M * 1000 + rps * 10 + C + int(offset))
    S = M // rps
    c = dict(M=M, rps=rps, C=C, S=S, offset=offset, ref={})
    c["x"] = torch.randn(M, C + 8, generator=g) * 1.7 + offset * 1.7 + torch.randn(M, 1, generator=g) * 0.3
    c["dy"] = torch.randn(M, C + 24, generator=g)
    c["dx"] = sentinel(M + 2, C + 40)
    c["a"] = torch.randn(M, C + 12, generator=g)
    c["a16"] = c["a"].bfloat16()
    c["da"] = sentinel(M + 2, C + 20, torch.bfloat16)
    c["mod"] = torch.randn(S, 6 * C, generator=g) * 0.3
    c["dmod"] = sentinel(S, 6 * C)
    c["at"] = dict(x=(0, 3, M, C), dy=(0, 16, M, C), dx=(1, 20, M, C), a=(0, 5, M, C), da=(1, 7, M, C), scale=(0, C, S, C), gate=(0, 2 * C, S, C),
                   dshift=(0, 0, S, C), dscale=(0, C, S, C), dgate=(0, 2 * C, S, C))
    c["dx0"] = torch.randn(M, C, generator=g)
    blk(c["dx"], c["at"]["dx"]).copy_(c["dx0"])
    return c


def ln_faults_of(c):
    return ["ld_is_C"] + (["skip_row_tail"] if c["M"] % ROWS_PER_WG else []) + (["drop_slices"] if c["rps"] > RED_SLICES // 2 else []) + \
        (["tail_lane"] if c["C"] % WAVE else [])


def ln_emu(c, use_scale=True, want_mod=True, fault=None, rows_per_wg=ROWS_PER_WG, slices=RED_SLICES):
    """ldt_layernorm_modulate_bwd on copies of the case's destinations -> {'dx', 'dmod'} whole buffers."""
    M, rps, C, S, at = c["M"], c["rps"], c["C"], c["S"], c["at"]
    dxb, dmod = c["dx"].clone(), c["dmod"].clone()
    x, dy, dx, scale = blk(c["x"], at["x"]), blk(c["dy"], at["dy"]), blk(dxb, at["dx"]), blk(c["mod"], at["scale"])
    if fault == "ld_is_C":
        x, dy, dx = restride(x, C), restride(dy, C), restride(dx, C)
    Cl = _col_count(C, fault)
    xw, gw, dw, sw = [restride(t, cols=Cl) for t in (x, dy, dx, scale)]
    rows = M // rows_per_wg * rows_per_wg if fault == "skip_row_tail" else M
    stats = torch.zeros(M, 2, dtype=torch.float32)
    Cf = torch.tensor(float(C), dtype=torch.float32)
    xr = xw[:rows]
    s1 = 1.0 + sw[torch.arange(rows) // rps] if use_scale else torch.ones(rows, Cl)
    mean = lane_sum(xr) / Cf
    d = xr - mean
    rstd = torch.rsqrt(lane_sum(d * d) / Cf + 1e-6)
    gg = gw[:rows] * s1
    xh = d * rstd
    mg, mgx = lane_sum(gg) / Cf, lane_sum(gg * xh) / Cf
    dw[:rows] += rstd * ((gg - mg) - xh * mgx)
    stats[:rows, 0:1], stats[:rows, 1:2] = mean, rstd
    if want_mod:
        xs = (restride(x, cols=Cl) - stats[:, 0:1]) * stats[:, 1:2]
        gs = restride(dy, cols=Cl)
        restride(blk(dmod, at["dshift"]), cols=Cl).copy_(slice_sum(gs.reshape(S, rps, Cl), slices, fault).float())
        restride(blk(dmod, at["dscale"]), cols=Cl).copy_(slice_sum((gs * xs).reshape(S, rps, Cl), slices, fault).float())
    return {"dx": dxb, "dmod": dmod}


def ln_check(c, out, use_scale=True, want_mod=True):
    """-> worst err / tol.  dx, dshift, dscale inside layernorm_modulate_bwd_ref's bounds, every other bit of both buffers unchanged."""
    M, rps, C, S, at = c["M"], c["rps"], c["C"], c["S"], c["at"]
    key = ("ln", use_scale)
    if key not in c["ref"]:
        scale = blk(c["mod"], at["scale"]) if use_scale else torch.zeros(S, C)
        c["ref"][key] = kc.layernorm_modulate_bwd_ref(blk(c["x"], at["x"]), blk(c["dy"], at["dy"]), scale, rps, c["dx0"])
    ref, tol, (mean, var) = c["ref"][key]
    if c["offset"]:
        assert 50 < float((mean ** 2 / var).min())
    w = Worst()
    what = "layernorm_modulate_bwd (M %d, rps %d, C %d)" % (M, rps, C)
    w(blk(out["dx"], at["dx"]), ref["dx"], tol["dx"], what + " dx")
    assert_outside_unchanged(c["dx"], out["dx"], [at["dx"]], what + " dx")
    if want_mod:
        w(blk(out["dmod"], at["dshift"]), ref["dshift"], tol["dshift"], what + " dshift")
        w(blk(out["dmod"], at["dscale"]), ref["dscale"], tol["dscale"], what + " dscale")
    assert_outside_unchanged(c["dmod"], out["dmod"], [at["dshift"], at["dscale"]] if want_mod else [], what + " dmod")
    return w.r


def gate_faults_of(c):
    return ["ld_is_C"] + (["drop_slices"] if c["rps"] > RED_SLICES // 2 else []) + (["tail_lane"] if c["C"] % WAVE else [])


def gate_emu(c, a_bf16=False, broadcast=False, want_dgate=True, fault=None, slices=RED_SLICES):
    """ldt_gate_residual_bwd -> {'da', 'dmod'} whole buffers.  broadcast: sample 0's gate row for every sample (gate_sample_stride 0)."""
    M, rps, C, S, at = c["M"], c["rps"], c["C"], c["S"], c["at"]
    dab, dmod = c["da"].clone(), c["dmod"].clone()
    dy, a, da, gate = blk(c["dy"], at["dy"]), blk(c["a16" if a_bf16 else "a"], at["a"]), blk(dab, at["da"]), blk(c["mod"], at["gate"])
    if fault == "ld_is_C":
        dy, a, da = restride(dy, C), restride(a, C), restride(da, C)
    Cl = _col_count(C, fault)
    dy, a, da, gate = [restride(t, cols=Cl) for t in (dy, a, da, gate)]
    g = gate[torch.zeros(M, dtype=torch.long) if broadcast else torch.arange(M) // rps]
    t = _written_rows(rps, slices, fault)
    rows = (torch.arange(S)[:, None] * rps + t[None, :]).reshape(-1)
    da[rows] = (dy * g).bfloat16()[rows]
    if want_dgate:
        restride(blk(dmod, at["dgate"]), cols=Cl).copy_(slice_sum((dy * a.float()).reshape(S, rps, Cl), slices, fault).float())
    return {"da": dab, "dmod": dmod}


def gate_check(c, out, a_bf16=False, broadcast=False, want_dgate=True):
    M, rps, C, S, at = c["M"], c["rps"], c["C"], c["S"], c["at"]
    key = ("gate", a_bf16, broadcast)
    if key not in c["ref"]:
        gate = blk(c["mod"], at["gate"])
        c["ref"][key] = kc.gate_residual_bwd_ref(blk(c["dy"], at["dy"]), gate[:1].expand(S, C) if broadcast else gate,
                                                 blk(c["a16" if a_bf16 else "a"], at["a"]), rps)
    ref, tol = c["ref"][key]
    w = Worst()
    what = "gate_residual_bwd (M %d, rps %d, C %d)" % (M, rps, C)
    w(blk(out["da"], at["da"]), ref["da"], tol["da"], what + " da")
    assert_outside_unchanged(c["da"], out["da"], [at["da"]], what + " da")
    if want_dgate:
        w(blk(out["dmod"], at["dgate"]), ref["dgate"], tol["dgate"], what + " dgate")
    assert_outside_unchanged(c["dmod"], out["dmod"], [at["dgate"]] if want_dgate else [], what + " dmod")
    return w.r


# ------------------------------------------------------------------------------------------------------------- GELU backward
GELU_SHAPES = ((257, 4096, False), (259, 4090, True))              # (M, C, strided): both cross the 1,048,576-thread sweep


@functools.lru_cache(maxsize=None)
def gelu_case(M, C, strided, dh_bf16):
    """The edge values sit in the last row: flat index (M - 1) C >= 1,048,576, the second sweep.  Contiguous: ld == C for all three, `out`
    between two sentinel rows; strided: three row strides."""
    g = gen(M + C + dh_bf16)
    pu, pd, po = ((2, 6), (9, 14), (4, 10)) if strided else ((0, 0), (0, 0), (0, 0))
    c = dict(M=M, C=C, strided=strided, ref={})
    c["u"] = (torch.randn(M, C + pu[1], generator=g) * 2.5).bfloat16()
    c["dh"] = torch.randn(M, C + pd[1], generator=g).to(torch.bfloat16 if dh_bf16 else torch.float32)
    c["out"] = sentinel(M + 2, C + po[1], torch.bfloat16)
    c["at"] = dict(u=(0, pu[0], M, C), dh=(0, pd[0], M, C), out=(1, po[0], M, C))
    blk(c["u"], c["at"]["u"])[M - 1, :8] = torch.tensor(GELU_EDGES).bfloat16()
    assert (M - 1) * C >= SWEEP_4096
    return c


def gelu_faults_of(c):
    return ["first_sweep"] + (["ld_is_C"] if c["strided"] else [])


def gelu_emu(c, fault=None, sweep=SWEEP_4096):
    M, C, at = c["M"], c["C"], c["at"]
    outb = c["out"].clone()
    u, dh, out = blk(c["u"], at["u"]), blk(c["dh"], at["dh"]), blk(outb, at["out"])
    if fault == "ld_is_C":
        u, dh, out = restride(u, C), restride(dh, C), restride(out, C)
    v = u.float()
    cdf = 0.5 * (1.0 + torch.erf(v * 0.70710678118654752440))
    pdf = 0.39894228040143267794 * torch.exp(-0.5 * v * v)
    val = (dh.float() * (cdf + v * pdf)).bfloat16()
    done = (torch.arange(M)[:, None] * C + torch.arange(C)[None, :]) < (sweep if fault == "first_sweep" else M * C)
    out[done] = val[done]
    return {"out": outb}


def gelu_check(c, out):
    at = c["at"]
    if "gelu" not in c["ref"]:
        c["ref"]["gelu"] = kc.gelu_bwd_ref(blk(c["u"], at["u"]), blk(c["dh"], at["dh"]))
    ref, tol = c["ref"]["gelu"]
    what = "gelu_bwd (%d x %d%s)" % (c["M"], c["C"], ", strided" if c["strided"] else "")
    r = kc.assert_elementwise(blk(out["out"], at["out"]).cpu(), ref, tol, what)
    assert_outside_unchanged(c["out"], out["out"], [at["out"]], what)
    return r


# ------------------------------------------------------------------------------------------------------------- SiLU and loss backward
N_2048 = SWEEP_2048 + TAIL                                          # 524,547: one full sweep of a 2048-block grid + 259


@functools.lru_cache(maxsize=None)
def silu_case():
    g = gen(3)
    c = dict(n=N_2048, ref={})
    c["c"], c["dy"] = torch.randn(N_2048, generator=g) * 3, torch.randn(N_2048, generator=g)
    c["c"][SWEEP_2048 + 12:SWEEP_2048 + 16] = torch.tensor(SILU_EDGES)                    # past the cap
    return c


def silu_emu(c, want_act, fault=None, sweep=SWEEP_2048):
    v, dy, n = c["c"], c["dy"], c["n"]
    k = sweep if fault == "first_sweep" else n
    sg = 1.0 / (1.0 + torch.exp(-v))
    out = {"dc": torch.full((n,), SENT)}
    out["dc"][:k] = (dy * (sg * (1.0 + v * (1.0 - sg))))[:k]
    if want_act:
        out["act"] = torch.full((n,), SENT)
        out["act"][:k] = (v / (1.0 + torch.exp(-v)))[:k]
    return out


def silu_check(c, out, want_act):
    if "silu" not in c["ref"]:
        c["ref"]["silu"] = kc.silu_bwd_ref(c["c"], c["dy"])
    ref, tol = c["ref"]["silu"]
    w = Worst()
    w(out["dc"].reshape(1, -1), ref["dc"].reshape(1, -1), tol["dc"].reshape(1, -1), "silu_bwd dc")
    if want_act:
        w(out["act"].reshape(1, -1), ref["act"].reshape(1, -1), tol["act"].reshape(1, -1), "silu_bwd act")
    return w.r


DSM_SHAPE = (3, 501, 349)                                           # per_sample 174,849, n 524,547: sample 2 runs across the cap


@functools.lru_cache(maxsize=None)
def dsm_case():
    g = gen(17)
    B, T, C = DSM_SHAPE
    assert T * C == 174849 and B * T * C == N_2048
    c = dict(B=B, per_sample=T * C, n=B * T * C, ref={})
    c["eta"], c["params"] = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    c["params"].view(-1)[SWEEP_2048 + 100:SWEEP_2048 + 104] = c["eta"].view(-1)[SWEEP_2048 + 100:SWEEP_2048 + 104]        # d = 0 past the cap
    c["w"] = torch.rand(B, generator=g) + 0.5
    return c


def dsm_faults_of(weighted):
    return ["first_sweep"] + (["frozen_sample"] if weighted else [])


def dsm_emu(c, weighted, l1, fault=None, sweep=SWEEP_2048):
    n, ps = c["n"], c["per_sample"]
    i = torch.arange(n)
    sample = (i % sweep if fault == "frozen_sample" else i) // ps
    w = c["w"][sample] if weighted else torch.ones(n)
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    d = c["eta"].reshape(-1) - c["params"].reshape(-1)
    dd = -torch.sign(d) if l1 else -2.0 * d
    k = sweep if fault == "first_sweep" else n
    out = torch.full((n,), SENT)
    out[:k] = (dd * w * inv_n)[:k]
    return {"dparams": out.view(DSM_SHAPE)}


def dsm_check(c, out, weighted, l1):
    key = ("dsm", weighted, l1)
    if key not in c["ref"]:
        c["ref"][key] = kc.dsm_loss_bwd_ref(c["eta"], c["params"], c["w"] if weighted else None, l1)
    ref, tol = c["ref"][key]
    return kc.assert_elementwise(out["dparams"].cpu().reshape(1, -1), ref.reshape(1, -1), tol.reshape(1, -1), "dsm_loss_bwd w=%d l1=%d" % (weighted, l1))


# ------------------------------------------------------------------------------------------------------------- column sum
COLSUM_CASES = ((17, 1024, False), (1, 40, False), (1000, 4096, True))     # (M, C, bf16 column block of a wider matrix)
GUARD = 4096


@functools.lru_cache(maxsize=None)
def colsum_case(M, C, wide_bf16):
    g = gen(M + C)
    c = dict(M=M, C=C, wide=wide_bf16, ref={})
    if wide_bf16:
        c["dy"], c["at"] = torch.randn(M, C + 16, generator=g).bfloat16(), (0, 8, M, C)
    else:
        c["dy"], c["at"] = torch.randn(M, C, generator=g), (0, 0, M, C)
    c["out"] = torch.full((C + 2 * GUARD,), SENT)
    return c


def colsum_faults_of(c):
    return (["ld_is_C"] if c["wide"] else []) + (["drop_slices"] if c["M"] > RED_SLICES // 2 else []) + (["tail_lane"] if c["C"] % RED_COLS else [])


def colsum_emu(c, fault=None, slices=RED_SLICES):
    M, C = c["M"], c["C"]
    dy = blk(c["dy"], c["at"])
    if fault == "ld_is_C":
        dy = restride(dy, C)
    Cl = _col_count(C, fault)
    if fault == "tail_lane" and not c["wide"]:                      # a contiguous operand has no column C: the next row's (or, after the last, nothing)
        dy = torch.cat([dy, torch.ones(M, 1, dtype=dy.dtype)], 1)
    else:
        dy = restride(dy, cols=Cl)
    out = c["out"].clone()
    out[GUARD:GUARD + Cl] = slice_sum(dy.float()[None], slices, fault)[0].float()
    return {"out": out}


def colsum_check(c, out):
    C = c["C"]
    if "colsum" not in c["ref"]:
        c["ref"]["colsum"] = kc.colsum_ref(blk(c["dy"], c["at"]))
    ref, tol = c["ref"]["colsum"]
    what = "colsum (%d x %d)" % (c["M"], C)
    r = kc.assert_elementwise(out["out"][GUARD:GUARD + C].cpu().reshape(1, -1), ref.reshape(1, -1), tol.reshape(1, -1), what)
    assert_outside_unchanged(c["out"], out["out"], [(GUARD, GUARD + C)], what)
    return r


# ------------------------------------------------------------------------------------------------------------- label embedding
EMB_CASES = ((5, 1024, 3, 1032, (2, 0, 2, 2, 0)), (2, 300, 2, 300, (1, 1)))      # (B, D, K, ld, labels): class 1 / class 0 is absent


@functools.lru_cache(maxsize=None)
def emb_case(B, D, K, ld, labels):
    g = gen(B + D)
    c = dict(B=B, D=D, K=K, ld=ld, ref={})
    c["dc"], c["at"] = torch.randn(B, ld, generator=g), (0, (ld - D) // 2, B, D)
    c["label"] = torch.tensor(labels)
    c["absent"] = [k for k in range(K) if k not in labels]
    return c


def emb_faults_of(c):
    return ["skip_blocks"] + (["ld_is_C"] if c["ld"] != c["D"] else [])


def emb_emu(c, fault=None, block=EMB_BLOCK):
    B, D, K = c["B"], c["D"], c["K"]
    dc = blk(c["dc"], c["at"])
    if fault == "ld_is_C":
        dc = restride(dc, D)
    out = sentinel(K, D)
    Dw = min(D, block) if fault == "skip_blocks" else D
    for k in range(K):
        acc = torch.zeros(D, dtype=torch.float32)
        for b in range(B):
            if int(c["label"][b]) == k:
                acc = acc + dc[b]
        out[k, :Dw] = acc[:Dw]
    return {"dE": out}


def emb_check(c, out):
    if "emb" not in c["ref"]:
        c["ref"]["emb"] = kc.embedding_grad_ref(blk(c["dc"], c["at"]), c["label"], c["K"])
    ref, tol = c["ref"]["emb"]
    r = kc.assert_elementwise(out["dE"].cpu(), ref, tol, "embedding_grad (B %d, D %d)" % (c["B"], c["D"]))
    for k in c["absent"]:
        assert float(out["dE"][k].abs().max()) == 0.0, "embedding_grad: the row of class %d, which nobody carries, is not exactly zero" % k
    return r


# ------------------------------------------------------------------------------------------------------------- transposing cast
TRANSPOSE_SHAPES = ((1, 40), (33, 33))


@functools.lru_cache(maxsize=None)
def transpose_case(R, C, src_bf16):
    """src: a column block of a wider matrix; dst: [C, pad64(R)] inside a bf16 buffer of 7.0 with a row above, a row below and 64 columns to
    the right (as test_transpose_cast_is_exact_and_zero_pads builds it)."""
    g = gen(R * 7 + C)
    Rp = kc.pad64(R)
    c = dict(R=R, C=C, Rp=Rp)
    src = torch.randn(R, C + 8, generator=g)
    c["src"], c["at_src"] = (src.bfloat16() if src_bf16 else src), (0, 5, R, C)
    c["dst"], c["at_dst"] = torch.full((C + 2, Rp + 64), 7.0, dtype=torch.bfloat16), (1, 0, C, Rp)
    c["want"] = kc.transpose_cast_want(blk(c["src"], c["at_src"]), Rp)
    return c


def transpose_emu(c, fault=None):
    R, C, Rp = c["R"], c["C"], c["Rp"]
    src = blk(c["src"], c["at_src"])
    if fault == "ld_is_C":
        src = restride(src, C)
    dstb = c["dst"].clone()
    dst = blk(dstb, c["at_dst"])
    dst[:, :R] = src.bfloat16().t()
    dst[:, R:] = 0
    return {"dst": dstb}


def transpose_check(c, out):
    what = "transpose_cast_bf16 (%d x %d)" % (c["R"], c["C"])
    assert torch.equal(blk(out["dst"], c["at_dst"]).cpu(), c["want"]), what + ": not bf16(src)^T with zero padding"
    assert_outside_unchanged(c["dst"], out["dst"], [c["at_dst"]], what)
    return 0.0


# ------------------------------------------------------------------------------------------------------------- Adam + EMA
ADAM_HYPER = dict(lr=2e-3, b2=0.999, eps=1e-8, decay=0.98)
ADAM_TAIL = 4096                                                    # sentinel elements after the n the kernel is given
N_ADAM = 2 * SWEEP_4096 + TAIL                                      # 2,097,411: two full sweeps + 259
ADAM_ZERO = (SWEEP_4096 + 1000, SWEEP_4096 + 1064)                  # g = m = v = 0, past the first sweep
ADAM_VARIANTS = ("lerp2", "no_ema")                                 # beta1 0.4 (w1 = 0.6: at::lerp's second form) | ema = None


def _oversized(t):
    return torch.cat([t, torch.full((ADAM_TAIL,), SENT)])


@functools.lru_cache(maxsize=None)
def adam_main_case():
    """One step at step 100000 from a seeded late state, weight_decay 0, |g| over sixteen decades.  late: m + w1 (g - m) can cancel here, so
    the parameter is judged with adam_ema_ref's moment_rounding term (stated there)."""
    g = gen(2024)
    n = N_ADAM
    p = torch.randn(n, generator=g)
    st = {"p": p, "m": 1e-3 * torch.randn(n, generator=g), "v": 1e-6 * torch.rand(n, generator=g)}
    st["ema"] = p + 1e-3 * torch.randn(n, generator=g)
    mag = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 16 - 12).float()
    grad = mag * (1 - 2 * torch.randint(0, 2, (n,), generator=g)).float()
    z0, z1 = ADAM_ZERO
    grad[z0:z1] = 0; st["m"][z0:z1] = 0; st["v"][z0:z1] = 0
    assert float((grad * grad)[grad != 0].min()) >= 2.0 ** -126                       # g g stays a normal fp32
    return dict(n=n, state=st, grads=[grad], steps=[100000], b1=0.9, wd=0.0, ema=True, ema_init=False, zero=ADAM_ZERO, late=True, ref={})


@functools.lru_cache(maxsize=None)
def adam_variant_case(variant, wd):
    """Three steps from zero state at n = 4099 (as test_adam_ema_step_against_torch_adam: the second gradient a tenth of the others)."""
    n = 4099
    g = gen(int(wd * 1000) + len(variant))
    st = {"p": torch.randn(n, generator=g), "m": torch.zeros(n), "v": torch.zeros(n), "ema": None if variant == "no_ema" else torch.zeros(n)}
    grads = [torch.randn(n, generator=g) * (0.1 if s == 2 else 1.0) for s in (1, 2, 3)]
    return dict(n=n, state=st, grads=grads, steps=[1, 2, 3], b1=0.4 if variant == "lerp2" else 0.9, wd=wd, ema=variant != "no_ema",
                ema_init=True, zero=None, late=False, ref={})


def adam_faults_of(c):
    return (["first_sweep"] if c["n"] > SWEEP_4096 else []) + (["lerp_form"] if 1.0 - c["b1"] >= 0.5 else []) + ([] if c["ema"] else ["ema_absent"])


def adam_buffers(st):
    """The state as the oversized buffers a step is given: n elements, then ADAM_TAIL of sentinel.  'guard': what an absent EMA must not reach."""
    b = {k: _oversized(v) for k, v in st.items() if v is not None}
    if st.get("ema") is None:
        b["guard"] = torch.full((st["p"].numel() + ADAM_TAIL,), SENT)
    return b


def adam_emu(c, bufs, grad, step, ema_init, fault=None, sweep=SWEEP_4096):
    """ldt_adam_ema_step (no clip factor) on the oversized buffers `bufs` -> new buffers.  Every operation where the kernel has it: the
    weight-decay sum in float64 rounded once, fmaf = fma32x, the rest one fp32 operation at a time."""
    n, h = c["n"], ADAM_HYPER
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
    w1, w2, eps, wde = f32(1.0 - c["b1"]), f32(1.0 - h["b2"]), f32(h["eps"]), f32(1.0 - h["decay"])
    nss = f32(-(h["lr"] / (1.0 - c["b1"] ** step)))
    bc2s = f32((1.0 - h["b2"] ** step) ** 0.5)
    k = min(n, sweep) if fault == "first_sweep" else n
    out = {nm: t.clone() for nm, t in bufs.items()}
    p, m, v, gi = bufs["p"][:k], bufs["m"][:k], bufs["v"][:k], grad[:k]
    if c["wd"] != 0.0:
        gi = (gi.double() + c["wd"] * p.double()).float()
    if float(w1) < 0.5 or fault == "lerp_form":
        m1 = fma32x(w1, gi - m, m)
    else:
        m1 = fma32x(w1 - 1.0, gi - m, gi)
    v1 = fma32x(w2, gi * gi - v, v)
    p1 = p + (nss * m1) / (torch.sqrt(v1) / bc2s + eps)
    out["p"][:k], out["m"][:k], out["v"][:k] = p1, m1, v1
    ema_to = "ema" if c["ema"] else ("guard" if fault == "ema_absent" else None)
    if ema_to:
        e = p1 if ema_init else bufs[ema_to][:k]
        out[ema_to][:k] = fma32x(wde, p1 - e, e)
    return out


def adam_check(c, before, out, grad, step, ema_init, exact=None):
    """`out` (buffers after the step) against adam_ema_ref from the fp32 state `before` the step: p, exp_avg, exp_avg_sq and the EMA inside the
    bound; the sentinel after element n and an absent EMA's guard untouched; the g = m = v = 0 block's p bit-identical at weight_decay 0;
    exp_avg and exp_avg_sq == `exact` (the faithful emulation of the same step; default: computed here) bit for bit."""
    n, h = c["n"], ADAM_HYPER
    st = {k: (before[k][:n] if k in before else None) for k in ("p", "m", "v", "ema")}
    ref, tol = kc.adam_ema_ref(st, grad, step, h["lr"], c["b1"], h["b2"], h["eps"], c["wd"], h["decay"], ema_init, moment_rounding=c["late"])
    w = Worst()
    for nm, key in (("p", "p"), ("exp_avg", "m"), ("exp_avg_sq", "v")) + ((("ema", "ema"),) if c["ema"] else ()):
        w(out[key][:n].reshape(1, -1), ref[nm].reshape(1, -1), tol[nm].reshape(1, -1), "adam_ema_step %s, step %d" % (nm, step))
    for key in out:
        assert_outside_unchanged(before[key], out[key], [(0, 0)] if key == "guard" else [(0, n)], "adam_ema_step %s, step %d" % (key, step))
    if c["ema"] and ema_init:
        assert torch.equal(out["ema"][:n], out["p"][:n]), "adam_ema_step: the EMA of a first step is not the new parameter"
    if c["zero"] and c["wd"] == 0.0:
        z0, z1 = c["zero"]
        assert torch.equal(_bits(out["p"][z0:z1]), _bits(before["p"][z0:z1])), "adam_ema_step: p moved where g = m = v = 0"
    exact = adam_emu(c, before, grad, step, ema_init) if exact is None else exact
    for key, nm in (("m", "exp_avg"), ("v", "exp_avg_sq")):
        diff = _bits(out[key][:n].cpu()) != _bits(exact[key][:n])
        assert not bool(diff.any()), "adam_ema_step %s, step %d: %d element(s) differ from the spelled-out fp32 chain (first at %d)" % (
            nm, step, int(diff.sum()), int(torch.nonzero(diff)[0]))
    return w.r


def adam_run(c, stepper):
    """Drive a case's steps, every one from the previous one's own output (each step is judged by the one-step bound).
    stepper(bufs, grad, step, ema_init) -> the buffers after the step (CPU).  -> worst err / tol."""
    bufs, worst = adam_buffers(c["state"]), 0.0
    for i, (grad, step) in enumerate(zip(c["grads"], c["steps"])):
        ema_init = c["ema_init"] and i == 0
        new = stepper(bufs, grad, step, ema_init)
        worst = max(worst, adam_check(c, bufs, new, grad, step, ema_init))
        bufs = new
    return worst
