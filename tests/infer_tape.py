"""The call tape of the inference forwards and the audits read from it (a plain helper module: test_gpu_infer_tape.py runs it on the MI355X,
test_infer_tape_host.py on a pure-torch emulation of the entry points, planted faults included).

`Compressor.forward` and `Compressor.sample` reach every kernel through the module attribute `ops` of ldt_amd.compressor and ldt_amd.blocks
(`train_tape.install_infer_ops`); train_tape.Tape records every call made through it: the operands as they were (strided column views as the
values the view shows plus the layout it had), the outputs, and for operands written in place the view and the whole storage, before and after.
  * `audit_numeric`: every call against float64 from its OWN recorded operands, with the reference and the bound that hold that kernel alone
    (kernel_checks, sgemm_checks, the formulas of test_gpu_kernel_exact.py restated in `gemm_reference` / `oproj_reference` below); around
    every destination the storage outside the view unchanged bit for bit.  No bound is new.  Where a reference states conditions on ITS inputs
    (a share of elements it can pin), the in-situ operands are what they are: the per-element bound is asserted, the shares are returned.
  * `audit_forward`, `audit_sample`: what every call's operands MUST be, written down from the reference (model/Compressor/Network.py:188-268,
    model/layers.py:183-246, model/Compressor/layers.py:26-42) and not from compressor.py / blocks.py: each link checked with torch.equal
    between a recorded operand and the recorded output of its producer, a parameter panel of `packed()` or an input, and for a column view its
    storage, offset and strides.  A stage is found by what it reads and writes, in whichever form it runs (one fused kernel or the chain it
    stands for), never by position; no call is left unplaced; the returned tensors are bit-equal to the outputs of the calls the table names.
Not covered (asserted, not assumed): class-conditional forwards, `pos_embedding: mlp`, `pre_group`."""
import copy

import torch

import kernel_checks as kc
import sgemm_checks as sc
import train_tape as tt
from train_tape import _eq, _eqflat

SHARE = " [share]"                                                      # keys of check_call's result that are shares, not err / bound


def _lib():
    from ldt_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------- numeric audit
def sample_rows_of(call, name, stride_arg, src=None):
    """The per-sample rows operand `name` as the KERNEL addresses it (row s at s * `stride_arg` elements behind the view's first): the recorded
    view where its row stride is that stride; its first row for every sample at stride 0."""
    r = (call.args if src is None else src).get(name)
    if r is None:
        return None
    assert isinstance(r, tt.Rec) and r.stride[-1] == 1, "%s: `%s` is not a row-major tensor" % (call, name)
    stride = (call.args if src is None else src).get(stride_arg, 0)
    if r.shape[0] == 1 or r.stride[0] == stride:
        return r.value
    assert stride == 0, "%s: the rows of `%s` lie %d elements apart and the kernel is told %s = %d" % (call, name, r.stride[0], stride_arg, stride)
    return r.value[:1].expand_as(r.value)


def _rows(t, M, rps, call, name):
    rps = rps or M
    need = (M + rps - 1) // rps
    assert t.shape[0] >= need or (t.shape[0] == 1 and rps >= M), "%s: `%s` has %d rows, rows_per_sample = %d asks for %d" % (call, name, t.shape[0], rps, need)
    return kc.sample_rows(t, M, rps)


def gemm_reference(x, w, bias, epilogue, resid=None, skip=None, gate_rows=None):
    """out = epi(x w^T + bias) in float64 and its bound: the formulas test_gpu_kernel_exact._plain_bound holds ldt_gemm_bf16 to, per epilogue
    (gate_rows: the gate expanded to one row per output row).  -> (ref, tol)"""
    L = _lib()
    pre = x.double() @ w.double().T
    if bias is not None:
        pre = pre + bias.double()
    acc = kc.gemm_acc_err(x, w, bias, x.shape[1])
    if epilogue == L.EPI_F32:
        return pre, acc + kc.U24 * pre.abs()
    if epilogue == L.EPI_BF16:
        return pre, acc * (1 + kc.U8) + kc.U8 * pre.abs()
    if epilogue == L.EPI_GELU_BF16:
        ref = torch.nn.functional.gelu(pre)
        return ref, (acc * kc.GELU_SLOPE + kc.GELU_FAST_ABS) * (1 + kc.U8) + kc.U8 * ref.abs()
    if epilogue == L.EPI_RELU_BF16:
        if skip is None:
            ref = torch.relu(pre)
            return ref, acc * (1 + kc.U8) + kc.U8 * ref.abs()
        ref = torch.relu(pre + skip.double())
        return ref, (acc + kc.U24 * (pre.abs() + skip.double().abs())) * (1 + kc.U8) + kc.U8 * ref.abs()
    assert epilogue == L.EPI_RESID_F32, "epilogue %r" % (epilogue,)
    upd = pre if gate_rows is None else gate_rows * pre
    ref = resid.double() + upd
    return ref, (acc if gate_rows is None else gate_rows.abs() * acc) + 2 * kc.U24 * (resid.double().abs() + upd.abs()) + kc.U24 * ref.abs()


def oproj_reference(q, k, v, B, H, Nq, Nk, wo, bo, x0, gate_rows=None):
    """x0 + gate (Wo Attn(q, k, v)' + bo) in float64 and its bound: test_gpu_kernel_exact.test_attention_oproj_bound_vs_float64's (O carries its
    bf16 rounding and that of P through |Wo|, the projection its fp32 accumulation over C terms, the update its gate).  -> (ref, tol)"""
    dh = 32
    C = H * dh
    att, vmax = kc.attention_ref64(q, k, v, B, H, Nq, Nk, dh)
    o = att.reshape(B * Nq, C)                                          # quirk Q1: [B][H][Nq][Dh] re-read raw as (B Nq, C) rows
    e_o = (kc.U8 * (att.abs() + vmax)).reshape(B * Nq, C)
    wa = wo.double().abs()
    upd = o @ wo.double().T + bo.double()
    e_u = 1.01 * (e_o @ wa.T) + C * kc.U24 * (o.abs() @ wa.T + bo.double().abs())
    if gate_rows is not None:
        upd, e_u = gate_rows * upd, gate_rows.abs() * e_u
    return x0.double() + upd, e_u + 2 * kc.U24 * (x0.double().abs() + upd.abs())


def knn_check(idx, xyz, centers, k, what):
    """ldt_knn's neighbour SETS as test_gpu_encoder.test_knn_sets holds them: k distinct indices in range per centre whose sorted distances
    (the reference's expanded form) are the k smallest up to ties at the k-th neighbour."""
    from oracle import ldt_oracle as O
    n = xyz.shape[1]
    idx = idx.cpu().long()
    ref_d = O.square_distance(centers.cpu(), xyz.cpu())
    ref_idx = torch.topk(ref_d, k, dim=-1, largest=False, sorted=False)[1]
    assert tuple(idx.shape) == tuple(ref_idx.shape) and int(idx.min()) >= 0 and int(idx.max()) < n, "%s: indices out of range" % what
    assert all(len(set(r.tolist())) == k for r in idx.reshape(-1, k)), "%s: a neighbour set repeats an index" % what
    got = torch.gather(ref_d, -1, idx).sort(-1)[0]
    want = torch.gather(ref_d, -1, ref_idx).sort(-1)[0]
    assert torch.allclose(got, want, rtol=1e-5, atol=2e-6), "%s: not the k nearest neighbours" % what
    return float((idx.sort(-1)[0] != ref_idx.sort(-1)[0]).any(-1).float().mean())


def _ln_kw(call, src=None, M=None):
    """The LayerNorm arguments of ln_linear / ln_mlp_resid_ (or of a `next_linear` dict) as kernel_checks.ln_stage takes them."""
    A = call.args if src is None else src
    val = lambda k: A[k].value if isinstance(A.get(k), tt.Rec) else None
    kw = dict(ln_w=val("ln_w"), ln_b=val("ln_b"))
    if A.get("shift") is not None:
        kw.update(shift=sample_rows_of(call, "shift", "mod_sample_stride", src), scale=sample_rows_of(call, "scale", "mod_sample_stride", src),
                  rows_per_sample=A.get("rows_per_sample") or M)
        _rows(kw["shift"], M, kw["rows_per_sample"], call, "shift")
    return kw


def check_call(call, ctx=None):
    """One call against float64 from its own recorded operands -> {what: err / bound, or a share under a key ending in SHARE}.
    ctx: {'grouper': [(wimg, w1, b1, w2, b2, w3, b3), ...]}: the panels a fragment image stands for (ldt_grouper_mlp reads only the image)."""
    a, nm = call.arg, call.name
    E = kc.assert_elementwise
    L = _lib()
    what = str(call)
    if nm == "sgemm":
        ref, tol = sc.reference(a("a"), a("w"), a("bias"), a("act_in"), a("act_out"))
        out = call.result()
        key = "sgemm" + ("".join(" %s %s" % (k, sc.ACT_NAMES[v]) for k, v in (("act_in", a("act_in")), ("act_out", a("act_out"))) if v)) + (" bf16 out" if out.dtype == torch.bfloat16 else "")
        if out.dtype != torch.bfloat16:
            return {key: E(out, ref, tol, what)}
        # sgemm_checks.check without its condition on the inputs (UNRESOLVED_CAP: "choose other inputs"): the resolved elements to the bit,
        # every element within the bound + the bf16 rounding
        res, _, unresolved = sc.bf16_shares(ref, tol)
        if bool(res.any()):
            kc.assert_bf16_of(out[res].reshape(1, -1), ref[res].reshape(1, -1), tol[res].reshape(1, -1), what)
        return {key: E(out, ref, tol * (1 + kc.U8) + kc.U8 * ref.abs() + 2.0 ** -133, what + " (bf16 rounding allowed)"), key + ", unresolved" + SHARE: unresolved}
    if nm == "gemm_bf16":
        assert a("step_ptr") is None, "%s: a step-indexed gate on an inference tape" % what
        x, epi = a("x"), a("epilogue")
        N = a("n") if a("n") is not None else a("w").shape[0]
        w, bias = a("w")[:N], None if a("bias") is None else a("bias")[:N]
        out = call.result()
        M = x.shape[0]
        resid = gate = None
        if epi == L.EPI_RESID_F32:
            ro, rr = call.inplace.get("out", {}).get("before"), call.args.get("resid")
            aliased = rr is None or (ro is not None and (rr.storage, rr.offset, rr.shape, rr.stride) == (ro.storage, ro.offset, ro.shape, ro.stride))
            assert ro is not None or rr is not None, "%s: a residual epilogue without a residual" % what
            resid = call.before("out") if aliased else a("resid")
            g = sample_rows_of(call, "gate", "gate_sample_stride")
            gate = None if g is None else _rows(g[:, :N], M, a("rows_per_sample"), call, "gate")
        ref, tol = gemm_reference(x, w, bias, epi, resid, a("skip"), gate)
        names = {L.EPI_F32: "fp32", L.EPI_BF16: "bf16", L.EPI_GELU_BF16: "gelu bf16", L.EPI_RELU_BF16: "relu bf16", L.EPI_RESID_F32: "resid fp32"}
        return {"gemm_bf16 %s%s" % (names[epi], " gated" if gate is not None else ""): E(out, ref, tol, what)}
    if nm == "layernorm_modulate":
        assert a("step_ptr") is None
        x = a("x")
        kw = dict(ln_w=a("w"), ln_b=a("b"))
        if a("shift") is not None:
            kw.update(shift=sample_rows_of(call, "shift", "mod_sample_stride"), scale=sample_rows_of(call, "scale", "mod_sample_stride"),
                      rows_per_sample=a("rows_per_sample") or x.shape[0])
            _rows(kw["shift"], x.shape[0], kw["rows_per_sample"], call, "shift")
        pre, al, _, _ = kc.ln_stage(x, **kw)                              # (LN_ALLOW is test_layernorm_modulate_and_cast_pad_guard_bands's 4 x 2^-20)
        return {nm: E(call.result(), pre, al + kc.U8 * pre.abs() * (1 + kc.U8), what)}
    if nm == "group_stats":
        x = a("x")
        ref, tol = kc.group_stats_ref(x, a("B"), a("T"), x.shape[1], a("groups"), a("eps"))
        return {nm: E(call.out(), ref, tol, what)}
    if nm == "norm_apply":
        x = a("x")
        kw = dict(w=a("w"), b=a("b"))
        if a("shift") is not None:
            kw.update(shift=sample_rows_of(call, "shift", "mod_sample_stride"), scale=sample_rows_of(call, "scale", "mod_sample_stride"),
                      rows_per_sample=a("rows_per_sample"))
            _rows(kw["shift"], x.shape[0], kw["rows_per_sample"], call, "shift")
        pre, acc = kc.norm_apply_ref(x, a("stats"), a("rows_per_stat"), **kw)
        return {nm + ", ambiguous" + SHARE: kc.assert_bf16_of(call.result(), pre, acc, what), nm: 0.0}
    if nm == "block_activation_":
        kind = {v: k for k, v in kc.BLOCK_ACT_KINDS.items()}[a("kind")]
        ratio, share = kc.check_block_act(call.after("x"), call.before("x"), kind, what)
        return {"%s %s" % (nm, kind): ratio, "%s %s, ambiguous%s" % (nm, kind, SHARE): share}
    if nm == "ln_linear":
        x = a("x")
        sr = kc.ln_linear_reference(x, a("w").float(), a("bias"), **_ln_kw(call, M=x.shape[0]))
        kc.assert_interval(call.result(), sr["lo"], sr["hi"], what)
        return {nm: 0.0, nm + ", off the point reference" + SHARE: float((call.result().double() != sr["ref"]).double().mean()), nm + ", pinned" + SHARE: sr["pinned"]}
    if nm == "ln_mlp_resid_":
        x0, x1 = call.before("x"), call.after("x")
        M, C = x0.shape
        kw = _ln_kw(call, M=M)
        g = sample_rows_of(call, "gate", "mod_sample_stride")
        if g is not None:
            kw.update(gate=g, rows_per_sample=a("rows_per_sample") or M)
            _rows(g, M, kw["rows_per_sample"], call, "gate")
        sr = kc.fused_mlp_reference(x0, a("w_up").float(), a("b_up"), a("w_dn").float(), a("b_dn"), **kw)
        r = {nm: E(x1, sr["ref"], sr["tol"], what + ", x"), nm + ", median(tol) / median(|update|)" + SHARE: sr["ratio"]}
        if "x_bf16_out" in call.inplace:
            im0, im1 = call.before("x_bf16_out"), call.after("x_bf16_out")
            assert torch.equal(im1[:, :C], x1.bfloat16()), "%s: the bf16 image `x_bf16_out` is not bf16 of the x this call left behind" % what
            assert torch.equal(tt._bits(im1[:, C:]), tt._bits(im0[:, C:])), "%s: columns of `x_bf16_out` beyond C were written" % what
            r[nm + " bf16 image"] = 0.0
        nx = call.args.get("next_linear")
        if nx is not None:
            assert len(call.outs) == 2 and call.outs[1] is not None, "%s: `next_linear` given and no projection returned" % what
            assert nx.get("out") is None, "%s: a `next_linear` destination of the caller's (unaudited)" % what
            bias = nx["bias"].value if isinstance(nx.get("bias"), tt.Rec) else None
            nr = kc.ln_linear_reference(x1, nx["w"].value.float(), bias, **_ln_kw(call, nx, M))
            kc.assert_interval(call.out(1), nr["lo"], nr["hi"], what + ": q_next against LN + linear of the x this call left behind")
            r[nm + " q_next"] = 0.0
            r[nm + " q_next, pinned" + SHARE] = nr["pinned"]
        else:
            assert len(call.outs) == 1, "%s: a projection returned without `next_linear`" % what
        return r
    if nm == "attention_fwd":
        B, H, Nq, Nk, dh = a("B"), a("H"), a("Nq"), a("Nk"), a("head_dim")
        C = H * dh
        ref, vmax = kc.attention_ref64(a("q")[:, :C], a("k")[:, :C], a("v")[:, :C], B, H, Nq, Nk, dh)
        return {"%s dh %d" % (nm, dh): E(call.result().reshape(-1, dh), ref.reshape(-1, dh), kc.attention_base_tol(ref, vmax).reshape(-1, dh), what)}
    if nm == "attention_oproj_resid_":
        B, H, Nq, Nk = a("B"), a("H"), a("Nq"), a("Nk")
        assert a("head_dim") == 32, "%s: head_dim %r" % (what, a("head_dim"))
        C = H * 32
        x0 = call.inplace["x"]["before"].value
        g = sample_rows_of(call, "gate", "gate_sample_stride")
        gate = None if g is None else _rows(g, B * Nq, Nq, call, "gate")
        ref, tol = oproj_reference(a("q")[:, :C], a("k")[:, :C], a("v")[:, :C], B, H, Nq, Nk, a("wo"), a("bo"), x0, gate)
        return {nm + (" gated" if gate is not None else ""): E(call.inplace["x"]["after"].value, ref, tol, what)}
    if nm == "actnorm_":
        B = a("B")
        x0 = call.before("x")
        assert x0.numel() == B * a("shift").numel() == B * a("log_scale").numel(), "%s: %d values in %d samples, and %d parameters" % (what, x0.numel(), B, a("shift").numel())
        ref, tol = kc.actnorm_ref(x0.reshape(B, -1), a("shift").reshape(-1), a("log_scale").reshape(-1))
        return {nm: E(call.after("x").reshape(B, -1), ref, tol, what)}
    if nm == "maxpool":
        assert torch.equal(call.out(), kc.maxpool_expr(a("x"), a("G"), a("n"))), "%s: not the maximum over each group's rows" % what
        return {nm: 0.0}
    if nm == "fps":
        from oracle import ldt_oracle as O
        from ldt_amd import ops
        skip = ops.FPS_SKIP_NEAR_ORIGIN if a("skip_near_origin") is None else bool(a("skip_near_origin"))
        want = O.fps(a("xyz").cpu(), a("m"), skip_near_origin=skip)
        assert call.out().dtype == torch.int32 and torch.equal(call.out().cpu().long(), want), "%s: not the farthest-point sequence" % what
        return {nm: 0.0}
    if nm == "knn":
        assert not a("return_dist")
        return {nm: 0.0, nm + ", sets that differ from topk's" + SHARE: knn_check(call.out(), a("xyz"), a("centers"), a("k"), what)}
    if nm == "gather_rows":
        src, idx = a("src"), a("idx").long()
        assert torch.equal(call.out(), torch.gather(src, 1, idx[:, :, None].expand(-1, -1, src.shape[2]))), "%s: not the indexed rows" % what
        return {nm: 0.0}
    if nm == "norm_points":
        ref, tol = kc.norm_points_ref(a("xyz"))
        return {nm: E(call.out(), ref, tol, what)}
    if nm == "group_normalize":
        assert not a("return_stats")
        D = a("feat").shape[2]
        ref = kc.group_reference(a("feat"), a("xyz"), a("fps_idx"), a("knn_idx"), a("alpha"), a("beta"), a("normalize"))
        U = call.out()
        k, S = a("knn_idx").shape[2], a("knn_idx").shape[1]
        lo, hi = kc.bf16_round(ref["pre"] - ref["a"]).reshape(-1, D + 3), kc.bf16_round(ref["pre"] + ref["a"]).reshape(-1, D + 3)
        kc.assert_interval(U[:, :D + 3], lo, hi, what + ": normalised columns", k=k, S=S)
        want = ref["anchor"].float().bfloat16()[:, :, None, :].expand(-1, -1, k, -1).reshape(-1, D).to(U.device)
        assert torch.equal(U[:, D + 3:2 * D + 3], want), what + ": anchor columns differ from bf16(feat[anchor])"
        assert bool((U[:, 2 * D + 3:].float() == 0).all()), what + ": K padding not zero"
        return {nm: 0.0, nm + ", pinned" + SHARE: float((lo == hi).double().mean())}
    if nm == "grouper_mlp":
        hit = [p for p in (ctx or {}).get("grouper", []) if _eq(a("wimg"), p[0])]
        assert hit, "%s: `wimg` is the fragment image of no panel set the audit was given" % what
        _, w1, b1, w2, b2, w3, b3 = hit[0]
        for got, want, n in ((a("b1"), b1, "b1"), (a("b2"), b2, "b2"), (a("b3"), b3, "b3")):
            assert _eqflat(got, want), "%s: `%s` is not the bias of the image's panel" % (what, n)
        g = kc.group_reference(a("feat"), a("xyz"), a("fps_idx"), a("knn_idx"), a("alpha"), a("beta"))
        sr = kc.grouper_staged_reference(g, w1, b1, w2, b2, w3, b3)
        kc.assert_interval(call.result(), sr["lo"], sr["hi"], what, k=sr["k"], S=sr["S"], slot=sr["slot"])
        return {nm: 0.0, nm + ", pinned" + SHARE: sr["pinned"]}
    if nm == "mixture_seed":
        ref, tol = kc.mixture_seed_ref(a("eps"), a("sig"), a("mu"), a("logits"))
        return {nm: E(call.out(), ref, tol, what)}
    if nm in ("reparam", "reparam_kl"):
        post = a("post")
        noise = a("noise").reshape(post.shape[0], -1)
        mu, lv, ref, tol = kc.reparam_ref(post, noise, a("lo"), a("hi"))
        eps = call.after("out")
        r = {nm + " eps": E(eps, ref, tol, what + ", eps")}
        if a("want_stats"):
            assert torch.equal(call.out(0), mu) and torch.equal(call.out(1), lv), "%s: mu / logvar are not the selections of `post`" % what
        else:
            assert call.outs[0] is None and call.outs[1] is None
        if nm == "reparam_kl":
            lq64, tol_q, kl64, tol_k = kc.reparam_kl_ref(eps, mu, lv)
            r[nm + " logqz"] = E(call.out(3), lq64, tol_q, what + ", logqz")
            r[nm + " kl"] = E(call.out(2), kl64, tol_k, what + ", kl")
            rps = a("rows_per_sample")
            want = call.out(2).double().reshape(-1, rps * eps.shape[1]).sum(1)          # another order of the kernel's own terms: 1e-6 relative,
            err = float((call.out(4).double() - want).abs().max() / want.abs().max())    # test_gpu_eval_kernels_exact's bound on the sample sums
            assert err <= 1e-6, "%s: kl_sample_sum is off the sum of its own kl by %.3g relative" % (what, err)
            r[nm + " sample sums"] = err / 1e-6
        return r
    if nm == "philox_normal":
        out = call.out()
        assert out.numel() % 4 == 0 and a("elem_offset") % 4 == 0, "%s: not whole Philox vectors" % what
        ref, tol = kc.philox_normal_ref(a("seed"), a("step"), a("elem_offset") // 4, out.numel() // 4)
        return {nm: E(out.reshape(-1, 4).cpu(), ref, tol, what)}
    if nm == "add_f32":
        assert torch.equal(call.result(), a("a") + a("b")), "%s: not the fp32 sum of the recorded operands" % what
        return {nm: 0.0}
    if nm == "cast_pad_bf16":
        return tt.check_call(call)
    raise AssertionError("%s: a call kind the audit has no reference for" % call)


def audit_numeric(calls, ctx=None, worst=None):
    """Every call of `calls`: check_untouched + check_call.  -> {call kind: largest err / bound (or share)}."""
    worst = {} if worst is None else worst
    for call in calls:
        tt.check_untouched(call)
        for k, r in check_call(call, ctx).items():
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


def ratios(worst):
    return {k: v for k, v in worst.items() if not k.endswith(SHARE)}


def grouper_ctx(model):
    """The panels behind every fragment image of `model.packed()`, for check_call."""
    P = model.packed()
    out = []
    for key in ("group", "pre_group"):
        G = P.get(key)
        if G is not None and "wimg" in G:
            D = model.hidden_dim
            out.append((G["wimg"], G["w_pre1"][:, :2 * D + 3].float(), G["b_pre1"], G["w_pre2"][:, :D].float(), G["b_pre2"], G["w_pre3"][:, :D].float(), G["b_pre3"]))
    return {"grouper": out}


# ------------------------------------------------------------------------------------------------------------- wiring audit
def _lay(r):
    return (r.storage, r.offset, r.shape, r.stride)


class Stream:
    """A tensor the forward updates in place: its value now, and the view it lives in once a call has written it."""

    def __init__(self, label, value, rec=None):
        self.label, self.value, self.lay = label, value, None if rec is None else _lay(rec)


class Table(tt.Wiring):
    """train_tape.Wiring plus what the inference tables share."""

    def __init__(self, calls, model, B):
        super().__init__(calls)
        L = _lib()
        self.L, self.m, self.P, self.B = L, model, model.packed(), B
        assert not model.pre_group and "w_pm1" not in self.P, "wiring: pre_group / pos_embedding: mlp are outside this table"

    def find(self, kind, pred, what):
        fresh = [c for c in self.calls if c.name == kind and c.index not in self.seen and pred(c)]
        if fresh:
            self.seen.add(fresh[0].index)
            return fresh[0]
        return super().find(kind, pred, what)

    def maybe(self, kind, pred):
        hits = [c for c in self.calls if c.name == kind and c.index not in self.seen and pred(c)]
        if hits:
            self.seen.add(hits[0].index)
            return hits[0]
        return None

    def none(self, call, arg, what):
        assert call.args.get(arg) is None, "wiring: %s: operand `%s` must be None (%s)" % (call, arg, what)

    def on_stream(self, call, arg, X, what):
        """The in-place operand `arg` of `call` is the stream X: its view (once known) and its value so far."""
        d = call.inplace.get(arg)
        assert d is not None, "wiring: %s: `%s` must be updated in place (%s)" % (call, arg, what)
        if X.lay is not None and _lay(d["before"]) != X.lay:
            raise AssertionError("wiring: %s: `%s` must be the view %s lives in (storage offset %d, shape %s, strides %s), not offset %d, shape %s, strides %s" % (
                call, arg, X.label, X.lay[1], list(X.lay[2]), list(X.lay[3]), d["before"].offset, list(d["before"].shape), list(d["before"].stride)))
        if not _eq(d["before"].value, X.value):
            raise AssertionError("wiring: %s: `%s` must come in as %s; %s" % (call, arg, X.label, self.identify(d["before"].value)))
        X.lay = _lay(d["before"])

    def writes(self, kind, arg, X, extra=lambda c: True):
        """The unclaimed call of `kind` whose in-place operand `arg` comes in bit-equal to the stream X (and in its view, once known)."""
        def pred(c):
            d = c.inplace.get(arg)
            return d is not None and _eq(d["before"].value, X.value) and (X.lay is None or _lay(d["before"]) == X.lay) and extra(c)
        return self.maybe(kind, pred)

    def column(self, call, arg, rows, k, width, what, stride_arg=None, src=None):
        """Operand `arg` is columns [k width, (k + 1) width) of `rows` (a recorded output): the values, the storage, the offset, the strides,
        and (stride_arg) the sample stride the kernel is told = the row stride of `rows`."""
        A = call.args if src is None else src
        r, n = A.get(arg), rows.shape[1]
        desc = "columns [%d C, %d C) of %s" % (k, k + 1, what)
        assert isinstance(r, tt.Rec), "wiring: %s: operand `%s` must be %s; it is %r" % (call, arg, desc, r)
        want = rows.value[:, k * width:(k + 1) * width]
        if not _eq(r.value, want):
            raise AssertionError("wiring: %s: operand `%s` must be %s; %s" % (call, arg, desc, self.identify(r.value)))
        if (r.storage, r.offset, r.stride) != (rows.storage, rows.offset + k * width, (n, 1)):
            raise AssertionError("wiring: %s: operand `%s` must be the view of %s itself (storage offset %d, strides %s), not offset %d, strides %s" % (
                call, arg, desc, rows.offset + k * width, [n, 1], r.offset, list(r.stride)))
        if stride_arg is not None and A.get(stride_arg) != n:
            raise AssertionError("wiring: %s: operand `%s` must be %d, the row stride of %s; it is %r" % (call, stride_arg, n, what, A.get(stride_arg)))

    # ---- the pieces of a ResidualBlock (layers.py:183-229) and of a FinalLayer (:240-246)
    def mod_rows(self, c, w, b, n, what):
        sg = self.find("sgemm", lambda k: _eq(k.arg("w"), w) and _eq(k.arg("a"), c), "forms adaLN(SiLU(c)) of %s from the condition" % what)
        self.link(sg, "bias", b, "the adaLN bias of %s" % what)
        self.link(sg, "act_in", self.L.ACT_SILU, "SiLU on the condition")
        self.link(sg, "act_out", self.L.ACT_NONE, "no activation behind adaLN")
        rows = sg.outs[0]
        assert rows.shape == (c.shape[0], n), "wiring: %s: the modulation rows must be [%d, %d]" % (sg, c.shape[0], n)
        return rows

    def norm_kw(self, call, names, affine, mod, k, C, rps, what, src=None):
        """The norm arguments of one call: (affine w, b | None) and (shift, scale = columns k, k + 1 of the modulation rows | None)."""
        A = call.args if src is None else src
        wn, bn, stride_arg = names
        for arg, p in ((wn, affine[0]), (bn, affine[1])):
            if p is None:
                assert A.get(arg) is None, "wiring: %s: operand `%s` must be None (%s has no affine)" % (call, arg, what)
            else:
                got = A.get(arg)
                if not (isinstance(got, tt.Rec) and _eqflat(got.value, p)):
                    raise AssertionError("wiring: %s: operand `%s` must be the affine of %s; %s" % (call, arg, what, self.identify(got.value) if isinstance(got, tt.Rec) else "it is %r" % (got,)))
        if mod is None:
            assert A.get("shift") is None and A.get("scale") is None, "wiring: %s: %s is not modulated" % (call, what)
            return
        self.column(call, "shift", mod, k, C, "the modulation rows: the shift of %s" % what, stride_arg, src)
        self.column(call, "scale", mod, k + 1, C, "the modulation rows: the scale of %s" % what, stride_arg, src)
        if A.get("rows_per_sample") != rps:
            raise AssertionError("wiring: %s: operand `rows_per_sample` must be %d, the rows one modulation row is broadcast over (%s); it is %r" % (call, rps, what, A.get("rows_per_sample")))

    def norm_chain(self, x, Pn, i, mod, k, C, B, N, act, what):
        """norm(x) [affine] [modulated] [activation] by the norm kernels -> the bf16 rows, or None where no such chain reads x."""
        kind, affine = Pn["kind"], Pn["affine"][i]
        if kind == "layer_norm":
            c = self.maybe("layernorm_modulate", lambda c: _eq(c.arg("x"), x))
            if c is None:
                return None
            self.norm_kw(c, ("w", "b", "mod_sample_stride"), affine if mod is None else (None, None), mod, k, C, N, what)
            self.none(c, "step_ptr", "no step index at inference")
        else:
            c = self.maybe("norm_apply", lambda c: _eq(c.arg("x"), x))
            if c is None:
                return None
            if kind == "group_norm":
                gs = self.find("group_stats", lambda g: _eq(g.arg("x"), x), "forms the group statistics of %s" % what)
                for arg, v in (("B", B), ("T", N), ("groups", Pn["groups"][i])):
                    self.link(gs, arg, v, "%s = %d" % (arg, v))
                self.link(gs, "eps", 1e-6, "GroupNorm's eps 1e-6")
                self.link(c, "stats", gs.out(), "the group statistics of %s" % what)
                self.link(c, "rows_per_stat", N, "N = %d rows per sample" % N)
            else:
                self.none(c, "stats", "the identity norm")
            self.norm_kw(c, ("w", "b", "mod_sample_stride"), affine if kind == "group_norm" else (None, None), mod, k, C, N, what)
        h = c.result()
        if act:
            ba = self.find("block_activation_", lambda b: _eq(b.before("x"), h), "applies the block activation behind %s" % what)
            self.link(ba, "kind", act, "the block's activation id %d" % act)
            h = ba.after("x")
        return self.name("norm + modulate of %s" % what, h)

    def gate(self, call, mod, k, C, rps, what, stride_arg, rps_arg=None):
        if mod is None:
            self.none(call, "gate", "%s has no gate" % what)
            return
        if rps_arg is not None and call.arg(rps_arg) != rps:
            raise AssertionError("wiring: %s: operand `%s` must be %d, the rows one gate row is broadcast over (%s); it is %r" % (call, rps_arg, rps, what, call.arg(rps_arg)))
        self.column(call, "gate", mod, k, C, "the modulation rows: the gate of %s" % what, stride_arg)

    def block(self, Pb, Pn, what, X, B, Nq, kv, Nk, c=None, hand=None, q_pre=None, image=None):
        """x = x + g1 fc_o(Attn(fc_q(n1(x)), K | V)); x = x + g2 mlp(n2(x)) on the stream X, K | V = `kv` (a recorded output, found by the caller).
        hand: (panels, norms) of the block whose LN1 + fc_q this block's last kernel may compute; q_pre: what the previous block handed over;
        image: True where the block must leave bf16(x) for a later reader.  -> dict(q_next, image)"""
        L, C, H = self.L, Pb["Co"], Pb["H"]
        assert Pb["C"] == C
        mod = self.mod_rows(c, Pb["wada"], Pb["bada"], 6 * C, what) if c is not None else None
        act = 0 if c is not None else Pb.get("act", 0)
        # ---- attention + out-projection + gated residual (layers.py:183-200, 218 / 225)
        fused = self.writes("attention_oproj_resid_", "x", X)
        if fused is not None:
            at = fused
            self.link(at, "wo", Pb["wo"], "the bf16 panel of fc_o of %s" % what)
            self.link(at, "bo", Pb["bo"], "the bias of fc_o of %s" % what)
            self.gate(at, mod, 2, C, Nq, "the attention branch of %s" % what, "gate_sample_stride")
            x_after = at.after("x")
            self.on_stream(at, "x", X, "the attention branch of %s" % what)
        else:
            rg = self.writes("gemm_bf16", "out", X, lambda k: _eq(k.arg("w"), Pb["wo"]))
            assert rg is not None, "wiring: no attention_oproj_resid_ and no residual gemm_bf16 through fc_o updates %s in place (%s)" % (X.label, what)
            self.on_stream(rg, "out", X, "the attention branch of %s" % what)
            self.link(rg, "epilogue", L.EPI_RESID_F32, "the residual epilogue")
            self.link(rg, "bias", Pb["bo"], "the bias of fc_o of %s" % what)
            assert rg.args.get("resid") is None or _lay(rg.args["resid"]) == _lay(rg.inplace["out"]["before"]), "wiring: %s: `resid` must be `out` itself (x = x + ...)" % rg
            self.gate(rg, mod, 2, C, Nq, "the attention branch of %s" % what, "gate_sample_stride", "rows_per_sample")
            at = self.find("attention_fwd", lambda k: _eqflat(k.result(), rg.arg("x")), "produces the [B][H][Nq][Dh] buffer fc_o of %s reads raw as (B Nq, C) rows (quirk Q1)" % what)
            self.link(at, "head_dim", C // H, "C / H")
            x_after = rg.after("out")
        for arg, v in (("B", B), ("H", H), ("Nq", Nq), ("Nk", Nk)):
            self.link(at, arg, v, "%s = %d" % (arg, v))
        # K | V: the two halves of `kv`, as views of it
        self.column(at, "k", kv, 0, C, "K | V of %s: K" % what)
        self.column(at, "v", kv, 1, C, "K | V of %s: V" % what)
        # q = fc_q(n1(x)): the previous block's hand-off, LN + linear in one kernel, or the norm chain and a GEMM
        q = at.arg("q")
        n1 = ("ln_w", "ln_b", "mod_sample_stride")
        if q_pre is not None and _eq(q, q_pre):
            pass                                                            # (held at its producer: panels, and numerically from the x it left)
        else:
            ll = self.maybe("ln_linear", lambda k: _eq(k.result(), q) and _eq(k.arg("x"), X.value))
            if ll is not None:
                self.link(ll, "w", Pb["wq"], "the bf16 panel of fc_q of %s" % what)
                self.link(ll, "bias", Pb["bq"], "the bias of fc_q of %s" % what)
                self.norm_kw(ll, n1, Pn["affine"][0] if mod is None else (None, None), mod, 0, C, Nq, "norm1 of %s" % what)
            else:
                h = self.norm_chain(X.value, Pn, 0, mod, 0, C, B, Nq, act, "norm1 of %s" % what)
                if h is None:
                    raise AssertionError("wiring: %s: operand `q` must be fc_q(norm1(x)) of %s at its entry: no ln_linear, norm chain or hand-off produces it; %s" % (at, what, self.identify(q)))
                gq = self.find("gemm_bf16", lambda k: _eq(k.arg("x"), h) and _eq(k.arg("w"), Pb["wq"]), "projects norm1 of %s through fc_q" % what)
                self.link(gq, "bias", Pb["bq"], "the bias of fc_q of %s" % what)
                self.link(gq, "epilogue", L.EPI_BF16, "the plain bf16 epilogue")
                self.link(at, "q", gq.result(), "fc_q(norm1(x)) of %s" % what)
        X.value = self.name("%s after the attention branch of %s" % (X.label, what), x_after)
        # ---- MLP + gated residual (layers.py:219 / 226)
        res = dict(q_next=None, image=None, imaged=False)
        mk = self.writes("ln_mlp_resid_", "x", X)
        if mk is not None:
            self.on_stream(mk, "x", X, "the MLP branch of %s" % what)
            for arg, key in (("w_up", "wup"), ("b_up", "bup"), ("w_dn", "wdn"), ("b_dn", "bdn")):
                self.link(mk, arg, Pb[key], "%s of the MLP of %s" % (key, what))
            self.norm_kw(mk, n1, Pn["affine"][1] if mod is None else (None, None), mod, 3, C, Nq, "norm2 of %s" % what)
            self.gate(mk, mod, 5, C, Nq, "the MLP branch of %s" % what, "mod_sample_stride")
            x_after = mk.after("x")
            if "x_bf16_out" in mk.inplace:
                res["image"], res["imaged"] = mk.inplace["x_bf16_out"]["after"], True
            nx = mk.args.get("next_linear")
            if nx is not None:
                assert hand is not None, "wiring: %s: a `next_linear` where no block follows on these rows (%s)" % (mk, what)
                hp, hn = hand
                for arg, want, w2 in (("w", hp["wq"], "the bf16 panel of fc_q"), ("bias", hp["bq"], "the bias of fc_q")):
                    got = nx.get(arg)
                    if not (isinstance(got, tt.Rec) and _eq(got.value, want)):
                        raise AssertionError("wiring: %s: `next_linear` %s must be %s of the NEXT block on these rows" % (mk, arg, w2))
                self.norm_kw(mk, n1, hn["affine"][0], None, 0, C, Nq, "norm1 of the next block", src=nx)
                res["q_next"] = self.name("q_next of %s" % what, mk.out(1))
        else:
            h2 = self.norm_chain(X.value, Pn, 1, mod, 3, C, B, Nq, act, "norm2 of %s" % what)
            assert h2 is not None, "wiring: no ln_mlp_resid_ and no norm chain reads %s (%s)" % (X.label, what)
            up = self.find("gemm_bf16", lambda k: _eq(k.arg("x"), h2) and _eq(k.arg("w"), Pb["wup"]), "projects norm2 of %s up" % what)
            self.link(up, "bias", Pb["bup"], "the bias of mlp.fc of %s" % what)
            self.link(up, "epilogue", L.EPI_GELU_BF16, "the GELU epilogue")
            dn = self.writes("gemm_bf16", "out", X, lambda k: _eq(k.arg("w"), Pb["wdn"]))
            assert dn is not None, "wiring: no residual gemm_bf16 through mlp.out updates %s in place (%s)" % (X.label, what)
            self.on_stream(dn, "out", X, "the MLP branch of %s" % what)
            self.link(dn, "x", up.result(), "GELU(mlp.fc(norm2(x))) of %s" % what)
            self.link(dn, "epilogue", L.EPI_RESID_F32, "the residual epilogue")
            self.link(dn, "bias", Pb["bdn"], "the bias of mlp.out of %s" % what)
            assert dn.args.get("resid") is None or _lay(dn.args["resid"]) == _lay(dn.inplace["out"]["before"]), "wiring: %s: `resid` must be `out` itself (x = x + ...)" % dn
            self.gate(dn, mod, 5, C, Nq, "the MLP branch of %s" % what, "gate_sample_stride", "rows_per_sample")
            x_after = dn.after("out")
        X.value = self.name("%s after %s" % (X.label, what), x_after)
        if image and res["image"] is None:                                  # the chain's image: one cast of the finished x
            cp = self.maybe("cast_pad_bf16", lambda k: _eq(k.arg("src"), X.value))
            res["imaged"] = cp is not None                                   # (torch copies it into the caller's buffer: held at its reader)
        return res

    def kv_of(self, y, Pb, what, why):
        """K | V = fc_kv(y) of a block whose K / V source is the RAW tensor y (quirk Q2) -> the recorded output."""
        g = self.find("gemm_bf16", lambda k: _eq(k.arg("w"), Pb["wkv"]) and _eq(k.arg("x"), y), "projects %s through fc_kv of %s" % (why, what))
        self.link(g, "bias", Pb["bkv"], "the bias of fc_kv of %s" % what)
        self.link(g, "epilogue", self.L.EPI_BF16, "the plain bf16 epilogue")
        assert "out" not in g.inplace
        return g.outs[0]

    def cast_of(self, X, width, what):
        """The bf16 cast of the stream X as it stands now (a K / V source) -> the recorded output."""
        want = kc.cast_pad_want(X.value, width)
        cp = self.find("cast_pad_bf16", lambda k: _eq(k.arg("src"), X.value) and _eq(k.result(), want), "casts %s, as it stands at the entry of %s, to its bf16 K / V source" % (X.label, what))
        return cp.result()

    def norms(self, blk):
        return dict(kind=getattr(blk.norm1, "kind", "layer_norm"), groups=(getattr(blk.norm1, "num_groups", 0), getattr(blk.norm2, "num_groups", 0)),
                    affine=[tuple(None if p is None else p.detach().float() for p in n.affine) for n in (blk.norm1, blk.norm2)])

    def initial_set(self, npts, keep_mask, seed_eps):
        """InitialSet.forward (Compressor/layers.py:26-42) -> the stream o."""
        m, P, B = self.m, self.P, self.B
        if m.max_outputs is None:
            M = P["mix"]
            if seed_eps is None:
                ph = self.find("philox_normal", lambda k: tuple(k.arg("shape")) == (B, npts, m.init_set.n_mixtures, m.hidden_dim), "draws the mixture's N(0, 1) rows")
                seed_eps = ph.out()
            ms = self.find("mixture_seed", lambda k: True, "forms the mixture rows")
            self.link(ms, "eps", seed_eps.float().reshape(B * npts, m.init_set.n_mixtures, m.hidden_dim), "the N(0, 1) draws of the seed rows")
            for arg in ("sig", "mu", "logits"):
                self.link(ms, arg, M[arg], "the parameter %s" % arg)
            s1 = self.find("sgemm", lambda k: _eq(k.arg("a"), ms.out()) and _eq(k.arg("w"), M["w1"]), "carries the mixture rows through output.0")
            self.link(s1, "bias", M["b1"], "output.0.bias"); self.link(s1, "act_out", self.L.ACT_SILU, "SiLU"); self.link(s1, "act_in", 0, "no activation in front")
            s2 = self.find("sgemm", lambda k: _eq(k.arg("a"), s1.result()) and _eq(k.arg("w"), M["w2"]), "carries them through output.2")
            self.link(s2, "bias", M["b2"], "output.2.bias"); self.link(s2, "act_out", 0, "no activation"); self.link(s2, "act_in", 0, "no activation")
            return Stream("the set stream o", self.name("the initial set", s2.result()), s2.outs[0])
        prior = P["prior"]
        if keep_mask is None:
            assert npts == m.max_outputs, "wiring: %d of %d prior rows and no keep mask" % (npts, m.max_outputs)
            o = prior.unsqueeze(0).expand(B, -1, -1).reshape(B * npts, -1)
        else:
            km = keep_mask.to(prior.device)
            o = torch.stack([prior[km[b]] for b in range(B)], 0).reshape(B * npts, -1)
        return Stream("the set stream o", self.name("the initial set (each sample's kept prior rows, in index order)", o.contiguous()))

    def decoder_level(self, j, o, eps_rec, eps_what, npts, T, q_pre, want_image):
        """DecoderBlock.forward (Network.py:80-83): o <- att1(o, ln(eps_j)), top-down (reversed(self.decoder), :217 / :263)."""
        m, P = self.m, self.P
        Ld = m.n_layers
        d, Pd = m.decoder[Ld - 1 - j], P["dec"][Ld - 1 - j]
        what = "decoder level %d (decoder.%d.att1)" % (j, Ld - 1 - j)
        sg = self.find("sgemm", lambda k: _eq(k.arg("w"), Pd["w_zkv"]), "forms K | V = fc_kv(ln(eps_%d)) of %s" % (j, what))
        got = sg.args["a"]
        if not _eq(got.value, eps_rec["value"]):
            raise AssertionError("wiring: %s: operand `a` must be %s; %s" % (sg, eps_what, self.identify(got.value)))
        if eps_rec.get("lay") is not None and (got.storage, got.offset, got.stride) != (eps_rec["lay"][0], eps_rec["lay"][1], eps_rec["lay"][3]):
            raise AssertionError("wiring: %s: operand `a` must be the view of %s itself (storage offset %d), not offset %d" % (sg, eps_what, eps_rec["lay"][1], got.offset))
        self.link(sg, "bias", Pd["b_zkv"], "fc_kv(ln.bias) + fc_kv.bias of %s" % what)
        self.link(sg, "act_in", 0, "no activation"); self.link(sg, "act_out", 0, "no activation")
        assert sg.result().dtype == torch.bfloat16, "wiring: %s: K | V must be bf16" % sg
        nxt = None
        if j + 1 < Ld:
            nxt = (P["dec"][Ld - 2 - j]["att1"], self.norms(m.decoder[Ld - 2 - j].att1))
        return self.block(Pd["att1"], self.norms(d.att1), what, o, self.B, npts, sg.outs[0], T, hand=nxt, q_pre=q_pre, image=want_image)

    def output_conv(self, o, got, npts):
        sg = self.find("sgemm", lambda k: _eq(k.arg("w"), self.P["w_out"]), "is the output conv (Network.py:231 / 266)")
        self.link(sg, "a", o.value, "the set stream after the last decoder level")
        self.link(sg, "bias", self.P["b_out"], "output.bias"); self.link(sg, "act_in", 0, "no activation"); self.link(sg, "act_out", 0, "no activation")
        if not _eqflat(got, sg.result()):
            raise AssertionError("wiring: the returned set is not what %s left; %s" % (sg, self.identify(got)))

    def finish(self):
        stray = [c for c in self.calls if c.index not in self.seen]
        assert not stray, "wiring: calls the table has no place for: %s" % ", ".join(str(c) for c in stray[:4])
        return len(self.seen)


def audit_forward(calls, model, x, res, post_noise=None, seed_eps=None, keep_mask=None, want_kl=False, num_points=None):
    """Compressor.forward (Network.py:188-249).  calls: the forward's; x: its input; res: what it returned; post_noise / seed_eps: what it was
    given (None: drawn on the device, then held at the Philox call); keep_mask: the InitialSet rows the forward drew, where it keeps a subset."""
    m = model
    B, N, _ = x.shape
    W = Table(calls, m, B)
    P, L = W.P, W.L
    T, D, z, Ld = m.z_scales, m.hidden_dim, m.z_dim, m.n_layers
    npts = m.outsize if num_points is None else num_points
    assert m.label_dim is None, "wiring: class-conditional forwards are outside this table"
    # ---- bottom_up (Network.py:188-206)
    pts = W.name("the input cloud", x.to(P["w_input"].device, torch.float32).contiguous())
    if m.norm_input:                                                        # :189-190
        np_ = W.find("norm_points", lambda k: True, "normalises the input cloud")
        W.link(np_, "xyz", pts, "the input cloud")
        pts = W.name("the normalised cloud", np_.out())
    si = W.find("sgemm", lambda k: _eq(k.arg("w"), P["w_input"]), "is the input conv (:192)")
    W.link(si, "a", pts.reshape(B * N, 3), "the cloud's points"); W.link(si, "bias", P["b_input"], "input.bias")
    W.link(si, "act_in", 0, "no activation"); W.link(si, "act_out", 0, "no activation")
    feat = W.name("the point features", si.result().reshape(B, N, D))
    k = N // T * 2                                                          # :195
    G = P["group"]
    fp = W.find("fps", lambda c: True, "samples the group centres")
    W.link(fp, "xyz", pts, "the cloud"); W.link(fp, "m", T, "z_scales = %d" % T)
    ce = W.find("gather_rows", lambda c: _eq(c.arg("idx"), fp.out()), "gathers the centres")
    W.link(ce, "src", pts, "the cloud")
    centers = W.name("the centres", ce.out())
    kn = W.find("knn", lambda c: True, "finds each centre's neighbours")
    W.link(kn, "xyz", pts, "the cloud"); W.link(kn, "centers", centers, "the centres"); W.link(kn, "k", k, "N / z_scales * 2 = %d" % k)
    gm = W.maybe("grouper_mlp", lambda c: True)
    grouped = lambda c: (W.link(c, "feat", feat, "the point features"), W.link(c, "xyz", pts, "the cloud"), W.link(c, "fps_idx", fp.out(), "the centres' indices"),
                         W.link(c, "knn_idx", kn.out(), "the neighbours' indices"), W.link(c, "alpha", G["alpha"], "affine_alpha"), W.link(c, "beta", G["beta"], "affine_beta"))
    if gm is not None:
        grouped(gm)
        W.link(gm, "wimg", G["wimg"], "the fragment image of the PreExtraction panels")
        for i in (1, 2, 3):
            W.link(gm, "b%d" % i, G["b_pre%d" % i], "the bias of PreExtraction layer %d" % i)
        tok0 = gm.result()
        tok_rec = gm.outs[0]
    else:
        gn = W.find("group_normalize", lambda c: True, "forms the grouped rows")
        grouped(gn)
        W.link(gn, "normalize", G["normalize"], "cluster_norm")
        h1 = W.find("gemm_bf16", lambda c: _eq(c.arg("w"), G["w_pre1"]), "is PreExtraction's transfer layer")
        W.link(h1, "x", gn.out(), "the grouped rows"); W.link(h1, "bias", G["b_pre1"], "its bias"); W.link(h1, "epilogue", L.EPI_RELU_BF16, "ReLU"); W.none(h1, "skip", "no residual")
        r1 = W.find("gemm_bf16", lambda c: _eq(c.arg("w"), G["w_pre2"]), "is the residual layer's net1")
        W.link(r1, "x", h1.result(), "the transfer layer's output"); W.link(r1, "bias", G["b_pre2"], "its bias"); W.link(r1, "epilogue", L.EPI_RELU_BF16, "ReLU"); W.none(r1, "skip", "no residual")
        h2 = W.find("gemm_bf16", lambda c: _eq(c.arg("w"), G["w_pre3"]), "is the residual layer's net2")
        W.link(h2, "x", r1.result(), "net1's output"); W.link(h2, "bias", G["b_pre3"], "its bias"); W.link(h2, "epilogue", L.EPI_RELU_BF16, "ReLU")
        W.link(h2, "skip", h1.result(), "the residual layer's input (act(net2(net1(x)) + x))")
        mp = W.find("maxpool", lambda c: _eq(c.arg("x"), h2.result()), "takes the maximum over each group's neighbours")
        W.link(mp, "G", B * T, "B z_scales groups"); W.link(mp, "n", k, "k = %d neighbours" % k)
        tok0, tok_rec = mp.out(), mp.outs[0]
    c1 = W.find("sgemm", lambda c: _eq(c.arg("w"), P["w_pe1"]), "is the position embedding's conv1 + bn1")
    W.link(c1, "a", centers.reshape(B * T, 3), "the centres"); W.link(c1, "bias", P["b_pe1"], "its folded bias"); W.link(c1, "act_out", L.ACT_RELU, "ReLU"); W.link(c1, "act_in", 0, "none")
    c2 = W.find("sgemm", lambda c: _eq(c.arg("w"), P["w_pe2"]), "is the position embedding's conv2 + bn2")
    W.link(c2, "a", c1.result(), "conv1's output"); W.link(c2, "bias", P["b_pe2"], "its folded bias"); W.link(c2, "act_out", L.ACT_RELU, "ReLU"); W.link(c2, "act_in", 0, "none")
    pm = W.find("maxpool", lambda c: _eq(c.arg("x"), c2.result()), "takes the maximum over each cloud's centres")
    W.link(pm, "G", B, "B clouds"); W.link(pm, "n", T, "z_scales centres")
    pf = W.find("sgemm", lambda c: _eq(c.arg("w"), P["w_pefc"]), "is the position embedding's fc")
    W.link(pf, "a", pm.out(), "the pooled features"); W.link(pf, "bias", P["b_pefc"], "fc.bias"); W.link(pf, "act_out", 0, "none"); W.link(pf, "act_in", 0, "none")
    pos = W.name("the position condition", pf.result())
    tok = Stream("the token stream", W.name("the grouped tokens", tok0), tok_rec)
    if "tokens" in res and res["tokens"] is not None and not _eqflat(res["tokens"], tok0):
        raise AssertionError("wiring: the returned `tokens` are not the grouped tokens before ActNorm; %s" % W.identify(res["tokens"]))
    # ActNorm: once, on the grouped tokens, before the first encoder block (:200-201)
    n_an = sum(c.name == "actnorm_" for c in calls)
    assert n_an == int(m.ActNorm is not None), "wiring: ActNorm must be applied %s before the first encoder block: %d actnorm_ call(s) on the tape" % (
        "exactly once" if m.ActNorm is not None else "never", n_an)
    if m.ActNorm is not None:
        an = W.find("actnorm_", lambda c: True, "applies ActNorm")
        W.on_stream(an, "x", tok, "ActNorm's input is the grouped tokens")
        W.link(an, "shift", P["an_shift"], "conv_in.shift"); W.link(an, "log_scale", P["an_logs"], "conv_in.log_scale")
        W.link(an, "B", B * T * D // P["an_shift"].numel(), "the number of rows the parameters are broadcast over")
        tok.value = W.name("the tokens after ActNorm", an.after("x"))
    enc_out = []
    for i, (enc, Pe) in enumerate(zip(m.encoder, P["enc"])):                # :203-205, 41-45: x = layer(x, x, pos) with the RAW x as K / V source
        for kb, (blk, Pa) in enumerate(zip(enc.atts, Pe["atts"])):
            what = "block %d of encoder stage %d" % (kb, i)
            y = W.cast_of(tok, kc.pad64(D), what)
            kv = W.kv_of(y, Pa, what, "the bf16 cast of the token stream at this block's entry")
            W.block(Pa, W.norms(blk), what, tok, B, T, kv, T, c=pos)
        what = "the FinalLayer of encoder stage %d" % i
        Pf = Pe["out"]
        mod = W.mod_rows(pos, Pf["wada"], Pf["bada"], 2 * D, what)
        fn = dict(kind=getattr(enc.conv_out.norm, "kind", "layer_norm"), groups=(getattr(enc.conv_out.norm, "num_groups", 0),) * 2, affine=[tuple(None if p is None else p.detach().float() for p in enc.conv_out.norm.affine)] * 2)
        h = W.norm_chain(tok.value, fn, 0, mod, 0, D, B, T, 0, what)
        assert h is not None, "wiring: no norm kernel reads the token stream for %s" % what
        fl = W.find("gemm_bf16", lambda c: _eq(c.arg("x"), h) and _eq(c.arg("w"), Pf["w"]), "is conv_out.ln of stage %d" % i)
        W.link(fl, "bias", Pf["b"], "conv_out.ln.bias"); W.link(fl, "epilogue", L.EPI_F32, "the fp32 epilogue"); W.link(fl, "n", Pf["n_out"], "its output width")
        enc_out.append(Stream("the output of encoder stage %d" % i, W.name("the output of encoder stage %d" % i, fl.result()), fl.outs[0]))
    # ---- top_down (:208-233)
    if m.max_outputs is not None and npts != m.max_outputs:
        assert keep_mask is not None, "wiring: the forward kept %d of %d prior rows: the audit needs the mask it drew" % (npts, m.max_outputs)
    o = W.initial_set(npts, keep_mask, seed_eps)
    q_pre, image, imaged, eps_lay0, last = None, None, False, None, None
    for j in range(Ld):
        d, Pd = m.decoder[Ld - 1 - j], P["dec"][Ld - 1 - j]
        xj = enc_out[-j - 1]                                                # :218
        what = "the posterior block of level %d (decoder.%d.att)" % (j, Ld - 1 - j)
        if j == 0:                                                          # compute_posterior(x, None): att(x, x)  (:73-75)
            y, nk = W.cast_of(xj, kc.pad64(D), what), T
            why = "the bf16 cast of this level's encoder output (level 0 attends to itself)"
        else:                                                               # att(x, o)  (:68-72)
            y, nk = kc.cast_pad_want(o.value, kc.pad64(D)), npts
            why = "bf16(o) as o stands after level %d's decoder block" % (j - 1)
            cp = W.maybe("cast_pad_bf16", lambda c: _eq(c.arg("src"), o.value) and _eq(c.result(), y))
            if cp is None and not imaged:
                raise AssertionError("wiring: nothing produces %s for %s" % (why, what))
            W.name(why, y)
        g = W.find("gemm_bf16", lambda c: _eq(c.arg("w"), Pd["att"]["wkv"]) and c.arg("x").shape[0] == B * nk, "projects the K / V source of %s through fc_kv" % what)
        W.link(g, "x", y, why)
        if j > 0 and image is not None:
            assert (g.args["x"].storage, g.args["x"].offset) == (image.storage, image.offset), "wiring: %s: `x` must be the bf16 image the decoder block of level %d wrote" % (g, j - 1)
        W.link(g, "bias", Pd["att"]["bkv"], "the bias of fc_kv of %s" % what); W.link(g, "epilogue", L.EPI_BF16, "the plain bf16 epilogue")
        W.block(Pd["att"], W.norms(d.att), what, xj, B, T, g.outs[0], nk)
        sp = W.find("sgemm", lambda c: _eq(c.arg("w"), Pd["w_prior"]), "is the `prior` head of level %d (SiLU, Conv1d D -> 2 z)" % j)
        W.link(sp, "a", xj.value, "the posterior block's output of level %d" % j); W.link(sp, "bias", Pd["b_prior"], "its bias")
        W.link(sp, "act_in", L.ACT_SILU, "SiLU in front"); W.link(sp, "act_out", 0, "none")
        if post_noise is None:
            ph = W.find("philox_normal", lambda c: c.arg("step") == j and tuple(c.arg("shape")) == (B, T, z), "draws the posterior noise of level %d" % j)
            nz = ph.out().reshape(B * T, z)
        else:
            nz = post_noise[j].to(pos.device, torch.float32).reshape(B * T, z)
        kind = "reparam_kl" if want_kl else "reparam"
        rp = W.find(kind, lambda c: _eq(c.arg("post"), sp.result()), "draws eps_%d from the posterior of level %d" % (j, j))
        W.link(rp, "noise", nz, "the N(0, 1) draw of level %d" % j, flat=True)
        W.link(rp, "lo", m.min_sigma, "min_sigma"); W.link(rp, "hi", 10., "10")
        if want_kl:
            W.link(rp, "rows_per_sample", T, "z_scales rows per sample")
        r = rp.inplace["out"]["before"]
        eps_lay0 = r.storage if eps_lay0 is None else eps_lay0
        if (r.storage, r.offset, r.shape, r.stride) != (eps_lay0, z * j, (B * T, z), (Ld * z, 1)):
            raise AssertionError("wiring: %s: `out` must be columns [%d z, %d z) of the one [B T, L z] latent buffer (storage offset %d, strides %s), not offset %d, strides %s" % (
                rp, j, j + 1, z * j, [Ld * z, 1], r.offset, list(r.stride)))
        eps_j = W.name("eps_%d, the latents the posterior wrote at level %d" % (j, j), rp.after("out"))
        if want_kl:
            for key, oi in (("kls", 2), ("all_logqz", 3)):
                if not _eqflat(res[key][j].transpose(1, 2), rp.out(oi)):
                    raise AssertionError("wiring: the returned %s[%d] is not what %s left" % (key, j, rp))
            if not _eq(res["kl_sample_sum"][:, j].contiguous(), rp.out(4)):
                raise AssertionError("wiring: the returned kl_sample_sum[:, %d] is not what %s left" % (j, rp))
        r2 = W.decoder_level(j, o, dict(value=eps_j, lay=_lay(r)), "columns [%d z, %d z) of the latents the posterior wrote at level %d" % (j, j + 1, j),
                             npts, T, q_pre, want_image=j + 1 < Ld)
        q_pre, image, imaged, last = r2["q_next"], r2["image"], r2["imaged"], rp
    W.output_conv(o, res["set"], npts)
    if not _eqflat(res["all_eps"], last.inplace["out"]["base_after"]):
        raise AssertionError("wiring: the returned all_eps is not the latent buffer as the last level's draw left it; %s" % W.identify(res["all_eps"]))
    return W.finish()


def audit_sample(calls, model, B, npts, given_eps, out, keep_mask=None, seed_eps=None):
    """Compressor.sample (Network.py:251-268): the initial set, per level the decoder block on columns [z j, z (j + 1)) of the GIVEN latents,
    the output conv."""
    m = model
    W = Table(calls, m, B)
    T, z, Ld = m.z_scales, m.z_dim, m.n_layers
    eps = given_eps.to(W.P["w_out"].device, torch.float32).contiguous().view(B * T, Ld * z)
    o = W.initial_set(npts, keep_mask, seed_eps)
    q_pre = None
    for j in range(Ld):
        lay = (None, z * j, (B * T, z), (Ld * z, 1))
        sg = [c for c in calls if c.name == "sgemm" and _eq(c.arg("w"), W.P["dec"][Ld - 1 - j]["w_zkv"])]
        if sg:
            lay = (sg[0].args["a"].storage,) + lay[1:]                        # (the caller's own copy of the latents: any storage, this offset)
        r = W.decoder_level(j, o, dict(value=eps[:, z * j:z * (j + 1)].contiguous(), lay=lay), "columns [%d z, %d z) of the given latents" % (j, j + 1),
                            npts, T, q_pre, want_image=False)
        q_pre = r["q_next"]
    W.output_conv(o, out, npts)
    return W.finish()


# ------------------------------------------------------------------------------------------------------------- cases
# every entry-point name ldt_amd/blocks.py and ldt_amd/compressor.py can reach through `ops` on the forms this table covers (written by hand;
# pad64 and stream_ptr carry no tensors and are not recorded)
REACHABLE = {
    "sgemm", "gemm_bf16", "cast_pad_bf16", "layernorm_modulate", "norm_apply", "group_stats", "block_activation_", "ln_linear", "ln_mlp_resid_",
    "attention_fwd", "attention_oproj_resid_", "actnorm_", "maxpool", "fps", "knn", "group_normalize", "grouper_mlp", "gather_rows", "norm_points",
    "mixture_seed", "reparam", "reparam_kl", "philox_normal",
}


# name: (config entries replaced in tests/golden/tiny_cfg.json's compressor, B, N input points): the smallest at which the forms differ
CASES = {
    # the fused forms: hidden 64, 2 heads of 32, 8 tokens, 3 levels, 2 encoder layers; N = 256 so that k = 64
    "fused": (dict(), 3, 256),
    # the chains: a width the fused LayerNorm kernels refuse, a head count (and width, 64) the out-projection kernel refuses; a mixture
    # InitialSet, norm_input, ActNorm with one row for all tokens.  (hidden 96 is no case: the norm chain's bf16 rows are the GEMMs' K, a
    # multiple of 64.)  A mixture draws its rows: the keep mask with dropped rows is on the fused case, where there are prior rows to drop
    "chain": (dict(hidden_dim=192, num_heads=3, max_outputs=None, outsize=40, norm_input=True, ActNorm="set", n_layers=2, encoder_layers=1, z_dim=12), 2, 96),
    # what neither reaches: the one-kernel grouper (hidden 128, k = 16), GroupNorm's two kernels, the decoder blocks' activation
    "grouped": (dict(hidden_dim=128, num_heads=4, norm="group_norm", decoder_act="gelu", n_layers=2, encoder_layers=1, max_outputs=24, outsize=24), 2, 64),
}
DROPPED = 40                                                            # of the fused case's 64 prior rows, where a run keeps a subset


def make_case(ccfg, seed=5, **over):
    """-> (a seeded Compressor(cfg).init() on the CPU in eval mode, its config), in compressor_tape.make_case's style: `over` replaces config
    entries; the norms' gamma / beta, ActNorm, the grouper's affine and BatchNorm's running statistics are moved off their default
    initialisation (1 / 0), where a dropped or doubled application would go unseen."""
    import ldt_amd
    c = copy.deepcopy(ccfg)
    for k, v in over.items():
        setattr(c, k, v)
    torch.manual_seed(seed)
    model = ldt_amd.Compressor(c)
    model.init()
    g = torch.Generator().manual_seed(seed + 11)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".norm1." in n or ".norm2." in n or n.endswith("conv_out.norm.weight") or n.endswith("conv_out.norm.bias"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif n.startswith("conv_in."):
                p.add_(0.3 * torch.randn(p.shape, generator=g))
            elif "affine_alpha" in n or "affine_beta" in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for n, b in model.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.2 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.mul_(0.5 + torch.rand(b.shape, generator=g))
    model.eval()
    return model, c


def clouds(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 3, generator=g) * 0.5 + 0.1 * torch.randn(B, 1, 3, generator=g)


# ------------------------------------------------------------------------------------------------------------- the C++ Score forward, by stage
# `ldt_score_forward` is one call: no proxy sees its launches.  Its workspace (X, Hb, QKV, Ob, U) is the caller's, its plan a struct the caller
# fills and its AdaLN table a tensor of the caller's, so two observation devices expose every stage without touching product code:
#   * prefix plans: the plan with `blocks = n` leaves Ob, U (QKV on the two-kernel route) of block n - 1 and X after n blocks; its FinalLayer
#     LayerNorm then reads the rows at mod + n 6 D, which for n < L are block n's shift_msa | scale_msa: Hb IS block n's LN1 output (the same
#     launcher, the same arguments); for n = L it is the FinalLayer's own;
#   * zero-gate tables: block l's gate_mlp columns zeroed make prefix l + 1 leave X after fc_o (X_mid); both gates of block 0 zeroed make
#     prefix 1 leave the ln_in output X_0, and with block 0's shift_msa | scale_msa copied over the rows that prefix's last LayerNorm reads
#     (`blocks = 0` is refused), its Hb is block 0's LN1 output.
# Every stage is then held from device-OBSERVED inputs only, with the bound that holds its kernel alone.  The LN-folded plans are outside:
# their xs rows are overwritten before any prefix could read them.
STAGE_BUFFERS = ("X", "Hb", "QKV", "Ob", "U")


def score_panels(model, kv_cond=None):
    """The operands of the unfolded branch by name, from `Score.packed()`."""
    P = model.packed()
    S = dict(w_in=P["w_in"], b_in=P["b_in"], w_out=P["w_out"], b_out=P["b_out"], blocks=[])
    for l in range(model.num_blocks):
        b = {k: P[k][l] for k in ("w_qkv", "b_qkv", "w_o", "b_o", "w_up", "b_up", "w_dn", "b_dn")}
        if kv_cond and l in kv_cond:
            b["w_q"], b["b_q"] = model._cross_panels(l)[:2]
            b["kv"] = kv_cond[l]
        S["blocks"].append(b)
    return S


def mod_variant(mod, D, zero=(), copy=()):
    """A copy of the AdaLN table with column blocks `zero` zeroed and, for (dst, src) in `copy`, block dst overwritten by block src (every row)."""
    m = mod.clone()
    for dst, src in copy:
        m[:, dst * D:(dst + 1) * D] = mod[:, src * D:(src + 1) * D]
    for k in zero:
        m[:, k * D:(k + 1) * D] = 0
    return m


def audit_score_stages(run, S, dims, x, mod, sample_stride, step=None):
    """run(n, table) -> {X, Hb, QKV, Ob, U, eps}: clones of the workspace (pre-filled with NaN by the runner) and of eps_out after the plan with
    `blocks = n` (None: the plan as the product builds it) ran on `table`.  S: score_panels; dims: (B, T, D, H, L, z); mod: the table
    [rows, n_mod], read at row `step` (batch-shared, sample_stride 0) or one row per sample (sample_stride = n_mod).
    -> {stage: worst err / bound (or a share)}; a failure names the stage and the block."""
    L_ = _lib()
    B, T, D, H, L, z = dims
    M, dh = B * T, D // H
    E = kc.assert_elementwise
    worst = {}

    def put(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    rows = mod if sample_stride else mod[(step or 0):(step or 0) + 1]            # the rows in use: one per sample, or the step's one
    assert sample_stride in (0, mod.shape[1]) and (rows.shape[0] == B if sample_stride else True)
    rps = T if sample_stride else M
    col = lambda k: rows[:, k * D:(k + 1) * D]
    nxt = 6 if L > 1 else 6 * L                                                   # the column block prefix 1's last LayerNorm reads
    base = {n: run(n, mod) for n in range(1, L + 1)}
    zmlp = {l: run(l + 1, mod_variant(mod, D, zero=(6 * l + 5,))) for l in range(L)}
    x0 = run(1, mod_variant(mod, D, zero=(2, 5), copy=((nxt, 0), (nxt + 1, 1))))
    # ---- what the observations rest on
    for n in range(1, L + 1):
        again = run(n, mod)
        for k in STAGE_BUFFERS + ("eps",):
            same = torch.equal(tt._bits(again[k]), tt._bits(base[n][k]))
            assert same, "score stages: two runs of prefix %d leave different bits in %s: not reproducible, the stage cannot be observed this way" % (n, k)
    two_kernel = {l: bool(torch.isfinite(base[l + 1]["QKV"][:, :(D if "kv" in S["blocks"][l] else 3 * D)].float()).all()) for l in range(L)}
    for name, obs in [("prefix %d" % n, base[n]) for n in base] + [("prefix %d with gate_mlp of block %d zeroed" % (l + 1, l), zmlp[l]) for l in zmlp] + [("prefix 1 with both gates of block 0 zeroed", x0)]:
        for k in ("X", "Hb", "Ob", "U"):
            assert bool(torch.isfinite(obs[k].float()).all()), "score stages: %s leaves non-finite values in %s (not written, or overflowed)" % (name, k)
    for l in range(L):                                                           # a zeroed gate must not move what runs before it
        for k, stage in (("Ob", "q | k | v + attention"), ("U", "LN2 + mlp.fc + GELU")):
            assert torch.equal(tt._bits(zmlp[l][k]), tt._bits(base[l + 1][k])), \
                "score stage `%s` of block %d: %s changes when gate_mlp of that block is zeroed (the stage reads AdaLN columns that are not its own)" % (stage, l, k)
    full = run(None, mod)
    assert torch.equal(tt._bits(full["eps"]), tt._bits(base[L]["eps"])), "score stages: the full plan's eps_out differs from the prefix-%d run's" % L
    # ---- ln_in: X_0 from the latents                                                                    (score.py:136-137)
    X = x0["X"]
    xin = kc.cast_pad_want(x.reshape(M, z).float(), S["w_in"].shape[1])
    ref, tol = gemm_reference(xin, S["w_in"], S["b_in"], L_.EPI_F32)
    put("ln_in X_0", E(X, ref, tol, "score stage `ln_in` (X_0 from cast_pad(x))"))

    def ln(stage, l, Xin, k, got):
        pre, al, _, _ = kc.ln_stage(Xin, shift=col(k), scale=col(k + 1), rows_per_sample=rps)
        return E(got, pre, al + kc.U8 * pre.abs() * (1 + kc.U8), "score stage `%s` of block %d (from the observed X, mod columns [%d D, %d D))" % (stage, l, k, k + 2))

    def gate_rows(k):
        return kc.sample_rows(col(k), M, rps)

    for l in range(L):
        Sb, what = S["blocks"][l], "of block %d" % l
        Hb1 = x0["Hb"] if l == 0 else base[l]["Hb"]
        put("LN1 Hb", ln("LN1", l, X, 6 * l, Hb1))
        # q | k | v + attention from the observed Hb                                                     (layers.py:183-197)
        obs = base[l + 1]
        cross = "kv" in Sb
        w, bias = (Sb["w_q"], Sb["b_q"]) if cross else (Sb["w_qkv"], Sb["b_qkv"])
        pre = Hb1.double() @ w.double().T + bias.double()
        acc = kc.gemm_acc_err(Hb1, w, bias, D)
        kv = (Sb["kv"][:, :D], Sb["kv"][:, D:]) if cross else None
        Nk = Sb["kv"].shape[0] // B if cross else None
        ref, tol, ratio, amb = kc.fused_attention_tol(pre, acc, B, H, T, dh, kv=kv, Nk=Nk)
        put("qkv + attention Ob", E(obs["Ob"].reshape(-1, dh), ref.reshape(-1, dh), tol.reshape(-1, dh), "score stage `q | k | v + attention` %s (Ob from the observed Hb)" % what))
        put("qkv + attention, tol / base max" + SHARE, float(ratio.max()))
        if two_kernel[l]:
            N = D if cross else 3 * D
            qkv = obs["QKV"][:, :N]
            put("QKV (two kernels)", E(qkv, pre, acc * (1 + kc.U8) + kc.U8 * pre.abs(), "score stage `q | k | v projection` %s (QKV from the observed Hb)" % what))
            k_, v_ = kv if cross else (qkv[:, D:2 * D], qkv[:, 2 * D:])
            r2, vmax = kc.attention_ref64(qkv[:, :D], k_, v_, B, H, T, Nk or T, dh)
            put("attention Ob (two kernels)", E(obs["Ob"].reshape(-1, dh), r2.reshape(-1, dh), kc.attention_base_tol(r2, vmax).reshape(-1, dh),
                                                "score stage `attention` %s (Ob from the observed QKV)" % what))
        # x = x + gate_msa fc_o(attention)                                                                (layers.py:198, 218)
        Xmid = zmlp[l]["X"]
        ref, tol = gemm_reference(obs["Ob"], Sb["w_o"], Sb["b_o"], L_.EPI_RESID_F32, resid=X, gate_rows=gate_rows(6 * l + 2))
        put("fc_o X_mid", E(Xmid, ref, tol, "score stage `fc_o + gated residual` %s (X_mid from the observed Ob and X)" % what))
        # U = GELU(mlp.fc(modulate(norm2(x))))                                                            (layers.py:219): fused_mlp_reference's first stages
        _, _, rh, eh = kc.ln_stage(Xmid, shift=col(6 * l + 3), scale=col(6 * l + 4), rows_per_sample=rps)
        Wu, Bu = Sb["w_up"].double(), Sb["b_up"].double()
        pu = rh @ Wu.T + Bu
        au = eh @ Wu.abs().T + kc.C_ACC * D * kc.U24 * (rh.abs() @ Wu.abs().T + Bu.abs())
        pg, ag = torch.nn.functional.gelu(pu), kc.GELU_SLOPE * au + kc.GELU_FAST_ABS
        lo, hi = kc.bf16_round(pg - ag), kc.bf16_round(pg + ag)
        kc.assert_interval(obs["U"], lo, hi, "score stage `LN2 + mlp.fc + GELU` %s (U from the observed X_mid)" % what)
        put("LN2 + up + GELU U", 0.0)
        put("LN2 + up + GELU U, pinned" + SHARE, float((lo == hi).double().mean()))
        # x = x + gate_mlp mlp.out(U)
        ref, tol = gemm_reference(obs["U"], Sb["w_dn"], Sb["b_dn"], L_.EPI_RESID_F32, resid=Xmid, gate_rows=gate_rows(6 * l + 5))
        put("mlp.out X_next", E(obs["X"], ref, tol, "score stage `mlp.out + gated residual` %s (X after the block from the observed U and X_mid)" % what))
        X = obs["X"]
    put("FinalLayer Hb", ln("FinalLayer LN", L, X, 6 * L, base[L]["Hb"]))
    ref, tol = gemm_reference(base[L]["Hb"], S["w_out"][:z], S["b_out"][:z], L_.EPI_F32)
    put("FinalLayer eps_out", E(base[L]["eps"].reshape(M, z), ref, tol, "score stage `FinalLayer projection` (eps_out from the observed Hb)"))
    return worst, two_kernel
