"""The call tape of the Compressor's three training steps and the audits read from it (a plain helper module: test_gpu_compressor_tape.py
runs it on the MI355X, test_compressor_tape_host.py on a pure-torch emulation of the entry points, planted faults included).

`ldt_amd.compressor_train` reaches every kernel through its module attribute `ops`; train_tape.Tape records every call made through it.
  * `audit_numeric`: every call of a backward against float64 from its OWN recorded operands, with the references and bounds that hold each
    kernel alone (kernel_checks, decoder_train_checks, topdown_train_checks, encoder_train_checks, narrow_bwd_checks); around every
    destination the storage outside the view unchanged bit for bit.  No bound is new.
  * `audit_centred`: the calls of `_centred_keys` on the forward's part of the tape (the forward builds the backward's K there).
  * `audit_decoder`, `audit_topdown`, `audit_encoder`: what every call's operands MUST be, written down from the reference
    (model/Compressor/Network.py:12-29, 41-45, 61-83, 200-233, 251-268, model/layers.py:103-107, 183-200, 210-226, 240-246,
    model/Compressor/layers.py:26-42), each link checked with torch.equal between a recorded operand and the recorded output of its
    producer, a saved forward tensor or a parameter; every trained parameter's final .grad bit-equal to what its owning call left; no call
    left unplaced.  Calls are found by what they read or write, never by position.
The references used here state no condition on their inputs beyond shapes and dtypes (attn_bwd_ref's bound is componentwise in the recorded
operands themselves); the shapes are asserted where a reference needs them (head width 32, the raw [B][H][Nq][32] buffers)."""
import copy

import torch

import decoder_train_checks as dc
import encoder_train_checks as ec
import kernel_checks as kc
import narrow_bwd_checks as nb
import topdown_train_checks as tc
import train_tape as tt
from train_tape import _eq, _eqflat, layout

ATTENTION = ("attention_bwd_cross", "attention_bwd_long", "attention_bwd_wide")


# ------------------------------------------------------------------------------------------------------------- numeric audit
def prior_row_map_want(keep):
    """The definition restated (Compressor/layers.py:34-37: a sample's kept prior rows, in index order, become its rows 0, 1, ...):
    src[b][r] = the position of r among sample b's kept rows, -1 where it is not kept."""
    keep = keep.to(torch.bool).cpu()
    want = torch.full(keep.shape, -1, dtype=torch.int32)
    for b in range(keep.shape[0]):
        rows = torch.nonzero(keep[b]).flatten()
        want[b, rows] = torch.arange(rows.numel(), dtype=torch.int32)
    return want


def check_call(call):
    """One call against float64 from its own recorded operands -> {what: err / tol}.  train_tape.check_call for the kinds it knows."""
    a, nm = call.arg, call.name
    E = kc.assert_elementwise
    if nm in ATTENTION:
        B, H, Nq, Nk = a("B"), a("H"), a("Nq"), a("Nk")
        assert a("head_dim") == 32, "%s: head_dim %r" % (call, a("head_dim"))
        C = H * 32
        # o and do: the raw [B][H][Nq][32] buffers (quirk Q1), whatever shape they were handed over in
        assert a("o").numel() == B * H * Nq * 32 and a("do").numel() == B * H * Nq * 32, "%s: o / do are not [B][H][Nq][32]" % call
        o, do = a("o").reshape(B, H, Nq, 32), a("do").reshape(B, H, Nq, 32)
        kv = torch.cat([a("k"), a("v")], 1)
        assert tuple(a("q").shape) == (B * Nq, C) and tuple(kv.shape) == (B * Nk, 2 * C), "%s: q / k / v shapes" % call
        got = {k: call.out(i) for i, k in enumerate(("dq", "dk", "dv"))}
        if "dkv_out" in call.inplace:
            assert _eq(torch.cat([got["dk"], got["dv"]], 1), call.after("dkv_out")), "%s: dk | dv are not the two halves of `dkv_out`" % call
        if nm == "attention_bwd_cross":
            return {nm: nb.check(got, a("q"), kv, o, do, B, H, Nq, Nk, 32, str(call))}
        r = (dc.long_check if nm == "attention_bwd_long" else tc.wide_check)(got, a("q"), kv, o, do, B, H, Nq, Nk, str(call))
        return {"%s %s" % (nm, k): v for k, v in r.items()}
    if nm == "reparam_kl_bwd":
        post, lo, hi = a("post"), a("lo"), a("hi")
        z = post.shape[1] // 2
        ref, tol = tc.reparam_kl_bwd_closed(post, a("noise"), a("d_eps"), a("kl_scale"), lo, hi)
        r = E(call.out(), ref, tol, str(call))
        dead = (post[:, z:] < lo) | (post[:, z:] > hi)
        assert bool((call.out()[:, z:][dead] == 0).all()), "%s: dlogvar is not exactly 0 outside the clamp" % call
        return {nm: r}
    if nm == "rows_gather_sum":
        ref, tol = dc.rows_gather_sum_ref(a("dy"), a("src"), a("N"))
        return {nm: E(call.out().cpu(), ref, tol, str(call))}
    if nm == "actnorm_bwd":
        B = a("B")
        dz = a("dz").reshape(B, -1)                                     # recorded BEFORE the call: `dx` may be the very tensor
        ref, tol = ec.actnorm_bwd_ref(dz, a("z").reshape(B, -1), a("log_scale").reshape(-1))
        dx = (call.after("dx") if "dx" in call.inplace else call.out(0)).reshape(B, -1)
        r = {"actnorm_bwd dx": E(dx, ref[0], tol[0], "%s, dx against the recorded dz" % call)}
        if a("want_sums"):
            for i, k in ((1, "dshift"), (2, "dlog_scale")):
                got = call.after(k) if k in call.inplace else call.out(i)
                r["actnorm_bwd " + k] = E(got.reshape(-1), ref[i], tol[i], "%s, %s" % (call, k))
        return r
    if nm == "widen_bf16":
        assert call.out().dtype == torch.float32 and torch.equal(call.out(), a("w").float()), "%s: not the bf16 values widened" % call
        return {nm: 0.0}
    if nm == "add_f32":
        assert torch.equal(call.result(), a("a") + a("b")), "%s: not the fp32 sum of the recorded operands" % call      # `a` as recorded before
        return {nm: 0.0}
    if nm == "prior_row_map":
        assert call.out().dtype == torch.int32 and torch.equal(call.out().cpu(), prior_row_map_want(a("keep"))), "%s: not the row map" % call
        return {nm: 0.0}
    if nm == "sgemm":
        assert not (a("act_in") or a("act_out") or a("out_bf16")), "%s: an sgemm with an activation on a backward's tape (unaudited)" % call
    return tt.check_call(call)                                          # (raises for a call kind without a reference)


def audit_numeric(calls, worst=None):
    """Every call of `calls` (a backward's): check_call + check_untouched.  -> {call kind: largest err / tol}."""
    worst = {} if worst is None else worst
    for call in calls:
        tt.check_untouched(call)
        for k, r in check_call(call).items():
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


def audit_centred(calls, groups, worst=None):
    """The calls of `_centred_keys` among `calls` (the forward's).  groups: one dict per block whose backward reads centred keys:
    y bf16 [B nk, C] (the K / V source), kv (the saved K | V the backward reads), w_k bf16 [C, C], b_k fp32 [C], B, nk, what.
    Per sample b: the column sum of the uncentred K rows; one sgemm forms b_k - mean key; the GEMM into kv[b nk : (b + 1) nk, :C] against
    float64 y W_k^T + bias_b with gemm_tol, the V half and the other samples' rows unchanged.  -> {kind: largest err / tol}."""
    from ldt_amd._lib import EPI_BF16
    worst = {} if worst is None else worst
    E = kc.assert_elementwise
    put = lambda k, r: worst.__setitem__(k, max(worst.get(k, 0.0), r))
    gemms = [c for c in calls if c.name == "gemm_bf16" and "out" in c.inplace and c.arg("epilogue") == EPI_BF16]
    sums, seen = [c for c in calls if c.name == "colsum"], set()
    for g in groups:
        B, nk, C, what = g["B"], g["nk"], g["w_k"].shape[0], g["what"]
        rows, cs = [], []
        for b in range(B):
            yb = g["y"][b * nk:(b + 1) * nk]
            hit = [c for c in gemms if c.index not in seen and _eq(c.arg("x"), yb) and _eq(c.arg("w"), g["w_k"])
                   and (c.inplace["out"]["before"].offset, c.inplace["out"]["before"].shape, c.inplace["out"]["before"].stride) == (b * nk * 2 * C, (nk, C), (2 * C, 1))]
            assert hit, "centred keys: no gemm_bf16 call writes the K half of rows [%d nk, %d nk) of %s from its K / V source and W_k" % (b, b + 1, what)
            c = hit[0]
            seen.add(c.index)
            tt.check_untouched(c)                                       # the V half and the other samples' rows: the same bits
            k_raw = c.before("out")
            s = [x for x in sums if x.index not in seen and _eq(x.arg("dy"), k_raw)]
            assert s, "centred keys: no colsum call reads the uncentred K rows of sample %d of %s" % (b, what)
            seen.add(s[0].index)
            ref, tol = kc.colsum_ref(s[0].arg("dy"))
            put("centred colsum", E(s[0].result(), ref, tol, "%s (sample %d of %s)" % (s[0], b, what)))
            rows.append(c)
            cs.append(s[0].result())
        off = torch.eye(C, dtype=torch.float32, device=g["w_k"].device) * (-1.0 / nk)
        sg = [c for c in calls if c.name == "sgemm" and c.index not in seen and _eq(c.arg("a"), torch.stack(cs)) and _eq(c.arg("w"), off)]
        assert sg, "centred keys: no sgemm call forms b_k - mean key from the %d column sums of %s" % (B, what)
        sg = sg[0]
        seen.add(sg.index)
        assert _eqflat(sg.arg("bias"), g["b_k"]) and not sg.arg("act_in") and not sg.arg("act_out"), "centred keys: %s: the bias must be b_k of %s, no activation" % (sg, what)
        ref, tol = kc.sgemm_ref(sg.arg("a"), sg.arg("w"), sg.arg("bias"))
        put("centred sgemm", E(sg.result(), ref, tol, "%s (%s)" % (sg, what)))
        for b, c in enumerate(rows):
            assert _eqflat(c.arg("bias"), sg.result()[b]), "centred keys: %s: the bias must be row %d of b_k - mean key of %s" % (c, b, what)
            x, w, bias = c.arg("x"), c.arg("w"), c.arg("bias")
            ref = x.double() @ w.double().T + bias.double()
            put("centred gemm_bf16", E(c.after("out"), ref, kc.gemm_tol(x, w, bias, x.shape[1], torch.bfloat16, ref=ref), "%s (sample %d of %s)" % (c, b, what)))
        last = rows[-1].inplace["out"]["base_after"]
        assert _eqflat(last, g["kv"]), "centred keys: the K | V the backward of %s reads is not what the last centring GEMM left" % what
        first = rows[0].inplace["out"]["base_before"].view(B * nk, 2 * C)
        assert torch.equal(first[:, C:], g["kv"][:, C:]), "centred keys: the V half of %s is not the forward's" % what
    return worst, len(seen)


# ------------------------------------------------------------------------------------------------------------- wiring audit
def _tr(t):
    return t.t().contiguous()


class Table(tt.Wiring):
    """train_tape.Wiring plus the pieces the three tables share."""

    def __init__(self, calls, model):
        super().__init__(calls)
        from ldt_amd import _lib
        self.epi_bf16, self.epi_f32 = _lib.EPI_BF16, _lib.EPI_F32
        self.grad_of = {}                                               # parameter -> (what its final .grad must be, the owning call)
        self.pname = {p: n for n, p in model.named_parameters()}

    def find(self, kind, pred, what):
        """train_tape's, preferring a call no link has claimed yet (two calls may read bit-equal operands)."""
        fresh = [c for c in self.calls if c.name == kind and c.index not in self.seen and pred(c)]
        if fresh:
            self.seen.add(fresh[0].index)
            return fresh[0]
        return super().find(kind, pred, what)

    def name_saved(self, S):
        """Every saved tensor of a decoder / top-down step by name, so that a message can say what a wrong operand IS."""
        for key, what in (("levels", "decoder level"), ("post", "posterior level")):
            for j, sb in enumerate(S.get(key, [])):
                for k, t in sb.items():
                    if torch.is_tensor(t):
                        self.name("%s of %s %d (saved forward)" % (k, what, j), t)

    def own(self, p, want, call):
        self.grad_of[p] = (want, call)

    def alias(self, call, dest, arg, what):
        """The in-place operand `dest` of `call` is the very view passed as `arg`."""
        d, s = call.inplace.get(dest, {}).get("before"), call.args.get(arg)
        ok = d is not None and isinstance(s, tt.Rec) and (d.storage, d.offset, d.shape, d.stride) == (s.storage, s.offset, s.shape, s.stride)
        assert ok, "wiring: %s: `%s` must be the very tensor passed as `%s` (%s)" % (call, dest, arg, what)

    def linear(self, layer, dy, x, what, flat_x=False):
        """dW = dy^T x into the layer's weight .grad (all its rows), db = column sums of dy into the bias .grad."""
        cw = self.dest("wgrad", "out", layer.weight.grad.view(layer.weight.shape[0], -1), "the .grad of %s" % self.pname[layer.weight])
        self.link(cw, "dy", dy, "the gradient of the output of %s" % what)
        self.link(cw, "x", x, "the forward's input of %s" % what, flat=flat_x)
        self.own(layer.weight, cw.after("out"), cw)
        cb = self.dest("colsum", "out", layer.bias.grad, "the .grad of %s" % self.pname[layer.bias])
        self.link(cb, "dy", dy, "the gradient of the output of %s" % what)
        self.own(layer.bias, cb.after("out"), cb)

    def dgrad(self, layer, dy, epilogue, what, w=None):
        """dX = dy W through the transposed bf16 panel of the CURRENT weights; an fp32 (or narrow) dy first becomes a padded bf16 operand."""
        from ldt_amd.layers import conv_w
        w = (conv_w(layer) if w is None else w).detach().contiguous()
        want = kc.transpose_cast_want(w)
        t = self.find("transpose_cast_bf16", lambda c: _eq(c.arg("src"), w) and _eq(c.result(), want), "transposes the current weights of %s" % what)
        if dy.dtype != torch.bfloat16 or dy.shape[1] % 64:
            cp = self.find("cast_pad_bf16", lambda c: _eq(c.arg("src"), dy), "casts the gradient of the output of %s to the dgrad's bf16 operand" % what)
            assert _eq(cp.result(), kc.cast_pad_want(dy, kc.pad64(dy.shape[1]))), "wiring: %s: not bf16(dy) padded to 64 columns" % cp
            dy = cp.result()
        dg = self.find("dgrad", lambda c: _eq(c.arg("w_t"), t.result()) and _eq(c.arg("dy"), dy), "multiplies the gradient of the output of %s by its transposed weights" % what)
        self.link(dg, "epilogue", epilogue, "epilogue %d" % epilogue)
        return self.name("dgrad through %s" % what, dg.result())

    def affine_ln(self, norm, x, dy, dx_in, what):
        """h = LN(x) gamma + beta (the no-condition block): the modulation backward with scale = fp32 gamma - 1, ONE sample of M rows,
        dshift / dscale the .grad views of beta / gamma, dx coming in as the stream gradient so far."""
        w, b = norm.affine
        M, C = x.shape
        c = self.dest("layernorm_modulate_bwd", "dshift", b.grad.view(1, C), "the .grad of %s (dshift of %s)" % (self.pname[b], what))
        r = c.inplace.get("dscale", {}).get("before")
        assert r is not None and (r.storage, r.offset, r.shape, r.stride) == layout(w.grad.view(1, C)), \
            "wiring: %s: dscale of %s must be the .grad of %s" % (c, what, self.pname[w])
        self.link(c, "x", x, "the forward's input of %s" % what)
        self.link(c, "dy", dy, "the gradient of the output of %s" % what)
        gm1 = (w.detach().float() - 1.0).view(1, C)
        self.link(c, "scale", gm1, "fp32 gamma - 1 of %s" % what)
        self.link(c, "rows_per_sample", M, "M = %d (one sample of all rows)" % M)
        self.link(c, "mod_sample_stride", 0, "0")
        self.link(c, "want_mod", True, "True")
        if not _eq(c.before("dx"), dx_in):
            raise AssertionError("wiring: %s: dx must come in as the stream gradient so far (%s); %s" % (c, what, self.identify(c.before("dx"))))
        ad = self.find("add_f32", lambda k: _eqflat(k.arg("a"), w.detach()) and _eqflat(k.result(), gm1), "forms gamma - 1 of %s" % what)
        self.link(ad, "b", torch.full_like(ad.arg("b"), -1.0), "-1 everywhere")
        self.own(w, c.after("dscale"), c)
        self.own(b, c.after("dshift"), c)
        return self.name("dX after %s" % what, c.after("dx"))

    def attention(self, kind, sb, do, B, H, Nq, Nk, what):
        """The attention backward of one block: which entry point, dO, the saved q / o, the two halves of the saved K | V, the lengths."""
        C = H * 32
        at = self.find(kind, lambda c: _eqflat(c.arg("do"), do), "reads dO = the bf16 dgrad of fc_o of %s as the raw [B][H][Nq][32] buffer" % what)
        self.link(at, "q", sb["q"], "the saved q of %s" % what)
        self.link(at, "o", sb["o"], "the saved attention output o of %s" % what, flat=True)
        self.link(at, "k", sb["kv"][:, :C].contiguous(), "columns [0, C) of the saved (centred) K | V of %s" % what)
        self.link(at, "v", sb["kv"][:, C:].contiguous(), "columns [C, 2 C) of the saved K | V of %s" % what)
        for nm, v in (("B", B), ("H", H), ("Nq", Nq), ("Nk", Nk), ("head_dim", 32)):
            self.link(at, nm, v, "%s = %d" % (nm, v))
        assert "dkv_out" in at.inplace, "wiring: %s: [dk | dv] must go to the `dkv_out` given" % at
        dkv = self.name("[dk | dv] of %s" % what, at.after("dkv_out"))
        assert _eq(torch.cat([at.out(1), at.out(2)], 1), dkv), "wiring: %s: dk | dv are not the two halves of `dkv_out`" % at
        return self.name("dq of %s" % what, at.out(0)), dkv

    def nocond_block(self, blk, sb, dX, B, H, Nq, Nk, kind, what):
        """The no-condition ResidualBlock (layers.py:224-226, 183-200) backwards: dX, the gradient of the block's result -> (the gradient of
        its input, [dk | dv])."""
        # x = x2 + mlp.out(GELU(mlp.fc(LN2(x2))))                                                      (layers.py:226)
        self.linear(blk.mlp.out, dX, sb["ug"], "mlp.out of %s" % what)
        dug = self.dgrad(blk.mlp.out, dX, self.epi_f32, "mlp.out of %s" % what)
        ge = self.find("gelu_bwd", lambda c: _eq(c.arg("dh"), dug), "reads the gradient of GELU's output in %s" % what)
        self.link(ge, "u", sb["u"], "the saved MLP pre-activation u of %s" % what)
        du = self.name("gradient of u, %s" % what, ge.result())
        self.linear(blk.mlp.fc[0][0], du, sb["h2"], "mlp.fc of %s" % what)
        dh2 = self.dgrad(blk.mlp.fc[0][0], du, self.epi_f32, "mlp.fc of %s" % what)
        dX = self.affine_ln(blk.norm2, sb["x2"], dh2, dX, "norm2 of %s" % what)
        # x2 = x1 + fc_o(attention(fc_q(LN1(x1)), K | V))                                              (layers.py:225)
        self.linear(blk.fc_o, dX, sb["o"], "fc_o of %s (the raw [B][H][Nq][32] O read as (M, C), quirk Q1)" % what, flat_x=True)
        do = self.dgrad(blk.fc_o, dX, self.epi_bf16, "fc_o of %s" % what)
        dq, dkv = self.attention(kind, sb, do, B, H, Nq, Nk, what)
        self.linear(blk.fc_q, dq, sb["h"], "fc_q of %s" % what)
        dh = self.dgrad(blk.fc_q, dq, self.epi_f32, "fc_q of %s" % what)
        return self.affine_ln(blk.norm1, sb["x1"], dh, dX, "norm1 of %s" % what), dkv

    def output_conv(self, m, dset, S):
        """set = output(o_L), Conv1d C -> 3 (Network.py:233, 266) -> the gradient of o_L."""
        from ldt_amd.layers import conv_w
        d2 = self.name("d_set", dset.detach().float().contiguous().view(-1, 3))
        self.linear(m.output, d2, S["xf"], "the output conv")
        sg = self.find("sgemm", lambda c: _eq(c.arg("a"), d2) and _eq(c.arg("w"), _tr(conv_w(m.output).detach().float())), "carries d_set through the output conv's weights, transposed")
        return self.name("gradient of the final set stream", sg.result())

    def decoder_level(self, m, S, j, dX, d_eps):
        """DecoderBlock.forward (Network.py:80-83): o <- att1(o, ln(eps_j)); K | V = fc_kv(ln(eps_j)) is ONE composed linear that hands its
        gradient to both factors.  -> (the gradient of the block's input stream, the recorded d_eps slice j)."""
        from ldt_amd.layers import conv_w
        L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
        B, N, T = S["B"], S["N"], S["T"]
        d = m.decoder[L - 1 - j]                                         # reversed(self.decoder), Network.py:263
        blk, what = d.att1, "decoder level %d (decoder.%d.att1)" % (j, L - 1 - j)
        dX, dkv = self.nocond_block(blk, S["levels"][j], dX, B, H, N, T, "attention_bwd_long", what)
        wd = self.find("widen_bf16", lambda c: _eq(c.arg("w"), dkv), "widens [dk | dv] of %s" % what)
        dkv32 = self.name("dkv32 of %s" % what, wd.result())
        e_j = S["eps"][:, z * j: z * (j + 1)].contiguous()
        s1 = self.find("sgemm", lambda c: _eq(c.arg("a"), _tr(dkv32)) and "out" not in c.inplace, "forms dW_zkv = dkv32^T eps_%d of %s" % (j, what))
        self.link(s1, "w", _tr(e_j), "columns [%d z, %d z) of the latents, transposed" % (j, j + 1))
        dW = self.name("dW_zkv of %s" % what, s1.result())
        cs = self.find("colsum", lambda c: _eq(c.arg("dy"), dkv32), "forms db_zkv = the column sums of dkv32 of %s" % what)
        db = self.name("db_zkv of %s" % what, cs.result())
        f32 = lambda t: t.detach().float().contiguous()
        w_kv, w_ln, b_ln = f32(conv_w(blk.fc_kv)), f32(conv_w(d.ln)), f32(d.ln.bias)
        s2 = self.dest("sgemm", "out", blk.fc_kv.weight.grad.view(2 * C, -1), "the .grad of %s" % self.pname[blk.fc_kv.weight])
        self.link(s2, "a", torch.cat([dW, db[:, None]], 1), "[dW_zkv | db_zkv] of %s (K = z + 1)" % what)
        self.link(s2, "w", torch.cat([w_ln, b_ln[:, None]], 1), "[W_ln | b_ln] of decoder.%d.ln" % (L - 1 - j))
        self.own(blk.fc_kv.weight, s2.after("out"), s2)
        self.own(blk.fc_kv.bias, db, cs)                                 # fc_kv.bias.grad = db_zkv (torch glue: held by the final .grad)
        s3 = self.dest("sgemm", "out", d.ln.weight.grad.view(C, -1), "the .grad of %s" % self.pname[d.ln.weight])
        self.link(s3, "a", _tr(w_kv), "W_kv^T of %s" % what)
        self.link(s3, "w", _tr(dW), "dW_zkv^T of %s" % what)
        self.own(d.ln.weight, s3.after("out"), s3)
        s4 = self.dest("sgemm", "out", d.ln.bias.grad.view(1, C), "the .grad of %s" % self.pname[d.ln.bias])
        self.link(s4, "a", db.view(1, 2 * C), "db_zkv of %s as one row" % what)
        self.link(s4, "w", _tr(w_kv), "W_kv^T of %s" % what)
        self.own(d.ln.bias, s4.after("out"), s4)
        de = d_eps.view(B * T, L * z)[:, z * j: z * (j + 1)]
        s5 = self.dest("sgemm", "out", de, "columns [%d z, %d z) of the one [B T, L z] d_eps buffer (level %d)" % (j, j + 1, j))
        self.link(s5, "a", dkv32, "dkv32 of %s" % what)
        w_zkv_t = S["w_zkv_t"][j]
        self.link(s5, "w", w_zkv_t, "the saved W_zkv^T of level %d" % j)
        ref, tol = kc.sgemm_ref(w_kv, _tr(w_ln))                         # the saved panel IS (W_kv W_ln)^T of the current weights
        kc.assert_elementwise(_tr(w_zkv_t), ref, tol, "the saved W_zkv of level %d against float64 W_kv W_ln" % j)
        return dX, self.name("d_eps slice %d" % j, s5.after("out"))

    def prior_rows(self, m, S, dX, keep_mask):
        """init_set.prior.grad = the rows of dX gathered per prior row and summed over the samples that kept it (Compressor/layers.py:26-42)."""
        B, N = S["B"], S["N"]
        keep = torch.ones((B, N), dtype=torch.bool) if keep_mask is None else keep_mask
        rg = self.find("rows_gather_sum", lambda c: True, "gathers the prior rows' gradient")
        self.link(rg, "dy", dX, "the gradient of the initial set, after every level")
        self.link(rg, "src", prior_row_map_want(keep).to(rg.arg("src").device), "prior_row_map of the call's keep mask")
        self.link(rg, "N", N, "N = %d" % N)
        self.own(m.init_set.prior, rg.out(), rg)

    def finish(self, params, skip=()):
        """Every trained parameter's final .grad is what its owning call left; no call of the backward is left unplaced."""
        for p, (want, c) in self.grad_of.items():
            self.name("what %s left for %s" % (c, self.pname[p]), want)
        for n, p in params:
            assert p in self.grad_of, "wiring: no call of the table produces the gradient of %s" % n
            want, c = self.grad_of[p]
            if not _eqflat(p.grad, want):
                rows = torch.nonzero((p.grad.reshape(want.shape[0], -1) != want.reshape(want.shape[0], -1)).any(1)).flatten()
                raise AssertionError("wiring: the final .grad of %s is not what %s left for it (%d of %d rows differ, the first %d); %s" % (
                    n, c, rows.numel(), want.shape[0], int(rows[0]), self.identify(p.grad)))
        stray = [c for c in self.calls if c.index not in self.seen and c.name not in skip]
        assert not stray, "wiring: calls the table has no place for: %s" % ", ".join(str(c) for c in stray[:4])
        return len(self.seen)


def audit_decoder(calls, model, S, dset, d_eps, keep_mask=None):
    """DecoderTrainStep.backward (Compressor.sample differentiated, Network.py:251-268).  S: the forward's saved dict as it was before the
    backward; dset: what backward() was given; d_eps: what it returned.  -> number of calls placed."""
    from ldt_amd.compressor_train import decoder_parameters
    W = Table(calls, model)
    W.name_saved(S)
    dX = W.output_conv(model, dset, S)
    for j in reversed(range(model.n_layers)):                            # the order of reversed(self.decoder), backwards
        dX, _ = W.decoder_level(model, S, j, dX, d_eps)
    W.prior_rows(model, S, dX, keep_mask)
    return W.finish(decoder_parameters(model))


def audit_topdown(calls, model, S, dset, kl_scale, d_eps, d_enc_out, keep_mask=None):
    """TopDownTrainStep.backward (Compressor.top_down differentiated, Network.py:208-233, 61-78, 12-29): per level, backwards, the decoder
    block, the draw with its KL term, the `prior` head, the posterior block `att` and its K / V source."""
    from ldt_amd.compressor_train import topdown_parameters
    from ldt_amd.layers import conv_w
    m = model
    W = Table(calls, m)
    L, C, H = m.n_layers, m.hidden_dim, m.num_heads
    B, N, T = S["B"], S["N"], S["T"]
    assert len(d_enc_out) == L, "wiring: %d encoder-output gradients for %d levels" % (len(d_enc_out), L)
    W.name_saved(S)
    dX = W.output_conv(m, dset, S)
    for j in reversed(range(L)):
        d, pb = m.decoder[L - 1 - j], S["post"][j]
        what = "posterior level %d (decoder.%d.att)" % (j, L - 1 - j)
        dX, dej = W.decoder_level(m, S, j, dX, d_eps)                    # (its first call reads dX AFTER level j + 1's add: linked there)
        # eps_j = mu + exp(clamp(logvar) / 2) noise, and kl_scale * kl                                 (Network.py:26-29, 219-224)
        rk = W.find("reparam_kl_bwd", lambda c: _eq(c.arg("d_eps"), dej), "reads the d_eps slice decoder level %d just wrote" % j)
        r, de = rk.args["d_eps"], d_eps.view(B * T, -1)[:, m.z_dim * j: m.z_dim * (j + 1)]
        assert (r.storage, r.offset, r.shape, r.stride) == layout(de), "wiring: %s: d_eps must be columns [%d z, %d z) of the d_eps buffer itself" % (rk, j, j + 1)
        W.link(rk, "post", pb["post"], "the saved (mu | logvar) of level %d" % j)
        W.link(rk, "noise", pb["noise"], "the posterior noise of level %d" % j)
        W.link(rk, "kl_scale", kl_scale, "the kl_scale given to backward()")
        W.link(rk, "lo", m.min_sigma, "min_sigma")
        W.link(rk, "hi", 10., "10")
        dpost = W.name("dpost of level %d" % j, rk.out())
        # (mu | logvar) = prior.1(SiLU(x3))                                                             (Network.py:76)
        lin = d.prior[1]
        sg = W.find("sgemm", lambda c: _eq(c.arg("a"), dpost) and _eq(c.arg("w"), _tr(conv_w(lin).detach().float())), "carries dpost of level %d through prior.1's weights, transposed" % j)
        si = W.find("silu_bwd", lambda c: _eq(c.arg("dy"), sg.result()), "reads the gradient of SiLU(x3) of level %d" % j)
        W.link(si, "c", pb["x3"], "the saved posterior-block output x3 of level %d" % j)
        W.link(si, "want_act", True, "True")
        W.linear(lin, dpost, si.out(1), "prior.1 of level %d (its input: SiLU(x3) from silu_bwd)" % j)
        dXp = W.name("dXp of level %d at the posterior block's output" % j, si.out(0))
        nk = T if j == 0 else N
        dXp, dkv = W.nocond_block(d.att, pb, dXp, B, H, T, nk, "attention_bwd_cross" if j == 0 else "attention_bwd_wide", what)
        # K / V from the RAW source (quirk Q2): level 0 the tokens themselves, level j >= 1 the set stream o_j                (Network.py:61-78)
        W.linear(d.att.fc_kv, dkv, pb["y"], "fc_kv of %s" % what)
        dy = W.dgrad(d.att.fc_kv, dkv, W.epi_f32, "fc_kv of %s" % what)
        if j == 0:
            ad = W.find("add_f32", lambda c: _eq(c.arg("b"), dy) and _eq(c.arg("a"), dXp), "adds the K / V-source gradient of level 0 to dXp (att(x, x))")
            dXp = W.name("dXp of level 0 after the add", ad.result())
        else:
            ad = W.find("add_f32", lambda c: _eq(c.arg("b"), dy) and _eq(c.arg("a"), dX),
                        "adds the K / V-source gradient of level %d to the SET stream's dX (att(x, o_%d)) before decoder level %d runs backward" % (j, j, j - 1))
            dX = W.name("dX after the add of level %d" % j, ad.result())
        W.alias(ad, "out", "a", "the stream gradient is accumulated in place")
        got = d_enc_out[L - 1 - j]
        if not _eqflat(got, dXp):
            raise AssertionError("wiring: d_enc_out[%d] must be level %d's final dXp; %s" % (L - 1 - j, j, W.identify(got)))
    W.prior_rows(m, S, dX, keep_mask)
    return W.finish(topdown_parameters(m))


def audit_encoder(calls, model, S, d_enc_out, d_tokens, d_pos):
    """EncoderTrainStep.backward (Network.py:200-205, 41-45; layers.py:210-219 with y = the raw x, 240-246, 103-107): the Score table's block
    with K / V from the raw stream, the FinalLayer's gradient added to the running stream gradient, the conditioning linear, ActNorm."""
    from ldt_amd.compressor_train import encoder_parameters
    m = model
    W = Table(calls, m)
    B, T = S["B"], S["T"]
    C, H, L, E = m.hidden_dim, m.num_heads, m.n_layers, m.encoder_layers
    M, mod = B * T, S["mod"]
    n_mod = L * (6 * E + 2) * C
    assert tuple(mod.shape) == (B, n_mod)
    first = [c for c in calls if c.name == "layernorm_modulate_bwd" and "dshift" in c.inplace]
    assert first, "wiring: no layernorm_modulate_bwd call writes a dshift"
    st0 = first[0].inplace["dshift"]["before"].storage
    assert all(c.inplace[k]["before"].storage == st0 for c in calls if c.name != "actnorm_bwd" for k in ("dshift", "dscale", "dgate") if k in c.inplace), \
        "wiring: the modulation-row gradients go to more than one buffer"
    view = lambda off: (st0, off, (B, C), (n_mod, 1))                    # a [B, C] column block of dmod
    col = lambda off: mod[:, off:off + C].contiguous()
    blocks = {}                                                          # column block of dmod -> what its owning call left
    for k in range(n_mod // C):
        W.name("mod columns [%d C, %d C)" % (k, k + 1), col(k * C))
    sample = lambda c, arg: (W.link(c, "rows_per_sample", T, "T = %d" % T), W.link(c, arg, n_mod, "n_mod = %d" % n_mod))

    def mod_ln(off, x, dy, dx_in, what):
        c = W.dest("layernorm_modulate_bwd", "dshift", view(off), "dmod columns [%d C, %d C): dshift of %s" % (off // C, off // C + 1, what))
        r = c.inplace.get("dscale", {}).get("before")
        assert r is not None and (r.storage, r.offset, r.shape, r.stride) == view(off + C), "wiring: %s: dscale of %s must be dmod columns [%d C, %d C)" % (c, what, off // C + 1, off // C + 2)
        W.link(c, "x", x, "the forward's input of %s" % what)
        W.link(c, "dy", dy, "the gradient of the modulated output of %s" % what)
        W.link(c, "scale", col(off + C), "mod columns [%d C, %d C): the scale of %s" % (off // C + 1, off // C + 2, what))
        sample(c, "mod_sample_stride")
        if not _eq(c.before("dx"), dx_in):
            raise AssertionError("wiring: %s: dx must come in as the running stream gradient (%s); %s" % (c, what, W.identify(c.before("dx"))))
        blocks[off // C], blocks[off // C + 1] = c.after("dshift"), c.after("dscale")
        return W.name("dX after %s" % what, c.after("dx"))

    def gate(off, dX, a_saved, what):
        c = W.dest("gate_residual_bwd", "dgate", view(off), "dmod columns [%d C, %d C): dgate of %s" % (off // C, off // C + 1, what))
        W.link(c, "dy", dX, "the stream gradient at the output of %s" % what)
        W.link(c, "gate", col(off), "mod columns [%d C, %d C): the gate of %s" % (off // C, off // C + 1, what))
        W.link(c, "a", a_saved, "the forward's output of %s before the gate" % what)
        sample(c, "gate_sample_stride")
        blocks[off // C] = c.after("dgate")
        return W.name("gated gradient of %s" % what, c.out(0))

    dX = W.name("zeros", torch.zeros_like(S["stages"][0]["xf"]))
    for i in reversed(range(L)):
        enc, st, base = m.encoder[i], S["stages"][i], i * (6 * E + 2) * C
        # enc_out[i] = conv_out.ln(modulate(LN(x))), and x runs on into stage i + 1                     (Network.py:41-45, layers.py:240-246)
        d2 = W.name("d_enc_out[%d]" % i, d_enc_out[i].detach().float().contiguous().view(M, C))
        W.name("xf of stage %d (saved forward)" % i, st["xf"])
        W.linear(enc.conv_out.ln, d2, st["hf"], "conv_out.ln of stage %d" % i)
        dhf = W.dgrad(enc.conv_out.ln, d2, W.epi_f32, "conv_out.ln of stage %d" % i)
        dX = mod_ln(base + 6 * E * C, st["xf"], dhf, dX, "the FinalLayer of stage %d" % i)
        for k in reversed(range(E)):
            blk, sb, m0 = enc.atts[k], st["blocks"][k], base + 6 * k * C
            what = "block %d of stage %d" % (k, i)
            for key, t in sb.items():
                W.name("%s of %s (saved forward)" % (key, what), t)
            da2 = gate(m0 + 5 * C, dX, sb["a2"], "the MLP branch of %s" % what)
            W.linear(blk.mlp.out, da2, sb["ug"], "mlp.out of %s" % what)
            dug = W.dgrad(blk.mlp.out, da2, W.epi_f32, "mlp.out of %s" % what)
            ge = W.find("gelu_bwd", lambda c: _eq(c.arg("dh"), dug), "reads the gradient of GELU's output in %s" % what)
            W.link(ge, "u", sb["u"], "the saved MLP pre-activation u of %s" % what)
            du = W.name("gradient of u, %s" % what, ge.result())
            W.linear(blk.mlp.fc[0][0], du, sb["h2"], "mlp.fc of %s" % what)
            dh2 = W.dgrad(blk.mlp.fc[0][0], du, W.epi_f32, "mlp.fc of %s" % what)
            dX = mod_ln(m0 + 3 * C, sb["x2"], dh2, dX, "norm2 of %s" % what)
            da1 = gate(m0 + 2 * C, dX, sb["a1"], "the attention branch of %s" % what)
            W.linear(blk.fc_o, da1, sb["o"], "fc_o of %s (the raw [B][H][T][32] O read as (M, C), quirk Q1)" % what, flat_x=True)
            do = W.dgrad(blk.fc_o, da1, W.epi_bf16, "fc_o of %s" % what)
            dq, dkv = W.attention("attention_bwd_cross", sb, do, B, H, T, T, what)
            W.linear(blk.fc_q, dq, sb["h"], "fc_q of %s" % what)
            dh = W.dgrad(blk.fc_q, dq, W.epi_f32, "fc_q of %s" % what)
            W.linear(blk.fc_kv, dkv, sb["y"], "fc_kv of %s (K / V from the raw y = bf16(x1), quirk Q2)" % what)
            dy = W.dgrad(blk.fc_kv, dkv, W.epi_f32, "fc_kv of %s" % what)
            dX = mod_ln(m0, sb["x1"], dh, dX, "norm1 of %s" % what)
            ad = W.find("add_f32", lambda c: _eq(c.arg("b"), dy) and _eq(c.arg("a"), dX), "adds fc_kv's dgrad of %s to dX AFTER norm1's backward" % what)
            W.alias(ad, "out", "a", "the stream gradient is accumulated in place")
            dX = W.name("dX at the input of %s" % what, ad.result())
    # the conditioning rows: mod = adaLN.1(SiLU(pos)) for every block and FinalLayer                    (layers.py:214, 238)
    assert sorted(blocks) == list(range(n_mod // C)), "wiring: dmod column blocks %s are never written" % sorted(set(range(n_mod // C)) - set(blocks))
    dmod = W.name("dmod", torch.cat([blocks[k] for k in range(n_mod // C)], 1))
    lins = [lin for e in m.encoder for lin in [a.adaLN[1] for a in e.atts] + [e.conv_out.adaLN[1]]]
    w_ada = torch.cat([lin.weight.detach().float() for lin in lins], 0)
    sg = W.find("sgemm", lambda c: _eq(c.arg("w"), _tr(w_ada)), "multiplies by the stacked adaLN weights, transposed")
    W.link(sg, "a", dmod, "dmod, every column block as the call that owns it left it")
    si = W.find("silu_bwd", lambda c: _eq(c.arg("dy"), sg.result()), "reads the gradient of SiLU(pos)")
    W.link(si, "c", S["pos"], "the position condition")
    sw = W.find("sgemm", lambda c: _eq(c.arg("w"), _tr(si.out(1))) and c.arg("a").shape[0] == n_mod, "forms the stacked adaLN weight gradient from SiLU(pos)")
    W.link(sw, "a", _tr(dmod), "dmod transposed")
    cb = W.find("colsum", lambda c: _eq(c.arg("dy"), dmod), "sums dmod over the samples (the stacked adaLN bias gradient)")
    r = 0
    for lin in lins:                                                     # block k of stage i owns rows [i (6 E + 2) C + 6 k C, + 6 C), its FinalLayer the 2 C after the blocks
        n = lin.weight.shape[0]
        W.own(lin.weight, sw.result()[r:r + n], sw)
        W.own(lin.bias, cb.result()[r:r + n], cb)
        r += n
    if not _eqflat(d_pos, si.out(0)):
        raise AssertionError("wiring: d_pos must be silu_bwd's gradient of pos; %s" % W.identify(d_pos))
    if m.ActNorm is not None:                                            # z = (x - shift) exp(-log_scale)                  (layers.py:103-107)
        ci = m.conv_in
        an = W.find("actnorm_bwd", lambda c: True, "runs ActNorm backwards")
        W.link(an, "dz", dX, "the stream gradient at the first block's input", flat=True)
        W.link(an, "z", S["stages"][0]["blocks"][0]["x1"] if E else S["stages"][0]["xf"], "the first block's saved x1 = ActNorm's OUTPUT z", flat=True)
        W.link(an, "log_scale", ci.log_scale.detach().float().reshape(-1), "the parameter log_scale")
        W.link(an, "B", M * C // ci.shift.numel(), "samples of %d values" % ci.shift.numel())
        W.alias(an, "dx", "dz", "ActNorm's backward runs in place")
        for arg, p in (("dshift", ci.shift), ("dlog_scale", ci.log_scale)):
            r = an.inplace.get(arg, {}).get("before")
            assert r is not None and (r.storage, r.offset, r.shape, r.stride) == layout(p.grad.view(-1)), "wiring: %s: `%s` must be the .grad of %s" % (an, arg, W.pname[p])
            W.own(p, an.after(arg), an)
        dX = W.name("dX after ActNorm's backward", an.after("dx"))
    if not _eqflat(d_tokens, dX):
        raise AssertionError("wiring: d_tokens must be dX after the last call that writes it; %s" % W.identify(d_tokens))
    return W.finish(encoder_parameters(m))


# ------------------------------------------------------------------------------------------------------------- counts
def expected_counts(step, L, E=0, actnorm=False):
    """Calls per kind on a backward's tape, from the number of levels / stages L and of blocks per stage E."""
    if step == "encoder":
        n = L * (1 + 5 * E)
        return {"wgrad": n, "colsum": n + 1, "dgrad": n, "transpose_cast_bf16": n, "cast_pad_bf16": L, "layernorm_modulate_bwd": L * (1 + 2 * E),
                "gate_residual_bwd": 2 * L * E, "gelu_bwd": L * E, "attention_bwd_cross": L * E, "add_f32": L * E, "sgemm": 2, "silu_bwd": 1,
                "actnorm_bwd": int(actnorm)}
    c = {"wgrad": 1 + 4 * L, "colsum": 1 + 5 * L, "dgrad": 4 * L, "transpose_cast_bf16": 4 * L, "cast_pad_bf16": 2 * L, "gelu_bwd": L,
         "layernorm_modulate_bwd": 2 * L, "add_f32": 2 * L, "attention_bwd_long": L, "widen_bf16": L, "sgemm": 1 + 5 * L, "rows_gather_sum": 1}
    if step == "topdown":
        for k, v in {"wgrad": 6 * L, "colsum": 6 * L, "dgrad": 5 * L, "transpose_cast_bf16": 5 * L, "cast_pad_bf16": 2 * L, "gelu_bwd": L,
                     "layernorm_modulate_bwd": 2 * L, "add_f32": 3 * L, "sgemm": L, "reparam_kl_bwd": L, "silu_bwd": L,
                     "attention_bwd_wide": L - 1, "attention_bwd_cross": 1}.items():
            c[k] = c.get(k, 0) + v
    return c


def assert_counts(calls, want, what):
    got = {}
    for c in calls:
        got[c.name] = got.get(c.name, 0) + 1
    want = {k: v for k, v in want.items() if v}
    assert got == want, "%s: calls per kind %s, expected %s" % (what, sorted(got.items()), sorted(want.items()))


# ------------------------------------------------------------------------------------------------------------- cases
# the smallest shapes that still split a tile or a chunk (head width 32 throughout)
CASES = {
    # N = 296 of 320 prior rows under a keep mask with one row no sample keeps: two 256-chunks of attention_bwd_long / _wide, the second
    # partial; M = 592: a partial last K-tile in every wgrad; T = 24: a partial 16-row block
    "ragged": dict(hidden=128, heads=4, levels=2, enc_layers=2, z=20, T=24, B=2, N=296, rows=320, p_dim=40, actnorm=True),
    # the scalar forms (z = 5, ldd = 15, sgemm at K = 6); one chunk; a middle level; ActNorm per channel ("set")
    "odd": dict(hidden=64, heads=2, levels=3, enc_layers=1, z=5, T=8, B=3, N=40, rows=40, p_dim=32, actnorm="set"),
    "odd-enc": dict(hidden=64, heads=2, levels=3, enc_layers=1, z=5, T=40, B=3, N=40, rows=40, p_dim=32, actnorm="set"),
    "odd-enc-plain": dict(hidden=64, heads=2, levels=3, enc_layers=1, z=5, T=40, B=3, N=40, rows=40, p_dim=32, actnorm=None),
}
KL_WEIGHT = 2.0                                                         # tests/golden/topdown_train_tiny.npz's


def make_case(ccfg, hidden, heads, levels, enc_layers, z, T, B, N, rows, p_dim, actnorm, seed=5, min_sigma=None):
    """-> dict: a seeded Compressor(cfg).init() on the CPU with the norms' gamma / beta and ActNorm perturbed, its state_dict copy, and
    seeded inputs of all three steps."""
    import ldt_amd
    c = copy.deepcopy(ccfg)
    c.hidden_dim, c.num_heads, c.n_layers, c.encoder_layers, c.z_dim, c.z_scales = hidden, heads, levels, enc_layers, z, T
    c.max_outputs, c.outsize, c.p_dim, c.ActNorm = rows, N, p_dim, actnorm
    if min_sigma is not None:
        c.min_sigma = min_sigma
    torch.manual_seed(seed)
    model = ldt_amd.Compressor(c)
    model.init()
    with torch.no_grad():                                                # away from the default init's gamma = 1, beta = 0
        for n, p in model.named_parameters():
            if ".norm1." in n or ".norm2." in n:
                p.add_(0.2 * torch.randn(p.shape))
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if actnorm is not None:
        ec.perturb_actnorm(init, seed=78)
        model.load_state_dict(init)
    g = torch.Generator().manual_seed(seed + 4)
    r = dict(model=model, init=init, cfg=c, B=B, N=N, T=T)
    r["eps"] = torch.randn(B, T, levels * z, generator=g)
    r["enc_out"] = [torch.randn(B, T, hidden, generator=g) for _ in range(levels)]
    r["post_noise"] = [torch.randn(B, T, z, generator=g) for _ in range(levels)]
    r["target"] = torch.randn(B, 56, 3, generator=g) * 0.5               # a target of another length than the set
    r["tokens"] = torch.randn(B, T, hidden, generator=g) * 1.3 + 0.2
    r["pos"] = torch.randn(B, p_dim, generator=g)
    r["d_enc"] = [torch.randn(B, T, hidden, generator=g) * 0.05 for _ in range(levels)]
    r["d_set"] = torch.randn(B, N, 3, generator=g) * 0.005          # (a Chamfer gradient's size: ~1 / (B N) per point)
    keep = None
    if N != rows:
        keep = torch.stack([torch.randperm(rows, generator=g) < N for _ in range(B)])
        keep[:, 17] = False                                              # a row no sample keeps (put one back per sample that lost one)
        for b in range(B):
            spare = torch.nonzero(~keep[b]).flatten()
            spare = spare[spare != 17]
            keep[b, spare[:N - int(keep[b].sum())]] = True
        assert bool((keep.sum(1) == N).all()) and not bool(keep[:, 17].any())
    r["keep"] = keep
    r["kl_scale"] = KL_WEIGHT / (levels * B * z * T)
    return r


def copy_saved(S):
    """The audit's own deep copy of a step's saved dict (the backward is handed the original and writes into some of it)."""
    if torch.is_tensor(S):
        return S.clone()
    if isinstance(S, dict):
        return {k: copy_saved(v) for k, v in S.items()}
    if isinstance(S, (list, tuple)):
        return type(S)(copy_saved(v) for v in S)
    return S


def centred_groups(model, S, step):
    """The blocks of a saved dict whose backward reads centred keys -> the groups of audit_centred."""
    from ldt_amd.layers import conv_w
    C = model.hidden_dim
    panel = lambda blk: kc.cast_pad_want(conv_w(blk.fc_kv).detach().float()[:C].contiguous(), kc.pad64(C))
    b_k = lambda blk: blk.fc_kv.bias.detach().float()[:C].contiguous()
    out = []
    if step == "topdown":
        L = model.n_layers
        for j, pb in enumerate(S["post"]):
            blk = model.decoder[L - 1 - j].att
            out.append(dict(y=pb["y"], kv=pb["kv"], w_k=panel(blk), b_k=b_k(blk), B=S["B"], nk=S["T"] if j == 0 else S["N"], what="the posterior block of level %d" % j))
    else:
        for i, st in enumerate(S["stages"]):
            for k, sb in enumerate(st["blocks"]):
                blk = model.encoder[i].atts[k]
                out.append(dict(y=sb["y"], kv=sb["kv"], w_k=panel(blk), b_k=b_k(blk), B=S["B"], nk=S["T"], what="block %d of stage %d" % (k, i)))
    return out
