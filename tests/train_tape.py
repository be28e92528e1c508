"""A call tape for `ScoreTrainStep` and the audit of a whole backward read from it (a plain helper module: test_gpu_train_tape.py runs it on the
MI355X, test_train_tape_host.py on a pure-torch emulation of the entry points, planted faults included).

`ldt_amd.train` reaches every kernel through its module attribute `ops`, which it also hands to the block of `ldt_amd.train_block`
(`install_ops` replaces the attribute on all the step modules at once).  `Tape(ops)` forwards every attribute and records, for each call made
through it, the function name, its operands (cloned, with their shapes, strides and dtypes) and its outputs (cloned); for operands written in
place (`out=`, `dx`, `dshift=`, `dscale=`, `dgate=`, and the Compressor entry points' `dq_out=`, `dkv_out=`, `dlog_scale=`, `stats_out=`:
the `.grad` views and the column blocks of `dmod` among them) the view AND the whole storage under it, before and after the call.

Two audits read the tape of a backward:
  * `audit_numeric`: every call's output against float64 computed from that call's OWN recorded operands, with the references and bounds of
    kernel_checks.py that test_gpu_train_kernels.py holds each kernel to alone (teacher forcing: the depth of the network never enters a
    bound); in-place accumulations as after - before; around every destination, the storage outside the view unchanged bit for bit.
  * `audit_wiring`: what each call's operands MUST be, written down below from the reference's block (model/layers.py:183-229,
    model/scorenet/score.py:110-151) and not from train.py, each link checked with torch.equal between the recorded operand and the recorded
    output of its producer (or a saved forward tensor, a parameter, a column block of the modulation rows); and every parameter's final `.grad`
    equal to the recorded output of the call the table names for it.
Calls are found by what they write or read (a destination in `dmod` or in a `.grad`, an operand bit-equal to a producer's output), never by
their position: a different order of independent branches passes."""
import inspect

import torch

import kernel_checks as kc

INPLACE = ("out", "dx", "dshift", "dscale", "dgate",
           "dq_out", "dkv_out", "dlog_scale", "stats_out",      # the Compressor steps' entry points (tests/compressor_tape.py)
           "x_bf16_out")                                        # the inference forwards' (tests/infer_tape.py): no training step passes one;
#                                                                 `resid` where it aliases `out` is held through `out`'s before / after
PLAIN = ("pad64", "stream_ptr")                      # no tensors: forwarded unrecorded
WRITES = {"attention_oproj_resid_": "x"}             # a `..._` entry point whose in-place operand is not its first (inference only)


def _epilogues():
    from ldt_amd import _lib
    return _lib.EPI_BF16, _lib.EPI_F32


class Rec:
    """A tensor operand as it was at one moment: a contiguous clone plus the layout it had."""
    __slots__ = ("value", "shape", "stride", "dtype", "offset", "storage")

    def __init__(self, t):
        self.value = t.detach().clone(memory_format=torch.contiguous_format)
        self.shape, self.stride, self.dtype, self.offset = tuple(t.shape), tuple(t.stride()), t.dtype, t.storage_offset()
        self.storage = t.untyped_storage().data_ptr()


def _whole_storage(t):
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage()).clone()


def _snap(v):
    if torch.is_tensor(v):
        return Rec(v)
    if isinstance(v, (tuple, list)):
        return type(v)(_snap(x) for x in v)
    if isinstance(v, dict):                              # ln_mlp_resid_'s `next_linear` (inference only)
        return {k: _snap(x) for k, x in v.items()}
    return v


class Call:
    def __init__(self, index, name, args):
        self.index, self.name, self.args = index, name, args     # args: {parameter name: Rec | plain value}
        self.outs, self.inplace = [], {}                           # inplace: {name: dict(before, after: Rec, base_before, base_after: flat storage)}

    def arg(self, name):
        v = self.args.get(name)
        return v.value if isinstance(v, Rec) else v

    def out(self, i=0):
        """Output i as returned; for a call that wrote into `out=` the view after the call."""
        return self.outs[i].value if self.outs[i] is not None else None

    def after(self, name):
        return self.inplace[name]["after"].value

    def before(self, name):
        return self.inplace[name]["before"].value

    def result(self):
        return self.after("out") if "out" in self.inplace else self.out(0)

    def __str__(self):
        shapes = ", ".join("%s%s" % (k, list(v.shape)) for k, v in self.args.items() if isinstance(v, Rec))
        return "call #%d %s(%s)" % (self.index, self.name, shapes)


class Tape:
    """Proxy of an `ops` module: forwards every attribute, records every call (see the module docstring)."""

    def __init__(self, ops):
        self._ops, self.calls, self.marks = ops, [], {}

    def mark(self, name):
        self.marks[name] = len(self.calls)

    def since(self, name):
        return self.calls[self.marks[name]:]

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if not callable(fn) or name in PLAIN or isinstance(fn, type):
            return fn
        sig = inspect.signature(fn)

        def recorded(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            call = Call(len(self.calls), name, {k: _snap(v) for k, v in bound.arguments.items()})
            dest = {k: v for k, v in bound.arguments.items() if k in INPLACE and torch.is_tensor(v)}
            if name.endswith("_"):
                first = WRITES.get(name) or next(iter(bound.arguments))
                dest[first] = bound.arguments[first]
            for k, v in dest.items():
                call.inplace[k] = {"before": call.args[k], "base_before": _whole_storage(v)}
            self.calls.append(call)
            ret = fn(*a, **kw)
            for k, v in dest.items():
                call.inplace[k].update(after=Rec(v), base_after=_whole_storage(v))
            call.outs = [None if r is None else Rec(r) for r in (ret if isinstance(ret, (tuple, list)) else (ret,))]
            return ret
        return recorded


# ------------------------------------------------------------------------------------------------------------- driving a step
def install_ops(mp, proxy):
    """`proxy` as the module attribute `ops` of every module a training step reaches its kernels through, in the MonkeyPatch context `mp`:
    ldt_amd.train, ldt_amd.compressor_train and ldt_amd.train_block, which holds the block they share.  A step hands its own module's `ops`
    to the block (`TrainBlock(ops)`); train_block's attribute is what a TrainBlock built without one falls back to, so no path is left out."""
    import importlib
    for name in ("train", "compressor_train", "train_block"):
        mp.setattr(importlib.import_module("ldt_amd." + name), "ops", proxy)


def install_infer_ops(mp, proxy):
    """`proxy` as the module attribute `ops` of the two modules the inference forwards (`Compressor.forward`, `Compressor.sample`) reach their
    kernels through: ldt_amd.compressor and ldt_amd.blocks (tests/infer_tape.py)."""
    import importlib
    for name in ("compressor", "blocks"):
        mp.setattr(importlib.import_module("ldt_amd." + name), "ops", proxy)


def flat_grads(model):
    """Zeroed `.grad` views of one flat fp32 buffer for every parameter, the way AdamEMA._ensure_flat lays them out (16-byte aligned views in
    parameter order).  On the GPU this IS AdamEMA (zero_grad()); on the CPU, where AdamEMA refuses, the same layout by hand.  -> the flat buffer."""
    params = list(model.parameters())
    if params[0].is_cuda:
        from ldt_amd.train import AdamEMA
        opt = AdamEMA(params, lr=1e-3)
        opt.zero_grad()
        model._tape_opt = opt                          # keeps the flat buffers alive with the model
        return opt.flat_grad
    n = sum((p.numel() + 3) // 4 * 4 for p in params)
    flat, o = torch.zeros(n), 0
    for p in params:
        p.grad = flat[o:o + p.numel()].view(p.shape)
        o += (p.numel() + 3) // 4 * 4
    return flat


# ------------------------------------------------------------------------------------------------------------- numeric audit
def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.int8}[t.element_size()])


def check_untouched(call):
    """Around the destinations of `call`: the storage outside the views it was given to write is the same bits before and after."""
    groups = {}
    for name, d in call.inplace.items():
        assert d["after"].storage == d["before"].storage and d["base_before"].numel() == d["base_after"].numel(), "%s: `%s` was re-allocated by the call" % (call, name)
        groups.setdefault((d["before"].storage, d["before"].dtype), []).append((name, d))
    for dests in groups.values():                                           # (dshift and dscale are two views of one buffer)
        b0, b1 = dests[0][1]["base_before"], dests[0][1]["base_after"]
        inside = torch.zeros(b0.numel(), dtype=torch.bool, device=b0.device)
        for _, d in dests:
            r = d["before"]
            inside[torch.arange(b0.numel(), device=b0.device).as_strided(r.shape, r.stride, r.offset).reshape(-1)] = True
        changed = (_bits(b0) != _bits(b1)) & ~inside
        if bool(changed.any()):
            where = torch.nonzero(changed).flatten()
            raise AssertionError("%s: %d element(s) outside the destination view(s) %s changed, the first at storage element %d" % (
                call, where.numel(), ", ".join("`%s` (offset %d, shape %s, strides %s)" % (n, d["before"].offset, list(d["before"].shape),
                                                                                          list(d["before"].stride)) for n, d in dests), int(where[0])))


def _heads(z, B, N, H):
    return z.reshape(B, N, H, 64).permute(0, 2, 1, 3)


def check_call(call):
    """One call against float64 from its own recorded operands.  -> {what: err / tol} (empty for a call kind that is exact or not a backward kernel)."""
    a, nm = call.arg, call.name
    E = kc.assert_elementwise
    epi_bf16, _ = _epilogues()
    if nm == "dsm_loss_bwd":
        ref, tol = kc.dsm_loss_bwd_ref(a("eta"), a("params"), a("weight"), a("l1"))
        return {nm: E(call.out(), ref, tol, str(call))}
    if nm == "cast_pad_bf16":
        src = a("src").reshape(-1, a("src").shape[-1])
        assert torch.equal(call.result(), kc.cast_pad_want(src, a("cols_pad") or (src.shape[1] + 3) // 4 * 4)), "%s: not bf16(src), zero padded" % call
        return {nm: 0.0}
    if nm == "transpose_cast_bf16":
        assert torch.equal(call.result(), kc.transpose_cast_want(a("src"), a("rows_pad"))), "%s: not bf16(src)^T, zero padded" % call
        return {nm: 0.0}
    if nm == "colsum":
        ref, tol = kc.colsum_ref(a("dy"))
        return {nm: E(call.result(), ref, tol, str(call))}
    if nm == "wgrad":
        ref, tol = kc.wgrad_ref(a("dy"), a("x"))
        return {nm: E(call.result(), ref, tol, str(call))}
    if nm == "dgrad":
        bf16 = a("epilogue") == epi_bf16
        ref, tol = kc.dgrad_ref(a("dy"), a("w_t"), torch.bfloat16 if bf16 else torch.float32)
        return {"dgrad bf16" if bf16 else "dgrad fp32": E(call.result(), ref, tol, str(call))}
    if nm == "sgemm":
        if a("act_in") or a("act_out"):
            return {}
        ref, tol = kc.sgemm_ref(a("a"), a("w"), a("bias"))
        return {nm: E(call.result(), ref, tol, str(call))}
    if nm == "layernorm_modulate_bwd":
        # dx is accumulated into: after - before against the added term; the bound's 2^-24 |after| for the add is layernorm_modulate_bwd_ref's
        # own last term (it is stated on before + term)
        ref, tol, _ = kc.layernorm_modulate_bwd_ref(a("x"), a("dy"), a("scale"), a("rows_per_sample") or a("x").shape[0], call.before("dx"))
        d = call.after("dx").double() - call.before("dx").double()
        r = {"layernorm_modulate_bwd dx": E(d, ref["dx"] - call.before("dx").double(), tol["dx"], "%s, dx after - before" % call)}
        if a("want_mod"):
            got = [call.after(k) if k in call.inplace else call.out(i) for i, k in enumerate(("dshift", "dscale"))]
            r["layernorm_modulate_bwd dshift"] = E(got[0], ref["dshift"], tol["dshift"], "%s, dshift" % call)
            r["layernorm_modulate_bwd dscale"] = E(got[1], ref["dscale"], tol["dscale"], "%s, dscale" % call)
        return r
    if nm == "gate_residual_bwd":
        C = a("dy").shape[1]
        ref, tol = kc.gate_residual_bwd_ref(a("dy"), a("gate").reshape(-1, a("gate").shape[-1])[:, :C], a("a"), a("rows_per_sample") or a("dy").shape[0])
        r = {"gate_residual_bwd da": E(call.after("out") if "out" in call.inplace else call.out(0), ref["da"], tol["da"], "%s, da" % call)}
        if a("a") is not None:
            r["gate_residual_bwd dgate"] = E(call.after("dgate") if "dgate" in call.inplace else call.out(1), ref["dgate"], tol["dgate"], "%s, dgate" % call)
        return r
    if nm == "gelu_bwd":
        ref, tol = kc.gelu_bwd_ref(a("u"), a("dh"))
        return {nm: E(call.result(), ref, tol, str(call))}
    if nm == "silu_bwd":
        ref, tol = kc.silu_bwd_ref(a("c"), a("dy"))
        r = {nm: E(call.out(0), ref["dc"], tol["dc"], str(call))}
        if a("want_act"):
            r["silu_bwd act"] = E(call.out(1), ref["act"], tol["act"], "%s, act" % call)
        return r
    if nm == "embedding_grad":
        ref, tol = kc.embedding_grad_ref(a("dc"), a("label").reshape(-1), a("n_classes"))
        return {nm: E(call.out(), ref, tol, str(call))}
    if nm == "attention_bwd":
        B, H, N = a("B"), a("H"), a("N")
        # o and do: the raw [B][H][N][64] buffers (quirk Q1), whatever shape they were handed over in
        ref, tol = kc.attn_bwd_ref(a("q"), a("k"), a("v"), a("o").reshape(B, H, N, 64), a("do").reshape(B, H, N, 64), B, H, N, N)
        return {"attention_bwd " + k: E(_heads(call.out(i), B, N, H), ref[k], tol[k], "%s, %s" % (call, k)) for i, k in enumerate(("dq", "dk", "dv"))}
    raise AssertionError("%s: a call kind the audit has no reference for" % call)


def audit_numeric(calls, worst=None):
    """Every call of `calls` (the backward's): check_call + check_untouched.  -> {call kind: largest err / tol}."""
    worst = {} if worst is None else worst
    for call in calls:
        check_untouched(call)
        for k, r in check_call(call).items():
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


# ------------------------------------------------------------------------------------------------------------- wiring audit
def _eq(a, b):
    return torch.is_tensor(a) and a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)


def _eqflat(a, b):
    return torch.is_tensor(a) and a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(a.reshape(-1), b.reshape(-1))


def layout(t):
    return t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride())


class Wiring:
    def __init__(self, calls):
        self.calls, self.known, self.seen = calls, [], set()

    def name(self, label, t):
        self.known.append((label, t))
        return t

    def identify(self, t):
        hits = [lb for lb, k in self.known if _eqflat(t, k)]
        return ("it is bit-equal to %s" % " / ".join(hits[:3])) if hits else "it equals no tensor the table knows"

    def find(self, kind, pred, what):
        """The call of `kind` that satisfies pred (what: the sentence for the message)."""
        hits = [c for c in self.calls if c.name == kind and pred(c)]
        if not hits:
            raise AssertionError("wiring: no %s call %s (%d %s calls on the tape: %s)" % (
                kind, what, sum(c.name == kind for c in self.calls), kind, ", ".join("#%d" % c.index for c in self.calls if c.name == kind)[:200]))
        self.seen.add(hits[0].index)
        return hits[0]

    def dest(self, kind, arg, like, what):
        """The call of `kind` whose in-place operand `arg` is exactly the view `like`: a tensor, or its (storage, offset, shape, strides)."""
        sp, off, shape, stride = layout(like) if torch.is_tensor(like) else like

        def pred(c):
            r = c.inplace.get(arg, {}).get("before")
            return r is not None and (r.storage, r.offset, r.shape, r.stride) == (sp, off, shape, stride)
        return self.find(kind, pred, "writes %s (`%s` = storage offset %d, shape %s, strides %s)" % (what, arg, off, list(shape), list(stride)))

    def link(self, call, arg, want, what, flat=False):
        got = call.arg(arg)
        if torch.is_tensor(want):
            ok = _eqflat(got, want) if flat else _eq(got, want)
        else:
            ok = got == want
        if not ok:
            raise AssertionError("wiring: %s: operand `%s` must be %s; %s" % (
                call, arg, what, self.identify(got) if torch.is_tensor(got) else "it is %r, not %r" % (got, want)))


def audit_wiring(calls, model, S, dparams):
    """The table.  calls: the backward's; S: the forward's saved tensors as they were BEFORE the backward (the audit's own copy); dparams: what
    backward() was given.  Checks every link, then every parameter's final .grad.  -> number of calls placed."""
    from ldt_amd.layers import conv_w
    epi_bf16, epi_f32 = _epilogues()
    W = Wiring(calls)
    m = model
    B, T = S["B"], S["T"]
    D, H, nb, n_mod, z = m.hidden_size, m.num_heads, m.num_blocks, m.n_mod, m.z_dim
    M = B * T
    mod = S["mod"]
    col = lambda k: W.name("mod columns [%d D, %d D)" % (k, k + 1), mod[:, k * D:(k + 1) * D].contiguous())
    for k in range(6 * nb + 2):
        col(k)
    for l, sb in enumerate(S["blocks"]):
        for key, t in sb.items():
            W.name("%s of block %d (saved forward)" % (key, l), t)
    for key in ("xf", "hf", "x_in", "c", "a_t", "e_t", "a_l", "e_l"):
        if key in S:
            W.name("%s (saved forward)" % key, S[key])
    grad_of = {}                                                          # parameter -> (recorded output that must be its final .grad, producing call)
    dmod_blocks = {}                                                      # column block of dmod -> recorded output of the call that writes it
    pname = {p: n for n, p in m.named_parameters()}
    sample_args = lambda c, stride_arg: (W.link(c, "rows_per_sample", T, "T = %d" % T), W.link(c, stride_arg, n_mod, "n_mod = %d" % n_mod))

    def linear(layer, dy, x, what, flat_x=False):
        """dW = dy^T x into the layer's weight .grad (all its rows), db = column sums of dy into the bias .grad."""
        cw = W.dest("wgrad", "out", layer.weight.grad.view(layer.weight.shape[0], -1), "the .grad of %s" % pname[layer.weight])
        W.link(cw, "dy", dy, "the gradient of the output of %s" % what)
        W.link(cw, "x", x, "the forward's input of %s" % what, flat=flat_x)
        grad_of[layer.weight] = (cw.after("out"), cw)
        cb = W.dest("colsum", "out", layer.bias.grad, "the .grad of %s" % pname[layer.bias])
        W.link(cb, "dy", dy, "the gradient of the output of %s" % what)
        grad_of[layer.bias] = (cb.after("out"), cb)

    def dgrad(w, dy, epilogue, what):
        """dX = dy W through the transposed bf16 panel of the CURRENT weights."""
        w = w.detach()
        want = kc.transpose_cast_want(w)
        tc = W.find("transpose_cast_bf16", lambda c: _eq(c.arg("src"), w.contiguous()) and _eq(c.result(), want), "transposes the weights of %s" % what)
        dg = W.find("dgrad", lambda c: _eq(c.arg("w_t"), tc.result()), "multiplies by the transposed weights of %s" % what)
        W.link(dg, "dy", dy, "the gradient of the output of %s" % what)
        W.link(dg, "epilogue", epilogue, "epilogue %d" % epilogue)
        return W.name("dgrad through %s" % what, dg.result())

    def ln_bwd(k, x, dy, dx_in, what):
        """LayerNorm + modulate backward whose (shift, scale) are column blocks k, k + 1 of the modulation rows."""
        c = W.dest("layernorm_modulate_bwd", "dshift", dmod_view(k), "dmod columns [%d D, %d D): dshift of %s" % (k, k + 1, what))
        r = c.inplace.get("dscale", {}).get("before")
        assert r is not None and r.offset == (k + 1) * D and r.stride == (n_mod, 1), "wiring: %s: dscale of %s must be dmod columns [%d D, %d D)" % (c, what, k + 1, k + 2)
        W.link(c, "x", x, "the forward's input of %s" % what)
        W.link(c, "dy", dy, "the gradient of the modulated output of %s" % what)
        W.link(c, "scale", mod[:, (k + 1) * D:(k + 2) * D].contiguous(), "mod columns [%d D, %d D): the scale of %s" % (k + 1, k + 2, what))
        sample_args(c, "mod_sample_stride")
        if not _eq(c.before("dx"), dx_in):
            raise AssertionError("wiring: %s: dx must come in as the residual-stream gradient so far; %s" % (c, W.identify(c.before("dx"))))
        dmod_blocks[k], dmod_blocks[k + 1] = c.after("dshift"), c.after("dscale")
        return W.name("dX after %s" % what, c.after("dx"))

    def gate_bwd(k, dX, a_saved, what):
        c = W.dest("gate_residual_bwd", "dgate", dmod_view(k), "dmod columns [%d D, %d D): dgate of %s" % (k, k + 1, what))
        W.link(c, "dy", dX, "the residual-stream gradient at the output of %s" % what)
        W.link(c, "gate", mod[:, k * D:(k + 1) * D].contiguous(), "mod columns [%d D, %d D): the gate of %s" % (k, k + 1, what))
        W.link(c, "a", a_saved, "the forward's output of %s before the gate" % what)
        sample_args(c, "gate_sample_stride")
        dmod_blocks[k] = c.after("dgate")
        return W.name("gated gradient of %s" % what, c.out(0))

    # dmod: found as the storage the final layer's dshift goes to; every destination in it is then an offset into that storage
    first = [c for c in calls if c.name == "layernorm_modulate_bwd" and "dshift" in c.inplace]
    assert first, "wiring: no layernorm_modulate_bwd call writes a dshift"
    dmod_storage = first[0].inplace["dshift"]["before"].storage
    assert all(c.inplace[k]["before"].storage == dmod_storage for c in calls for k in ("dshift", "dscale", "dgate") if k in c.inplace), \
        "wiring: the modulation-row gradients go to more than one buffer"

    dmod_view = lambda k: (dmod_storage, k * D, (B, D), (n_mod, 1))          # a [B, D] column block of dmod

    # ---- FinalLayer (layers.py:240-246): out = ln(modulate(norm(xf), shift, scale))
    d2 = W.name("dparams", dparams.contiguous().view(M, z))
    fin = m.ln_out.ln
    linear(fin, d2, S["hf"], "ln_out.ln")
    cp = W.find("cast_pad_bf16", lambda c: _eq(c.arg("src"), d2), "casts dparams to the bf16 operand of the final dgrad")
    dhf = dgrad(conv_w(fin), cp.result(), epi_f32, "ln_out.ln")
    dX = ln_bwd(6 * nb, S["xf"], dhf, torch.zeros_like(S["xf"]), "the final LayerNorm")
    for l in reversed(range(nb)):
        blk, sb, k0 = m.Transformer[l], S["blocks"][l], 6 * l
        # x = x2 + gate_mlp * mlp(modulate(norm2(x2), shift_mlp, scale_mlp))                      (layers.py:219; chunks 3, 4, 5)
        da2 = gate_bwd(k0 + 5, dX, sb["a2"], "the MLP branch of block %d" % l)
        linear(blk.mlp.out, da2, sb["ug"], "mlp.out of block %d" % l)
        dug = dgrad(conv_w(blk.mlp.out), da2, epi_f32, "mlp.out of block %d" % l)
        ge = W.find("gelu_bwd", lambda c: _eq(c.arg("dh"), dug), "reads the gradient of GELU's output in block %d" % l)
        W.link(ge, "u", sb["u"], "the MLP pre-activation u of block %d" % l)
        du = W.name("gradient of u, block %d" % l, ge.result())
        linear(blk.mlp.fc[0][0], du, sb["h2"], "mlp.fc of block %d" % l)
        dh2 = dgrad(conv_w(blk.mlp.fc[0][0]), du, epi_f32, "mlp.fc of block %d" % l)
        dX = ln_bwd(k0 + 3, sb["x2"], dh2, dX, "norm2 of block %d" % l)
        # x2 = x1 + gate_msa * fc_o(attention(fc_q(h), fc_kv(h)))                                 (layers.py:218, 183-200; chunks 0, 1, 2)
        da1 = gate_bwd(k0 + 2, dX, sb["a1"], "the attention branch of block %d" % l)
        linear(blk.fc_o, da1, sb["o"], "fc_o of block %d (the raw [B][H][T][64] buffer read as (M, D), quirk Q1)" % l, flat_x=True)
        do = dgrad(conv_w(blk.fc_o), da1, epi_bf16, "fc_o of block %d" % l)
        at = W.find("attention_bwd", lambda c: _eqflat(c.arg("do"), do), "reads dO = the dgrad of fc_o of block %d as the raw [B][H][T][64] buffer" % l)
        qkv = sb["qkv"]
        for i, nm in enumerate("qkv"):
            W.link(at, nm, qkv[:, i * D:(i + 1) * D].contiguous(), "columns [%d D, %d D) of the saved qkv of block %d" % (i, i + 1, l))
        W.link(at, "o", sb["o"], "the saved attention output of block %d" % l, flat=True)
        for nm, v in (("B", B), ("H", H), ("N", T), ("head_dim", 64)):
            W.link(at, nm, v, "%s = %d" % (nm, v))
        dq, dk, dv = at.out(0), at.out(1), at.out(2)
        dqkv = W.name("[dq | dk | dv] of block %d" % l, torch.cat([dq, dk, dv], 1))
        assert "out" not in at.inplace or _eq(at.after("out"), dqkv), "wiring: %s: dq | dk | dv are not the three column blocks of its `out`" % at
        W.name("[dq | dk] of block %d" % l, torch.cat([dq, dk], 1))
        linear(blk.fc_q, W.name("dq of block %d" % l, dq), sb["h"], "fc_q of block %d" % l)
        linear(blk.fc_kv, W.name("[dk | dv] of block %d" % l, torch.cat([dk, dv], 1)), sb["h"], "fc_kv of block %d" % l)
        dh = dgrad(torch.cat([conv_w(blk.fc_q), conv_w(blk.fc_kv)], 0), dqkv, epi_f32, "fc_q | fc_kv of block %d" % l)
        dX = ln_bwd(k0, sb["x1"], dh, dX, "norm1 of block %d" % l)
    linear(m.ln_in, dX, S["x_in"], "ln_in")                                                      # score.py:110
    # ---- conditioning rows: mod = adaLN(SiLU(c)), c = TimeEmbedding(t) [+ LabelEmbedding(label)]  (layers.py:172, 214, 238; score.py:135)
    assert sorted(dmod_blocks) == list(range(6 * nb + 2)), "wiring: dmod column blocks %s are never written" % sorted(set(range(6 * nb + 2)) - set(dmod_blocks))
    dmod = W.name("dmod", torch.cat([dmod_blocks[k] for k in range(6 * nb + 2)], 1))
    lins = [blk.adaLN[1] for blk in m.Transformer] + [m.ln_out.adaLN[1]]
    w_ada = torch.cat([ln.weight.detach() for ln in lins], 0)
    tr = lambda t: t.t().contiguous()
    sg = W.find("sgemm", lambda c: _eq(c.arg("w"), tr(w_ada)), "multiplies by the stacked adaLN weights, transposed")
    W.link(sg, "a", dmod, "dmod, every column block as the call that owns it left it")
    si = W.find("silu_bwd", lambda c: _eq(c.arg("dy"), sg.result()), "reads the gradient of SiLU(c)")
    W.link(si, "c", S["c"], "the conditioning rows c")
    dc, s_c = W.name("dc", si.out(0)), si.out(1)
    sw = W.find("sgemm", lambda c: _eq(c.arg("w"), tr(s_c)) and c.arg("a").shape[0] == n_mod, "forms the stacked adaLN weight gradient from SiLU(c)")
    W.link(sw, "a", tr(dmod), "dmod transposed")
    cb = W.find("colsum", lambda c: _eq(c.arg("dy"), dmod), "sums dmod over the samples (the stacked adaLN bias gradient)")
    r = 0
    for ln in lins:                                                        # block l owns rows [6 l D, 6 (l + 1) D), the final layer the last 2 D
        n = ln.weight.shape[0]
        grad_of[ln.weight], grad_of[ln.bias] = (sw.result()[r:r + n], sw), (cb.result()[r:r + n], cb)
        r += n

    def mlp2(seq, a_pre, e_in, what):
        """Linear, SiLU, Linear: -> the gradient of the first Linear's output."""
        s1 = W.find("sgemm", lambda c: _eq(c.arg("a"), dc) and _eq(c.arg("w"), tr(seq[2].weight.detach())), "carries dc through the second Linear of %s" % what)
        sl = W.find("silu_bwd", lambda c: _eq(c.arg("dy"), s1.result()), "reads the gradient of the SiLU of %s" % what)
        W.link(sl, "c", a_pre, "the saved pre-activation of %s" % what)
        d_a, s_a = sl.out(0), sl.out(1)
        for lin, dy, x in ((seq[2], dc, s_a), (seq[0], d_a, e_in)):
            c = W.dest("sgemm", "out", lin.weight.grad, "the .grad of %s" % pname[lin.weight])
            W.link(c, "a", tr(dy), "the output gradient, transposed")
            W.link(c, "w", tr(x), "the Linear's input, transposed")
            grad_of[lin.weight] = (c.after("out"), c)
            c = W.dest("colsum", "out", lin.bias.grad, "the .grad of %s" % pname[lin.bias])
            W.link(c, "dy", dy, "the output gradient")
            grad_of[lin.bias] = (c.after("out"), c)
        return d_a

    mlp2(m.TimeEmbedding.mlp, S["a_t"], S["e_t"], "TimeEmbedding")
    if S["label"] is not None:
        le = m.LabelEmbedding
        d_a = mlp2(le.mlp, S["a_l"], S["e_l"], "LabelEmbedding")
        se = W.find("sgemm", lambda c: _eq(c.arg("a"), d_a) and _eq(c.arg("w"), tr(le.mlp[0].weight.detach())), "carries the gradient to the embedding rows")
        eg = W.find("embedding_grad", lambda c: _eq(c.arg("dc"), se.result()), "scatters the gradient of the embedding rows")
        W.link(eg, "label", S["lab"].to(eg.arg("label").dtype).reshape(eg.arg("label").shape), "the labels")
        W.link(eg, "n_classes", le.label_emb.weight.shape[0], "the number of classes")
        grad_of[le.label_emb.weight] = (eg.out(), eg)
    # ---- every parameter's final .grad is what its call left
    for p, (want, c) in grad_of.items():
        W.name("what %s left for %s" % (c, pname[p]), want)
    for n, p in m.named_parameters():
        assert p in grad_of, "wiring: no call of the table produces the gradient of %s" % n
        want, c = grad_of[p]
        if not _eqflat(p.grad, want):
            rows = torch.nonzero((p.grad.reshape(want.shape[0], -1) != want.reshape(want.shape[0], -1)).any(1)).flatten()
            raise AssertionError("wiring: the final .grad of %s is not what %s left for it (%d of %d rows differ, the first %d); %s" % (
                n, c, rows.numel(), want.shape[0], int(rows[0]), W.identify(p.grad)))
    stray = [c for c in calls if c.index not in W.seen and c.name != "dsm_loss_bwd"]
    assert not stray, "wiring: calls the table has no place for: %s" % ", ".join(str(c) for c in stray[:4])
    return len(W.seen)


# ------------------------------------------------------------------------------------------------------------- cases
# hidden / heads / blocks, B x T, classes, labels: the smallest shapes at which these paths can still go wrong (z = 120, t_dim = 64)
CASES = {
    # M = 216 (pad64 -> 256: a partial last K-tile in every wgrad); T = 72 (partial 16-row, 32-column and 64-key steps of the attention
    # backward); H = 4 != T in the Q1 reinterpretation; classes 1 and 3 absent, class 2 twice
    "ragged": dict(hidden=256, heads=4, blocks=2, B=3, T=72, classes=4, labels=[2, 0, 2]),
    "t32": dict(hidden=128, heads=2, blocks=3, B=5, T=32, classes=1, labels=None),      # the shipped token count; n_mod stride 2560, a middle block
    "t256": dict(hidden=128, heads=2, blocks=1, B=2, T=256, classes=1, labels=None),    # the headline token count: M = 512, 16 row blocks per head
    "one": dict(hidden=128, heads=2, blocks=1, B=1, T=40, classes=1, labels=None),      # one sample: rows_per_sample = M < 64
}


def make_case(score_cfg, hidden, heads, blocks, B, T, classes, labels, seed=5):
    """-> (Score on the CPU with seeded default initialisation, x [B, T, z], t [B], label or None, eta [B, T, z])."""
    import copy
    import ldt_amd
    cfg = copy.deepcopy(score_cfg)
    cfg.hidden_size, cfg.num_heads, cfg.num_blocks, cfg.num_categorys, cfg.z_dim, cfg.t_dim = hidden, heads, blocks, classes, 120, 64
    torch.manual_seed(seed)
    model = ldt_amd.Score(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    x, eta = torch.randn(B, T, cfg.z_dim, generator=g), torch.randn(B, T, cfg.z_dim, generator=g)
    t = torch.rand(B, generator=g) * 0.98 + 0.01
    return model, x, t, None if labels is None else torch.tensor(labels), eta


def copy_saved(S):
    """The audit's own copy of ScoreTrainStep.saved (the backward is handed the original)."""
    cp = lambda v: v.clone() if torch.is_tensor(v) else v
    out = {k: cp(v) for k, v in S.items() if k != "blocks"}
    out["blocks"] = [{k: cp(v) for k, v in sb.items()} for sb in S["blocks"]]
    return out
