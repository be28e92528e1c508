"""CPU: the teeth of the whole-backward audit (tests/train_tape.py, run on the MI355X by test_gpu_train_tape.py).

A pure-torch emulation of the `ops` entry points the backward uses (fp32 arithmetic, bf16 where the kernels round, the same signatures) stands
in for the kernels; `ScoreTrainStep.backward` itself — the product's, unchanged — runs on it on the CPU, from a saved-activation dict built with
the oracle's layer functions.  The numeric and the wiring audit must pass on that tape, in both accumulation orders and with the calls of
independent branches reordered; every planted fault must fail with a message that names the call."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import kernel_checks as kc
import train_tape as tt

bf = lambda t: t.to(torch.bfloat16)
CASE = dict(hidden=128, heads=2, blocks=2, B=3, T=24, classes=4, labels=[2, 0, 2])      # M = 72: pad64 -> 128, the last 64-token tile partial


# ------------------------------------------------------------------------------------------------------------- the emulated entry points
class Emu:
    """ldt_amd.ops for the backward, in torch.  rev: every contraction runs in the opposite order (a different, equally legitimate rounding)."""

    def __init__(self, rev=False):
        self.rev = rev

    pad64 = staticmethod(kc.pad64)

    def _mm(self, a, b):                                                  # fp32 a [M, K] @ b [N, K]^T
        a, b = a.float(), b.float()
        return a.flip(1) @ b.flip(1).T if self.rev else a @ b.T

    @staticmethod
    def _into(out, val):
        if out is None:
            return val
        out.copy_(val)
        return out

    def cast_pad_bf16(self, src, cols_pad=None, out=None):
        src = src.reshape(-1, src.shape[-1])
        return self._into(out, kc.cast_pad_want(src, cols_pad or (src.shape[1] + 3) // 4 * 4))

    def transpose_cast_bf16(self, src, rows_pad=None, out=None):
        return self._into(out, kc.transpose_cast_want(src, rows_pad))

    def colsum(self, dy, out=None):
        return self._into(out, dy.double().sum(0).float())

    def wgrad(self, dy, x, out=None):
        return self._into(out, self._mm(self.transpose_cast_bf16(dy), self.transpose_cast_bf16(x)))

    def dgrad(self, dy, w_t, epilogue=None, out=None):
        from ldt_amd._lib import EPI_BF16
        r = self._mm(dy, w_t)
        return self._into(out, bf(r) if epilogue == EPI_BF16 else r)

    def sgemm(self, a, w, bias=None, act_in=0, act_out=0, out=None, out_bf16=False):
        assert not act_in and not act_out and not out_bf16
        r = self._mm(a, w)
        return self._into(out, r if bias is None else r + bias)

    def layernorm_modulate_bwd(self, x, dy, dx, scale=None, mod_sample_stride=0, rows_per_sample=None, want_mod=True, dshift=None, dscale=None):
        M, C = x.shape
        rps = M if rows_per_sample is None else rows_per_sample
        d = x - x.mean(1, keepdim=True)
        rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-6)
        xh = d * rstd
        g = dy * (1 + scale.repeat_interleave(rps, 0))
        dx.add_(rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)))
        if not want_mod:
            return None, None
        sh = dy.double().view(M // rps, rps, C).sum(1).float()
        sc = (dy * xh).double().view(M // rps, rps, C).sum(1).float()
        return self._into(dshift, sh), self._into(dscale, sc)

    def gelu_bwd(self, u, dh, out=None):
        u = u.float()
        dg = 0.5 * (1 + torch.erf(u * 0.7071067811865476)) + u * torch.exp(-0.5 * u * u) * 0.3989422804014327
        return self._into(out, bf(dh.float() * dg))

    def gate_residual_bwd(self, dy, gate, a=None, gate_sample_stride=None, rows_per_sample=None, out=None, dgate=None):
        M, C = dy.shape
        rps = M if rows_per_sample is None else rows_per_sample
        da = self._into(out, bf(dy * gate[:, :C].repeat_interleave(rps, 0)))
        if a is None:
            return da, None
        return da, self._into(dgate, (dy * a.float()).double().view(M // rps, rps, C).sum(1).float())

    def silu_bwd(self, c, dy, want_act=False):
        sg = torch.sigmoid(c)
        out = dy * sg * (1 + c * (1 - sg))
        return (out, c * sg) if want_act else out

    def dsm_loss_bwd(self, eta, params, weight=None, l1=False):
        d = params - eta
        g = torch.sign(d) if l1 else 2 * d
        if weight is not None:
            g = g * weight.reshape(-1)[:, None, None]
        return g * (1.0 / eta.numel())

    def embedding_grad(self, dc, label, n_classes):
        return torch.zeros(n_classes, dc.shape[1]).index_add_(0, label.reshape(-1).long(), dc)

    def attention_bwd(self, q, k, v, o, do, B, H, N, head_dim=64, out=None):
        C = H * 64
        hd = lambda z: z.float().reshape(B, N, H, 64).permute(0, 2, 1, 3)
        q4, k4, v4 = hd(q), hd(k), hd(v)
        o4, g4 = o.float().reshape(B, H, N, 64), do.float().reshape(B, H, N, 64)              # the raw buffers (Q1)
        s = q4 @ k4.transpose(-1, -2) * 0.125
        p = torch.exp(s - s.amax(-1, keepdim=True))
        P = p / p.sum(-1, keepdim=True)
        dS = P * (g4 @ v4.transpose(-1, -2) - (g4 * o4).sum(-1, keepdim=True))
        dSb, Pb = bf(dS).float(), bf(P).float()
        rows = lambda z: bf(z.permute(0, 2, 1, 3).reshape(B * N, C))
        if out is None:
            out = torch.empty(B * N, 3 * C, dtype=torch.bfloat16)
        out[:, :C], out[:, C:2 * C], out[:, 2 * C:] = rows(dSb @ k4 * 0.125), rows(dSb.transpose(-1, -2) @ q4 * 0.125), rows(Pb.transpose(-1, -2) @ g4)
        return out[:, :C], out[:, C:2 * C], out[:, 2 * C:]


class Faulty:
    """Emu with one planted fault in one entry point (the tape sits outside: it records the operands the step handed over)."""

    def __init__(self, emu, fault, D, M):
        self._emu, self._fault, self._D, self._M, self._n = emu, fault, D, M, {}

    def __getattr__(self, name):
        fn = getattr(self._emu, name)
        f, D, M = self._fault, self._D, self._M

        def count():
            self._n[name] = self._n.get(name, 0) + 1
            return self._n[name]

        def keep(g):                                                      # the tape binds operands by the entry point's parameter names
            g.__signature__ = inspect.signature(fn)
            return g
        if f == "scale block off by D" and name == "layernorm_modulate_bwd":
            def g(x, dy, dx, scale=None, **kw):
                if count() == 2:                                          # norm2 of the last block: its gate's columns instead of its scale's
                    scale = scale.as_strided(scale.shape, scale.stride(), scale.storage_offset() + D)
                return fn(x, dy, dx, scale=scale, **kw)
            return keep(g)
        if f == "dX overwritten" and name == "layernorm_modulate_bwd":
            def g(x, dy, dx, **kw):
                if count() == 3:
                    dx.zero_()
                return fn(x, dy, dx, **kw)
            return keep(g)
        if f == "fc_kv rows off by one block" and name == "wgrad":
            def g(dy, x, out=None):
                if dy.shape[1] == 2 * D and dy.stride(0) == 3 * D:        # [dk | dv] -> [dq | dk]
                    dy = dy.as_strided(dy.shape, dy.stride(), dy.storage_offset() - D)
                return fn(dy, x, out=out)
            return keep(g)
        if f == "last token tile dropped" and name == "wgrad":
            def g(dy, x, out=None):
                return fn(dy[:M // 64 * 64], x[:M // 64 * 64], out=out) if count() == 4 else fn(dy, x, out=out)
            return keep(g)
        if f == "dO permuted" and name == "attention_bwd":
            def g(q, k, v, o, do, B, H, N, **kw):
                return fn(q, k, v, o, do.reshape(B, H, N, 64).permute(0, 2, 1, 3).contiguous(), B, H, N, **kw)
            return keep(g)
        if f == "class row misplaced" and name == "embedding_grad":
            def g(dc, label, n_classes):
                r = fn(dc, label, n_classes)
                return r[[1, 0, 2, 3]]
            return keep(g)
        return fn


# ------------------------------------------------------------------------------------------------------------- the saved forward, from the oracle
def saved_from_oracle(model, x, t, label):
    """What ScoreTrainStep.forward keeps, computed with the oracle's layer functions in fp32 and rounded to bf16 where the kernels round.
    -> (S, params [B, T, z])."""
    from oracle import ldt_oracle as O
    from ldt_amd.layers import conv_w
    m = model
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    B, T, z = x.shape
    D, H, nb = m.hidden_size, m.num_heads, m.num_blocks
    M = B * T
    lin = lambda a, mod_: bf(a).float() @ bf(conv_w(mod_).detach()).float().T + mod_.bias.detach()
    S = {"B": B, "T": T, "label": label}
    S["e_t"] = O.sinusoid(t, m.t_dim // 4)
    S["a_t"] = O.linear(sd, "TimeEmbedding.mlp.0", S["e_t"])
    c = O.linear(sd, "TimeEmbedding.mlp.2", F.silu(S["a_t"]))
    if label is not None:
        S["lab"] = label.long()
        S["e_l"] = sd["LabelEmbedding.label_emb.weight"][S["lab"]].contiguous()
        S["a_l"] = O.linear(sd, "LabelEmbedding.mlp.0", S["e_l"])
        c = c + O.linear(sd, "LabelEmbedding.mlp.2", F.silu(S["a_l"]))
    S["c"] = c
    lins = [blk.adaLN[1] for blk in m.Transformer] + [m.ln_out.adaLN[1]]
    w_ada, b_ada = torch.cat([l.weight.detach() for l in lins], 0).contiguous(), torch.cat([l.bias.detach() for l in lins], 0)
    mod = S["mod"] = F.linear(F.silu(c), w_ada, b_ada)
    per_tok = lambda k: mod[:, k * D:(k + 1) * D].repeat_interleave(T, 0)
    lnmod = lambda X, k: bf(O.modulate(O.layer_norm(X), per_tok(k), per_tok(k + 1)))
    S["x_in"] = x.contiguous().view(M, z)
    X = lin(S["x_in"], m.ln_in)
    S["blocks"] = []
    for l, blk in enumerate(m.Transformer):
        k0 = 6 * l
        sb = {"x1": X.clone()}
        sb["h"] = lnmod(X, k0)
        sb["qkv"] = bf(torch.cat([lin(sb["h"], blk.fc_q), lin(sb["h"], blk.fc_kv)], 1))
        hd = lambda i: sb["qkv"][:, i * D:(i + 1) * D].float().reshape(B, T, H, 64).permute(0, 2, 1, 3)
        sb["o"] = bf((hd(0) @ hd(1).transpose(-1, -2) * 0.125).softmax(-1) @ hd(2)).contiguous()    # [B, H, T, 64]
        a1 = lin(sb["o"].view(M, D), blk.fc_o)                                                       # the raw reinterpretation (Q1)
        sb["a1"] = bf(a1)
        X = X + per_tok(k0 + 2) * a1
        sb["x2"] = X.clone()
        sb["h2"] = lnmod(X, k0 + 3)
        sb["u"] = bf(lin(sb["h2"], blk.mlp.fc[0][0]))
        sb["ug"] = bf(F.gelu(sb["u"].float()))
        a2 = lin(sb["ug"], blk.mlp.out)
        sb["a2"] = bf(a2)
        X = X + per_tok(k0 + 5) * a2
        S["blocks"].append(sb)
    S["xf"] = X
    S["hf"] = lnmod(X, 6 * nb)
    model.stacked_adaln = lambda: (w_ada, b_ada)                          # (the product's builds them from the packed device panels)
    return S, lin(S["hf"], m.ln_out.ln).view(B, T, z)


_SETUP = {}


def setup(tiny_cfg):
    if not _SETUP:
        model, x, t, label, eta = tt.make_case(tiny_cfg.score, **CASE)
        with torch.no_grad():
            S, params = saved_from_oracle(model, x, t, label)
        _SETUP.update(model=model, S=S, params=params, eta=eta, x=x, t=t, label=label)
    return _SETUP


def backward_on(tiny_cfg, monkeypatch, ops, corrupt=None, step_fault=None):
    """One taped backward of the product's ScoreTrainStep on `ops`.  corrupt(S_fed): edits the saved dict the step is handed (the audit keeps the
    pristine one).  step_fault: a Faulty fault planted BETWEEN the step and the tape (the step hands over a wrong operand, the kernel is right on
    what it gets); a fault inside `ops` sits behind the tape (the operands are right, the kernel is wrong).  -> (tape, model, S, dparams)."""
    import ldt_amd.train as train
    d = setup(tiny_cfg)
    model, S = d["model"], d["S"]
    tt.flat_grads(model)
    tape = tt.Tape(ops)
    tt.install_ops(monkeypatch, tape if step_fault is None else Faulty(tape, step_fault, model.hidden_size, S["B"] * S["T"]))
    step = train.ScoreTrainStep(model)
    step.saved = tt.copy_saved(S)
    if corrupt is not None:
        corrupt(step.saved)
    tape.mark("backward")
    dparams = tape.dsm_loss_bwd(d["eta"], d["params"])
    step.backward(dparams)
    monkeypatch.undo()
    assert step.saved is None
    return tape, model, S, dparams


def audit(tape, model, S, dparams):
    calls = tape.since("backward")
    worst = tt.audit_numeric(calls)
    tt.audit_wiring(calls, model, S, dparams)
    return worst


# ------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("rev", [False, True])
def test_emulated_backward_passes_the_audit_in_both_orders(tiny_cfg, monkeypatch, rev):
    tape, model, S, dparams = backward_on(tiny_cfg, monkeypatch, Emu(rev))
    worst = audit(tape, model, S, dparams)
    kinds = {"wgrad", "colsum", "dgrad fp32", "dgrad bf16", "sgemm", "layernorm_modulate_bwd dx", "layernorm_modulate_bwd dshift",
             "layernorm_modulate_bwd dscale", "gate_residual_bwd da", "gate_residual_bwd dgate", "gelu_bwd", "silu_bwd", "silu_bwd act", "dsm_loss_bwd",
             "embedding_grad", "attention_bwd dq", "attention_bwd dk", "attention_bwd dv", "transpose_cast_bf16", "cast_pad_bf16"}
    assert set(worst) == kinds and max(worst.values()) <= 1.0
    # the emulated step is the right gradient: against the oracle's float64 autograd (loosely, 1e-3 rel-MSE: the yardstick is the GPU test's)
    from oracle import ldt_oracle as O
    from conftest import rel_mse
    d = setup(tiny_cfg)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items()}
    lab = O.linear(sd, "LabelEmbedding.mlp.2", F.silu(O.linear(sd, "LabelEmbedding.mlp.0", sd["LabelEmbedding.label_emb.weight"][d["label"]])))
    ((d["eta"].double() - O.score_forward(sd, model.cfg, d["x"].double(), d["t"].double(), label_emb=lab)) ** 2).mean().backward()
    for n, p in model.named_parameters():
        assert rel_mse(p.grad, sd[n].grad) <= 1e-3, n


def test_reordered_independent_branches_pass(tiny_cfg, monkeypatch):
    """The weight and bias gradients of a layer hang off the chain: run first or last, the audit finds them by what they write."""
    tape, model, S, dparams = backward_on(tiny_cfg, monkeypatch, Emu())
    calls = tape.since("backward")
    side = [c for c in calls if c.name in ("wgrad", "colsum")]
    reordered = side[::-1] + [c for c in calls if c.name not in ("wgrad", "colsum")]
    tt.audit_numeric(reordered)
    tt.audit_wiring(reordered, model, S, dparams)


def _swap(key_from, key_to, block):
    def corrupt(S):
        S["blocks"][block][key_to] = S["blocks"][block][key_from]
    return corrupt


def _misplace_adaln(model):
    a, b = model.Transformer[0].adaLN[1].weight.grad, model.Transformer[1].adaLN[1].weight.grad
    b.copy_(a)


FAULTS = [  # name, (where, fault) or None, corruption of the saved dict or None, edit after the backward or None, what the message must name
    ("x2 fed where x1 belongs", None, _swap("x2", "x1", 1), None, r"layernorm_modulate_bwd.*operand `x` must be .*norm1 of block 1.*x2 of block 1"),
    ("a1 fed for the second gate", None, _swap("a1", "a2", 0), None, r"gate_residual_bwd.*operand `a` must be .*MLP branch of block 0.*a1 of block 0"),
    ("scale block off by D", ("step", "scale block off by D"), None, None, r"layernorm_modulate_bwd.*operand `scale` must be .*norm2 of block 1.*mod columns \[11 D"),
    ("fc_kv rows off by one block", ("step", "fc_kv rows off by one block"), None, None, r"wgrad.*operand `dy` must be .*fc_kv of block 1.*\[dq \| dk\] of block 1"),
    ("dX overwritten by the step", ("step", "dX overwritten"), None, None, r"layernorm_modulate_bwd.*dx must come in as the residual-stream gradient"),
    ("dX overwritten by the kernel", ("kernel", "dX overwritten"), None, None, r"layernorm_modulate_bwd.*dx after - before"),
    ("dO permuted to (B, T, H, 64)", ("step", "dO permuted"), None, None, r"no attention_bwd call reads dO = the dgrad of fc_o of block 1"),
    ("last token tile dropped from a wgrad", ("kernel", "last token tile dropped"), None, None, r"call #\d+ wgrad"),
    ("class row of the embedding gradient misplaced", ("kernel", "class row misplaced"), None, None, r"call #\d+ embedding_grad"),
    ("adaLN slice copied to the neighbour", None, None, _misplace_adaln, r"final \.grad of Transformer\.1\.adaLN\.1\.weight is not what call #\d+ sgemm"),
]


@pytest.mark.parametrize("name,fault,corrupt,after,names", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_faults_fail_the_audit_naming_the_call(tiny_cfg, monkeypatch, name, fault, corrupt, after, names):
    where, f = fault or (None, None)
    ops = Faulty(Emu(), f, CASE["hidden"], CASE["B"] * CASE["T"]) if where == "kernel" else Emu()
    tape, model, S, dparams = backward_on(tiny_cfg, monkeypatch, ops, corrupt, step_fault=f if where == "step" else None)
    if after is not None:
        after(model)
    with pytest.raises(AssertionError, match=names):
        audit(tape, model, S, dparams)


def test_a_write_outside_the_destination_view_is_caught(tiny_cfg, monkeypatch):
    class Spill(Emu):
        def gate_residual_bwd(self, dy, gate, a=None, gate_sample_stride=None, rows_per_sample=None, out=None, dgate=None):
            r = Emu.gate_residual_bwd(self, dy, gate, a, gate_sample_stride, rows_per_sample, out, dgate)
            if dgate is not None:
                dgate.as_strided((1,), (1,), dgate.storage_offset() + dgate.shape[1]).fill_(3.0)    # one element past the column block
            return r
    tape, *_ = backward_on(tiny_cfg, monkeypatch, Spill())
    with pytest.raises(AssertionError, match=r"gate_residual_bwd.*outside the destination view"):
        tt.audit_numeric(tape.since("backward"))


def test_the_transposed_operands_of_one_sample_are_row_major():
    """Found by the `one` case of test_gpu_train_tape.py: `x.t().contiguous()` returns a [1, n] row's transpose with strides (1, n), which
    ops.sgemm refuses; the step's transposing helper must hand over canonical strides for any shape."""
    from ldt_amd.train import _t
    for shape in ((1, 7), (7, 1), (3, 5), (1, 1)):
        x = torch.arange(shape[0] * shape[1], dtype=torch.float32).view(shape)
        y = _t(x)
        assert y.shape == (shape[1], shape[0]) and y.stride() == (shape[0], 1) and torch.equal(y, x.t())
