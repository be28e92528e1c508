"""CPU: the teeth of the call-by-call audit of the Compressor's three training steps (tests/compressor_tape.py, run on the MI355X by
test_gpu_compressor_tape.py).

test_train_tape_host.Emu, the pure-torch emulation of the `ops` entry points, is extended by the entry points the Compressor steps add
(the three attention backwards, ldt_reparam_kl_bwd, ldt_rows_gather_sum, ldt_actnorm_bwd, widen / add / the row map, and the per-sample
GEMM of the centred keys).  The product's `DecoderTrainStep.backward`, `TopDownTrainStep.backward` and `EncoderTrainStep.backward` run
unchanged on it on the CPU, from saved dicts built here by hand with the oracle's layer functions (the forwards refuse CPU tensors); the
centred keys are formed by the product's `_centred_keys` itself on the emulation.  Both audits must pass in both contraction orders, and
every planted fault must fail with a message that names the call or the link."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import compressor_tape as cpt
import decoder_train_checks as dc
import encoder_train_checks as ec
import kernel_checks as kc
import narrow_bwd_checks as nb
import topdown_train_checks as tc
import train_tape as tt
from test_train_tape_host import Emu, bf

# a shape of the `odd` kind, with a keep mask (40 of 48 prior rows) and a clamp that is live (min_sigma close under the logvar's range)
HOST = dict(hidden=64, heads=2, levels=3, enc_layers=1, z=5, T=8, B=3, N=40, rows=48, p_dim=32, actnorm=True, min_sigma=-0.05)


# ------------------------------------------------------------------------------------------------------------- the emulated entry points
class CEmu(Emu):
    """Emu plus what ldt_amd.compressor_train calls on top of the Score backward's entry points."""

    def __init__(self, rev=False, faults=()):
        super().__init__(rev)
        self.faults = dict(faults)                                      # entry point -> a fault its checks module plants

    def gemm_bf16(self, x, w, bias=None, epilogue=None, out=None, resid=None, skip=None, gate=None, gate_sample_stride=0, rows_per_sample=0,
                  step_ptr=None, gate_step_stride=0, n=None):
        from ldt_amd._lib import EPI_BF16
        assert epilogue == EPI_BF16 and resid is None and skip is None and gate is None
        r = self._mm(x, w)
        return self._into(out, bf(r if bias is None else r + bias))

    @staticmethod
    def _attn_out(r, rows, C, dq_out, dkv_out):
        dq = r["dq"] if dq_out is None else dq_out.copy_(r["dq"])
        if dkv_out is None:
            dkv_out = torch.empty(rows, 2 * C, dtype=torch.bfloat16)
        dkv_out[:, :C], dkv_out[:, C:] = r["dk"], r["dv"]
        return dq, dkv_out[:, :C], dkv_out[:, C:]

    def attention_bwd_cross(self, q, k, v, o, do, B, H, Nq, Nk, head_dim, dq_out=None, dkv_out=None):
        r = nb.emulate(q, torch.cat([k, v], 1), o.reshape(B, H, Nq, head_dim), do.reshape(B, H, Nq, head_dim), B, H, Nq, Nk, head_dim, True)
        return self._attn_out(r, B * Nk, H * head_dim, dq_out, dkv_out)

    def attention_bwd_long(self, q, k, v, o, do, B, H, Nq, Nk, dq_out=None, dkv_out=None, head_dim=32, scratch=None, stats_out=None):
        r = dc.long_emulate(q, torch.cat([k, v], 1), o.reshape(B, H, Nq, 32), do.reshape(B, H, Nq, 32), B, H, Nq, Nk)
        return self._attn_out(r, B * Nk, H * 32, dq_out, dkv_out)

    def attention_bwd_wide(self, q, k, v, o, do, B, H, Nq, Nk, dq_out=None, dkv_out=None, head_dim=32, scratch=None, stats_out=None):
        r, _ = tc.wide_emulate(q, torch.cat([k, v], 1), o.reshape(B, H, Nq, 32), do.reshape(B, H, Nq, 32), B, H, Nq, Nk)
        return self._attn_out(r, B * Nk, H * 32, dq_out, dkv_out)

    def reparam_kl_bwd(self, post, noise, d_eps, kl_scale, lo, hi):
        return tc.reparam_kl_bwd_closed(post, noise, d_eps, kl_scale, lo, hi, dt=torch.float32, fault=self.faults.get("reparam_kl_bwd"))

    def rows_gather_sum(self, dy, src, N):
        return dc.rows_gather_sum_emulate(dy, src, N, fault=self.faults.get("rows_gather_sum"))

    def actnorm_bwd(self, dz, z, log_scale, B, dx=None, dshift=None, dlog_scale=None, want_sums=True):
        r = ec.actnorm_bwd_emulate(dz.reshape(B, -1), z.reshape(B, -1), log_scale.reshape(-1), fault=self.faults.get("actnorm_bwd"))
        dx = r[0].reshape(dz.shape) if dx is None else dx.copy_(r[0].reshape(dz.shape))
        if not want_sums:
            return dx, None, None
        return dx, self._into(dshift, r[1]), self._into(dlog_scale, r[2])

    def widen_bf16(self, w):
        return w.float()

    def add_f32(self, a, b, out=None):
        return self._into(out, a + b)

    def prior_row_map(self, keep):
        keep = keep.to(torch.bool)
        pos = keep.to(torch.int32).cumsum(1, dtype=torch.int32) - 1
        return torch.where(keep, pos, torch.full_like(pos, -1)).contiguous()


class Plant:
    """One planted fault in front of `inner` (between the step and the tape: the step hands over a wrong operand, the kernel is right on what
    it gets; or behind the tape: the operands are right, the kernel is wrong).  sigs: where the entry points' signatures are read."""

    def __init__(self, inner, fault, ctx, sigs):
        self._inner, self._fault, self._ctx, self._sigs, self._n, self._state = inner, fault, ctx, sigs, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        handler = FAULTS.get(self._fault, {}).get(name)
        if handler is None:
            return fn
        sig = inspect.signature(getattr(self._sigs, name))

        def g(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            self._n[name] = self._n.get(name, 0) + 1
            return handler(bound.arguments, lambda A=bound.arguments: fn(**A), self._n[name], self._ctx, self._state)
        g.__signature__ = sig
        return g


def _shift(t, by):
    return t.as_strided(t.shape, t.stride(), t.storage_offset() + by)


def _dy_into_dxp():
    def silu(A, call, n, ctx, st):
        r = call()
        st["dXp"] = r[0]
        return r

    def add(A, call, n, ctx, st):
        if A["a"].shape[0] == ctx["B"] * ctx["N"] and "done" not in st:  # level L - 1's add into the set stream
            st["done"] = True
            A["a"], A["b"], A["out"] = st["dXp"], A["b"][:st["dXp"].shape[0]].contiguous(), st["dXp"]
        return call()
    return {"silu_bwd": silu, "add_f32": add}


def _final_ln_from_zeros(A, call, n, ctx, st):
    if n == 1 + 2 * ctx["E"] + 1:                                        # the FinalLayer of the last stage but one
        A["dx"].zero_()
    return call()


def _ln_bias_from_dw(A, call, n, ctx, st):
    C = ctx["C"]
    if A["out"] is not None and tuple(A["out"].shape) == (1, C) and "done" not in st:
        st["done"] = True
        A["a"] = st["dW"][:, 0].reshape(1, 2 * C).contiguous()
    r = call()
    if A["out"] is None and tuple(r.shape) == (2 * C, ctx["z"]):
        st["dW"] = r
    return r


def _d_eps_one_level_off(A, call, n, ctx, st):
    o = A["out"]
    if o is not None and tuple(o.shape) == (ctx["B"] * ctx["T"], ctx["z"]) and o.stride(0) == ctx["L"] * ctx["z"] and "done" not in st:
        st["done"] = True
        A["out"] = _shift(o, -ctx["z"])
    return call()


def _kl_scale_dropped(A, call, n, ctx, st):
    A["kl_scale"] = 0.0
    return call()


def _o_of_level_0(A, call, n, ctx, st):
    if n == 1:                                                           # decoder level L - 1 runs backward first
        A["o"] = ctx["S"]["levels"][0]["o"]
    return call()


def _x_for_z(A, call, n, ctx, st):
    ci = ctx["model"].conv_in
    per = ci.shift.numel()
    A["z"] = (A["z"].reshape(-1, per) * torch.exp(ci.log_scale.detach().reshape(-1)) + ci.shift.detach().reshape(-1)).reshape(A["z"].shape)
    return call()


def _scale_is_gamma(A, call, n, ctx, st):
    if "done" not in st and bool((A["b"] == -1).all()):
        st["done"] = True
        A["b"] = torch.zeros_like(A["b"])
    return call()


def _dgate_off_by_c(A, call, n, ctx, st):
    if n == 1:
        A["dgate"] = _shift(A["dgate"], ctx["C"])
    return call()


def _roomy_dkv(A, call, n, ctx, st):
    """The step's side of `one row written past dkv_out`: the destination gets a row of storage behind it, so that the emulated kernel's
    stray store lands in memory the tape watches (on the CPU it could not be planted otherwise)."""
    if n != 1:
        return call()
    mine = A["dkv_out"]
    big = torch.zeros(mine.shape[0] + 1, mine.shape[1], dtype=mine.dtype)
    A["dkv_out"] = big[:mine.shape[0]]
    dq, _, _ = call()
    mine.copy_(big[:mine.shape[0]])
    C = mine.shape[1] // 2
    return dq, mine[:, :C], mine[:, C:]


def _row_past_dkv(A, call, n, ctx, st):
    r = call()
    if n == 1:
        o = A["dkv_out"]
        o.as_strided((1, o.shape[1]), (o.shape[1], 1), o.storage_offset() + o.shape[0] * o.shape[1]).fill_(3.0)
    return r


def _v_overwritten(A, call, n, ctx, st):
    from ldt_amd._lib import EPI_BF16
    r = call()
    if A["out"] is not None and A["epilogue"] == EPI_BF16 and "done" not in st:
        st["done"] = True
        _shift(A["out"], ctx["C"]).add_(1.0)
    return r


FAULTS = {
    "dy into dXp at level >= 1": _dy_into_dxp(),
    "FinalLayer from zeros": {"layernorm_modulate_bwd": _final_ln_from_zeros},
    "ln.bias from dW_zkv": {"sgemm": _ln_bias_from_dw},
    "d_eps one level off": {"sgemm": _d_eps_one_level_off},
    "kl_scale dropped": {"reparam_kl_bwd": _kl_scale_dropped},
    "o of level 0": {"attention_bwd_long": _o_of_level_0},
    "x for z": {"actnorm_bwd": _x_for_z},
    "scale = gamma": {"add_f32": _scale_is_gamma},
    "dgate off by C": {"gate_residual_bwd": _dgate_off_by_c},
    "roomy dkv": {"attention_bwd_long": _roomy_dkv},
    "row past dkv_out": {"attention_bwd_long": _row_past_dkv},
    "V overwritten": {"gemm_bf16": _v_overwritten},
}


# ------------------------------------------------------------------------------------------------------------- the saved forwards, by hand
def _lin(a, layer):
    from ldt_amd.layers import conv_w
    return bf(a).float() @ bf(conv_w(layer).detach()).float().T + layer.bias.detach()


def _attend(q, kv, B, H, Nq, Nk):
    """bf16 [B, H, Nq, 32], contiguous: the saved attention output."""
    C = H * 32
    hd = lambda t, n: t.float().reshape(B, n, H, 32).permute(0, 2, 1, 3)
    s = hd(q, Nq) @ hd(kv[:, :C], Nk).transpose(-1, -2) * 32 ** -0.5
    return bf(s.softmax(-1) @ hd(kv[:, C:], Nk)).contiguous()


def _key_panel(blk):
    from ldt_amd.layers import conv_w
    C = blk.fc_q.weight.shape[0]
    return {"C": C, "wkv": kc.cast_pad_want(conv_w(blk.fc_kv).detach().float().contiguous(), kc.pad64(C)), "bkv": blk.fc_kv.bias.detach().float().contiguous()}


def _nocond_block(blk, X, kv, B, H, Nq, Nk):
    """layers.py:224-226 on the fp32 rows X, bf16 where the kernels round -> (the block's tape as _block_fwd keeps it, the new X)."""
    from oracle import ldt_oracle as O
    M, C = X.shape
    ln = lambda x, norm: bf(O.layer_norm(x, norm.affine[0].detach(), norm.affine[1].detach()))
    sb = {"x1": X.clone()}
    sb["h"] = ln(X, blk.norm1)
    sb["q"] = bf(_lin(sb["h"], blk.fc_q))
    sb["kv"] = kv
    sb["o"] = _attend(sb["q"], kv, B, H, Nq, Nk)
    X = X + _lin(sb["o"].view(M, C), blk.fc_o)
    sb["x2"] = X.clone()
    sb["h2"] = ln(X, blk.norm2)
    sb["u"] = bf(_lin(sb["h2"], blk.mlp.fc[0][0]))
    sb["ug"] = bf(F.gelu(sb["u"].float()))
    return sb, X + _lin(sb["ug"], blk.mlp.out)


def saved_topdown(ct, case):
    """What TopDownTrainStep.forward keeps (DecoderTrainStep's is the same dict without `post`, on the same latents)."""
    from ldt_amd.layers import conv_w
    m = case["model"]
    L, z, C, H = m.n_layers, m.z_dim, m.hidden_dim, m.num_heads
    B, N, T = case["B"], case["N"], case["T"]
    f32 = lambda t: t.detach().float().contiguous()
    prior = f32(m.init_set.prior)
    X = torch.stack([prior[case["keep"][b]] for b in range(B)], 0).reshape(B * N, C)
    all_eps = torch.empty(B * T, L * z)
    S = {"B": B, "N": N, "T": T, "eps": all_eps, "src": ct.ops.prior_row_map(case["keep"]), "w_zkv_t": [None] * L, "levels": [], "post": []}
    for j in range(L):
        d = m.decoder[L - 1 - j]
        xj = case["enc_out"][-j - 1].reshape(B * T, C).clone()
        y, nk = (kc.cast_pad_want(xj, kc.pad64(C)), T) if j == 0 else (kc.cast_pad_want(X, kc.pad64(C)), N)
        pb, xj = _nocond_block(d.att, xj, bf(_lin(y, d.att.fc_kv)), B, H, T, nk)
        pb["y"], pb["x3"] = y, xj
        pb["kv"] = ct._centred_keys(_key_panel(d.att), y, pb["kv"], B, nk)                   # the product's own, on the emulation
        pb["post"] = F.linear(F.silu(xj), f32(conv_w(d.prior[1])), f32(d.prior[1].bias))
        pb["noise"] = case["post_noise"][j].reshape(B * T, z).contiguous()
        mu, lv = pb["post"][:, :z], pb["post"][:, z:].clamp(m.min_sigma, 10.)
        all_eps[:, z * j: z * (j + 1)] = mu + torch.exp(lv / 2) * pb["noise"]
        S["post"].append(pb)
        w_kv, w_ln = f32(conv_w(d.att1.fc_kv)), f32(conv_w(d.ln))
        w_zkv, b_zkv = w_kv @ w_ln, w_kv @ f32(d.ln.bias) + f32(d.att1.fc_kv.bias)
        S["w_zkv_t"][j] = w_zkv.t().contiguous()
        kv1 = bf(all_eps[:, z * j: z * (j + 1)] @ w_zkv.T + b_zkv)
        sb, X = _nocond_block(d.att1, X, kv1, B, H, N, T)
        S["levels"].append(sb)
    S["xf"] = X
    return S


def saved_encoder(ct, case):
    """What EncoderTrainStep.forward keeps."""
    from oracle import ldt_oracle as O
    m = case["model"]
    C, H, L, E = m.hidden_dim, m.num_heads, m.n_layers, m.encoder_layers
    B, T = case["B"], case["T"]
    M = B * T
    X = case["tokens"].reshape(M, C).clone()
    if m.ActNorm is not None:
        ci = m.conv_in
        per = ci.shift.numel()
        X = ((X.reshape(-1, per) - ci.shift.detach().reshape(-1)) * torch.exp(-ci.log_scale.detach().reshape(-1))).reshape(M, C)
    S = {"B": B, "T": T, "stages": [], "pos": case["pos"].clone()}
    lins = [lin for e in m.encoder for lin in [a.adaLN[1] for a in e.atts] + [e.conv_out.adaLN[1]]]
    S["w_ada"] = torch.cat([lin.weight.detach() for lin in lins], 0).contiguous()
    mod = S["mod"] = F.linear(F.silu(S["pos"]), S["w_ada"], torch.cat([lin.bias.detach() for lin in lins], 0))
    mv = lambda off: mod[:, off:off + C].repeat_interleave(T, 0)
    lnmod = lambda x, off: bf(O.modulate(O.layer_norm(x), mv(off), mv(off + C)))
    m0 = 0
    for enc in m.encoder:
        st = {"blocks": []}
        for blk in enc.atts:
            sb = {"x1": X.clone()}
            sb["h"] = lnmod(X, m0)
            sb["y"] = kc.cast_pad_want(X, kc.pad64(C))                   # K / V from the RAW x (quirk Q2)
            sb["q"] = bf(_lin(sb["h"], blk.fc_q))
            kv = bf(_lin(sb["y"], blk.fc_kv))
            sb["o"] = _attend(sb["q"], kv, B, H, T, T)
            sb["kv"] = ct._centred_keys(_key_panel(blk), sb["y"], kv, B, T)
            a1 = _lin(sb["o"].view(M, C), blk.fc_o)
            sb["a1"] = bf(a1)
            X = X + mv(m0 + 2 * C) * a1
            sb["x2"] = X.clone()
            sb["h2"] = lnmod(X, m0 + 3 * C)
            sb["u"] = bf(_lin(sb["h2"], blk.mlp.fc[0][0]))
            sb["ug"] = bf(F.gelu(sb["u"].float()))
            a2 = _lin(sb["ug"], blk.mlp.out)
            sb["a2"] = bf(a2)
            X = X + mv(m0 + 5 * C) * a2
            st["blocks"].append(sb)
            m0 += 6 * C
        st["xf"] = X.clone()
        st["hf"] = lnmod(X, m0)
        m0 += 2 * C
        S["stages"].append(st)
    return S


class OnDevice(torch.Tensor):
    """A CPU tensor that answers `is_cuda` with True: EncoderTrainStep.backward refuses host gradients before it launches anything, and the
    step has to run here unchanged.  Nothing else about the tensor differs."""
    is_cuda = property(lambda self: True)


# ------------------------------------------------------------------------------------------------------------- driving the steps
def drive(tiny_cfg, kind, emu=None, step_fault=None, kernel_fault=None, corrupt=None):
    """One taped backward of the product's step `kind` on the emulation -> a dict the audits read."""
    import ldt_amd.compressor_train as ct
    emu = CEmu() if emu is None else emu
    case = cpt.make_case(tiny_cfg.compressor, **HOST)
    m = case["model"]
    tt.flat_grads(m)
    ctx = dict(C=m.hidden_dim, B=case["B"], N=case["N"], T=case["T"], z=m.z_dim, L=m.n_layers, E=m.encoder_layers, model=m)
    tape = tt.Tape(emu if kernel_fault is None else Plant(emu, kernel_fault, ctx, emu))
    r = dict(case=case, model=m, tape=tape, kind=kind)
    with pytest.MonkeyPatch.context() as mp:
        tt.install_ops(mp, tape)
        S = saved_encoder(ct, case) if kind == "encoder" else saved_topdown(ct, case)
        ctx["S"] = S
        tt.install_ops(mp, tape if step_fault is None else Plant(tape, step_fault, ctx, emu))
        fed = cpt.copy_saved(S)
        if corrupt is not None:
            corrupt(fed)
        tape.mark("backward")
        if kind == "decoder":
            step = ct.DecoderTrainStep(m)
            step.saved = fed
            r.update(dset=case["d_set"], d_eps=step.backward(case["d_set"]))
        elif kind == "topdown":
            step = ct.TopDownTrainStep(m)
            step.saved = fed
            d_enc = step.backward(case["d_set"], case["kl_scale"])
            r.update(dset=case["d_set"], d_eps=step.d_eps, d_enc=[t.clone() for t in d_enc], kl_scale=case["kl_scale"])
        else:
            step = ct.EncoderTrainStep(m)
            step.saved = fed
            d_tokens, d_pos = step.backward([t.as_subclass(OnDevice) for t in case["d_enc"]])
            r.update(d_enc=case["d_enc"], d_tokens=d_tokens, d_pos=d_pos)
        assert step.saved is None
    r["S"] = S
    return r


def audit(r, numeric=True):
    """The numeric audit (with the centred keys of the forward part), then the table.  -> {call kind: worst err / tol}."""
    tape, m, S, kind = r["tape"], r["model"], r["S"], r["kind"]
    calls = tape.since("backward")
    worst = cpt.audit_numeric(calls) if numeric else {}
    if kind != "decoder" and numeric:
        cpt.audit_centred(tape.calls[:tape.marks["backward"]], cpt.centred_groups(m, S, kind), worst)
    if kind == "decoder":
        cpt.audit_decoder(calls, m, S, r["dset"], r["d_eps"], r["case"]["keep"])
    elif kind == "topdown":
        cpt.audit_topdown(calls, m, S, r["dset"], r["kl_scale"], r["d_eps"], r["d_enc"], r["case"]["keep"])
    else:
        cpt.audit_encoder(calls, m, S, r["d_enc"], r["d_tokens"], r["d_pos"])
    return worst


# ------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("kind", ["decoder", "topdown", "encoder"])
def test_emulated_backward_passes_both_audits_in_both_orders(tiny_cfg, kind, rev):
    from conftest import rel_mse
    r = drive(tiny_cfg, kind, CEmu(rev))
    m, case = r["model"], r["case"]
    calls = r["tape"].since("backward")
    cpt.assert_counts(calls, cpt.expected_counts(kind, m.n_layers, m.encoder_layers, True), kind)
    worst = audit(r)
    assert max(worst.values()) <= 1.0
    want = {"decoder": {"attention_bwd_long dq", "rows_gather_sum", "widen_bf16", "add_f32", "sgemm", "wgrad"},
            "topdown": {"attention_bwd_wide dq", "attention_bwd_cross", "reparam_kl_bwd", "silu_bwd", "centred gemm_bf16", "centred colsum", "centred sgemm"},
            "encoder": {"attention_bwd_cross", "actnorm_bwd dx", "actnorm_bwd dlog_scale", "gate_residual_bwd dgate", "centred gemm_bf16"}}[kind]
    assert want <= set(worst), sorted(want - set(worst))
    # the emulated step is the right gradient: against the float64 restatements (loosely: the yardstick is the GPU test's)
    import ldt_amd.compressor_train as ct
    if kind == "decoder":
        from test_gpu_decoder_train import oracle_step
        names = [n for n, _ in ct.decoder_parameters(m)]
        eps = r["S"]["eps"].view(case["B"], case["T"], -1)
        ref = oracle_step(case["init"], case["cfg"], names, eps, case["target"], torch.float64, keep_mask=case["keep"], d_set=case["d_set"])[0]
        got = {"d_eps": r["d_eps"]}
    elif kind == "topdown":
        names = [n for n, _ in ct.topdown_parameters(m)]
        ref = tc.oracle_step(case["init"], case["cfg"], names, case["enc_out"], case["post_noise"], case["target"], torch.float64, cpt.KL_WEIGHT,
                             keep_mask=case["keep"], d_set=case["d_set"])[0]
        got = {"d_enc_out.%d" % i: t for i, t in enumerate(r["d_enc"])}
    else:
        names = [n for n, _ in ct.encoder_parameters(m)]
        ref = ec.encoder_step(case["init"], case["cfg"], names, case["tokens"], case["pos"], case["d_enc"], torch.float64)[0]
        got = {"d_tokens": r["d_tokens"], "d_pos": r["d_pos"]}
    got.update({n: dict(m.named_parameters())[n].grad for n in names})
    for n, g in got.items():
        e = rel_mse(g.detach().as_subclass(torch.Tensor).reshape(ref[n].shape), ref[n])
        assert e <= 1e-2, (n, e)


def test_reordered_independent_branches_pass(tiny_cfg):
    """The weight and bias gradients hang off the chain: listed first or last, the tables find them by what they write."""
    r = drive(tiny_cfg, "topdown")
    calls = r["tape"].since("backward")
    side = [c for c in calls if c.name in ("wgrad", "colsum")]
    r["tape"].calls[r["tape"].marks["backward"]:] = side[::-1] + [c for c in calls if c.name not in ("wgrad", "colsum")]
    audit(r)


def test_a_call_kind_without_a_reference_and_an_activated_sgemm_are_refused():
    """Nothing slips through unaudited: an entry point the audit does not know raises, and so does an ldt_sgemm with an activation (the
    one kind train_tape.check_call answers with {}: the Compressor's backwards make none)."""
    one = torch.ones(2, 2)
    with pytest.raises(AssertionError, match=r"mixture_seed.*a call kind the audit has no reference for"):
        cpt.check_call(tt.Call(0, "mixture_seed", {"e": tt.Rec(one)}))
    call = tt.Call(1, "sgemm", {"a": tt.Rec(one), "w": tt.Rec(one), "bias": None, "act_in": 1, "act_out": 0, "out": None, "out_bf16": False})
    with pytest.raises(AssertionError, match=r"call #1 sgemm.*an sgemm with an activation on a backward's tape"):
        cpt.check_call(call)


def test_the_clamp_is_live_in_the_host_case(tiny_cfg):
    """min_sigma = -0.05 puts part of every level's logvar below the clamp: the mask of reparam_kl_bwd is exercised, not vacuous."""
    r = drive(tiny_cfg, "topdown")
    z = r["model"].z_dim
    for pb in r["S"]["post"]:
        dead = pb["post"][:, z:] < r["model"].min_sigma
        assert 0 < int(dead.sum()) < dead.numel()


def test_centring_the_keys_leaves_the_attention_backward_alone():
    """The premise of _centred_keys, in float64: dq, dk and dv of attn_bwd_ref are the same, to 1e-12 relative, with K and with
    K - mean_j K_j (softmax is invariant under a shift common to a row's logits; sum_j dS_j = 0)."""
    B, H, Nq, Nk = 2, 2, 24, 40
    C = H * 32
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B * n, C, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk))
    k = k + 3.0 * torch.randn(1, C, generator=g, dtype=torch.float64)                      # a large common component
    do = torch.randn(B, H, Nq, 32, generator=g, dtype=torch.float64)
    P = torch.softmax(kc.heads(q, B, Nq, H, 32) @ kc.heads(k, B, Nk, H, 32).transpose(-1, -2) * 32 ** -0.5, -1)
    o = P @ kc.heads(v, B, Nk, H, 32)
    kc_ = (k.view(B, Nk, C) - k.view(B, Nk, C).mean(1, keepdim=True)).reshape(B * Nk, C)
    a, _ = kc.attn_bwd_ref(q, k, v, o, do, B, H, Nq, Nk, 32)
    b, _ = kc.attn_bwd_ref(q, kc_, v, o, do, B, H, Nq, Nk, 32)
    for n in ("dq", "dk", "dv"):
        assert float((a[n] - b[n]).abs().max()) <= 1e-12 * float(a[n].abs().max()), n


def _reverse_d_enc(r):
    r["d_enc"] = r["d_enc"][::-1]


def _stale_bias(r):
    r["model"].decoder[1].att1.fc_kv.bias.grad.zero_()


def _first_rows_src(S):
    B, R = S["src"].shape
    keep = torch.zeros(B, R, dtype=torch.bool)
    keep[:, :S["N"]] = True                                              # (a mask that keeps the first N rows: what src is without a keep mask)
    S["src"] = cpt.prior_row_map_want(keep)


PLANTED = [  # name, step, dict(step_fault / kernel_fault / corrupt / after / emu faults), what the message must name
    ("the posterior's dy added to dXp at a level j >= 1", "topdown", dict(step_fault="dy into dXp at level >= 1"),
     r"no add_f32 call adds the K / V-source gradient of level 2 to the SET stream's dX"),
    ("the FinalLayer's LayerNorm backward started from zeros in an earlier stage", "encoder", dict(step_fault="FinalLayer from zeros"),
     r"layernorm_modulate_bwd.*dx must come in as the running stream gradient \(the FinalLayer of stage 1\)"),
    ("fc_kv.bias.grad left stale", "decoder", dict(after=_stale_bias), r"final \.grad of decoder\.1\.att1\.fc_kv\.bias is not what call #\d+ colsum"),
    ("ln.bias.grad from dW_zkv instead of db_zkv", "decoder", dict(step_fault="ln.bias from dW_zkv"), r"sgemm.*operand `a` must be db_zkv of decoder level 2"),
    ("the d_eps slice one level off", "decoder", dict(step_fault="d_eps one level off"),
     r"no sgemm call writes columns \[2 z, 3 z\) of the one \[B T, L z\] d_eps buffer"),
    ("d_enc_out in reversed order", "topdown", dict(after=_reverse_d_enc), r"d_enc_out\[0\] must be level 2's final dXp"),
    ("kl_scale dropped", "topdown", dict(step_fault="kl_scale dropped"), r"reparam_kl_bwd.*operand `kl_scale` must be the kl_scale given"),
    ("src from a mask of the first N rows under a keep mask", "decoder", dict(corrupt=_first_rows_src),
     r"rows_gather_sum.*operand `src` must be prior_row_map of the call's keep mask"),
    ("o of another level handed to the attention backward", "decoder", dict(step_fault="o of level 0"),
     r"attention_bwd_long.*operand `o` must be the saved attention output o of decoder level 2.*o of decoder level 0"),
    ("x instead of z in actnorm_bwd", "encoder", dict(step_fault="x for z"), r"actnorm_bwd.*operand `z` must be the first block's saved x1"),
    ("scale = gamma instead of gamma - 1", "decoder", dict(step_fault="scale = gamma"), r"layernorm_modulate_bwd.*operand `scale` must be fp32 gamma - 1 of norm2 of decoder level 2"),
    ("a dgate block off by C", "encoder", dict(step_fault="dgate off by C"),
     r"no gate_residual_bwd call writes dmod columns \[21 C, 22 C\): dgate of the MLP branch of block 0 of stage 2"),
    ("one row written past dkv_out", "decoder", dict(step_fault="roomy dkv", kernel_fault="row past dkv_out"),
     r"attention_bwd_long.*outside the destination view\(s\) `dkv_out`"),
    ("uncentred V overwritten by the centring GEMM", "topdown", dict(kernel_fault="V overwritten"), r"gemm_bf16.*outside the destination view"),
    ("the clamp mask ignored by the kernel", "topdown", dict(emu={"reparam_kl_bwd": "clamp mask ignored"}), r"call #\d+ reparam_kl_bwd"),
    ("the wrong samples' rows gathered by the kernel", "decoder", dict(emu={"rows_gather_sum": "wrong sample set"}), r"call #\d+ rows_gather_sum"),
    ("exp(+log_scale) inside the ActNorm kernel", "encoder", dict(emu={"actnorm_bwd": "exp(+log_scale)"}), r"call #\d+ actnorm_bwd"),
]


@pytest.mark.parametrize("name,kind,plant,names", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_faults_fail_the_audit_naming_the_call_or_the_link(tiny_cfg, name, kind, plant, names):
    r = drive(tiny_cfg, kind, CEmu(faults=plant.get("emu", ())), plant.get("step_fault"), plant.get("kernel_fault"), plant.get("corrupt"))
    if "after" in plant:
        plant["after"](r)
    # a fault between the step and the tape leaves every kernel right on what it was handed: the table alone is asked (the emulation's fp32
    # sums are torch's, not the kernels', and on the operands a fault makes up they need not sit inside a kernel's statistical bound)
    with pytest.raises(AssertionError, match=names):
        audit(r, numeric="kernel_fault" in plant or "emu" in plant)
