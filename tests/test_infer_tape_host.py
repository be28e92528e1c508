"""CPU: the teeth of the call-by-call audit of the inference forwards (tests/infer_tape.py, run on the MI355X by test_gpu_infer_tape.py).

test_train_tape_host.Emu, the pure-torch emulation of the `ops` entry points, is extended by every entry point `Compressor.forward` and
`Compressor.sample` reach (float64 definitions rounded where the kernels round; the contractions in fp32, in either order).  The product's two
forwards run UNCHANGED on it on the CPU: `Compressor._device` answers with a device string whose `.type` is "cuda" (the forwards refuse host
parameters before they launch anything; nothing else about the run differs).  Both audits must pass on that tape, in both contraction orders
and with independent calls reordered; every planted fault must fail with a message that names the call or the link."""
import inspect

import pytest
import torch

import infer_tape as it
import kernel_checks as kc
import train_tape as tt
from test_train_tape_host import Emu, bf


# ------------------------------------------------------------------------------------------------------------- the emulated entry points
def _krows(t, stride, M, rps):
    """Per-sample rows as the KERNEL addresses them: row r of the result is the C values at (r // rps) * stride behind t's first."""
    rps = rps or M
    n = (M + rps - 1) // rps
    rows = t[:1] if n == 1 else t.as_strided((n, t.shape[1]), (stride, 1), t.storage_offset())
    return rows.double()[torch.arange(M) // rps]


def _ln64(x, w=None, b=None, shift=None, scale=None, stride=0, rps=0):
    xd = x.double()
    h = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6)
    if w is not None:
        h = h * w.double() + b.double()
    if shift is not None:
        h = h * (1 + _krows(scale, stride, x.shape[0], rps)) + _krows(shift, stride, x.shape[0], rps)
    return h


def _act64(v, act):
    from ldt_amd._lib import ACT_GELU, ACT_RELU, ACT_SILU
    if act == ACT_SILU:
        return v / (1 + torch.exp(-v))
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_GELU:
        return torch.nn.functional.gelu(v)
    return v


class IEmu(Emu):
    """Emu plus what ldt_amd.compressor and ldt_amd.blocks call.  faults: kernel-side faults by name."""
    FPS_SKIP_NEAR_ORIGIN = True
    GROUPER_FRAGS = 132

    def __init__(self, rev=False, faults=()):
        super().__init__(rev)
        self.faults = set(faults)

    def sgemm(self, a, w, bias=None, act_in=0, act_out=0, out=None, out_bf16=False):
        r = self._mm(_act64(a.double(), act_in).float(), w)
        r = _act64((r if bias is None else r + bias).double(), act_out).float()
        return self._into(out, bf(r) if (out_bf16 or (out is not None and out.dtype == torch.bfloat16)) else r)

    def gemm_bf16(self, x, w, bias=None, epilogue=None, out=None, resid=None, skip=None, gate=None, gate_sample_stride=0, rows_per_sample=0,
                  step_ptr=None, gate_step_stride=0, n=None):
        from ldt_amd._lib import EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RELU_BF16, EPI_RESID_F32
        N = w.shape[0] if n is None else n
        r = self._mm(x, w[:N])
        if bias is not None:
            r = r + bias[:N]
        if epilogue == EPI_F32:
            return self._into(out, r)
        if epilogue == EPI_BF16:
            return self._into(out, bf(r))
        if epilogue == EPI_GELU_BF16:
            return self._into(out, bf(torch.nn.functional.gelu(r.double()).float()))
        if epilogue == EPI_RELU_BF16:
            return self._into(out, bf(torch.relu(r if skip is None else r + skip.float())))
        assert epilogue == EPI_RESID_F32
        resid = out if resid is None else resid
        upd = r.double() if gate is None else _krows(gate, gate_sample_stride, x.shape[0], rows_per_sample)[:, :N] * r.double()
        val = (resid.double() + upd).float()
        return self._into(out, val)

    def layernorm_modulate(self, x, w=None, b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0, step_ptr=None, mod_step_stride=0, out=None):
        return self._into(out, bf(_ln64(x, w, b, shift, scale, mod_sample_stride, rows_per_sample).float()))

    def group_stats(self, x, B, T, groups, eps=1e-6):
        return kc.group_stats_ref(x, B, T, x.shape[1], groups, eps)[0].float()

    def norm_apply(self, x, stats=None, rows_per_stat=1, w=None, b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=1, out=None):
        M = x.shape[0]
        kw = {} if shift is None else dict(shift=_krows(shift, mod_sample_stride, M, rows_per_sample)[::rows_per_sample].float(),
                                           scale=_krows(scale, mod_sample_stride, M, rows_per_sample)[::rows_per_sample].float(), rows_per_sample=rows_per_sample)
        return self._into(out, bf(kc.norm_apply_ref(x, stats, rows_per_stat, w=w, b=b, **kw)[0].float()))

    def block_activation_(self, x, kind):
        name = {v: k for k, v in kc.BLOCK_ACT_KINDS.items()}[kind]
        x.copy_(kc.block_act_exact(x, name) if name in kc.EXACT_ACTS else bf(kc.block_act_ref(x, name)[0].float()))
        return x

    def ln_linear(self, x, w, bias=None, ln_w=None, ln_b=None, shift=None, scale=None, mod_sample_stride=0, rows_per_sample=0, out=None):
        h = bf(_ln64(x, ln_w, ln_b, shift, scale, mod_sample_stride, rows_per_sample).float())
        r = self._mm(h, w)
        return self._into(out, bf(r if bias is None else r + bias))

    def ln_mlp_resid_(self, x, w_up, b_up, w_dn, b_dn, ln_w=None, ln_b=None, shift=None, scale=None, gate=None, mod_sample_stride=0, rows_per_sample=0,
                      x_bf16_out=None, next_linear=None):
        M, C = x.shape
        x0 = x.clone()
        h = bf(_ln64(x, ln_w, ln_b, shift, scale, mod_sample_stride, rows_per_sample).float())
        u = bf(torch.nn.functional.gelu((self._mm(h, w_up) + b_up).double()).float())
        upd = (self._mm(u, w_dn) + b_dn).double()
        if gate is not None:
            upd = _krows(gate, mod_sample_stride, M, rows_per_sample) * upd
        x.copy_((x.double() + upd).float())
        if x_bf16_out is not None:
            x_bf16_out[:, :C] = bf(x0 if "image before the MLP residual" in self.faults else x)
            room = x_bf16_out.untyped_storage().nbytes() // 2 - x_bf16_out.storage_offset() - M * x_bf16_out.stride(0)
            if "a row past the image" in self.faults and room >= C:           # (where the forward's side of the fault left room: once)
                x_bf16_out.as_strided((1, C), (x_bf16_out.stride(0), 1), x_bf16_out.storage_offset() + M * x_bf16_out.stride(0)).fill_(3.0)
        if next_linear is None:
            return x
        nx = next_linear
        src = x0 if "q_next before the MLP residual" in self.faults else x
        hn = bf(_ln64(src, nx.get("ln_w"), nx.get("ln_b"), nx.get("shift"), nx.get("scale"), nx.get("mod_sample_stride", 0), nx.get("rows_per_sample", 0)).float())
        q = self._mm(hn, nx["w"])
        return x, bf(q if nx.get("bias") is None else q + nx["bias"])

    def attention_fwd(self, q, k, v, B, H, Nq, Nk, head_dim, out=None):
        C = H * head_dim
        o = bf(kc.attention_ref64(q[:, :C], k[:, :C], v[:, :C], B, H, Nq, Nk, head_dim)[0].float()).contiguous()
        return self._into(out, o)

    def attention_oproj_resid_(self, q, k, v, B, H, Nq, Nk, head_dim, wo, bo, x, gate=None, gate_sample_stride=0):
        C = H * head_dim
        o = self.attention_fwd(q, k, v, B, H, Nq, Nk, head_dim).view(B * Nq, C)                # quirk Q1
        upd = self._mm(o, wo)
        if "fc_o bias dropped" not in self.faults:
            upd = upd + bo
        upd = upd.double()
        if gate is not None:
            upd = _krows(gate, gate_sample_stride, B * Nq, Nq) * upd
        x.copy_((x.double() + upd).float())
        return x

    def actnorm_(self, x, shift, log_scale, B):
        v = (x.double().reshape(B, -1) - shift.double().reshape(-1)) * torch.exp(-log_scale.double().reshape(-1))
        x.copy_(v.float().reshape(x.shape))
        return x

    def maxpool(self, x, G, n):
        return kc.maxpool_expr(x, G, n)

    def fps(self, xyz, m, skip_near_origin=None):
        from oracle import ldt_oracle as O
        return O.fps(xyz, m, skip_near_origin=self.FPS_SKIP_NEAR_ORIGIN if skip_near_origin is None else skip_near_origin).int()

    def knn(self, xyz, centers, k, return_dist=False):
        from oracle import ldt_oracle as O
        return O.knn(k, xyz, centers).int()

    def gather_rows(self, src, idx):
        return torch.gather(src, 1, idx.long()[:, :, None].expand(-1, -1, src.shape[2]))

    def norm_points(self, xyz):
        return kc.norm_points_ref(xyz)[0].float()

    def group_normalize(self, feat, xyz, fps_idx, knn_idx, alpha, beta, normalize="anchor", return_stats=False):
        B, n, D = feat.shape
        S, k = knn_idx.shape[1], knn_idx.shape[2]
        ref = kc.group_reference(feat, xyz, fps_idx, knn_idx, alpha, beta, normalize)
        U = torch.zeros(B * S * k, kc.pad64(2 * D + 3), dtype=torch.bfloat16)
        U[:, :D + 3] = bf(ref["pre"].float()).reshape(-1, D + 3)
        U[:, D + 3:2 * D + 3] = bf(ref["anchor"].float())[:, :, None, :].expand(-1, -1, k, -1).reshape(-1, D)
        return U

    def grouper_mlp(self, feat, xyz, fps_idx, knn_idx, alpha, beta, wimg, b1, b2, b3, out=None):
        w1, w2, w3 = self.panels[id(wimg)] if hasattr(self, "panels") else (None, None, None)
        g = kc.group_reference(feat, xyz, fps_idx, knn_idx, alpha, beta)
        return self._into(out, kc.grouper_staged_reference(g, w1, b1, w2, b2, w3, b3)["ref"].float())

    def mixture_seed(self, eps, sig, mu, logits):
        return kc.mixture_seed_ref(eps, sig, mu, logits)[0].float()

    def reparam(self, post, noise, out, lo, hi, want_stats=False):
        mu, lv, ref, _ = kc.reparam_ref(post, noise.reshape(post.shape[0], -1), lo, hi)
        out.copy_(ref.float())
        return (mu, lv) if want_stats else (None, None)

    def reparam_kl(self, post, noise, out, lo, hi, rows_per_sample, want_stats=False):
        mu, lv, ref, _ = kc.reparam_ref(post, noise.reshape(post.shape[0], -1), lo, hi)
        out.copy_(ref.float())
        lq, _, kl, _ = kc.reparam_kl_ref(out, mu, lv)
        kl = kl.float()
        ks = kl.double().reshape(-1, rows_per_sample * kl.shape[1]).sum(1).float()
        return (mu if want_stats else None), (lv if want_stats else None), kl, lq.float(), ks

    def philox_normal(self, shape, device, seed, step=0, elem_offset=0):
        n = 1
        for s in shape:
            n *= s
        return torch.as_tensor(kc.philox_normal_ref(seed, step, elem_offset // 4, n // 4)[0]).float().reshape(shape)

    def add_f32(self, a, b, out=None):
        return self._into(out, a + b)


# ------------------------------------------------------------------------------------------------------------- planted faults between step and tape
class Plant:
    """One planted fault in front of `inner` (test_compressor_tape_host.Plant's scheme: the forward hands over a wrong operand, the kernel is
    right on what it gets).  sigs: where the entry points' signatures are read."""

    def __init__(self, inner, fault, ctx, sigs):
        self._inner, self._fault, self._ctx, self._sigs, self._n, self._state = inner, fault, ctx, sigs, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        handler = STEP_FAULTS.get(self._fault, {}).get(name)
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


def _eps_one_level_off(A, call, n, ctx, st):
    a = A["a"]
    if tuple(a.shape) == (ctx["B"] * ctx["T"], ctx["z"]) and a.stride(0) == ctx["L"] * ctx["z"] and a.storage_offset() == ctx["z"]:
        A["a"] = _shift(a, -ctx["z"])                                       # level 1 reads level 0's latents
    return call()


def _kv_swapped(A, call, n, ctx, st):
    if n == 1:
        A["k"], A["v"] = A["v"], A["k"]
    return call()


def _gate_stride_zero(A, call, n, ctx, st):
    if n == 1 and A["gate"] is not None:
        A["gate_sample_stride"] = 0
    return call()


def _rows_per_sample_one(A, call, n, ctx, st):
    """rows_per_sample = 1 on the first gated residual GEMM; the gate rows get storage for one row per output row (the kernel would read past
    the B modulation rows: on the CPU that cannot be planted otherwise)."""
    from ldt_amd._lib import EPI_RESID_F32
    if A["epilogue"] == EPI_RESID_F32 and A["gate"] is not None and "done" not in st:
        st["done"] = True
        g, M = A["gate"], A["x"].shape[0]
        big = torch.zeros(M, A["gate_sample_stride"])
        big[:, :g.shape[1]] = g[torch.arange(M) % g.shape[0]]
        A["gate"], A["rows_per_sample"] = big[:, :g.shape[1]], 1
    return call()


def _actnorm_skipped(A, call, n, ctx, st):
    return A["x"]


def _actnorm_twice(A, call, n, ctx, st):
    call()
    return call()


def _final_shift_scale_swapped(A, call, n, ctx, st):
    if A["shift"] is not None and A["mod_sample_stride"] == 2 * ctx["C"] and "done" not in st:
        st["done"] = True
        A["shift"], A["scale"] = A["scale"], A["shift"]
    return call()


def _level0_reads_the_set(A, call, n, ctx, st):
    P = ctx["model"].packed()
    if A["w"] is P["dec"][ctx["L"] - 1]["att"]["wkv"]:                      # level 0's posterior block
        o0 = P["prior"].unsqueeze(0).expand(ctx["B"], -1, -1).reshape(-1, ctx["C"])
        A["x"] = kc.cast_pad_want(o0.contiguous(), kc.pad64(ctx["C"]))[:A["x"].shape[0]].contiguous()
    return call()


def _roomy_image(A, call, n, ctx, st):
    """The forward's side of `one row written past x_bf16_out`: the image gets a row of storage behind it, so that the emulated kernel's
    stray store lands in memory the tape watches."""
    mine = A["x_bf16_out"]
    if mine is None or "done" in st:
        return call()
    st["done"] = True
    big = torch.zeros(mine.shape[0] + 1, mine.shape[1], dtype=mine.dtype)
    A["x_bf16_out"] = big[:mine.shape[0]]
    r = call()
    mine.copy_(big[:mine.shape[0]])
    return r


STEP_FAULTS = {
    "eps_j one level off": {"sgemm": _eps_one_level_off},
    "K and V halves swapped": {"attention_oproj_resid_": _kv_swapped},
    "gate_sample_stride 0": {"attention_oproj_resid_": _gate_stride_zero},
    "rows_per_sample 1": {"gemm_bf16": _rows_per_sample_one},
    "ActNorm skipped": {"actnorm_": _actnorm_skipped},
    "ActNorm twice": {"actnorm_": _actnorm_twice},
    "FinalLayer shift and scale swapped": {"layernorm_modulate": _final_shift_scale_swapped},
    "level 0 attends to o_bf": {"gemm_bf16": _level0_reads_the_set},
    "roomy image": {"ln_mlp_resid_": _roomy_image},
}


# ------------------------------------------------------------------------------------------------------------- driving the forwards
class Dev(str):
    """A device string that answers `.type` with "cuda": the forwards refuse host parameters before they launch anything."""
    type = "cuda"


def drive(tiny_cfg, which="fused", mode="forward", emu=None, step_fault=None, want_kl=False, given_noise=True, dropped=False):
    over, B, N = it.CASES[which]
    model, cfg = it.make_case(tiny_cfg.compressor, **over)
    emu = IEmu() if emu is None else emu
    tape = tt.Tape(emu)
    T, z, Ld = model.z_scales, model.z_dim, model.n_layers
    ctx = dict(model=model, B=B, T=T, z=z, L=Ld, C=model.hidden_dim, N=N)
    g = torch.Generator().manual_seed(9)
    npts = it.DROPPED if dropped else model.outsize
    r = dict(model=model, tape=tape, mode=mode, B=B, want_kl=want_kl, npts=npts, keep=None)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(type(model), "_device", lambda self: Dev("cpu"))
        tt.install_infer_ops(mp, tape)
        P = model.packed()
        if "wimg" in P["group"]:
            G, D = P["group"], model.hidden_dim
            emu.panels = {id(G["wimg"]): (G["w_pre1"][:, :2 * D + 3].float(), G["w_pre2"][:, :D].float(), G["w_pre3"][:, :D].float())}
        tt.install_infer_ops(mp, tape if step_fault is None else Plant(tape, step_fault, ctx, emu))
        tape.mark("forward")
        if mode == "forward":
            r["x"] = it.clouds(B, N, 3)
            r["post_noise"] = [torch.randn(B, T, z, generator=g) for _ in range(Ld)] if given_noise else None
            torch.manual_seed(4)
            r["res"] = model(r["x"], num_points=npts, post_noise=r["post_noise"], want_kl=want_kl, want_stats=want_kl)
            if dropped:                                                     # the rows the forward drew first (Network.py:215 before :220)
                torch.manual_seed(4)
                r["keep"] = model._presence(B, npts)
        else:
            r["eps"] = torch.randn(B, T, Ld * z, generator=g)
            if dropped:
                r["keep"] = torch.stack([torch.randperm(model.max_outputs, generator=g) < npts for _ in range(B)])
            torch.manual_seed(4)
            r["out"] = model.sample((B, npts), given_eps=r["eps"], keep_mask=r["keep"])
    return r


def audit(r, numeric=True):
    m, tape = r["model"], r["tape"]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(type(m), "_device", lambda self: Dev("cpu"))
        calls = tape.since("forward")
        worst = it.audit_numeric(tape.calls, it.grouper_ctx(m)) if numeric else {}
        if r["mode"] == "forward":
            it.audit_forward(calls, m, r["x"], r["res"], post_noise=r["post_noise"], keep_mask=r["keep"], want_kl=r["want_kl"], num_points=r["npts"])
        else:
            it.audit_sample(calls, m, r["B"], r["npts"], r["eps"], r["out"], keep_mask=r["keep"])
    return worst


# ------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("which,mode,want_kl", [("fused", "forward", False), ("fused", "forward", True), ("chain", "forward", False), ("grouped", "forward", True),
                                                ("fused", "sample", False), ("chain", "sample", False)])
def test_emulated_forward_passes_both_audits_in_both_orders(tiny_cfg, which, mode, want_kl, rev):
    r = drive(tiny_cfg, which, mode, IEmu(rev), want_kl=want_kl, given_noise=which != "chain", dropped=which == "fused" and (want_kl or mode == "sample"))
    worst = audit(r)
    bad = {k: v for k, v in it.ratios(worst).items() if v > 1.0}
    assert not bad, bad
    names = {c.name for c in r["tape"].since("forward")}
    want = {("fused", "forward"): {"ln_linear", "ln_mlp_resid_", "attention_oproj_resid_", "group_normalize", "actnorm_", "reparam_kl" if want_kl else "reparam"},
            ("chain", "forward"): {"layernorm_modulate", "attention_fwd", "mixture_seed", "norm_points", "philox_normal", "cast_pad_bf16"},
            ("grouped", "forward"): {"grouper_mlp", "group_stats", "norm_apply", "block_activation_"},
            ("fused", "sample"): {"ln_mlp_resid_", "attention_oproj_resid_"}, ("chain", "sample"): {"mixture_seed", "attention_fwd"}}[(which, mode)]
    assert want <= names, "this case no longer reaches %s" % sorted(want - names)


def test_the_cases_together_reach_every_entry_point(tiny_cfg):
    seen = set()
    for which, mode, kl in (("fused", "forward", False), ("fused", "forward", True), ("chain", "forward", False), ("grouped", "forward", False), ("fused", "sample", False)):
        seen |= {c.name for c in drive(tiny_cfg, which, mode, want_kl=kl, given_noise=which != "chain")["tape"].calls}
    assert it.REACHABLE <= seen, "this case no longer reaches %s" % sorted(it.REACHABLE - seen)
    assert seen <= it.REACHABLE | {"add_f32"}, "entry points the hand-written set does not know: %s" % sorted(seen - it.REACHABLE)


def test_reordered_independent_calls_pass(tiny_cfg):
    """The K | V projections and the casts hang off the chain: listed first or last, the table finds them by what they read."""
    r = drive(tiny_cfg, "fused")
    tape = r["tape"]
    calls = tape.since("forward")
    side = [c for c in calls if c.name in ("cast_pad_bf16", "sgemm")]
    tape.calls[tape.marks["forward"]:] = side[::-1] + [c for c in calls if c.name not in ("cast_pad_bf16", "sgemm")]
    audit(r, numeric=False)


def test_a_call_kind_without_a_reference_is_refused():
    with pytest.raises(AssertionError, match=r"emd_approx.*a call kind the audit has no reference for"):
        it.check_call(tt.Call(0, "emd_approx", {"x": tt.Rec(torch.ones(2, 2))}))


def test_the_training_tapes_record_as_before(tiny_cfg):
    """The two additions to the tape (x_bf16_out in place, attention_oproj_resid_'s x) name operands no training entry point has."""
    from ldt_amd import ops
    for name in dir(ops):
        fn = getattr(ops, name)
        if callable(fn) and not isinstance(fn, type) and not name.startswith("_") and "x_bf16_out" in inspect.signature(fn).parameters:
            assert name in ("ln_mlp_resid_",), name
    assert set(tt.WRITES) == {"attention_oproj_resid_"}


PLANTED = [  # name, case, mode, dict(step_fault / emu faults), what the message must name
    ("x_bf16_out written from x before the MLP residual", "fused", dict(emu=["image before the MLP residual"]),
     r"call #\d+ ln_mlp_resid_.*the bf16 image `x_bf16_out` is not bf16 of the x this call left behind"),
    ("q_next from the pre-residual x", "fused", dict(emu=["q_next before the MLP residual"]), r"call #\d+ ln_mlp_resid_.*q_next against LN \+ linear of the x this call left behind"),
    ("eps_j one level off", "fused", dict(step_fault="eps_j one level off"),
     r"sgemm.*operand `a` must be (the view of )?columns \[1 z, 2 z\) of the latents the posterior wrote at level 1"),
    ("K and V halves swapped", "fused", dict(step_fault="K and V halves swapped"), r"attention_oproj_resid_.*operand `k` must be columns \[0 C, 1 C\) of K \| V of block 0 of encoder stage 0: K"),
    ("gate_sample_stride 0", "fused", dict(step_fault="gate_sample_stride 0"), r"attention_oproj_resid_.*operand `gate_sample_stride` must be 384, the row stride of the modulation rows: the gate"),
    ("rows_per_sample 1 instead of Nq", "chain", dict(step_fault="rows_per_sample 1"), r"gemm_bf16.*operand `rows_per_sample` must be 8, the rows one gate row is broadcast over"),
    ("fc_o's bias dropped", "fused", dict(emu=["fc_o bias dropped"]), r"call #\d+ attention_oproj_resid_"),
    ("ActNorm skipped", "fused", dict(step_fault="ActNorm skipped"), r"ActNorm must be applied exactly once before the first encoder block: 0 actnorm_"),
    ("ActNorm applied twice", "fused", dict(step_fault="ActNorm twice"), r"ActNorm must be applied exactly once before the first encoder block: 2 actnorm_"),
    ("FinalLayer's shift and scale swapped", "fused", dict(step_fault="FinalLayer shift and scale swapped"),
     r"layernorm_modulate.*operand `shift` must be columns \[0 C, 1 C\) of the modulation rows: the shift of the FinalLayer of encoder stage 0"),
    ("level 0's posterior attending to o_bf", "fused", dict(step_fault="level 0 attends to o_bf"),
     r"gemm_bf16.*operand `x` must be the bf16 cast of this level's encoder output \(level 0 attends to itself\)"),
    ("a write one row past a destination view", "fused", dict(step_fault="roomy image", emu=["a row past the image"]), r"ln_mlp_resid_.*outside the destination view\(s\) `x`|ln_mlp_resid_.*outside the destination view\(s\) `x_bf16_out`"),
]


@pytest.mark.parametrize("name,which,plant,names", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_faults_fail_the_audit_naming_the_call_or_the_link(tiny_cfg, name, which, plant, names):
    r = drive(tiny_cfg, which, "forward", IEmu(faults=plant.get("emu", ())), plant.get("step_fault"))
    # a fault between the forward and the tape leaves every kernel right on what it was handed: the table alone is asked
    with pytest.raises(AssertionError, match=names):
        audit(r, numeric="emu" in plant)


# ------------------------------------------------------------------------------------------------------------- the Score forward, by stage
def emulated_score_forward(emu, S, dims, W, x, table, blocks, step_stride, sample_stride, step, faults=()):
    """`score_forward_impl`'s unfolded branch (csrc/api.hip) over the workspace dict W, on the emulated entry points: the same buffers reused
    across blocks, the AdaLN offsets m + k D into the flat table.  -> eps_out."""
    from ldt_amd._lib import EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_F32
    B, T, D, H, L, z = dims
    M, dh = B * T, D // H
    flat = table.reshape(-1)
    base = (step or 0) * step_stride
    nS = B if sample_stride else 1

    def rows(off):                                                          # [nS, D] at base + s sample_stride + off
        return flat.as_strided((nS, D), (sample_stride if sample_stride else D, 1), base + off) if nS > 1 else flat[base + off:base + off + D].reshape(1, D)

    kw = dict(mod_sample_stride=sample_stride, rows_per_sample=T if sample_stride else M)
    gk = dict(gate_sample_stride=sample_stride, rows_per_sample=T if sample_stride else M)
    xin = emu.cast_pad_bf16(x.reshape(M, z).float(), S["w_in"].shape[1])
    emu.gemm_bf16(xin, S["w_in"], S["b_in"], EPI_F32, out=W["X"])
    for l in range(blocks):
        Sb, m = S["blocks"][l], l * 6 * D
        emu.layernorm_modulate(W["X"], shift=rows(m), scale=rows(m + D), out=W["Hb"], **kw)
        cross = "kv" in Sb
        N = D if cross else 3 * D
        emu.gemm_bf16(W["Hb"], Sb["w_q"] if cross else Sb["w_qkv"], Sb["b_q"] if cross else Sb["b_qkv"], EPI_BF16, out=W["QKV"][:, :N])
        q = W["QKV"][:, :D]
        k, v, Nk = (Sb["kv"][:, :D], Sb["kv"][:, D:], Sb["kv"].shape[0] // B) if cross else (W["QKV"][:, D:2 * D], W["QKV"][:, 2 * D:], T)
        if "QKV read with the wrong batch stride" in faults and not cross and l == 1:
            k, v = k.reshape(B, T, D).roll(1, 0).reshape(M, D), v.reshape(B, T, D).roll(1, 0).reshape(M, D)
        if not ("Ob of the previous block reused" in faults and l == 1):
            W["Ob"].copy_(emu.attention_fwd(q, k, v, B, H, T, Nk, dh).reshape(M, D))
        emu.gemm_bf16(W["Ob"], Sb["w_o"], Sb["b_o"], EPI_RESID_F32, out=W["X"], resid=W["X"], gate=rows(m + 2 * D), **gk)
        off = D if ("mod offset off by D" in faults and l == 1) else 0
        emu.layernorm_modulate(W["X"], shift=rows(m + 3 * D + off), scale=rows(m + 4 * D + off), out=W["Hb"], **kw)
        emu.gemm_bf16(W["Hb"], Sb["w_up"], Sb["b_up"], EPI_GELU_BF16, out=W["U"])
        emu.gemm_bf16(W["U"], Sb["w_dn"], Sb["b_dn"], EPI_RESID_F32, out=W["X"], resid=W["X"], gate=rows(m + 5 * D), **gk)
    m = blocks * 6 * D
    emu.layernorm_modulate(W["X"], shift=rows(m), scale=rows(m + D), out=W["Hb"], **kw)
    return emu.gemm_bf16(W["Hb"], S["w_out"], S["b_out"], EPI_F32, n=z).reshape(B, T, z)


def score_twin(tiny_cfg, blocks=2, B=3, T=8, cond_tokens=0, shared=False, faults=(), rev=False):
    import ldt_amd.score as sm
    emu = IEmu(rev)
    model, x, _, _, _ = tt.make_case(tiny_cfg.score, 128, 2, blocks, B, T, 1, None)
    D, H, z = model.hidden_size, model.num_heads, model.z_dim
    g = torch.Generator().manual_seed(21)
    kv = {l: bf(torch.randn(B * cond_tokens, 2 * D, generator=g)) for l in range(0, blocks, 2)} if cond_tokens else None
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(type(model), "_device", lambda self: Dev("cpu"))
        mp.setattr(sm, "ops", emu)
        S = it.score_panels(model, kv)
    n_mod = model.n_mod
    mod = 0.3 * torch.randn(9 if shared else B, n_mod, generator=g)
    step_stride, sample_stride, step = (n_mod, 0, 7) if shared else (0, n_mod, None)
    dims = (B, T, D, H, blocks, z)
    F = S["blocks"][0]["w_up"].shape[0]

    def run(n, table):
        W = {"X": torch.full((B * T, D), float("nan")), "Hb": torch.full((B * T, D), float("nan"), dtype=torch.bfloat16),
             "QKV": torch.full((B * T, 3 * D), float("nan"), dtype=torch.bfloat16), "Ob": torch.full((B * T, D), float("nan"), dtype=torch.bfloat16),
             "U": torch.full((B * T, F), float("nan"), dtype=torch.bfloat16)}
        eps = emulated_score_forward(emu, S, dims, W, x, table, blocks if n is None else n, step_stride, sample_stride, step, faults)
        return dict(W, eps=eps)
    return it.audit_score_stages(run, S, dims, x, mod, sample_stride, step)


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(blocks=4, cond_tokens=24), dict(shared=True), dict(blocks=1)], ids=["tiny", "cross", "table-row-7", "one-block"])
def test_emulated_score_forward_passes_the_stage_audit(tiny_cfg, kw, rev):
    worst, two = score_twin(tiny_cfg, rev=rev, **kw)
    bad = {k: v for k, v in it.ratios(worst).items() if v > 1.0}
    assert not bad, bad
    assert all(two.values()) and {"LN1 Hb", "QKV (two kernels)", "fc_o X_mid", "mlp.out X_next", "FinalLayer eps_out"} <= set(worst)


@pytest.mark.parametrize("fault,names", [
    ("mod offset off by D", r"score stage `LN2 \+ mlp\.fc \+ GELU` of block 1"),
    ("Ob of the previous block reused", r"score stage `q \| k \| v \+ attention` of block 1"),
    ("QKV read with the wrong batch stride", r"score stage `q \| k \| v \+ attention` of block 1"),
])
def test_planted_score_faults_name_the_stage_and_the_block(tiny_cfg, fault, names):
    with pytest.raises(AssertionError, match=names):
        score_twin(tiny_cfg, faults=(fault,))
