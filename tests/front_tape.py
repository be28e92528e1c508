"""The front training step audited in situ (tests/test_gpu_front_tape.py), after tests/compressor_tape.py: a recording stand-in for the
`ops` of ldt_amd/compressor_train.py keeps every call of one FrontTrainStep forward + backward with its operands as they were BEFORE the call
(a backward kernel may write over its own input) and what it returned; `audit` then holds each call per element against its float64
reference ON THE OPERANDS THE TAPE HANDED IT (tests/front_train_checks.py, tests/kernel_checks.py).  Selections never differ between the two
sides: a call is judged on its own inputs, the BatchNorm backward's mask from the fp32 arithmetic of the x and the statistics it was given.

What the per-kernel tests cannot see and this does: the operands as the step forms them (strided views of padded bf16 rows, `.grad` views of
an optimizer's flat buffer, dx aliasing dy), and the links — which saved tensor goes into which call."""
import torch

import front_train_checks as fc
import kernel_checks as kc


class Recorder:
    """Stands in for a module's `ops`: every callable is wrapped, its tensor arguments cloned before the call, its result after."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not callable(f):
            return f
        snap = lambda v: v.detach().clone() if torch.is_tensor(v) else (tuple(snap(e) for e in v) if isinstance(v, tuple) else v)

        def wrapped(*a, **kw):
            before = ([snap(v) for v in a], {k: snap(v) for k, v in kw.items()})
            out = f(*a, **kw)
            self.calls.append({"name": name, "args": before[0], "kw": before[1], "out": snap(out),
                               "after": ([snap(v) for v in a], {k: snap(v) for k, v in kw.items()})})
            return out
        return wrapped


def _cpu(t):
    return t.detach().cpu()


def check_call(c):
    """-> (kind, worst err / tol) of one recorded call, or None for calls that move data only."""
    n, a, kw, out = c["name"], c["args"], c["kw"], c["out"]
    if n == "bn_stats":
        x, rm, rv = _cpu(a[0]), _cpu(a[2]), _cpu(a[3])
        ref, tol = fc.bn_stats_ref(x, rm, rv, eps=a[1], momentum=a[4])
        got = {"mean": _cpu(out)[0], "rstd": _cpu(out)[1], "running_mean": _cpu(c["after"][0][2]), "running_var": _cpu(c["after"][0][3])}
        return n, max(kc.assert_elementwise(got[k], ref[k], tol[k], "tape bn_stats " + k) for k in ref)
    if n == "bn_relu_fwd":
        x, st, g, b = (_cpu(t) for t in a[:4])
        bf = out.dtype == torch.bfloat16
        ref, tol = fc.bn_relu_fwd_ref(x, st, g, b, bf)
        C = x.shape[1]
        assert bool((out[:, C:].float() == 0).all())
        return n, kc.assert_elementwise(_cpu(out)[:, :C].float(), ref, tol, "tape bn_relu_fwd")
    if n == "bn_relu_bwd":
        dy, x, st, g, b = (_cpu(t) for t in a[:5])
        ref, tol = fc.bn_relu_bwd_ref(dy, x, st, g, b)
        return n, max(kc.assert_elementwise(_cpu(o), r, t, "tape bn_relu_bwd " + nm) for o, r, t, nm in zip(out, ref, tol, ("dx", "dgamma", "dbeta")))
    if n == "maxpool_argmax":
        x, G, k = _cpu(a[0]).float(), a[1], a[2]
        want, arg = fc.maxpool_argmax_ref(x, G, k)
        if kw.get("relu"):
            want = want.clamp_min(0)
        assert torch.equal(_cpu(out[0]), want) and torch.equal(_cpu(out[1]), arg), "tape maxpool_argmax"
        return n, 0.0
    if n == "maxpool_relu_bwd":
        assert torch.equal(_cpu(out), fc.maxpool_relu_bwd_ref(_cpu(a[0]), _cpu(a[1]), _cpu(a[2]), a[3])), "tape maxpool_relu_bwd"
        return n, 0.0
    if n == "group_normalize_bwd":
        dU, feat, xyz, fi, ki, al = (_cpu(t) for t in a[:6])
        D = feat.shape[2]
        case = dict(feat=feat, xyz=xyz, fi=fi, ki=ki, alpha=al, dU=dU[:, :2 * D + 3].contiguous())
        ref, tol = fc.group_normalize_bwd_ref(case)
        return n, max(kc.assert_elementwise(_cpu(o), r, t, "tape group_normalize_bwd " + nm) for o, r, t, nm in zip(out, ref, tol, ("dalpha", "dbeta", "dfeat")))
    if n == "colsum":
        ref, tol = kc.colsum_ref(_cpu(a[0]).float())
        return n, kc.assert_elementwise(_cpu(out), ref, tol, "tape colsum")
    if n == "wgrad":
        ref, tol = kc.wgrad_ref(_cpu(a[0]), _cpu(a[1]))
        return n, kc.assert_elementwise(_cpu(out), ref, tol, "tape wgrad")
    if n == "dgrad":
        ref, tol = kc.dgrad_ref(_cpu(a[0]), _cpu(a[1]))
        return n, kc.assert_elementwise(_cpu(out), ref, tol, "tape dgrad")
    if n == "sgemm":
        x, w = _cpu(a[0]), _cpu(a[1])
        bias = _cpu(a[2]) if len(a) > 2 and a[2] is not None else None
        ref, tol = kc.sgemm_ref(x, w, bias)
        return n, kc.assert_elementwise(_cpu(out), ref, tol, "tape sgemm")
    if n == "gemm_bf16":
        x, w, bias, epi = _cpu(a[0]), _cpu(a[1]), _cpu(a[2]), a[3]
        ref = x.double() @ w.double().T + bias.double()
        tol = kc.gemm_tol(x, w, bias, x.shape[1], torch.float32)
        if "resid" in kw:                                               # EPI_RESID_F32: out = resid + (x w^T + b), one more rounding
            r = _cpu(kw["resid"]).double()
            ref = ref + r
            tol = tol + kc.U24 * (ref.abs() + r.abs())
        return n, kc.assert_elementwise(_cpu(out), ref, tol, "tape gemm_bf16 epilogue %d" % epi)
    if n == "add_f32":
        assert torch.equal(_cpu(out), _cpu(a[0]) + _cpu(a[1])), "tape add_f32"
        return n, 0.0
    return None


def audit(calls):
    """Every recorded call against its reference -> {kind: (count, worst err / tol)}."""
    worst = {}
    for c in calls:
        r = check_call(c)
        if r is not None:
            cnt, w = worst.get(r[0], (0, 0.0))
            worst[r[0]] = (cnt + 1, max(w, r[1]))
    return worst


# the calls one forward + backward makes, by kind (the links: a dropped or doubled call shows here)
EXPECTED = {"bn_stats": 4, "bn_relu_fwd": 5, "bn_relu_bwd": 4, "maxpool_argmax": 2, "maxpool_relu_bwd": 2, "group_normalize_bwd": 1, "add_f32": 1,
            "gemm_bf16": 3, "wgrad": 3, "dgrad": 3, "colsum": 7, "sgemm": 10}
