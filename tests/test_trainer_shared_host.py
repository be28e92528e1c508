"""CPU: the steps the three trainer modules share (ldt_amd/evalloop.py and the draw / EMA helpers of `ldt_amd.Trainer`), held on CPU trainers
with `sample`, the Compressor call, the Score step and `ldt_amd.metrics.compute_all_metrics` stubbed — the pattern of
test_host_logic.py::test_valsample_has_the_reference_signature_and_loader_semantics.  The first part characterises the evaluation loops, the
`update` protocol and the checkpoint path as they were before the shared module existed (the GPU suite alone held them then); the second part
holds the shared time draw and the EMA scope against restated expressions."""
import copy
import os

import numpy as np
import pytest
import torch


def _cfg(tiny_cfg, tmp_path, ncat=1, test_batch_size=None):
    c = copy.deepcopy(tiny_cfg)
    c.log.save_path = str(tmp_path)
    c.data.num_categorys = ncat
    if test_batch_size:
        c.data.test_batch_size = test_batch_size
    return c


def _trainer(cfg, cls="Trainer"):
    import ldt_amd
    return getattr(ldt_amd, cls)(cfg, ldt_amd.Score(cfg.score), ldt_amd.Compressor(cfg.compressor), "cpu")


def _compressor_trainer(cfg):
    import ldt_amd
    return ldt_amd.CompressorTrainer(cfg, ldt_amd.Compressor(cfg.compressor), "cpu")


def _loader(P, cates):
    """Dict batches with every de-normalisation field the loaders carry, each distinct, so that a wrong pair shows."""
    g = torch.Generator().manual_seed(3)
    out = []
    for c in cates:
        B = len(c)
        out.append({"te_points": torch.randn(B, P, 3, generator=g), "tr_points": torch.randn(B, P, 3, generator=g),
                    "shift": torch.randn(B, 1, 3, generator=g), "scale": torch.rand(B, 1, 1, generator=g) + 0.5,
                    "mean": torch.randn(B, 1, 3, generator=g) + 4.0, "std": torch.rand(B, 1, 1, generator=g) + 2.5,
                    "cate_idx": torch.tensor(c)})
    return out


def _cat(loader, key, cate=None):
    return torch.cat([d[key] if cate is None else d[key][d["cate_idx"] == cate] for d in loader], 0)


@pytest.fixture
def metrics(monkeypatch):
    """`compute_all_metrics` replaced where the trainers look it up; -> the dict the stub fills with what it was handed."""
    import ldt_amd.compressor_trainer as ct
    import ldt_amd.metrics as Mx
    seen = {}

    def fake_metrics(smp, ref, batch_size):
        seen.update(smp=smp.clone(), ref=ref.clone(), batch_size=batch_size)
        return {"mmd-CD": torch.tensor(0.25), "cov-CD": 0.5}

    monkeypatch.setattr(Mx, "compute_all_metrics", fake_metrics)
    monkeypatch.setattr(ct, "compute_all_metrics", fake_metrics, raising=False)      # (a module that bound the name at import)
    return seen


WANT_RES = {"val/gen/mmd-CD": 0.25, "val/gen/cov-CD": 0.5}


class StubModel:
    """A Compressor whose reconstruction is a known function of its input; records (batch, label) per call."""

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def __call__(self, x, *args, **kw):
        assert args == () and set(kw) <= {"label"}
        self.calls.append((x.clone(), kw.get("label")))
        return {"set": 2.0 * x + 1.0, "all_eps": torch.zeros(x.shape[0], 2, 3)}


# ------------------------------------------------------------------------------------------------ HybridTrainer.valsample
def _stub_sample(tr, P, calls):
    def fake_sample(num_samples, label=None, condition=None, **kw):
        assert condition is None and kw == {}
        calls.append((num_samples, None if label is None else label.clone()))
        return torch.full((num_samples, P, 3), float(len(calls)))
    tr.sample = fake_sample


def test_hybrid_valsample_single_category(tiny_cfg, tmp_path, metrics, capsys):
    P = tiny_cfg.data.tr_max_sample_points
    tr = _trainer(_cfg(tiny_cfg, tmp_path), "HybridTrainer")
    calls = []
    _stub_sample(tr, P, calls)
    loader = _loader(P, [[0, 0, 0], [0, 0]])
    assert tr.valsample(loader) == WANT_RES
    assert [c[0] for c in calls] == [3, 2] and all(c[1] is None for c in calls)       # one sample() per batch, of len(tr_points), no label
    want_smp = torch.cat([torch.full((3, P, 3), 1.0), torch.full((2, P, 3), 2.0)], 0)
    assert torch.equal(metrics["smp"], want_smp) and torch.equal(metrics["ref"], _cat(loader, "te_points")) and metrics["batch_size"] == 64
    assert torch.equal(tr.last_valsample["samples"], want_smp) and torch.equal(tr.last_valsample["refs"], _cat(loader, "te_points"))
    assert os.listdir(str(tmp_path)) == ["smp{:}_ep1.npy"]                             # upstream's literal name
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "smp{:}_ep1.npy")), want_smp.numpy())
    out = capsys.readouterr().out
    assert "Sample rate:" in out and "Validation Sample (unit) Epoch:1" in out


def test_hybrid_valsample_by_category_does_not_cut_and_refuses_an_empty_category_first(tiny_cfg, tmp_path, metrics):
    P = tiny_cfg.data.tr_max_sample_points
    tr = _trainer(_cfg(tiny_cfg, tmp_path, ncat=55, test_batch_size=3), "HybridTrainer")
    calls = []
    _stub_sample(tr, P, calls)
    loader = _loader(P, [[13, 2, 13], [13, 13]])
    assert tr.valsample(loader, val_cate=13) == WANT_RES
    assert [c[0] for c in calls] == [3, 3]                                            # ceil(4 / 3) batches of test_batch_size
    assert all(torch.equal(c[1], torch.full((3,), 13, dtype=torch.int32)) for c in calls)
    assert metrics["smp"].shape == (6, P, 3) and metrics["batch_size"] == 64          # NOT cut to len(ref) = 4
    assert torch.equal(metrics["ref"], _cat(loader, "te_points", 13)) and metrics["ref"].shape[0] == 4
    assert np.load(os.path.join(str(tmp_path), "smp{:}_ep1.npy")).shape == (6, P, 3)
    calls.clear()
    with pytest.raises(ValueError, match="cate_idx == 7"):
        tr.valsample(loader, val_cate=7)
    assert calls == []                                                                # refused before anything was sampled


# ------------------------------------------------------------------------------------------------ valrecon / reconstrustion
RECON = {  # who: (trainer, method, stubbed attribute, fields of the multi-category branch, label passed, metrics batch size)
    "valrecon": (lambda c: _trainer(c, "HybridTrainer"), "valrecon", "compressor", ("mean", "std"), False, 256),
    "reconstrustion": (_compressor_trainer, "reconstrustion", "model", ("shift", "scale"), True, 128),
}


@pytest.mark.parametrize("who", sorted(RECON))
def test_reconstruction_single_category(tiny_cfg, tmp_path, metrics, who):
    make, method, attr, _, _, bsize = RECON[who]
    P = tiny_cfg.data.tr_max_sample_points
    tr = make(_cfg(tiny_cfg, tmp_path))
    stub = StubModel()
    setattr(tr, attr, stub)
    loader = _loader(P, [[0, 0, 0], [0, 0]])
    assert getattr(tr, method)(loader) == WANT_RES
    assert [c[0].shape[0] for c in stub.calls] == [3, 2] and all(c[1] is None for c in stub.calls)      # batch by batch, no label
    assert torch.equal(torch.cat([c[0] for c in stub.calls], 0), _cat(loader, "te_points"))
    rec = torch.cat([(2.0 * d["te_points"] + 1.0) * d["scale"] + d["shift"] for d in loader], 0)         # shift / scale in both classes
    ref = torch.cat([d["te_points"] * d["scale"] + d["shift"] for d in loader], 0)
    assert torch.equal(metrics["smp"], rec) and torch.equal(metrics["ref"], ref) and metrics["batch_size"] == bsize
    assert os.listdir(str(tmp_path)) == ["rec_ep1.npy"]
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rec_ep1.npy")), rec.numpy())
    last = tr.last_valrecon if who == "valrecon" else tr.last_reconstruction
    assert torch.equal(last["rec"], rec) and torch.equal(last["ref"], ref)


@pytest.mark.parametrize("who", sorted(RECON))
def test_reconstruction_by_category(tiny_cfg, tmp_path, metrics, who):
    make, method, attr, (shift_key, scale_key), labelled, bsize = RECON[who]
    P = tiny_cfg.data.tr_max_sample_points
    tr = make(_cfg(tiny_cfg, tmp_path, ncat=3, test_batch_size=5))
    stub = StubModel()
    setattr(tr, attr, stub)
    loader = _loader(P, [[2, 0, 2, 1], [2, 2, 2, 2], [0, 1, 2, 0]])
    assert getattr(tr, method)(loader, val_cate=2) == WANT_RES
    pts, sh, sc = _cat(loader, "te_points", 2), _cat(loader, shift_key, 2), _cat(loader, scale_key, 2)
    assert pts.shape[0] == 7 and [c[0].shape[0] for c in stub.calls] == [5, 2]        # re-batched by test_batch_size
    assert torch.equal(torch.cat([c[0] for c in stub.calls], 0), pts)
    for x, label in stub.calls:
        if labelled:
            assert torch.equal(label, torch.full((x.shape[0],), 2, dtype=torch.int32))
        else:
            assert label is None
    rec, ref = (2.0 * pts + 1.0) * sc + sh, pts * sc + sh
    assert torch.equal(metrics["smp"], rec) and torch.equal(metrics["ref"], ref) and metrics["batch_size"] == bsize
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rec_ep1.npy")), rec.numpy())
    last = tr.last_valrecon if who == "valrecon" else tr.last_reconstruction
    assert torch.equal(last["rec"], rec) and torch.equal(last["ref"], ref)
    stub.calls.clear()
    with pytest.raises(ValueError, match="%s: no test shape has cate_idx == 5" % method):
        getattr(tr, method)(loader, val_cate=5)
    assert stub.calls == []


# ------------------------------------------------------------------------------------------------ CompressorTrainer.valsample
def test_compressor_valsample(tiny_cfg, tmp_path, metrics, capsys):
    # Runs only with the clock's synchronisation behind `_sync(device)`: before that, this loop called torch.cuda.synchronize() bare and
    # could not run on a CPU trainer.
    P = tiny_cfg.data.tr_max_sample_points
    tr = _compressor_trainer(_cfg(tiny_cfg, tmp_path, ncat=3))                        # (this loop has no category branch)
    calls = []

    def fake_sample(num_samples, num_points, given_eps=None):
        calls.append((num_samples, num_points, given_eps))
        return torch.full((num_samples, num_points, 3), float(len(calls)))
    tr.sample = fake_sample
    loader = _loader(P, [[2, 0, 1], [0, 2]])
    assert tr.valsample(loader, 48) == WANT_RES
    assert calls == [(3, 48, None), (2, 48, None)]
    want_smp = torch.cat([torch.full((3, 48, 3), 1.0), torch.full((2, 48, 3), 2.0)], 0)
    assert torch.equal(metrics["smp"], want_smp) and torch.equal(metrics["ref"], _cat(loader, "te_points")) and metrics["batch_size"] == 128
    assert os.listdir(str(tmp_path)) == ["smp_ep1.npy"]
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "smp_ep1.npy")), want_smp.numpy())
    assert "Sample rate:" in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="mitsuba"):
        tr.valsample(loader, 48, vis=True)


# ------------------------------------------------------------------------------------------------ update: the EMA protocol
class HostPoints:
    """Stands for data['tr_points']: `.to(device)` hands back host points whatever the device."""

    def to(self, *args, **kw):
        return torch.zeros(2, 64, 3)


@pytest.mark.parametrize("cls", ["Trainer", "CompletionTrainer"])
def test_update_swaps_ema_weights_from_the_second_iteration_on(tiny_cfg, tmp_path, monkeypatch, cls):
    tr = _trainer(_cfg(tiny_cfg, tmp_path), cls)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    tr.device = "cuda"                                                                # passes the device refusal; nothing below touches a device
    stub = StubModel()
    tr.compressor = stub
    swaps, steps = [], []
    monkeypatch.setattr(tr.optimizer, "swap_parameters_with_ema", lambda store_params_in_ema: swaps.append(store_params_in_ema))
    fail = []

    def fake_update_score(eps, condition=None, cates=None, discrete=False, **kw):
        assert kw == {} and cates is None
        steps.append(dict(swaps=len(swaps), encodes=len(stub.calls), discrete=discrete, condition=condition, eps=tuple(eps.shape)))
        if fail:
            raise KeyError("the step failed")
        return torch.tensor(1.5)
    tr.update_score = fake_update_score
    condition = (torch.zeros(2, 128, 4), 0.) if cls == "CompletionTrainer" else None
    data = {"tr_points": HostPoints()}
    assert float(tr.update(data, condition)) == 1.5
    assert swaps == [] and tr.itr == 1                                                # first iteration: no swap
    assert steps[-1] == dict(swaps=0, encodes=1, discrete=tiny_cfg.opt.discrete, condition=condition, eps=(2, 2, 3))
    assert float(tr.update(data, condition)) == 1.5
    assert swaps == [True, True] and tr.itr == 2                                      # in before the encode and the step, out after
    assert steps[-1]["swaps"] == 1 and steps[-1]["encodes"] == 2
    fail.append(1)
    with pytest.raises(KeyError, match="the step failed"):
        tr.update(data, condition)
    assert swaps == [True] * 4 and tr.itr == 2                                        # swapped back, itr untouched


# ------------------------------------------------------------------------------------------------ the checkpoint path
@pytest.mark.parametrize("cls", ["Trainer", "CompressorTrainer"])
def test_resume_takes_the_epoch_from_the_last_row_of_training_csv(tiny_cfg, tmp_path, monkeypatch, cls):
    cfg = _cfg(tiny_cfg, tmp_path)
    with open(os.path.join(str(tmp_path), "training.csv"), "w") as f:
        f.write("epoch,itr,loss,time\n3,10,0.5,1\n7.0,123,0.4,2\n")
    if cls == "Trainer":
        tr = _trainer(cfg)
        ckpt = {"score_state_dict": tr.model.state_dict(), "compressor_state_dict": tr.compressor.state_dict(),
                "score_optim_state_dict": {"state": {}, "param_groups": []}, "epoch": 7, "itr": 123, "time": 2.5}
    else:
        tr = _compressor_trainer(cfg)
        ckpt = {"state_dict": tr.model.state_dict(), "epoch": 7, "itr": 123, "time": 2.5}
    paths = []

    def fake_load(path, *args, **kw):
        paths.append(path)
        return ckpt
    monkeypatch.setattr(torch, "load", fake_load)
    tr.resume()
    assert paths == [os.path.join(str(tmp_path), "checkpt_7.pth")] and (tr.epoch, tr.itr, tr.time) == (8, 123, 2.5)
    tr.resume(epoch=3)
    assert paths[-1] == os.path.join(str(tmp_path), "checkpt_3.pth")


# ================================================================================================ the shared draw and the EMA scope
def test_draw_times_discrete_branch(tiny_cfg, tmp_path):
    tr = _trainer(_cfg(tiny_cfg, tmp_path))
    N, B = tiny_cfg.sde.train_N, 6
    np.random.seed(11)
    idx = np.random.choice(np.arange(N), B, replace=True)
    after = np.random.get_state()
    np.random.seed(11)
    torch_state = torch.get_rng_state()
    t, e2int_f, var, weight = tr._draw_times(B, True, "val_loss")
    want_t = torch.linspace(1.0, tiny_cfg.sde.sample_time_eps, N).index_select(0, torch.as_tensor(idx).long())
    assert t.dtype == torch.float32 and t.device.type == "cpu" and torch.equal(t, want_t)
    assert torch.equal(e2int_f, tr.SDE.e2int_f(want_t)) and torch.equal(var, tr.SDE.var(want_t)) and weight is None
    now = np.random.get_state()
    assert now[0] == after[0] and np.array_equal(now[1], after[1]) and now[2:] == after[2:]      # exactly one choice(arange(N), B)
    assert torch.equal(torch.get_rng_state(), torch_state)                                      # and nothing from torch's generator
    # t_index given: numpy's generator is not touched
    before = np.random.get_state()
    t2, e2, v2, _ = tr._draw_times(B, True, "val_loss", t_index=idx)
    now = np.random.get_state()
    assert np.array_equal(now[1], before[1]) and now[2:] == before[2:]
    assert torch.equal(t2, want_t) and torch.equal(e2, e2int_f) and torch.equal(v2, var)
    assert torch.equal(tr.timesteps, torch.linspace(1.0, tiny_cfg.sde.sample_time_eps, N))
    with pytest.raises(ValueError, match=r"update_score: t_index holds 5 entries for a batch of 6"):
        tr._draw_times(B, True, "update_score", t_index=idx[:5])


@pytest.mark.parametrize("mode", ["drop_all_iw", "ll_uniform", "drop_all_uniform"])
def test_draw_times_importance_weighted_branch(tiny_cfg, tmp_path, mode):
    tr = _trainer(_cfg(tiny_cfg, tmp_path))
    B = 6
    rho = torch.linspace(0.05, 0.95, B)
    np_state = np.random.get_state()
    t, e2int_f, var, weight = tr._draw_times(B, False, "val_nelbo", iw_mode=mode, rho=rho)
    want_t, want_var, want_m, want_w, _, _ = tr.SDE.iw_quantities(B, tiny_cfg.sde.time_eps, mode, False, rho=rho)
    assert torch.equal(t, want_t) and torch.equal(weight, want_w) and weight.shape == want_w.shape
    assert torch.equal(e2int_f, want_m.reshape(-1).float()) and torch.equal(var, want_var.reshape(-1).float())
    assert all(x.dtype == torch.float32 and x.device.type == "cpu" for x in (t, e2int_f, var, weight))
    # without rho: ONE torch.rand(B) on the CPU generator, nothing from numpy's
    torch.manual_seed(5)
    drawn = torch.rand(B)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    t2 = tr._draw_times(B, False, "update_score", iw_mode=mode)[0]
    assert torch.equal(torch.get_rng_state(), after)
    assert torch.equal(t2, tr.SDE.iw_quantities(B, tiny_cfg.sde.time_eps, mode, False, rho=drawn)[0])
    now = np.random.get_state()
    assert np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]


def test_ema_scope_swaps_in_and_out_also_when_the_body_raises(tiny_cfg, tmp_path):
    tr = _trainer(_cfg(tiny_cfg, tmp_path))
    params = [p for p in tr.model.parameters() if p.requires_grad]
    raw = [p.data.clone() for p in params]
    g = torch.Generator().manual_seed(2)
    ema = [torch.randn(p.shape, generator=g) for p in params]
    for p, e in zip(params, ema):
        tr.optimizer.state[p] = {"ema": e.clone()}

    def is_back():
        return (all(torch.equal(p.data, r) for p, r in zip(params, raw))
                and all(torch.equal(tr.optimizer.state[p]["ema"], e) for p, e in zip(params, ema)))

    with tr._ema_weights():
        assert all(torch.equal(p.data, e) for p, e in zip(params, ema))               # the body sees the EMA tensors
        assert all(torch.equal(tr.optimizer.state[p]["ema"], r) for p, r in zip(params, raw))
    assert is_back()
    with pytest.raises(KeyError):
        with tr._ema_weights(True):
            assert all(torch.equal(p.data, e) for p, e in zip(params, ema))
            raise KeyError("the body failed")
    assert is_back()
    swaps = []
    real = tr.optimizer.swap_parameters_with_ema
    tr.optimizer.swap_parameters_with_ema = lambda **kw: swaps.append(kw) or real(**kw)
    with tr._ema_weights(active=False):
        assert is_back()
    assert swaps == [] and is_back()
