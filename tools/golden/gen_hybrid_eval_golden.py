"""TEST INFRASTRUCTURE ONLY — writes tests/golden/iw_quantities.npz, hybrid_nelbo_tiny.npz and jsd.npz: what the reference computes on
the hybrid trainer's evaluation path.

Runs only where the upstream reference can be imported (through oracle/ref_import.py, on CPU); the fixtures are data, the reference does
not travel.

  * iw_quantities.npz — `DiffusionBase.iw_quantities` (diffusion/diffusion_continuous.py:340-592) of the four SDE families (the constants
    of sde_types.npz) for every mode that family defines, on a stored `rho` of 64 draws with the end points 0 and 1 - 2^-24 (upstream's
    `torch.rand` is patched to return it): the six outputs in fp32, and `<key>_f64`, the same reference code run in float64 (default dtype
    float64 while the SDE object builds its constants, a float64 `rho`) — the yardstick for how well conditioned each output is.
  * hybrid_nelbo_tiny.npz — the KL term of `Trainer.clc_compressor` (trainer/Hybrid_Trainer.py:117-143) on the tiny config with the
    weights and inputs of eval_tiny.npz, composed from the reference `Compressor`, `Score` and SDE objects in the method's order, both
    models in eval mode (the method itself goes on to EMD_loss, backward and two optimizer steps).  The draws are injected by patching
    `torch.rand` / `torch.randn_like` / `np.random.choice`, and stored.
  * jsd.npz — two seeded sets of clouds (2048 points; one inside radius 0.45, one reaching radius 1), the reference's
    `entropy_of_occupancy_grid` / `jsd_between_point_cloud_sets` on them, and the per-cell Bernoulli counts recomputed with the
    reference's own NearestNeighbors call.  Precondition (asserted): for every point the float64 squared distances to the nearest
    and the second-nearest cell differ by more than 1e-12, so no stored count hangs on a tie; a float64 brute force over all cells
    reproduces the reference's counters.

    python tools/golden/gen_hybrid_eval_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FAMILIES = {                                     # the constants of tests/golden/sde_types.npz
    "vpsde": dict(),
    "sub_vpsde": dict(),
    "vesde": dict(sigma2_min=0.01, sigma2_max=4.0, sigma2_0=0.01),
    "geometric_sde": dict(sigma2_min=3e-5, sigma2_max=0.999, sigma2_0=0.0),
}
MODES = ("ll_uniform", "ll_iw", "drop_all_uniform", "drop_all_iw", "drop_sigma2t_iw", "drop_sigma2t_uniform", "rescale_iw")
OUTPUTS = ("t", "var_t", "m_t", "obj_weight_t", "obj_weight_t_ll", "g2_t")
NELBO_CASES = (("vpsde", "discrete"), ("vpsde", "ll_uniform"), ("vpsde", "ll_iw"), ("sub_vpsde", "ll_iw"), ("vesde", "ll_iw"))
RHO_SEED, ETA_SEED, IDX_SEED, JSD_SEED = 41, 99, 2024, 7
JSD_CLOUDS, JSD_POINTS, JSD_RES = 16, 2048, 28


def tiny_cfg():
    with open(os.path.join(GOLDEN, "tiny_cfg.json")) as f:
        return R.dict2ns(json.load(f))


def family_cfg(name):
    c = tiny_cfg()
    c.sde.sde_type = name
    for k, v in FAMILIES[name].items():
        setattr(c.sde, k, v)
    return c


def weights(npz, prefix):
    return {k[len(prefix):]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(prefix)}


class patched:
    """Replace attributes for the length of a `with` block (the reference draws through torch.rand / torch.randn_like / np.random.choice)."""

    def __init__(self, *triples):
        self.triples = triples

    def __enter__(self):
        self.saved = [(o, n, getattr(o, n)) for o, n, _ in self.triples]
        for o, n, v in self.triples:
            setattr(o, n, v)

    def __exit__(self, *exc):
        for o, n, v in self.saved:
            setattr(o, n, v)


def save(name, out):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------------------ iw_quantities
def gen_iw():
    from diffusion.diffusion_continuous import make_diffusion
    g = torch.Generator().manual_seed(RHO_SEED)
    rho = torch.rand(64, generator=g)
    rho[0], rho[1] = 0.0, 1.0 - 2.0 ** -24
    out = {"rho": rho}
    for name in FAMILIES:
        c = family_cfg(name)
        out["%s/time_eps" % name] = c.sde.time_eps
        for k, v in FAMILIES[name].items():
            out["%s/%s" % (name, k)] = v
        with R.quiet():
            fam32 = make_diffusion(c.sde)
            torch.set_default_dtype(torch.float64)
            try:
                fam64 = make_diffusion(c.sde)                   # its auxiliary constants in float64
            finally:
                torch.set_default_dtype(torch.float32)
        for mode in MODES:
            res = {}
            for tag, fam, r in (("", fam32, rho), ("_f64", fam64, rho.double())):
                with patched((torch, "rand", lambda *a, r=r, **k: r.clone())):
                    try:
                        res[tag] = fam.iw_quantities(rho.numel(), c.sde.time_eps, mode, name == "sub_vpsde")
                    except AssertionError:
                        res[tag] = None                         # drop_all_iw is defined for the (sub-)VP SDE and the VE SDE only
            if res[""] is None:
                assert res["_f64"] is None
                out["%s/%s/raises" % (name, mode)] = "AssertionError"
                continue
            for tag, six in res.items():
                for key, v in zip(OUTPUTS, six):
                    if tag:
                        v = v.double()                          # (upstream's `torch.ones(1)` of drop_all_uniform stays fp32)
                    assert v.dtype == (torch.float64 if tag else torch.float32), (name, mode, key, v.dtype)
                    assert bool(torch.isfinite(v).all()), (name, mode, key)
                    out["%s/%s/%s%s" % (name, mode, key, tag)] = v
    save("iw_quantities.npz", out)


# ------------------------------------------------------------------------------------------------ the KL term of clc_compressor
def gen_nelbo():
    from model.scorenet.score import Score
    from model.Compressor.Network import Compressor
    from diffusion.diffusion_continuous import DiffusionSubVPSDE, DiffusionVESDE, DiffusionVPSDE
    cfg = tiny_cfg()
    comp = Compressor(cfg.compressor).eval()
    comp.load_state_dict(weights(np.load(os.path.join(GOLDEN, "trainer_sample_tiny.npz")), "c::"), strict=True)
    comp.init()
    score = Score(cfg.score).eval()
    score.load_state_dict(weights(np.load(os.path.join(GOLDEN, "score_tiny.npz")), "w::"), strict=True)
    fwd = np.load(os.path.join(GOLDEN, "compressor_fwd_tiny.npz"))
    point = torch.from_numpy(fwd["pts"])
    size = point.shape[0]
    torch.manual_seed(ETA_SEED)
    eta_draw = torch.randn(torch.from_numpy(fwd["all_eps"]).shape)
    np.random.seed(IDX_SEED)
    idx_draw = np.random.choice(np.arange(cfg.sde.train_N), size, replace=True)
    g = torch.Generator().manual_seed(RHO_SEED + 1)
    out = {"eta": eta_draw, "idx": idx_draw, "post_noise": fwd["post_noise"], "pts": point}
    for sde_type, mode in NELBO_CASES:
        c = family_cfg(sde_type)
        c.sde.iw_sample_q_mode = mode
        with R.quiet():
            SDE = {"vpsde": DiffusionVPSDE, "sub_vpsde": DiffusionSubVPSDE, "vesde": DiffusionVESDE}[sde_type](c.sde)
        N, time_eps = c.sde.train_N, c.sde.time_eps
        timesteps = torch.linspace(1.0, c.sde.sample_time_eps, N)
        discrete = mode == "discrete"
        rho = torch.rand(size, generator=g)
        noise = iter([torch.from_numpy(n).transpose(1, 2).contiguous() for n in fwd["post_noise"]])   # drawn as (B, z, tokens)
        with patched((torch, "randn", lambda *a, **k: next(noise))):
            output = comp(point)                                                     # Hybrid_Trainer.py:117
        assert torch.equal(output["all_eps"], torch.from_numpy(fwd["all_eps"])), "not the forward compressor_fwd_tiny.npz recorded"
        with patched((torch, "rand", lambda *a, **k: rho.clone()), (torch, "randn_like", lambda x, **k: eta_draw.clone()),
                     (np.random, "choice", lambda *a, **k: idx_draw.copy())):
            recon, logqz = output['set'], output['all_logqz']                        # :118-143, the method's lines
            logqz = torch.cat(logqz, dim=1).transpose(1, 2)
            eps = output["all_eps"]
            if discrete:
                idx = torch.from_numpy(np.random.choice(np.arange(N), size, replace=True))
                t = timesteps.index_select(0, idx)
                e2int_f = SDE.e2int_f(t)[:, None, None]
                var = SDE.var(t)[:, None, None]
                weight_q = SDE.g2(t)[:, None, None] / (2 * var)
            else:
                t, var, e2int_f, weight_q, _, g2 = SDE.iw_quantities(size, time_eps=time_eps, iw_sample_mode=c.sde.iw_sample_q_mode,
                                                                     iw_subvp_like_vp_sde=True if sde_type == 'sub_vpsde' else False)
                e2int_f = e2int_f[:, :, None]
                var = var[:, :, None]
                weight_q = weight_q[:, :, None]
            eta = torch.randn_like(eps)
            std = torch.sqrt(var)
            xt = eps * e2int_f + std * eta
            params = score(xt, t, condition=None, label=None)
            distance = torch.square(eta - params)
            cross_entropy_const = 0.5 * (1.0 + torch.log(2.0 * np.pi * SDE.var(t=torch.tensor(time_eps))))
            logpz = -(distance * weight_q + cross_entropy_const)
            kl_loss = (logqz - logpz).mean()
        tag = "%s/%s" % (sde_type, mode)
        for k, v in FAMILIES[sde_type].items():
            out["%s/%s" % (sde_type, k)] = v
        out.update({tag + "/rho": rho, tag + "/t": t, tag + "/var": var.reshape(-1), tag + "/e2int_f": e2int_f.reshape(-1),
                    tag + "/weight_q": weight_q.reshape(-1), tag + "/xt": xt, tag + "/params": params,
                    tag + "/cross_entropy_const": cross_entropy_const, tag + "/kl_loss": kl_loss,
                    tag + "/terms_rms": (logqz - logpz).double().pow(2).mean().sqrt()})
        out["logqz"], out["all_eps"], out["set"] = logqz.contiguous(), eps, recon
        print(tag, "t", t.tolist(), "kl", float(kl_loss), "rms of the terms", float(out[tag + "/terms_rms"]))
    save("hybrid_nelbo_tiny.npz", out)


# ------------------------------------------------------------------------------------------------ JSD
def cloud_sets():
    """Two sets of anisotropic Gaussian blobs with a few dense arms each: set 'in' scaled so that every cloud's farthest point lies at
    0.30..0.45 from the origin, set 'out' at 0.9..1.0 (the reference's ShapeNet normalisation reaches radius 1: the cells on the
    boundary of the grid collect everything outside it)."""
    g = np.random.RandomState(JSD_SEED)
    sets = {}
    for name, (lo, hi) in (("in", (0.30, 0.45)), ("out", (0.90, 1.00))):
        clouds = []
        for _ in range(JSD_CLOUDS):
            axes = g.uniform(0.15, 1.0, size=3)
            p = g.randn(JSD_POINTS, 3) * axes
            arm = g.randint(0, JSD_POINTS, size=JSD_POINTS // 4)
            p[arm] = p[arm] * np.array([2.5, 0.08, 0.08])[g.permutation(3)]
            p = p + g.randn(3) * 0.1
            p = p / np.sqrt((p ** 2).sum(1)).max() * g.uniform(lo, hi)
            clouds.append(p.astype(np.float32))
        sets[name] = np.stack(clouds)
    return sets


def gen_jsd():
    from sklearn.neighbors import NearestNeighbors
    from evaluation import evaluation_metrics as E
    sets = cloud_sets()
    out = {"resolution": JSD_RES}
    min_gap = np.inf
    for in_sphere in (True, False):
        grid, _ = E.unit_cube_grid_point_cloud(JSD_RES, in_sphere)
        cells = grid.reshape(-1, 3)
        tag = "sphere" if in_sphere else "cube"
        out["grid_" + tag] = cells
        nn = NearestNeighbors(n_neighbors=1).fit(cells)                  # the reference's own call (:380)
        c64 = torch.from_numpy(cells).double()
        for name, pcs in sets.items():
            acc_entropy, grid_counters = E.entropy_of_occupancy_grid(pcs, JSD_RES, in_sphere)
            bern = np.zeros(len(cells), dtype=np.int64)
            brute = np.zeros(len(cells), dtype=np.int64)
            for pc in pcs:
                _, indices = nn.kneighbors(pc)
                bern[np.unique(np.squeeze(indices))] += 1
                for lo in range(0, len(pc), 256):                                  # float64 brute force, (dx^2 + dy^2) + dz^2
                    d = torch.from_numpy(pc[lo:lo + 256]).double()[:, None, :] - c64[None, :, :]
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    two, arg = torch.topk(d2, 2, dim=1, largest=False)
                    min_gap = min(min_gap, float((two[:, 1] - two[:, 0]).min()))
                    assert np.array_equal(arg[:, 0].numpy(), np.squeeze(indices)[lo:lo + 256]), "the float64 brute force and the tree disagree"
                    np.add.at(brute, arg[:, 0].numpy(), 1)
            assert np.array_equal(brute, grid_counters.astype(np.int64))
            assert grid_counters.sum() == pcs.shape[0] * pcs.shape[1] and bern.max() <= pcs.shape[0]
            out["%s/%s/grid_counters" % (name, tag)] = grid_counters
            out["%s/%s/bernoulli" % (name, tag)] = bern
            out["%s/%s/acc_entropy" % (name, tag)] = acc_entropy
            print(name, tag, "cells", len(cells), "occupied", int((grid_counters > 0).sum()), "acc_entropy", acc_entropy)
    assert min_gap > 1e-12, min_gap
    print("smallest float64 gap between the nearest and the second-nearest cell: %.3e" % min_gap)
    for name, pcs in sets.items():
        out["pcs_" + name] = pcs
    out["jsd"] = E.jsd_between_point_cloud_sets(sets["in"], sets["out"], JSD_RES)
    out["jsd_self"] = E.jsd_between_point_cloud_sets(sets["out"], sets["out"], JSD_RES)
    print("jsd", out["jsd"], "of a set with itself", out["jsd_self"])
    save("jsd.npz", out)


def main():
    R.setup()
    torch.set_grad_enabled(False)
    gen_iw()
    gen_nelbo()
    gen_jsd()


if __name__ == "__main__":
    main()
