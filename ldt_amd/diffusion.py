"""The SDE families and the discrete reverse-SDE sampler (reference: diffusion/diffusion_continuous.py).

`DiffusionBase` holds the samplers, written against the schedule (`f, g2, var, e2int_f`) a family supplies: `DiffusionVPSDE` (:626-678;
also `betas, alpha, alphas_cump, N` for the ancestral / ddim / PNDM predictors), `DiffusionSubVPSDE` (:681-729), `DiffusionVESDE`
(:732-766), `DiffusionGeometric` (:595-623); `make_diffusion` is upstream's factory (:18-29).  Every class keeps the reference
constructor (`args` = cfg.sde Namespace) and `sample_discrete(...)` (:133-338).
Schedule scalars are host-side fp32 tables computed with the reference's own op order (SURVEY hard
part 4: var(1e-6) is exactly one ulp in fp32 and must not be recomputed with a different expf) and uploaded.

`sample_discrete` has the reference signature and is a dispatcher: argument rules, `step_table`, the initial latents (`torch.randn` on the
CPU generator, then — unless `noise` is injected — `torch.randint` for the Philox key), placement, then one of two loops on HIP kernels:
  * `_sample_fused` — `score_fn` is the bound `Trainer.score_fn` of an `ldt_amd.Score`, no corrector / record / print_steps: `partition`
    cuts the batch into sub-batches, a builder (`_SharedModulation`: one AdaLN table for all N steps, LN fold, probe, monitor;
    `_PerSampleModulation`: label / condition rows via `Score.cond_args`) plans each, and `_run_jobs` issues one `ldt_sample_loop` per
    `_Job` = N x (Score forward -> predictor update with in-kernel Philox noise -> ++step), optionally replayed from a captured hipGraph;
  * `_sample_generic` — any other `score_fn(t, x, label=, condition=) -> (score, params)`, driven step by step from Python on the device
    its tensors live on; updates by `ldt_sampler_step` (params, not score, feed it), the corrector chosen once (`_corrector`).
The partition rule and the draw schedule are held by tests/test_sampler_schedule_host.py.  Extra keyword-only arguments (not in the
reference): `x0`, `noise` (inject the CPU draws for parity), `sample_offset` (global index of this rank's first sample, keeps Philox
streams shard-invariant), `streams` (sub-batches sampled concurrently on their own HIP streams; default `LDT_STREAMS` or 1).
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib

PREDICTORS = ("reversediffusion", "ancestral", "eulermaruyama", "ddim")
# iw_sample_mode names of DiffusionBase.iw_quantities (diffusion_continuous.py:362-417); the second tuple draws t uniformly
IW_MODES = ("ll_uniform", "ll_iw", "drop_all_uniform", "drop_all_iw", "drop_sigma2t_iw", "drop_sigma2t_uniform", "rescale_iw")
_IW_UNIFORM_T = ("ll_uniform", "drop_all_uniform", "drop_sigma2t_uniform", "rescale_iw")


# ---- environment switches of the fused loop, each read once per call, where no keyword decides
def _env_streams():                     # sub-batches on concurrent streams; opt-in, so that per-kernel accounting (bench roofline, rocprof)
    return int(os.environ.get("LDT_STREAMS", "1"))                                    # stays one launch = the whole batch


def _env_adaln_bf16():                  # per-sample AdaLN rows from the bf16 weight panel; 0 keeps the fp32 SGEMM (Score.stacked_adaln_bf16)
    return bool(int(os.environ.get("LDT_ADALN_BF16", "1")))


def _env_fold_monitor_every():          # the in-loop LN-fold monitor runs every so many steps and on the last one (default 50: 47 launches
    return int(os.environ.get("LDT_FOLD_MONITOR_EVERY", "50"))                        # of ~5 us per monitored step = 0.05 % of a call)


# ---- set-up every sampler shares
def _cuda_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("%s: device %s — the HIP path has no CPU fallback" % (who, device))
    return dev


def _initial_latents(num_samples, shape, given, dev=None):
    """The initial sample: a CPU-generator draw like the reference (:237) unless `given`; with `dev`, a private fp32 copy placed there."""
    x = torch.randn((num_samples,) + tuple(shape)) if given is None else given
    return x if dev is None else x.to(dev, torch.float32).contiguous().clone()


# ---- sub-batches of the fused loop
SubBatch = namedtuple("SubBatch", "lo hi slot gemm_wgs elem_offset")
_Job = namedtuple("_Job", "plan cond x x_mean eps_tmp counter noise elem_offset traj")       # one ldt_sample_loop call


def partition(B, streams, per_sample, elem_offset):
    """`streams` (clamped to [1, B]) row ranges [lo, hi) = [B i // streams, B (i + 1) // streams) of a batch of B, each with its workspace
    slot i, the persistent-grid cap of its GEMMs (0 = the whole chip for one stream, else its share of the 256 CUs) and the Philox
    element offset of its first row, so that the draws do not depend on the split (tests/test_sampler_schedule_host.py)."""
    streams = max(1, min(int(streams), B))
    bounds = [B * i // streams for i in range(streams + 1)]
    return [SubBatch(lo, hi, i, 0 if streams == 1 else max(256 // streams, 1), elem_offset + lo * per_sample)
            for i, (lo, hi) in enumerate(zip(bounds, bounds[1:]))]


class _SharedModulation:
    """Plans of an unconditional batch: AdaLN rows for every step, shared by the batch, and — where a route exists — the LN-fold table,
    guarded by a probe before the loop and a monitor inside it.  `monitor`: the running max of mean^2 / variance over the monitored
    steps (a device scalar), or None when nothing folds."""
    def __init__(self, model, ts_d, T):
        self.model, self.T, self.fold, self.monitor, self.every = model, T, None, None, _env_fold_monitor_every()
        self.mod = model.time_table(ts_d)[1]

    def build(self, sb, xs):
        model, Bs = self.model, sb.hi - sb.lo
        if self.fold is None and model.can_fold(Bs, self.T, sb.gemm_wgs):
            self.fold = model.fold_table(self.mod)                                    # (+ the LN-folding S / C rows)
            # guard: a monitored forward on the first sub-batch at step 0 (0.1 % of a 1000-step call); rows whose
            # mean dwarfs their spread switch this model to the LayerNorm kernels (Score.fold_probe)
            model.fold_probe(xs, 0, self.mod, self.fold)
        folding = model.can_fold(Bs, self.T, sb.gemm_wgs)                             # (the probe may just have switched it off)
        if folding and self.monitor is None:
            self.monitor = torch.zeros(1, dtype=torch.float32, device=xs.device)
        # inside the loop the same monitor runs every LDT_FOLD_MONITOR_EVERY steps and on the last step; the running maximum is read at the
        # NEXT call's first can_fold() (a trajectory that passes the bound mid-way is seen, not just its two ends)
        return model.plan(Bs, self.T, self.mod, model.n_mod, 0, fold=self.fold if folding else None, slot=sb.slot, gemm_wgs=sb.gemm_wgs,
                          monitor=self.monitor if folding else None, monitor_every=self.every), None


class _PerSampleModulation:
    """Plans of a labelled / conditioned batch: per-sample AdaLN rows, rebuilt every step inside the loop from the time embedding of all
    steps plus each sample's label / image embedding (`Score.cond_args`); a point condition adds the cross-attention K|V rows."""
    def __init__(self, model, ts_d, T, label, condition):
        self.model, self.T, self.monitor = model, T, None                             # (no LN fold with per-sample rows: nothing to monitor)
        self.extra, self.kv, self.S = model.condition_embedding(label, condition)
        self.temb, self.weights = model.time_embedding(ts_d), model.adaln_stack(_env_adaln_bf16())

    def build(self, sb, xs):
        model, (lo, hi), Bs, S = self.model, sb[:2], sb.hi - sb.lo, self.S
        modb = torch.empty((Bs, model.n_mod), dtype=torch.float32, device=xs.device)
        ex = None if self.extra is None else self.extra[lo:hi].contiguous()
        kvs = None if self.kv is None else {l: t.view(-1, S, t.shape[-1])[lo:hi].reshape(Bs * S, -1) for l, t in self.kv.items()}
        plan = model.plan(Bs, self.T, modb, 0, model.n_mod, kv_cond=kvs, cond_tokens=S, slot=sb.slot, gemm_wgs=sb.gemm_wgs)
        return plan, model.cond_args(self.weights, self.temb, ex, modb)


def _run_jobs(jobs, launch, dev, sync):
    """`launch(job)` for every sub-batch: one inline on the caller's stream; several each on a stream and a thread of its own, fenced
    against the caller's stream on both sides, the first error handed back.  `sync`: the caller's scratch must outlive the loop.
    Why concurrent streams (trajectories are independent): with the persistent GEMM grids capped at half the chip each, one stream's
    HBM-bound phases (epilogues, attention) run beside the other's MFMA-bound main loops instead of all 256 CUs alternating between the
    two (measured -2.6 % per SDE step at B=64, T=256; a deliberate phase skew between the streams gained nothing, four quarter batches
    lose: too few tiles).  Only where a half batch still fills its half of the chip with whole 256x256 tiles."""
    main = torch.cuda.current_stream()
    if len(jobs) == 1:
        launch(jobs[0])
    else:
        import threading
        subs, errs = [torch.cuda.Stream(device=dev) for _ in jobs], []

        def worker(job, st):
            try:
                torch.cuda.set_device(dev)
                st.wait_stream(main)                                                  # tables / x0 were produced on the caller's stream
                with torch.cuda.stream(st):
                    launch(job)
            except BaseException as e:                                                # noqa: BLE001 - re-raised on the caller's thread
                errs.append(e)

        th = [threading.Thread(target=worker, args=(j, st)) for j, st in zip(jobs, subs)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()                                                                 # (ctypes releases the GIL inside the C call)
        if errs:
            raise errs[0]
        for st in subs:
            main.wait_stream(st)
    if sync or len(jobs) > 1:
        main.synchronize()                                                            # scratch / sub-streams must outlive the loop


def make_diffusion(args):
    """diffusion_continuous.py:18-29."""
    if args.sde_type == "geometric_sde":
        return DiffusionGeometric(args)
    if args.sde_type == "vpsde":
        return DiffusionVPSDE(args)
    if args.sde_type == "sub_vpsde":
        return DiffusionSubVPSDE(args)
    if args.sde_type == "vesde":
        return DiffusionVESDE(args)
    raise ValueError("Unrecognized sde type: {}".format(args.sde_type))


class DiffusionBase:
    """diffusion_continuous.py:32-624: the samplers, written against the schedule a subclass supplies (f, g2, var, e2int_f).
    `score_kind` / `score_consts()` name the subclass's var(t) for ldt_sde_score (Trainer.score_fn)."""
    score_kind = None

    def __init__(self, args):
        self.sigma2_0 = args.sigma2_0
        self.sde_type = args.sde_type
        self.time_eps = args.time_eps
        self.sample_time_eps = args.sample_time_eps

    def f(self, t):
        raise NotImplementedError

    def g2(self, t):
        raise NotImplementedError

    def var(self, t):
        raise NotImplementedError

    def e2int_f(self, t):
        raise NotImplementedError

    def std(self, t):
        return torch.sqrt(self.var(t))

    def inv_var(self, var):
        """diffusion_continuous.py:73-76: the time at which var(t) equals `var` (the sub-VP SDE has no closed form, as upstream)."""
        raise NotImplementedError

    def sample_q(self, x_init, noise, var_t, m_t):
        """diffusion_continuous.py:78-81: a draw of q(x_t | x_0) = N(m_t x_0, var_t) given the N(0,1) `noise`.  Device latents
        (B, ...) with one (m_t, var_t) per sample — (B,) or (B, 1, ..., 1), as the trainers pass them — go through
        ldt_diffuse_q; anything else (host tensors, a shared scalar, full-shape coefficients) is the host expression."""
        B = x_init.shape[0] if torch.is_tensor(x_init) and x_init.dim() > 0 else 0
        per_sample = all(torch.is_tensor(c) and c.is_cuda and c.numel() == B for c in (var_t, m_t))
        if per_sample and x_init.is_cuda and x_init.dtype == torch.float32 and (x_init.numel() // B) % 4 == 0:
            return ops.diffuse_q(x_init, m_t.float(), var_t.float(), noise.to(x_init))[0]
        return m_t * x_init + torch.sqrt(var_t) * noise

    def cross_entropy_const(self, ode_eps):
        """diffusion_continuous.py:83-86: the constant term of CE(q(z_0 | x) || p(z_0)), 1/2 (1 + log(2 pi var(ode_eps))), for the
        ODE integration cutoff `ode_eps` (a host scalar tensor; upstream builds it on the device)."""
        return 0.5 * (1.0 + torch.log(2.0 * np.pi * self.var(t=torch.tensor(ode_eps))))

    # ---- importance-weighted time sampling (:340-592) -----------------------------------------------
    def iw_quantities(self, size, time_eps, iw_sample_mode, iw_subvp_like_vp_sde, *, rho=None, device=None):
        """diffusion_continuous.py:340-592: `size` diffusion times drawn under the importance-sampling scheme `iw_sample_mode`, with the
        objective weights that go with each time.  Dispatch by `sde_type` as upstream (:340-348): 'vpsde' / 'geometric_sde' the VP-like
        form (:351-423), 'sub_vpsde' :425-512 (its IW modes are defined through the VP-SDE with the same beta(t) and need
        `iw_subvp_like_vp_sde`, else NotImplementedError), 'vesde' :514-592.  Modes: `IW_MODES`; anything else is upstream's ValueError.
        Returns upstream's six tensors (t (B,), var_t (B,1), m_t (B,1), obj_weight_t, obj_weight_t_ll, g2_t (B,1)); obj_weight_t is (1,1)
        for 'drop_all_uniform', (B,1) otherwise.  obj_weight_t is the factor in front of the l2 distance under the mode, obj_weight_t_ll
        the one that turns the mode's sampling into likelihood weighting.

        Host fp32, operation for operation in upstream's order (the arrays are (B,): a kernel would add rounding differences and no
        speed), then moved to `device` (None: they stay on the host).  Keyword extension: `rho` (B,) replaces upstream's
        `torch.rand(size, device='cuda')`, which no other device reproduces; by default it is ONE `torch.rand(size)` on the CPU generator."""
        if self.sde_type in ("geometric_sde", "vpsde"):
            family = self._iw_vpsdelike
        elif self.sde_type == "sub_vpsde":
            family = self._iw_subvpsdelike
        elif self.sde_type == "vesde":
            family = self._iw_vesde
        else:
            raise NotImplementedError
        if rho is None:
            rho = torch.rand(size)
        rho = torch.as_tensor(rho).detach().to("cpu", torch.float32).reshape(-1)
        if rho.numel() != size:
            raise ValueError("iw_quantities: rho holds %d draws for size %d" % (rho.numel(), size))
        if iw_sample_mode not in IW_MODES:
            raise ValueError("Unrecognized importance sampling type: {}".format(iw_sample_mode))
        if iw_sample_mode in _IW_UNIFORM_T:                       # uniform t: the same lines in all three upstream functions
            t = rho * (1. - time_eps) + time_eps
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t_ll = g2_t / (2.0 * var_t)
            if iw_sample_mode == "ll_uniform":
                obj_weight_t = obj_weight_t_ll
            elif iw_sample_mode == "drop_all_uniform":
                obj_weight_t = torch.ones(1)
            elif iw_sample_mode == "drop_sigma2t_uniform":
                obj_weight_t = g2_t / 2.0
            else:                                                 # rescale_iw (uniform t upstream too, despite the name)
                obj_weight_t = 0.5 / (1.0 - var_t)
        else:
            t, var_t, m_t, obj_weight_t, obj_weight_t_ll, g2_t = family(rho, time_eps, iw_sample_mode, iw_subvp_like_vp_sde)
        out = (t, var_t.view(-1, 1), m_t.view(-1, 1), obj_weight_t.view(-1, 1), obj_weight_t_ll.view(-1, 1), g2_t.view(-1, 1))
        return out if device is None else tuple(o.to(device) for o in out)

    def _iw_erfinv_t(self, rho):
        """t for the 'drop_all_iw' mode of the (sub-)VP SDE: the inverse CDF of a density ~ 1 / (1 - var_vpsde(t)) (:389-390, :472-473)."""
        return torch.sqrt(1.0 / self.delta_beta_half) * torch.erfinv(rho * self.const_norm_2 + self.const_erf) - self.beta_frac

    def _iw_vpsdelike(self, rho, time_eps, mode, _unused):
        ones = torch.ones_like(rho)
        if mode == "ll_iw":                                       # :368-376
            sigma2_1, sigma2_eps = self.var(ones), self.var(time_eps * ones)
            log_sigma2_1, log_sigma2_eps = torch.log(sigma2_1), torch.log(sigma2_eps)
            var_t = torch.exp(rho * log_sigma2_1 + (1 - rho) * log_sigma2_eps)
            t = self.inv_var(var_t)
            m_t, g2_t = self.e2int_f(t), self.g2(t)
            obj_weight_t = obj_weight_t_ll = 0.5 * (log_sigma2_1 - log_sigma2_eps) / (1.0 - var_t)
        elif mode == "drop_all_iw":                               # :385-393
            assert self.sde_type == "vpsde", "Importance sampling for fully unweighted objective is currently only " \
                                             "implemented for the regular VPSDE."
            t = self._iw_erfinv_t(rho)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t = self.const_norm / (1.0 - var_t)
            obj_weight_t_ll = obj_weight_t * g2_t / (2.0 * var_t)
        else:                                                     # drop_sigma2t_iw :395-403
            sigma2_1, sigma2_eps = self.var(ones), self.var(time_eps * ones)
            var_t = rho * sigma2_1 + (1 - rho) * sigma2_eps
            t = self.inv_var(var_t)
            m_t, g2_t = self.e2int_f(t), self.g2(t)
            obj_weight_t = 0.5 * (sigma2_1 - sigma2_eps) / (1.0 - var_t)
            obj_weight_t_ll = obj_weight_t / var_t
        return t, var_t, m_t, obj_weight_t, obj_weight_t_ll, g2_t

    def _iw_subvpsdelike(self, rho, time_eps, mode, like_vp_sde):
        if not like_vp_sde:                                       # :457-458, :477-478, :490-491
            raise NotImplementedError("iw_sample_mode %r of the sub-VP SDE is only defined through the analogous VP-SDE "
                                      "(iw_subvp_like_vp_sde=True)" % (mode,))
        ones = torch.ones_like(rho)
        if mode == "ll_iw":                                       # :445-456
            sigma2_1, sigma2_eps = self.var_vpsde(ones), self.var_vpsde(time_eps * ones)
            log_sigma2_1, log_sigma2_eps = torch.log(sigma2_1), torch.log(sigma2_eps)
            var_t_vpsde = torch.exp(rho * log_sigma2_1 + (1 - rho) * log_sigma2_eps)
            t = self.inv_var_vpsde(var_t_vpsde)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t = obj_weight_t_ll = g2_t / (2.0 * var_t) * (log_sigma2_1 - log_sigma2_eps) * var_t_vpsde / (1 - var_t_vpsde) / self.beta(t)
        elif mode == "drop_all_iw":                               # :467-476
            assert self.sde_type == "sub_vpsde", "Importance sampling for fully unweighted objective is " \
                                                 "currently only implemented for the Sub-VPSDE."
            t = self._iw_erfinv_t(rho)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t = self.const_norm / (1.0 - self.var_vpsde(t))
            obj_weight_t_ll = obj_weight_t * g2_t / (2.0 * var_t)
        else:                                                     # drop_sigma2t_iw :480-489
            sigma2_1, sigma2_eps = self.var_vpsde(ones), self.var_vpsde(time_eps * ones)
            var_t_vpsde = rho * sigma2_1 + (1 - rho) * sigma2_eps
            t = self.inv_var_vpsde(var_t_vpsde)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t = 0.5 * g2_t / self.beta(t) * (sigma2_1 - sigma2_eps) / (1.0 - var_t_vpsde)
            obj_weight_t_ll = obj_weight_t / var_t
        return t, var_t, m_t, obj_weight_t, obj_weight_t_ll, g2_t

    def _iw_vesde(self, rho, time_eps, mode, _unused):
        ones = torch.ones_like(rho)
        if mode in ("ll_iw", "drop_all_iw"):                      # :529-541, :550-562: one sampling law, two weightings
            nsigma2_1, nsigma2_eps, sigma2_eps = self.var_N(ones), self.var_N(time_eps * ones), self.var(time_eps * ones)
            log_frac_sigma2_1, log_frac_sigma2_eps = torch.log(self.sigma2_max / nsigma2_1), torch.log(nsigma2_eps / sigma2_eps)
            var_N_t = (1.0 - self.sigma2_min) / (1.0 - torch.exp(rho * (log_frac_sigma2_1 + log_frac_sigma2_eps) - log_frac_sigma2_eps))
            t = self.inv_var_N(var_N_t)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t_ll = 0.5 * (log_frac_sigma2_1 + log_frac_sigma2_eps) * self.var_N(t) / (1.0 - self.sigma2_min)
            if mode == "ll_iw":
                obj_weight_t = obj_weight_t_ll
            else:
                obj_weight_t = 2.0 * obj_weight_t_ll / np.log(self.sigma2_max / self.sigma2_min)
        else:                                                     # drop_sigma2t_iw :564-572
            nsigma2_1, nsigma2_eps = self.var_N(ones), self.var_N(time_eps * ones)
            var_N_t = torch.exp(rho * torch.log(nsigma2_1) + (1 - rho) * torch.log(nsigma2_eps))
            t = self.inv_var_N(var_N_t)
            var_t, m_t, g2_t = self.var(t), self.e2int_f(t), self.g2(t)
            obj_weight_t = 0.5 * torch.log(nsigma2_1 / nsigma2_eps) * self.var_N(t)
            obj_weight_t_ll = obj_weight_t / var_t
        return t, var_t, m_t, obj_weight_t, obj_weight_t_ll, g2_t

    def _init_iw_constants(self):
        """The auxiliary constants of the linear-beta families (:637-645, :691-699; host fp32 scalars where upstream builds CUDA ones):
        `delta_beta_half`, `beta_frac`, `const_aq`, `const_erf`, `const_norm`, `const_norm_2` — the erf normalisation of 'drop_all_iw'."""
        self.delta_beta_half = torch.tensor(0.5 * (self.beta_end - self.beta_start))
        self.beta_frac = torch.tensor(self.beta_start / (self.beta_end - self.beta_start))
        self.const_aq = (1.0 - self.sigma2_0) * torch.exp(0.5 * self.beta_frac) * torch.sqrt(0.25 * np.pi / self.delta_beta_half)
        self.const_erf = torch.erf(torch.sqrt(self.delta_beta_half) * (self.time_eps + self.beta_frac))
        self.const_norm = self.const_aq * (torch.erf(torch.sqrt(self.delta_beta_half) * (1.0 + self.beta_frac)) - self.const_erf)
        self.const_norm_2 = torch.erf(torch.sqrt(self.delta_beta_half) * (1.0 + self.beta_frac)) - self.const_erf

    # ---- per-step coefficient table for ldt_sampler_step ------------------------------------------
    def step_table(self, N, predictor, time_eps, probability_flow=False):
        """-> (timesteps [N] fp32 CPU, coef [N,4] fp32 CPU, mode).  All scalars are produced on the CPU with
        the reference's expressions (fp32 tensors), the folded forms in fp64 then rounded once."""
        if predictor not in PREDICTORS:
            raise NotImplementedError("preditor not Implemented")           # diffusion_continuous.py:328
        ts = torch.linspace(1.0, time_eps, N)                               # :238
        if predictor == "ancestral":                                        # :152-162 — exact op order on device
            idx = (ts * (N - 1) / 1.0).long()
            beta = self.betas[idx]
            coef = torch.stack([beta, self.std(ts), torch.sqrt(1. - beta), torch.sqrt(beta)], 1)
            return ts, coef.contiguous(), 0
        std = self.std(ts).double()
        if predictor in ("reversediffusion", "eulermaruyama"):              # :141-150 (dt = (1 - time_eps) / N), :182-191 (dt = -1 / N)
            h = ((1 - time_eps) if predictor == "reversediffusion" else 1.0) / N   # |dt|: negation is exact, so one form serves both signs
            g2 = self.g2(ts).double(); ff = self.f(ts).double()     # fp32 like upstream, then folded in fp64
            k = 0.5 if probability_flow else 1.0
            A = 1 - ff * h
            Bc = -g2 * k * h / std                 # x_mean = x - (f x - g2 k score) dt, score = -params/std
            Cc = torch.zeros_like(g2) if probability_flow else torch.sqrt(g2) * np.sqrt(h)
        else:                                                              # ddim :164-180 (sigma = 0)
            idx = (ts * (N - 1) / 1.0).long()
            at = self.alphas_cump[idx].double()
            at_next = torch.where(idx - 1 < 0, torch.ones_like(at), self.alphas_cump[(idx - 1).clamp_min(0)].double())
            A = at_next.sqrt() / at.sqrt()
            Bc = -at_next.sqrt() * (1 - at).sqrt() / at.sqrt() + (1 - at_next).sqrt()
            Cc = torch.zeros_like(at)
        coef = torch.stack([A, Bc, Cc, torch.zeros_like(A)], 1).float()
        return ts, coef.contiguous(), 1

    # ---- probability-flow ODE sampling (sample_mode: continuous) -----------------------------------------
    @torch.no_grad()
    def sample_model_ode(self, score_fn, num_samples, shape, ode_eps, ode_solver_tol, enable_autocast=False, noise=None,
                         condition=None, label=None, *, device="cuda", solver="scipy", shared_t=None):
        """diffusion_continuous.py:88-131: dx/dt = f(t) x - g2(t)/2 * score, from t = 1 to `ode_eps`, solved the way the
        reference's `torchdiffeq.odeint(method="scipy_solver", options={"solver": "RK45"})` does it: scipy's RK45 on the
        host over the flattened float64 state, time reversed to increasing s = -t, rtol = atol = `ode_solver_tol`; every
        function evaluation is one Score forward on the GPU (`score_fn(t, x)` with t a (B,) vector, as upstream).
        Returns (samples, nfe_count, seconds) like the reference.  `noise` defaults to a CPU-generator draw (the reference
        draws on the CUDA generator, :107 — not reproducible across devices either way).
        NB the bf16 Score limits the smoothness the step controller sees to ~1e-3 relative: tolerances much below that
        (the shipped `ode_tol: 1e-5`) are met only by many small steps.  torchdiffeq is not vendored upstream: its wrapper's
        behaviour is restated from its published semantics — parity unpinned.

        solver (keyword-only, not in the reference): "scipy" (default) is the host path above; "device" keeps the float64 state and
        the seven stage derivatives on the GPU and runs the same Dormand-Prince steps there (`_sample_model_ode_device`; ldt_amd/ode.py,
        csrc/ode_rk45.hip), reading one double back per step attempt.  `shared_t` applies to the device solver only."""
        import time
        if solver not in ("scipy", "device"):
            raise ValueError("sample_model_ode: solver=%r (\"scipy\" or \"device\")" % (solver,))
        dev = _cuda_device(device, "sample_model_ode")
        if solver == "device":
            return self._sample_model_ode_device(score_fn, num_samples, shape, ode_eps, ode_solver_tol, noise, condition, label, dev,
                                                 shared_t)
        from scipy.integrate import solve_ivp
        x0 = _initial_latents(num_samples, shape, noise)
        full = tuple(x0.shape)
        nfe = [0]

        def fun(s, y):
            t = torch.full((full[0],), -float(s), dtype=torch.float32, device=dev)
            x = torch.from_numpy(y).to(dev, torch.float32).reshape(full)
            score, _ = score_fn(t, x, label=label, condition=condition)
            dx = self.f(t)[:, None, None] * x - 0.5 * self.g2(t)[:, None, None] * score
            nfe[0] += 1
            return (-dx).reshape(-1).double().cpu().numpy()

        t0 = time.time()
        sol = solve_ivp(fun, t_span=[-1.0, -float(ode_eps)], y0=x0.reshape(-1).double().cpu().numpy(),
                        t_eval=[-1.0, -float(ode_eps)], method="RK45", rtol=ode_solver_tol, atol=ode_solver_tol)
        out = torch.from_numpy(sol.y[:, -1]).to(dev, torch.float32).reshape(full)
        return out, nfe[0], time.time() - t0

    def _sample_model_ode_device(self, score_fn, num_samples, shape, ode_eps, ode_solver_tol, noise, condition, label, dev, shared_t):
        """`sample_model_ode(solver="device")`: the same ODE, tolerances, reversed time and `noise` handling as the scipy path, with
        RK45's arithmetic on the device.  The host keeps the step controller (ldt_amd/ode.py: float64 Python scalars, scipy's rules);
        per evaluation it forms the batch-uniform fp32 scalars f(t), g2(t), sqrt(var(t)) with this SDE object's own methods — so every
        family works — and launches: ldt_ode_stage (stage state in float64 + its fp32 cast), one Score forward, ldt_ode_rhs (the
        stage derivative in the operation order of `Trainer.score_fn` + `fun()` above, widened to float64).  The error norm comes
        back as one double per step attempt (ldt_ode_scaled_sumsq); nothing else crosses the bus.

        Score evaluation: every sample sits at the same t, so when `score_fn` is the bound `Trainer.score_fn` of an `ldt_amd.Score`
        and there is no label and no condition, `Score.forward_shared_t` is used (ONE AdaLN row per evaluation, LN folding where
        `can_fold` says so; the fold monitor's contract is untouched).  Otherwise the opaque route calls the model with a (B,) time
        vector as the scipy path does: the params of a stock `Trainer.score_fn` (`_params_fn`), or — for any other callable — the
        score it returns, taken as is.  `shared_t` True / False forces a route (True raises where the shared route does not exist).

        Under a sharded batch each rank integrates its own rows with its own step sequence, exactly as on the scipy path: the error
        norm is over the local rows, there is no collective here, and results are therefore not world-size invariant.
        `self.last_ode` keeps {"accepted", "rejected", "t", "route"} of the last call."""
        import time
        from . import ode
        x0 = _initial_latents(num_samples, shape, noise)
        full = tuple(x0.shape)
        B = full[0]
        model = _fused_model(score_fn)
        can_share = model is not None and label is None and condition is None
        if shared_t is None:
            shared_t = can_share
        elif shared_t and not can_share:
            raise ValueError("sample_model_ode: shared_t=True needs the bound Trainer.score_fn of an ldt_amd.Score and no label / condition")
        stock = _is_stock_score_fn(score_fn) and getattr(getattr(score_fn, "__self__", None), "model", None) is not None
        params_of = _params_fn(score_fn) if stock and not shared_t else None
        backend = ode.HipBackend(dev)

        def fun(s, x, k_out):
            th = torch.tensor(-float(s), dtype=torch.float32)                         # the fp32 time every sample shares
            f, g2, sd = float(self.f(th)), float(self.g2(th)), float(torch.sqrt(self.var(th)))
            xb = x.view(full)
            if shared_t:
                p, is_score = model.forward_shared_t(xb, float(th)), False
            else:
                t = torch.full((B,), float(th), dtype=torch.float32, device=dev)
                if params_of is not None:
                    p, is_score = params_of(t, xb, label=label, condition=condition), False
                else:
                    p, is_score = score_fn(t, xb, label=label, condition=condition)[0], True
            backend.rhs(x, p.to(torch.float32), f, g2, sd, k_out, is_score=is_score)

        t0 = time.time()
        y0 = x0.reshape(-1).double().to(dev).contiguous()
        y, nfe, accepted, rejected, trace = ode.rk45_solve(backend, fun, y0, y0.float(), -1.0, -float(ode_eps), ode_solver_tol, ode_solver_tol)
        out = y.to(torch.float32).reshape(full)
        torch.cuda.synchronize(dev)
        self.last_ode = {"accepted": accepted, "rejected": rejected, "t": trace, "route": "shared_t" if shared_t else "opaque"}
        return out, nfe, time.time() - t0

    # ---- the sampler --------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_discrete(self, score_fn, num_samples, N, predictor, corrector, corrector_steps, shape, time_eps,
                        probability_flow, denoise, snr, device, condition=None, label=None, print_steps=None,
                        *, x0=None, noise=None, sample_offset=0, seed=None, use_graph=None, record=None, streams=None, global_batch=None,
                        trajectory=None):
        """Reverse-SDE predictor(-corrector) sampling, diffusion_continuous.py:133-338.

        corrector: None, 'ancestral' (AncestralCorrector :212-229; alpha = 1 by the reference's quirk Q11) or 'langevin'
        (LangevinCorrector :193-210).  predictor 'pndm' runs PNDM (:260-316; corrector / noise are not used by it).
        Langevin and PNDM multiply a (B,1) factor into (B,tokens,z) latents: the reference only runs them when B == 1 or
        B == tokens (the factor is batch-uniform, so the result is well defined then) and raises torch's broadcasting
        error otherwise; the same rule is applied here to the GLOBAL batch (`global_batch`, default num_samples).
        Langevin's step size uses batch means of norms — under a sharded batch the two norm sums are all-reduced (the one
        cross-sample quantity on the path); everything else stays per rank.
        print_steps: the trajectory dump of :239-257 (returns the list of tensors).
        trajectory: a list; the fused loop appends ONE tensor [N, B, tokens, z] holding x after every step (parity curves)."""
        if corrector not in (None, "ancestral", "langevin"):
            raise NotImplementedError("corrector not Implemented")           # diffusion_continuous.py:335
        gb = num_samples if global_batch is None else int(global_batch)
        if predictor == "pndm" or corrector == "langevin":
            if not (gb == 1 or gb == shape[0]) or shape[0] == 1 and gb != 1:
                raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1"
                                   % (gb, shape[0]))                         # what torch raises at :208 / :269
        if predictor == "pndm":
            return self._sample_pndm(score_fn, num_samples, shape, time_eps, device, condition, label, x0)
        ts, coef, mode = self.step_table(N, predictor, time_eps, probability_flow)
        dev = _cuda_device(device, "sample_discrete")
        x = _initial_latents(num_samples, shape, x0, dev)      # drawn before the seed: the order on the CPU generator is part of the contract
        if seed is None:                                       # Philox key from the (seedable) CPU generator; not drawn (the
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0   # reference's stream is kept) when noise is injected
        ncs = corrector_steps if corrector is not None else 0  # noise draws per step: 1 predictor + ncs corrector
        if noise is not None:
            noise = noise.to(dev, torch.float32).contiguous()
            assert noise.shape == (N * (1 + ncs),) + tuple(x.shape), "noise must be [N*(1+corrector_steps), B, tokens, z]"
        run = dict(ts=ts, coef=coef.to(dev), mode=mode, noise=noise, elem_offset=int(sample_offset) * int(np.prod(shape)), seed=seed,
                   denoise=denoise, condition=condition, label=label, trajectory=trajectory)
        model = _fused_model(score_fn)
        if model is not None and record is None and corrector is None and print_steps is None:
            return self._sample_fused(model, x, use_graph=use_graph, streams=streams, **run)
        return self._sample_generic(score_fn, x, corrector=corrector, ncs=ncs, snr=snr, global_batch=gb, sharded=global_batch is not None,
                                    n_valid=max(0, min(num_samples, gb - int(sample_offset))), print_steps=print_steps, record=record, **run)

    def _sample_fused(self, model, x, *, ts, coef, mode, noise, elem_offset, seed, denoise, condition, label, trajectory, use_graph, streams):
        """The fused loop over `x` (placed, fp32, updated in place): one `ldt_sample_loop` call per sub-batch.  -> x_mean if `denoise` else x."""
        dev, N, (B, T) = x.device, ts.numel(), x.shape[:2]
        if use_graph is None:
            use_graph = B * T <= 4096                                                 # launch-bound regime only
        parts = partition(B, _env_streams() if streams is None else streams, int(np.prod(x.shape[1:])), elem_offset)
        shared = condition is None and label is None
        plans = _SharedModulation(model, ts.to(dev), T) if shared else _PerSampleModulation(model, ts.to(dev), T, label, condition)
        x_mean, jobs = torch.empty_like(x), []
        for sb in parts:
            xs = x[sb.lo:sb.hi]                                                       # contiguous row slices, updated in place
            eps_tmp = torch.empty_like(xs)
            tj = None if trajectory is None else torch.empty((N,) + tuple(xs.shape), dtype=torch.float32, device=dev)
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            plan, cond = plans.build(sb, xs)
            nz = None if noise is None else noise[:, sb.lo:sb.hi]
            if nz is not None and len(parts) > 1:
                nz = nz.contiguous()                                                  # [N, Bs, T, z] with step stride Bs*T*z
            jobs.append(_Job(plan, cond, xs, x_mean[sb.lo:sb.hi], eps_tmp, counter, nz, sb.elem_offset, tj))

        def launch(job):                                                              # (on the current stream)
            check(lib().ldt_sample_loop(ctypes.byref(job.plan), job.x.data_ptr(), job.x_mean.data_ptr(), job.eps_tmp.data_ptr(),
                                        coef.data_ptr(), mode, ops._p(job.noise), job.x.numel() if job.noise is not None else 0,
                                        job.elem_offset, seed, job.counter.data_ptr(), N, None if job.cond is None else ctypes.byref(job.cond),
                                        ops._p(job.traj), int(bool(use_graph)), ops.stream_ptr()), "ldt_sample_loop")
        _run_jobs(jobs, launch, dev, sync=not shared)                                 # per-sample scratch must outlive the loop
        if trajectory is not None:
            trajectory.append(torch.cat([j.traj for j in jobs], 1))
        if plans.monitor is not None:
            model.defer_fold_ratio(plans.monitor)                                     # read (a device sync) at the next can_fold(): affects later calls
        return x_mean if denoise else x

    def _corrector(self, corrector, ncs, x, x_mean, ts, snr, noise, elem_offset, seed, global_batch, n_valid, sharded):
        """The update of corrector step j of predictor step i as `(x, params, i, j) -> x`; its draw is noise row / Philox stream
        i (1 + ncs) + 1 + j."""
        dev = x.device
        if corrector == "ancestral":                           # AncestralCorrector :212-229, folded: x_mean = x - 2 snr^2 std params,
            std = self.std(ts).double()                        # x = x_mean + 2 snr std z   (score = -params / std)
            ccoef = torch.stack([torch.ones_like(std), -2.0 * snr * snr * std, 2.0 * snr * std, torch.zeros_like(std)], 1)
            ccoef_d = ccoef.float().contiguous().to(dev)
            return lambda x, params, i, j: ops.sampler_step(
                x, params, ccoef_d, i, 1, noise=None if noise is None else noise[i * (1 + ncs) + 1 + j], x_mean_out=x_mean,
                elem_offset=elem_offset, seed=seed, philox_mul=1 + ncs, philox_add=1 + j)
        if corrector == "langevin":                            # LangevinCorrector :193-210: step size from batch-mean norms, formed on
            std_host = self.std(ts)                            # the device per draw
            scratch = tuple(torch.empty(n, dtype=torch.float32, device=dev) for n in (4, 2, x.shape[0]))   # coef, sums, norms

            def langevin(x, params, i, j):
                k = i * (1 + ncs) + 1 + j
                z = noise[k] if noise is not None else ops.philox_normal(x.shape, dev, seed, step=k, elem_offset=elem_offset)
                return langevin_update(x, params, z, x_mean, float(std_host[i]), snr, global_batch, n_valid, sharded, scratch)
            return langevin

    def _sample_generic(self, score_fn, x, *, ts, coef, mode, noise, elem_offset, seed, denoise, condition, label, trajectory, corrector, ncs,
                        snr, global_batch, n_valid, sharded, print_steps, record):
        """The generic loop: any score_fn, correctors, trajectory dumps; every update is still one HIP kernel, on whatever device `x`
        (placed, fp32) lives.  Draw schedule: predictor step i uses noise row / Philox stream k = i (1 + ncs), its corrector steps the
        ncs after it (tests/test_sampler_schedule_host.py)."""
        dev, N, num_samples = x.device, ts.numel(), x.shape[0]
        ts_d = ts.to(dev)
        x_mean = torch.empty_like(x)
        correct = self._corrector(corrector, ncs, x, x_mean, ts, snr, noise, elem_offset, seed, global_batch, n_valid, sharded)
        out_list, every = None, None
        traj_list = [] if trajectory is not None else None
        if print_steps is not None:
            out_list, every = [x.clone()], (N - 1) // (print_steps - 2)
        params_of = _params_fn(score_fn)
        for i in range(N):
            vec_t = torch.ones((num_samples,), device=dev) * ts_d[i]                 # :243-244
            params = params_of(vec_t, x, label=label, condition=condition)
            k = i * (1 + ncs)                                  # index of this step's first draw (noise row / Philox stream id)
            x_new = ops.sampler_step(x, params.contiguous(), coef, i, mode, noise=None if noise is None else noise[k],
                                     x_mean_out=x_mean, elem_offset=elem_offset, seed=seed, philox_mul=1 + ncs)
            if record is not None:
                record.append((x, params, x_mean.clone(), x_new))
            x = x_new
            for j in range(ncs):
                x = correct(x, params_of(vec_t, x, label=label, condition=condition).contiguous(), i, j)
            if traj_list is not None:
                traj_list.append(x.clone())
            if out_list is not None and (i + 1) % every == 0:
                out_list.append(x_mean.clone())
        if traj_list is not None:
            trajectory.append(torch.stack(traj_list))
        if out_list is not None:
            out_list.append((x_mean if denoise else x).clone())
            return out_list
        return x_mean if denoise else x

    @torch.no_grad()
    def _sample_pndm(self, score_fn, num_samples, shape, time_eps, device, condition, label, x0):
        """PNDM (diffusion_continuous.py:260-316) around the HIP Score: the pseudo linear multistep sampler with three
        Runge-Kutta warm-up steps (4 Score evaluations each), self.N steps over self.train_N training levels.  Every
        sample sits at the same t, so the (B,1) schedule factors of transfer() (:267-271) are three scalars per call,
        formed here in fp32 exactly as upstream; the element-wise updates are HIP kernels.  Index quirk kept: at the last
        step `timesteps[t_next*2 - 1]` with t_next = 0 reads timesteps[-1] = 1.0 (:307)."""
        dev = _cuda_device(device, "sample_discrete")
        N, train_N = self.N, self.train_N
        x = _initial_latents(num_samples, shape, x0, dev)
        betas = torch.from_numpy(np.linspace(self.beta_start / train_N, self.beta_end / train_N, train_N,
                                             dtype=np.float64)).to(torch.float32)                    # :310-313
        alphas_cump = torch.cat((torch.ones(1), (1.0 - betas).cumprod(dim=0)))                     # :314-315 (train_N + 1)
        timesteps = torch.linspace(time_eps, 1.0, N * 2)                                             # :262
        def level(t):                                            # :264-265
            return int((train_N * (t - time_eps) + 1).long())

        def transfer(xx, t, t_next, et):                         # :263-274
            at, at_next = alphas_cump[level(t)], alphas_cump[level(t_next)]
            d = at_next - at
            p = 1 / (at.sqrt() * (at.sqrt() + at_next.sqrt()))
            q = 1 / (at.sqrt() * (((1 - at_next) * at).sqrt() + ((1 - at) * at_next).sqrt()))
            return ops.pndm_transfer(xx, et, float(d), float(p), float(q))

        def eps_at(t, xx):
            vec_t = (torch.ones((num_samples,)) * t).to(dev)
            return params_of(vec_t, xx, condition=condition, label=label).contiguous()

        params_of = _params_fn(score_fn)
        ets = []
        for idx in range(N, 0, -1):                              # :316-317
            t_next = idx - 1
            if len(ets) > 2:                                     # :296-300 linear multistep
                ets.append(eps_at(timesteps[idx * 2 - 1], x))
                ets = ets[-4:]
                noise = ops.lincomb4((ets[-1], ets[-2], ets[-3], ets[-4]), (55.0, -59.0, 37.0, -9.0), 1 / 24)
            else:                                                # :276-292 Runge-Kutta warm-up
                t1, t2, t3 = timesteps[idx * 2 - 1], timesteps[int((idx + t_next) / 2 * 2) - 1], timesteps[int(t_next * 2) - 1]
                e1 = eps_at(t1, x)
                ets.append(e1)
                e2 = eps_at(t2, transfer(x, t1, t2, e1))
                e3 = eps_at(t2, transfer(x, t1, t2, e2))
                e4 = eps_at(t3, transfer(x, t1, t3, e3))
                noise = ops.lincomb4((e1, e2, e3, e4), (1.0, 2.0, 2.0, 1.0), 1 / 6)
            x = transfer(x, timesteps[idx * 2 - 1], timesteps[t_next * 2 - 1], noise)               # :304-307
        return x


class DiffusionVPSDE(DiffusionBase):
    """diffusion_continuous.py:626-678: dz = -beta(t)/2 z dt + sqrt(beta(t)) dW, linear beta(t)."""
    score_kind = 0

    def __init__(self, args):
        super().__init__(args)
        self.beta_start = args.beta_start
        self.beta_end = args.beta_end
        self._init_iw_constants()
        self.train_N = args.train_N
        if args.sample_mode == "discrete":
            self.N = args.sample_N
            self.betas = torch.from_numpy(np.linspace(self.beta_start / self.N, self.beta_end / self.N, self.N,
                                                      dtype=np.float64)).to(torch.float32)
            self.alpha = 1.0 - self.betas
            self.alphas_cump = self.alpha.cumprod(dim=0)

    def score_consts(self):
        return self.beta_start, self.beta_end, self.sigma2_0

    # ---- schedule (tensor in, tensor out; any device) ------------------------------------------
    def g2(self, t):
        return self.beta_start + (self.beta_end - self.beta_start) * t

    def f(self, t):
        return -0.5 * self.g2(t)

    def var(self, t):
        return 1.0 - (1.0 - self.sigma2_0) * torch.exp(
            -self.beta_start * t - 0.5 * (self.beta_end - self.beta_start) * t * t)

    def e2int_f(self, t):
        return torch.exp(-0.5 * self.beta_start * t - 0.25 * (self.beta_end - self.beta_start) * t * t)

    def discrete(self, idx):
        return self.betas.index_select(0, idx), self.alpha.index_select(0, idx)

    def inv_var(self, var):
        return _inv_var_linear_beta(var, self.beta_start, self.beta_end, self.sigma2_0)


class DiffusionSubVPSDE(DiffusionBase):
    """diffusion_continuous.py:681-729: the sub-VP SDE (same drift as the VP-SDE, g2 = beta (1 - exp(-2 int beta))).  It has
    no `betas` table upstream either: the 'ancestral' / 'ddim' predictors raise the reference's AttributeError."""
    score_kind = 1

    def __init__(self, args):
        super().__init__(args)
        self.beta_start = args.beta_start
        self.beta_end = args.beta_end
        self._init_iw_constants()                               # (:691-699: "assumes regular VPSDE")

    def score_consts(self):
        return self.beta_start, self.beta_end, self.sigma2_0

    def beta(self, t):
        return self.beta_start + (self.beta_end - self.beta_start) * t

    def f(self, t):
        return -0.5 * self.beta(t)

    def g2(self, t):
        return self.beta(t) * (1.0 - torch.exp(-2.0 * self.beta_start * t - (self.beta_end - self.beta_start) * t * t))

    def var(self, t):
        int_term = torch.exp(-self.beta_start * t - 0.5 * (self.beta_end - self.beta_start) * t * t)
        return torch.square(1.0 - int_term) + self.sigma2_0 * int_term

    def e2int_f(self, t):
        return torch.exp(-0.5 * self.beta_start * t - 0.25 * (self.beta_end - self.beta_start) * t * t)

    def var_vpsde(self, t):
        """:718-720: the variance of the VP-SDE with the same beta(t) (importance weighting 'like the VP-SDE')."""
        return 1.0 - (1.0 - self.sigma2_0) * torch.exp(
            -self.beta_start * t - 0.5 * (self.beta_end - self.beta_start) * t * t)

    def inv_var_vpsde(self, var):
        """:722-729."""
        return _inv_var_linear_beta(var, self.beta_start, self.beta_end, self.sigma2_0)


class _GeometricVariance(DiffusionBase):
    """var(t) = sigma2_min (sigma2_max / sigma2_min)^t - sigma2_min + sigma2_0, shared by the VE and the geometric SDE."""
    score_kind = 2

    def __init__(self, args):
        super().__init__(args)
        self.sigma2_min = args.sigma2_min
        self.sigma2_max = args.sigma2_max

    def score_consts(self):
        return self.sigma2_min, self.sigma2_max / self.sigma2_min, self.sigma2_0

    def var(self, t):
        return self.sigma2_min * ((self.sigma2_max / self.sigma2_min) ** t) - self.sigma2_min + self.sigma2_0

    def inv_var(self, var):
        """:621-623, :755-757."""
        return torch.log((var + self.sigma2_min - self.sigma2_0) / self.sigma2_min) / np.log(self.sigma2_max / self.sigma2_min)


class DiffusionVESDE(_GeometricVariance):
    """diffusion_continuous.py:732-766: dz = sqrt(beta(t)) dW."""

    def __init__(self, args):
        super().__init__(args)
        assert self.sigma2_min == self.sigma2_0, "VESDE was proposed implicitly assuming sigma2_min = sigma2_0!"

    def f(self, t):
        return torch.zeros_like(t)

    def g2(self, t):
        return self.sigma2_min * np.log(self.sigma2_max / self.sigma2_min) * ((self.sigma2_max / self.sigma2_min) ** t)

    def e2int_f(self, t):
        return torch.ones_like(t)

    def var_N(self, t):
        """:759-760: the variance of the normalised process, 1 - sigma2_min + sigma2_min (sigma2_max / sigma2_min)^t."""
        return 1.0 - self.sigma2_min + self.sigma2_min * ((self.sigma2_max / self.sigma2_min) ** t)

    def inv_var_N(self, var):
        """:762-763."""
        return torch.log((var + self.sigma2_min - 1.0) / self.sigma2_min) / np.log(self.sigma2_max / self.sigma2_min)


class DiffusionGeometric(_GeometricVariance):
    """diffusion_continuous.py:595-623: the VP drift with a geometric progression of the variance."""

    def f(self, t):
        return -0.5 * self.g2(t)

    def g2(self, t):
        sigma2_geom = self.sigma2_min * ((self.sigma2_max / self.sigma2_min) ** t)
        log_term = np.log(self.sigma2_max / self.sigma2_min)
        return sigma2_geom * log_term / (1.0 - self.sigma2_0 + self.sigma2_min - sigma2_geom)

    def e2int_f(self, t):
        return torch.sqrt(
            1.0 + self.sigma2_min * (1.0 - (self.sigma2_max / self.sigma2_min) ** t) / (1.0 - self.sigma2_0))


def _inv_var_linear_beta(var, beta_start, beta_end, sigma2_0):
    """t with 1 - (1 - sigma2_0) exp(-beta_start t - (beta_end - beta_start) t^2 / 2) = var: the positive root of the quadratic
    in t (diffusion_continuous.py:674-678 for the VP-SDE, :722-729 for the sub-VP SDE's VP twin), upstream's operation order."""
    c = torch.log((1 - var) / (1 - sigma2_0))
    a = beta_end - beta_start
    return (-beta_start + torch.sqrt(np.square(beta_start) - 2 * a * c)) / a


def langevin_update(x, params, z, x_mean, std_t, snr, n_total, n_valid, sharded, scratch):
    """One LangevinCorrector update (diffusion_continuous.py:193-210) of this rank's rows.  The step size uses BATCH means of
    per-sample norms — the path's only cross-sample quantity: the two sums are formed over this rank's `n_valid` real rows
    (the zero-padding rows of the last rank do not count; a rank may hold none), all-reduced when the batch is sharded, and
    divided by the GLOBAL batch `n_total`.  scratch = (coef[4], sums[2], norms[rows]) device tensors.  Returns the new x
    (x_mean is written in place)."""
    lv_coef, lv_sums, lv_norms = scratch
    per = x[0].numel()
    if n_valid > 0:
        ops.batch_norm_sum(params, n_valid, per, lv_norms, lv_sums)
        ops.batch_norm_sum(z, n_valid, per, lv_norms, lv_sums[1:])
    else:
        lv_sums.zero_()
    if sharded:
        from . import dist as ldist
        ldist.all_reduce_sum_(lv_sums)
    ops.langevin_coef(lv_sums, n_total, snr, std_t, lv_coef)
    return ops.sampler_step(x, params, lv_coef, 0, 1, noise=z, x_mean_out=x_mean)


def _is_stock_score_fn(score_fn):
    """True for the bound `ldt_amd.Trainer.score_fn` itself (a subclass that overrides it is driven as an opaque callable)."""
    from .trainer import Trainer
    return getattr(score_fn, "__func__", None) is Trainer.score_fn


def _params_fn(score_fn):
    """The samplers only consume `params` (the eps prediction) of `score_fn`'s (score, params) pair.  For the bound,
    un-overridden `Trainer.score_fn` the model is called directly, so the score (-params / std, one more pass over the
    latents per evaluation) is not formed just to be dropped; any other callable is evaluated as given."""
    owner = getattr(score_fn, "__self__", None)
    model = getattr(owner, "model", None)
    if model is not None and _is_stock_score_fn(score_fn):
        return lambda t, x, label=None, condition=None: model(x, t.to(x), label=label, condition=condition)
    return lambda t, x, label=None, condition=None: score_fn(t, x, label=label, condition=condition)[1]


def _fused_model(score_fn):
    """The `ldt_amd.Score` behind a bound `Trainer.score_fn`, else None."""
    from .score import Score
    owner = getattr(score_fn, "__self__", None)
    model = getattr(owner, "model", None)
    if isinstance(model, Score) and not model.host_blocks and _is_stock_score_fn(score_fn):
        return model                                            # (the U-Net / non-LayerNorm variants are driven by the generic loop)
    return None
