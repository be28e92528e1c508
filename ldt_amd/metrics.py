"""Generation-quality metrics of the reference's validation loop (evaluation/evaluation_metrics.py), MI355X path.

Same function names / argument order / result keys as the reference module, so `from ldt_amd.metrics import
compute_all_metrics` replaces `from evaluation import compute_all_metrics` (trainer/Latent_SDE_Trainer.py:12,217):

    distChamfer(a, b)                  :23-33     -> (dl, dr)                     ldt_chamfer
    emd_approx(sample, ref)            :40-46     -> match_cost / n               ldt_emd_approx  (approxmatch.cu)
    EMD_CD(...)                        :69-109    -> {'mmd-CD', 'mmd-EMD'}
    _pairwise_EMD_CD_ / _pairwise_CD_  :112-199   -> (N_sample, N_ref) matrices   ldt_chamfer_pairwise / ldt_emd_approx
    knn(Mxx, Mxy, Myy, k)              :202-231   1-NN two-sample test
    lgan_mmd_cov(all_dist)             :234-246   MMD / COV
    compute_all_metrics / compute_CD_metrics / compute_MMD_metrics  :249-321
    unit_cube_grid_point_cloud / entropy_of_occupancy_grid / jensen_shannon_divergence / _jsdiv / jsd_between_point_cloud_sets
                                       :324-439   JSD: occupancy histograms by ldt_occupancy_grid, entropies in float64 numpy

The O(N_sample * N_ref * n * m) work — every cloud pair's Chamfer and EMD — runs in two HIP kernels, one workgroup per
pair with both clouds in LDS; the reference loops over pairs in Python and materialises (B, n, m) matrices.  The
bookkeeping on the resulting (N, N) matrices (min / unique / top-k) is plain torch on the device.  `batch_size` is
accepted for signature parity and ignored (no intermediate is large enough to need chunking).  There is no CPU path.
"""
import warnings

import numpy as np
import torch

from . import ops


def _dev(t):
    if not t.is_cuda:
        raise RuntimeError("metrics: tensors are on %s; the HIP path has no CPU fallback (.cuda() them)" % t.device)
    return t.float().contiguous()


def distChamfer(a, b):
    return ops.chamfer(_dev(a), _dev(b))


def L2_ChamferEval_1000(array1, array2):
    """completion_trainer/Latent_SDE_Trainer.py:41-44: (mean dist1 + mean dist2) * 1000 over the whole batch."""
    dist1, dist2 = distChamfer(array1, array2)
    return (torch.mean(dist1) + torch.mean(dist2)) * 1000


def F1Score(array1, array2, threshold=0.001):
    """completion_trainer/Latent_SDE_Trainer.py:47-53: per-cloud F1 of the two nearest-neighbour precisions at `threshold`
    (squared distance); 0/0 -> 0.  Returns (fscore, precision_1, precision_2)."""
    dist1, dist2 = distChamfer(array1, array2)
    precision_1 = torch.mean((dist1 < threshold).float(), dim=1)
    precision_2 = torch.mean((dist2 < threshold).float(), dim=1)
    fscore = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    fscore[torch.isnan(fscore)] = 0
    return fscore, precision_1, precision_2


def emd_approx(sample, ref):
    """emd_approx_cuda (:40-46): approximate-matching cost / n, one value per cloud pair (sample[b], ref[b])."""
    B, N, N_ref = sample.size(0), sample.size(1), ref.size(1)
    assert N == N_ref, "Not sure what would EMD do in this case"
    return ops.emd_approx(_dev(sample), _dev(ref)) / float(N)


def EMD_CD(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=True, reduced=True, accelerated_emd=True):
    N_sample, N_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    assert N_sample == N_ref, "REF:%d SMP:%d" % (N_ref, N_sample)
    dl, dr = distChamfer(sample_pcs, ref_pcs)
    cd = dl.mean(dim=1) + dr.mean(dim=1)
    emd = emd_approx(sample_pcs, ref_pcs)
    if reduced:
        cd, emd = cd.mean(), emd.mean()
    return {"mmd-CD": cd, "mmd-EMD": emd}


def _pairwise_CD_(sample_pcs, ref_pcs, batch_size=None, verbose=True):
    return ops.chamfer_pairwise(_dev(sample_pcs), _dev(ref_pcs))                 # (N_sample, N_ref)


def _pairwise_EMD_CD_(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=True, accelerated_emd=True):
    s, r = _dev(sample_pcs), _dev(ref_pcs)
    assert s.shape[1] == r.shape[1], "Not sure what would EMD do in this case"
    return ops.chamfer_pairwise(s, r), ops.emd_approx(s, r, pairwise=True) / float(s.shape[1])


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """:202-231 (upstream: GAN-Metrics) — leave-one-out k-NN two-sample test on the stacked distance matrix of
    {x: label 1} U {y: label 0}: a point is predicted "x" when at least k/2 of its k nearest others are x."""
    n0, n1 = Mxx.shape[0], Myy.shape[0]
    is_x = torch.zeros(n0 + n1, dtype=Mxx.dtype, device=Mxx.device)
    is_x[:n0] = 1.
    D = torch.cat([torch.cat([Mxx, Mxy], dim=1), torch.cat([Mxy.t(), Myy], dim=1)], dim=0)
    if sqrt:
        D = D.abs().sqrt()
    D = D.clone()
    D.fill_diagonal_(float("inf"))                               # a point is not its own neighbour
    nearest = D.topk(k, dim=0, largest=False).indices            # [k, n0+n1], per column
    votes = is_x[nearest].sum(dim=0)
    pred = (votes >= k / 2.).to(Mxx.dtype)
    tp, fp = (pred * is_x).sum(), (pred * (1 - is_x)).sum()
    fn, tn = ((1 - pred) * is_x).sum(), ((1 - pred) * (1 - is_x)).sum()
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": tp / (tp + fp + 1e-10), "recall": tp / (tp + fn + 1e-10),
            "acc": (pred == is_x).float().mean()}


def lgan_mmd_cov(all_dist):
    """:234-246 — all_dist (N_sample, N_ref).  MMD: mean over reference clouds of the distance to their nearest sample;
    COV: fraction of reference clouds that are the nearest reference of some sample."""
    n_ref = all_dist.shape[1]
    matched = all_dist.argmin(dim=1).unique().numel()
    return {"mmd": all_dist.min(dim=0).values.mean(), "cov": torch.tensor(matched / float(n_ref)).to(all_dist)}


def _mmd_cov(results, M_rs, tag):
    results.update({"%s-%s" % (k, tag): v for k, v in lgan_mmd_cov(M_rs.t()).items()})


def _one_nn(results, M_rr, M_rs, M_ss, tag):
    results.update({"1-NN-%s-%s" % (tag, k): v for k, v in knn(M_rr, M_rs, M_ss, 1, sqrt=False).items() if "acc" in k})


def _report(results):
    for k, v in results.items():
        print("[%s] %.8f" % (k, v.item()))


def _mmd_part(sample_pcs, ref_pcs):
    results = {}
    M_rs_cd, M_rs_emd = _pairwise_EMD_CD_(ref_pcs, sample_pcs)
    _mmd_cov(results, M_rs_cd, "CD")
    _mmd_cov(results, M_rs_emd, "EMD")
    _report(results)
    return results, M_rs_cd, M_rs_emd


def compute_MMD_metrics(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=True, accelerated_emd=True):
    """:280-296 — MMD / COV under CD and EMD (rows = reference clouds, columns = samples, then transposed)."""
    return _mmd_part(sample_pcs.cuda(), ref_pcs.cuda())[0]


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=True, accelerated_emd=True):
    """:249-277 — MMD / COV plus the 1-NN accuracies under CD and EMD (keys as upstream)."""
    ref_pcs, sample_pcs = ref_pcs.cuda(), sample_pcs.cuda()
    results, M_rs_cd, M_rs_emd = _mmd_part(sample_pcs, ref_pcs)
    M_rr_cd, M_rr_emd = _pairwise_EMD_CD_(ref_pcs, ref_pcs)
    M_ss_cd, M_ss_emd = _pairwise_EMD_CD_(sample_pcs, sample_pcs)
    _one_nn(results, M_rr_cd, M_rs_cd, M_ss_cd, "CD")
    _one_nn(results, M_rr_emd, M_rs_emd, M_ss_emd, "EMD")
    return results


def compute_CD_metrics(sample_pcs, ref_pcs, batch_size=None):
    """:299-321 — the Chamfer-only subset."""
    results = {}
    M_rs_cd = _pairwise_CD_(ref_pcs, sample_pcs)
    _mmd_cov(results, M_rs_cd, "CD")
    _report(results)
    _one_nn(results, _pairwise_CD_(ref_pcs, ref_pcs), M_rs_cd, _pairwise_CD_(sample_pcs, sample_pcs), "CD")
    return results


# ---- JSD (:324-439; from the latent_3d_points evaluation) ---------------------------------------------------------------------
# The occupancy histograms — every point of every cloud to its nearest grid cell — run in ldt_occupancy_grid; the upstream code asks
# sklearn's NearestNeighbors per cloud and counts in Python loops.  What is left is float64 numpy on two G-length vectors.
def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """:324-342 — the cell centres of a resolution^3 grid in the unit cube, float32 (resolution, resolution, resolution, 3), and the
    spacing; clip_sphere keeps the (G, 3) cells with norm <= 0.5.  Each coordinate is `i * spacing - 0.5` in Python float64 rounded
    to float32 on assignment, and the norm is numpy's float32 one, as upstream: the in-sphere mask is upstream's to the bit."""
    spacing = 1.0 / float(resolution - 1)
    axis = np.array([i * spacing - 0.5 for i in range(resolution)], dtype=np.float64).astype(np.float32)
    grid = np.empty((resolution, resolution, resolution, 3), np.float32)
    grid[..., 0] = axis[:, None, None]
    grid[..., 1] = axis[None, :, None]
    grid[..., 2] = axis[None, None, :]
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[np.linalg.norm(grid, axis=1) <= 0.5]
    return grid, spacing


def _entropy(pk, base=None):
    """scipy.stats.entropy(pk, base=base) for a 1-D float64 vector: normalise by the sum, sum -p log p (0 log 0 = 0), divide by log(base)."""
    pk = np.asarray(pk, dtype=np.float64)
    pk = 1.0 * pk / np.sum(pk)
    with np.errstate(divide="ignore", invalid="ignore"):
        vec = np.where(pk > 0, -pk * np.log(pk), np.where(pk == 0, 0.0, -np.inf))
    S = np.sum(vec)
    if base is not None:
        S /= np.log(base)
    return S


def occupancy_counts(pclouds, grid_resolution, in_sphere=False):
    """-> (grid_counters, grid_bernoulli_rvars), int64 numpy [G]: the two histograms of :378-389, from ldt_occupancy_grid.  `pclouds`
    (S, n, 3): a numpy array or a tensor; host data is uploaded.  There is no CPU path."""
    pts = torch.from_numpy(np.ascontiguousarray(pclouds)) if isinstance(pclouds, np.ndarray) else pclouds
    if not pts.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("metrics: point clouds are on %s and there is no device; the HIP path has no CPU fallback" % pts.device)
        pts = pts.cuda()
    grid_coordinates, _ = unit_cube_grid_point_cloud(grid_resolution, in_sphere)
    cells = torch.from_numpy(np.ascontiguousarray(grid_coordinates.reshape(-1, 3))).to(pts.device)
    counters, bernoulli = ops.occupancy_grid(pts.detach().float().contiguous(), cells)
    wide = lambda c: c.cpu().numpy().view(np.uint32).astype(np.int64)               # the kernel's counts are unsigned
    return wide(counters), wide(bernoulli)


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """:359-398 — (the mean over the grid cells of the entropy of the Bernoulli variable "some point of a cloud falls into the cell",
    the float64 per-cell point counts).  pclouds: (#clouds, points, 3), numpy or tensor."""
    epsilon = 10e-4
    bound = 0.5 + epsilon
    if verbose:                                                   # (upstream evaluates both tests always and warns only when verbose)
        p = torch.as_tensor(pclouds)
        if abs(float(p.max())) > bound or abs(float(p.min())) > bound:
            warnings.warn('Point-clouds are not in unit cube.')
        if in_sphere and float(torch.sqrt(torch.sum(p ** 2, dim=2)).max()) > bound:
            warnings.warn('Point-clouds are not in unit sphere.')
    counters, bernoulli = occupancy_counts(pclouds, grid_resolution, in_sphere)
    grid_counters = counters.astype(np.float64)
    n = float(len(pclouds))
    acc_entropy = 0.0
    for g in bernoulli[bernoulli > 0]:                            # upstream's order of accumulation
        p = float(g) / n
        acc_entropy += _entropy([p, 1.0 - p])
    return acc_entropy / len(grid_counters), grid_counters


def jensen_shannon_divergence(P, Q):
    """:401-420."""
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError('Negative values.')
    if len(P) != len(Q):
        raise ValueError('Non equal size.')
    P_ = P / np.sum(P)  # Ensure probabilities.
    Q_ = Q / np.sum(Q)
    e1 = _entropy(P_, base=2)
    e2 = _entropy(Q_, base=2)
    e_sum = _entropy((P_ + Q_) / 2.0, base=2)
    res = e_sum - ((e1 + e2) / 2.0)
    res2 = _jsdiv(P_, Q_)
    if not np.allclose(res, res2, atol=10e-5, rtol=0):
        warnings.warn('Numerical values of two JSD methods don\'t agree.')
    return res


def _jsdiv(P, Q):
    """:423-439 — the same divergence as the mean of two KL terms against the mixture."""
    def _kldiv(A, B):
        idx = np.logical_and(A > 0, B > 0)
        a, b = A[idx], B[idx]
        return np.sum(a * np.log2(a / b))

    P_ = P / np.sum(P)
    Q_ = Q / np.sum(Q)
    M = 0.5 * (P_ + Q_)
    return 0.5 * (_kldiv(P_, M) + _kldiv(Q_, M))


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """:345-356 — the JSD between the occupancy distributions of two sets of clouds (S1, n1, 3) / (S2, n2, 3) on the in-sphere cells of
    a resolution^3 grid (Achlioptas et al., Learning Representations and Generative Models for 3D Point Clouds)."""
    in_unit_sphere = True
    sample_grid_var = entropy_of_occupancy_grid(sample_pcs, resolution, in_unit_sphere)[1]
    ref_grid_var = entropy_of_occupancy_grid(ref_pcs, resolution, in_unit_sphere)[1]
    return jensen_shannon_divergence(sample_grid_var, ref_grid_var)
