"""What the evaluation loops of the three trainer modules share (trainer.py, hybrid_trainer.py, compressor_trainer.py), each step said once as
a plain function of what it needs: the references of a test loader (`collect_refs`), the matching clouds through a `sample_fn` with the
clock around each call (`sample_clouds`), the encode / reconstruct / de-normalise loop (`reconstruct`), the `val/gen/<key>` report, the
`.npy` dump into cfg.log.save_path, the `vis=True` refusal, the checkpoint path and the learning-rate warm-up.  What differs between the
reference's trainers — which fields de-normalise, whether a label is passed, who prints, who dumps — is an argument at the call site.
Plain torch on finished tensors; nothing here launches a kernel of its own."""
import math
import os
import time

import numpy as np
import torch


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def refuse_vis(who, vis):
    if vis:
        raise NotImplementedError("%s(vis=True): mitsuba rendering (tools/vis_utils.py) is not on this path" % who)


def warm_up(cfg, optimizer, itr):
    """trainer/base.py:32-37: the linear learning-rate warm-up over cfg.opt.warmup_iters."""
    if itr < cfg.opt.warmup_iters:
        lr = cfg.opt.lr * min(float(itr + 1) / max(cfg.opt.warmup_iters, 1), 1.0)
        for param_group in optimizer.param_groups:
            param_group["lr"] = lr


def checkpoint_path(cfg, epoch=None):
    """`<cfg.log.save_path>/checkpt_<epoch>.pth`; `epoch` None: the last row of `training.csv` there."""
    if epoch is None:
        import csv
        with open(os.path.join(cfg.log.save_path, "training.csv")) as f:
            epoch = int(float(list(csv.DictReader(f))[-1]["epoch"]))
    return os.path.join(cfg.log.save_path, "checkpt_{:}.pth".format(epoch))


def dump(cfg, name, clouds, chief=True):
    """`clouds` as `<cfg.log.save_path>/<name>` when a save path is set (and this rank is the one that writes)."""
    path = getattr(getattr(cfg, "log", None), "save_path", "") or ""
    if path and chief:
        np.save(os.path.join(path, name), clouds.detach().cpu().numpy())


def report(epoch, gen_res, chief=True):
    """The summary print and the returned `{"val/gen/<key>": float}` dict of `compute_all_metrics`'s result."""
    if chief:
        print("Validation Sample (unit) Epoch:%d " % epoch, gen_res)
    return {("val/gen/%s" % k): (v if isinstance(v, float) else v.item()) for k, v in gen_res.items()}


def collect_refs(test_loader, device, who, val_cate=None, batch_size=None, fields=()):
    """-> (ref (n, points, 3) fp32 on the device, sizes, [data[f] rows of the references, fp32 on the device, for f in fields]).
    val_cate None: every batch's `te_points`, sizes = len(batch['tr_points']) per batch.  Otherwise the rows with `cate_idx == val_cate`
    and sizes = ceil(n / batch_size) batches of batch_size; no such row is a ValueError in `who`'s name."""
    cols, sizes = [[] for _ in range(1 + len(fields))], []
    for data in test_loader:
        rows = slice(None) if val_cate is None else data["cate_idx"] == val_cate
        for col, key in zip(cols, ("te_points",) + tuple(fields)):
            col.append(data[key][rows])
        if val_cate is None:
            sizes.append(data["tr_points"].size(0))
    if val_cate is not None and sum(c.shape[0] for c in cols[0]) == 0:
        raise ValueError("%s: no test shape has cate_idx == %r" % (who, val_cate))
    ref, *rest = (torch.cat(col, dim=0).float().to(device) for col in cols)
    if val_cate is not None:
        sizes = [batch_size] * math.ceil(ref.shape[0] / batch_size)
    return ref, sizes, rest


def sample_clouds(sample_fn, sizes, device, label=None):
    """One `sample_fn(num_samples=n)` per entry of sizes (with `label=` n times the category `label` as int32 on the device, when given)
    -> (the clouds concatenated, the seconds spent inside sample_fn with the device drained before and after each call)."""
    clouds, seconds = [], 0.
    for n in sizes:
        kw = {} if label is None else {"label": (torch.ones(n) * label).int().to(device)}
        _sync(device)
        t0 = time.time()
        clouds.append(sample_fn(num_samples=n, **kw))
        _sync(device)
        seconds += time.time() - t0
    return torch.cat(clouds, dim=0), seconds


def reconstruct(model, test_loader, cfg, device, val_cate, who, *, fields, with_label):
    """Encode and reconstruct the test shapes with `model(points)['set']` and de-normalise both -> (rec, ref).
    cfg.data.num_categorys == 1: batch by batch as the loader yields them, by the loader's `shift` / `scale`.  Otherwise: the shapes with
    `cate_idx == val_cate`, re-batched by cfg.data.test_batch_size, de-normalised by fields = (shift key, scale key); with_label: each
    re-batched call gets `label=` its size times val_cate as int32."""
    if cfg.data.num_categorys == 1:
        all_ref, all_rec = [], []
        for data in test_loader:
            ref_pts = data["te_points"].to(device).float()
            rec_pts = model(ref_pts)["set"]
            shift, scale = data["shift"].float().to(device), data["scale"].float().to(device)
            all_ref.append(ref_pts * scale + shift)
            all_rec.append(rec_pts * scale + shift)
        return torch.cat(all_rec, dim=0), torch.cat(all_ref, dim=0)
    pts, _, (shift, scale) = collect_refs(test_loader, device, who, val_cate, cfg.data.test_batch_size, fields)
    all_rec, bsize = [], cfg.data.test_batch_size
    for i in range(math.ceil(pts.shape[0] / bsize)):
        chunk = pts[i * bsize:(i + 1) * bsize]
        kw = {"label": (torch.ones(chunk.shape[0]) * val_cate).int().to(device)} if with_label else {}
        all_rec.append(model(chunk, **kw)["set"])
    return torch.cat(all_rec, dim=0) * scale + shift, pts * scale + shift
