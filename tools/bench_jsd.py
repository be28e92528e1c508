"""Time of the JSD metric at the evaluation size: ldt_occupancy_grid by HIP events (warm-up, then the median of several calls) and
`jsd_between_point_cloud_sets` end to end (wall clock, host bookkeeping and the upload included).
    python tools/bench_jsd.py [N_clouds] [calls]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ldt_amd import metrics, ops  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n, res = 2048, 28
g = torch.Generator().manual_seed(0)


def clouds(scale):
    """blobs normalised like the reference's ShapeNet loader: the farthest point of a cloud at `scale`"""
    p = torch.randn(S, n, 3, generator=g) * torch.rand(S, 1, 3, generator=g).clamp_min(0.15)
    return p / p.norm(dim=2).amax(dim=1)[:, None, None] * scale


smp, ref = clouds(0.5), clouds(1.0)
cells = torch.from_numpy(np.ascontiguousarray(metrics.unit_cube_grid_point_cloud(res, True)[0])).cuda()
for name, pts in (("inside the grid", smp.cuda()), ("reaching radius 1", ref.cuda())):
    ops.occupancy_grid(pts, cells)
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        counters = torch.zeros(cells.shape[0], dtype=torch.int32, device="cuda")
        bern = torch.zeros_like(counters)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.occupancy_grid(pts, cells, counters, bern)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    pairs = S * n * cells.shape[0]
    med = float(np.median(ms))
    print("ldt_occupancy_grid %d clouds x %d points x %d cells (%s): median %.3f ms of %d calls (min %.3f, max %.3f) = %.1f G pairs/s"
          % (S, n, cells.shape[0], name, med, CALLS, min(ms), max(ms), pairs / med / 1e6))
smp_np, ref_np = smp.numpy(), ref.numpy()
metrics.jsd_between_point_cloud_sets(smp_np[:2], ref_np[:2], res)
t0 = time.time()
jsd = metrics.jsd_between_point_cloud_sets(smp_np, ref_np, res)
print("jsd_between_point_cloud_sets S = R = %d x %d points from host arrays: %.3f s (JSD %.6f)" % (S, n, time.time() - t0, jsd))
