"""Training losses on the HIP path.

cd_loss restates `CD_loss` (evaluation/loss.py:71-78) over the Chamfer kernels of csrc/chamfer_loss.hip: the nearest neighbours with their
indices, the loss on the device, and its gradient with respect to the estimated cloud (all the reference's reconstruction losses ever
feed).  No CPU fallback: a host tensor raises.  A pair at distance exactly 0 contributes exactly 0 to the gradient (the reference's
inf * 0 there is NaN)."""
from . import ops


def cd_loss(esti, shapes, type="l1", want_grad=False, upstream=1.0):
    """esti [B, n, 3], shapes [B, m, 3] fp32 device tensors -> the loss as a 0-dim device tensor, or (loss, d_esti [B, n, 3]) with
    d_esti = upstream * d loss / d esti.  type: 'l1' (mean sqrt d1 + mean sqrt d2) or 'l2' (mean d1 + mean d2)."""
    d1, i1, d2, i2 = ops.chamfer_nn(esti, shapes)
    loss = ops.cd_loss(d1, d2, type)[0]
    if not want_grad:
        return loss
    return loss, ops.cd_loss_bwd(esti, shapes, i1, i2, type, upstream)
