import torch
import torch.nn as nn

from ._fn import loss_value
from ..torch_ops import _DISTILL_KINDS


class DistillLoss(nn.Module):
    """``rank(y_pred, y_true) + alpha * kd(y_pred[:, :Nt], teacher)``: a rank loss on the label row plus a distillation term on the
    teacher's scores of a row's own ``Nt`` passages (reference losses/kl_div.py, margin_mse.py; the in-batch columns ``Nt..`` have no
    teacher score and stay out of the term).  ``rank=None``: the distillation term alone (``y_true`` may be None)."""

    def __init__(self, rank="lambda_mrr", kd="margin_mse", alpha=1.0, T=1.0):
        super(DistillLoss, self).__init__()
        if rank not in ("lambda_mrr", "ranknet", None):
            raise ValueError("rank must be 'lambda_mrr', 'ranknet' or None")
        if kd not in _DISTILL_KINDS:
            raise ValueError(f"kd must be one of {_DISTILL_KINDS}")
        if not alpha >= 0.0 or not T > 0.0:
            raise ValueError("need alpha >= 0 and T > 0")
        self.rank, self.kd, self.alpha, self.T = rank, kd, float(alpha), float(T)
        self.last_kd = None          # the unweighted term of the last call (device scalar)

    def forward(self, y_pred, y_true, teacher):
        assert y_pred.dim() == teacher.dim() == 2
        if not y_pred.is_cuda:
            raise RuntimeError("cldrd_amd.losses run on the GPU only (no CPU path)")
        if teacher.shape[0] != y_pred.shape[0] or not 1 <= teacher.shape[1] <= y_pred.shape[1]:
            raise ValueError(f"teacher must be [B, Nt] with 1 <= Nt <= {y_pred.shape[1]}, got {tuple(teacher.shape)}")
        out, _ = torch.ops.cldrd.distill_term(y_pred, teacher, _DISTILL_KINDS.index(self.kd), self.alpha, self.T)
        self.last_kd = out[1].detach()
        if self.rank is None:
            return out[0]
        if y_true is None:
            raise ValueError(f"rank={self.rank!r} needs y_true")
        return loss_value(y_pred, y_true, self.rank) + out[0]
