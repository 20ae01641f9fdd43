import torch
import torch.nn as nn

from .. import torch_ops  # noqa: F401  (registers torch.ops.cldrd.*)


class SoftmaxCE(nn.Module):
    """Softmax cross-entropy (InfoNCE) of each row's positives against its negatives at ``temperature`` - this package's definition, the
    reference has no such loss (include/cldrd_hip.h: cldrd_softmax_ce).  ``y_true`` [B, Np] decides the classes of a row's columns:
    positive ``label >= pos_min`` (``pos_min=None``: the row's maximum label), negative ``label <= neg_max`` and not positive, the rest
    neutral (in neither sum, no gradient).  ``pids`` (int64 [B, nway], with the scoring ``mode`` 0 / 1 / 2 of the logits): a negative whose
    passage id is also behind a positive or neutral column of its row becomes neutral.  ``last_valid``: the valid-row count of the last call
    (device scalar)."""

    def __init__(self, temperature=1.0, pos_min=None, neg_max=0.0, reduction="mean"):
        super(SoftmaxCE, self).__init__()
        if not float(temperature) > 0.0:
            raise ValueError("temperature must be > 0")
        if pos_min is not None and not float(pos_min) > float(neg_max):
            raise ValueError("pos_min must be > neg_max")
        if reduction not in ("mean", "sum"):
            raise ValueError("Reduction method can be either sum or mean")
        self.temperature, self.neg_max, self.reduction = float(temperature), float(neg_max), reduction
        self.pos_min = None if pos_min is None else float(pos_min)
        self.last_valid = None

    def forward(self, y_pred, y_true, pids=None, mode=0, nway=None):
        assert y_pred.dim() == y_true.dim() == 2
        if not y_pred.is_cuda:
            raise RuntimeError("cldrd_amd.losses run on the GPU only (no CPU path)")
        if pids is not None and nway is not None and pids.shape[1] != nway:
            raise ValueError(f"pids must be [B, nway = {nway}], got {tuple(pids.shape)}")
        out, _ = torch.ops.cldrd.softmax_ce(y_pred, y_true, pids, int(mode), self.temperature, self.pos_min, self.neg_max,
                                            self.reduction == "mean")
        self.last_valid = out[1].detach()
        return out[0]
