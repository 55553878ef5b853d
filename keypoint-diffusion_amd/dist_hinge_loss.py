"""`DistanceHingeLoss`: upstream's losses/dist_hinge_loss.py on the segmented HIP kernel (kpd_dist_hinge, csrc/dist_hinge.hip).

loss = sum_{i,j} max(thr - ||a_i - b_j||, 0) over every pair (cross mode) or over the pairs i < j of one point set (self mode,
`pos_b=None`).  `segmented_dist_hinge` evaluates it for a whole batch of (A, B) segments in one launch -- the model's receptor-ligand
term (ligand_diffuser.py) -- and returns the total and the per-segment losses.  The gradients are computed by the forward launch
for whichever inputs require them; backward only scales them by the incoming gradient.  GPU only: there is no CPU path.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import hip


class _DistHingeFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pos_a, a_ptr, pos_b, b_ptr, threshold):
        need_a = ctx.needs_input_grad[0]
        need_b = pos_b is not None and ctx.needs_input_grad[2]
        seg, total, ga, gb = hip.dist_hinge(pos_a.detach(), a_ptr, None if pos_b is None else pos_b.detach(), b_ptr, threshold,
                                            grad_a=need_a, grad_b=need_b)
        ctx.grads = (ga, gb)
        ctx.mark_non_differentiable(seg)
        return total[0], seg

    @staticmethod
    def backward(ctx, d_total, d_seg):
        ga, gb = ctx.grads
        ctx.grads = None
        return (None if ga is None else ga * d_total, None, None if gb is None else gb * d_total, None, None)


def segmented_dist_hinge(pos_a: torch.Tensor, a_ptr: torch.Tensor, pos_b: Optional[torch.Tensor], b_ptr: Optional[torch.Tensor],
                         threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total, per-segment losses [S]) of the hinge over S segments: segment s pairs rows [a_ptr[s], a_ptr[s+1]) of pos_a with rows
    [b_ptr[s], b_ptr[s+1]) of pos_b (int32 GPU offsets [S+1]); pos_b = b_ptr = None pairs each A segment with itself (i < j).
    The total is differentiable with respect to pos_a and pos_b; each segment's value is bitwise independent of the others."""
    return _DistHingeFn.apply(pos_a, a_ptr, pos_b, b_ptr, float(threshold))


class DistanceHingeLoss(nn.Module):
    """losses/dist_hinge_loss.py:4-25: forward(pos_a [Na,3], pos_b [Nb,3] = None) -> scalar sum of max(thr - d, 0)."""

    def __init__(self, distance_threshold: float):
        super().__init__()
        self.distance_threshold = distance_threshold

    def forward(self, pos_a: torch.Tensor, pos_b: torch.Tensor = None) -> torch.Tensor:
        for name, t in (('pos_a', pos_a), ('pos_b', pos_b)):
            if t is not None and not t.is_cuda:
                raise hip.KpdError(f'DistanceHingeLoss: {name} must live on the GPU (got {t.device}); there is no CPU implementation')

        def single(t):
            ptr = torch.zeros(2, dtype=torch.int32, device=t.device)      # [0, n] without a host -> device copy
            ptr[1] = t.shape[0]
            return ptr

        total, _ = segmented_dist_hinge(pos_a, single(pos_a), pos_b, None if pos_b is None else single(pos_b), self.distance_threshold)
        return total
