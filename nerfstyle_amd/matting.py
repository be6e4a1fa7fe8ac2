"""Photorealism regulariser of the stylisation stage: the matting Laplacian of Levin et al. as Deep Photo Style Transfer uses
it, the reference's MattingLaplacian (loss.py:217-278; constructed at trainers/style.py:54, weighted by photo_lambda).

The reference builds the HW x HW sparse Laplacian in float64 on every call (81 entries per 3x3 window: 61 M entries, ~1.5 GB
at 1008x756), coalesces it and multiplies.  Here one HIP launch (nsr_matting_laplacian, csrc/matting.hip) evaluates
trace(V M V^T) window by window in fp64 and writes d loss / d style_map in the same pass; the backward only scales that
gradient.  The inputs are read as float32 (the renderer's output and the ground-truth frame are float32)."""
import torch
from torch import nn

from . import _lib as L


class _matting_laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, style_map, win_rad, eps):
        ctx.set_materialize_grads(False)
        H, W = int(target.shape[1]), int(target.shape[2])
        t = target.detach().to(torch.float32).contiguous()
        v = style_map.detach().to(torch.float32).contiguous()
        pt, pv = L.p(t), L.p(v)
        dev = t.device
        loss = torch.empty((), dtype=torch.float64, device=dev)
        grad = torch.empty(3, H, W, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        ws = torch.empty(max(1, int(L.lib().nsr_matting_laplacian_workspace_bytes(H, W, win_rad)) // 8), dtype=torch.float64,
                         device=dev)
        L.check(L.lib().nsr_matting_laplacian(pt, pv, H, W, win_rad, float(eps), L.p(loss), L.p(grad), L.p(ws), L.stream()),
                'matting_laplacian')
        ctx.save_for_backward(grad)
        ctx.v_dtype = style_map.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        if go is None or grad is None:
            return None, None, None, None
        return None, (grad * go).to(ctx.v_dtype), None, None


def matting_laplacian(target: torch.Tensor, style_map: torch.Tensor, win_rad: int = 1, eps: float = 1e-7) -> torch.Tensor:
    """target, style_map [3,H,W] on the HIP device -> 0-dim float64 trace(V M V^T), differentiable with respect to style_map.
    No gradient flows to target: one that requires grad is refused."""
    if target.requires_grad:
        raise RuntimeError('matting_laplacian: no gradient with respect to `target`; pass target.detach()')
    if target.dim() != 3 or target.shape[0] != 3 or style_map.shape != target.shape:
        raise ValueError('matting_laplacian: target and style_map must both be [3,H,W]; got {} and {}'.format(
            tuple(target.shape), tuple(style_map.shape)))
    return _matting_laplacian.apply(target, style_map, int(win_rad), float(eps))


class MattingLaplacian(nn.Module):
    """Drop-in for the reference's `loss.MattingLaplacian(device, win_rad=1, eps=1e-7)`: forward(target [3,H,W],
    style_map [3,H,W]) -> float64 scalar.  win_rad in {1, 2}."""

    def __init__(self, device: torch.device = None, win_rad: int = 1, eps: float = 1e-7) -> None:
        super().__init__()
        self.device = device
        self.win_rad = win_rad
        self.eps = eps

    def forward(self, target: torch.Tensor, style_map: torch.Tensor) -> torch.Tensor:
        return matting_laplacian(target, style_map, self.win_rad, self.eps)
