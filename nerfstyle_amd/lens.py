"""Lens refinement: focal length, principal point and two radial terms learnt through the rays, beside the field and the poses
(the "train intrinsics" of instant-ngp's joint refinement).

COLMAP hands LLFF scenes one estimated focal length and no distortion; what is wrong with them a PoseRefiner can only absorb
with 6 F extrinsic parameters that do not represent it.  The rays take the lens as six float32 in device memory,
(fx, fy, cx, cy, k1, k2), through generate_rays(..., lens=) / generate_rays_frames(..., lens=) / Renderer.render(..., lens=) /
Renderer.render_frames(..., lens=); include/nsr.h states the model (nsr_generate_rays_lens) and the gradient
(nsr_generate_rays_lens_backward, one deterministic fp64 sum per parameter).  k1, k2 scale the pinhole coordinates in the
UNPROJECTION direction, pixel to ray: s = 1 + r2 (k1 + r2 k2).  They are not OpenCV's forward coefficients."""
import torch
from torch import nn

from .common import Intrinsics


class LensRefiner(nn.Module):
    """Three parameters, so that a torch Adam can give each a group (and a rate) of its own, all zero at the start:
    `log_focal` [2] (fx, fy scale by exp), `center` [2] (pixels added to cx, cy) and `dist` [2] (k1, k2).
    forward() -> [6] = (fx0 exp(lf0), fy0 exp(lf1), cx0 + c0, cy0 + c1, k1, k2), what the ray functions take as `lens`; at zero
    exactly the intrinsics it was made from, and with them the rays of the lens-less calls bit for bit.
    intrinsics() -> an Intrinsics with the current focal lengths and centre, for logging and checkpoints (host floats: it
    synchronises).
    The gradient arrives through Renderer.pose_gradients = True, as PoseRefiner.delta's does."""

    def __init__(self, intr: Intrinsics):
        super().__init__()
        self.h, self.w = int(intr.h), int(intr.w)
        self.register_buffer('base', torch.tensor([float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy)], dtype=torch.float32))
        self.log_focal = nn.Parameter(torch.zeros(2, dtype=torch.float32))
        self.center = nn.Parameter(torch.zeros(2, dtype=torch.float32))
        self.dist = nn.Parameter(torch.zeros(2, dtype=torch.float32))

    def forward(self):
        return torch.cat((self.base[:2] * torch.exp(self.log_focal), self.base[2:] + self.center, self.dist))

    def intrinsics(self) -> Intrinsics:
        fx, fy, cx, cy = (float(v) for v in self.forward().detach()[:4].cpu())
        return Intrinsics(self.h, self.w, fx, fy, cx, cy)
