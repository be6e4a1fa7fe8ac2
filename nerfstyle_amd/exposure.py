"""Per-frame exposure and white balance: a log2 gain per frame and colour channel, learnt beside the field and the poses.

Real captures are auto-exposed; a field that must explain a brighter frame without a gain explains it as view-dependent fog, and
the pose refiner and the error map then chase photometric error that is not geometric.  The gain is applied inside the fused
loss (recon_loss(exposure=...), nsr_recon_loss_exposure): frame f is modelled to have observed rgb_map * 2**exposure[f], and the
kernel returns d loss / d exposure as one deterministic fp64 sum per frame (include/nsr.h states the order)."""
import torch
from torch import nn


class ExposureRefiner(nn.Module):
    """`log2_gain` [F,3]: the learnt log2 gains per frame and colour channel, zero (identity) at the start.
    forward() -> [F,3] float32, what recon_loss takes as `exposure`.  zero_mean: the mean over the frames is subtracted per channel
    (in torch, so autograd projects the gradient) -- a gain common to all frames is indistinguishable from the field's own colours,
    and this fixes the gauge the way instant-ngp does.
    apply(rgb_map, frame) -> rgb_map * 2**forward()[frame]: a render as frame `frame` saw it (frame: an index, or one per row).
    The parameter goes to an ordinary torch.optim.Adam, beside the model's fused optimiser, like PoseRefiner.delta.  Its gradient
    comes out of the fused loss and carries the loss scale (scale * factor), as the gradients of the renderer's outputs do:
    unscale it with the others before the step.  Under data parallelism the caller all-reduces log2_gain.grad as for any torch
    parameter."""

    def __init__(self, num_frames, zero_mean=True):
        super().__init__()
        if int(num_frames) < 1:
            raise ValueError('num_frames: at least one frame')
        self.zero_mean = bool(zero_mean)
        self.log2_gain = nn.Parameter(torch.zeros(int(num_frames), 3, dtype=torch.float32))

    def forward(self):
        e = self.log2_gain
        return e - e.mean(dim=0, keepdim=True) if self.zero_mean else e

    def apply(self, rgb_map, frame=None):
        if frame is None and callable(rgb_map):          # nn.Module.apply(fn), which a parent module's apply() recurses into
            return super().apply(rgb_map)
        assert frame is not None, 'frame: the index of the frame, or one per row of rgb_map'
        return rgb_map * torch.exp2(self.forward()[frame]).to(rgb_map.dtype)
