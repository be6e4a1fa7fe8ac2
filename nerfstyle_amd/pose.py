"""Camera pose refinement: one se(3) correction per frame on top of the dataset's poses (the "train extrinsics" of instant-ngp,
the camera optimiser of nerfstudio, BARF).  Plain torch, off the hot path: a [3,4] matrix per step, or all of them ([F,3,4], forward_all) for a step whose rays come from
many frames; the gradient comes from `Renderer.render(pose, ..., training=True)` / `Renderer.render_frames(poses, batch)` with
`Renderer.pose_gradients = True` (nsr_generate_rays_backward, nsr_generate_rays_frames_backward and friends)."""
import torch
import torch.nn as nn


def _skew(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack((torch.stack((z, -w[2], w[1])), torch.stack((w[2], z, -w[0])), torch.stack((-w[1], w[0], z))))


def se3_exp(delta):
    """delta [6] = (axis-angle w, translation v) -> (R [3,3], t [3]) of exp([w]x, v): R = I + A K + B K^2 (Rodrigues),
    t = (I + B K + C K^2) v, with A = sin(th)/th, B = (1 - cos th)/th^2, C = (1 - A)/th^2 and their Taylor series below
    th^2 = 1e-8, so that value and gradient are finite at zero.  At delta = 0 the result is exactly (I, 0)."""
    w, v = delta[:3], delta[3:]
    t2 = (w * w).sum()
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = torch.sqrt(t2s)
    A = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120, torch.sin(th) / th)
    B = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - torch.cos(th)) / t2s)
    C = torch.where(small, 1 / 6 - t2 / 120 + t2 * t2 / 5040, (1 - torch.sin(th) / th) / t2s)
    K = _skew(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=delta.dtype, device=delta.device)
    return eye + A * K + B * K2, (eye + B * K + C * K2) @ v


def se3_exp_many(delta):
    """se3_exp for delta [F,6] at once -> (R [F,3,3], t [F,3]): the same closed forms and the same series below th^2 = 1e-8 per
    row, exactly (I, 0) for a zero row."""
    w, v = delta[:, :3], delta[:, 3:]
    t2 = (w * w).sum(dim=1)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = torch.sqrt(t2s)
    A = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120, torch.sin(th) / th)
    B = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - torch.cos(th)) / t2s)
    C = torch.where(small, 1 / 6 - t2 / 120 + t2 * t2 / 5040, (1 - torch.sin(th) / th) / t2s)
    z = torch.zeros_like(t2)
    K = torch.stack((torch.stack((z, -w[:, 2], w[:, 1]), dim=1), torch.stack((w[:, 2], z, -w[:, 0]), dim=1),
                     torch.stack((-w[:, 1], w[:, 0], z), dim=1)), dim=1)
    K2 = K @ K
    eye = torch.eye(3, dtype=delta.dtype, device=delta.device)
    A, B, C = A[:, None, None], B[:, None, None], C[:, None, None]
    return eye + A * K + B * K2, ((eye + B * K + C * K2) @ v[:, :, None])[:, :, 0]


class PoseRefiner(nn.Module):
    """poses [F,3,4] (or [F,4,4]) camera-to-world matrices, kept as a buffer; `delta` [F,6] the learnt corrections, zero at the
    start.  forward(frame) -> [3,4] = exp(delta[frame]) o poses[frame]: rotation R(w) R0, translation R(w) t0 + V(w) v;
    forward_all() -> [F,3,4], the same for every frame at once.
    The parameter goes to an ordinary torch.optim.Adam, beside the model's fused optimiser."""

    def __init__(self, poses):
        super().__init__()
        poses = torch.as_tensor(poses, dtype=torch.float32)
        assert poses.dim() == 3 and poses.shape[1] >= 3 and poses.shape[2] == 4, 'poses [F,3,4] or [F,4,4]'
        self.register_buffer('poses', poses[:, :3, :].clone())
        self.delta = nn.Parameter(torch.zeros(poses.shape[0], 6, dtype=poses.dtype))

    def forward(self, frame: int):
        R, t = se3_exp(self.delta[frame])
        P = self.poses[frame].to(R.dtype)
        return torch.cat((R @ P[:, :3], (R @ P[:, 3] + t)[:, None]), dim=1)

    def forward_all(self):
        """-> [F,3,4]: every frame's corrected pose in one batched expression, for Renderer.render_frames; row f is forward(f)"""
        R, t = se3_exp_many(self.delta)
        P = self.poses.to(R.dtype)
        return torch.cat((R @ P[:, :, :3], (R @ P[:, :, 3:] + t[:, :, None])), dim=2)
