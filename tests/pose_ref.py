"""Reference for the camera pose gradients (torch, CPU): a differentiable restatement of generate_rays, the marched samples
re-attached to their rays as xyz = o + t d with t taken from the marched positions and detached (the convention: the march's
parameters, the set of samples and the depth normalisation are constants), then oracle.torch_port.Field and
torch_port.composite_marched with the white-background epilogue and an MSE loss."""
import numpy as np
import torch

from oracle import torch_port as TP


def camera_dirs(w, fx, fy, cx, cy, camera_flip, pix, dtype):
    """camera-frame direction of every pixel id (nerf_lib.py:114-122): ((x + .5 - cx) / fx, (y + .5 - cy) / fy, 1) * flip"""
    pix = torch.as_tensor(np.asarray(pix), dtype=torch.int64)
    px, py = (pix % w).to(dtype), torch.div(pix, w, rounding_mode='floor').to(dtype)
    f = [-1.0 if (camera_flip >> b) & 1 else 1.0 for b in (2, 1, 0)]
    return torch.stack((((px + 0.5) - cx) / fx * f[0], ((py + 0.5) - cy) / fy * f[1], torch.full_like(px, f[2])), dim=1)


def generate_rays(pose, w, fx, fy, cx, cy, camera_flip, pix):
    """pose [3,4] | [4,4] (its dtype is the working precision) -> (origins [N,3], unit directions [N,3])"""
    c = camera_dirs(w, fx, fy, cx, cy, camera_flip, pix, pose.dtype)
    v = c @ pose[:3, :3].t()
    return pose[:3, 3].expand(c.shape[0], 3), v / v.norm(dim=1, keepdim=True)


def sample_rays(rays_info, n_samples):
    """ray row (position in rays_info, which is what origins / directions are indexed by) of every sample slot below n_samples"""
    owner = np.full(n_samples, -1, np.int64)
    for n, (_, off, cnt) in enumerate(np.asarray(rays_info)):
        owner[off:min(off + cnt, n_samples)] = n
    assert np.all(owner >= 0), 'a slot below the count belongs to no ray'
    return torch.as_tensor(owner)


def march_parameters(pose0, cam, pix, xyzs, rays_info):
    """t [n] of the marched samples: (xyz - o) . d on the rays of the pose the march ran with -- a constant of differentiation"""
    with torch.no_grad():
        o, d = generate_rays(pose0, *cam, pix)
        owner = sample_rays(rays_info, xyzs.shape[0])
        idx = torch.as_tensor(np.asarray(rays_info)[:, 0].astype(np.int64))
        o, d = o[idx][owner], d[idx][owner]
        return ((torch.as_tensor(xyzs, dtype=pose0.dtype) - o) * d).sum(dim=1)


def positions(pose, cam, pix, t, rays_info):
    """the marched samples as o + t d of the rays of `pose` (rays_info[n, 0] names the row of the ray batch of march row n)"""
    o, d = generate_rays(pose, *cam, pix)
    owner = sample_rays(rays_info, t.shape[0])
    idx = torch.as_tensor(np.asarray(rays_info)[:, 0].astype(np.int64))
    return o[idx][owner] + t.to(pose.dtype)[:, None] * d[idx][owner]


def render_loss(pose, cam, pix, t, deltas, rays_info, capacity, field, target, density_scale=1.0, T_thresh=1e-4, half=None,
                table_half=False):
    """MSE of the training render's rgb_map against target [N,3] as a function of the pose.  t (march_parameters) / deltas: the
    slots below the march's count; capacity: the M of its drop test."""
    pts = positions(pose, cam, pix, t, rays_info)
    out, sigmas = field(pts, half=half, table_half=table_half)
    sigmas = sigmas[:, 0] * density_scale
    deltas = torch.as_tensor(deltas, dtype=pose.dtype)
    if t.shape[0] < capacity:                 # composite_marched drops a ray that ends at the buffer's end: one slot of padding
        sigmas, out, deltas = (torch.cat((a, torch.zeros_like(a[:1]))) for a in (sigmas, out, deltas))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(pose.dtype)          # composite_marched allocates its outputs in the default type
    try:
        ws, _, image = TP.composite_marched(sigmas, out, deltas, torch.as_tensor(np.asarray(rays_info)), T_thresh)
    finally:
        torch.set_default_dtype(prev)
    rgb_map = image[:, :3] + (1 - ws)[:, None]
    return ((rgb_map - torch.as_tensor(target, dtype=pose.dtype)) ** 2).mean(), rgb_map
