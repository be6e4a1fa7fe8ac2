"""Ray generation: counterpart of nerf_lib.generate_rays (nerf_lib.py:69-142) + RayBatch's
normalisation (common.py:139-147), done by one device kernel (nsr_generate_rays) instead of a
NumPy meshgrid + H2D copy + einsum per call."""
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import profiling
from .common import Box2D, Intrinsics, RayBatch


def pixel_window(intr: Intrinsics, patch: Optional[Box2D] = None, precrop: float = 1.):
    """(w, h, dx, dy) of the full frame / centre crop / patch (nerf_lib.py:106-113)."""
    W, H = intr.size()
    w, h, dx, dy = W, H, 0, 0
    if precrop < 1.:
        w, h = int(W * precrop), int(H * precrop)
        dx, dy = (W - w) // 2, (H - h) // 2
    if patch is not None:
        dx, dy, w, h = patch.x, patch.y, min(patch.w, W - patch.x), min(patch.h, H - patch.y)
    return w, h, dx, dy


def pixel_ids(intr: Intrinsics, patch: Optional[Box2D] = None, precrop: float = 1., device=None):
    """Row-major pixel ids (y * W + x) of the full frame / centre crop / patch, as the reference
    slices x_coords / y_coords (nerf_lib.py:106-113).  Returns (ids int32 [w*h], w, h, dx, dy)."""
    assert 0. <= precrop <= 1.
    assert precrop >= 1. or patch is None, 'Using both precrop and patch is not supported'
    W, H = intr.size()
    w, h, dx, dy = pixel_window(intr, patch, precrop)
    ys = torch.arange(dy, dy + h, device=device, dtype=torch.int32)
    xs = torch.arange(dx, dx + w, device=device, dtype=torch.int32)
    ids = (ys[:, None] * W + xs[None, :]).reshape(-1)
    return ids, w, h, dx, dy


def _empty_rays(N, device):
    """(rays_o, rays_d) for a forward kernel to fill"""
    return torch.empty(N, 3, dtype=torch.float32, device=device), torch.empty(N, 3, dtype=torch.float32, device=device)


def _backward_inputs(g_o, g_d, workspace_bytes, device):
    """what every ray backward takes: the two incoming gradients as contiguous float32 and its fp64 workspace"""
    return (g_o.to(torch.float32).contiguous(), g_d.to(torch.float32).contiguous(),
            torch.empty(int(workspace_bytes) // 8, dtype=torch.float64, device=device))


def _pad_pose_rows(grad, rows):
    """grad [F,3,4] (or None) as the gradient of poses with `rows` rows: the last rows of [F,4,4] poses never reach the rays"""
    if grad is None or rows == 3:
        return grad
    return torch.cat((grad, torch.zeros(grad.shape[0], 1, 4, dtype=torch.float32, device=grad.device)), dim=1)


def _launch_generate_rays(pose, W, H, fx, fy, cx, cy, camera_flip, ids):
    N = ids.shape[0]
    rays_o, rays_d = _empty_rays(N, pose.device)
    L.check(L.lib().nsr_generate_rays(L.p(pose), W, H, fx, fy, cx, cy, camera_flip, L.p(ids), N, L.p(rays_o), L.p(rays_d), L.stream()),
            'generate_rays')
    return rays_o, rays_d


class _generate_rays_fn(torch.autograd.Function):
    """nsr_generate_rays with a gradient for the pose (nsr_generate_rays_backward): pose [3,4] or [4,4] -> (rays_o, rays_d)."""

    @staticmethod
    def forward(ctx, pose, W, H, fx, fy, cx, cy, camera_flip, ids):
        flat = pose.detach().contiguous()
        ctx.save_for_backward(flat, ids)
        ctx.args = (W, H, fx, fy, cx, cy, camera_flip)
        return _launch_generate_rays(flat, W, H, fx, fy, cx, cy, camera_flip, ids)

    @staticmethod
    def backward(ctx, g_o, g_d):
        pose, ids = ctx.saved_tensors
        N = ids.shape[0]
        g_o, g_d, ws = _backward_inputs(g_o, g_d, L.lib().nsr_generate_rays_backward_workspace_bytes(N), pose.device)
        grad = torch.zeros_like(pose)            # a [4,4] pose: its last row never reaches the rays
        L.check(L.lib().nsr_generate_rays_backward(L.p(pose), *ctx.args, L.p(ids), N, L.p(g_o), L.p(g_d), L.p(ws), L.p(grad),
                                                   L.stream()), 'generate_rays_backward')
        return (grad,) + (None,) * 8


def generate_rays(pose, intr: Intrinsics, img=None, patch: Optional[Box2D] = None, precrop: float = 1.,
                  bsize: Optional[int] = None, camera_flip: int = 0, pix_subset=None, device=None, pose_grad: bool = False,
                  lens=None):
    """Same arguments and returns as the reference (RayBatch, target).  bsize: that many pixels
    drawn without replacement with np.random.choice, exactly like nerf_lib.py:134 (pass
    `pix_subset`, positions into the cropped pixel list, to supply your own / device-side draw).
    img: [C, H, W] tensor -> target [K, C].
    pose_grad (Renderer.pose_gradients): the rays stay attached to a pose tensor that requires grad; by default the pose
    is a constant, as in the reference.
    lens ([6] float32 on the device, LensRefiner.forward()): the rays go through that lens instead of intr's four values
    (nsr_generate_rays_lens with one frame and one segment), and with pose_grad stay attached to it as well."""
    _check_lens(lens)
    device = device or (pose.device if torch.is_tensor(pose) else None)
    pose_in = pose
    pose = torch.as_tensor(pose, dtype=torch.float32, device=device).contiguous()
    device = pose.device
    W, H = intr.size()
    if pix_subset is not None and patch is None and precrop >= 1.:
        # positions into the uncropped frame ARE the pixel ids: no id grid (two aranges, a multiply-add over the frame and a
        # gather -- five launches that a 4 096-ray step notices)
        ids = pix_subset.to(torch.int32).contiguous()
    else:
        ids, w, h, dx, dy = pixel_ids(intr, patch, precrop, device)
        if bsize is not None and pix_subset is None:
            pix_subset = torch.from_numpy(np.random.choice(np.arange(w * h), bsize, replace=False)).to(device)
        if pix_subset is not None:
            ids = ids[pix_subset.long()].contiguous()
    args = (W, H, float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy), int(camera_flip), ids)
    if lens is not None:
        attached = pose_in if torch.is_tensor(pose_in) and pose_in.requires_grad else pose
        rays_o, rays_d = _rays_lens(attached.to(device=device, dtype=torch.float32)[None], lens, W, H, int(camera_flip),
                                    torch.zeros(1, dtype=torch.int32, device=device), ids, ids.shape[0], pose_grad)
    elif pose_grad and torch.is_tensor(pose_in) and pose_in.requires_grad and torch.is_grad_enabled():
        rays_o, rays_d = _generate_rays_fn.apply(pose_in.to(device=device, dtype=torch.float32), *args)
    else:
        rays_o, rays_d = _launch_generate_rays(pose, *args)
    target = None
    if img is not None:
        if H != img.shape[-2] or W != img.shape[-1]:
            img = torch.nn.functional.interpolate(img.unsqueeze(0), size=(H, W)).squeeze(0)
        target = img.reshape(img.shape[0], -1).t()[ids.long()]
    rays = RayBatch.__new__(RayBatch)    # directions are already unit length (normalised in-kernel)
    rays.origins, rays.dirs = rays_o, rays_d
    return rays, target


# ---- mixed-frame batches: S segments of K rays, segment s of frame seg_frame[s] (nsr_generate_rays_frames) ----------------------
def _launch_generate_rays_frames(poses, W, H, fx, fy, cx, cy, camera_flip, seg_frame, pix, K):
    F, S = poses.shape[0], seg_frame.shape[0]
    rays_o, rays_d = _empty_rays(S * K, poses.device)
    with profiling.timed('generate_rays_frames'):
        L.check(L.lib().nsr_generate_rays_frames(L.p(poses), F, W, H, fx, fy, cx, cy, camera_flip, L.p(seg_frame), L.p(pix), S, K,
                                                 L.p(rays_o), L.p(rays_d), L.stream()), 'generate_rays_frames')
    return rays_o, rays_d


class _generate_rays_frames_fn(torch.autograd.Function):
    """nsr_generate_rays_frames with a gradient for the poses (nsr_generate_rays_frames_backward): poses [F,3,4] or [F,4,4] ->
    (rays_o, rays_d)."""

    @staticmethod
    def forward(ctx, poses, W, H, fx, fy, cx, cy, camera_flip, seg_frame, pix, K):
        flat = poses.detach()[:, :3, :].contiguous()
        ctx.save_for_backward(flat, seg_frame, pix)
        ctx.args, ctx.K, ctx.rows = (W, H, fx, fy, cx, cy, camera_flip), K, poses.shape[1]
        return _launch_generate_rays_frames(flat, W, H, fx, fy, cx, cy, camera_flip, seg_frame, pix, K)

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, seg_frame, pix = ctx.saved_tensors
        F, S, K, dev = poses.shape[0], seg_frame.shape[0], ctx.K, poses.device
        g_o, g_d, ws = _backward_inputs(g_o, g_d, L.lib().nsr_generate_rays_frames_backward_workspace_bytes(F, S, K), dev)
        grad = torch.empty(F, 3, 4, dtype=torch.float32, device=dev)
        with profiling.timed('generate_rays_frames_bwd'):
            L.check(L.lib().nsr_generate_rays_frames_backward(L.p(poses), F, *ctx.args, L.p(seg_frame), L.p(pix), S, K, L.p(g_o),
                                                              L.p(g_d), L.p(ws), L.p(grad), L.stream()), 'generate_rays_frames_backward')
        return (_pad_pose_rows(grad, ctx.rows),) + (None,) * 10


def generate_rays_frames(poses, seg_frame, pix, K: int, intr: Intrinsics, camera_flip: int = 0, pose_grad: bool = False,
                         lens=None) -> RayBatch:
    """Rays of a mixed-frame batch: poses [F,3,4] (or [F,4,4]), seg_frame [S] int32 and pix [S*K] int32 on the device (what
    ResidentDataset.draw returns); ray n is pixel pix[n] of frame seg_frame[n // K], bit for bit the ray generate_rays makes
    from that frame's pose.  One set of intrinsics for all frames.  A seg_frame entry outside [0, F) gives NaN rays.
    pose_grad (Renderer.pose_gradients): the rays stay attached to a `poses` tensor that requires grad; its gradient is the
    per-frame sum, zero rows for frames the batch does not name.
    lens ([6] float32 on the device, LensRefiner.forward()): one lens for all frames instead of intr's four values
    (nsr_generate_rays_lens); with pose_grad the rays stay attached to it as well, one autograd node for both gradients."""
    _check_lens(lens)
    assert poses.dim() == 3 and poses.shape[1] in (3, 4) and poses.shape[2] == 4, 'poses [F,3,4] or [F,4,4]'
    assert seg_frame.dtype == torch.int32 and pix.dtype == torch.int32 and pix.numel() == seg_frame.numel() * K, \
        'seg_frame [S] int32, pix [S*K] int32'
    W, H = intr.size()
    args = (W, H, float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy), int(camera_flip), seg_frame, pix, int(K))
    if lens is not None:
        rays_o, rays_d = _rays_lens(poses.to(torch.float32), lens, W, H, int(camera_flip), seg_frame, pix, int(K), pose_grad)
    elif pose_grad and poses.requires_grad and torch.is_grad_enabled():
        rays_o, rays_d = _generate_rays_frames_fn.apply(poses.to(torch.float32), *args)
    else:
        rays_o, rays_d = _launch_generate_rays_frames(poses.detach().to(torch.float32)[:, :3, :].contiguous(), *args)
    rays = RayBatch.__new__(RayBatch)    # directions are already unit length (normalised in-kernel)
    rays.origins, rays.dirs = rays_o, rays_d
    return rays


# ---- lens refinement: the same batches through a lens in device memory (nsr_generate_rays_lens) ---------------------------------
def _check_lens(lens):
    if lens is not None and not (torch.is_tensor(lens) and tuple(lens.shape) == (6,) and lens.dtype == torch.float32):
        raise ValueError('lens: a [6] float32 tensor (fx, fy, cx, cy, k1, k2), LensRefiner.forward()')


def _launch_generate_rays_lens(poses, lens, W, H, camera_flip, seg_frame, pix, K):
    F, S = poses.shape[0], seg_frame.shape[0]
    rays_o, rays_d = _empty_rays(S * K, poses.device)
    with profiling.timed('generate_rays_lens'):
        L.check(L.lib().nsr_generate_rays_lens(L.p(poses), F, W, H, L.p(lens), camera_flip, L.p(seg_frame), L.p(pix), S, K, L.p(rays_o),
                                               L.p(rays_d), L.stream()), 'generate_rays_lens')
    return rays_o, rays_d


class _generate_rays_lens_fn(torch.autograd.Function):
    """nsr_generate_rays_lens with gradients for the poses and the lens (nsr_generate_rays_lens_backward): poses [F,3,4] or
    [F,4,4], lens [6] -> (rays_o, rays_d).  The pose gradient is computed only when the poses want one."""

    @staticmethod
    def forward(ctx, poses, lens, W, H, camera_flip, seg_frame, pix, K):
        flat, lens = poses.detach()[:, :3, :].contiguous(), lens.detach().contiguous()
        ctx.save_for_backward(flat, lens, seg_frame, pix)
        ctx.size, ctx.flip, ctx.K, ctx.rows = (W, H), camera_flip, K, poses.shape[1]
        return _launch_generate_rays_lens(flat, lens, W, H, camera_flip, seg_frame, pix, K)

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, lens, seg_frame, pix = ctx.saved_tensors
        F, S, K, dev = poses.shape[0], seg_frame.shape[0], ctx.K, poses.device
        g_o, g_d, ws = _backward_inputs(g_o, g_d, L.lib().nsr_generate_rays_lens_backward_workspace_bytes(F, S, K), dev)
        grad = torch.empty(F, 3, 4, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        grad_lens = torch.empty(6, dtype=torch.float32, device=dev)
        with profiling.timed('generate_rays_lens_bwd'):
            L.check(L.lib().nsr_generate_rays_lens_backward(L.p(poses), F, *ctx.size, L.p(lens), ctx.flip, L.p(seg_frame), L.p(pix), S, K,
                                                            L.p(g_o), L.p(g_d), L.p(ws), L.p(grad), L.p(grad_lens), L.stream()),
                    'generate_rays_lens_backward')
        return (_pad_pose_rows(grad, ctx.rows), grad_lens if ctx.needs_input_grad[1] else None) + (None,) * 6


def _rays_lens(poses, lens, W, H, camera_flip, seg_frame, pix, K, pose_grad):
    """poses [F,3,4] or [F,4,4] float32 -> (rays_o, rays_d), attached to poses and lens when pose_grad is set and one of them
    requires grad"""
    if pose_grad and torch.is_grad_enabled() and (poses.requires_grad or lens.requires_grad):
        return _generate_rays_lens_fn.apply(poses, lens, W, H, camera_flip, seg_frame, pix, K)
    return _launch_generate_rays_lens(poses.detach()[:, :3, :].contiguous(), lens.detach().contiguous(), W, H, camera_flip, seg_frame,
                                      pix, K)


def frustum_bounds(w: int, h: int, fx, fy, cx, cy, k1=0.0, k2=0.0):
    """(x_lo, x_hi, y_lo, y_hi), host floats computed in fp64: the rectangle in pinhole coordinates that holds every ray of a
    w x h frame, for the frustum test of raymarching.mark_untrained_grid.  Pinhole: the frame's outer pixel edges,
    (0 - cx) / fx .. (w - cx) / fx and likewise y.  With a radial term the bounding rectangle of (x s, y s),
    s = 1 + r2 (k1 + r2 k2) (the lens of nsr_generate_rays_lens), over the four corners of every border pixel; with
    k1 = k2 = 0 exactly the pinhole rectangle."""
    fx, fy, cx, cy, k1, k2 = (np.float64(v) for v in (fx, fy, cx, cy, k1, k2))
    if k1 == 0 and k2 == 0:
        return float((0 - cx) / fx), float((w - cx) / fx), float((0 - cy) / fy), float((h - cy) / fy)
    u, v = np.meshgrid(np.arange(w + 1, dtype=np.float64), np.arange(h + 1, dtype=np.float64))
    border = (u <= 1) | (u >= w - 1) | (v <= 1) | (v >= h - 1)
    x, y = (u[border] - cx) / fx, (v[border] - cy) / fy
    r2 = x * x + y * y
    s = 1 + r2 * (k1 + r2 * k2)
    return float((x * s).min()), float((x * s).max()), float((y * s).min()), float((y * s).max())


def tile_order(w: int, h: int, tile_w: int = 8, tile_h: int = 8, device=None) -> torch.Tensor:
    """Every pixel id of a w x h frame once, visited tile by tile (tile_w x tile_h pixels, row-major inside a tile and over the
    tiles; edge tiles are partial).  For batches that cover the whole frame: `np.random.choice(w * h, w * h, replace=False)`
    (nerf_lib.py:134) is the whole frame in an order the loss -- a sum over the rays -- does not depend on, and in THIS order the
    64 rays of a marching wave cross the same occupancy cells, so the thread-per-ray march loop stops running both of its
    branches for the longest of 64 unrelated rays (bench frame: march 2.37 -> 1.87 ms, step 36.1 -> 34.8 ms)."""
    import numpy as np
    yy, xx = np.divmod(np.arange(w * h, dtype=np.int64), w)
    key = ((yy // tile_h) * ((w + tile_w - 1) // tile_w) + xx // tile_w) * (tile_w * tile_h) + (yy % tile_h) * tile_w + xx % tile_w
    return torch.as_tensor(np.argsort(key, kind='stable'), device=device)
