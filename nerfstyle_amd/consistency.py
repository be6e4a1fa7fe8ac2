"""Multi-view consistency of rendered frames as one fused HIP op (nsr_reproject_frames, csrc/reproject.hip): the warped error
between views that every style-transfer paper on radiance fields reports for the stylisation stage.

A frame and the distance map the field renders for it are reprojected into a neighbouring camera, the pixels that camera cannot
see (out of frame, behind it, occluded, no surface) are discarded, and what is left is compared: short range between neighbouring
frames, long range between frames several apart (sequence_pairs).  include/nsr.h, "View reprojection", states every step; the
geometry is fp64 and the sums have a fixed order, so a number is the same bits from call to call.  Composed in torch the same
result takes a grid_sample, gathers and masked reductions, a dozen full-frame passes a pair.

Renderer.render_rgbd supplies the distance maps and Renderer.view_consistency the whole protocol."""
import torch

from . import _lib as L


def sequence_pairs(F, gap):
    """-> [(i, i + gap)] for i in 0 .. F - gap - 1: frame i is the destination, frame i + gap the source.  gap = 1 is the
    short-range protocol, a larger gap the long-range one."""
    F, gap = int(F), int(gap)
    if F < 1:
        raise ValueError('sequence_pairs: F must be >= 1; got {}'.format(F))
    if gap < 1:
        raise ValueError('sequence_pairs: gap must be >= 1; got {}'.format(gap))
    return [(i, i + gap) for i in range(F - gap)]


def _host_pairs(pairs, F):
    """pairs as a CPU int32 tensor [P, 2], every index checked against [0, F) on the host"""
    if torch.is_tensor(pairs):
        if pairs.is_cuda:
            raise ValueError('reproject_frames: pairs must be a Python sequence or a CPU tensor (it is validated on the host)')
        if pairs.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError('reproject_frames: pairs must be an integer tensor; got {}'.format(pairs.dtype))
        t = pairs.to(torch.int64)
    else:
        rows = [tuple(r) for r in pairs]
        if any(len(r) != 2 for r in rows):
            raise ValueError('reproject_frames: pairs must be [P, 2] (dst, src)')
        if any(int(v) != v for r in rows for v in r):
            raise ValueError('reproject_frames: pairs must be integers')
        t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError('reproject_frames: pairs must be [P, 2] (dst, src); got {}'.format(tuple(t.shape)))
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= F):
        raise ValueError('reproject_frames: pairs name a frame outside [0, {})'.format(F))
    return t.to(torch.int32).contiguous()


def _check(name, t, shape, what):
    """a float32, contiguous device tensor of `shape` (read in place: nothing is copied or cast)"""
    if not torch.is_tensor(t):
        raise TypeError('reproject_frames: {} must be a tensor'.format(name))
    if tuple(t.shape) != tuple(shape):
        raise ValueError('reproject_frames: {} must be {} {}; got {}'.format(name, what, tuple(shape), tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError('reproject_frames: {} must be float32; got {}'.format(name, t.dtype))
    if not t.is_contiguous():
        raise ValueError('reproject_frames: {} must be contiguous'.format(name))


@torch.no_grad()
def reproject_frames(rgb, dist, poses, intr, pairs, camera_flip=0, depth_tol=0.01, want_warped=True, want_mask=True):
    """Warps frame b into camera a for every (a, b) of pairs -> (warped [P, H*W, 3] float32 | None, mask [P, H*W] uint8 | None,
    stats [P, 2] float64 = (sse, n_valid)), all on the device; warp_error turns stats into (rmse, coverage).
    rgb: [F, H*W, 3] or [F, H, W, 3]; dist: [F, H*W] or [F, H, W], the distance from the camera origin along the pixel's unit ray,
    anything not finite or not > 0 meaning no surface (Renderer.render_rgbd's 'distance'); poses: [F, 3, 4] camera to world;
    intr: the Intrinsics of the frames (H, W >= 2); pairs: a Python sequence or a CPU integer tensor [P, 2] of (dst, src), checked
    on the host; depth_tol: the relative tolerance of the occlusion test.  All three tensors float32, contiguous, on one device.
    No gradient and no host read of device memory."""
    H, W = int(intr.h), int(intr.w)
    if W < 2 or H < 2:
        raise ValueError('reproject_frames: the bilinear taps need W >= 2 and H >= 2; got W = {}, H = {}'.format(W, H))
    if not (float(depth_tol) >= 0.0):
        raise ValueError('reproject_frames: depth_tol must be >= 0; got {}'.format(depth_tol))
    if not 0 <= int(camera_flip) <= 7:
        raise ValueError('reproject_frames: camera_flip must be in 0..7; got {}'.format(camera_flip))
    if not torch.is_tensor(rgb) or rgb.dim() not in (3, 4):
        raise ValueError('reproject_frames: rgb must be [F, H*W, 3] or [F, H, W, 3]')
    F = int(rgb.shape[0])
    if F < 1:
        raise ValueError('reproject_frames: no frames')
    _check('rgb', rgb, (F, H, W, 3) if rgb.dim() == 4 else (F, H * W, 3), '[F, H, W, 3]' if rgb.dim() == 4 else '[F, H*W, 3]')
    if not torch.is_tensor(dist) or dist.dim() not in (2, 3):
        raise ValueError('reproject_frames: dist must be [F, H*W] or [F, H, W]')
    _check('dist', dist, (F, H, W) if dist.dim() == 3 else (F, H * W), '[F, H, W]' if dist.dim() == 3 else '[F, H*W]')
    _check('poses', poses, (F, 3, 4), '[F, 3, 4]')
    pairs = _host_pairs(pairs, F)
    if dist.device != rgb.device or poses.device != rgb.device:
        raise ValueError('reproject_frames: rgb, dist and poses are on different devices')
    if not rgb.is_cuda:
        raise RuntimeError('reproject_frames: rgb, dist and poses are {} tensors; nerfstyle_amd kernels need HIP device tensors '
                           '(there is no CPU fallback)'.format(rgb.device))
    P, dev = int(pairs.shape[0]), rgb.device
    stats = torch.zeros(P, 2, dtype=torch.float64, device=dev)
    warped = torch.empty(P, H * W, 3, dtype=torch.float32, device=dev) if want_warped else None
    mask = torch.empty(P, H * W, dtype=torch.uint8, device=dev) if want_mask else None
    if P == 0:
        return warped, mask, stats
    nbytes = int(L.lib().nsr_reproject_frames_workspace_bytes(P, H, W))
    if nbytes == 0:
        raise ValueError('reproject_frames: {} pairs of {} x {} pixels are more than one call takes'.format(P, W, H))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    pairs_dev = pairs.to(dev)
    with torch.cuda.device(dev):
        L.check(L.lib().nsr_reproject_frames(L.p(rgb), L.p(dist), L.p(poses), F, H, W, float(intr.fx), float(intr.fy), float(intr.cx),
                                             float(intr.cy), int(camera_flip), L.p(pairs_dev), P, float(depth_tol), L.p(warped),
                                             L.p(mask), L.p(stats), L.p(ws), L.stream()), 'reproject_frames')
    return warped, mask, stats


def warp_error(stats, H, W):
    """stats [P, 2] (sse, n_valid) of reproject_frames -> [P, 2] float64 (rmse, coverage) on the device of stats:
    rmse = sqrt(sse / (3 n_valid)) over the pixels both cameras see, NaN where there is none; coverage = n_valid / (H W).
    No host read."""
    if not torch.is_tensor(stats) or stats.dim() != 2 or stats.shape[1] != 2:
        raise ValueError('warp_error: stats must be [P, 2] (sse, n_valid)')
    s = stats.to(torch.float64)
    sse, n = s[:, 0], s[:, 1]
    rmse = torch.sqrt(sse / (3.0 * n))                   # 0 / 0 = NaN where no pixel is valid
    return torch.stack((rmse, n / float(int(H) * int(W))), dim=1)
