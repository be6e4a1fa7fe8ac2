"""Structural similarity of rendered frames as one fused HIP op (nsr_ssim, csrc/ssim.hip): the metric every NeRF table reports
beside PSNR, and the D-SSIM loss term lambda * (1 - SSIM) of 3DGS and many NeRF variants.

Wang et al. 2004 in the form 3DGS and pytorch-ssim use: three channels, data range 1, an 11-tap Gaussian window of sigma 1.5,
C1 = 0.01^2, C2 = 0.03^2.  padding='same' zero-pads by 5 and counts every pixel (what 3DGS trains with); padding='valid' counts
only the pixels whose whole window lies inside the image (the original paper's form, for reported numbers).

Images are read where they are, as the renderer and the resident dataset hold them: pixel-major rows [H*W, 3 or 4] or
[H, W, 3 or 4], a patch view of a larger frame included; nothing is permuted or copied.  Written in torch the same number
costs some fifteen grouped 11x11 convolutions, their autograd twins and the permutes around them.  One call evaluates value,
optional map and the gradient towards `img`; the backward only scales the stored gradient (the pattern of recon_loss.py and
matting.py)."""
import math

import torch
from torch import nn

from . import _lib as L

TILE = 32           # SS_T of csrc/ssim.hip: the edge of the square tile a workgroup owns
WINDOW_SIZE = 11
SIGMA = 1.5


def window():
    """the eleven window weights as the kernel uses them: normalised to sum 1 in fp64, then rounded to f32 -> [11] float32"""
    g = [math.exp(-((i - WINDOW_SIZE // 2) ** 2) / (2.0 * SIGMA * SIGMA)) for i in range(WINDOW_SIZE)]
    s = math.fsum(g)
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(torch.float32)


def _geometry(name, t, H, W):
    """-> (tensor to read, H, W, stride in floats per pixel, pitch in pixels per image row).  The tensor is read in place
    when it is float32 with channels contiguous, 3 or 4 floats from pixel to pixel, whole pixels from row to row and the base
    aligned as the kernel asks; otherwise from one contiguous float32 copy."""
    if not torch.is_tensor(t):
        raise TypeError('ssim: {} must be a tensor'.format(name))
    if t.dim() == 3 and t.shape[0] == 3 and t.shape[2] not in (3, 4):
        raise ValueError('ssim: {} looks like [3,H,W] {}; images are pixel-major [H,W,3]: pass {}.permute(1, 2, 0)'.format(
            name, tuple(t.shape), name))
    if not t.is_cuda:
        raise RuntimeError('ssim: {} is a {} tensor; nerfstyle_amd kernels need HIP device tensors (there is no CPU '
                           'fallback)'.format(name, t.device))
    if t.dim() == 3:
        if (H is not None and int(H) != t.shape[0]) or (W is not None and int(W) != t.shape[1]):
            raise ValueError('ssim: {} is {}, not H = {}, W = {}'.format(name, tuple(t.shape), H, W))
        H, W = int(t.shape[0]), int(t.shape[1])
    elif t.dim() == 2:
        if H is None or W is None:
            raise ValueError('ssim: {} is rows {}; H and W must be given'.format(name, tuple(t.shape)))
        H, W = int(H), int(W)
        if H * W != t.shape[0]:
            raise ValueError('ssim: {} has {} rows, not H * W = {} * {}'.format(name, t.shape[0], H, W))
    else:
        raise ValueError('ssim: {} must be [H,W,C] or [H*W,C] with C in (3, 4); got {}'.format(name, tuple(t.shape)))
    C = int(t.shape[-1])
    if C not in (3, 4):
        raise ValueError('ssim: {} must have 3 or 4 floats a pixel; got {}'.format(name, tuple(t.shape)))
    if H < 1 or W < 1:
        raise ValueError('ssim: {} is empty: {}'.format(name, tuple(t.shape)))
    t = t.detach()
    if t.dtype == torch.float32 and t.stride(-1) == 1:
        s = t.stride(-2)
        if t.dim() == 2:
            row = W * s
        else:
            row = t.stride(0) if H > 1 else W * s
        if s in (3, 4) and s >= C and row % s == 0 and row // s >= W and t.data_ptr() % (16 if s == 4 else 4) == 0:
            return t, H, W, s, row // s
    t = t.to(torch.float32).contiguous()
    return t, H, W, C, W


class _ssim(torch.autograd.Function):
    """value [, map] and the stored gradient coef * scale * dSSIM/dimg.  dssim None: returns SSIM (coef 1).  dssim = lam * factor:
    returns the loss dssim * scale * (1 - SSIM) as float32, the stored gradient carrying coef = -dssim and the device scale."""

    @staticmethod
    def forward(ctx, img, target, H, W, valid, want_map, dssim, scale):
        ctx.set_materialize_grads(False)
        x, H, W, xs, xp = _geometry('img', img, H, W)
        y, H2, W2, ys, yp = _geometry('target', target, H, W)
        if (H2, W2) != (H, W):
            raise ValueError('ssim: img is {} x {}, target {} x {}'.format(H, W, H2, W2))
        if y.device != x.device:
            raise ValueError('ssim: img and target are on different devices')
        if valid and (H < WINDOW_SIZE or W < WINDOW_SIZE):
            raise ValueError("ssim: padding='valid' needs H, W >= {}; got {} x {}".format(WINDOW_SIZE, H, W))
        dev = x.device
        want_grad = ctx.needs_input_grad[0]
        out = torch.empty(4, dtype=torch.float64, device=dev)
        grad = torch.empty(H * W, 3, dtype=torch.float32, device=dev) if want_grad else None
        smap = torch.empty(H * W, 3, dtype=torch.float32, device=dev) if want_map else None
        ws = torch.empty(int(L.lib().nsr_ssim_workspace_bytes(H, W, 1 if want_grad else 0)) // 8, dtype=torch.float64, device=dev)
        if scale is not None and not (scale.dtype == torch.float32 and scale.numel() == 1 and scale.device == dev):
            raise ValueError('ssim: scale must be a 0-dim float32 tensor on the device of img')
        coef = 1.0 if dssim is None else -float(dssim)
        L.check(L.lib().nsr_ssim(x.data_ptr(), xs, xp, y.data_ptr(), ys, yp, H, W, 1 if valid else 0, coef, L.p(scale), L.p(out),
                                 L.p(smap), L.p(grad), L.p(ws), L.stream()), 'ssim')
        ctx.save_for_backward(grad)
        ctx.img_shape, ctx.img_dtype = tuple(img.shape), img.dtype
        ctx.terms = out
        if dssim is None:
            value = out[0]
        else:
            value = ((1.0 - out[0]) * float(dssim)).to(torch.float32)
            if scale is not None:
                value = value * scale.reshape(())
        if smap is None:
            return value
        smap = smap.view(H, W, 3)
        ctx.mark_non_differentiable(smap)
        return value, smap

    @staticmethod
    def backward(ctx, go, *_):
        (grad,) = ctx.saved_tensors
        if go is None or grad is None:
            return (None,) * 8
        # the stored gradient already carries coef * scale; `go` is 1 for value.backward()
        return (_as_img(grad * go.to(torch.float32), ctx.img_shape, ctx.img_dtype),) + (None,) * 7


def _as_img(grad, shape, dtype):
    """the kernel's [H*W,3] float32 gradient in the shape and dtype of img (a fourth float gets zero)"""
    g = grad.view(shape[:-1] + (3,))
    if shape[-1] == 4:
        g = torch.cat((g, torch.zeros_like(g[..., :1])), dim=-1)
    return g.to(dtype)


def _check(img, target, padding):
    if padding not in ('same', 'valid'):
        raise ValueError("ssim: padding must be 'same' or 'valid'; got {!r}".format(padding))
    if torch.is_tensor(target) and target.requires_grad:
        raise RuntimeError('ssim: no gradient with respect to `target`; pass target.detach()')
    return padding == 'valid'


def ssim(img, target, H=None, W=None, padding='same', return_map=False):
    """-> 0-dim float64 device tensor: the mean SSIM of img against target, differentiable with respect to img.
    img, target: [H,W,C] or [H*W,C] with H, W given; C in {3, 4} (a fourth float is never read), last dimension contiguous; a
    view with its own row pitch, frame.view(H,W,C)[y0:y1, x0:x1], is read in place.  return_map: (value, map [H,W,3] float32, 0
    where a pixel is not counted).  The per-channel means of the last call: channel_means(value)."""
    valid = _check(img, target, padding)
    return _ssim.apply(img, target, H, W, valid, bool(return_map), None, None)


def channel_means(value):
    """the three per-channel SSIM means behind a value returned by ssim / dssim_loss, as a device tensor [3] (no host sync)"""
    if hasattr(value, '_nsr_terms'):
        return value._nsr_terms[1:]
    fn = value[0].grad_fn if isinstance(value, tuple) else value.grad_fn
    return fn.terms[1:] if fn is not None and hasattr(fn, 'terms') else None


def dssim_loss(img, target, H=None, W=None, lam=0.2, factor=1.0, scale=None, padding='same', backward=False):
    """-> 0-dim float32 loss = factor * scale * lam * (1 - SSIM(img, target)), the D-SSIM term that stands beside the pixel loss.
    scale: 0-dim float32 device tensor (LossScaler.scale_tensor) or None; factor: a host float (1 / world size).
    backward=True: the gradient the kernel has just written, which already carries -lam * factor * scale, is pushed into img
    from here and the returned loss is detached, as recon_loss(..., backward=True) does."""
    valid = _check(img, target, padding)
    loss = _ssim.apply(img, target, H, W, valid, False, float(lam) * float(factor), scale)
    if not backward or loss.grad_fn is None:
        return loss
    fn = loss.grad_fn
    (grad,) = fn.saved_tensors
    if grad is not None and img.requires_grad:
        torch.autograd.backward([img], [_as_img(grad, tuple(img.shape), img.dtype)])
    det = loss.detach()
    det._nsr_terms = fn.terms
    return det


class DSSIM(nn.Module):
    """forward(img, target, H=None, W=None) -> lam * (1 - SSIM), see dssim_loss"""

    def __init__(self, lam: float = 0.2, padding: str = 'same') -> None:
        super().__init__()
        self.lam = lam
        self.padding = padding

    def forward(self, img, target, H=None, W=None, factor=1.0, scale=None, backward=False):
        return dssim_loss(img, target, H, W, lam=self.lam, factor=factor, scale=scale, padding=self.padding, backward=backward)


@torch.no_grad()
def frame_metrics(img, target, H=None, W=None):
    """-> device tensor [2] float64: PSNR = -10 ln(MSE) / ln(10) over the colour channels (the reference's compute_psnr,
    utils/__init__.py:323-325) and SSIM with padding='valid'.  No host read."""
    value = ssim(img, target, H, W, padding='valid')
    mse = torch.mean((img.detach()[..., :3].to(torch.float32) - target.detach()[..., :3].to(torch.float32)) ** 2)
    psnr = -10.0 * torch.log(mse) / math.log(10.0)
    return torch.stack((psnr.to(torch.float64), value))
