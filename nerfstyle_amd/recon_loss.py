"""Reconstruction-stage loss of the reference's Trainer.calc_loss (trainers/base.py:251-304) as one fused HIP op:

    loss = MSE(rgb_map, target_rgb[pix]) + ce_lambda * CrossEntropy(classes, target_cls[pix])        (ce_lambda = 0.001, :281)

value and gradient in ONE pass over the rays (nsr_recon_loss), the target gather fused, optionally multiplied by the
device-side loss scale (optim.LossScaler) and a host factor (1 / world size).  The reference -- and rounds 1-2 of this build --
spend ~50 small torch kernels on it per step (slices, subtraction, square, mean, logsumexp, gather and their autograd
twins: 1.7 ms of a 37 ms full-frame step, a third of a 4 096-ray step).  Any other loss can still be written in torch on the
renderer's outputs; this op is the hot-path form of the reference's own loss."""
import torch

from . import _lib as L


def _prepare(rgb_map, classes, target_rgb, target_cls, pix, ce_lambda, ray_weight, ray_err_out):
    """what the forward of both Functions does before its launch -> (N, rgb_map, cls, nc, target_cls or None, g_rgb, g_cls, out):
    the inputs detached as contiguous float32, the gradient and loss-term buffers, the checks of targets, pix and weights"""
    N = rgb_map.shape[0]
    rgb_map = rgb_map.detach().to(torch.float32).contiguous()
    with_ce = classes is not None and classes.shape[1] > 0 and ce_lambda != 0.0
    cls = classes.detach().to(torch.float32).contiguous() if with_ce else None
    g_rgb = torch.empty_like(rgb_map)
    g_cls = torch.empty_like(cls) if with_ce else None
    out = torch.empty(3, dtype=torch.float32, device=rgb_map.device)
    assert target_rgb.dtype == torch.float32 and target_rgb.is_contiguous()
    if with_ce:
        assert target_cls.dtype == torch.int64 and target_cls.is_contiguous()
    if pix is not None:
        assert pix.dtype == torch.int64 and pix.is_contiguous() and pix.numel() == N
    else:
        assert target_rgb.shape[0] == N
    for t in (ray_weight, ray_err_out):
        assert t is None or (t.dtype == torch.float32 and t.numel() == N and not t.requires_grad), 'ray_weight / ray_err_out: [N] float32'
    return N, rgb_map, cls, cls.shape[1] if with_ce else 0, target_cls if with_ce else None, g_rgb, g_cls, out


class _recon_loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_map, classes, target_rgb, target_cls, pix, ce_lambda, factor, scale, ray_weight=None, ray_err_out=None):
        ctx.set_materialize_grads(False)
        N, rgb_map, cls, nc, target_cls, g_rgb, g_cls, out = _prepare(rgb_map, classes, target_rgb, target_cls, pix, ce_lambda, ray_weight,
                                                                      ray_err_out)
        ws = torch.empty(int(L.lib().nsr_recon_loss_workspace_bytes(N)) // 4, dtype=torch.float32, device=rgb_map.device)
        if ray_weight is None and ray_err_out is None:
            L.check(L.lib().nsr_recon_loss(L.p(rgb_map), L.p(cls), N, nc, L.p(target_rgb), L.p(target_cls), L.p(pix), float(ce_lambda),
                                           float(factor), L.p(scale), L.p(g_rgb), L.p(g_cls), L.p(out), L.p(ws), L.stream()), 'recon_loss')
        else:
            L.check(L.lib().nsr_recon_loss_weighted(L.p(rgb_map), L.p(cls), N, nc, L.p(target_rgb), L.p(target_cls), L.p(pix),
                                                    L.p(ray_weight), float(ce_lambda), float(factor), L.p(scale), L.p(g_rgb), L.p(g_cls),
                                                    L.p(ray_err_out), L.p(out), L.p(ws), L.stream()), 'recon_loss_weighted')
        ctx.save_for_backward(g_rgb, g_cls)
        ctx.terms = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        g_rgb, g_cls = ctx.saved_tensors
        if go is None:
            return (None,) * 10
        # the stored gradients already carry scale * factor; `go` is 1 for loss.backward()
        return (g_rgb * go, (g_cls * go if g_cls is not None else None)) + (None,) * 8


class _recon_loss_exposure(torch.autograd.Function):
    """_recon_loss on nsr_recon_loss_exposure: a gain per frame and channel, and the gradient towards it"""

    @staticmethod
    def forward(ctx, rgb_map, classes, exposure, target_rgb, target_cls, pix, ce_lambda, factor, scale, ray_weight, ray_err_out, seg_frame, K):
        ctx.set_materialize_grads(False)
        N, rgb_map, cls, nc, target_cls, g_rgb, g_cls, out = _prepare(rgb_map, classes, target_rgb, target_cls, pix, ce_lambda, ray_weight,
                                                                      ray_err_out)
        F, S = exposure.shape[0], seg_frame.numel()
        exposure = exposure.detach().contiguous()
        g_exp = torch.empty_like(exposure)
        ws = torch.empty(int(L.lib().nsr_recon_loss_exposure_workspace_bytes(N, F, S, K)) // 8, dtype=torch.float64, device=rgb_map.device)
        L.check(L.lib().nsr_recon_loss_exposure(L.p(rgb_map), L.p(cls), N, nc, L.p(target_rgb), L.p(target_cls), L.p(pix), L.p(ray_weight),
                                                L.p(exposure), F, L.p(seg_frame), S, K, float(ce_lambda), float(factor), L.p(scale),
                                                L.p(g_rgb), L.p(g_cls), L.p(g_exp), L.p(ray_err_out), L.p(out), L.p(ws), L.stream()),
                'recon_loss_exposure')
        ctx.save_for_backward(g_rgb, g_cls, g_exp)
        ctx.terms = out
        return out[0]

    @staticmethod
    def backward(ctx, go):
        g_rgb, g_cls, g_exp = ctx.saved_tensors
        if go is None:
            return (None,) * 13
        # the stored gradients already carry scale * factor; `go` is 1 for loss.backward()
        return (g_rgb * go, (g_cls * go if g_cls is not None else None), g_exp * go) + (None,) * 10


def _exposure_arguments(rgb_map, exposure, seg_frame, rays_per_segment):
    """the host-side checks of recon_loss(exposure=...) -> K"""
    if seg_frame is None:
        raise ValueError('seg_frame: exposure needs the frame of every segment (FrameBatch.seg_frame)')
    if rays_per_segment is None:
        raise ValueError('rays_per_segment: exposure needs the rays per segment (FrameBatch.K)')
    if not (torch.is_tensor(exposure) and exposure.dtype == torch.float32 and exposure.dim() == 2 and exposure.shape[1] == 3
            and exposure.shape[0] > 0):
        raise ValueError('exposure: [F,3] float32 log2 gains')
    if not (torch.is_tensor(seg_frame) and seg_frame.dtype == torch.int32 and seg_frame.dim() == 1 and seg_frame.is_contiguous()
            and not seg_frame.requires_grad):
        raise ValueError('seg_frame: [S] int32, contiguous')
    K = int(rays_per_segment)
    if K < 1 or K != rays_per_segment or seg_frame.numel() * K != rgb_map.shape[0]:
        raise ValueError('rays_per_segment: rgb_map has {} rays, not {} segments of {}'.format(rgb_map.shape[0], seg_frame.numel(),
                                                                                              rays_per_segment))
    for name, t in (('rgb_map', rgb_map), ('exposure', exposure), ('seg_frame', seg_frame)):
        if not t.is_cuda:
            raise NotImplementedError(name + ': on the CPU; the exposure loss has no CPU fallback')
    if exposure.device != rgb_map.device or seg_frame.device != rgb_map.device:
        raise ValueError('exposure / seg_frame: on another device than rgb_map')
    return K


def recon_loss(rgb_map, classes, target_rgb, target_cls=None, pix=None, ce_lambda=1e-3, factor=1.0, scale=None, backward=False,
               ray_weight=None, ray_err_out=None, exposure=None, seg_frame=None, rays_per_segment=None):
    """-> 0-dim loss tensor = factor * scale * (mse + ce_lambda * ce).  rgb_map [N,3], classes [N,nc] (or None) from
    Renderer.render(training=True); target_rgb [P,3] f32 / target_cls [P] int64 resident on the device, pix [N] int64 their rows
    (None: P == N, row n).  scale: 0-dim float32 device tensor (LossScaler.scale_tensor) or None.
    backward=True: the gradient the kernel has just written is back-propagated from here -- autograd.backward(outputs of the
    renderer, d loss / d outputs) -- and the returned loss is detached: `loss.backward()` on the plain form costs a ones-fill and
    one multiply per stored gradient (three launches, 1.5 % of a 4 096-ray captured step) to apply a factor that is 1.
    ray_weight [N] f32 (ErrorMap.draw's weights): every ray's terms, value and gradient, times its weight, the means still over
    N (nsr_recon_loss_weighted).  ray_err_out [N] f32: written with the ray's unweighted sum of squared colour differences, what
    ErrorMap.update takes.  Both are constants of differentiation; with both None the plain kernel runs.
    exposure [F,3] f32 (ExposureRefiner.forward()): log2 gains per frame and colour channel, with seg_frame [S] int32 and
    rays_per_segment = K of the mixed-frame batch (FrameBatch.seg_frame, .K; N == S * K).  Ray n is compared as
    rgb_map[n] * 2**exposure[seg_frame[n // K]] (nsr_recon_loss_exposure), ray_err_out becomes the exposure-corrected error, and
    d loss / d exposure, one deterministic fp64 sum per frame carrying scale * factor, reaches exposure.grad through autograd; with
    backward=True it is pushed together with the renderer's outputs.  ray_weight and ray_err_out stay optional.  With
    exposure None nothing of this runs."""
    if exposure is None:
        loss = _recon_loss.apply(rgb_map, classes, target_rgb, target_cls, pix, ce_lambda, factor, scale, ray_weight, ray_err_out)
        inputs = (rgb_map, classes)
    else:
        K = _exposure_arguments(rgb_map, exposure, seg_frame, rays_per_segment)
        loss = _recon_loss_exposure.apply(rgb_map, classes, exposure, target_rgb, target_cls, pix, ce_lambda, factor, scale, ray_weight,
                                          ray_err_out, seg_frame, K)
        inputs = (rgb_map, classes, exposure)
    if not backward or loss.grad_fn is None:
        return loss
    # the inputs that want a gradient with the one the kernel stored for them (none for classes without the cross-entropy term)
    pairs = [(t, g) for t, g in zip(inputs, loss.grad_fn.saved_tensors) if g is not None and t is not None and t.requires_grad]
    if pairs:
        torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    det = loss.detach()
    det._nsr_terms = loss.grad_fn.terms
    return det


def last_terms(loss):
    """(mse, ce_lambda * ce) of a loss returned by recon_loss, unscaled, as a device tensor [2] (no host sync)."""
    if hasattr(loss, '_nsr_terms'):
        return loss._nsr_terms[1:]
    fn = loss.grad_fn
    return fn.terms[1:] if fn is not None and hasattr(fn, 'terms') else None
