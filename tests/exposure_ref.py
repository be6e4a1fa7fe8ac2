"""NumPy fp64 restatement of nsr_recon_loss_exposure (include/nsr.h): the weighted reconstruction loss with a log2 gain per frame
and colour channel, its gradients, and the error bounds the GPU test holds the kernel to.

    ray n: segment s = n // K, frame f = seg_frame[s];  gain = 2**exposure[f] if 0 <= f < F else 1;  p = rgb_map[n] * gain
    df = p - target[row];  mse = sum w df^2 / (3N);  gp = 2 df w s_ / (3N);  grad_rgb_map = gp * gain
    grad_exposure[f] = ln2 * sum over the frame's rays of gp * p;  ray_err[n] = sum_c df^2

Bounds (fp32 kernel against this fp64 restatement; eps = 2^-24 is one fp32 rounding).  The per-ray chain gain -> p -> df -> gp ->
gp * gain (or gp * p) makes about six roundings, the first of them in p, and p's error survives the cancellation in df: every
rounding is at most eps * (|p| + |t|) in df's units, so 2^-20 = 16 eps leaves headroom, and the fp64 per-frame sum adds nothing
visible:
    grad_rgb_map:   2^-20 * (2 w s_ / 3N) * gain * (|p| + |t|)                        elementwise
    grad_exposure:  2^-20 * ln2 * sum over the frame's rays of (2 w s_ / 3N) * |p| * (|p| + |t|)
    ray_err:        2^-22 * ray_err + 2^-22 * sum_c (|p| + |t|)^2"""
import numpy as np

LN2 = float(np.log(2.0))


def gains(exposure, seg_frame, K):
    """-> (gain [N,3] f64, frame [N] int64 with -1 for rays whose segment names no frame)"""
    e = np.asarray(exposure, np.float64)
    F = e.shape[0]
    f = np.repeat(np.asarray(seg_frame, np.int64), K)
    ok = (f >= 0) & (f < F)
    g = np.ones((f.size, 3))
    g[ok] = np.exp2(e[f[ok]])
    return g, np.where(ok, f, -1)


def loss(rgb_map, target_rgb, exposure, seg_frame, K, pix=None, ray_weight=None, classes=None, target_cls=None, ce_lambda=1e-3,
         s_=1.0):
    """every argument as the kernel takes it (s_ = scale * factor) -> dict of fp64 arrays:
    total (scaled), mse, ce (unscaled, ce times ce_lambda), grad_rgb_map [N,3], grad_classes [N,nc] or None, grad_exposure [F,3],
    ray_err [N], bound_rgb [N,3], bound_exposure [F,3], bound_err [N], frame [N]"""
    r = np.asarray(rgb_map, np.float64)
    N = r.shape[0]
    F = np.asarray(exposure).shape[0]
    rows = np.arange(N) if pix is None else np.asarray(pix, np.int64)
    t = np.asarray(target_rgb, np.float64)[rows]
    w = np.ones(N) if ray_weight is None else np.asarray(ray_weight, np.float64)
    gain, frame = gains(exposure, seg_frame, K)
    p = r * gain
    df = p - t
    k = (2.0 * w * s_ / (3.0 * N))[:, None]
    gp = k * df
    res = {'mse': float((w[:, None] * df * df).sum() / (3.0 * N)), 'ce': 0.0, 'grad_classes': None, 'frame': frame}
    res['grad_rgb_map'] = gp * gain
    res['ray_err'] = (df * df).sum(1)
    term = LN2 * gp * p
    mag = np.abs(p) + np.abs(t)
    tb = 2.0 ** -20 * LN2 * k * np.abs(p) * mag
    res['grad_exposure'] = np.zeros((F, 3))
    res['bound_exposure'] = np.zeros((F, 3))
    for f in range(F):
        res['grad_exposure'][f] = term[frame == f].sum(0)
        res['bound_exposure'][f] = tb[frame == f].sum(0)
    res['bound_rgb'] = 2.0 ** -20 * k * gain * mag
    res['bound_err'] = 2.0 ** -22 * res['ray_err'] + 2.0 ** -22 * (mag * mag).sum(1)
    if classes is not None and np.asarray(classes).shape[1] > 0 and ce_lambda != 0.0:
        lg = np.asarray(classes, np.float64)
        label = np.asarray(target_cls, np.int64)[rows]
        mx = lg.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(1))
        res['ce'] = float(ce_lambda * (w * (lse - lg[np.arange(N), label])).sum() / N)
        soft = np.exp(lg - lse[:, None])
        soft[np.arange(N), label] -= 1.0
        res['grad_classes'] = soft * (ce_lambda * w * s_ / N)[:, None]
    res['total'] = (res['mse'] + res['ce']) * s_
    return res


# ---- the recovery experiment of tests/test_gpu_exposure.py, with the gradient left to the caller ---------------------------------
REC_S, REC_K, REC_F = 64, 64, 8
REC_LR, REC_STEPS, REC_GAMMA = 0.1, 400, 0.985
# max |e - e_true| this loop ends with when the gradient is this file's loss() (tests/test_exposure_cpu.py runs it), and the bar
# of the GPU run: ten times that, and no tighter than 1e-4
REC_CPU_ERR = 2.148e-5
REC_BAR = max(10.0 * REC_CPU_ERR, 1e-4)


def recovery_inputs():
    """-> (rgb_map [4096,3] f32, target [4096,3] f32 = rgb_map * 2**e_true, seg_frame [64] i32, e_true [8,3] f64 in [-1, 1])"""
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0.05, 0.95, (REC_S * REC_K, 3)).astype(np.float32)
    e_true = rng.uniform(-1.0, 1.0, (REC_F, 3))
    seg = (np.arange(REC_S) % REC_F).astype(np.int32)
    target = (rgb.astype(np.float64) * np.exp2(e_true[np.repeat(seg, REC_K)])).astype(np.float32)
    return rgb, target, seg, e_true


def recover(e, grad_of):
    """torch Adam (lr REC_LR, times REC_GAMMA per step) on the [8,3] zero parameter e for REC_STEPS steps; grad_of() sets e.grad.
    -> e's final value as a NumPy array"""
    import torch
    opt = torch.optim.Adam([e], lr=REC_LR)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, REC_GAMMA)
    for _ in range(REC_STEPS):
        opt.zero_grad(set_to_none=True)
        grad_of()
        opt.step()
        sched.step()
    return e.detach().cpu().numpy()
