"""Reference for the lens refinement (NumPy / torch, CPU): the ray model of include/nsr.h ("Lens refinement") restated in fp64,
in fp32 in the kernel's operation order, and differentiably in torch; the closed-form gradients of
nsr_generate_rays_lens_backward towards the poses and the lens in fp64; and the recovery problem the CPU and the GPU tests share.

lens = (fx, fy, cx, cy, k1, k2);  x = (i - cx) / fx, y = (j - cy) / fy, r2 = x^2 + y^2, s = 1 + r2 (k1 + r2 k2),
c = (x s f0, y s f1, f2), v = R c, d = v / |v|, o = t."""
import numpy as np
import torch


def flip_signs(camera_flip):
    return [-1.0 if (camera_flip >> b) & 1 else 1.0 for b in (2, 1, 0)]


def pixel_centres(w, pix):
    pix = np.asarray(pix, np.int64)
    return (pix % w) + 0.5, (pix // w) + 0.5


def _frames(F, seg_frame, K):
    frame = np.repeat(np.asarray(seg_frame, np.int64), K)
    return frame, (frame >= 0) & (frame < F)


def rays(poses, w, lens, camera_flip, seg_frame, pix, K, dtype=np.float64):
    """-> (origins [N,3], unit directions [N,3]) in `dtype`; NaN rows for a segment naming no frame in [0, F).  With float32
    every operation is rounded to fp32 in the order of ru_write_ray_lens (no contraction): the fp32 restatement."""
    t = dtype
    poses, L = np.asarray(poses, t), np.asarray(lens, t)
    frame, ok = _frames(poses.shape[0], seg_frame, K)
    i, j = (a.astype(t) for a in pixel_centres(w, pix))
    f0, f1, f2 = (t(f) for f in flip_signs(camera_flip))
    x, y = (i - L[2]) / L[0], (j - L[3]) / L[1]
    r2 = x * x + y * y
    s = t(1) + r2 * (L[4] + r2 * L[5])
    c0, c1, c2 = (x * s) * f0, (y * s) * f1, np.full_like(x, f2)
    P = poses[np.where(ok, frame, 0)]
    v = [P[:, r, 0] * c0 + P[:, r, 1] * c1 + P[:, r, 2] * c2 for r in range(3)]
    nrm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    d = np.stack([v[0] / nrm, v[1] / nrm, v[2] / nrm], axis=1)
    o = P[:, :3, 3].copy()
    assert o.dtype == t and d.dtype == t
    o[~ok], d[~ok] = np.nan, np.nan
    return o, d


def rays_torch(poses, lens, w, camera_flip, seg_frame, pix, K):
    """the same rays, differentiable towards poses [F,3|4,4] and lens [6] (their dtype is the working precision); every segment
    must name a frame"""
    frame = torch.as_tensor(np.repeat(np.asarray(seg_frame, np.int64), K))
    i, j = (torch.as_tensor(a, dtype=lens.dtype) for a in pixel_centres(w, pix))
    f = flip_signs(camera_flip)
    x, y = (i - lens[2]) / lens[0], (j - lens[3]) / lens[1]
    r2 = x * x + y * y
    s = 1 + r2 * (lens[4] + r2 * lens[5])
    c = torch.stack((x * s * f[0], y * s * f[1], torch.full_like(x, f[2])), dim=1)
    P = poses[frame]
    v = (P[:, :3, :3] @ c[:, :, None])[:, :, 0]
    return P[:, :3, 3], v / v.norm(dim=1, keepdim=True)


def ray_terms(poses, w, lens, camera_flip, seg_frame, pix, K, g_o, g_d):
    """fp64 per-ray terms -> (pose terms [N,3,4], lens terms [N,6], frame [N], ok [N]): with h = (I - d d^T) g_d / |v|, the pose
    terms are h c^T and g_o; with q = R^T h, gX = q0 f0, gY = q1 f1, m = gX x + gY y, s' = k1 + 2 k2 r2, gx = gX s + 2 m s' x,
    gy = gY s + 2 m s' y the lens terms are (-gx x / fx, -gy y / fy, -gx / fx, -gy / fy, m r2, m r2^2).  Rows of segments that
    name no frame are zero."""
    poses, L = np.asarray(poses, np.float64), np.asarray(lens, np.float64)
    g_o, g_d = np.asarray(g_o, np.float64), np.asarray(g_d, np.float64)
    frame, ok = _frames(poses.shape[0], seg_frame, K)
    i, j = pixel_centres(w, pix)
    f0, f1, f2 = flip_signs(camera_flip)
    x, y = (i - L[2]) / L[0], (j - L[3]) / L[1]
    r2 = x * x + y * y
    s, ds = 1 + r2 * (L[4] + r2 * L[5]), L[4] + 2 * L[5] * r2
    c = np.stack((x * s * f0, y * s * f1, np.full_like(x, f2)), axis=1)
    R = poses[np.where(ok, frame, 0)][:, :3, :3]
    v = np.einsum('nrk,nk->nr', R, c)
    nv = np.linalg.norm(v, axis=1, keepdims=True)
    dn = v / nv
    h = (g_d - dn * (dn * g_d).sum(1, keepdims=True)) / nv
    pose_terms = np.concatenate((h[:, :, None] * c[:, None, :], g_o[:, :, None]), axis=2)
    q = np.einsum('nrk,nr->nk', R, h)
    gX, gY = q[:, 0] * f0, q[:, 1] * f1
    m = gX * x + gY * y
    gx, gy = gX * s + 2 * m * ds * x, gY * s + 2 * m * ds * y
    lens_terms = np.stack((-gx * x / L[0], -gy * y / L[1], -gx / L[0], -gy / L[1], m * r2, m * r2 * r2), axis=1)
    pose_terms[~ok], lens_terms[~ok] = 0.0, 0.0
    return pose_terms, lens_terms, frame, ok


def pose_gradient(poses, w, lens, camera_flip, seg_frame, pix, K, g_o, g_d):
    """fp64: (grad [F,3,4], sum |term| [F,3,4], rays per frame [F]), as frame_batch_ref.pose_gradient"""
    F = np.asarray(poses).shape[0]
    terms, _, frame, _ = ray_terms(poses, w, lens, camera_flip, seg_frame, pix, K, g_o, g_d)
    grad, mag, count = np.zeros((F, 3, 4)), np.zeros((F, 3, 4)), np.zeros(F, np.int64)
    for f in range(F):
        sel = frame == f
        grad[f], mag[f], count[f] = terms[sel].sum(0), np.abs(terms[sel]).sum(0), int(sel.sum())
    return grad, mag, count


def lens_gradient(poses, w, lens, camera_flip, seg_frame, pix, K, g_o, g_d):
    """fp64: (grad [6], sum |term| [6], number of rays whose segment names a frame)"""
    _, terms, _, ok = ray_terms(poses, w, lens, camera_flip, seg_frame, pix, K, g_o, g_d)
    return terms.sum(0), np.abs(terms).sum(0), int(ok.sum())


# ---- the recovery problem: a true lens found again from the directions alone ----------------------------------------------------
REC_W, REC_H = 24, 16
REC_CAM = (20.0, 21.0, 11.5, 8.25)
REC_SEG, REC_K, REC_FLIP = [2, 0, 2, 1, 2], 257, 0
# focal +3 %, centre (+0.7, -0.4) px, k = (-0.08, 0.02)
REC_TRUE = (REC_CAM[0] * 1.03, REC_CAM[1] * 1.03, REC_CAM[2] + 0.7, REC_CAM[3] - 0.4, -0.08, 0.02)
# torch Adam (betas 0.9 / 0.999), one group per parameter of LensRefiner.  Chosen on the CPU (fp64, rays_torch under autograd,
# tests/test_lens_cpu.py::test_recovery_on_the_restatement runs it): the loss sum |d - d*|^2 starts at REC_LOSS_START and is
# below 1 % of it for the first time after REC_STEPS steps, where it is REC_LOSS_CPU.
REC_RATES = {'log_focal': 2e-3, 'center': 5e-2, 'dist': 5e-3}
REC_STEPS = 37
REC_LOSS_START = 1.856717056
REC_LOSS_CPU = 1.455943470e-02


def recovery_problem(poses):
    """poses [>=3,3|4,4] -> (pix [5*257] int32, target directions [N,3] float32 of the true lens)"""
    rng = np.random.default_rng(2024)
    pix = rng.integers(0, REC_W * REC_H, len(REC_SEG) * REC_K).astype(np.int32)
    _, d = rays(np.asarray(poses, np.float64)[:3, :3, :], REC_W, REC_TRUE, REC_FLIP, REC_SEG, pix, REC_K)
    return pix, d.astype(np.float32)


def recovery_loop(refiner, directions, target, steps):
    """`steps` Adam steps on sum |directions(refiner()) - target|^2 from where the refiner stands -> the loss before every step
    and after the last one (steps + 1 floats)"""
    opt = torch.optim.Adam([{'params': [getattr(refiner, k)], 'lr': lr} for k, lr in REC_RATES.items()])
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = ((directions(refiner()) - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(((directions(refiner()) - target) ** 2).sum()))
    return losses
