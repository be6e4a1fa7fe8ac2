"""Reference for the mixed-frame batches (NumPy, CPU): Philox4x32-10 and the draw of nsr_draw_frame_batch restated, and the
fp64 per-frame pose gradient of nsr_generate_rays_frames_backward from the closed form of include/nsr.h."""
import numpy as np

from pose_ref import camera_dirs

M32 = np.uint64(0xffffffff)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays (or scalars) of 32-bit values -> four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(a, dtype=np.uint64)) & M32 for a in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def umulhi(a, b):
    return (np.asarray(a, np.uint64) * np.uint64(b)) >> np.uint64(32)


def draw(F, P, S, K, seed, seq, stream_id=0, fixed_frames=None):
    """-> (seg_frame [S] int32, pix [S*K] int32, rows [S*K] int64) of nsr_draw_frame_batch at the summed sequence `seq`"""
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    seq &= 0xffffffff
    if fixed_frames is None:
        seg = umulhi(philox(np.arange(S), seq, 2, stream_id, k0, k1)[0], F).astype(np.int64)
    else:
        seg = np.asarray(fixed_frames, np.int64)
    pix = umulhi(philox(np.arange(S * K), seq, 3, stream_id, k0, k1)[0], P).astype(np.int64)
    return seg.astype(np.int32), pix.astype(np.int32), np.repeat(seg, K) * P + pix


def pose_gradient(poses, w, fx, fy, cx, cy, camera_flip, seg_frame, pix, K, g_o, g_d):
    """fp64: (grad [F,3,4], sum |term| [F,3,4], rays per frame [F]) -- per ray, with c the camera-frame direction, v = R c and
    d = v / |v|, the term ((I - d d^T) g_d / |v|) c^T for the rotation and g_o for the translation, summed over the rays of the
    segments that name the frame; segments naming no frame in [0, F) count nowhere"""
    import torch
    F = poses.shape[0]
    frame = np.repeat(np.asarray(seg_frame, np.int64), K)
    cd = camera_dirs(w, fx, fy, cx, cy, camera_flip, pix, torch.float64).numpy()
    grad, mag, count = np.zeros((F, 3, 4)), np.zeros((F, 3, 4)), np.zeros(F, np.int64)
    for f in range(F):
        sel = frame == f
        if not sel.any():
            continue
        c, gd = cd[sel], np.asarray(g_d, np.float64)[sel]
        v = c @ np.asarray(poses[f], np.float64)[:3, :3].T
        nv = np.linalg.norm(v, axis=1, keepdims=True)
        dn = v / nv
        h = (gd - dn * (dn * gd).sum(1, keepdims=True)) / nv
        terms = np.concatenate((h[:, :, None] * c[:, None, :], np.asarray(g_o, np.float64)[sel][:, :, None]), axis=2)      # [n,3,4]
        grad[f], mag[f], count[f] = terms.sum(0), np.abs(terms).sum(0), int(sel.sum())
    return grad, mag, count
