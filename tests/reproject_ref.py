"""NumPy fp64 restatement of the view reprojection (include/nsr.h, "View reprojection"), vectorised over the pixels of a pair,
and the analytic scene the CPU and GPU tests share.

Every step is written in the operation order the header states, with NumPy's correctly rounded fp64 +, -, *, /, sqrt and floor,
so the restatement runs the very sequence of IEEE operations csrc/reproject_core.h runs.  The scene is nevertheless chosen with
margins (margins(), asserted by the tests): no pixel sits within 1e-9 relative of a threshold that decides its outcome."""
import math

import numpy as np

VALID, NO_DST, BEHIND, OUT_OF_FRAME, NO_TAP, OCCLUDED = 0, 1, 2, 3, 4, 5
OUTCOMES = {VALID: 'valid', NO_DST: 'no surface at dst', BEHIND: 'behind the camera', OUT_OF_FRAME: 'out of frame',
            NO_TAP: 'no surface at a tap', OCCLUDED: 'occluded'}


def flip_signs(camera_flip):
    return (-1.0 if (camera_flip >> 2) & 1 else 1.0, -1.0 if (camera_flip >> 1) & 1 else 1.0, -1.0 if camera_flip & 1 else 1.0)


def has_surface(t):
    t = np.asarray(t)
    return np.isfinite(t) & (t > 0)


def _bilinear(v00, v01, v10, v11, ax, ay):
    top = v00 * (1.0 - ax) + v01 * ax
    bot = v10 * (1.0 - ax) + v11 * ax
    return top * (1.0 - ay) + bot * ay


def pixel_dirs(pose, intr, camera_flip):
    """step 2 for every pixel of a frame -> (v / |v| as three [H*W] arrays, origin), fp64"""
    fx, fy, cx, cy, W, H = intr
    fx, fy, cx, cy = (float(np.float32(x)) for x in (fx, fy, cx, cy))
    f0, f1, f2 = flip_signs(camera_flip)
    P = np.asarray(pose, np.float32).astype(np.float64)
    p = np.arange(H * W)
    py, px = p // W, p % W
    c0 = ((px.astype(np.float64) + 0.5 - cx) / fx) * f0
    c1 = ((py.astype(np.float64) + 0.5 - cy) / fy) * f1
    c2 = f2
    v = [P[r, 0] * c0 + P[r, 1] * c1 + P[r, 2] * c2 for r in range(3)]
    n = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [v[r] / n for r in range(3)], P[:, 3]


def reproject_pair(rgb, dist, poses, intr, a, b, camera_flip=0, depth_tol=0.01):
    """Pair (dst a, src b) -> dict: 'warped' [H*W,3] float32, 'warped64' (before the rounding), 'mask' [H*W] uint8, 'sse',
    'n_valid', 'abs_err' (the sum of |e| over the valid pixels and channels), 'outcome' [H*W] (the codes above) and
    'margin' {threshold: the smallest relative distance of a pixel that reaches the threshold from it}."""
    fx, fy, cx, cy, W, H = intr
    fx, fy, cx, cy = (float(np.float32(x)) for x in (fx, fy, cx, cy))
    f0, f1, f2 = flip_signs(camera_flip)
    HW = H * W
    rgb = np.asarray(rgb, np.float32).reshape(-1, HW, 3)
    dist = np.asarray(dist, np.float32).reshape(-1, HW)
    poses = np.asarray(poses, np.float32)
    Pb = poses[b].astype(np.float64)
    outcome = np.full(HW, -1, np.int64)
    with np.errstate(all='ignore'):
        # 1
        ta = dist[a]
        s1 = has_surface(ta)
        outcome[~s1] = NO_DST
        t = np.where(s1, ta, 1.0).astype(np.float64)
        # 2
        d, oa = pixel_dirs(poses[a], intr, camera_flip)
        X = [oa[r] + t * d[r] for r in range(3)]
        # 3
        dx = [X[r] - Pb[r, 3] for r in range(3)]
        q = [Pb[0, k] * dx[0] + Pb[1, k] * dx[1] + Pb[2, k] * dx[2] for k in range(3)]
        z = q[2] * f2
        r = np.sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])
        s3 = s1 & (z > 0.0)
        outcome[s1 & ~s3] = BEHIND
        # 4
        zs = np.where(s3, z, 1.0)
        u = fx * (q[0] * f0 / zs) + cx - 0.5
        w = fy * (q[1] * f1 / zs) + cy - 0.5
        inside = (u >= 0.0) & (u <= W - 1.0) & (w >= 0.0) & (w <= H - 1.0)
        s4 = s3 & inside
        outcome[s3 & ~s4] = OUT_OF_FRAME
        xf = np.where(s4, np.minimum(np.floor(u), W - 2.0), 0.0)
        yf = np.where(s4, np.minimum(np.floor(w), H - 2.0), 0.0)
        ax, ay = u - xf, w - yf
        i00 = yf.astype(np.int64) * W + xf.astype(np.int64)
        taps = (i00, i00 + 1, i00 + W, i00 + W + 1)
        # 5
        tt = [dist[b][i] for i in taps]
        s5a = s4 & has_surface(tt[0]) & has_surface(tt[1]) & has_surface(tt[2]) & has_surface(tt[3])
        outcome[s4 & ~s5a] = NO_TAP
        tt = [np.where(s5a, x, 1.0).astype(np.float64) for x in tt]
        tbar = _bilinear(tt[0], tt[1], tt[2], tt[3], ax, ay)
        gap = np.abs(r - tbar)
        valid = s5a & (gap <= depth_tol * r)
        outcome[s5a & ~valid] = OCCLUDED
        outcome[valid] = VALID
        # 6
        w64 = np.zeros((HW, 3))
        for k in range(3):
            ch = rgb[b][:, k].astype(np.float64)
            w64[:, k] = np.where(valid, _bilinear(ch[taps[0]], ch[taps[1]], ch[taps[2]], ch[taps[3]], ax, ay), 0.0)
        # 7
        e = w64[valid] - rgb[a][valid].astype(np.float64)
        terms = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        margin = {
            'z': float(np.min(np.abs(z[s1]) / r[s1])) if s1.any() else np.inf,
            'frame': float(min(np.min(np.abs(u[s3])), np.min(np.abs(u[s3] - (W - 1.0))), np.min(np.abs(w[s3])),
                               np.min(np.abs(w[s3] - (H - 1.0)))) / max(W - 1.0, H - 1.0)) if s3.any() else np.inf,
            'depth': float(np.min(np.abs(gap[s5a] - depth_tol * r[s5a]) / r[s5a])) if s5a.any() else np.inf,
        }
    assert (outcome >= 0).all()
    return {'warped': w64.astype(np.float32), 'warped64': w64, 'mask': valid.astype(np.uint8), 'sse': math.fsum(terms.tolist()),
            'n_valid': int(valid.sum()), 'abs_err': math.fsum(np.abs(e).ravel().tolist()), 'outcome': outcome, 'margin': margin}


def reproject_frames(rgb, dist, poses, intr, pairs, camera_flip=0, depth_tol=0.01):
    """-> (warped [P,H*W,3] float32, mask [P,H*W] uint8, stats [P,2] float64, the per-pair dicts)"""
    res = [reproject_pair(rgb, dist, poses, intr, a, b, camera_flip, depth_tol) for a, b in pairs]
    return (np.stack([r['warped'] for r in res]), np.stack([r['mask'] for r in res]),
            np.asarray([[r['sse'], r['n_valid']] for r in res], np.float64), res)


def warp_error(stats, H, W):
    stats = np.asarray(stats, np.float64)
    with np.errstate(all='ignore'):
        return np.stack((np.sqrt(stats[:, 0] / (3.0 * stats[:, 1])), stats[:, 1] / float(H * W)), axis=1)


# ---- the error bound of sse ------------------------------------------------------------------------------------------------
def sse_tolerance(res, intr):
    """The absolute bound on |sse - res['sse']| for an implementation of the header's steps in fp64 with its own summation order.
      * summation: any order of n = 3 H W non-negative fp64 terms is within n 2^-52 relative of the exact sum (the issue's bound);
      * the squared-rounding term: the implementation's warped value (before its f32 rounding) may differ from the restatement's
        by delta.  The index coordinates u, w come out of a chain of fewer than 64 rounded fp64 operations on quantities bounded
        by max(W, H) in pixel units, so they differ by at most 64 * 2^-53 * max(W, H); a bilinear mean of taps in [0, 1] moves
        by at most that per axis, and its own five roundings add 8 * 2^-53:  delta = (128 max(W, H) + 8) 2^-53.  A term
        e^2 then moves by at most 2 |e| delta + delta^2, summed:  2 delta * sum|e| + 3 n_valid delta^2."""
    W, H = intr[4], intr[5]
    delta = (128.0 * max(W, H) + 8.0) * 2.0 ** -53
    return 3.0 * H * W * 2.0 ** -52 * res['sse'] + 2.0 * delta * res['abs_err'] + 3.0 * res['n_valid'] * delta * delta


# ---- the scene -------------------------------------------------------------------------------------------------------------
CAMERA_FLIP = 3              # x right, y up, looking along -z of the camera (the flip the LLFF scenes of the project use)
SPHERE_C, SPHERE_R = np.array([0.15, -0.1, 1.4]), 0.55


def _rot(rx, ry, rz):
    cx_, sx = math.cos(rx), math.sin(rx)
    cy_, sy = math.cos(ry), math.sin(ry)
    cz, sz = math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def scene_poses():
    """four cameras on a small baseline above the plane z = 0, looking down at it, and a fifth turned away from it"""
    cams = [((0.00, 0.00, 4.0), (0.00, 0.00, 0.00)), ((0.35, 0.05, 4.1), (0.01, 0.06, 0.02)), ((-0.30, 0.20, 3.9), (-0.04, -0.05, -0.03)),
            ((0.10, -0.35, 4.0), (0.07, 0.02, 0.01)), ((0.05, 0.05, 4.0), (math.pi, 0.0, 0.0))]
    poses = np.zeros((len(cams), 3, 4), np.float32)
    for i, (o, ang) in enumerate(cams):
        poses[i, :, :3] = _rot(*ang)
        poses[i, :, 3] = o
    return poses


def scene_colour(X):
    """a smooth colour of the world point -> [..., 3] in [0.1, 0.9]"""
    x, y, z = X
    return np.stack((0.5 + 0.4 * np.sin(1.3 * x + 0.7 * y + 0.2), 0.5 + 0.4 * np.sin(0.9 * y - 1.1 * x + 0.5 * z + 1.0),
                     0.5 + 0.4 * np.cos(0.8 * x + 1.2 * y - 0.6 * z)), axis=-1)


def make_scene(W=37, H=23, holes=True):
    """A textured plane (z = 0) with a sphere in front of it, seen by scene_poses(): exact ray intersections in fp64, rounded to
    float32.  holes: the outer ring of every frame and two columns of frame 1 have no surface (0), one pixel of frame 0 is NaN
    and one is -1.  -> dict(rgb [F,H*W,3], dist [F,H*W], poses [F,3,4], intr (fx, fy, cx, cy, W, H), camera_flip)"""
    s = W / 37.0
    intr = (float(np.float32(31.0 * s)), float(np.float32(33.0 * s)), float(np.float32(18.2 * s)), float(np.float32(11.9 * s)), W, H)
    poses = scene_poses()
    F, HW = poses.shape[0], H * W
    rgb = np.zeros((F, HW, 3), np.float32)
    dist = np.zeros((F, HW), np.float32)
    for f in range(F):
        d, o = pixel_dirs(poses[f], intr, CAMERA_FLIP)
        with np.errstate(all='ignore'):
            tp = np.where(d[2] < 0.0, -o[2] / d[2], np.inf)                       # the plane
            oc = [o[r] - SPHERE_C[r] for r in range(3)]
            bq = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]
            disc = bq * bq - (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - SPHERE_R * SPHERE_R)
            ts = np.where(disc > 0.0, -bq - np.sqrt(np.where(disc > 0.0, disc, 0.0)), np.inf)
            ts = np.where(ts > 0.0, ts, np.inf)
        t = np.minimum(tp, ts)
        hit = np.isfinite(t)
        tt = np.where(hit, t, 0.0)
        rgb[f] = np.where(hit[:, None], scene_colour([o[r] + tt * d[r] for r in range(3)]), 1.0).astype(np.float32)
        dist[f] = tt.astype(np.float32)
    if holes:
        g = dist.reshape(F, H, W)
        g[:, 0, :] = 0.0; g[:, -1, :] = 0.0; g[:, :, 0] = 0.0; g[:, :, -1] = 0.0
        g[1, :, (5 * W) // 8:(5 * W) // 8 + 2] = 0.0
        g[0, H // 3, W // 4] = np.nan
        g[0, (2 * H) // 3, (2 * W) // 3] = -1.0
    return {'rgb': rgb, 'dist': dist, 'poses': poses, 'intr': intr, 'camera_flip': CAMERA_FLIP}


# the pairs of the GPU test: an (a, a) pair, a repeated pair and the camera that faces away, as dst and as src
SCENE_PAIRS = [(0, 1), (2, 2), (0, 1), (4, 0), (3, 4)]
# the pairs whose outcomes together must cover every code (the CPU test adds the rest of the baseline)
ALL_PAIRS = SCENE_PAIRS + [(1, 0), (1, 2), (2, 3), (3, 0)]
