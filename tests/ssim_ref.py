"""The definition of SSIM that nsr_ssim implements, restated for the tests (Wang et al. 2004 in the form 3DGS and pytorch-ssim
use): three channels, data range 1, C1 = 0.01^2, C2 = 0.03^2, an 11-tap Gaussian window of sigma 1.5 normalised in fp64 and
then rounded to f32, applied separably; no clamping of the variances; padding 'same' (zero padding of 5, every pixel counts) or
'valid' (only pixels whose whole window lies inside the image count).

ssim_ref    separable torch conv2d on the CPU with the f32-rounded window held in `dtype` (fp64: the ground truth; f32: what
            the same formulas give in the kernel's precision, the source of the tests' tolerances), gradient by autograd
ssim_loops  a second, independent evaluation for tiny images: plain loops over the 121 taps of the outer-product window, and
            the gradient from the closed form  dSSIM/dx(q) = [(G*A)(q) + 2 x(q) (G*B)(q) + y(q) (G*C)(q)] / count
plus the image kinds of the tests and the packing of an image into rows with a stride and a pitch."""
import numpy as np
import torch
import torch.nn.functional as F

R = 5
K = 2 * R + 1
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window64():
    """[11] float64 holding the f32-rounded weights"""
    i = np.arange(K, dtype=np.float64)
    g = np.exp(-(i - R) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def _blur(p, g, pad):
    """p [1,3,H,W] -> separable window sums, rows first then columns"""
    c = p.shape[1]
    p = F.conv2d(p, g.view(1, 1, 1, K).expand(c, 1, 1, K), padding=(0, pad), groups=c)
    return F.conv2d(p, g.view(1, 1, K, 1).expand(c, 1, K, 1), padding=(pad, 0), groups=c)


def ssim_ref(img, target, padding='same', dtype=torch.float64, want_grad=True):
    """img, target [H,W,3] arrays -> dict(value, channels [3], map [H,W,3] (0 where not counted), grad [H,W,3] = dSSIM/dimg),
    numpy arrays of `dtype`"""
    assert padding in ('same', 'valid')
    x = torch.tensor(np.asarray(img), dtype=dtype).permute(2, 0, 1)[None].contiguous().requires_grad_(want_grad)
    y = torch.tensor(np.asarray(target), dtype=dtype).permute(2, 0, 1)[None].contiguous()
    H, W = x.shape[2], x.shape[3]
    pad = R if padding == 'same' else 0
    assert pad or (H >= K and W >= K)
    g = torch.tensor(window64(), dtype=dtype)
    mx, my = _blur(x, g, pad), _blur(y, g, pad)
    sxx = _blur(x * x, g, pad) - mx * mx
    syy = _blur(y * y, g, pad) - my * my
    sxy = _blur(x * y, g, pad) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    value = m.mean()
    out = {'value': value.detach().numpy().copy(), 'channels': m.mean(dim=(0, 2, 3)).detach().numpy().copy()}
    full = torch.zeros(3, H, W, dtype=dtype)
    full[:, R - pad:H - (R - pad), R - pad:W - (R - pad)] = m.detach()[0]
    out['map'] = full.permute(1, 2, 0).contiguous().numpy()
    if want_grad:
        value.backward()
        out['grad'] = x.grad[0].permute(1, 2, 0).contiguous().numpy()
    return out


def ssim_loops(img, target, padding='same'):
    """the same numbers from plain fp64 loops over the 11x11 outer-product window -> dict as ssim_ref.  Tiny images only."""
    x, y = np.asarray(img, np.float64), np.asarray(target, np.float64)
    H, W = x.shape[:2]
    g = window64()
    w2 = np.outer(g, g)
    lo = 0 if padding == 'same' else R
    counted = np.zeros((H, W), bool)
    counted[lo:H - lo, lo:W - lo] = True
    count = 3 * int(counted.sum())

    def wsum(p, cy, cx):
        s = 0.0
        for i in range(K):
            for j in range(K):
                yy, xx = cy + i - R, cx + j - R
                if 0 <= yy < H and 0 <= xx < W:
                    s += w2[i, j] * p[yy, xx]
        return s

    m = np.zeros((H, W, 3))
    A, B, C = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for c in range(3):
        xc, yc = x[:, :, c], y[:, :, c]
        for py in range(H):
            for px in range(W):
                if not counted[py, px]:
                    continue
                mx, my = wsum(xc, py, px), wsum(yc, py, px)
                sxx = wsum(xc * xc, py, px) - mx * mx
                syy = wsum(yc * yc, py, px) - my * my
                sxy = wsum(xc * yc, py, px) - mx * my
                a1, a2 = 2 * mx * my + C1, 2 * sxy + C2
                b1, b2 = mx * mx + my * my + C1, sxx + syy + C2
                mm = a1 * a2 / (b1 * b2)
                m[py, px, c] = mm
                dmx = 2 * my * a2 / (b1 * b2) - mm * 2 * mx / b1
                dsxx = -mm / b2
                dsxy = 2 * a1 / (b1 * b2)
                A[py, px, c], B[py, px, c], C[py, px, c] = dmx - 2 * mx * dsxx - my * dsxy, dsxx, dsxy
    grad = np.zeros((H, W, 3))
    for c in range(3):
        for py in range(H):
            for px in range(W):
                grad[py, px, c] = (wsum(A[:, :, c], py, px) + 2 * x[py, px, c] * wsum(B[:, :, c], py, px)
                                   + y[py, px, c] * wsum(C[:, :, c], py, px)) / count
    return {'value': m.sum() / count, 'channels': m.sum(axis=(0, 1)) / (count // 3), 'map': m, 'grad': grad}


# ---- the image kinds of the tests ---------------------------------------------------------------------------------------

def pattern(H, W, seed):
    """a smooth pattern with an edge and noise, [H,W,3] float32 in [0, 1]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W] / 7.0
    t = np.stack([0.45 + 0.25 * np.sin(xx + c) * np.cos(yy * (0.5 * c + 1)) for c in range(3)], axis=-1)
    t = t + 0.05 * rng.random((H, W, 3))
    t[:, W // 3:] += 0.12
    return t.astype(np.float32)              # within [0.2, 0.87]: nothing is clipped, no flat saturated areas


NEAR_NOISE = 0.035      # uniform noise of this width on the pattern: SSIM about 0.98


def image_pairs(H, W, seed=0):
    """-> [(kind, img, target)]: pattern against a partly correlated one, a near-identical pair, a constant against the pattern"""
    rng = np.random.default_rng(1000 + seed)
    p = pattern(H, W, seed)
    partly = np.clip(0.6 * p[:, :, ::-1] + 0.4 * rng.random((H, W, 3)), 0.0, 1.0).astype(np.float32)
    near = (p + NEAR_NOISE * (rng.random((H, W, 3)) - 0.5)).astype(np.float32)
    const = np.full((H, W, 3), 0.4, np.float32)
    return [('partly', partly, p), ('near', near, p), ('constant', const, p)]


def pack(img, stride, pitch=None, rows_above=0, cols_left=0, fill=-7.0):
    """img [H,W,3] -> buffer [H + 2 rows_above, pitch, stride] float32 filled with `fill`, the image at (rows_above, cols_left)"""
    H, W = img.shape[:2]
    pitch = W if pitch is None else pitch
    buf = np.full((H + 2 * rows_above, pitch, stride), fill, np.float32)
    buf[rows_above:rows_above + H, cols_left:cols_left + W, :3] = img
    return buf


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
