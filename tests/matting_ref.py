"""Test-side restatements of the matting-Laplacian loss (the reference's MattingLaplacian, loss.py:217-278), written from the
definition of Levin et al., not from the reference code: for every (2r+1)^2 window inside the image, with D the window's
target pixels minus their mean and Sigma = D^T D / k + (eps / k) Id, the window's block of the Laplacian is
    Lw = Id_k - (1 + D Sigma^-1 D^T) / k
and the loss is sum over windows and channels of v_w^T Lw v_w.

matting_dense: that per-window dense form, in any float dtype (small images).
matting_fast:  the same sums vectorised over windows with numpy, fp64 (full frames)."""
import numpy as np


def matting_dense(target, v, r, eps, dtype=np.float64):
    """target, v [3,H,W] -> (value, d value / d v [3,H,W]), every operation in `dtype`."""
    t = np.asarray(target).astype(dtype)
    v = np.asarray(v).astype(dtype)
    _, H, W = t.shape
    d = 2 * r + 1
    k = d * d
    one, kk = dtype(1), dtype(k)
    value = dtype(0)
    grad = np.zeros_like(v)
    for y in range(r, H - r):
        for x in range(r, W - r):
            I = t[:, y - r:y + r + 1, x - r:x + r + 1].reshape(3, k).T            # [k,3]
            D = I - I.mean(0, dtype=dtype)
            S = (D.T @ D) / kk + dtype(eps) / kk * np.eye(3, dtype=dtype)
            Lw = np.eye(k, dtype=dtype) - (one + D @ np.linalg.inv(S).astype(dtype) @ D.T) / kk
            V = v[:, y - r:y + r + 1, x - r:x + r + 1].reshape(3, k)            # [3,k]
            LV = V @ Lw                                                        # Lw is symmetric
            value = value + (LV * V).sum(dtype=dtype)
            grad[:, y - r:y + r + 1, x - r:x + r + 1] += (dtype(2) * LV).reshape(3, d, d)
    return value, grad


def matting_fast(target, v, r, eps):
    """fp64, vectorised over windows: per window mu, Sigma, s0 = sum v, s2 = sum v^2, u = sum v (I - mu), a = Sigma^-1 u / k;
    value = sum s2 - s0^2 / k - u.a; gradient 2 sum_{w contains p} (v_p - s0/k - (I_p - mu).a)."""
    t = np.asarray(target, np.float64)
    v = np.asarray(v, np.float64)
    _, H, W = t.shape
    d = 2 * r + 1
    k = float(d * d)
    h, w = H - 2 * r, W - 2 * r
    shifts = [(dy, dx) for dy in range(d) for dx in range(d)]

    def win(a, dy, dx):
        return a[..., dy:dy + h, dx:dx + w]
    mu = sum(win(t, dy, dx) for dy, dx in shifts) / k                                   # [3,h,w]
    D = [win(t, dy, dx) - mu for dy, dx in shifts]
    S = sum(np.einsum('ihw,jhw->hwij', Di, Di) for Di in D) / k + eps / k * np.eye(3)   # [h,w,3,3]
    s0 = sum(win(v, dy, dx) for dy, dx in shifts)                                       # [3,h,w]
    s2 = sum(win(v, dy, dx) ** 2 for dy, dx in shifts)
    u = sum(np.einsum('chw,ihw->hwic', win(v, dy, dx), Di) for (dy, dx), Di in zip(shifts, D))   # [h,w,3(i),3(c)]
    a = np.linalg.solve(S, u) / k                                                       # [h,w,3(i),3(c)]
    value = float(s2.sum() - (s0 ** 2).sum() / k - np.einsum('hwic,hwic->', u, a))
    grad = np.zeros_like(v)
    for (dy, dx), Di in zip(shifts, D):
        grad[:, dy:dy + h, dx:dx + w] += 2.0 * (win(v, dy, dx) - s0 / k - np.einsum('ihw,hwic->chw', Di, a))
    return value, grad


def rel_err(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def fixture_cases(npz):
    """(name, win_rad, eps, target, v, value, grad64, grad32) of tests/golden/matting_reference.npz"""
    names = sorted({k[:-len('_meta')] for k in npz.files if k.endswith('_meta')})
    out = []
    for n in names:
        r, eps = npz[n + '_meta']
        v = npz[n + '_v'] if n + '_v' in npz.files else npz['r1_24x31_v']             # the near-flat case shares v
        out.append((n, int(r), float(eps), npz[n + '_target'], v, float(npz[n + '_value']), npz[n + '_grad64'],
                    npz[n + '_grad32']))
    return out
