"""Generates tests/golden/matting_reference.npz: the reference's MattingLaplacian (loss.py:217-278) evaluated on seeded
inputs, value and gradient (run in the authoring container only; the reference does not travel).  The reference `loss`
module is imported exactly as make_goldens.py imports it.  The outputs are data only (inputs + expected outputs).

Per case <name>: <name>_target, <name>_v [3,H,W] f32 inputs (the near-flat case reuses r1_24x31's v), <name>_meta =
(win_rad, eps), <name>_value (float64 scalar), <name>_grad64 = d value / d v for a float64 style_map, <name>_grad32 the same
for a float32 style_map (the reference casts to float64 inside forward; autograd rounds the gradient back).

Usage: python tests/golden/make_matting_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import import_reference  # noqa: E402


def cases():
    rng = np.random.default_rng(2024)
    out = []

    def rand(h, w):
        return rng.random((3, h, w)).astype(np.float32)
    out.append(('r1_3x3', 1, rand(3, 3), rand(3, 3)))
    out.append(('r1_9x13', 1, rand(9, 13), rand(9, 13)))
    v24 = rand(24, 31)
    out.append(('r1_24x31', 1, rand(24, 31), v24))
    # near-flat target: Sigma is dominated by eps / k ~ 1.1e-8, its inverse reaches ~1e8 (why fp64 is needed)
    out.append(('r1_24x31_flat', 1, (0.5 + 1e-4 * rng.random((3, 24, 31))).astype(np.float32), v24))
    # flat target with one step edge: the windows across it have a rank-1 covariance + eps / k
    t = np.full((3, 9, 12), 0.25, np.float32)
    t[:, :, 5:] = np.array([0.75, 0.6, 0.9], np.float32)[:, None, None]
    out.append(('r1_9x12_edge', 1, t, rand(9, 12)))
    out.append(('r2_11x10', 2, rand(11, 10), rand(11, 10)))
    return out


def main():
    _, _, _, loss = import_reference()
    eps = 1e-7
    out = {}
    for name, r, target, v in cases():
        m = loss.MattingLaplacian(device=torch.device('cpu'), win_rad=r, eps=eps)
        grads = {}
        for dt in (torch.float64, torch.float32):
            sm = torch.tensor(v, dtype=dt, requires_grad=True)
            val = m(torch.tensor(target), sm)
            val.backward()
            grads[dt] = sm.grad.numpy()
            if dt == torch.float64:
                value = float(val.detach())
        out[name + '_target'] = target
        if name != 'r1_24x31_flat':
            out[name + '_v'] = v
        out[name + '_meta'] = np.array([r, eps], np.float64)
        out[name + '_value'] = np.float64(value)
        out[name + '_grad64'] = grads[torch.float64].astype(np.float64)
        out[name + '_grad32'] = grads[torch.float32].astype(np.float32)
        print('{:16s} r={} value {:.17g}'.format(name, r, value))
    path = os.path.join(HERE, 'matting_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
