"""Field forward and backward time with and without directions, alternating the two in ONE process, at the bench frame's
sample count (762 048 rays x 63.7 samples = 48.6 M samples; --samples for another count).

    python tools/bench_dirs.py [--samples N] [--rounds R]

Positions are uniform in the box, walked in nsr_sample_order's spatial order like a dense training batch (lattice forward,
gradients-out backward + table scatter), f16 tables, f16 MFMA.  Prints one JSON line: the median of R rounds in ms for
fwd / bwd x plain / dirs.  A microbenchmark of the field alone; `bench.py` measures the training step and stays direction-less.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=48_600_000)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig
    from nerfstyle_amd.style_nerf import StyleTCNerf
    dev = torch.device('cuda:0')
    M = a.samples
    g = torch.Generator(device=dev).manual_seed(1)
    pts = torch.rand(M, 3, device=dev, generator=g) * 4 - 2
    d = torch.randn(M, 3, device=dev, generator=g)
    dirs = d / d.norm(dim=1, keepdim=True)
    del d
    gs = torch.randn(M, device=dev, generator=g) * 1e-2
    gr = torch.randn(M, 8, device=dev, generator=g)
    models = {k: StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, None, view_dependent=(k == 'dirs')).to(dev)
              for k in ('plain', 'dirs')}
    perm = models['plain'].sample_order(pts)
    times = {k + '_' + w: [] for k in models for w in ('fwd', 'bwd')}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for rnd in range(a.rounds + 1):                     # round 0 warms up
        for k, m in models.items():                     # alternating: both see the same clocks and the same neighbours
            m._ensure_grad().zero_()
            ev[0].record()
            sig, rgb = m.field(pts, perm=perm, dirs=dirs if k == 'dirs' else None)
            ev[1].record()
            torch.autograd.backward([sig, rgb], [gs, gr])
            ev[2].record()
            torch.cuda.synchronize()
            if rnd:
                times[k + '_fwd'].append(ev[0].elapsed_time(ev[1]))
                times[k + '_bwd'].append(ev[1].elapsed_time(ev[2]))
            del sig, rgb
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({'samples': M, 'rounds': a.rounds, 'ms': {k: round(v, 3) for k, v in med.items()},
                      'all_ms': {k: [round(x, 3) for x in v] for k, v in times.items()}}))


if __name__ == '__main__':
    main()
