"""What per-frame exposure adds to the loss of a training step (HIP events, no renderer):

    python tools/bench_exposure.py [--reps R] [--limit SECONDS]

nsr_recon_loss_exposure (four launches: loss, final pass, per-segment sums, per-frame sums) against nsr_recon_loss_weighted (two
launches, the same kernel as before the feature) in the same process, both with weights and the per-ray error output, at the
batch shapes of the benchmarks: 4 096 rays as (S, K) = (64, 64), and one full frame's worth of 762 048 rays (1008 x 756) as one
segment (1, 762048) and as 36 segments (36, 21168).  35 frames.  Every shape runs in a process of its own under a time limit of
its own (--limit); the first that fails or runs out of time ends the tool.  Times are microseconds per call: ten calls captured as
one graph, the median of --reps replays after a warm-up."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'rays4096': (64, 64), 'frame1': (1, 762048), 'frame36': (36, 21168)}
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--limit', type=int, default=120)
ap.add_argument('--child', choices=tuple(SHAPES), help='one shape, in this process')
args = ap.parse_args()

F = 35

if args.child is None:
    for shape in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--child', shape]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.exit('{}: exit status {}; stopping'.format(shape, rc))
    sys.exit(0)

import numpy as np
import torch
from nerfstyle_amd.recon_loss import recon_loss

dev = torch.device('cuda:0')
S, K = SHAPES[args.child]
N = S * K
g = torch.Generator().manual_seed(1)
rgb_map = torch.rand(N, 3, generator=g).to(dev)
target = torch.rand(N, 3, generator=g).to(dev)
rows = torch.randperm(N, generator=g).to(dev)
weights = (0.25 + 3.75 * torch.rand(N, generator=g)).to(dev)
exposure = (torch.rand(F, 3, generator=g) * 2.0 - 1.0).to(dev)
seg_frame = torch.randint(0, F, (S,), generator=g).to(torch.int32).to(dev)
err_buf = torch.empty(N, device=dev)

INNER = 10


def timed(fn):
    """microseconds per call: INNER calls captured as one graph (both calls are capture-safe), so that the events see the kernels
    and not the host preparing them; the median over --reps replays, divided by INNER"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(INNER):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / INNER)
    return float(np.median(times))


with torch.no_grad():
    res = [('loss, weighted + ray_err (nsr_recon_loss_weighted)',
            timed(lambda: recon_loss(rgb_map, None, target, pix=rows, ray_weight=weights, ray_err_out=err_buf))),
           ('loss, exposure + weights + ray_err (nsr_recon_loss_exposure)',
            timed(lambda: recon_loss(rgb_map, None, target, pix=rows, ray_weight=weights, ray_err_out=err_buf, exposure=exposure,
                                     seg_frame=seg_frame, rays_per_segment=K)))]
print('S={} K={} ({} rays), {} frames'.format(S, K, N, F), flush=True)
for name, us in res:
    print('    {:62s} {:9.1f} us'.format(name, us), flush=True)
print('    added per step: {:.1f} us'.format(res[1][1] - res[0][1]), flush=True)
