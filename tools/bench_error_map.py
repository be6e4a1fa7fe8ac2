"""What error-map importance sampling adds to a training step, kernel by kernel (HIP events, no renderer):

    python tools/bench_error_map.py [--reps R] [--limit SECONDS]

the error draw (ErrorMap.draw, with and without frames_by_error) against the uniform draw (ResidentDataset.draw), the weighted
loss (with the per-ray error output) against the plain loss, and the map's accumulate and rebuild, at the two batch shapes of the
benchmarks: 4 096 rays as (S, K) = (64, 64) and one full frame of 762 048 rays (1008 x 756) -- drawn as one segment for the draw,
and for the loss and the accumulate the whole frame in rays.tile_order's 8 x 8 tiles, which puts the 64 lanes of a wave into one
16 x 16 cell (the shape the accumulate kernel's wave-level sum exists for).  35 frames, the default map (cell = 16: 3 024 cells
per frame).  Every shape runs in a process of its own under a time limit of its own (--limit); the first that fails or runs out
of time ends the tool.  Times are the median of --reps launches after a warm-up, in microseconds."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--limit', type=int, default=120)
ap.add_argument('--child', choices=('rays4096', 'frame'), help='one shape, in this process')
args = ap.parse_args()

F, W, H = 35, 1008, 756

if args.child is None:
    for shape in ('rays4096', 'frame'):
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
from nerfstyle_amd.common import Intrinsics
from nerfstyle_amd.dataset import ErrorMap, FrameBatch, ResidentDataset
from nerfstyle_amd.rays import tile_order
from nerfstyle_amd.recon_loss import recon_loss

dev = torch.device('cuda:0')
S, K = (64, 64) if args.child == 'rays4096' else (1, W * H)
N = S * K
# the targets' values do not matter to the time: grey frames, identity poses
ds = ResidentDataset(np.full((F, 3, H, W), 0.5, np.float32), np.tile(np.eye(4, dtype=np.float32), (F, 1, 1)),
                     Intrinsics(H, W, 800.0, 800.0, W / 2, H / 2), 2.0, dev)
em = ErrorMap(ds)
g = torch.Generator().manual_seed(1)
em.err.copy_((10.0 ** (-3.0 * torch.rand(em.err.shape, generator=g))).to(dev))        # three decades, like a half-converged scene
em.rebuild()
seq = torch.zeros(1, dtype=torch.int32, device=dev)
rows_rgb = ds.target_rgb_rows
rgb_map = torch.rand(N, 3, generator=g).to(dev)
err_buf = torch.empty(N, device=dev)


INNER = 10


def timed(fn):
    """microseconds per call: INNER calls captured as one graph (every call here is capture-safe), so that the events see the
    kernels and not the host preparing them; the median over --reps replays, divided by INNER"""
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


uniform = ds.draw(S, K, seed=7, sequence_dev=seq)
by_err = em.draw(S, K, seed=7, sequence_dev=seq)
res = [('draw, uniform (nsr_draw_frame_batch)', timed(lambda: ds.draw(S, K, seed=7, sequence_dev=seq, advance=True, out=uniform))),
       ('draw, error map', timed(lambda: em.draw(S, K, seed=7, sequence_dev=seq, advance=True, out=by_err))),
       ('draw, error map, frames_by_error', timed(lambda: em.draw(S, K, seed=7, sequence_dev=seq, advance=True, frames_by_error=True, out=by_err)))]
# loss, accumulate, rebuild: on the drawn batch (4 096 rays) or the frame in tile order
if args.child == 'frame':
    pix = tile_order(W, H, device=dev).to(torch.int32)
    batch = FrameBatch(torch.full((1,), 3, dtype=torch.int32, device=dev), pix, pix.long() + 3 * W * H, 1, N)
    weights = torch.ones(N, device=dev)
else:
    batch, weights = em.draw(S, K, seed=7)
with torch.no_grad():
    res += [('loss, plain (nsr_recon_loss)', timed(lambda: recon_loss(rgb_map, None, rows_rgb, pix=batch.rows))),
            ('loss, weighted + ray_err', timed(lambda: recon_loss(rgb_map, None, rows_rgb, pix=batch.rows, ray_weight=weights, ray_err_out=err_buf)))]
res += [('error map accumulate', timed(lambda: em.accumulate(batch, err_buf))),
        ('error map rebuild (2 launches)', timed(em.rebuild)),
        ('error map update (3 launches)', timed(lambda: em.update(batch, err_buf)))]
print('S={} K={} ({} rays), {} frames of {}x{}, {} cells per frame'.format(S, K, N, F, W, H, em.G), flush=True)
for name, us in res:
    print('    {:40s} {:9.1f} us'.format(name, us), flush=True)
added = res[1][1] - res[0][1] + res[4][1] - res[3][1] + res[7][1]
print('    added per step (draw + loss differences, update): {:.1f} us'.format(added), flush=True)
