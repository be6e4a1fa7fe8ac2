"""What a mixed-frame batch costs: training steps (draw, render_frames, fused loss, backward) whose rays come from many frames,
against the same number of rays from one frame, with Renderer.pose_gradients on and off:

    python tools/bench_frames.py [--cap K] [--reps R] [--limit SECONDS]

4 096 rays as (S, K) = (1, 4096), (32, 128) and (4096, 1), and one full-frame-sized batch as (35, 21 772) = 762 020 rays
(1008x756 = 762 048 pixels; 35 segments of equal length fit 21 772 each), beside the same number of rays from one frame.  Every configuration runs in a process of its own
under a time limit of its own (--limit); the first one that fails or runs out of time ends the tool.  Per configuration: the wall
time of a step, the event times of the three mixed-frame kernels' calls, and the march, field and composite stages beside them --
mixing frames costs the march its ray coherence and the field kernels their shared table rows."""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cap', type=int, default=192)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--limit', type=int, default=150)
ap.add_argument('--child', nargs=3, metavar=('S', 'K', 'POSE_GRAD'), help='one configuration, in this process')
args = ap.parse_args()

F, W, H = 35, 1008, 756
CONFIGS = [(1, 4096), (32, 128), (4096, 1), (1, 35 * ((W * H) // 35)), (35, (W * H) // 35)]

if args.child is None:
    for S, K in CONFIGS:
        for on in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), '--cap', str(args.cap), '--reps', str(args.reps), '--child', str(S), str(K), str(on)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                sys.exit('S={} K={} pose_gradients={}: exit status {}; stopping'.format(S, K, on, rc))
    sys.exit(0)

import numpy as np
import torch
from nerfstyle_amd import profiling, raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.dataset import ResidentDataset
from nerfstyle_amd.pose import PoseRefiner
from nerfstyle_amd.recon_loss import recon_loss
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
from nerfstyle_amd.style_nerf import StyleTCNerf

S, K, on = int(args.child[0]), int(args.child[1]), bool(int(args.child[2]))
dev = torch.device('cuda:0')
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
with torch.no_grad():
    model.arena[:model.table_elems].uniform_(-0.5, 0.5)
poses, intr, _ = load_room_cameras(2)
assert intr.size() == (W, H)
poses = np.asarray(poses, np.float32)
poses = poses[np.arange(F) % len(poses)]
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=8, samples_per_ray_cap=args.cap).to(dev)
r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 28, 0), device=dev)
r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
r.update_occ = False
r.pose_gradients = on
# the targets' values do not matter to the time: grey frames
ds = ResidentDataset(np.full((F, 3, H, W), 0.5, np.float32), poses, intr, 2.0, dev)
refiner = PoseRefiner(torch.tensor(poses)).to(dev)
rows_rgb = ds.target_rgb_rows
seq = torch.zeros(1, dtype=torch.int32, device=dev)
LOSS_SCALE = 65536.0 if S * K > 100000 else 1.0       # a mean over 2.3 M entries underflows the f16 backward without it
batch = None


def step():
    global batch
    P = refiner.forward_all() if on else ds.poses[:, :3, :]
    batch = ds.draw(S, K, seed=7, sequence_dev=seq, advance=True, out=batch)
    out = r.render_frames(P, batch)
    recon_loss(out['rgb_map'], None, rows_rgb, pix=batch.rows, factor=LOSS_SCALE, backward=True)
    model.arena.grad.zero_()
    g = refiner.delta.grad
    refiner.delta.grad = None
    return g


step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    g = step()
torch.cuda.synchronize()
wall = (time.perf_counter() - t0) / args.reps * 1e3
profiling.reset()
profiling.enabled = True
step()
torch.cuda.synchronize()
profiling.enabled = False
print('S={:5d} K={:6d} ({:7d} rays, {} frames in the batch) pose_gradients={!s:5}  {:8.3f} ms/step  {} samples{}'.format(
    S, K, S * K, len(torch.unique(batch.seg_frame)), on, wall, int(r._last_counter[0]),
    '' if g is None else '  |delta.grad| {:.3e}'.format(float(g.norm()) / LOSS_SCALE)), flush=True)
for name, (n, _, avg) in sorted(profiling.summary().items()):
    print('    {:26s} {:8.3f} ms ({} launch{})'.format(name, avg, n, '' if n == 1 else 'es'), flush=True)
