"""What lens refinement costs (HIP events for the kernels, wall clock for a step):

    python tools/bench_lens.py [--cap K] [--reps R] [--limit SECONDS]

Kernels: nsr_generate_rays_lens against nsr_generate_rays_frames, and nsr_generate_rays_lens_backward (pose rows and lens row)
against nsr_generate_rays_frames_backward -- the kernels from before the feature, unchanged -- at the (S, K) rows of
tools/bench_frames.py, 1008x756, 35 frames, in one process, alternating.  Times are microseconds per call: ten calls captured as
one graph, the median of --reps replays after a warm-up.
Step: the wall clock of a 4 096-ray training step as (S, K) = (32, 128) (draw, render_frames, fused loss, backward; the mean of
--reps eager steps) with pose refinement alone and with lens and pose refinement, a process each.
Every child runs under a time limit of its own (--limit); the first that fails or runs out of time ends the tool."""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--cap', type=int, default=192)
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--limit', type=int, default=150)
ap.add_argument('--child', choices=('kernels', 'step-pose', 'step-lens'), help='one part, in this process')
args = ap.parse_args()

F, W, H = 35, 1008, 756
CONFIGS = [(1, 4096), (32, 128), (4096, 1), (1, 35 * ((W * H) // 35)), (35, (W * H) // 35)]

if args.child is None:
    for part in ('kernels', 'step-pose', 'step-lens'):
        cmd = [sys.executable, os.path.abspath(__file__), '--cap', str(args.cap), '--reps', str(args.reps), '--child', part]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.exit('{}: exit status {}; stopping'.format(part, rc))
    sys.exit(0)

import numpy as np
import torch
from nerfstyle_amd import _lib as L
from nerfstyle_amd.scene import load_room_cameras

dev = torch.device('cuda:0')
poses, intr, _ = load_room_cameras(2)
assert intr.size() == (W, H)
poses = np.asarray(poses, np.float32)
poses = poses[np.arange(F) % len(poses)]
CAM = (float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy))
FLIP = 3

if args.child == 'kernels':
    INNER = 10
    P = torch.tensor(poses[:, :3, :], device=dev).contiguous()
    lens = torch.tensor(CAM + (-0.08, 0.02), dtype=torch.float32, device=dev)
    lib = L.lib()

    def graph_of(fn):
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
        return graph

    def alternating(graphs):
        """microseconds per call of every graph: one replay of each in turn, --reps rounds, the median per graph"""
        times = [[] for _ in graphs]
        for _ in range(args.reps):
            for k, graph in enumerate(graphs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graph.replay()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3 / INNER)
        return [float(np.median(t)) for t in times]

    print('us per call, {} frames, {}x{}; frames = the kernels from before the feature'.format(F, W, H), flush=True)
    print('    {:>8s} {:>8s} | {:>10s} {:>10s} | {:>10s} {:>10s} {:>12s}'.format('S', 'K', 'frames fwd', 'lens fwd', 'frames bwd', 'lens bwd',
                                                                         'lens bwd,-P'), flush=True)
    for S, K in CONFIGS:
        N = S * K
        g = torch.Generator().manual_seed(S)
        seg = torch.randint(0, F, (S,), generator=g).to(torch.int32).to(dev)
        pix = torch.randint(0, W * H, (N,), generator=g).to(torch.int32).to(dev)
        g_o, g_d = torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev)
        ro, rd = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
        ws = torch.empty(int(lib.nsr_generate_rays_lens_backward_workspace_bytes(F, S, K)) // 8, dtype=torch.float64, device=dev)
        gp, gl = torch.empty(F, 3, 4, device=dev), torch.empty(6, device=dev)
        head = (L.p(seg), L.p(pix), S, K)

        def frames_fwd():
            L.check(lib.nsr_generate_rays_frames(L.p(P), F, W, H, *CAM, FLIP, *head, L.p(ro), L.p(rd), L.stream()))

        def lens_fwd():
            L.check(lib.nsr_generate_rays_lens(L.p(P), F, W, H, L.p(lens), FLIP, *head, L.p(ro), L.p(rd), L.stream()))

        def frames_bwd():
            L.check(lib.nsr_generate_rays_frames_backward(L.p(P), F, W, H, *CAM, FLIP, *head, L.p(g_o), L.p(g_d), L.p(ws), L.p(gp), L.stream()))

        def lens_bwd(with_poses=True):
            L.check(lib.nsr_generate_rays_lens_backward(L.p(P), F, W, H, L.p(lens), FLIP, *head, L.p(g_o), L.p(g_d), L.p(ws),
                                                        L.p(gp) if with_poses else None, L.p(gl), L.stream()))
        t = alternating([graph_of(f) for f in (frames_fwd, lens_fwd, frames_bwd, lens_bwd, lambda: lens_bwd(False))])
        print('    {:8d} {:8d} | {:10.1f} {:10.1f} | {:10.1f} {:10.1f} {:12.1f}'.format(S, K, *t), flush=True)
    sys.exit(0)

from nerfstyle_amd import profiling, raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.dataset import ResidentDataset
from nerfstyle_amd.lens import LensRefiner
from nerfstyle_amd.pose import PoseRefiner
from nerfstyle_amd.recon_loss import recon_loss
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import synthetic_density_grid
from nerfstyle_amd.style_nerf import StyleTCNerf

S, K, with_lens = 32, 128, args.child == 'step-lens'
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
with torch.no_grad():
    model.arena[:model.table_elems].uniform_(-0.5, 0.5)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=8, samples_per_ray_cap=args.cap).to(dev)
r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 28, 0), device=dev)
r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
r.update_occ = False
r.pose_gradients = True
ds = ResidentDataset(np.full((F, 3, H, W), 0.5, np.float32), poses, intr, 2.0, dev)       # grey frames: the values do not matter
refiner, lens_refiner = PoseRefiner(torch.tensor(poses)).to(dev), LensRefiner(intr).to(dev)
seq = torch.zeros(1, dtype=torch.int32, device=dev)
batch = None


def step():
    global batch
    batch = ds.draw(S, K, seed=7, sequence_dev=seq, advance=True, out=batch)
    out = r.render_frames(refiner.forward_all(), batch, lens=lens_refiner() if with_lens else None)
    recon_loss(out['rgb_map'], None, ds.target_rgb_rows, pix=batch.rows, backward=True)
    model.arena.grad.zero_()
    grads = [refiner.delta.grad] + [p.grad for p in lens_refiner.parameters()]
    for p in [refiner.delta] + list(lens_refiner.parameters()):
        p.grad = None
    return grads


step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    grads = step()
torch.cuda.synchronize()
wall = (time.perf_counter() - t0) / args.reps * 1e3
profiling.reset()
profiling.enabled = True
step()
torch.cuda.synchronize()
profiling.enabled = False
print('S={} K={} ({} rays) pose refinement{}: {:.3f} ms/step, {} samples, |grad| {}'.format(
    S, K, S * K, ' + lens refinement' if with_lens else ' alone', wall, int(r._last_counter[0]),
    ' '.join('-' if g is None else '{:.3e}'.format(float(g.norm())) for g in grads)), flush=True)
for name, (n, _, avg) in sorted(profiling.summary().items()):
    if name.startswith('generate_rays'):
        print('    {:26s} {:8.3f} ms ({} launch{})'.format(name, avg, n, '' if n == 1 else 'es'), flush=True)
