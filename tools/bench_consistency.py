"""The fused view reprojection against the same result composed from torch ops, on one device in one process (HIP events):

    python tools/bench_consistency.py [--reps R] [--h 756 --w 1008] [--frames 8] [--no-renderer]

Per pair at one frame size (default 1008 x 756), on an analytic scene (a textured plane with a sphere in front of it, two
cameras on a small baseline, exact fp64 distances rounded to f32):
    fused metric         nsr_reproject_frames writing stats only (what Renderer.view_consistency launches)
    fused warped + mask  the same call writing the warped frame and the mask as well
    torch composition    what a caller would write: the rays, the world points and the projection as elementwise fp64 ops,
                         torch.nn.functional.grid_sample (bilinear, align_corners) of the src colours, of the src distances
                         and of the src "has a surface" plane, the masks and a masked sum
Every variant is captured as one graph of INNER calls (the fused ones through the C entry point with the caller's buffers, as a
captured step would hold them), the graphs are replayed in turn, --reps rounds, and the median per variant is reported in
microseconds per pair with the spread (min, max), beside the bytes the kernel has to move for a pair and the rate that makes.
Then, unless --no-renderer: Renderer.view_consistency over --frames frames of the room cameras (gaps 1 and frames - 1) on the
seeded field, split into its renders and its reprojection calls, beside one training step of 4096 rays of the same renderer."""
import argparse, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--h', type=int, default=756)
ap.add_argument('--w', type=int, default=1008)
ap.add_argument('--frames', type=int, default=8)
ap.add_argument('--no-renderer', action='store_true')
args = ap.parse_args()

import torch
import torch.nn.functional as F
from nerfstyle_amd import _lib as L
from nerfstyle_amd import consistency as C
from nerfstyle_amd.common import Intrinsics

assert torch.cuda.is_available(), 'bench_consistency.py needs a HIP device'
dev = torch.device('cuda:0')
H, W = args.h, args.w
HW = H * W
INNER = 10
TOL = 0.01
f64 = torch.float64
intr = Intrinsics(H, W, 0.84 * W, 0.84 * W, W / 2.0 - 0.3, H / 2.0 + 0.4)


def rot(rx, ry):
    cx, sx, cy, sy = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry)
    return torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=f64) @ torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=f64)


def pixel_dirs(pose):
    """unit ray directions of every pixel, camera_flip 0, fp64 on the device -> [H*W, 3]"""
    p = torch.arange(HW, device=dev)
    x = ((p % W).to(f64) + 0.5 - intr.cx) / intr.fx
    y = ((p // W).to(f64) + 0.5 - intr.cy) / intr.fy
    v = torch.stack((x, y, torch.ones_like(x)), dim=1) @ pose[:, :3].to(f64).t()
    return v / v.norm(dim=1, keepdim=True)


def make_scene():
    """the plane z = 4 and a sphere in front of it, two cameras at the origin's side looking along +z"""
    poses = torch.zeros(2, 3, 4, dtype=torch.float32)
    poses[0, :, :3], poses[1, :, :3] = rot(0.0, 0.0).float(), rot(0.02, -0.05).float()
    poses[1, :, 3] = torch.tensor([0.3, 0.05, 0.1])
    poses = poses.to(dev)
    centre, radius = torch.tensor([0.15, -0.1, 2.6], dtype=f64, device=dev), 0.55
    rgb, dist = [], []
    for f in range(2):
        d, o = pixel_dirs(poses[f]), poses[f, :, 3].to(f64)
        tp = torch.where(d[:, 2] > 0, (4.0 - o[2]) / d[:, 2], torch.full_like(d[:, 2], float('inf')))
        oc = o - centre
        b = d @ oc
        disc = b * b - (oc @ oc - radius * radius)
        ts = torch.where(disc > 0, -b - torch.sqrt(disc.clamp(min=0)), torch.full_like(b, float('inf')))
        t = torch.minimum(tp, torch.where(ts > 0, ts, torch.full_like(ts, float('inf'))))
        X = o + t[:, None] * d
        rgb.append(torch.stack((0.5 + 0.4 * torch.sin(1.3 * X[:, 0] + 0.7 * X[:, 1]), 0.5 + 0.4 * torch.sin(0.9 * X[:, 1] - 1.1 * X[:, 0] + 1.0),
                                0.5 + 0.4 * torch.cos(0.8 * X[:, 0] + 1.2 * X[:, 1] - 0.6 * X[:, 2])), dim=1).float())
        dist.append(t.float())
    return torch.stack(rgb).contiguous(), torch.stack(dist).contiguous(), poses


rgb, dist, poses = make_scene()
PAIRS = [(0, 1), (1, 0)]
P = len(PAIRS)
pairs_dev = torch.tensor(PAIRS, dtype=torch.int32, device=dev)
warped = torch.empty(P, HW, 3, device=dev)
mask = torch.empty(P, HW, dtype=torch.uint8, device=dev)
stats = torch.empty(P, 2, dtype=f64, device=dev)
ws = torch.empty(int(L.lib().nsr_reproject_frames_workspace_bytes(P, H, W)) // 8, dtype=f64, device=dev)


def fused(want_outputs):
    L.check(L.lib().nsr_reproject_frames(L.p(rgb), L.p(dist), L.p(poses), 2, H, W, intr.fx, intr.fy, intr.cx, intr.cy, 0, L.p(pairs_dev), P,
                                         TOL, L.p(warped) if want_outputs else None, L.p(mask) if want_outputs else None, L.p(stats),
                                         L.p(ws), L.stream()), 'reproject_frames')


DIRS = [pixel_dirs(poses[f]) for f in range(2)]          # the composition may keep its rays: they do not depend on the images
SURF = [((dist[f] > 0) & torch.isfinite(dist[f])) for f in range(2)]
torch_stats = torch.zeros(P, 2, dtype=f64, device=dev)


def torch_pair(i, a, b):
    """steps 1 to 7 of include/nsr.h for one pair, composed from torch ops in fp64"""
    o_a, o_b, R_b = poses[a, :, 3].to(f64), poses[b, :, 3].to(f64), poses[b, :, :3].to(f64)
    t = torch.where(SURF[a], dist[a], torch.ones_like(dist[a])).to(f64)
    dx = o_a + t[:, None] * DIRS[a] - o_b
    q = dx @ R_b
    z = q[:, 2]
    zs = torch.where(z > 0, z, torch.ones_like(z))
    u = intr.fx * (q[:, 0] / zs) + intr.cx - 0.5
    w = intr.fy * (q[:, 1] / zs) + intr.cy - 0.5
    inside = (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
    grid = torch.stack((u / (W - 1) * 2 - 1, w / (H - 1) * 2 - 1), dim=1).view(1, H, W, 2)
    planes = torch.cat((rgb[b].view(H, W, 3).permute(2, 0, 1), dist[b].view(1, H, W), SURF[b].view(1, H, W).float()), dim=0).to(f64)[None]
    s = F.grid_sample(planes, grid, mode='bilinear', padding_mode='border', align_corners=True)[0].reshape(5, HW)
    r = dx.norm(dim=1)
    valid = SURF[a] & (z > 0) & inside & (s[4] >= 1.0) & ((r - s[3]).abs() <= TOL * r)
    e = (s[:3].t() - rgb[a].to(f64)) * valid[:, None]
    torch_stats[i, 0] = (e * e).sum()
    torch_stats[i, 1] = valid.sum()


def torch_all():
    for i, (a, b) in enumerate(PAIRS):
        torch_pair(i, a, b)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
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
    """microseconds per pair of every graph: one replay of each in turn, --reps rounds -> {name: (median, min, max)}"""
    times = {k: [] for k in graphs}
    for _ in range(args.reps):
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / (INNER * P))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


fused(True)
torch_all()
torch.cuda.synchronize()
fs, tsn = stats.cpu(), torch_stats.cpu()
print('{}x{}, {} pairs: fused (sse, n_valid) {}; torch composition {}'.format(W, H, P, fs.tolist(), tsn.tolist()))
print('  rmse fused {}  torch {}; n_valid differs by {}'.format(C.warp_error(fs, H, W)[:, 0].tolist(), C.warp_error(tsn, H, W)[:, 0].tolist(),
                                                                (fs[:, 1] - tsn[:, 1]).abs().tolist()))
res = alternating({'fused metric': capture(lambda: fused(False)), 'fused warped + mask': capture(lambda: fused(True)),
                   'torch composition': capture(torch_all)})
# what a pair has to move: dist[a] and rgb[a] once, every row of dist[b] and rgb[b] once (neighbouring pixels share their taps through
# the caches), the two slots; with the outputs the warped frame and the mask
bytes_metric = HW * (4 + 12 + 4 + 12) + 16 * ((HW + 255) // 256)
bytes_full = bytes_metric + HW * 13
for k, (med, lo, hi) in res.items():
    nb = {'fused metric': bytes_metric, 'fused warped + mask': bytes_full}.get(k)
    rate = '; {:.2f} MB a pair, {:.2f} TB/s'.format(nb / 1e6, nb / med / 1e6) if nb else ''
    print('  {:20s} {:9.1f} us per pair (min {:.1f}, max {:.1f}; {} rounds of {} calls of {} pairs){}'.format(k, med, lo, hi, args.reps, INNER,
                                                                                                          P, rate))
print('  torch / fused metric = {:.1f}x, torch / fused warped + mask = {:.1f}x'.format(res['torch composition'][0] / res['fused metric'][0],
                                                                                       res['torch composition'][0] / res['fused warped + mask'][0]))

if not args.no_renderer:
    import numpy as np
    from nerfstyle_amd import raymarching
    from nerfstyle_amd.common import BBox
    from nerfstyle_amd.config import NetworkConfig, RendererConfig
    from nerfstyle_amd.optim import FusedAdam
    from nerfstyle_amd.renderer import Renderer
    from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
    from nerfstyle_amd.style_nerf import StyleTCNerf

    torch.manual_seed(0)
    model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, use_dir=False)
    cam_poses, cam_intr, _ = load_room_cameras()
    cfg = RendererConfig.llff()
    cfg.density_scale = 40.0
    r = Renderer(model, cfg, cam_intr.scale(W, H), 2.0, raymarch_channels=8, samples_per_ray_cap=128).to(dev)
    r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 48, 0), device=dev)
    r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
    r.update_occ = False
    Fn = min(args.frames, len(cam_poses))
    vposes = torch.tensor(np.asarray(cam_poses[:Fn], np.float32), device=dev)
    gaps = (1, max(Fn - 1, 1))

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    r.view_consistency(vposes[:2], gaps=(1,))                      # warm-up of every shape the timed calls use
    total, out = timed(lambda: r.view_consistency(vposes, gaps=gaps), 2)
    frames = [r.render_rgbd(vposes[i]) for i in range(Fn)]
    held = (torch.stack([f['rgb_map'] for f in frames]), torch.stack([f['distance'] for f in frames]))
    metric, _ = timed(lambda: r.view_consistency(vposes, gaps=gaps, frames=held), 5)
    print('view_consistency, {} frames of {}x{}, gaps {}: {:.1f} ms in all, of which {:.2f} ms the {} reprojected pairs (the rest: {} '
          'render_rgbd calls); fell back to the loop: {}'.format(Fn, W, H, gaps, total, metric, sum(Fn - g for g in gaps), Fn, r.last_test_overflow))
    print('  coverage (gap {}) {}'.format(gaps[0], [round(v, 3) for v in out[gaps[0]][:, 1].tolist()]))
    opt = FusedAdam(model, lr=1e-3)
    pix = torch.randint(0, HW, (4096,), device=dev)

    def step():
        o = r.render(vposes[0], None, training=True, pix_subset=pix)
        torch.mean((o['rgb_map'] - 0.5) ** 2).backward()
        opt.step()

    step()
    ms, _ = timed(step, 20)
    print('  one eager training step of 4096 rays on the same renderer: {:.2f} ms; the metric of the {} frames is {:.1f} steps, the renders '
          'included {:.1f}'.format(ms, Fn, metric / ms, total / ms))
