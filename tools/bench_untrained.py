"""What Renderer.mark_untrained_grid does on the two shipped camera sets (LLFF room and fern, the default 128^3 grid, bound 2):

    python tools/bench_untrained.py [--reps R] [--margin M] [--min-views V]

Per scene: the share of cells marked per cascade by the training cameras (every 8th frame is held out, the LLFF convention), the
time of nsr_occ_mark_untrained (HIP events, the median of --reps calls; the call is idempotent), and last_infer_stats() --
(samples shaded, rays finished) -- of render_test_fused for the first held-out pose on a freshly initialised model after one
full occupancy update, without and with the marks.  A fresh model's density is about 1 everywhere, so that update's threshold is
the grid's mean, which the marks lower (a marked cell counts as 0): the last line renders the same view with every cell
occupied against every SEEN cell occupied, the geometric share of the view's samples that lie in marked cells."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--margin', type=float, default=1.5)
ap.add_argument('--min-views', type=int, default=1)
args = ap.parse_args()

import numpy as np
import torch
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.rays import generate_rays
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_cameras
from nerfstyle_amd.style_nerf import StyleTCNerf

dev = torch.device('cuda:0')


def fresh(intr):
    model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
    return Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=8).to(dev)


def shaded(r, pose, intr):
    """one full occupancy update from the model, then the held-out frame through the streaming render"""
    r.update_state()
    rays, _ = generate_rays(pose, intr, None, camera_flip=r.cfg.flip_camera, device=dev)
    r.render_test_fused(rays, dense_shape=intr.size())
    torch.cuda.synchronize()
    occupied = int(torch.count_nonzero(r.density_grid > 0))
    return [int(v) for v in r.last_infer_stats().cpu()], occupied


for scene in ('room', 'fern'):
    poses, intr, _ = load_cameras(scene)
    held = np.arange(len(poses)) % 8 == 0
    train, test_pose = poses[~held], poses[held][0]
    r = fresh(intr)
    H3 = r.cfg.grid_size ** 3
    n_un = r.mark_untrained_grid(train, margin_cells=args.margin, min_views=args.min_views).cpu().numpy()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r.mark_untrained_grid(train, margin_cells=args.margin, min_views=args.min_views)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    print('{}: {} training frames of {}, {}x{}, grid {} x {}^3, margin {}, min_views {}'.format(
        scene, len(train), len(poses), intr.w, intr.h, r.cascade, r.cfg.grid_size, args.margin, args.min_views), flush=True)
    print('    marked share per cascade: {}'.format(' '.join('{:.4f}'.format(n / H3) for n in n_un)), flush=True)
    print('    mark_untrained_grid: {:.1f} us per call (median of {}, host wrapper included)'.format(float(np.median(times)), args.reps), flush=True)
    (s1, f1), occ1 = shaded(r, test_pose, intr)
    (s0, f0), occ0 = shaded(fresh(intr), test_pose, intr)
    print('    held-out pose, fresh model, one full update: occupied cells {} -> {}, samples shaded {} -> {} ({:+.1f} %), rays finished {} -> {}'.format(
        occ0, occ1, s0, s1, 100.0 * (s1 - s0) / max(s0, 1), f0, f1), flush=True)
    # the same view with the threshold taken out: every cell occupied, against every cell the training cameras see
    geo = []
    for marks in (False, True):
        q = fresh(intr)
        q.density_bitfield.fill_(0xFF)
        if marks:
            q.mark_untrained_grid(train, margin_cells=args.margin, min_views=args.min_views)
        rays, _ = generate_rays(test_pose, intr, None, camera_flip=q.cfg.flip_camera, device=dev)
        q.render_test_fused(rays, dense_shape=intr.size())
        geo.append(int(q.last_infer_stats().cpu()[0]))
    print('    held-out pose, all cells occupied -> all seen cells occupied: samples shaded {} -> {} ({:+.1f} %)'.format(
        geo[0], geo[1], 100.0 * (geo[1] - geo[0]) / max(geo[0], 1)), flush=True)
