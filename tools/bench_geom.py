"""Times the per-ray geometry kernels (nsr_ray_geometry_forward / _backward) beside the training composite pair
(nsr_render_train_forward / _backward) on the SAME buffers: the marched samples of the bench frame (1008x756 room camera, the
seeded 28-box occupancy, 160 samples per ray of capacity, f16 tables), shaded once by the fused field.

    timeout 300 python tools/bench_geom.py [--scale 2] [--cap 160] [--rounds 15]

One process.  The four launches alternate round by round (geometry fwd, geometry bwd, composite fwd, composite bwd, again ...),
each timed by a pair of events around the one launch after two untimed warm-up rounds; the medians over the rounds are printed,
with the min and max, and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nerfstyle_amd import _lib as L  # noqa: E402
from nerfstyle_amd import raymarching  # noqa: E402
from nerfstyle_amd.common import BBox  # noqa: E402
from nerfstyle_amd.config import NetworkConfig, RendererConfig  # noqa: E402
from nerfstyle_amd.rays import generate_rays  # noqa: E402
from nerfstyle_amd.renderer import Renderer  # noqa: E402
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid  # noqa: E402
from nerfstyle_amd.style_nerf import StyleTCNerf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scale', type=int, default=2, help='2 = 1008x756 (the bench frame), 1 = 504x378')
ap.add_argument('--cap', type=int, default=160)
ap.add_argument('--rounds', type=int, default=15)
args = ap.parse_args()

dev = torch.device('cuda:0')
nc = 5
C = 3 + nc
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), nc, enc_dtype=None, use_dir=False)
poses, intr, _ = load_room_cameras(args.scale)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=C, samples_per_ray_cap=args.cap).to(dev)
r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 28, 0), device=dev)
r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
r.update_occ = False
rays, _ = generate_rays(torch.tensor(poses[0], device=dev), intr, None, camera_flip=r.cfg.flip_camera, device=dev)
with torch.no_grad():
    mt = r.march_train(rays)
    sigmas, rgbs = model.field(mt['xyzs'], sigma_only=False, m_dev=mt['counter'], density_scale=r.cfg.density_scale)
deltas, rinfo, nears, fars = mt['deltas'], mt['rays_info'], mt['nears'], mt['fars']
N, M, T_thresh = mt['N'], mt['M'], float(r.cfg.t_thresh)
count = int(mt['counter'][0])
print('{}x{}: {} rays, {} samples in a buffer of {}'.format(intr.w, intr.h, N, count, M))


def f32(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


depth, dist, totals = f32(N), f32(N), f32(N, 4)
ws, depth_raw, image, rgb_map, depth_norm, classes = f32(N), f32(N), f32(N, C), f32(N, 3), f32(N), f32(N, nc)
g_depth, g_dist, g_rgb, g_cls = torch.rand(N, device=dev), torch.rand(N, device=dev), torch.rand(N, 3, device=dev), torch.rand(N, nc, device=dev)
gs_geo, gs_cmp, gr_cmp = f32(M), f32(M), f32(M, C)
lib, s = L.lib(), L.stream()

launches = {
    'geometry_fwd': lambda: lib.nsr_ray_geometry_forward(L.p(sigmas), L.p(deltas), L.p(rinfo), L.p(nears), L.p(fars), M, N, T_thresh, 0,
                                                         L.p(depth), L.p(dist), L.p(totals), s),
    'geometry_bwd': lambda: lib.nsr_ray_geometry_backward(L.p(g_depth), L.p(g_dist), L.p(sigmas), L.p(deltas), L.p(rinfo), L.p(nears),
                                                          L.p(fars), L.p(totals), M, N, T_thresh, 0, L.p(gs_geo), s),
    'composite_fwd': lambda: lib.nsr_render_train_forward(L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rinfo), L.p(nears), L.p(fars), M, N, C,
                                                          T_thresh, L.p(ws), L.p(depth_raw), L.p(image), L.p(rgb_map), L.p(depth_norm),
                                                          L.p(classes), s),
    'composite_bwd': lambda: lib.nsr_render_train_backward(L.p(g_rgb), L.p(g_cls), None, L.p(sigmas), L.p(rgbs), L.p(deltas), L.p(rinfo),
                                                           L.p(ws), L.p(image), M, N, C, T_thresh, L.p(gs_cmp), L.p(gr_cmp), s),
}
times = {k: [] for k in launches}
for rnd in range(args.rounds + 2):
    for name, fn in launches.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(fn(), name)
        e1.record()
        e1.synchronize()
        if rnd >= 2:
            times[name].append(e0.elapsed_time(e1))
res = {}
for name, t in times.items():
    res[name] = statistics.median(t)
    print('{:14s} median {:7.3f} ms   min {:7.3f}   max {:7.3f}   ({} rounds)'.format(name, res[name], min(t), max(t), len(t)))
res.update(rays=N, samples=count, capacity=M)
print(json.dumps(res))
