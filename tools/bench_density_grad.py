"""Runs the sigma-only fused forward and the forward-mode density gradient on the marched samples of one full frame, for a
rocprofv3 --kernel-trace --stats run to time k_field_fwd (sigma only) against k_field_density_grad at the same M:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_density_grad.py [scale] [--cap K] [--reps R]

scale 1 = 504x378, 2 = 1008x756 (default).  Prints the sample count and wall-clock ms per call of either as a cross-check."""
import argparse, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nerfstyle_amd import raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.rays import generate_rays
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
from nerfstyle_amd.style_nerf import StyleTCNerf

ap = argparse.ArgumentParser()
ap.add_argument('scale', nargs='?', type=int, default=2)
ap.add_argument('--cap', type=int, default=192)
ap.add_argument('--reps', type=int, default=10)
args = ap.parse_args()

dev = torch.device('cuda:0')
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
with torch.no_grad():
    model.arena[:model.table_elems].uniform_(-0.5, 0.5)
poses, intr, _ = load_room_cameras(args.scale)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=8, samples_per_ray_cap=args.cap).to(dev)
r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 28, 0), device=dev)
r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
r.update_occ = False
rays, _ = generate_rays(torch.tensor(poses[0], device=dev), intr, None, camera_flip=r.cfg.flip_camera, device=dev)
with torch.no_grad():
    mt = r.march_train(rays)
    xyzs, cnt = mt['xyzs'], mt['counter']
    print('{}x{}: {} samples in a buffer of {}'.format(intr.w, intr.h, int(cnt[0]), mt['M']))
    for name, fn in (('field(sigma_only)', lambda: model.field(xyzs, sigma_only=True, m_dev=cnt)),
                     ('density_gradient', lambda: model.density_gradient(xyzs, m_dev=cnt)),
                     ('density_gradient(normalize)', lambda: model.density_gradient(xyzs, m_dev=cnt, normalize=True))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        print('{:28s} {:8.3f} ms/call'.format(name, (time.perf_counter() - t0) / args.reps * 1e3))
