"""One full-frame training step (render, MSE, backward) with Renderer.pose_gradients on and one with it off, and the three
pose-gradient kernels' times from the profiling events of the step with it on:

    python tools/bench_pose_grad.py [scale] [--cap K] [--reps R]

scale 1 = 504x378, 2 = 1008x756 (default).  For per-kernel figures of k_field_xgrad, k_rays_pos_bwd and k_generate_rays_bwd run it
under rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_pose_grad.py."""
import argparse, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nerfstyle_amd import profiling, raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
from nerfstyle_amd.style_nerf import StyleTCNerf

ap = argparse.ArgumentParser()
ap.add_argument('scale', nargs='?', type=int, default=2)
ap.add_argument('--cap', type=int, default=192)
ap.add_argument('--reps', type=int, default=5)
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
image = torch.rand(3, intr.h, intr.w, device=dev)
LOSS_SCALE = 65536.0


def step(on):
    r.pose_gradients = on
    pose = torch.tensor(poses[0], device=dev)[:3].clone().requires_grad_(on)
    out = r.render(pose, image, training=True)
    # a mean over 2.3 M entries: without the trainer's loss scale the f16 operands of the MLP backward underflow to zero
    (((out['rgb_map'] - out['target']) ** 2).mean() * LOSS_SCALE).backward()
    model.arena.grad.zero_()
    return None if pose.grad is None else pose.grad / LOSS_SCALE


for on in (False, True):
    step(on)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        g = step(on)
    torch.cuda.synchronize()
    print('pose_gradients={!s:5}  {:8.3f} ms/step{}'.format(on, (time.perf_counter() - t0) / args.reps * 1e3,
                                                         '' if g is None else '  |pose.grad| {:.3e}'.format(float(g.norm()))))
print('{}x{}: {} samples'.format(intr.w, intr.h, int(r._last_counter[0])))
profiling.reset()
profiling.enabled = True
step(True)
torch.cuda.synchronize()
profiling.enabled = False
for name, (n, _, avg) in sorted(profiling.summary().items()):
    if name in ('field_pos_grad', 'rays_position_bwd', 'field_bwd', 'field_fwd'):
        print('{:20s} {:8.3f} ms ({} launch{})'.format(name, avg, n, '' if n == 1 else 'es'))
