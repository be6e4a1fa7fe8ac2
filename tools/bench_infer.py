"""Times a full-frame inference render (render.py:97 path: Renderer.render(pose) -> render_test), the same frame through the
training path without gradients, and through the streaming kernel with either composite (render_test_fused,
render_train_fused); prints ms, peak memory over the call and samples shaded / samples emitted, and the PSNR between the paths.

    python tools/bench_infer.py [scale] [--density-scale S] [--cap K] [--reps R]

scale 1 = 504x378, 2 = 1008x756 (default).  --density-scale: 1 (default) is a fog no ray terminates in, a few hundred makes the
synthetic boxes opaque.  --cap: samples per ray of the buffered paths' sample buffers (default 192; the fused path has none)."""
import argparse, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from nerfstyle_amd import raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_room_cameras, synthetic_density_grid
from nerfstyle_amd.style_nerf import StyleTCNerf

ap = argparse.ArgumentParser()
ap.add_argument('scale', nargs='?', type=int, default=2)
ap.add_argument('--density-scale', type=float, default=1.0)
ap.add_argument('--cap', type=int, default=192)
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()

dev = torch.device('cuda:0')
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False)
with torch.no_grad():
    model.arena[:model.table_elems].uniform_(-0.5, 0.5)
poses, intr, _ = load_room_cameras(args.scale)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=8, samples_per_ray_cap=args.cap).to(dev)
r.cfg.density_scale = args.density_scale
r.density_grid = torch.tensor(synthetic_density_grid(2.0, 128, 28, 0), device=dev)
r.density_bitfield = raymarching.packbits(r.density_grid, 0.5)
r.update_occ = False
pose = torch.tensor(poses[0], device=dev)
print('density_scale {}  buffered paths: {} samples per ray'.format(args.density_scale, args.cap))
imgs = {}
emitted = None
for name, training, fused in (('render_test', False, False), ('render_train(no_grad)', True, False), ('render_test_fused', False, True),
                              ('render_train_fused(no_grad)', True, True)):
    r.fused_inference = fused and not training
    r.fused_nograd_train = fused and training
    with torch.no_grad():
        out = r.render(pose, None, training=training)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = r.render(pose, None, training=training)
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.reps * 1e3
    peak = torch.cuda.max_memory_allocated() - before
    note = ''
    if training and not fused:
        emitted = int(r._last_counter[0])
        note = '  emitted {} samples{}'.format(emitted, ' (buffer overflowed: rays dropped)' if emitted >= r._last_capacity else '')
    elif fused:
        shaded = int(r.last_infer_stats()[0])
        note = '  shaded {} samples = {:.3f} of emitted'.format(shaded, shaded / max(emitted, 1))
    elif r.last_test_overflow:
        note = '  (buffer overflowed: fell back to the host loop)'
    print('{:24s} {}x{}: {:8.2f} ms/frame  ({:.2f} Mrays/s)  peak {:9.1f} MB{}'.format(
        name, intr.w, intr.h, ms, intr.w * intr.h / ms / 1e3, peak / 1e6, note))
    imgs[name] = out['rgb_map']


def psnr(a, b):
    return -10 * np.log10(max(float(((a - b) ** 2).mean()), 1e-12))


print('PSNR(render_train vs render_train_fused) = {:.1f} dB, max |diff| {:.2e}'.format(
    psnr(imgs['render_train(no_grad)'], imgs['render_train_fused(no_grad)']),
    float((imgs['render_train(no_grad)'] - imgs['render_train_fused(no_grad)']).abs().max())))
print('PSNR(render_test vs render_train) = {:.1f} dB'.format(psnr(imgs['render_test'], imgs['render_train(no_grad)'])))
print('PSNR(render_test vs render_test_fused) = {:.1f} dB, max |diff| {:.2e}'.format(
    psnr(imgs['render_test'], imgs['render_test_fused']), float((imgs['render_test'] - imgs['render_test_fused']).abs().max())))
