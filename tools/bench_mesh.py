"""Mesh export on one device (HIP events and a host clock around a synchronise, no profiler):

    python tools/bench_mesh.py [--reps R] [--res 256 512] [--iso ISO]

On bench.py's model (the seeded random initialisation over the bound-2 box; its density is 1.0 +- 0.09, so the default iso is the
median of the sampled volume: half the lattice is inside and the surface is as large and as ragged as this field makes it -- an
upper bound on the output a trained scene of the same resolution writes), per resolution:
    density_volume    the sigma-only lattice sweep
    count, emit       nsr_surface_nets_count and nsr_surface_nets_emit on that volume, events around each call; the same two on
                      a smooth analytic field of the same size, whose surface has the O(res^2) vertices of a real scene
    surface_nets      the Python call: workspace and outputs allocated, count, the host read of V and Q, emit
    extract_mesh      Renderer.extract_mesh: all of the above plus normals, colours and labels of the vertices
and the bytes the extractor has to move (the volume once per pass: count, vertices, faces; cell_vertex written once and read
four times a quad; verts and faces written once) over the time of count + emit, against the HBM peak of the MI355X: 8.0 TB/s on
the data sheet, 6.29 TB/s measured with a float4 copy."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
ap.add_argument('--iso', type=float, default=None, help='default: the median of the sampled volume')
ap.add_argument('--num-classes', type=int, default=5)
args = ap.parse_args()

import ctypes
import torch
from nerfstyle_amd import _lib as L
from nerfstyle_amd import mesh
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_cameras
from nerfstyle_amd.style_nerf import StyleTCNerf

assert torch.cuda.is_available(), 'bench_mesh.py needs a HIP device'
dev = torch.device('cuda:0')
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12

model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), args.num_classes, enc_dtype=None, use_dir=False, compute_dtype=torch.float16)
_, intr, _ = load_cameras('room', 2)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=3 + args.num_classes).to(dev)
LO, HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)


def median(v):
    return sorted(v)[len(v) // 2]


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(label, res, vol, iso, whole):
    shape = (res, res, res)
    n = res ** 3
    lo32, step = mesh.lattice_step(LO, HI, shape)
    fp = ctypes.POINTER(ctypes.c_float)
    ws = torch.empty(int(L.lib().nsr_surface_nets_workspace_bytes(*shape)) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def count():
        L.check(L.lib().nsr_surface_nets_count(L.p(vol), *shape, iso, L.p(ws), L.p(counts), L.stream()), 'count')
    count()
    V, Q = counts.cpu().tolist()
    verts = torch.empty(V, 3, device=dev)
    faces = torch.empty(2 * Q, 3, dtype=torch.int32, device=dev)

    def emit():
        L.check(L.lib().nsr_surface_nets_emit(L.p(vol), *shape, iso, lo32.ctypes.data_as(fp), step.ctypes.data_as(fp), L.p(ws), V, Q,
                                              L.p(verts), L.p(faces), L.stream()), 'emit')
    emit()
    t_count, t_emit, t_sn, t_all = [], [], [], []
    for _ in range(args.reps):
        t_count.append(event_ms(count))
        t_emit.append(event_ms(emit))
        t_sn.append(host_ms(lambda: mesh.surface_nets(vol, iso, LO, HI))[0])
    del verts, faces, ws
    moved = 3 * 4 * n + 4 * V + 16 * Q + 12 * V + 24 * Q
    kern_ms = median(t_count) + median(t_emit)
    rate = moved / (kern_ms * 1e-3)
    print('{}^3 {}, iso {:.4f}: V {} F {} ({:.1f} % of the cells active)'.format(res, label, iso, V, 2 * Q, 100.0 * V / (res - 1) ** 3))
    print('  count          {:9.3f} ms (min {:.3f}, max {:.3f}; the volume once: {:.2f} TB/s)'.format(
        median(t_count), min(t_count), max(t_count), 4 * n / (median(t_count) * 1e-3) / 1e12))
    print('  emit           {:9.3f} ms (min {:.3f}, max {:.3f}; with its host read of the header)'.format(median(t_emit), min(t_emit), max(t_emit)))
    print('  surface_nets   {:9.3f} ms (min {:.3f}, max {:.3f}; host clock, allocations and the host read of the counts in)'.format(
        median(t_sn), min(t_sn), max(t_sn)))
    print('  count + emit move {:.1f} MB in {:.3f} ms = {:.2f} TB/s: {:.0f} % of the {:.1f} TB/s data sheet, {:.0f} % of the {:.2f} TB/s copy'.format(
        moved / 1e6, kern_ms, rate / 1e12, 100 * rate / HBM_SPEC, HBM_SPEC / 1e12, 100 * rate / HBM_COPY, HBM_COPY / 1e12))
    if whole:
        for _ in range(max(args.reps // 4, 3)):
            t_all.append(host_ms(lambda: r.extract_mesh(resolution=res, iso=iso))[0])
        print('  extract_mesh   {:9.2f} ms (min {:.2f}, max {:.2f}; host clock)'.format(median(t_all), min(t_all), max(t_all)))


for res in args.res:
    n = res ** 3
    vol_ms, vol = host_ms(lambda: mesh.density_volume(model, LO, HI, res, density_scale=r.cfg.density_scale))
    vol_ms = min(vol_ms, host_ms(lambda: mesh.density_volume(model, LO, HI, res, density_scale=r.cfg.density_scale))[0])
    iso = float(vol.reshape(-1)[::max(n // (1 << 22), 1)].median()) if args.iso is None else args.iso
    print('{}^3: density_volume {:.2f} ms'.format(res, vol_ms))
    measure('model density', res, vol, iso, True)
    del vol
    # a smooth field, the surface a reconstructed scene has: O(res^2) vertices, the passes are the reads of the volume
    g = torch.linspace(-1.0, 1.0, res, device=dev)
    smooth = (torch.sin(3.1 * g + 0.3)[:, None, None] * torch.sin(2.3 * g + 1.1)[None, :, None] * torch.sin(4.2 * g + 0.7)[None, None, :]).contiguous()
    measure('smooth field', res, smooth, 0.3, False)
    del smooth
