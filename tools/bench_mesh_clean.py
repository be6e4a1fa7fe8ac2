"""Mesh cleaning on one device (HIP events and a host clock around a synchronise, no profiler):

    python tools/bench_mesh_clean.py [--reps R] [--res 512] [--min-faces M]

On the two volumes of tools/bench_mesh.py per resolution -- bench.py's model density at its median (about 70 % of the cells
active: an upper bound on what a scene writes, and thousands of components) and the smooth analytic field (O(res^2) vertices,
a few large sheets) -- the mesh of nsr_surface_nets_count / _emit, then, events around each call:
    labelling      nsr_mesh_components (init, the union-find over the faces, flatten) and its compare-and-swap rate: two
                   unites a face, each at least one compare-and-swap or a find that ends in the same root
    statistics     nsr_mesh_component_stats
    filter count   nsr_mesh_filter_count, filter emit: nsr_mesh_filter_emit (with its host read of the header)
    filter_components   the Python call: all of the above, the keep rule in torch, allocations and host reads
beside the extractor's own time (count + emit) and the number of components; and on the model, the whole
Renderer.extract_mesh without and with min_faces."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--res', type=int, nargs='+', default=[512])
ap.add_argument('--min-faces', type=int, default=64)
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

assert torch.cuda.is_available(), 'bench_mesh_clean.py needs a HIP device'
dev = torch.device('cuda:0')

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


def line(name, t, note=''):
    print('  {:18s} {:9.3f} ms (min {:.3f}, max {:.3f}){}'.format(name, median(t), min(t), max(t), note))


def measure(label, res, vol, iso, whole):
    shape = (res, res, res)
    lo32, step = mesh.lattice_step(LO, HI, shape)
    fp = ctypes.POINTER(ctypes.c_float)
    lib = L.lib()
    ws = torch.empty(int(lib.nsr_surface_nets_workspace_bytes(*shape)) // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def sn_count():
        L.check(lib.nsr_surface_nets_count(L.p(vol), *shape, iso, L.p(ws), L.p(counts), L.stream()), 'count')
    sn_count()
    V, Q = counts.cpu().tolist()
    F = 2 * Q
    verts = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

    def sn_emit():
        L.check(lib.nsr_surface_nets_emit(L.p(vol), *shape, iso, lo32.ctypes.data_as(fp), step.ctypes.data_as(fp), L.p(ws), V, Q,
                                          L.p(verts), L.p(faces), L.stream()), 'emit')
    sn_emit()
    t_sn = [event_ms(sn_count) + event_ms(sn_emit) for _ in range(args.reps)]
    del ws

    labels = torch.empty(V, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)

    def label_():
        L.check(lib.nsr_mesh_components(L.p(faces), V, F, L.p(labels), L.p(bad), L.stream()), 'components')
    label_()
    n_verts = torch.empty(V, dtype=torch.int32, device=dev)
    n_faces = torch.empty(V, dtype=torch.int32, device=dev)
    blo, bhi = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)

    def stats_():
        L.check(lib.nsr_mesh_component_stats(L.p(verts), L.p(faces), L.p(labels), V, F, L.p(n_verts), L.p(n_faces), L.p(blo), L.p(bhi),
                                             L.stream()), 'stats')
    stats_()
    st = mesh.component_stats(verts, faces, labels)
    keep = mesh.keep_components(st, V, min_faces=args.min_faces)
    comps = int(st.roots.shape[0])
    largest = int(st.n_faces.max()) if comps else 0
    del st
    fws = torch.empty(int(lib.nsr_mesh_filter_workspace_bytes(V, F)) // 4, dtype=torch.int32, device=dev)

    def fcount():
        L.check(lib.nsr_mesh_filter_count(L.p(faces), L.p(labels), L.p(keep), V, F, L.p(fws), L.p(counts), L.stream()), 'filter_count')
    fcount()
    Vk, Fk = counts.cpu().tolist()
    imap = torch.empty(V, dtype=torch.int32, device=dev)
    vo, fo = torch.empty(Vk, 3, device=dev), torch.empty(Fk, 3, dtype=torch.int32, device=dev)

    def femit():
        L.check(lib.nsr_mesh_filter_emit(L.p(verts), L.p(faces), L.p(labels), L.p(keep), V, F, L.p(fws), Vk, Fk, L.p(imap), L.p(vo),
                                         L.p(fo), L.stream()), 'filter_emit')
    femit()
    t = {k: [] for k in ('label', 'stats', 'count', 'emit', 'python')}
    for _ in range(args.reps):
        t['label'].append(event_ms(label_))
        t['stats'].append(event_ms(stats_))
        t['count'].append(event_ms(fcount))
        t['emit'].append(event_ms(femit))
    del n_verts, n_faces, blo, bhi, imap, vo, fo, fws, keep, labels
    for _ in range(max(args.reps // 3, 3)):
        t['python'].append(host_ms(lambda: mesh.filter_components(verts, faces, min_faces=args.min_faces))[0])
    sn = median(t_sn)
    kern = sum(median(t[k]) for k in ('label', 'stats', 'count', 'emit'))
    print('{}^3 {}, iso {:.4f}: V {} F {}; {} components, the largest of {} faces; min_faces {} keeps V {} F {}'.format(
        res, label, iso, V, F, comps, largest, args.min_faces, Vk, Fk))
    line('surface nets', t_sn, '  count + emit')
    line('labelling', t['label'], '  {:.2f} G unites/s, {:.0f} % of surface nets'.format(2 * F / (median(t['label']) * 1e-3) / 1e9,
                                                                                       100 * median(t['label']) / sn))
    line('statistics', t['stats'], '  {:.0f} % of surface nets'.format(100 * median(t['stats']) / sn))
    line('filter count', t['count'], '  {:.0f} % of surface nets'.format(100 * median(t['count']) / sn))
    line('filter emit', t['emit'], '  {:.0f} % of surface nets; with its host read of the header'.format(100 * median(t['emit']) / sn))
    print('  the four calls     {:9.3f} ms = {:.0f} % of surface nets'.format(kern, 100 * kern / sn))
    line('filter_components', t['python'], '  host clock: the keep rule in torch, allocations and host reads in')
    del verts, faces
    if whole:
        n = max(args.reps // 3, 3)
        t_raw = [host_ms(lambda: r.extract_mesh(resolution=res, iso=iso))[0] for _ in range(n)]
        t_clean = [host_ms(lambda: r.extract_mesh(resolution=res, iso=iso, min_faces=args.min_faces))[0] for _ in range(n)]
        line('extract_mesh', t_raw, '  host clock, no cleaning')
        line('extract_mesh clean', t_clean, '  host clock, min_faces {}: {:+.0f} % of extract_mesh'.format(
            args.min_faces, 100 * (median(t_clean) - median(t_raw)) / median(t_raw)))


for res in args.res:
    n = res ** 3
    vol = mesh.density_volume(model, LO, HI, res, density_scale=r.cfg.density_scale)
    iso = float(vol.reshape(-1)[::max(n // (1 << 22), 1)].median())
    measure('model density', res, vol, iso, True)
    del vol
    g = torch.linspace(-1.0, 1.0, res, device=dev)
    smooth = (torch.sin(3.1 * g + 0.3)[:, None, None] * torch.sin(2.3 * g + 1.1)[None, :, None] * torch.sin(4.2 * g + 0.7)[None, None, :]).contiguous()
    measure('smooth field', res, smooth, 0.3, False)
    del smooth
