"""The occupancy-grid floater cull on one device (HIP events and a host clock around a synchronise, no profiler):

    python tools/bench_occ_cull.py [--reps R] [--timeout S]

At the LLFF grid (2 cascades of 128^3 cells, a 512 KiB bitfield) on three bitfields --
    random   seeded, 30 % of the bits set: hundreds of thousands of small components
    full     every bit set: one component of 2 M cells a cascade, every hook and every statistic aimed at one root
    model    bench.py's model (random initialisation, seed 0) after one full Renderer.update_state
-- events around each of the three C calls
    labelling    nsr_occ_components (init, the union-find over the cells, flatten)
    statistics   nsr_occ_component_stats
    cull         nsr_occ_cull with a grid (the permanent mode), on a copy of the bitfield, with min_cells 64
and a host clock around the whole Renderer.cull_floaters(min_cells=64) (the three calls, the keep rule in torch, allocations),
restoring the grid between calls.  Each bitfield is measured by a child process of its own under --timeout seconds; the first
one that fails ends the run.  Nothing is compared against a threshold."""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ('random', 'full', 'model')
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--timeout', type=float, default=120.0, help='seconds a bitfield may take')
ap.add_argument('--min-cells', type=int, default=64)
ap.add_argument('--num-classes', type=int, default=5)
ap.add_argument('--case', choices=CASES, help='measure this bitfield in this process (what the parent starts)')
args = ap.parse_args()

if args.case is None:
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), '--case', case, '--reps', str(args.reps), '--min-cells', str(args.min_cells),
               '--num-classes', str(args.num_classes)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit('bench_occ_cull.py: {} did not end within {:.0f} s'.format(case, args.timeout))
        if rc != 0:
            sys.exit('bench_occ_cull.py: {} ended with status {}'.format(case, rc))
    sys.exit(0)

import numpy as np
import torch
from nerfstyle_amd import _lib as L
from nerfstyle_amd import raymarching
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig, RendererConfig
from nerfstyle_amd.renderer import Renderer
from nerfstyle_amd.scene import load_cameras
from nerfstyle_amd.style_nerf import StyleTCNerf

assert torch.cuda.is_available(), 'bench_occ_cull.py needs a HIP device'
dev = torch.device('cuda:0')
torch.manual_seed(0)
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), args.num_classes, enc_dtype=None, use_dir=False, compute_dtype=torch.float16)
_, intr, _ = load_cameras('room', 2)
r = Renderer(model, RendererConfig.llff(), intr, 2.0, raymarch_channels=3 + args.num_classes).to(dev)
r.manual_seed(0)
C, H = r.cascade, r.cfg.grid_size
cells = C * H ** 3
assert (C, H) == (2, 128)

if args.case == 'random':
    bits = torch.from_numpy(np.packbits(np.random.default_rng(0).random(cells) < 0.3, bitorder='little')).to(dev)
    grid = torch.ones(C, H ** 3, device=dev)
elif args.case == 'full':
    bits = torch.full((cells // 8,), 0xFF, dtype=torch.uint8, device=dev)
    grid = torch.ones(C, H ** 3, device=dev)
else:
    r.update_state()
    bits, grid = r.density_bitfield.clone(), r.density_grid.clone()


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(name, t, note=''):
    print('  {:14s} {:9.3f} ms (min {:.3f}, max {:.3f}){}'.format(name, median(t), min(t), max(t), note))


lib = L.lib()
labels = torch.empty(cells, dtype=torch.int32, device=dev)
n_cells = torch.empty(cells, dtype=torch.int32, device=dev)
lo, hi = (torch.empty(cells, 3, dtype=torch.int32, device=dev) for _ in range(2))
n_culled = torch.empty(C, dtype=torch.int32, device=dev)
work_bits, work_grid = bits.clone(), grid.clone()


def label_():
    L.check(lib.nsr_occ_components(L.p(bits), C, H, L.p(labels), L.stream()), 'components')


def stats_():
    L.check(lib.nsr_occ_component_stats(L.p(labels), C, H, L.p(n_cells), L.p(lo), L.p(hi), L.stream()), 'stats')


label_()
stats_()
keep = raymarching.keep_occupancy_components(n_cells, lo, hi, C, H, r.bound, min_cells=args.min_cells)


def cull_():
    L.check(lib.nsr_occ_cull(L.p(work_grid), L.p(work_bits), L.p(labels), L.p(keep), C, H, L.p(n_culled), L.stream()), 'cull')


t = {k: [] for k in ('label', 'stats', 'cull', 'python')}
for _ in range(args.reps):
    t['label'].append(event_ms(label_))
    t['stats'].append(event_ms(stats_))
    work_bits.copy_(bits)
    work_grid.copy_(grid)
    t['cull'].append(event_ms(cull_))
for _ in range(args.reps):
    r.density_bitfield, r.density_grid = bits.clone(), grid.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r.cull_floaters(min_cells=args.min_cells)
    torch.cuda.synchronize()
    t['python'].append((time.perf_counter() - t0) * 1e3)

occupied = int(torch.from_numpy(np.unpackbits(bits.cpu().numpy(), bitorder='little')).sum())
roots = int((labels == torch.arange(cells, dtype=torch.int32, device=dev)).sum())
print('{}: {} of {} cells occupied, {} components, the largest of {} cells; min_cells {} culls {} cells'.format(
    args.case, occupied, cells, roots, int(n_cells.max()), args.min_cells, n_culled.cpu().tolist()))
line('labelling', t['label'], '  {:.2f} G occupied cells/s'.format(occupied / (median(t['label']) * 1e-3) / 1e9 if occupied else 0.0))
line('statistics', t['stats'])
line('cull', t['cull'])
print('  the three calls {:8.3f} ms'.format(sum(median(t[k]) for k in ('label', 'stats', 'cull'))))
line('cull_floaters', t['python'], '  host clock: the three calls, the keep rule in torch, allocations')
