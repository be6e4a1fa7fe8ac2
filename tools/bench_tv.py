"""What the total-variation regulariser costs on the LLFF grid (the fused model's arena: 16 levels, resolutions 16 .. 4096,
6.3 M rows of four fp32 lanes, every level hashed):

    python tools/bench_tv.py [--reps R] [--windows W] [--n-samples N ...]

Per case the time of one TVRegulariser.add_grad() -- nsr_grid_tv and the counter's kernel, host wrapper included -- from HIP
events around a window of --reps back-to-back calls (the median of --windows windows, after a warm-up window; a window is
tens of milliseconds of device work, and every call draws afresh as in training), with the draws, the row reads (seven rows of
16 bytes per draw) and the atomic bytes the call makes and the rates they come to.  Cases:
    density      lambda_density only (two lanes written), the default n_samples (and every --n-samples given)
    both         both tables (four lanes written)
    value        density, through value(): the gradient-free fp64 pass with its ordered reduction
    all-sweep    levels 0-4 only, n_samples = V_4: every selected level enumerates its vertices, x fastest
A fine level has up to 4097^3 vertices, more than any n_samples, so no call sweeps all sixteen levels.
Compare with the training step of bench.py on the same box (ms_per_step of its JSON line)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=100, help='calls per timed window')
ap.add_argument('--windows', type=int, default=7)
ap.add_argument('--n-samples', type=int, nargs='*', default=[], help='further n_samples for the density case')
args = ap.parse_args()

import numpy as np
import torch
from nerfstyle_amd import _lib as L
from nerfstyle_amd.common import BBox
from nerfstyle_amd.config import NetworkConfig
from nerfstyle_amd.style_nerf import StyleTCNerf
from nerfstyle_amd.tv import DEFAULT_SAMPLES, TVRegulariser

dev = torch.device('cuda:0')
model = StyleTCNerf(NetworkConfig(), BBox.from_radius(2.0), 5, enc_dtype=None, use_dir=False).to(dev)
model._ensure_grad()
n_levels = len(model._offsets_np) - 1
res = (L.u32 * n_levels)()
L.check(L.lib().nsr_grid_resolutions(n_levels, model.S, int(model.cfg.pos_enc.min_res), res))
V = [(int(r) + 1) ** 3 for r in res]
print('grid: {} levels, resolutions {} .. {}, {} rows x 4 lanes ({:.1f} MB of fp32 masters)'.format(
    n_levels, int(res[0]), int(res[-1]), model.rows, model.table_elems * 4 / 1e6), flush=True)


def time_calls(fn):
    """median over the windows of (HIP-event time of --reps calls) / reps, in microseconds"""
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / args.reps)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def case(name, n_samples, lanes_written, fn, levels=None):
    lv = range(n_levels) if levels is None else levels
    draws = sum(min(n_samples, V[l]) for l in lv)
    swept = sum(1 for l in lv if n_samples >= V[l])
    med, lo, hi = time_calls(fn)
    read_b, atomic_b = draws * 7 * 16, draws * lanes_written * 4
    print('{:<10} n_samples {:>8}: {:>9.1f} us per call (windows {:.1f} .. {:.1f}), {} draws ({} of {} levels swept), '
          'row reads {:.1f} MB = {:.0f} GB/s, atomic adds {:.1f} MB = {:.0f} GB/s'.format(
              name, n_samples, med, lo, hi, draws, swept, len(lv), read_b / 1e6, read_b / med / 1e3, atomic_b / 1e6,
              atomic_b / med / 1e3 if lanes_written else 0.0), flush=True)


for n in [DEFAULT_SAMPLES] + list(args.n_samples):
    tv = TVRegulariser(model, lambda_density=1e-6, n_samples=n)
    case('density', n, 2, tv.add_grad)
tv = TVRegulariser(model, lambda_density=1e-6, lambda_color=1e-6, n_samples=DEFAULT_SAMPLES)
case('both', DEFAULT_SAMPLES, 4, tv.add_grad)
tv = TVRegulariser(model, lambda_density=1e-6, n_samples=DEFAULT_SAMPLES)
case('value', DEFAULT_SAMPLES, 0, tv.value)
coarse = [l for l in range(n_levels) if V[l] <= V[4]]
tv = TVRegulariser(model, lambda_density=1e-6, n_samples=V[4], levels=coarse)
case('all-sweep', V[4], 2, tv.add_grad, coarse)
