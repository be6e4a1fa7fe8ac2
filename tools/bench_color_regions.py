"""Cost of the region-wise colour transfer's two passes (nsr_color_region_moments, nsr_color_region_apply) on a full-size resident
training set, F = 35 frames of 1008x756 with a segment channel, K = 5, synthetic values, on two kinds of label map:
  blocky   rectangles of 64x48 pixels (3072 pixels each), one class per rectangle: what a segmentation looks like to a wave
  random   a fresh class per pixel: every wave holds all K regions in every slot, the worst case of the per-region loop
against (same rows, same session, alternating windows)
  global   nsr_color_moments / nsr_color_apply, the one-transform passes
  torch    the same result composed from torch: K + 1 masked fp64 sums, K + 1 masked affine maps

  python tools/bench_color_regions.py
  python tools/bench_color_regions.py --regions 5 --repeats 20 --inner 5

Every figure is a median over `repeats` windows of `inner` back-to-back calls timed by device events, after a warm-up.  Bytes
are counted from the shapes: the moments read n * 16 bytes, the map reads and writes them.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_color_match import alternate  # noqa: E402


def label_maps(kind, F, H, W, K, dev, g):
    if kind == 'random':
        return torch.randint(0, K, (F, H * W), device=dev, generator=g).float()
    by, bx = (H + 47) // 48, (W + 63) // 64
    blocks = torch.randint(0, K, (F, by, bx), device=dev, generator=g).float()
    return blocks.repeat_interleave(48, 1).repeat_interleave(64, 2)[:, :H, :W].reshape(F, H * W)


def run(dev, kind, F, H, W, K, args):
    from nerfstyle_amd import _lib as L
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = F * H * W
    targets = torch.rand(F, H * W, 4, device=dev, generator=g)
    targets[:, :, 3] = label_maps(kind, F, H, W, K, dev, g)
    rows = targets.view(-1, 4)
    tfs = torch.eye(4, device=dev).repeat(K + 1, 1, 1)
    tfs[:, :3, :3] += 0.05 * torch.randn(K + 1, 3, 3, device=dev, generator=g)
    tfs[:, :3, 3] = 0.02 * torch.randn(K + 1, 3, device=dev, generator=g)
    tf = tfs[K].contiguous()
    lib, stream = L.lib(), L.stream()
    moments = torch.empty(K + 1, 10, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.nsr_color_region_moments_workspace_bytes(n, K)) // 8, dtype=torch.float64, device=dev)
    gm = torch.empty(9, dtype=torch.float64, device=dev)
    gws = torch.empty(int(lib.nsr_color_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    pt, pm, pw, ptfs, pg, pgw, ptf = L.p(targets), L.p(moments), L.p(ws), L.p(tfs), L.p(gm), L.p(gws), L.p(tf)

    def region_moments():
        lib.nsr_color_region_moments(pt, n, 4, None, K, pm, pw, stream)

    def global_moments():
        lib.nsr_color_moments(pt, n, 4, pg, pgw, stream)

    def torch_moments():
        x = rows[:, :3].double()
        second = torch.cat([x[:, :1] * x, x[:, 1:2] * x[:, 1:], x[:, 2:] * x[:, 2:]], 1)
        out = []
        for k in range(K + 1):
            m = (rows[:, 3] == k) if k < K else ~((rows[:, 3] >= 0) & (rows[:, 3] < K))
            md = m.double().unsqueeze(1)
            out.append(torch.cat([md.sum(0), (x * md).sum(0), (second * md).sum(0)]))
        return torch.stack(out)

    def region_apply():
        lib.nsr_color_region_apply(pt, pt, n, 4, None, K, ptfs, 1, stream)

    def global_apply():
        lib.nsr_color_apply(pt, pt, n, 4, ptf, 1, stream)

    def torch_apply():
        x = rows[:, :3]
        y = x.clone()
        for k in range(K + 1):
            m = (rows[:, 3] == k) if k < K else ~((rows[:, 3] >= 0) & (rows[:, 3] < K))
            y = torch.where(m.unsqueeze(1), x @ tfs[k, :3, :3].T + tfs[k, :3, 3].view(1, 3), y)
        rows[:, :3].copy_(y.clamp_(0.0, 1.0))

    L.check(lib.nsr_color_region_moments(pt, n, 4, None, K, pm, pw, stream), 'color_region_moments')
    L.check(lib.nsr_color_region_apply(pt, pt, n, 4, None, K, ptfs, 1, stream), 'color_region_apply')
    torch.cuda.synchronize()
    med_m, span_m = alternate({'region': region_moments, 'global': global_moments}, args.warmup, args.repeats, args.inner)
    med_a, span_a = alternate({'region': region_apply, 'global': global_apply}, args.warmup, args.repeats, args.inner)
    med_t, span_t = alternate({'moments_torch': torch_moments, 'apply_torch': torch_apply}, 1, args.torch_repeats, 1)
    nbytes = n * 16

    def entry(ms, span, traffic):
        return {'ms': round(ms, 4), 'ms_min_max': [round(span[0], 4), round(span[1], 4)], 'TBps': round(traffic / (ms * 1e-3) / 1e12, 3)}

    return {'moments_region': entry(med_m['region'], span_m['region'], nbytes), 'moments_global': entry(med_m['global'], span_m['global'], nbytes),
            'moments_torch': entry(med_t['moments_torch'], span_t['moments_torch'], nbytes),
            'apply_region': entry(med_a['region'], span_a['region'], 2 * nbytes), 'apply_global': entry(med_a['global'], span_a['global'], 2 * nbytes),
            'apply_torch': entry(med_t['apply_torch'], span_t['apply_torch'], 2 * nbytes),
            'moments_region_over_global': round(med_m['region'] / med_m['global'], 2),
            'apply_region_over_global': round(med_a['region'] / med_a['global'], 2),
            'moments_torch_over_region': round(med_t['moments_torch'] / med_m['region'], 1),
            'apply_torch_over_region': round(med_t['apply_torch'] / med_a['region'], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=35)
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=15, help='timed windows per candidate, alternating')
    ap.add_argument('--inner', type=int, default=5, help='back-to-back calls per window')
    ap.add_argument('--torch-repeats', type=int, default=3, help='timed single calls of the torch compositions')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'F': args.frames, 'H': 756, 'W': 1008, 'K': args.regions, 'rows': args.frames * 756 * 1008}
    for kind in ('blocky', 'random'):
        out[kind] = run(dev, kind, args.frames, 756, 1008, args.regions, args)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
