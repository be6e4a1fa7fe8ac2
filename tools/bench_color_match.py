"""Cost of the colour transfer's two passes (nsr_color_moments, nsr_color_apply) on a full-size resident training set,
F = 35 frames of 1008x756, synthetic values, against the same work written in torch on the device as the reference formulates
it (utils/__init__.py:262-295: mean, centred matmul; rows[:, :3] @ A.T + b, clamp, copy back).

  python tools/bench_color_match.py                 C = 4 (targets with a segment channel) and C = 3
  python tools/bench_color_match.py --channels 4 --repeats 30 --inner 10

Every figure is a median over `repeats` windows of `inner` back-to-back calls timed by device events, after a warm-up; the HIP and
the torch windows alternate in the same process.  Bytes are counted from the shapes: the moments read n * C * 4 bytes, the map
reads and writes them.  Shares are of the 6.3 TB/s a streaming kernel reaches on an MI355X (peak 8 TB/s).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ACHIEVABLE_BPS, PEAK_BPS = 6.3e12, 8.0e12


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, warmup, repeats, inner):
    """{name: median ms per call}; the windows of the candidates alternate, the order flips every repeat"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    names = list(fns)
    for r in range(repeats):
        for k in (names if r % 2 == 0 else names[::-1]):
            times[k].append(window_ms(fns[k], inner))
    return {k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def run(dev, F, HW, C, args):
    from nerfstyle_amd import _lib as L
    from nerfstyle_amd import color_match as CM
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    targets = torch.rand(F, HW, C, device=dev, generator=g)
    style = torch.rand(512 * 512, 3, device=dev, generator=g) * 0.5 + 0.25
    n = F * HW
    nbytes = n * C * 4
    tf = CM.solve_color_transform(CM.color_moments(targets), n, CM.color_moments(style), style.shape[0])
    A, b = tf[:3, :3].contiguous(), tf[:3, 3].contiguous()
    moments = torch.empty(9, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib().nsr_color_moments_workspace_bytes(n)) // 8, dtype=torch.float64, device=dev)
    lib, stream = L.lib(), L.stream()
    pt, pm, pw, ptf = L.p(targets), L.p(moments), L.p(ws), L.p(tf)
    rows = targets.view(-1, C)

    def hip_moments():
        lib.nsr_color_moments(pt, n, C, pm, pw, stream)

    def torch_moments():
        x = rows[:, :3]
        mu = x.mean(0, keepdim=True)
        d = x - mu
        return mu, torch.matmul(d.transpose(1, 0), d) / float(n)

    def hip_apply():
        lib.nsr_color_apply(pt, pt, n, C, ptf, 1, stream)

    def torch_apply():
        y = rows[:, :3] @ A.T + b.view(1, 3)
        rows[:, :3].copy_(y.clamp_(0.0, 1.0))

    med_m, span_m = alternate({'hip': hip_moments, 'torch': torch_moments}, args.warmup, args.repeats, args.inner)
    med_a, span_a = alternate({'hip': hip_apply, 'torch': torch_apply}, args.warmup, args.repeats, args.inner)
    L.check(lib.nsr_color_moments(pt, n, C, pm, pw, stream), 'color_moments')
    torch.cuda.synchronize()

    def entry(ms, span, traffic):
        bps = traffic / (ms * 1e-3)
        return {'ms': round(ms, 4), 'ms_min_max': [round(span[0], 4), round(span[1], 4)], 'TBps': round(bps / 1e12, 3),
                'share_of_6.3TBps': round(bps / ACHIEVABLE_BPS, 3), 'share_of_8TBps_peak': round(bps / PEAK_BPS, 3)}

    return {'rows': n, 'bytes': nbytes,
            'moments_hip': entry(med_m['hip'], span_m['hip'], nbytes), 'moments_torch': entry(med_m['torch'], span_m['torch'], nbytes),
            'apply_hip': entry(med_a['hip'], span_a['hip'], 2 * nbytes), 'apply_torch': entry(med_a['torch'], span_a['torch'], 2 * nbytes),
            'moments_torch_over_hip': round(med_m['torch'] / med_m['hip'], 2), 'apply_torch_over_hip': round(med_a['torch'] / med_a['hip'], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, nargs='*', default=[4, 3])
    ap.add_argument('--frames', type=int, default=35)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=20, help='timed windows per candidate, alternating')
    ap.add_argument('--inner', type=int, default=10, help='back-to-back calls per window')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {'F': args.frames, 'H': 756, 'W': 1008}
    for C in args.channels:
        out['C%d' % C] = run(dev, args.frames, 1008 * 756, C, args)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
