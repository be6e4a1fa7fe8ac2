"""The fused SSIM against the same number composed from torch ops, on one device in one process (HIP events, no renderer):

    python tools/bench_ssim.py [--reps R] [--h 756 --w 1008]

Four variants at one frame size (default 1008 x 756, the frame configs[1] trains on), each for padding 'same' and 'valid':
    fused value          nerfstyle_amd.ssim.ssim on the renderer's rows [H*W,3], no gradient wanted (two launches)
    fused value + grad   the same with the gradient towards the image (three launches; what a D-SSIM term costs)
    torch value          the composition a caller would write: permute to [1,3,H,W], five grouped 11x11 conv2d over x, y, xx, yy,
                         xy (as separable row and column passes, the cheaper form), the SSIM formula, mean
    torch value + grad   the same through autograd, the gradient brought back to [H*W,3]
Every variant is captured as one graph of INNER calls, so that the events see kernels and not the host preparing them; the
graphs are replayed in turn, --reps rounds, and the median per variant is reported in microseconds per call, with the spread
(min, max).  The torch composition runs in f32 like the kernel.  Prints one line per variant, the ratio, the share of a
31.6 ms training step, and the distance of the two implementations from each other."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=40)
ap.add_argument('--h', type=int, default=756)
ap.add_argument('--w', type=int, default=1008)
ap.add_argument('--step-ms', type=float, default=31.6, help='the bench.py training step the share is quoted against')
args = ap.parse_args()

import torch
import torch.nn.functional as F
from nerfstyle_amd import ssim as S

assert torch.cuda.is_available(), 'bench_ssim.py needs a HIP device'
dev = torch.device('cuda:0')
H, W = args.h, args.w
INNER = 10
C1, C2 = 0.01 ** 2, 0.03 ** 2

g = torch.Generator().manual_seed(1)
yy, xx = torch.meshgrid(torch.arange(H) / 97.0, torch.arange(W) / 97.0, indexing='ij')
base = torch.stack([0.45 + 0.25 * torch.sin(xx + c) * torch.cos(yy * (c + 1)) for c in range(3)], dim=-1)
target = (base + 0.1 * torch.rand(H, W, 3, generator=g)).reshape(-1, 3).to(dev)
image = (0.7 * base.flip(-1) + 0.3 * torch.rand(H, W, 3, generator=g)).reshape(-1, 3).to(dev)
win = S.window().to(dev)
WROW, WCOL = win.view(1, 1, 1, 11).expand(3, 1, 1, 11).contiguous(), win.view(1, 1, 11, 1).expand(3, 1, 11, 1).contiguous()


def blur(p, pad):
    return F.conv2d(F.conv2d(p, WROW, padding=(0, pad), groups=3), WCOL, padding=(pad, 0), groups=3)


def torch_ssim(rows, target_rows, padding):
    """what a caller writes today: rows [H*W,3] -> mean SSIM, f32"""
    pad = 5 if padding == 'same' else 0
    x = rows.view(H, W, 3).permute(2, 0, 1)[None]
    y = target_rows.view(H, W, 3).permute(2, 0, 1)[None]
    mx, my = blur(x, pad), blur(y, pad)
    sxx, syy, sxy = blur(x * x, pad) - mx * mx, blur(y * y, pad) - my * my, blur(x * y, pad) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return m.mean()


def variants(padding):
    leaf = image.clone().requires_grad_(True)
    leaf.grad = torch.zeros_like(leaf)

    def fused_value():
        return S.ssim(image, target, H, W, padding=padding)

    def fused_grad():
        S.ssim(leaf, target, H, W, padding=padding).backward()

    def torch_value():
        with torch.no_grad():
            return torch_ssim(image, target, padding)

    def torch_grad():
        torch_ssim(leaf, target, padding).backward()

    return {'fused value': fused_value, 'fused value + grad': fused_grad, 'torch value': torch_value, 'torch value + grad': torch_grad}


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(INNER):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def alternating(graphs):
    """microseconds per call of every graph: one replay of each in turn, --reps rounds -> {name: (median, min, max)}"""
    times = {k: [] for k in graphs}
    for _ in range(args.reps):
        for k, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / INNER)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


for padding in ('same', 'valid'):
    # the two implementations compute the same thing
    x1 = image.clone().requires_grad_(True)
    v1 = S.ssim(x1, target, H, W, padding=padding)
    v1.backward()
    x2 = image.clone().requires_grad_(True)
    v2 = torch_ssim(x2, target, padding)
    v2.backward()
    dv = abs(float(v1.detach()) - float(v2.detach()))
    dg = float((x1.grad - x2.grad).norm() / x1.grad.norm())
    fns = variants(padding)
    res = alternating({k: capture(fn) for k, fn in fns.items()})
    print('{}x{} padding={}: SSIM {:.6f}; fused vs torch f32: |dvalue| {:.2e}, gradient relative L2 {:.2e}'.format(
        W, H, padding, float(v1.detach()), dv, dg))
    for k, (med, lo, hi) in res.items():
        print('  {:20s} {:9.1f} us per call (min {:.1f}, max {:.1f}; {} rounds of {} calls)'.format(k, med, lo, hi, args.reps, INNER))
    for what in ('value', 'value + grad'):
        f, t = res['fused ' + what][0], res['torch ' + what][0]
        print('  {:20s} torch / fused = {:.2f}x; fused is {:.3f} % of a {:.1f} ms step'.format(what, t / f, 100.0 * f / (args.step_ms * 1e3),
                                                                                               args.step_ms))
