"""Cost of the matting-Laplacian photorealism term (nsr_matting_laplacian) at 1008x756.

  python tools/bench_matting.py               kernel: ms per call (value + gradient; value only) for win_rad 1 and 2, by device
                                              events over back-to-back launches; then the stylisation iteration of
                                              `bench.py --stage style` (resident back-propagation, f16, autocast loss) with
                                              StyleCriterion(photo_lambda=1e-4) against photo_lambda=0, in alternating blocks
  python tools/bench_matting.py --kernel-only --iters 20
                                              only the launches (for `rocprofv3 --kernel-trace --stats -- python ...`)

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def kernel_ms(dev, H, W, r, iters, with_grad):
    from nerfstyle_amd import _lib as L
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    t = torch.rand(3, H, W, device=dev, generator=g)
    v = torch.rand(3, H, W, device=dev, generator=g)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    grad = torch.empty(3, H, W, device=dev) if with_grad else None
    ws = torch.empty(int(L.lib().nsr_matting_laplacian_workspace_bytes(H, W, r)) // 8, dtype=torch.float64, device=dev)
    args = (L.p(t), L.p(v), H, W, r, 1e-7, L.p(loss), L.p(grad), L.p(ws), L.stream())
    for _ in range(3):
        L.check(L.lib().nsr_matting_laplacian(*args), 'matting_laplacian')
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.lib().nsr_matting_laplacian(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def style_iteration_ms(dev, steps, blocks):
    import bench
    from nerfstyle_amd.losses import SemanticStyleLoss
    from nerfstyle_amd.optim import FusedAdam, LossScaler
    from nerfstyle_amd.stylize import StyleCriterion, resident_backprop_step
    from nerfstyle_amd.vgg import VGG16FeatureExtractor
    a = argparse.Namespace(num_classes=5, table_dtype='f16', compute_dtype='f16', scene='room', res_scale=2, max_steps=512,
                           samples_cap=160, seed=69420, no_occ_update=True, sort_samples='auto', occ_phase='steady')
    model, r, _, poses, intr = bench.build(a, dev, 0)
    W, H = intr.size()
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    style = torch.rand(3, H, W, device=dev, generator=g)
    seg = torch.randint(0, a.num_classes, (H, W), device=dev, generator=g)
    target = torch.rand(3, H, W, device=dev, generator=g)
    fx = VGG16FeatureExtractor(['relu3']).to(dev)
    crits = {}
    for lam in (0.0, 1e-4):
        crits[lam] = StyleCriterion(fx, SemanticStyleLoss(['relu3'], clusters=seg), content_lambda=0.001, style_lambda=1.0,
                                    amp_dtype=torch.float16, photo_lambda=lam)
        crits[lam].init_style(style, num_classes=a.num_classes)
    opt = FusedAdam(model, lr=0.1, keywords=['x_color_embedder'])
    scaler = LossScaler(init_scale=65536.0)
    scale = scaler.scale_tensor(dev)

    def step(lam, it):
        frame = (it * 7) % poses.shape[0]
        resident_backprop_step(r, poses[frame], lambda rgb, cls: crits[lam](rgb, target, cls, frame_key=frame, it=it)[0],
                               loss_scale=scale, optimizer=opt, with_classes=True)
        opt.step(scaler=scaler)

    it = 0
    for lam in (0.0, 1e-4):
        for _ in range(3):
            step(lam, it)
            it += 1
    times = {0.0: [], 1e-4: []}
    for b in range(blocks):
        for lam in ((0.0, 1e-4) if b % 2 == 0 else (1e-4, 0.0)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(lam, it)
                it += 1
            torch.cuda.synchronize()
            times[lam].append((time.perf_counter() - t0) * 1e3 / steps)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=10, help='style iterations per timed block')
    ap.add_argument('--blocks', type=int, default=6, help='timed blocks per photo_lambda, alternating')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    H, W = 756, 1008
    out = {'H': H, 'W': W}
    for r in (1, 2):
        out['kernel_ms_r%d' % r] = round(kernel_ms(dev, H, W, r, args.iters, True), 4)
        out['kernel_ms_r%d_value_only' % r] = round(kernel_ms(dev, H, W, r, args.iters, False), 4)
    if not args.kernel_only:
        times = style_iteration_ms(dev, args.steps, args.blocks)
        m0, m1 = statistics.median(times[0.0]), statistics.median(times[1e-4])
        out.update({'style_ms_photo0': round(m0, 3), 'style_ms_photo1e-4': round(m1, 3),
                    'style_overhead_pct': round(100 * (m1 / m0 - 1), 2),
                    'style_ms_blocks': {str(k): [round(x, 3) for x in v] for k, v in times.items()}})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
