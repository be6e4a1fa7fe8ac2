"""References for the per-ray geometry terms (nsr_ray_geometry_forward / _backward, raymarching.ray_geometry).

geometry_torch: a torch fp64 restatement of the definitions -- one plain loop over the rays, the pair term of the distortion
as the O(n^2) double sum it is defined as, gradients by autograd.
closed_form:    a NumPy evaluation of the formula the kernel implements (prefix sums for the pair term, per-ray totals minus
prefixes for the sums over the samples behind one), sample by sample in the serial order, in the dtype asked for: float64 pins
the formula against autograd, float32 shows what the number format alone costs (no scan reassociation)."""
import numpy as np
import torch


def _range_ok(R):
    return bool(R > 0) and bool(np.isfinite(R))


def geometry_torch(sigmas, deltas, rays, nears, fars, T_thresh, is_ndc=False):
    """sigmas: float64 tensor [M] (requires_grad for gradients); the rest NumPy -> (depth [N], distortion [N]) float64 tensors"""
    col = 2 if is_ndc else 0
    M, N = sigmas.shape[0], len(rays)
    dl = torch.as_tensor(np.asarray(deltas, np.float64))
    depth, dist = [None] * N, [None] * N
    zero = sigmas.new_zeros(())
    for index, offset, steps in np.asarray(rays, np.int64):
        near, R = float(nears[index]), float(np.float64(fars[index]) - np.float64(nears[index]))
        depth[index] = dist[index] = zero
        if steps == 0 or offset + steps >= M or not _range_ok(R):
            continue
        sg = sigmas[offset:offset + steps]
        delta, tau = dl[offset:offset + steps, col], dl[offset:offset + steps, col + 1]
        alpha = 1.0 - torch.exp(-sg * delta)
        T = torch.cat([sg.new_ones(1), torch.cumprod(1.0 - alpha, 0)[:-1]])
        live = T.detach() >= T_thresh                     # the live set is held constant
        live[0] = True
        w = torch.where(live, alpha * T, torch.zeros_like(T))
        t = torch.cumsum(tau, 0)
        d = (w * t).sum()
        pair = (w[:, None] * w[None, :] * (t[:, None] - t[None, :]).abs()).sum()
        depth[index] = torch.clamp(d - near, min=0.0) / R
        dist[index] = (pair + (w * w * delta).sum() / 3.0) / R
    return torch.stack(depth), torch.stack(dist)


def closed_form(sigmas, deltas, rays, nears, fars, T_thresh, is_ndc=False, g_depth=None, g_dist=None, dtype=np.float64):
    """-> (depth [N], distortion [N], grad_sigmas [M]) in `dtype`, every operation rounded to it, samples in serial order.
    grad_sigmas is zero outside the live samples of valid rays."""
    f = dtype
    col = 2 if is_ndc else 0
    sg_all, dl = np.asarray(sigmas).astype(f), np.asarray(deltas).astype(f)
    M, N = len(sg_all), len(rays)
    depth, dist, grad = np.zeros(N, f), np.zeros(N, f), np.zeros(M, f)
    two, three, thr = f(2), f(3), f(T_thresh)
    for index, offset, steps in np.asarray(rays, np.int64):
        near = f(nears[index])
        R = f(fars[index]) - near
        if steps == 0 or offset + steps >= M or not _range_ok(R):
            continue
        # forward: weights, prefixes, totals
        T, t, W, S, P, Q = f(1), f(0), f(0), f(0), f(0), f(0)
        rec = []
        for i in range(steps):
            p = offset + i
            delta = dl[p, col]
            om = np.exp(-sg_all[p] * delta).astype(f)
            alpha = f(1) - om
            t = t + dl[p, col + 1]
            if not (i == 0 or T >= thr):
                break
            w = alpha * T
            rec.append((p, delta, om, T, t, w, W, S))      # W, S: over the samples in front
            P = P + w * (t * W - S)
            Q = Q + w * w * delta
            W, S = W + w, S + w * t
            T = T * (f(1) - alpha)
        num = two * P + Q / three
        depth[index] = max(S - near, f(0)) / R
        dist[index] = num / R
        gd = f(0) if g_depth is None else f(g_depth[index])
        gx = f(0) if g_dist is None else f(g_dist[index])
        cD = gd / R if S > near else f(0)
        cX = gx / R
        Ft = cD * S + cX * (two * num)                     # sum_k f_k w_k: cD d + the degree-2 homogeneity of the numerator
        F = f(0)
        for p, delta, om, Tb, tk, w, Wex, Sex in rec:
            Win, Sin = Wex + w, Sex + w * tk
            A = (tk * Wex - Sex) + ((S - Sin) - tk * (W - Win))
            fk = cD * tk + cX * (two * A + (two / three) * (w * delta))
            F = F + fk * w
            grad[p] = delta * (fk * (Tb * om) - (Ft - F))
    return depth, dist, grad


# ---- the shared test case: helpers.edge_rays with a range per ray ----------------------------------------------------
NEAR, FAR = 0.2, 2.2
UPSTREAM = ('depth', 'dist', 'both')
_cases = {}


def geometry_case(is_ndc, replicas=4):
    """helpers.edge_rays(3, is_ndc) with nears = 0.2 and fars = 2.2, one long unstopped ray given near == far == FLT_MAX, seeded
    uniform upstream gradients, and the fp64 results: depth, dist, grads[k] for k in UPSTREAM (G_depth only, G_dist only, both).
    Computed once per key; the arrays are read-only."""
    from helpers import EDGE_T_THRESH, edge_rays, owned_slots
    key = (bool(is_ndc), replicas)
    if key in _cases:
        return _cases[key]
    sig, _, deltas, rays, M, stop = edge_rays(3, is_ndc, replicas=replicas)
    N = len(rays)
    nears, fars = np.full(N, NEAR, np.float32), np.full(N, FAR, np.float32)
    miss = int(np.nonzero((rays[:, 2] == 200) & (stop == 200))[0][0])          # row of a ray that misses the box
    nears[rays[miss, 0]] = fars[rays[miss, 0]] = np.finfo(np.float32).max
    rng = np.random.default_rng(7)
    g_depth, g_dist = rng.random(N).astype(np.float32), rng.random(N).astype(np.float32)
    s64 = torch.tensor(sig.astype(np.float64), requires_grad=True)
    depth, dist = geometry_torch(s64, deltas, rays, nears, fars, EDGE_T_THRESH, is_ndc)
    gd, gx = torch.tensor(g_depth.astype(np.float64)), torch.tensor(g_dist.astype(np.float64))
    grads = {}
    for k, loss in (('depth', (depth * gd).sum()), ('dist', (dist * gx).sum()), ('both', (depth * gd).sum() + (dist * gx).sum())):
        grads[k] = torch.autograd.grad(loss, s64, retain_graph=True)[0].numpy()
    valid = np.zeros(N, bool)                                                   # by ray index: kept, not empty, with a range
    for n, (index, offset, steps) in enumerate(rays):
        valid[index] = steps != 0 and offset + steps < M and n != miss
    case = dict(sig=sig, deltas=deltas, rays=rays, M=M, N=N, stop=stop, nears=nears, fars=fars, g_depth=g_depth, g_dist=g_dist,
                depth=depth.detach().numpy(), dist=dist.detach().numpy(), grads=grads, valid=valid, miss=miss,
                owned=owned_slots(rays, M), T_thresh=EDGE_T_THRESH, is_ndc=bool(is_ndc))
    for v in list(case.values()) + list(grads.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cases[key] = case
    return case


def upstream(case, which):
    """(g_depth | None, g_dist | None) of UPSTREAM entry `which`"""
    return (case['g_depth'] if which in ('depth', 'both') else None, case['g_dist'] if which in ('dist', 'both') else None)
