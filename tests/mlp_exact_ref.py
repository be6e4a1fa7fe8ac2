"""Operand-exact float64 restatement of the stand-alone MLP (nsr_mlp_forward / nsr_mlp_backward, csrc/mlp.hip).

The kernels round inputs, weights, hidden activations and masked hidden gradients to the compute type and accumulate
products in fp32 (MFMA, fp32 LDS atomics, fp32 global atomics).  With small integers everywhere, every product and every
partial sum is an integer below 2^24, so no rounding happens at all and the order of any summation is immaterial: the kernel
must give the bytes of this float64 computation cast to fp32.  `reference(check=True)` asserts that this holds for a case:

  * every value rounded to the compute type is an integer with |v| <= 2048 (f16, 11 significant bits) or <= 256 (bf16, 8);
  * every fp32 accumulation (each pre-activation, each gradient, each dparams element over all M samples) has
    sum |terms| < 2^24, so every partial sum in any order is an exactly representable integer;
  * each hidden layer has at least a quarter of its (sample, unit) entries active and at least a quarter inactive, so the
    ReLU and the gradient masks are exercised both ways.

Parameter layout: include/nsr.h (row-major [out, in] per layer, layers concatenated, last layer padded to 16 rows).
"""
import numpy as np

INT_MAX = {'f16': 2048, 'bf16': 256}
ACC_MAX = float(2 ** 24)
CHUNK = 1 << 16

# (compute type, n_in, hidden layers): the eight instantiations of mlp_dispatch
DISPATCH = [(dt, n_in, nh) for dt in ('f16', 'bf16') for n_in in (32, 16) for nh in (1, 2)]


def layer_shapes(n_in, nh):
    return [(64, n_in)] + [(64, 64)] * (nh - 1) + [(16, 64)]


def _pattern_matrix(rng, o, i, k):
    """{-1, 0, +1} matrix [o, i]: k signed patterns, each a random permutation laid over the longer side and wrapped over
    the shorter, so a row holds at most k * max(o, i) / o non-zeros and a column at most k * max(o, i) / i.  Random
    permutations and signs make it asymmetric: a transposed, shifted or row-swapped copy is a different matrix."""
    n = max(o, i)
    w = np.zeros((o, i), np.float64)
    for _ in range(k):
        perm = rng.permutation(n)
        sign = rng.integers(0, 2, n) * 2 - 1
        w[np.arange(n) % o, perm % i] = sign
    return w


def make_weights(seed, n_in, nh, n_out, pad_value=0.0):
    """Flat fp32 parameters.  Rows n_out..15 of the last layer hold pad_value (their outputs are discarded)."""
    rng = np.random.default_rng(seed)
    ws = []
    for li, (o, i) in enumerate(layer_shapes(n_in, nh)):
        last = li == nh
        w = _pattern_matrix(rng, o, i, 2 if last else 3)
        if last:
            w[n_out:] = pad_value
        ws.append(w)
    return np.concatenate([w.reshape(-1) for w in ws]).astype(np.float32)


def split(params, n_in, nh):
    out, p = [], 0
    for (o, i) in layer_shapes(n_in, nh):
        out.append(np.asarray(params[p:p + o * i], np.float64).reshape(o, i))
        p += o * i
    assert p == len(params)
    return out


def make_inputs(seed, M, n_in, n_out, x_max=2, dy_rows=None):
    """x [M, n_in] integers in [-x_max, x_max], dy [M, n_out] integers in [-2, 2]; dy_rows (bool [M]) zeroes the others."""
    rng = np.random.default_rng(seed + 1000003)
    x = rng.integers(-x_max, x_max + 1, (M, n_in)).astype(np.float32)
    dy = rng.integers(-2, 3, (M, n_out)).astype(np.float32)
    if dy_rows is not None:
        dy[~dy_rows] = 0
    return x, dy


class Case:
    def __init__(self, dt, n_in, nh, n_out, M, seed, act='none', large=False):
        self.dt, self.n_in, self.nh, self.n_out, self.M, self.seed, self.act, self.large = dt, n_in, nh, n_out, M, seed, act, large

    @property
    def id(self):
        return '%s-in%d-h%d-out%d-M%d%s' % (self.dt, self.n_in, self.nh, self.n_out, self.M, '-sig' if self.act != 'none' else '')

    def weights(self, pad_value=0.0):
        return make_weights(self.seed, self.n_in, self.nh, self.n_out, pad_value)

    def inputs(self):
        if not self.large:
            return make_inputs(self.seed, self.M, self.n_in, self.n_out)
        # the workgroup cap: inputs in {-1, 0, 1}, dy on about one row in 64 and on the rows of the last tile
        rng = np.random.default_rng(self.seed + 7)
        rows = rng.random(self.M) < 1.0 / 64
        rows[(self.M - 1) // 16 * 16:] = True
        return make_inputs(self.seed, self.M, self.n_in, self.n_out, x_max=1, dy_rows=rows)


M_EDGES = [1, 15, 16, 17, 63, 64, 65, 513, 16 * 128 + 1]
N_OUTS = [1, 3, 5, 16]
M_LARGE = 16 * 65536 + 17


def exact_cases():
    """Every dispatch case meets every M and every n_out at least once: M runs over all nine edges for each dispatch case,
    n_out cycles with a stride that pairs each (n_in, hidden) with all four widths."""
    cases = []
    for d, (dt, n_in, nh) in enumerate(DISPATCH):
        for j, M in enumerate(M_EDGES):
            cases.append(Case(dt, n_in, nh, N_OUTS[(j + d) % 4], M, seed=100 * d + j))
    return cases


def large_cases():
    return [Case('f16', 32, 2, 5, M_LARGE, seed=901, large=True), Case('bf16', 16, 1, 3, M_LARGE, seed=902, large=True)]


def sigmoid_cases():
    return [Case('f16', 32, 1, 3, 65, seed=801, act='sigmoid'), Case('bf16', 16, 2, 16, 513, seed=802, act='sigmoid')]


def module_cases():
    return [Case('f16', 16, 1, 5, 513, seed=77), Case('bf16', 32, 2, 5, 513, seed=78)]


def reference(params, x, dy, n_in, nh, n_out, dt=None, check=False):
    """float64 forward and backward with out_act = None.  Returns dict(o, dx, dparams) in float64 (o: the pre-activation,
    which is y).  check=True (dt given) also asserts the exactness conditions and returns the ReLU shares.  Works through
    the samples in chunks, so the large cases need no [M, 64] float64 arrays."""
    ws = split(params, n_in, nh)
    wo = ws[-1][:n_out]
    M = x.shape[0]
    o = np.empty((M, n_out), np.float64)
    dx = np.empty((M, n_in), np.float64)
    dws = [np.zeros_like(w) for w in ws]
    dws_abs = [np.zeros_like(w) for w in ws]
    active = np.zeros(nh)
    lim = INT_MAX[dt] if check else None

    def is_small_int(a, what):
        assert np.all(a == np.rint(a)) and np.abs(a).max(initial=0) <= lim, what

    def acc_ok(a, b, what):
        """sum |a_k| |b_k| over the contraction < 2^24 for every output element of a @ b"""
        assert (np.abs(a) @ np.abs(b)).max(initial=0) < ACC_MAX, what

    if check:
        for li, w in enumerate(ws):
            is_small_int(w, 'weights %d' % li)
    for s in range(0, M, CHUNK):
        xs, dys = x[s:s + CHUNK].astype(np.float64), dy[s:s + CHUNK].astype(np.float64)
        acts = [xs]
        for li in range(nh):
            z = acts[-1] @ ws[li].T
            if check:
                acc_ok(acts[-1], ws[li].T, 'pre-activation %d' % li)
                active[li] += float((z > 0).sum())
            acts.append(np.maximum(z, 0.0))
        o[s:s + CHUNK] = acts[-1] @ wo.T
        g = dys
        if check:
            is_small_int(xs, 'x')
            is_small_int(dys, 'dy')
            for li in range(nh):
                is_small_int(acts[li + 1], 'hidden activation %d' % li)
            acc_ok(acts[-1], wo.T, 'output')
        for li in range(nh, -1, -1):
            w = wo if li == nh else ws[li]
            dw = g.T @ acts[li]
            dws[li][:dw.shape[0]] += dw
            dws_abs[li][:dw.shape[0]] += np.abs(g).T @ np.abs(acts[li])
            if check:
                acc_ok(g, w, 'gradient into layer %d' % li)
            g = g @ w
            if li > 0:
                g = g * (acts[li] > 0)
                if check:
                    is_small_int(g, 'masked hidden gradient %d' % li)
        dx[s:s + CHUNK] = g
    out = {'o': o + 0.0, 'dx': dx + 0.0, 'dparams': np.concatenate([d.reshape(-1) for d in dws]) + 0.0}
    if check:
        worst = max(float(d.max()) for d in dws_abs)
        assert worst < ACC_MAX, ('dparams', worst)
        share = active / (64.0 * M)
        assert np.all(share >= 0.25) and np.all(share <= 0.75), ('ReLU shares', share)
        out['relu_share'], out['dparams_abs_max'] = share, worst
    return out


def f32_bytes(a):
    """fp64 -> fp32 -> the 32-bit patterns; the values are exact integers, so the cast rounds nothing"""
    a32 = np.ascontiguousarray(a, np.float32)
    assert np.array_equal(a32.astype(np.float64), np.asarray(a, np.float64))
    return a32.view(np.uint32)


def sigmoid_bar(o):
    """The bar of the sigmoid comparison and its two ingredients: 4 x the max abs error of the same fp32 expression
    1 / (1 + exp(-o)) evaluated by torch on the CPU against float64, and 2^-23 (half an fp32 ulp of values in [0.5, 1))."""
    import torch
    t = torch.tensor(np.asarray(o, np.float32))
    y32 = (1.0 / (1.0 + torch.exp(-t))).numpy().astype(np.float64)
    y64 = 1.0 / (1.0 + np.exp(-np.asarray(o, np.float64)))
    e32 = float(np.abs(y32 - y64).max())
    return max(4.0 * e32, 2.0 ** -23), e32, y64
