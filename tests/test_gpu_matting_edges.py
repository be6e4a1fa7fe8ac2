"""GPU: nsr_matting_laplacian (csrc/matting.hip: k_matting<1>, k_matting<2>, k_matting_final) through the C ABI at its tile,
halo and grid edges.  Shapes, inputs and fp64 references come from matting_cases.py.

Harness.  grad_v, the workspace (exactly nsr_matting_laplacian_workspace_bytes long) and loss_out each lie at a 256-byte
aligned address between two guard bands of GUARD bytes of 0xA5; grad_v is pre-filled with NaN, loss_out and the workspace
with sentinels.  After every call the guards must be intact; after a successful one no NaN is left in grad_v, after a
refused one every output still holds its fill.

Bars.  The value: relative 1e-9, VALUE_TOL of test_gpu_matting.py.  The gradient, per element:
    |got - ref| <= 2^-23 |ref| + ADD max|ref|
2^-23 |ref| is one rounding of an fp64 result to fp32 (2^-24) with a factor 2 of slack; ADD covers the evaluation-order
difference between two fp64 computations of the same sums and comes from the two CPU restatements alone
(test_matting_cpu.py::test_edge_shapes_dense_and_vectorised_restatements_agree prints it for every case):
  * edge shapes, r = 1 and 2, 24 shapes each: matting_dense and matting_fast differ by at most 1.03e-15 max|grad| per
    element (3.7e-16 .. 1.03e-15) and by at most 1.63e-14 relative in the value.  1.03e-15 is far below a quarter of 1e-9,
    so ADD = 1e-9 as the issue sets it.
  * the conditioned seam case, (17, 65), a step of 0.5 on the x = 32 seam plus 1e-3 noise: the two restatements differ by
    4.64e-11 max|grad| (r = 1) and 1.98e-11 max|grad| (r = 2); ADD is four times that, 1.86e-10 and 7.9e-11
    (matting_cases.COND_FLOOR).  Both are far below 1e-5, so the noise stays at 1e-3.
    With raw window moments the kernel missed this bar at r = 1 (one element 1.67 times over it, 3.0e-10 max|grad|);
    with the moments taken about the window's centre pixel it is at 0.48 of the bar, the fp32 rounding alone.
  * the grid cap, r = 1, H = 65535 * 8, W = 3: matting_fast alone takes about a second on the host, so the numbers are
    compared at that H with the bars of the edge shapes.

What each group would catch: a halo origin off by one, (a) and (c); `cx < W - R` as `<=`, (a) at W = 32+r+1; the value
gate dropped, the value doubles at seams in (a); an n_p clamp wrong at a border, (c); s_cf read on the NULL path, (d); a
final sum that stops at 256 partials, (e)."""
import numpy as np
import pytest
import torch

import matting_cases as C
from matting_ref import matting_fast, rel_err

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-9                          # relative; the bar of test_gpu_matting.py
ADD = 1e-9                                # see the docstring
GUARD = 4096
PATTERN = 0xA5
LOSS_FILL, WS_FILL = -7.25, -3.5
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2


class Guarded:
    """`nbytes` device bytes at a 256-byte aligned address between two guard bands"""

    def __init__(self, nbytes, dev, dtype, fill):
        self.buf = torch.full((nbytes + 2 * GUARD + 256,), PATTERN, dtype=torch.uint8, device=dev)
        self.off = ((self.buf.data_ptr() + GUARD + 255) & ~255) - self.buf.data_ptr()
        self.nbytes = nbytes
        self.t = self.buf[self.off:self.off + nbytes].view(dtype)
        self.fill = fill
        self.refill()

    def refill(self):
        self.t.fill_(self.fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.off] == PATTERN).all()) and bool((self.buf[self.off + self.nbytes:] == PATTERN).all())

    def untouched(self):
        if self.fill != self.fill:
            return bool(torch.isnan(self.t).all())
        return bool((self.t == self.fill).all())


class Call:
    """One image's buffers around nsr_matting_laplacian"""

    def __init__(self, dev, H, W, r):
        from nerfstyle_amd import _lib as L
        self.L, self.H, self.W, self.r = L, H, W, r
        self.ws_bytes = int(L.lib().nsr_matting_laplacian_workspace_bytes(H, W, r))
        assert self.ws_bytes == ((W + C.TX - 1) // C.TX) * ((H + C.TY - 1) // C.TY) * 8
        self.grad = Guarded(3 * H * W * 4, dev, torch.float32, float('nan'))
        self.ws = Guarded(self.ws_bytes, dev, torch.float64, WS_FILL)
        self.loss = Guarded(8, dev, torch.float64, LOSS_FILL)
        self.dev = dev

    def __call__(self, t, v, with_grad=True, eps=C.EPS, r=None, H=None, W=None, ws_offset=0, null=()):
        """-> status.  `null` names the pointers passed as NULL."""
        tt = t if torch.is_tensor(t) else torch.tensor(np.ascontiguousarray(t), device=self.dev)
        vt = v if torch.is_tensor(v) else torch.tensor(np.ascontiguousarray(v), device=self.dev)
        for g in (self.grad, self.ws, self.loss):
            g.refill()
        status = self.L.lib().nsr_matting_laplacian(
            None if 'target' in null else tt.data_ptr(), None if 'v' in null else vt.data_ptr(),
            self.H if H is None else H, self.W if W is None else W, self.r if r is None else r, eps,
            None if 'loss' in null else self.loss.ptr, self.grad.ptr if with_grad else None,
            None if 'workspace' in null else self.ws.ptr + ws_offset, self.L.stream())
        torch.cuda.synchronize()
        assert self.grad.guards_intact() and self.ws.guards_intact() and self.loss.guards_intact(), 'write into a guard band'
        return status

    def outputs_untouched(self):
        return self.grad.untouched() and self.ws.untouched() and self.loss.untouched()

    def value(self):
        return float(self.loss.t[0])

    def gradient(self):
        g = self.grad.t.view(3, self.H, self.W).cpu().numpy()
        assert not np.isnan(g).any(), 'a gradient element was not written'
        return g


def check_value(got, ref, what):
    e = rel_err(got, ref)
    print('{}: value rel err {:.3e}'.format(what, e))
    assert e <= VALUE_TOL, (what, got, ref)


def check_grad(got, ref, add, what):
    err = np.abs(got.astype(np.float64) - ref)
    bar = 2.0 ** -23 * np.abs(ref) + add * np.abs(ref).max()
    ratio = err / bar
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('{}: largest gradient error / bar {:.3f} at {}, max |err| / max|ref| {:.3e}'.format(
        what, float(ratio[i]), i, float(err.max() / np.abs(ref).max())))
    assert ratio[i] <= 1.0, (what, i, float(got[i]), float(ref[i]), float(bar[i]))


def _ids(cases):
    return ['r{}-{}x{}'.format(*c) for c in cases]


EDGE = [(r, H, W) for r in (1, 2) for H, W in C.edge_shapes(r)]


# ---- a. edge shapes, with gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('r,H,W', EDGE, ids=_ids(EDGE))
def test_edge_shape_value_and_gradient_per_element(dev, r, H, W):
    t, v, value, grad = C.edge_case(r, H, W)
    call = Call(dev, H, W, r)
    assert call(t, v) == OK
    what = 'r={} {}x{}'.format(r, H, W)
    check_value(call.value(), value, what)
    check_grad(call.gradient(), grad, ADD, what)


# ---- b. conditioned seam case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2])
def test_step_on_the_tile_seam_near_rank_one_sigma(dev, r):
    t, v, value, grad = C.conditioned_case(r)
    add = 4.0 * C.COND_FLOOR[r]
    assert add <= 1e-5
    call = Call(dev, 17, 65, r)
    assert call(t, v) == OK
    check_value(call.value(), value, 'seam step r={}'.format(r))
    check_grad(call.gradient(), grad, add, 'seam step r={}'.format(r))


# ---- c. window counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2])
def test_constant_and_affine_style_maps_lie_in_the_null_space_on_every_edge_shape(dev, r):
    for H, W in C.edge_shapes(r):
        t, _, _, _ = C.edge_case(r, H, W)
        what = 'r={} {}x{}'.format(r, H, W)
        call = Call(dev, H, W, r)
        # v = 1: every window has s2 - s0^2/k = 0, u = 0, a = 0, beta = 1, so the gradient is 2 (n_p - windows gathered)
        assert call(t, np.ones_like(t)) == OK
        g = call.gradient()
        miss = np.argwhere(np.abs(g) >= 1e-6)
        assert abs(call.value()) < 1e-9 * H * W, (what, call.value())
        assert miss.size == 0, (what, 'pixel (c, y, x), gradient, windows that hold it',
                                [(tuple(p), float(g[tuple(p)]), int(C.window_count(H, W, r)[p[1], p[2]])) for p in miss[:8]])
        # v = the target's first channel in all three: affine in the image inside every window, the loss is eps-order
        v_aff = np.ascontiguousarray(np.broadcast_to(t[0], t.shape))
        ref_value, _ = C.reference(t, v_aff, r)
        assert call(t, v_aff) == OK
        call.gradient()
        print('{}: affine value {:.6e}, fp64 reference {:.6e}'.format(what, call.value(), ref_value))
        assert call.value() <= ref_value * 1.001 + 1e-12, (what, call.value(), ref_value)


@pytest.mark.parametrize('r', [1, 2])
def test_gradient_is_the_window_count_form_when_eps_drowns_sigma(dev, r):
    """eps = 1e30: Sigma^-1 vanishes, a = 0 and beta is the window's mean of v, so the gradient is
    2 (n_p v_p - sum of the means of the windows that hold p) with n_p the closed-form count that test_matting_cpu.py checks
    against a brute-force count: n_p off by one at a border moves that pixel's gradient by 2 v_p."""
    for H, W in C.edge_shapes(r):
        t, v, _, _ = C.edge_case(r, H, W)
        call = Call(dev, H, W, r)
        assert call(t, v, eps=1e30) == OK
        what = 'eps=1e30 r={} {}x{}'.format(r, H, W)
        check_value(call.value(), matting_fast(t, v, r, 1e30)[0], what)
        check_grad(call.gradient(), C.count_gradient(v, r), ADD, what)


# ---- d. value-only path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r,H,W', [(1, 3, 3), (1, 11, 34), (1, 10, 37), (1, 17, 65), (2, 24, 31)],
                         ids=_ids([(1, 3, 3), (1, 11, 34), (1, 10, 37), (1, 17, 65), (2, 24, 31)]))
def test_null_gradient_gives_the_same_value_and_partials_and_writes_no_gradient(dev, r, H, W):
    t, v = C.inputs(r, H, W)
    call = Call(dev, H, W, r)
    assert call(t, v) == OK
    call.gradient()
    loss_bits, partials = call.loss.t.view(torch.int64).clone(), call.ws.t.view(torch.int64).clone()
    check_value(call.value(), matting_fast(t, v, r, C.EPS)[0], 'r={} {}x{}'.format(r, H, W))
    assert call(t, v, with_grad=False) == OK                 # refills all three; the NaN buffer sits where the gradient went
    assert torch.equal(call.loss.t.view(torch.int64), loss_bits)
    assert torch.equal(call.ws.t.view(torch.int64), partials)
    assert call.grad.untouched()


# ---- e. grid cap -----------------------------------------------------------------------------------------------------------
def test_tallest_accepted_image_and_one_row_more(dev):
    r, W, H = 1, 3, 65535 * C.TY
    t, v = C.inputs(r, H, W)
    value, grad = matting_fast(t, v, r, C.EPS)
    call = Call(dev, H, W, r)
    assert call.ws_bytes == 65535 * 8                        # grid.y at its maximum, 65535 partials through k_matting_final
    assert call(t, v) == OK
    assert bool(torch.isfinite(call.ws.t).all()) and np.isfinite(call.value())
    check_value(call.value(), value, 'H={}'.format(H))
    check_grad(call.gradient(), grad, ADD, 'H={}'.format(H))
    # one row more: refused, nothing written
    tall = Call(dev, H + 1, W, r)
    big = torch.zeros(3, H + 1, W, device=dev)
    assert tall(big, big) == INVALID_ARG
    assert tall.outputs_untouched()


# ---- f. refusals through the ABI -------------------------------------------------------------------------------------------
def test_refused_calls_leave_every_output_untouched(dev):
    H, W = 16, 16
    t = torch.rand(3, H, W, device=dev)
    call = Call(dev, H, W, 1)
    for r in (1, 2):
        for kw in ({'H': 2 * r}, {'W': 2 * r}):
            assert call(t, t, r=r, **kw) == INVALID_ARG and call.outputs_untouched(), (r, kw)
    for r in (0, 3):
        assert call(t, t, r=r) == UNSUPPORTED and call.outputs_untouched(), r
    # a workspace off 8-byte alignment; the buffer is 8 bytes longer so that an accepted call would stay inside it
    wide = Call(dev, H, W, 1)
    wide.ws = Guarded(wide.ws_bytes + 8, dev, torch.float64, WS_FILL)
    assert wide(t, t, ws_offset=4) == INVALID_ARG and wide.outputs_untouched()
    for name in ('target', 'v', 'loss', 'workspace'):        # NSR_CHECK_PTR
        assert call(t, t, null=(name,)) == INVALID_ARG and call.outputs_untouched(), name
    # the same buffers still work
    assert call(t, torch.ones_like(t)) == OK and abs(call.value()) < 1e-9 * H * W


# ---- g. capture and replay -------------------------------------------------------------------------------------------------
def test_graph_capture_replays_with_new_contents(dev):
    from nerfstyle_amd.matting import matting_laplacian
    r, H, W = 2, 17, 65
    sets = [C.inputs(r, H, W), C.conditioned_inputs(r), C.inputs(1, H, W)]
    t = torch.tensor(sets[0][0], device=dev)
    v = torch.tensor(sets[0][1], device=dev).requires_grad_(True)

    def body():
        loss = matting_laplacian(t, v, r)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = body()
    for tn, vn in sets[1:]:
        with torch.no_grad():
            t.copy_(torch.tensor(tn, device=dev))
            v.copy_(torch.tensor(vn, device=dev))
        graph.replay()
        torch.cuda.synchronize()
        q = torch.tensor(vn, device=dev).requires_grad_(True)
        loss_e = matting_laplacian(torch.tensor(tn, device=dev), q, r)
        loss_e.backward()
        assert torch.equal(loss_g.view(torch.int64), loss_e.detach().view(torch.int64))
        assert torch.equal(v.grad.view(torch.int32), q.grad.view(torch.int32)) and float(q.grad.abs().max()) > 0
        check_value(float(loss_g), matting_fast(tn, vn, r, C.EPS)[0], 'replay')
