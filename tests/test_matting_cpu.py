"""Matting-Laplacian photorealism loss (the reference's MattingLaplacian, loss.py:217-278), host side: the test's own fp64
restatements against the reference's recorded outputs (tests/golden/make_matting_goldens.py), properties of the loss,
why the kernel computes in fp64, the C ABI's host-only paths, and the reference side of the edge tests
(matting_cases.py): the noise floor of the two restatements and the closed-form window count."""
import ctypes
import os

import numpy as np
import pytest
import torch

import matting_cases as C
from matting_ref import fixture_cases, matting_dense, matting_fast, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bars the HIP kernel is held to (tests/test_gpu_matting.py): value relative error, gradient relative L2 error
VALUE_TOL, GRAD_TOL = 1e-9, 1e-6


@pytest.fixture(scope='module')
def fixture():
    return fixture_cases(np.load(os.path.join(ROOT, 'tests', 'golden', 'matting_reference.npz')))


@pytest.fixture(scope='module')
def built():
    from nerfstyle_amd import build
    return build.build()


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def test_fixture_covers_the_issue_cases(fixture):
    got = {(n, r, t.shape) for n, r, _, t, *_ in fixture}
    assert got == {('r1_3x3', 1, (3, 3, 3)), ('r1_9x13', 1, (3, 9, 13)), ('r1_24x31', 1, (3, 24, 31)),
                   ('r1_24x31_flat', 1, (3, 24, 31)), ('r1_9x12_edge', 1, (3, 9, 12)), ('r2_11x10', 2, (3, 11, 10))}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'matting_reference.npz')) < 100 * 1024


def test_dense_restatement_equals_reference(fixture):
    for name, r, eps, t, v, value, g64, g32 in fixture:
        val, g = matting_dense(t, v, r, eps)
        assert rel_err(val, value) < 1e-10, name
        assert rel_l2(g, g64) < 1e-8, name
        # the reference's gradient for a float32 style_map is its float64 gradient rounded once
        assert np.array_equal(g64.astype(np.float32), g32), name


def test_vectorised_restatement_equals_reference(fixture):
    for name, r, eps, t, v, value, g64, _ in fixture:
        val, g = matting_fast(t, v, r, eps)
        assert rel_err(val, value) < 1e-10, name
        assert rel_l2(g, g64) < 1e-8, name


def test_loss_properties():
    rng = np.random.default_rng(7)
    H, W = 126, 168
    t = rng.random((3, H, W))
    v = rng.random((3, H, W))
    L_rand, _ = matting_fast(t, v, 1, 1e-7)
    assert L_rand > 0
    for r in (1, 2):
        assert matting_fast(t[:, :20, :24], v[:, :20, :24], r, 1e-7)[0] >= 0.0
    # a constant style map lies in the Laplacian's null space
    L_const, _ = matting_fast(t, np.full_like(v, 0.3), 1, 1e-7)
    assert abs(L_const) <= 1e-10 * H * W, L_const
    # so does (up to the eps regulariser) any affine function of the target's colours
    A = rng.standard_normal((3, 3))
    b = rng.standard_normal(3)
    v_aff = np.einsum('ci,ihw->chw', A, t) + b[:, None, None]
    L_aff, _ = matting_fast(t, v_aff, 1, 1e-7)
    assert 0 <= L_aff < 1e-4 * L_rand, (L_aff, L_rand)


def test_float32_evaluation_fails_the_kernel_tolerance_on_a_near_flat_target(fixture):
    """Why the kernel computes in fp64: on the near-flat target Sigma is dominated by eps / k ~ 1.1e-8, and the same
    per-window formula evaluated in float32 misses the bars the HIP result is held to; on a random target it is close."""
    case = {c[0]: c for c in fixture}
    _, r, eps, t, v, value, g64, _ = case['r1_24x31_flat']
    val32, g32 = matting_dense(t, v, r, eps, dtype=np.float32)
    assert rel_err(val32, value) > VALUE_TOL or rel_l2(g32, g64) > GRAD_TOL
    assert rel_l2(g32, g64) > 10 * GRAD_TOL
    _, r, eps, t, v, value, g64, _ = case['r1_24x31']
    val32, g32 = matting_dense(t, v, r, eps, dtype=np.float32)
    assert rel_err(val32, value) < 1e-5 and rel_l2(g32, g64) < 1e-5


def test_workspace_query_and_invalid_arguments_on_the_host(built):
    from nerfstyle_amd import _lib
    L = _lib.lib()
    assert L.nsr_abi_version() == 6
    assert L.nsr_matting_laplacian_workspace_bytes(756, 1008, 1) == 32 * 95 * 8
    assert L.nsr_matting_laplacian_workspace_bytes(3, 3, 1) == 8
    assert L.nsr_matting_laplacian_workspace_bytes(11, 10, 2) == 2 * 8
    fake = ctypes.c_void_p(256)            # never dereferenced: every call below returns before touching the device
    loss = ctypes.c_void_p(512)
    ws = ctypes.c_void_p(1024)
    # null pointers -> NSR_ERR_INVALID_ARG
    assert L.nsr_matting_laplacian(None, fake, 8, 8, 1, 1e-7, loss, None, ws, None) == -1
    assert L.nsr_matting_laplacian(fake, None, 8, 8, 1, 1e-7, loss, None, ws, None) == -1
    assert L.nsr_matting_laplacian(fake, fake, 8, 8, 1, 1e-7, None, None, ws, None) == -1
    assert L.nsr_matting_laplacian(fake, fake, 8, 8, 1, 1e-7, loss, None, None, None) == -1
    # fewer than 2r+1 rows or columns: no window fits
    assert L.nsr_matting_laplacian(fake, fake, 2, 8, 1, 1e-7, loss, None, ws, None) == -1
    assert L.nsr_matting_laplacian(fake, fake, 8, 2, 1, 1e-7, loss, None, ws, None) == -1
    assert L.nsr_matting_laplacian(fake, fake, 4, 9, 2, 1e-7, loss, None, ws, None) == -1
    # win_rad outside {1, 2}
    assert L.nsr_matting_laplacian(fake, fake, 16, 16, 0, 1e-7, loss, None, ws, None) == -2
    assert L.nsr_matting_laplacian(fake, fake, 16, 16, 3, 1e-7, loss, None, ws, None) == -2


def test_module_refuses_cpu_tensors_and_a_target_that_requires_grad(built):
    from nerfstyle_amd.losses import MattingLaplacian
    from nerfstyle_amd.matting import MattingLaplacian as M2
    assert MattingLaplacian is M2
    m = MattingLaplacian(torch.device('cpu'))
    assert (m.win_rad, m.eps) == (1, 1e-7)
    t = torch.rand(3, 8, 9)
    v = torch.rand(3, 8, 9, requires_grad=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(t, v)
    with pytest.raises(RuntimeError, match='target'):
        m(t.clone().requires_grad_(True), v)


def test_style_criterion_photo_lambda_defaults_off():
    import inspect
    from nerfstyle_amd.stylize import StyleCriterion
    assert inspect.signature(StyleCriterion).parameters['photo_lambda'].default == 0.0
    crit = StyleCriterion(None, None)
    assert crit.photo_loss is None and crit.last_photo is None
    crit = StyleCriterion(None, None, photo_lambda=1e-4)
    assert crit.photo_loss.win_rad == 1 and crit.photo_loss.eps == 1e-7


# ---- the reference side of tests/test_gpu_matting_edges.py ------------------------------------------------------------

def test_edge_shapes_are_the_issue_list():
    for r in (1, 2):
        D = 2 * r + 1
        shapes = C.edge_shapes(r)
        assert len(shapes) == len(set(shapes)) and all(H >= D and W >= D for H, W in shapes)
        assert {(D, D), (D, D + 1), (D + 1, D), (D, 97), (61, D), (8 + r + 1, 32 + r + 1), (17, 65),
                (8 + 2 * r + 1, 64 + 2 * r + 1)} <= set(shapes)
        assert {W for H, W in shapes if H == 11} >= {31, 32, 33, 32 + r, 32 + r + 1, 32 + 2 * r, 32 + 2 * r + 1, 63, 64, 65}
        assert {H for H, W in shapes if W == 37} >= {7, 8, 9, 8 + r, 8 + r + 1, 8 + 2 * r, 8 + 2 * r + 1, 16, 17}
        assert max(H * W for H, W in shapes) <= C.DENSE_LIMIT                  # matting_dense is the reference of every one
    t, v = C.inputs(1, 11, 33)
    t2, v2 = C.inputs(1, 11, 33)
    assert t.dtype == v.dtype == np.float32 and np.array_equal(t, t2) and np.array_equal(v, v2)
    assert not np.array_equal(t, C.inputs(2, 11, 33)[0]) and 0.0 <= t.min() and t.max() < 1.0


def test_edge_shapes_dense_and_vectorised_restatements_agree():
    """The noise floor under the per-element bars of the GPU edge tests: how far two fp64 evaluations of the same loss
    differ.  The additive term of the bar, 1e-9 max|grad|, stands only while this floor is at most a quarter of it."""
    worst_g = worst_v = 0.0
    for r in (1, 2):
        for H, W in C.edge_shapes(r):
            t, v = C.inputs(r, H, W)
            fg, fv = C.floor(t, v, r)
            print('r={} {}x{}: dense vs fast, gradient {:.3e} max|grad| per element, value {:.3e} relative'.format(r, H, W, fg, fv))
            worst_g, worst_v = max(worst_g, fg), max(worst_v, fv)
    print('edge shapes: largest gradient floor {:.3e}, largest value floor {:.3e}'.format(worst_g, worst_v))
    assert worst_g <= 0.25 * 1e-9 and worst_v <= 0.25 * VALUE_TOL
    for r in (1, 2):
        t, v = C.conditioned_inputs(r)
        fg, fv = C.floor(t, v, r)
        print('seam step r={}: dense vs fast, gradient {:.3e} max|grad| per element (recorded {:.3e}), value {:.3e} relative'.format(
            r, fg, C.COND_FLOOR[r], fv))
        # the GPU bar adds 4 x the recorded floor: the record must cover what is measured, and the case must stay testable
        assert fg <= 2.0 * C.COND_FLOOR[r] and 4.0 * C.COND_FLOOR[r] <= 1e-5 and fv <= 0.25 * VALUE_TOL
        # the windows on the seam are what the case is for: Sigma's smallest eigenvalue is orders below its largest
        k = (2 * r + 1) ** 2
        I = t[:, 8 - r:8 + r + 1, C.TX - r:C.TX + r + 1].reshape(3, k).astype(np.float64)
        ev = np.linalg.eigvalsh(np.cov(I, bias=True) + C.EPS / k * np.eye(3))
        assert ev[0] < 1e-4 * ev[-1], ev


def test_closed_form_window_count_equals_a_brute_force_count():
    for r in (1, 2):
        for H, W in C.edge_shapes(r):
            n = C.window_count(H, W, r)
            assert np.array_equal(n, C.window_count_brute(H, W, r)), (r, H, W)
            assert n.min() >= 1 and n.max() <= (2 * r + 1) ** 2 and n.sum() == (2 * r + 1) ** 2 * (H - 2 * r) * (W - 2 * r)


def test_count_form_of_the_gradient_is_the_loss_with_a_drowned_sigma():
    """eps = 1e30 leaves 2 (n_p v_p - sum of window means): what the GPU test of the window count compares against"""
    for r in (1, 2):
        for H, W in ((2 * r + 1, 2 * r + 2), (11, 32 + r + 1), (17, 65)):
            t, v = C.inputs(r, H, W)
            _, g = matting_fast(t, v, r, 1e30)
            ref = C.count_gradient(v, r)
            assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max(), (r, H, W)
