"""tests/np_bn_elu.py, the float64 statement of csrc/ssdhip_bntrain.hip, against torch's own CPU autograd in float64
(F.batch_norm(training=True) -> F.elu -> F.max_pool2d), plus hand-worked cases of the pool winner rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import np_bn_elu as ref

TOL = 1e-10


def _torch_chain(y, gamma, beta, rm, rv, momentum, eps, g_full, g_pooled):
    """NHWC float64 arrays in, torch's results out (as NHWC arrays)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    yt = t(y).permute(0, 3, 1, 2).clone().requires_grad_(True)
    gt, bt = t(gamma).clone().requires_grad_(True), t(beta).clone().requires_grad_(True)
    rmt, rvt = t(rm).clone(), t(rv).clone()
    full = F.elu(F.batch_norm(yt, rmt, rvt, gt, bt, True, momentum, eps))
    loss = (full * t(g_full).permute(0, 3, 1, 2)).sum() if g_full is not None else 0.0
    pooled = None
    if g_pooled is not None:
        pooled = F.max_pool2d(full, 2, 2)
        loss = loss + (pooled * t(g_pooled).permute(0, 3, 1, 2)).sum()
    loss.backward()
    nhwc = lambda x: None if x is None else x.detach().permute(0, 2, 3, 1).numpy()
    return nhwc(full), nhwc(pooled), nhwc(yt.grad), gt.grad.numpy(), bt.grad.numpy(), rmt.numpy(), rvt.numpy()


CASES = [(shape, form) for shape in [(2, 6, 4, 5), (3, 7, 5, 8), (1, 1, 2, 3), (2, 3, 3, 4)] for form in ("pooled", "both", "full")
         if form == "full" or min(shape[1:3]) >= 2]           # a map without a window has the full form only


@pytest.mark.parametrize("shape,form", CASES)
def test_reference_equals_torch_autograd(shape, form):
    b, h, w, c = shape
    rng = np.random.RandomState(b * 100 + h * 10 + w)
    y = rng.randn(*shape) * 1.5 + rng.randn(c) * 2          # continuous: no tied windows
    gamma = rng.rand(c) + 0.5
    gamma[::2] *= -1
    gamma[c // 2] = 0.0
    beta = rng.randn(c) * 0.5
    rm, rv = rng.randn(c), rng.rand(c) + 0.5
    momentum, eps = 0.01, 1e-3
    g_full = rng.randn(*shape) if form != "pooled" else None
    g_pooled = rng.randn(b, h // 2, w // 2, c) if form != "full" else None
    full, pooled, dy, dgamma, dbeta, rm_t, rv_t = _torch_chain(y, gamma, beta, rm, rv, momentum, eps, g_full, g_pooled)
    got = ref.forward(y, gamma, beta, eps)
    np.testing.assert_allclose(got["full"], full, rtol=0, atol=TOL)
    if pooled is not None:
        np.testing.assert_allclose(got["pooled"], pooled, rtol=0, atol=TOL)
    np.testing.assert_allclose(ref.running_update(rm, got["mean"], momentum), rm_t, rtol=0, atol=TOL)
    np.testing.assert_allclose(ref.running_update(rv, got["var_unbiased"], momentum), rv_t, rtol=0, atol=TOL)
    dy_r, dgamma_r, dbeta_r, _ = ref.backward(y, gamma, beta, eps, g_full, g_pooled)
    np.testing.assert_allclose(dy_r, dy, rtol=0, atol=TOL)
    np.testing.assert_allclose(dgamma_r, dgamma, rtol=0, atol=TOL)
    np.testing.assert_allclose(dbeta_r, dbeta, rtol=0, atol=TOL)


def test_winner_rule_by_hand():
    """One 2 x 2 window, five channels: a plain maximum; a tie of the largest value (first in row-major order wins); gamma < 0 (the
    smallest y wins); gamma < 0 with tied smallest values; gamma = 0 (position (0,0))."""
    #            (0,0) (0,1) (1,0) (1,1)
    cols = [[1.0, 4.0, 2.0, 3.0],
            [5.0, 7.0, 7.0, 7.0],
            [1.0, 4.0, -2.0, 3.0],
            [3.0, -1.0, 5.0, -1.0],
            [1.0, 9.0, 2.0, 3.0]]
    y = np.array(cols).T.reshape(1, 2, 2, 5)
    gamma = np.array([1.0, 2.0, -1.0, -0.5, 0.0])
    win = ref.winners(y, gamma).reshape(4, 5)
    assert win.T.astype(int).tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]]
    # the routed gradient lands on the winner alone, and the forward's pooled value is the winner's
    gp = np.arange(1.0, 6.0).reshape(1, 1, 1, 5)
    beta = np.full(5, 0.25)
    _, _, _, routed = ref.backward(y, gamma, beta, 1e-3, None, gp)
    assert np.array_equal(routed.reshape(4, 5), win * gp.reshape(1, 5))
    out = ref.forward(y, gamma, beta, 1e-3)
    assert np.array_equal(out["pooled"].reshape(5), (out["full"].reshape(4, 5) * win).sum(axis=0))


def test_odd_edges_count_in_the_statistics_and_receive_the_mean_terms():
    """3 x 3 map, pooled form only: row 2 and column 2 belong to no window, yet they move mean / variance and their dy is the
    -(dbeta + xhat dgamma) / M part alone (their own dv is zero)."""
    rng = np.random.RandomState(5)
    y = rng.randn(2, 3, 3, 4)
    gamma, beta, eps = np.array([1.0, -1.5, 0.7, 2.0]), rng.randn(4) * 0.3, 1e-3
    gp = rng.randn(2, 1, 1, 4)
    mean, var, _ = ref.batch_stats(y)
    inner_mean = y[:, :2, :2].reshape(-1, 4).mean(axis=0)
    assert np.all(np.abs(mean - inner_mean) > 1e-3)                 # the edge values entered the statistics
    dy, dgamma, dbeta, routed = ref.backward(y, gamma, beta, eps, None, gp)
    assert not routed[:, 2].any() and not routed[:, :, 2].any()
    m = 2 * 3 * 3
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (y - mean) * invstd
    want = gamma * invstd * (-dbeta / m - xhat * dgamma / m)
    edge = np.ones((3, 3), dtype=bool)
    edge[:2, :2] = False
    np.testing.assert_allclose(dy[:, edge], want[:, edge], rtol=0, atol=1e-14)
    assert np.abs(dy[:, edge]).min() > 0
