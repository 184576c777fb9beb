"""The float64 restatements of tests/storage_reference.py against ATen / float64 autograd of the PyTorch ops they stand for, and
the sensitivity of the bound the GPU tests use (tests/test_storage_edge_gpu.py).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import storage_reference as R

D = torch.float64


def rnd(seed, *shape, dtype=torch.float32):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).to(dtype)


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 9, 17, 20])
def test_interp_matrix_is_atens_float32_recipe(n):
    M = R.interp_matrix(n)
    assert M.shape == (2 * n, n)
    eye = torch.eye(n, dtype=torch.float32)
    # rows: interpolate the identity along H (W = 1 stays 1 -> 2 identical columns)
    up = F.interpolate(eye.t().reshape(1, n, n, 1), scale_factor=2, mode="bilinear", align_corners=True)   # (1, n, 2n, 2)
    got = up[0, :, :, 0].t().double()
    # ATen evaluates l0*v0 + l1*v1 in float32 on an identity basis: each entry is one of the float32 weights (or their sum on the
    # last row, where both taps read the same pixel)
    assert float((M - got).abs().max()) <= 2.0 ** -23
    assert bool(((M.sum(1) - 1.0).abs() <= 2.0 ** -23).all())
    # the adjoint restatement is float64 autograd of the forward one
    a = rnd(n, 2, 3, n, max(1, n - 1), dtype=D).requires_grad_(True)
    gu = rnd(n + 1, 2, 3, 2 * n, 2 * max(1, n - 1), dtype=D)
    out, _ = R.up2x(a, a.abs())
    (g_auto,) = torch.autograd.grad(out, a, gu)
    g_ref, g_abs = R.up2x_adj(gu)
    assert close(g_ref, g_auto) and bool((g_abs >= g_ref.abs() - 1e-12).all())
    # and the forward agrees with ATen in float64 up to the float32-vs-float64 weights: src = ratio*o carries the float32 rounding of
    # ratio times o <= 2n and one rounding of the product of magnitude <= n, so each lambda is within 3n * 2^-24 and a blend of two
    # taps per axis within 4 * 3n * 2^-24 max|a|
    ref64 = F.interpolate(a.detach(), scale_factor=2, mode="bilinear", align_corners=True)
    assert float((out.detach() - ref64).abs().max()) <= 12 * n * 2.0 ** -24 * float(a.detach().abs().max())


@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (3, 16, 6, 10)])
def test_pool_add_and_bn_backward_restatements(shape):
    B, C, H, W = shape
    y = rnd(1, *shape)
    sc = torch.from_numpy(np.random.RandomState(2).uniform(0.5, 1.5, C).astype(np.float32))
    sh = 0.3 * rnd(3, C)
    a, a_abs = R.bnrelu(y, sc, sh)
    assert close(a, F.relu(y.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)))
    assert close(R.pool2(a, a_abs)[0], F.avg_pool2d(a, 2, 2))
    raw, raw_abs = R.bnrelu(y, None, None)
    assert torch.equal(raw, y.double()) and torch.equal(raw_abs, y.double().abs())
    p = rnd(4, *shape)
    assert close(R.add(p, a, a_abs)[0], p.double() + a)
    # pooling adjoint = autograd of avg_pool2d
    t = rnd(5, *shape, dtype=D).requires_grad_(True)
    gp = rnd(6, B, C, H // 2, W // 2, dtype=D)
    (auto,) = torch.autograd.grad(F.avg_pool2d(t, 2, 2), t, gp)
    assert close(R.pool2_bwd(gp)[0], auto)
    g0 = rnd(7, *shape)
    r, ra = R.pool2_bwd(gp, g0)
    assert close(r, auto + g0.double()) and bool((ra >= r.abs() - 1e-12).all())
    # BatchNorm(training) + ReLU backward: dy = scale*dz + k1*y + k0 against float64 autograd of relu(batch_norm(y))
    y64 = y.double().requires_grad_(True)
    gamma, beta = sc.double().requires_grad_(True), sh.double().requires_grad_(True)
    g = rnd(8, *shape)
    out = F.relu(F.batch_norm(y64, None, None, gamma, beta, training=True, eps=1e-5))
    dy_a, dga_a, dbe_a = torch.autograd.grad(out, [y64, gamma, beta], g.double())
    mean = y.double().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.double().var((0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma.detach() * invstd
    shift = beta.detach() - mean * scale
    ref = R.bn_bwd(g, y, scale, shift, mean, invstd)
    assert close(ref["dy"], dy_a, 1e-10) and close(ref["dgamma"], dga_a, 1e-10) and close(ref["dbeta"], dbe_a, 1e-10)
    assert bool((ref["dy_abs"] >= ref["dy"].abs() - 1e-12).all())
    coef, coef_a, coef_f, _ = R.coef_from_sums(ref["dbeta"], ref["dgamma"], scale, shift, mean, invstd, beta.detach(), B * H * W)
    assert close(coef, ref["coef"]) and bool((coef_a >= coef.abs() - 1e-12).all())
    # coef_f describes the same dy on z = y*sc + sh
    z = y.double() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    k1f, k0f = coef_f[2 * C:3 * C].view(1, -1, 1, 1), coef_f[3 * C:].view(1, -1, 1, 1)
    assert close(scale.view(1, -1, 1, 1) * ref["dz"] + k1f * z + k0f, ref["dy"], 1e-10)
    sums, sums_abs = R.bn_sums_y(g, y, scale, shift)
    assert close(sums[:, 0], ref["dbeta"]) and close(invstd * (sums[:, 1] - mean * sums[:, 0]), ref["dgamma"], 1e-9)
    assert bool((sums_abs >= sums.abs()).all())


@pytest.mark.parametrize("shape,cin,cout", [((2, 1, 7), 2, 16), ((2, 2, 3), 2, 16), ((2, 1, 7), 16, 1), ((2, 2, 3), 16, 1),
                                            ((1, 1, 1), 16, 1), ((1, 3, 3), 2, 16)])
def test_thin_conv_restatements_at_heights_one_and_two(shape, cin, cout):
    B, H, W = shape
    a = rnd(11, B, cin, H, W, dtype=D).requires_grad_(True)
    w = rnd(12, cout, cin, 3, 3, dtype=D).requires_grad_(True)
    bias = rnd(13, cout, dtype=D)
    g = rnd(14, B, cout, H, W, dtype=D)
    out = F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), w, bias)
    assert close(R.conv3_rep(a.detach(), w.detach(), bias), out.detach())
    ga, gw = torch.autograd.grad(out, [a, w], g)
    assert close(R.conv3_rep_dgrad(g, w.detach()), ga) and close(R.conv3_rep_wgrad(a.detach(), g), gw)


def test_bound_helper_bites():
    rs = np.random.RandomState(21)
    a = torch.from_numpy(rs.standard_normal(4096).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(4096).astype(np.float32))
    ref, ref_abs = a.double() + b.double(), a.double().abs() + b.double().abs()
    k = R.K["add"]
    v32 = a + b                                                  # an fp32 result (one rounding)
    assert R.check(v32, ref, ref_abs, k, False) <= 1.0
    assert R.check(R.rb(v32), ref, ref_abs, k, True) <= 1.0       # RNE-rounded: passes
    trunc = (v32.view(torch.int32) & -65536).view(torch.float32)  # the same result truncated to bf16
    with pytest.raises(AssertionError):
        R.check(trunc, ref, ref_abs, k, True)
    twice = R.rb(R.rb(a) + b)                                     # double rounding
    err = (twice.double() - ref).abs()
    assert bool((err > R.bound(ref, ref_abs, k, True)).any())
    with pytest.raises(AssertionError):
        R.check(twice, ref, ref_abs, k, True)
    # one interpolation weight off by 1e-3
    x = torch.from_numpy(rs.standard_normal((3, 16, 7, 9)).astype(np.float32))
    My, Mx = R.interp_matrix(7), R.interp_matrix(9)
    up, up_abs = R.up2x(x.double(), x.double().abs(), My, Mx)
    My_bad = My.clone()
    My_bad[5, 2] += 1e-3
    bad, _ = R.up2x(x.double(), x.double().abs(), My_bad, Mx)
    assert R.check(up.float(), up, up_abs, R.K["up2x"], False) <= 1.0 and R.check(R.rb(up.float()), up, up_abs, R.K["up2x"], True) <= 1.0
    for bf16 in (False, True):
        with pytest.raises(AssertionError):
            R.check(R.stored(bad.float(), bf16), up, up_abs, R.K["up2x"], bf16)
    # the reduced-output bar is relative to the sum of magnitudes
    s, s_abs = ref.sum().view(1), ref_abs.sum().view(1)
    assert R.check_sum((a + b).sum().view(1), s, s_abs, R.BAR_SUM) <= 1.0
    with pytest.raises(AssertionError):
        R.check_sum(s + 2e-5 * s_abs, s, s_abs, R.BAR_SUM)
