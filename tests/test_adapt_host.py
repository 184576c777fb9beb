"""CPU: fine-tuning a trained model -- what can be held without a GPU.

  * the pins of include/sifsr_adapt.h for the `sifsra_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_adapt_gpu.py,
  * workspace sizes and the error codes that are found before anything is launched,
  * the restatements of tests/adapt_reference.py: the frozen network with every mask taken from its own forward IS plain torch
    eval-mode autograd; the operator-level input gradient against a written-out scatter; the tile targets against gaps_reference
    on a granule that holds an empty, a partly valid and a fully valid tile (asserted),
  * the public names and their defaults."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import adapt_reference as A
from tests import gaps_reference as G
from tests.capi_host import L  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sifsra_conv_in_dgrad", "sifsra_model_backward", "sifsra_model_forward", "sifsra_model_workspace_bytes", "sifsra_tile_targets"]


# ---- 1. the pins of include/sifsr_adapt.h (the gate itself is tests/test_capi_gate.py) ------------------------------------------
def test_every_writing_adapt_entry_point_has_a_contract_case(L):
    from tests import test_adapt_gpu as T
    names, writers = L.declared("adapt"), L.writers("adapt")
    assert names == NAMES
    assert writers == {"sifsra_model_forward": ["sr", "workspace"],
                       "sifsra_model_backward": ["grads", "dx", "workspace"],
                       "sifsra_conv_in_dgrad": ["dx"],
                       "sifsra_tile_targets": ["lst_out", "valid_out", "n_valid_out"]}
    assert "sifsra_model_workspace_bytes" not in writers                      # host only
    assert sorted(T.CONTRACT) == sorted(writers)
    assert len(T.CONTRACT["sifsra_model_backward"]) >= 2                       # with and without dx


def test_running_is_const_in_the_frozen_forward():
    text = open(os.path.join(ROOT, "include", "sifsr_adapt.h")).read()
    assert re.search(r"sifsra_model_forward\(const float\* x, float\* sr, const float\* params, const float\* running,", text)


def test_host_only_entry_points(L):
    for b, h, w in ((1, 24, 24), (2, 40, 56), (64, 256, 256)):
        assert L.call("sifsra_model_workspace_bytes", b, h, w) == L.call("sifsr_model_workspace_bytes", b, h, w, 1) > 0
    for b, h, w in ((0, 32, 32), (1, 16, 32), (1, 32, 36), (1, 24, 20)):
        assert L.call("sifsra_model_workspace_bytes", b, h, w) == 0
    one = ctypes.c_void_p(4096)
    need = L.call("sifsra_model_workspace_bytes", 1, 24, 24)
    fwd, bwd = L.lib().sifsra_model_forward, L.lib().sifsra_model_backward
    assert fwd(one, one, one, one, one, need, 1, 24, 20, 1e-5, None) == 1001
    assert fwd(one, one, one, one, one, need - 4, 1, 24, 24, 1e-5, None) == 1003
    for i in range(5):
        a = [one] * 5
        a[i] = None
        assert fwd(*a, need, 1, 24, 24, 1e-5, None) == 1002
    assert bwd(one, one, one, one, None, one, need, 1, 24, 20, 1, None) == 1001
    assert bwd(one, one, one, one, None, one, need - 4, 1, 24, 24, 1, None) == 1003
    assert bwd(one, one, one, one, None, one, need, 1, 24, 24, 2, None) == 1002
    for i in (0, 1, 2, 3, 5):
        a = [one] * 6
        a[i] = None
        assert bwd(*a, need, 1, 24, 24, 0, None) == 1002
    dg = L.lib().sifsra_conv_in_dgrad
    for b, h, w in ((0, 8, 8), (1, 2, 8), (1, 8, 2)):
        assert dg(one, one, one, one, one, one, one, b, h, w, None) == 1001
    for i in range(7):
        a = [one] * 7
        a[i] = None
        assert dg(*a, 1, 8, 8, None) == 1002
    assert dg(ctypes.c_void_p(4100), one, one, one, one, one, one, 1, 8, 8, None) == 1002      # g not 16-byte aligned
    tt = L.lib().sifsra_tile_targets
    args = lambda **kw: [kw.get(k, one) for k in ("filled", "valid", "active", "n_active")] + \
        [kw.get("first", 0), kw.get("count", 4), kw.get("h", 24), kw.get("w", 32), kw.get("win", 8), kw.get("overlap", 0), 0, 307.0,
         kw.get("std", 5.5)] + [kw.get(k, one) for k in ("lst_out", "valid_out", "n_valid_out")] + [None]
    for bad in (dict(win=6), dict(win=68), dict(h=4), dict(overlap=5), dict(first=-1), dict(count=0), dict(std=0.0)):
        assert tt(*args(**bad)) == 1001, bad
    for k in ("filled", "valid", "active", "n_active", "lst_out", "valid_out", "n_valid_out"):
        assert tt(*args(**{k: None})) == 1002, k
    assert tt(*args(n_valid_out=ctypes.c_void_p(4100))) == 1002


# ---- 2. the restatements -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", ["dsr", "sr2"])
def test_frozen_restatement_is_torch_eval_autograd(upstream):
    """network_ref(training=False) with every mask from its own forward against the same network built from torch.nn modules in
    eval mode: sr, dX and all 53 parameter gradients to 1e-12"""
    B, H, W = 2, 24, 32
    sd = O.synthetic_state(3)
    x, lst, dsr = A.network_inputs(5, B, H, W)
    loss_fn = lambda sr: O.LOSSES["sr2"](sr, lst.double(), x[:, 1:2].double(), A.MEAN, A.STD, 0.5, -0.25)
    up = dsr if upstream == "dsr" else loss_fn
    O.RECORD_MASKS = {}
    try:
        sr0, dx0, g0, _ = A.network_ref(sd, x, up)
        masks = dict(O.RECORD_MASKS)
    finally:
        O.RECORD_MASKS = None
    sr1, dx1, g1, _ = A.network_ref(sd, x, up, masks=masks)
    assert torch.equal(sr0, sr1) and torch.equal(dx0, dx1) and all(torch.equal(g0[n], g1[n]) for n in g0)

    nn = torch.nn
    class Net(nn.Module):                                   # plain torch: Conv2d(replicate) / BatchNorm2d / ReLU, eval mode
        def __init__(self):
            super().__init__()
            self.convs = nn.ModuleList(nn.Conv2d(ci, co, 3, padding=1, padding_mode="replicate", bias=False) for _, _, ci, co in O.CONV_BN_LAYERS)
            self.bns = nn.ModuleList(nn.BatchNorm2d(co) for _, _, _, co in O.CONV_BN_LAYERS)
            self.out = nn.Conv2d(16, 1, 3, padding=1, padding_mode="replicate")
        def unit(self, i, t):
            return torch.relu(self.bns[i](self.convs[i](t)))
        def forward(self, t):
            s = [self.unit(1, self.unit(0, t))]
            i = 2
            for _ in range(3):
                p = torch.nn.functional.avg_pool2d(s[-1], 2)
                s.append(self.unit(i + 2, p + self.unit(i + 1, self.unit(i, p))))
                i += 3
            u = s[3]
            for k in range(3):
                u = torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="bilinear", align_corners=True), s[2 - k]], 1)
                u = self.unit(i + 1, self.unit(i, u))
                i += 2
            return self.out(u)
    net = Net().double()
    with torch.no_grad():
        for i, (conv, bn, _, _) in enumerate(O.CONV_BN_LAYERS):
            net.convs[i].weight.copy_(sd[conv + ".weight"])
            net.bns[i].weight.copy_(sd[bn + ".weight"]); net.bns[i].bias.copy_(sd[bn + ".bias"])
            net.bns[i].running_mean.copy_(sd[bn + ".running_mean"]); net.bns[i].running_var.copy_(sd[bn + ".running_var"])
        net.out.weight.copy_(sd["outlay.weight"]); net.out.bias.copy_(sd["outlay.bias"])
    net.eval()
    xl = x.double().requires_grad_(True)
    sr = net(xl)
    loss = (sr * dsr.double()).sum() if upstream == "dsr" else loss_fn(sr)[-1]
    loss.backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert rel(sr.detach(), sr0) < 1e-12 and rel(xl.grad, dx0) < 1e-12
    for i, (conv, bn, _, _) in enumerate(O.CONV_BN_LAYERS):
        assert rel(net.convs[i].weight.grad, g0[conv + ".weight"]) < 1e-12, conv
        assert rel(net.bns[i].weight.grad, g0[bn + ".weight"]) < 1e-12 and rel(net.bns[i].bias.grad, g0[bn + ".bias"]) < 1e-12, bn
    assert rel(net.out.weight.grad, g0["outlay.weight"]) < 1e-12 and rel(net.out.bias.grad, g0["outlay.bias"]) < 1e-12
    assert all(float(g0[n].abs().max()) > 0 for n in g0) and float(dx0.abs().max()) > 0


@pytest.mark.parametrize("hw", [(3, 3), (3, 17), (17, 33)])
def test_conv_in_dgrad_restatement_against_a_scatter(hw):
    """the autograd form against the definition written as a scatter: every (q, tap) adds w * dy[q] at clamp(q + tap)"""
    H, W = hw
    g, y, scale, shift, coef, w = A.op_inputs(7, 2, H, W)
    ref = A.conv_in_dgrad_ref(g, y, scale, shift, coef, w)
    dz = torch.where(y.double() * scale.double() + shift.double() > 0, g.double(), torch.zeros(()).double())
    dy = coef[:16] * dz + (coef[16:32] * y.double() + coef[32:48])
    out = torch.zeros_like(ref)
    for qy in range(H):
        for qx in range(W):
            for ky in range(3):
                for kx in range(3):
                    py, px = min(max(qy + ky - 1, 0), H - 1), min(max(qx + kx - 1, 0), W - 1)
                    out[:, :, py, px] += dy[:, qy, qx, :] @ w[:, :, ky, kx].double()
    assert float((out - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    r = A.regions(H, W)
    assert int(r["corners"].sum()) == 4 and int(r["edges"].sum()) == 2 * (H - 2) + 2 * (W - 2) and int(r["interior"].sum()) == (H - 2) * (W - 2)


@pytest.mark.parametrize("overlap,cover", [(0, False), (2, False), (0, True), (2, True)])
def test_tile_targets_restatement(overlap, cover):
    lst, ndvi, filled, valid, active = A.granule_reference(A.WIN, overlap, cover)
    empty, partly, full = A.tile_kinds(valid, A.WIN, overlap, cover)
    assert empty >= 1 and partly >= 1 and full >= 1                     # the three kinds of tile
    assert len(active) == partly + full
    n = len(active)
    for first, count in ((0, n), (n - 2, 5), (3, 1)):                   # the whole list; wrapping; one tile
        tl, tv, nv = A.tile_targets_ref(filled, valid, active, first, count, A.WIN, overlap, cover, A.MEAN, A.STD)
        assert tl.dtype == np.float32 and tv.dtype == np.uint8 and set(np.unique(tv)) <= {0, 1}
        for i in range(count):
            t = int(active[(first + i) % n])
            oy, ox = G.origins(lst.shape[0], A.WIN, overlap, cover), G.origins(lst.shape[1], A.WIN, overlap, cover)
            y, x = oy[t // len(ox)], ox[t % len(ox)]
            want = (filled[y:y + A.WIN, x:x + A.WIN].astype(np.float64) - A.MEAN) / A.STD
            assert np.abs(tl[i, 0] - want).max() < 1e-5 and tv[i, 0].any()          # an active tile holds a valid pixel
            assert np.array_equal(tv[i, 0] != 0, G.valid_ref(lst)[y:y + A.WIN, x:x + A.WIN] != 0)
        assert nv == int(tv.sum()) > 0
    # at valid pixels the target is the normalised observation itself
    tl, tv, _ = A.tile_targets_ref(filled, valid, active, 0, n, A.WIN, overlap, cover, A.MEAN, A.STD)
    assert np.isfinite(tl).all()


# ---- 3. the public names -------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import adapt
    assert sifsr.adapt is adapt
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(adapt.input_gradient) == [("model", E), ("x", E), ("dsr", None)]
    assert sig(adapt.tile_targets) == [("filled", E), ("valid", E), ("active", E), ("n_active", E), ("first", E), ("count", E), ("stats", E),
                                       ("window", 64), ("overlap", 0), ("cover_edges", False)]
    s = dict(sig(adapt.adapt_granule))
    assert list(s)[:4] == ["model", "lst_g", "ndvi_g", "stats"]
    assert (s["mask"], s["kind"], s["batch"], s["window"], s["overlap"], s["cover_edges"], s["optimizer"]) == (None, "sr2", 16, 64, 0, False, None)
    m = sifsr.ModelB_2(2)
    assert m.bn_frozen is False and m.training
    m.eval()
    with adapt.frozen_bn(m) as inside:
        assert inside is m and m.bn_frozen is True and m.training
    assert m.bn_frozen is False and not m.training
    del m.bn_frozen                                                             # a pickle from before the attribute existed
    with adapt.frozen_bn(m):
        assert m.bn_frozen is True
    assert m.bn_frozen is False
    z = torch.zeros((1, 2, 24, 24))
    with pytest.raises(sifsr.SifsrError):                                       # no CPU path
        adapt.input_gradient(m, z)
    with pytest.raises(sifsr.SifsrError):
        adapt.adapt_granule(m, torch.zeros((24, 32)), torch.zeros((96, 128)), A.STATS)
