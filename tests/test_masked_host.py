"""CPU: training on partly valid patches -- what can be held without a GPU.

  * the restatement tests/masked_reference.py against the oracle: with an all-ones mask the masked loss IS O.LOSSES[kind] in values
    and gradient (1e-12), an image that is entirely invalid gets an exactly zero gradient, a NaN planted in `lst` at invalid
    pixels changes nothing, n = 0 gives zeros,
  * the inputs of the GPU loss tests reach both Huber branches: a condition on the inputs, asserted here,
  * the per-patch fill restatement: the planted patches are what they are meant to be, the moments are NumPy's,
  * the pins of include/sifsr_masked.h for the `sifsrm_` entry points (the gate itself is tests/test_capi_gate.py): the declared
    names, every entry point that can write through a pointer has a memory-contract case in tests/test_masked_gpu.py,
  * the public names exist with the defaults that leave every existing call as it was."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O
from tests import gaps_reference as G
from tests import masked_reference as R
from tests.capi_host import L  # noqa: F401  (the fixture)

CASES = [(hw, k, m) for hw in R.SHAPES for k in R.KINDS for m in R.MASKS]
IDS = [f"{hw[0]}x{hw[1]}-{k[0]}-a{k[1]}-{m}" for hw, k, m in CASES]


# ---- 1. the masked loss against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.SHAPES)
@pytest.mark.parametrize("kind,alpha,gamma", R.KINDS)
def test_all_valid_is_the_oracle_loss(hw, kind, alpha, gamma):
    sr, lst, ndvi = (t.double() for t in R.loss_inputs(hw))
    a, b = sr.clone().requires_grad_(True), sr.clone().requires_grad_(True)
    want = O.LOSSES[kind](a, lst, ndvi, R.MEAN, R.STD, alpha, gamma)
    got = R.masked_loss_ref(kind, b, lst, torch.ones(lst.shape, dtype=torch.uint8), ndvi, R.MEAN, R.STD, alpha, gamma)
    for g, w in zip(got, want):
        assert abs(float(g.detach()) - float(w.detach())) <= 1e-12 * abs(float(w.detach()))
    (ga,), (gb,) = torch.autograd.grad(want[2], a), torch.autograd.grad(got[2], b)
    assert float((ga - gb).abs().max()) <= 1e-12 * float(ga.abs().max())


@pytest.mark.parametrize("hw,kind,mask", [(hw, k, m) for hw, k, m in CASES if m != "random30"][::2])
def test_invalid_image_has_zero_gradient_and_nan_is_inert(hw, kind, mask):
    kind, alpha, gamma = kind
    sr, lst, ndvi, valid, n, losses, g = R.loss_reference(hw, kind, alpha, gamma, mask)
    assert (valid[0] == 0).all() and n == (valid != 0).sum() > 0
    assert (g[0] == 0).all() and (g[1] != 0).any()                      # image 0 is entirely invalid: EXACTLY zero
    planted = lst.clone()
    planted[valid == 0] = float("nan")
    s = sr.double().requires_grad_(True)
    out = R.masked_loss_ref(kind, s, planted, valid, ndvi, R.MEAN, R.STD, alpha, gamma)
    (g2,) = torch.autograd.grad(out[2], s)
    assert tuple(float(o.detach()) for o in out) == losses and torch.equal(g2, g)
    # n = 0
    s = sr.double().requires_grad_(True)
    out = R.masked_loss_ref(kind, s, planted, torch.zeros_like(valid), ndvi, R.MEAN, R.STD, alpha, gamma)
    (g0,) = torch.autograd.grad(out[2], s)
    assert [float(o.detach()) for o in out] == [0.0, 0.0, 0.0] and (g0 == 0).all()


@pytest.mark.parametrize("hw,kind,mask", CASES, ids=IDS)
def test_the_inputs_reach_both_huber_branches(hw, kind, mask):
    """Among the valid elements of each term the share with |e| > 1 lies in [5 %, 95 %].  The consistency term of the `single`
    mask has ONE element, for which no share can lie there; that pixel is chosen in the linear branch on purpose
    (masked_reference.loss_mask), and the quadratic branch of that term is reached by the other two masks."""
    kind, alpha, gamma = kind
    sr, lst, ndvi = (t.double() for t in R.loss_inputs(hw))
    v = R.loss_mask(hw, mask) != 0
    e1, e2 = R.residuals_ref(kind, sr, lst, ndvi, R.MEAN, R.STD, gamma)
    vh = v.repeat_interleave(4, 2).repeat_interleave(4, 3).expand_as(e2)
    s1, s2 = float((e1[v].abs() > 1).double().mean()), float((e2[vh].abs() > 1).double().mean())
    print(f"{hw} {kind} {mask}: share of |e| > 1: consistency {s1:.3f} of {int(v.sum())}, high-frequency {s2:.3f} of {int(vh.sum())}")
    assert 0.05 <= s2 <= 0.95
    if mask == "single":
        assert int(v.sum()) == 1 and s1 == 1.0
    else:
        assert 0.05 <= s1 <= 0.95
    if mask == "random30":
        assert 0.25 <= 1.0 - float(v.double().mean()) <= 0.35
        assert len(np.unique(R.loss_mask(hw, mask).numpy())) > 3         # any non-zero byte means valid


# ---- 2. the per-patch fill restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 20, 64])
def test_the_patches_are_what_they_are_planted_for(w):
    p = R.make_patches(w)
    filled, valid, mom = R.fill_patches_ref(p)
    assert filled.shape == valid.shape == (4, w, w) and filled.dtype == np.float32 and valid.dtype == np.uint8 and mom.shape == (4, 5)
    assert valid[0].all() and not valid[1].any() and valid[2].sum() == 1 and valid[2, w - 1, w - 1] == 1
    assert (filled[1] == 0).all() and (filled[2] == p[2, w - 1, w - 1]).all() and np.array_equal(filled[0], p[0])
    assert 0 < valid[3].sum() < w * w and valid[3, 0, w - 1] == 0 and valid[3, w - 1, 0] == 0 and np.isfinite(filled).all()
    level = G.fill_ref(p[3], None, True)[2]
    assert level.max() >= 2                                                  # the hole is deeper than one 2 x 2 block
    assert mom[0].tolist()[:1] == [w * w] and mom[1].tolist() == [0, 0, 0, np.inf, -np.inf]
    assert mom[2].tolist() == [1, float(p[2, -1, -1]), 0, float(p[2, -1, -1]), float(p[2, -1, -1])]
    ok = valid[3] != 0
    assert mom[3, 0] == ok.sum() and mom[3, 3] == p[3][ok].min() and mom[3, 4] == p[3][ok].max()
    assert abs(mom[3, 1] - p[3][ok].astype(np.float64).mean()) <= 1e-12 * mom[3, 1]
    assert abs(mom[3, 2] - p[3][ok].astype(np.float64).var() * ok.sum()) <= 1e-9 * mom[3, 2]
    for f, q in zip(filled, p):                                             # the closed form agrees
        assert np.array_equal(f.view(np.uint32), G.fill_ref_closed(q)[0].view(np.uint32))
    if w == 20:
        assert [s.shape[0] for s, _ in G.pyramid_ref(p[0], valid[0])] == [20, 10, 5, 3, 2, 1]     # ceil halving


def test_ten_percent_holes():
    p = R.holes_10_percent(6, 20)
    assert (p == 0).sum() * 10 == p.size and p[p != 0].min() >= 290 and p.max() <= 310
    assert p.astype(np.float64).mean() <= 0.9 * 310


# ---- 3. the pins of include/sifsr_masked.h (the gate itself is tests/test_capi_gate.py) -----------------------------------------
def test_every_writing_masked_entry_point_has_a_contract_case(L):
    from tests import test_masked_gpu as T
    names, writers = L.declared("masked"), L.writers("masked")
    assert names == ["sifsrm_patches_fill", "sifsrm_sif_loss", "sifsrm_sif_loss_workspace_bytes"]
    assert writers == {"sifsrm_patches_fill": ["filled", "valid", "moments"], "sifsrm_sif_loss": ["workspace", "losses3", "dsr"]}
    assert "sifsrm_sif_loss_workspace_bytes" not in writers                   # host only, no pointers: not a writer
    assert sorted(T.CONTRACT) == sorted(writers)
    assert all(len(cases) >= 3 for cases in T.CONTRACT.values())


def test_host_only_entry_points(L):
    """the workspace is the unmasked loss's; shape and argument errors are found before anything is launched (none needs a GPU)"""
    for kind, b, h, w in ((2, 2, 64, 64), (1, 2, 100, 36), (2, 64, 256, 256)):
        assert L.call("sifsrm_sif_loss_workspace_bytes", kind, b, h, w) == L.call("sifsr_sif_loss_workspace_bytes", kind, b, h, w) > 0
    fn, one = L.lib().sifsrm_patches_fill, ctypes.c_void_p(4096)
    for n, w in ((0, 8), (1, 0), (1, 2), (1, 6), (1, 68), (1, 128), (-1, 8)):
        assert fn(one, one, one, one, n, w, None) == 1001
    for i in range(4):
        a = [one] * 4
        a[i] = None
        assert fn(*a, 1, 8, None) == 1002
    loss = L.lib().sifsrm_sif_loss
    taps = (ctypes.c_float * 9)(*([1 / 9] * 9))
    args = lambda **kw: [kw.get("kind", 2)] + [kw.get(k, one) for k in ("sr", "lst", "valid", "n_valid", "ndvi")] + \
        [kw.get("B", 2), kw.get("H", 64), kw.get("W", 64), 307.0, 5.5, 0.5, -0.25, taps, taps, kw.get("ws", one), kw.get("nbytes", 1 << 30),
         kw.get("losses3", one), one, None]
    for bad in (dict(H=62), dict(W=8), dict(B=0), dict(B=65536), dict(H=66)):
        assert loss(*args(**bad)) == 1001
    for bad in (dict(kind=3), dict(sr=None), dict(lst=None), dict(valid=None), dict(n_valid=None), dict(ndvi=None), dict(ws=None),
                dict(losses3=None)):
        assert loss(*args(**bad)) == 1002
    assert loss(*args(nbytes=L.call("sifsrm_sif_loss_workspace_bytes", 2, 2, 64, 64) - 1)) == 1003


# ---- 4. the public names -------------------------------------------------------------------------------------------------------
def test_public_interface():
    import sifsr
    from sifsr import dataset, products, sif_ops, train
    E = inspect.Parameter.empty
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    assert sifsr.masked_sif_loss is sif_ops.masked_sif_loss and sifsr.masked_sif_loss_with_grad is sif_ops.masked_sif_loss_with_grad
    assert sifsr.sif_loss is sif_ops.sif_loss
    names = ["kind", "sr", "lst", "valid", "n_valid", "ndvi", "mean", "std", "alpha", "gamma"]
    assert [k for k, _ in sig(sif_ops.masked_sif_loss)] == [k for k, _ in sig(sif_ops.masked_sif_loss_with_grad)] == names
    assert [k for k, _ in sig(products.fill_patches)] == ["lst"]
    assert sig(products.MinedPatches.fill) == [("self", E)]
    assert sig(products.MinedPatches.statistics) == [("self", E), ("split", "Train"), ("valid_only", False)]
    # `loader` keeps the signature tests/test_products_host.py pins; the masked loader is a method of its own
    assert sig(products.MinedPatches.masked_loader) == sig(products.MinedPatches.loader)
    assert sig(products.PatchLoader.__init__)[-1] == ("masked", False)
    assert sig(dataset.MinedDataset.__init__) == [("self", E), ("mined", E), ("split", "Train"), ("stats", None), ("masked", False)]
    for f in (train.train_step, train.eval_step):
        assert sig(f)[-2:] == [("valid", None), ("n_valid", None)]
    assert sig(train.GraphedTrainStep.__init__)[-1] == ("masked", False)
    assert sig(train.GraphedTrainStep.__call__)[-2:] == [("valid", None), ("n_valid", None)]
    with pytest.raises(sifsr.SifsrError):                                      # no CPU path
        products.fill_patches(torch.zeros((2, 1, 8, 8)))
    z = torch.zeros((1, 1, 16, 16))
    with pytest.raises(sifsr.SifsrError):
        sifsr.masked_sif_loss("sr2", z, z[:, :, :4, :4], torch.ones((1, 1, 4, 4), dtype=torch.uint8), 16, z, 0.0, 1.0, 0.5, -0.25)
    with pytest.raises(ValueError):
        train.train_step(None, None, z, z, z, {}, 0.5, -0.25, valid=torch.ones(1))


def test_batches_of_three_and_five():
    from sifsr import train
    a, b, c = torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 16, 16), torch.ones(2, 1, 16, 16)
    out = train._unpack_batch((a, b, c), "cpu")
    assert out[3] is None and out[4] is None and torch.equal(out[2], c)
    v = torch.ones(2, 1, 4, 4, dtype=torch.uint8)
    for count in (torch.tensor([16, 9]), torch.tensor(25), torch.tensor([16, 9], dtype=torch.int32)):
        out = train._unpack_batch([a, b, c, v, count], "cpu")
        assert out[4].dtype == torch.int64 and out[4].dim() == 0 and int(out[4]) == 25 and out[3] is not None
    with pytest.raises(ValueError):
        train._unpack_batch((a, b, c, v), "cpu")
