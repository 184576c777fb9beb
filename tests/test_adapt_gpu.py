"""GPU: fine-tuning a trained model (include/sifsr_adapt.h) against the float64 restatements of
tests/adapt_reference.py.

  * frozen forward = the eval-mode forward, bit for bit; BatchNorm buffers keep their bits through forward and backward,
  * frozen gradients: all 53 parameter gradients and dX within TOL = 1e-4 (tests.conftest.rel_err, every tensor) of the float64
    restatement at the ReLU masks the device forward took -- a random upstream gradient and both SIF losses, four shapes,
  * training-mode dX: `grads` bit-equal to sifsr_model_backward, dX within TOL of the batch-statistics oracle at equal masks,
  * no cross-sample coupling in frozen mode; the second stream changes no bit,
  * sifsra_conv_in_dgrad at edge shapes: corners, edges and interior each within 1e-4, two runs bit-equal,
  * the memory contract of the four writers in the guarded, poisoned arena of tests/memcheck.py (CONTRACT is the table
    tests/test_capi_gate.py checks against the header),
  * tile_targets bit-equal to the restatement; adapt_granule bit-equal to the loop written out here, its first step against the
    float64 oracle; the frozen step captured into a hipGraph; the refusals."""
import numpy as np
import pytest
import torch

from oracle import checks as C
from oracle import sif_oracle as O
from tests import adapt_reference as A
from tests.conftest import rel_err
from tests.contract import L, S, run_contract, sifsr  # noqa: F401  (L and sifsr are the fixtures)
from tests.memcheck import bit_equal
from tests.test_model_gpu import TOL, make_model, read_masks

pytestmark = pytest.mark.gpu
MEAN, STD = A.MEAN, A.STD
ALPHA, GAMMA = 0.5, -0.25
F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64


def flat_params(sd):
    return torch.cat([sd[n].reshape(-1) for n in O.param_names()]).float()


def flat_running(sd):
    return torch.cat([torch.cat((sd[bn + ".running_mean"], sd[bn + ".running_var"])) for _, bn, _, _ in O.CONV_BN_LAYERS]).float()


def named(flat, like=None):
    out, off = {}, 0
    for n, shape, _ in O.state_dict_spec():
        if n in O.param_names():
            k = int(np.prod(shape))
            out[n] = flat[off:off + k].view(shape).cpu()
            off += k
    return out


def hip_run(L, sd, x, upstream, frozen=1, want_dx=True):
    """forward + backward through the C ABI on a workspace the test keeps: -> dict(sr, dx, grads (flat), masks, dsr).  `upstream`:
    dsr, or a function of the device sr returning it.  frozen=0: sifsr_model_forward in training mode, then sifsra_model_backward."""
    x = x.cuda().contiguous()
    B, _, H, W = x.shape
    fp, fr = flat_params(sd).cuda(), flat_running(sd).cuda()
    wsb = L.call("sifsra_model_workspace_bytes", B, H, W)
    ws = torch.empty(wsb // 4, dtype=F32, device="cuda")
    sr = torch.empty((B, 1, H, W), device="cuda")
    if frozen:
        L.call("sifsra_model_forward", x, sr, fp, fr, ws, wsb, B, H, W, 1e-5, S())
    else:
        L.call("sifsr_model_forward", x, sr, fp, fr.clone(), torch.zeros(17, dtype=I64, device="cuda"), ws, wsb, B, H, W, 1, 0.1, 1e-5, S())
    dsr = (upstream(sr) if callable(upstream) else upstream.cuda()).contiguous()
    grads = torch.empty_like(fp)
    dx = torch.empty_like(x) if want_dx else None
    ws_fwd = ws.clone()
    L.call("sifsra_model_backward", x, dsr, fp, grads, dx, ws, wsb, B, H, W, frozen, S())
    torch.cuda.synchronize()
    return dict(sr=sr, dx=dx, grads=grads, masks=read_masks(ws, B, H, W), dsr=dsr, ws=ws, ws_fwd=ws_fwd, wsb=wsb, fp=fp, x=x)


def loss_upstream(sifsr, kind, lst, ndvi):
    return lambda sr: sifsr.sif_loss_with_grad(kind, sr, lst.cuda(), ndvi.cuda().contiguous(), MEAN, STD, ALPHA, GAMMA)[3]


def loss_ref(kind, lst, ndvi):
    return lambda sr: O.LOSSES[kind](sr, lst.double(), ndvi.double(), MEAN, STD, ALPHA, GAMMA)


def assert_grads(tag, got_flat, got_dx, ref_g, ref_dx):
    g = named(got_flat)
    errs = {n: rel_err(g[n], ref_g[n]) for n in g}
    errs["dX"] = rel_err(got_dx, ref_dx)
    worst = max(errs, key=errs.get)
    print(f"[{tag}] worst rel err vs float64 at equal masks: {errs[worst]:.2e} ({worst}); dX {errs['dX']:.2e}")
    assert len(g) == 53
    for n, e in errs.items():
        assert e < TOL, (tag, n, e)


# ---- frozen forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frozen_forward_is_the_eval_forward_and_buffers_keep_their_bits(sifsr, shape):
    B, H, W = shape
    sd = O.synthetic_state(31)
    x, _, dsr = A.network_inputs(41, B, H, W)
    m = make_model(sifsr, sd).eval()
    with torch.no_grad():
        want = m(x.cuda())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with sifsr.adapt.frozen_bn(m):
        with torch.no_grad():
            assert torch.equal(m(x.cuda()), want)               # no backward to follow: the eval schedule itself
        xg = x.cuda().requires_grad_(True)
        sr = m(xg)                                              # sifsra_model_forward
        assert torch.equal(sr.detach(), want)
        sr.backward(dsr.cuda())
        assert xg.grad is not None and tuple(xg.grad.shape) == (B, 2, H, W) and m.flat_grad() is not None
    assert not m.training and m.bn_frozen is False
    for k, v in m.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(v, before[k]) and torch.equal(v.cpu(), sd[k]), k
        else:
            assert torch.equal(v, before[k]), k


# ---- frozen gradients ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", ["dsr", "sr2", "sr1"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frozen_gradients_vs_float64_at_equal_masks(sifsr, L, shape, upstream):
    B, H, W = shape
    sd = O.synthetic_state(32)
    x, lst, dsr = A.network_inputs(42 + B, B, H, W)
    ndvi = x[:, 1:2]
    up_dev = dsr if upstream == "dsr" else loss_upstream(sifsr, upstream, lst, ndvi)
    up_ref = dsr if upstream == "dsr" else loss_ref(upstream, lst, ndvi)
    r = hip_run(L, sd, x, up_dev)
    sr_ref, dx_ref, g_ref, _ = A.network_ref(sd, x, up_ref, training=False, masks=r["masks"])
    assert rel_err(r["sr"], sr_ref) < TOL
    assert_grads(f"frozen {B}x{H}x{W} {upstream}", r["grads"], r["dx"], g_ref, dx_ref)


def test_frozen_gradients_at_a_trained_operating_point(sifsr, L):
    import json, os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_weight_stats_v1.json")) as f:
        stats = json.load(f)["checkpoints"]
    sd = O.matched_state(stats[sorted(stats)[0]], 7)
    B, H, W = 2, 32, 48
    x, lst, dsr = A.network_inputs(77, B, H, W)
    r = hip_run(L, sd, x, dsr)
    sr_ref, dx_ref, g_ref, _ = A.network_ref(sd, x, dsr, training=False, masks=r["masks"])
    assert rel_err(r["sr"], sr_ref) < TOL
    assert_grads("frozen matched_state 2x32x48", r["grads"], r["dx"], g_ref, dx_ref)


# ---- training-mode dX ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 32, 48), (3, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_training_mode_input_gradient(sifsr, L, shape):
    B, H, W = shape
    sd = O.synthetic_state(33)
    x, _, dsr = A.network_inputs(52, B, H, W)
    r = hip_run(L, sd, x, dsr, frozen=0)
    # the parameter gradients and every workspace byte are sifsr_model_backward's; dx == NULL: the same call, bit for bit
    ws2, grads2 = r["ws_fwd"].clone(), torch.empty_like(r["grads"])
    L.call("sifsr_model_backward", r["x"], r["dsr"], r["fp"], grads2, ws2, r["wsb"], B, H, W, S())
    ws3, grads3 = r["ws_fwd"].clone(), torch.empty_like(r["grads"])
    L.call("sifsra_model_backward", r["x"], r["dsr"], r["fp"], grads3, None, ws3, r["wsb"], B, H, W, 0, S())
    torch.cuda.synchronize()
    assert torch.equal(grads2, r["grads"])
    assert torch.equal(grads3, grads2) and torch.equal(ws3.view(I32), ws2.view(I32))
    sr_ref, dx_ref, g_ref, _ = A.network_ref(sd, x, dsr, training=True, masks=r["masks"])
    assert rel_err(r["sr"], sr_ref) < TOL
    assert_grads(f"training {B}x{H}x{W}", r["grads"], r["dx"], g_ref, dx_ref)
    # ... and through the module: x.requires_grad in train() mode returns the same dX
    m = make_model(sifsr, sd).train()
    xg = x.cuda().requires_grad_(True)
    m(xg).backward(dsr.cuda())
    assert torch.equal(xg.grad, r["dx"]) and torch.equal(m.flat_grad(), r["grads"])


# ---- no cross-sample coupling, second stream ---------------------------------------------------------------------------------
def test_frozen_mode_does_not_couple_the_samples(sifsr, L):
    B, H, W = 3, 32, 48
    sd = O.synthetic_state(34)
    x, _, dsr = A.network_inputs(53, B, H, W)
    full = hip_run(L, sd, x, dsr)
    total = torch.zeros_like(full["grads"], dtype=F64)
    for b in range(B):
        one = hip_run(L, sd, x[b:b + 1], dsr[b:b + 1])
        assert rel_err(full["sr"][b:b + 1], one["sr"]) < TOL and rel_err(full["dx"][b:b + 1], one["dx"]) < TOL
        total += one["grads"].double()
    g, s = named(full["grads"]), named(total)
    for n in g:
        assert rel_err(g[n], s[n]) < TOL, n


def test_second_stream_changes_no_bit(sifsr, L):
    B, H, W = 1, 64, 96
    sd = O.synthetic_state(35)
    x, _, dsr = A.network_inputs(54, B, H, W)
    try:
        L.call("sifsr_set_wgrad_stream", 1)
        a = hip_run(L, sd, x, dsr)
        L.call("sifsr_set_wgrad_stream", 0)
        b = hip_run(L, sd, x, dsr)
    finally:
        L.call("sifsr_set_wgrad_stream", -1)
    assert torch.equal(a["grads"], b["grads"]) and torch.equal(a["dx"], b["dx"])


# ---- operator level ------------------------------------------------------------------------------------------------------------
def run_op(L, ops, B, H, W):
    g, y, scale, shift, coef, w = (t.cuda() for t in ops)
    dx = torch.full((B, 2, H, W), float("nan"), device="cuda")
    L.call("sifsra_conv_in_dgrad", g, y, scale, shift, coef, w, dx, B, H, W, S())
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", A.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_in_dgrad(L, hw, B):
    H, W = hw
    ops = A.op_inputs(100 + H * W + B, B, H, W)
    ref = A.conv_in_dgrad_ref(*ops)
    got = run_op(L, ops, B, H, W)
    assert not torch.isnan(got).any()
    errs = {}
    for name, m in A.regions(H, W).items():
        assert m.any(), name
        errs[name] = rel_err(got.cpu()[:, :, m], ref[:, :, m])
    print(f"[conv_in_dgrad B={B} {H}x{W}] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < 1e-4, (name, e)
    assert torch.equal(run_op(L, ops, B, H, W), got)


# ---- memory contract -------------------------------------------------------------------------------------------------------------
def model_case(stage, with_dx=True, frozen=1, shape=(2, 32, 48)):
    def build(A_, L):
        B, H, W = shape
        sd = O.synthetic_state(36)
        x, _, dsr = A.network_inputs(55, B, H, W)
        xin, p = A_.input(x, "x"), A_.input(flat_params(sd), "params")
        wsb = L.call("sifsra_model_workspace_bytes", B, H, W)
        sr = A_.output((B, 1, H, W), F32, "sr")
        ws = A_.scratch(wsb, "workspace")
        if frozen:
            r = A_.input(flat_running(sd), "running")
            fwd = lambda: L.call("sifsra_model_forward", xin, sr, p, r, ws, wsb, B, H, W, 1e-5, S())
        else:
            r, nbt = A_.inout(flat_running(sd), "running"), A_.inout(torch.zeros(17, dtype=I64), "nbt")
            fwd = lambda: L.call("sifsr_model_forward", xin, sr, p, r, nbt, ws, wsb, B, H, W, 1, 0.1, 1e-5, S())
        if stage == "forward":
            return fwd, {"sr": sr}
        d = A_.input(dsr, "dsr")
        grads = A_.output((p.numel(),), F32, "grads")
        dx = A_.output((B, 2, H, W), F32, "dx") if with_dx else None

        def call():
            fwd()
            L.call("sifsra_model_backward", xin, d, p, grads, dx, ws, wsb, B, H, W, frozen, S())
        outs = {"sr": sr, "grads": grads}
        if with_dx:
            outs["dx"] = dx
        return call, outs
    return build


def op_case(B, H, W):
    def build(A_, L):
        g, y, scale, shift, coef, w = (A_.input(t, n) for t, n in zip(A.op_inputs(9, B, H, W), ("g", "y", "scale", "shift", "coef", "w")))
        dx = A_.output((B, 2, H, W), F32, "dx")
        return (lambda: L.call("sifsra_conv_in_dgrad", g, y, scale, shift, coef, w, dx, B, H, W, S())), {"dx": dx}
    return build


def targets_case(first, count, overlap=0, cover=False, n_override=None):
    def build(A_, L):
        _, _, filled, valid, active = A.granule_reference(A.WIN, overlap, cover)
        h, w = filled.shape
        T = len(A.origins(h, A.WIN, overlap, cover)) * len(A.origins(w, A.WIN, overlap, cover))
        act = np.full(T, -1, np.int32)
        act[:len(active)] = active
        n = len(active) if n_override is None else n_override
        f, v = A_.input(torch.from_numpy(filled), "filled"), A_.input(torch.from_numpy(valid), "valid")
        a, na = A_.input(torch.from_numpy(act), "active"), A_.input(torch.tensor([n], dtype=I32), "n_active")
        lo, vo = A_.output((count, 1, A.WIN, A.WIN), F32, "lst_out"), A_.output((count, 1, A.WIN, A.WIN), U8, "valid_out")
        nv = A_.output((1,), I64, "n_valid_out")
        call = lambda: L.call("sifsra_tile_targets", f, v, a, na, first, count, h, w, A.WIN, overlap, 1 if cover else 0, MEAN, STD, lo, vo, nv, S())
        return call, {"lst_out": lo, "valid_out": vo, "n_valid_out": nv}
    return build


CONTRACT = {"sifsra_model_forward": [model_case("forward"), model_case("forward", shape=(1, 24, 24))],
            "sifsra_model_backward": [model_case("backward", True), model_case("backward", False), model_case("backward", True, frozen=0),
                                      model_case("backward", True, shape=(1, 24, 24))],
            "sifsra_conv_in_dgrad": [op_case(3, 17, 33), op_case(1, 3, 3), op_case(1, 24, 40)],
            "sifsra_tile_targets": [targets_case(0, 4), targets_case(9, 5, 2, True), targets_case(0, 3, n_override=0)]}
CASES = [(name, i) for name, cases in CONTRACT.items() for i in range(len(cases))]


@pytest.mark.parametrize("name,idx", CASES, ids=[f"{n[7:]}-{i}" for n, i in CASES])
def test_memory_contract(L, name, idx):
    """every output written in full and nowhere else -- NaN-free under the NaN poison, bit-identical under every poison of the
    outputs AND the workspace (no workspace byte is read before it is written) --, const inputs untouched, and the same bits on
    ordinary allocations."""
    run_contract(L, lambda k: CONTRACT[name][idx](k.A, k.L), seed=0, capacity=96 << 20)     # (the cases are not seeded)


# ---- tile targets ----------------------------------------------------------------------------------------------------------------
def device_granule(sifsr, overlap, cover):
    lst, ndvi = A.make_granule()
    lst_d, ndvi_d = torch.from_numpy(lst).cuda(), torch.from_numpy(ndvi).cuda()
    filled, valid = sifsr.gaps.fill_gaps(lst_d)
    slot, active, n_active = sifsr.gaps.select_tiles(valid, A.WIN, overlap, cover)
    return lst_d, ndvi_d, filled, valid, slot, active, n_active


@pytest.mark.parametrize("overlap,cover", [(0, False), (2, False), (0, True), (2, True)])
def test_tile_targets_bit_equal_to_the_restatement(sifsr, overlap, cover):
    _, _, filled_r, valid_r, active_r = A.granule_reference(A.WIN, overlap, cover)
    empty, partly, full = A.tile_kinds(valid_r, A.WIN, overlap, cover)
    assert empty >= 1 and partly >= 1 and full >= 1
    _, _, filled, valid, _, active, n_active = device_granule(sifsr, overlap, cover)
    n = len(active_r)
    assert int(n_active) == n and np.array_equal(active[:n].cpu().numpy(), active_r)
    assert np.array_equal(filled.cpu().numpy().view(np.uint32), filled_r.view(np.uint32))
    for first, count in ((0, n), (n - 2, 5), (3, 1), (2 * n + 1, 3)):          # whole list; first + count > n_active; one; first > n
        tl, tv, nv = sifsr.adapt.tile_targets(filled, valid, active, n_active, first, count, A.STATS, A.WIN, overlap, cover)
        rl, rv, rn = A.tile_targets_ref(filled_r, valid_r, active_r, first, count, A.WIN, overlap, cover, MEAN, STD)
        assert tl.shape == (count, 1, A.WIN, A.WIN) and tl.dtype == F32 and tv.dtype == U8 and nv.dtype == I64 and nv.numel() == 1
        assert np.array_equal(tl.cpu().numpy().view(np.uint32), rl.view(np.uint32))
        assert np.array_equal(tv.cpu().numpy(), rv) and int(nv) == rn


# ---- adapt_granule -------------------------------------------------------------------------------------------------------------
LR, STEPS, BATCH = 1e-3, 3, 4


def test_adapt_granule_is_the_written_out_loop(sifsr):
    sd = O.synthetic_state(37)
    lst_d, ndvi_d, filled, valid, slot, active, n_active = device_granule(sifsr, 0, False)
    n = int(n_active)
    assert n % BATCH != 0 and STEPS * BATCH > n                                  # the third step wraps
    m = make_model(sifsr, sd).eval()
    p0 = m.flat_parameters().detach().clone()
    buffers = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    res = sifsr.adapt.adapt_granule(m, lst_d, ndvi_d, A.STATS, steps=STEPS, lr=LR, alpha=ALPHA, gamma=GAMMA, kind="sr2", batch=BATCH,
                                    window=A.WIN)
    assert res.n_active == n and tuple(res.losses.shape) == (STEPS, 3) and res.losses.is_cuda
    assert not m.training and m.bn_frozen is False                               # mode and attribute as they were
    # the loop, written out
    m2 = make_model(sifsr, sd)
    opt2 = sifsr.FlatAdam(m2.parameters(), lr=LR)
    x = sifsr.gaps.prepare_active_tiles(filled, ndvi_d, A.STATS, active, n_active, n, A.WIN, 0, False)
    m2.bn_frozen = True
    losses = []
    for i in range(STEPS):
        first = (i * BATCH) % n
        xb = x[[(first + j) % n for j in range(BATCH)]]
        tl, tv, nv = sifsr.adapt.tile_targets(filled, valid, active, n_active, first, BATCH, A.STATS, A.WIN, 0, False)
        losses.append(torch.stack(sifsr.train.train_step(m2, opt2, tl, xb[:, 0:1], xb[:, 1:2], A.STATS, ALPHA, GAMMA, "sr2", valid=tv,
                                                         n_valid=nv)).detach())
    assert torch.equal(res.losses, torch.stack(losses))
    assert torch.equal(m.flat_parameters(), m2.flat_parameters()) and not torch.equal(m.flat_parameters(), p0)
    assert torch.equal(res.optimizer._m, opt2._m) and torch.equal(res.optimizer._v, opt2._v) and res.optimizer._step == opt2._step == STEPS
    for k, v in m.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]) and torch.equal(v.cpu(), sd[k]), k
    # prediction with the adapted network = a fresh model loaded with its state_dict
    out = sifsr.predict.predict_granule_gaps(m, lst_d, ndvi_d, A.STATS, window=A.WIN, batch=BATCH, overlap=2, cover_edges=True)
    fresh = make_model(sifsr, {k: v.cpu() for k, v in m.state_dict().items()})
    assert bit_equal(out, sifsr.predict.predict_granule_gaps(fresh, lst_d, ndvi_d, A.STATS, window=A.WIN, batch=BATCH, overlap=2,
                                                             cover_edges=True))
    res.restore()
    assert torch.equal(m.flat_parameters(), p0)


def test_adapt_granule_all_invalid_takes_no_step_and_no_forward(sifsr):
    m = make_model(sifsr, O.synthetic_state(37)).eval()
    p0 = m.flat_parameters().detach().clone()
    calls = []
    h = m.register_forward_hook(lambda *a: calls.append(1))
    try:
        res = sifsr.adapt.adapt_granule(m, torch.zeros(A.GRANULE_HW, device="cuda"), torch.zeros((96, 128), device="cuda"), A.STATS,
                                        steps=STEPS, lr=LR, batch=BATCH, window=A.WIN)
    finally:
        h.remove()
    assert res.n_active == 0 and res.losses.shape[0] == 0 and not calls and torch.equal(m.flat_parameters(), p0)
    res.restore()
    assert torch.equal(m.flat_parameters(), p0)


@pytest.mark.parametrize("kind", ["sr2", "sr1"])
def test_first_adaptation_step_against_the_oracle(sifsr, L, kind):
    lst_d, ndvi_d, filled, valid, slot, active, n_active = device_granule(sifsr, 0, False)
    n = int(n_active)
    x_all = sifsr.gaps.prepare_active_tiles(filled, ndvi_d, A.STATS, active, n_active, n, A.WIN, 0, False)
    sd = A.calibrated_state(O.synthetic_state(38), x_all.cpu())     # running statistics that describe the granule (see there)
    m = make_model(sifsr, sd)
    p_before = m.flat_parameters().detach().clone()
    res = sifsr.adapt.adapt_granule(m, lst_d, ndvi_d, A.STATS, steps=1, lr=LR, alpha=ALPHA, gamma=GAMMA, kind=kind, batch=BATCH, window=A.WIN)
    p_after = m.flat_parameters().detach().clone()
    # the same batch through the C ABI, to read the masks the device forward took
    x = x_all[:BATCH]
    tl, tv, nv = sifsr.adapt.tile_targets(filled, valid, active, n_active, 0, BATCH, A.STATS, A.WIN, 0, False)
    up = lambda sr: sifsr.masked_sif_loss_with_grad(kind, sr, tl, tv, nv, x[:, 1:2].contiguous(), MEAN, STD, ALPHA, GAMMA)[3]
    r = hip_run(L, sd, x.cpu(), up, want_dx=False)
    losses_ref, g_ref, upd_ref, p_ref = A.masked_step_ref(sd, x.cpu(), tl.cpu(), tv.cpu(), kind, ALPHA, GAMMA, LR, masks=r["masks"])
    got = [float(v) for v in res.losses[0]]
    print(f"[{kind}] step 0 losses {got} | float64 {list(losses_ref)}")
    for a, b in zip(got, losses_ref):
        assert abs(a - b) < 1e-4 * abs(b), (kind, a, b)
    sig = C.significant_mask([g_ref], O.param_names())
    C.update_parity((p_after - p_before).double().cpu(), upd_ref, sig, p_after, p_ref, LR, 1, what=f"adapt {kind} step 0")


# ---- capture -------------------------------------------------------------------------------------------------------------------
def test_graph_captured_frozen_step(sifsr):
    B = 2
    m = make_model(sifsr, O.synthetic_state(39)).train()
    m.bn_frozen = True
    opt = sifsr.FlatAdam(m.parameters(), lr=LR, capturable=True)
    lst_s = torch.zeros(B, 1, 16, 16, device="cuda"); up_s = torch.zeros(B, 1, 64, 64, device="cuda"); nd_s = torch.zeros_like(up_s)

    def step():
        for p in m.parameters():
            p.grad = None
        sr = m(torch.cat((up_s, nd_s), 1))
        ds, pl, loss = sifsr.sif_loss("sr2", sr, lst_s, nd_s, MEAN, STD, ALPHA, GAMMA)
        loss.backward()
        opt.step()
        return loss.detach(), m.flat_grad()

    def load(seed):
        x, lst, _ = A.network_inputs(seed, B, 64, 64)
        lst_s.copy_(lst); up_s.copy_(x[:, 0:1]); nd_s.copy_(x[:, 1:2])

    load(61)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p0 = m.flat_parameters().detach().clone()
    buffers = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}

    def reset():
        with torch.no_grad():
            m.flat_parameters().copy_(p0)
            opt._m.zero_(); opt._v.zero_(); opt._step_dev.zero_()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = step()
    load(62)
    replays = []
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        replays.append((loss_g.clone(), grad_g.clone(), m.flat_parameters().detach().clone()))
    reset()
    loss_e, grad_e = step()
    torch.cuda.synchronize()
    for loss_r, grad_r, p_r in replays:
        assert torch.equal(loss_r, loss_e) and torch.equal(grad_r, grad_e) and torch.equal(p_r, m.flat_parameters())
    assert not torch.equal(m.flat_parameters(), p0)
    for k, v in m.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(sifsr):
    m = make_model(sifsr, O.synthetic_state(40))
    x = torch.randn(1, 2, 24, 24, device="cuda")
    m.compute_dtype = "bf16"
    m.train()
    with pytest.raises(sifsr.SifsrError):                       # a requested dX in bf16 mode
        m(x.clone().requires_grad_(True))
    with pytest.raises(sifsr.SifsrError):
        sifsr.adapt.input_gradient(m, x)
    m.bn_frozen = True
    with pytest.raises(sifsr.SifsrError):                       # frozen statistics in bf16 mode
        m(x)
    m.compute_dtype = "fp32"
    m.bn_frozen = False
    m.eval()
    y = m(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):                    # eval-mode backward stays refused
        y.sum().backward()
    m.bn_frozen = True                                          # ... whatever the attribute says
    y = m(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        y.sum().backward()


def test_input_gradient_leaves_the_model_alone(sifsr, L):
    sd = O.synthetic_state(32)
    B, H, W = 2, 40, 56
    x, _, dsr = A.network_inputs(42 + B, B, H, W)
    m = make_model(sifsr, sd).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    dx = sifsr.adapt.input_gradient(m, x.cuda(), dsr.cuda())
    r = hip_run(L, sd, x, dsr)
    assert torch.equal(dx, r["dx"])
    ones = sifsr.adapt.input_gradient(m, x.cuda())
    assert torch.equal(ones, hip_run(L, sd, x, torch.ones_like(dsr))["dx"])
    assert not m.training and m.flat_grad() is None and all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
