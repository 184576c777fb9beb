"""The two full-size workloads against the float64 oracle: the benchmark's training step (SR2, batch 64 of 256 x 256) in its
backward, and BASELINE config 4 (the eval forward replayed from a hipGraph) at its real batch of 256.

At batch 64 the fused 16 -> 16 backward walks 64 tiles per workgroup, the Winograd weight-gradient slabs and their batched
reductions run at full size and the backward uses both streams with one early slab reduction per encoder stage -- none of which
the B <= 8 checks of tests/test_model_gpu.py reach.  Every weight gradient sums over 64 images, so one wrong 16 x 16 tile moves
a layer's gradient by ~1/16,384 of its size, far under the 1e-4 bar: the per-image probes take the backward of one image at a
time (at fixed ReLU masks the backward is linear in d loss / d sr), where the same tile is worth ~1/256.

The probes are harder for fp32 arithmetic than the full step: the fp32 CPU oracle, printed beside each HIP error, sits at ~1e-3
on some level-0 / level-1 weight gradients of a probe, while the HIP kernels stay at ~2e-6 (measured on an MI355X).

Host cost: one float64 forward graph of the oracle at batch 64, kept alive only for the probes inside one fixture, and float64
eval forwards at batch 256 -- about 5 minutes and 54 GB peak RSS for the module on a 16-CPU host; each module-scoped result keeps
only gradients and outputs."""
import copy
import gc
import json
import os
import resource
import time

import pytest
import torch

from oracle import sif_oracle as O
from tests.conftest import rel_err
from tests.test_model_gpu import (MEAN, STD, TOL, make_model, normalised_per_image_err, oracle_eval_y, per_image_rel_err,
                                  read_masks)

pytestmark = pytest.mark.gpu

B, HR = 64, 256
ALPHA, GAMMA = 0.5, -0.25
PROBES = (0, 29, 63)          # first, one in between, last image of the batch


@pytest.fixture(scope="module")
def sifsr():
    import sifsr as pkg
    assert torch.cuda.is_available()
    return pkg


@pytest.fixture(scope="module", autouse=True)
def report_host_cost():
    """The module's wall time and peak host RSS (the float64 oracle dominates both), printed when it ends."""
    t0 = time.time()
    yield
    print(f"\n[test_full_size_gpu] wall {time.time() - t0:.0f} s, peak host RSS {_rss_gb():.1f} GB")


def _rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20


def _split(flat, shapes):
    out, off = {}, 0
    flat = flat.detach().cpu()
    for n, shp in shapes.items():
        k = int(torch.Size(shp).numel())
        out[n] = flat[off:off + k].view(shp)
        off += k
    assert off == flat.numel()
    return out


def _hip_side(sifsr, sd, lst, lst_up, ndvi):
    """The benchmark step through the C ABI with the workspace kept: forward, sif_ops.sif_loss_with_grad (the loss op
    train.train_step seeds the backward with), backward -- with the second stream (default) and forced off -- then one
    forward + backward per probe image, the forward re-run before each backward so no backward reads a workspace an earlier
    backward changed."""
    from sifsr import _lib as L
    m = make_model(sifsr, sd).train()
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    x = torch.cat((lst_up, ndvi), 1).cuda()
    fp, fr, fn = m._flat_state(x.device)
    wsb = L.call("sifsr_model_workspace_bytes", B, HR, HR, 1)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device="cuda")
    sr = torch.empty(B, 1, HR, HR, device="cuda")
    S = torch.cuda.current_stream().cuda_stream

    def forward():
        L.call("sifsr_model_forward", x, sr, fp, fr, fn, ws, wsb, B, HR, HR, 1, 0.1, 1e-5, S)

    def backward(dsr):
        grads = torch.zeros_like(fp)
        L.call("sifsr_model_backward", x, dsr.contiguous(), fp, grads, ws, wsb, B, HR, HR, S)
        torch.cuda.synchronize()
        return grads

    res = {}
    forward()
    torch.cuda.synchronize()
    sr0 = sr.clone()
    res["sr"] = sr0.cpu()
    res["masks"] = read_masks(ws, B, HR, HR)
    msd = m.state_dict()
    res["bn"] = {k: v.detach().cpu().clone() for k, v in msd.items() if k.endswith(("running_mean", "running_var"))}
    ds, pl, loss, dsr = sifsr.sif_ops.sif_loss_with_grad("sr2", sr, lst.cuda(), ndvi.cuda(), MEAN, STD, ALPHA, GAMMA)
    dsr = dsr.clone()
    res["losses"] = (float(ds), float(pl), float(loss))
    res["dsr"] = dsr.cpu()
    g_two = backward(dsr)
    try:
        L.call("sifsr_set_wgrad_stream", 0)
        forward()
        assert torch.equal(sr, sr0), "the training forward is not bit-reproducible"
        g_one = backward(dsr)
    finally:
        L.call("sifsr_set_wgrad_stream", -1)
    res["grads"] = _split(g_two, shapes)
    res["grads_single_stream"] = _split(g_one, shapes)
    res["probes"] = {}
    for b in PROBES:
        dsr_b = torch.zeros_like(dsr)
        dsr_b[b] = dsr[b]
        forward()
        assert torch.equal(sr, sr0), "the training forward is not bit-reproducible"
        res["probes"][b] = _split(backward(dsr_b), shapes)
    del ws, x, fp, fr, fn, sr, sr0
    torch.cuda.empty_cache()
    return res


def _oracle_side(sd, lst, lst_up, ndvi, masks, dsr_hip, dtype):
    """One forward of the oracle at the HIP masks (oracle.RELU_MASKS) in ``dtype``, its graph kept for: the losses and
    d loss / d sr, the 53 parameter gradients of the loss, and one vector-Jacobian product per probe image with the probe's
    d loss / d sr (the HIP one, masked to image b: both sides get the same upstream gradient)."""
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = O.param_names()
    O.RELU_MASKS = masks
    try:
        sr, leaves = O.forward_with_leaves(sdd, lst_up.to(dtype), ndvi.to(dtype))
    finally:
        O.RELU_MASKS = None
    ds, pl, loss = O.sr2_loss(sr, lst.to(dtype), ndvi.to(dtype), MEAN, STD, ALPHA, GAMMA)
    *g, dsr = torch.autograd.grad(loss, leaves + [sr], retain_graph=True)
    res = {"sr": sr.detach(), "losses": (float(ds.detach()), float(pl.detach()), float(loss.detach())), "dsr": dsr.detach(), "grads": dict(zip(names, g)),
           "bn": {k: v for k, v in sdd.items() if k.endswith(("running_mean", "running_var"))}, "probes": {}}
    for b in PROBES:
        dsr_b = torch.zeros_like(sr)
        dsr_b[b] = dsr_hip[b].to(dtype)
        res["probes"][b] = dict(zip(names, torch.autograd.grad(sr, leaves, dsr_b, retain_graph=True)))
    del sr, leaves, ds, pl, loss, g
    gc.collect()
    return res


@pytest.fixture(scope="module")
def bench_step(sifsr):
    """HIP and oracle (float64, and fp32 for the yardstick) results of the benchmark step and its probes; the graphs are freed
    before the tests run."""
    t0 = time.time()
    sd = O.synthetic_state(64)
    lst, lst_up, ndvi = O.synthetic_batch(1264, B)
    hip = _hip_side(sifsr, sd, lst, lst_up, ndvi)
    t_hip = time.time() - t0
    o64 = _oracle_side(copy.deepcopy(sd), lst, lst_up, ndvi, hip["masks"], hip["dsr"], torch.float64)
    t64 = time.time() - t0 - t_hip
    o32 = _oracle_side(copy.deepcopy(sd), lst, lst_up, ndvi, hip["masks"], hip["dsr"], torch.float32)
    del hip["masks"]
    gc.collect()
    print(f"\n[B=64 step] HIP {t_hip:.1f} s, float64 oracle {t64:.1f} s, fp32 oracle {time.time() - t0 - t_hip - t64:.1f} s; "
          f"peak host RSS so far {_rss_gb():.1f} GB")
    return hip, o64, o32


def test_bench_step_backward_vs_float64_oracle(bench_step):
    """The benchmark step end to end at the HIP masks: the forward, the losses and d loss / d sr of sif_loss_with_grad at 1e-4 (overall and
    per image), each of the 53 parameter gradients at 1e-4, the BatchNorm running buffers at 1e-5; gradients bit-identical
    with the second stream forced off."""
    hip, o64, o32 = bench_step
    assert rel_err(hip["sr"], o64["sr"]) < TOL
    for got, ref, name in zip(hip["losses"], o64["losses"], ("ds", "pl", "loss")):
        assert abs(got - ref) < TOL * abs(ref), (name, got, ref)
    e_dsr = rel_err(hip["dsr"], o64["dsr"])
    per_img = [rel_err(hip["dsr"][b], o64["dsr"][b]) for b in range(B)]
    e_hip = {n: rel_err(hip["grads"][n], o64["grads"][n]) for n in o64["grads"]}
    e_cpu = {n: rel_err(o32["grads"][n], o64["grads"][n]) for n in o64["grads"]}
    print(f"[B=64 step] dsr rel err {e_dsr:.2e} (worst image {max(per_img):.2e}); worst grad rel err vs float64 at equal masks: "
          f"HIP {max(e_hip.values()):.2e} ({max(e_hip, key=e_hip.get)}) | fp32 CPU oracle {max(e_cpu.values()):.2e}")
    assert e_dsr < TOL and max(per_img) < TOL, (e_dsr, per_img)
    assert len(e_hip) == 53
    for n in e_hip:
        assert e_hip[n] < TOL, (n, e_hip[n], e_cpu[n])
    for k, v in o64["bn"].items():
        assert rel_err(hip["bn"][k], v) < 1e-5, k
    for n in hip["grads"]:
        assert torch.equal(hip["grads"][n], hip["grads_single_stream"][n]), ("second stream changed a bit", n)


@pytest.mark.parametrize("b", PROBES)
def test_bench_step_per_image_probe_vs_float64_oracle(bench_step, b):
    """The backward of d loss / d sr restricted to image b (zero elsewhere): each of the 53 gradients at 1e-4 against the float64
    oracle's vector-Jacobian product with the same upstream gradient.  A wrong tile of image b is ~1/256 of these gradients."""
    hip, o64, o32 = bench_step
    e_hip = {n: rel_err(hip["probes"][b][n], o64["probes"][b][n]) for n in o64["probes"][b]}
    e_cpu = {n: rel_err(o32["probes"][b][n], o64["probes"][b][n]) for n in o64["probes"][b]}
    print(f"[B=64 probe image {b}] worst grad rel err vs float64: HIP {max(e_hip.values()):.2e} ({max(e_hip, key=e_hip.get)}) "
          f"| fp32 CPU oracle {max(e_cpu.values()):.2e}")
    for n in sorted(e_hip, key=e_hip.get, reverse=True)[:5]:
        print(f"    {n:42s} HIP {e_hip[n]:.2e} | fp32 CPU oracle {e_cpu[n]:.2e}")
    assert len(e_hip) == 53
    for n in e_hip:
        assert e_hip[n] < TOL, (n, e_hip[n], e_cpu[n])


def _weights(kind):
    if kind == "synthetic":
        return O.synthetic_state(64)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = json.load(open(os.path.join(here, "golden_real_v1.json")))["cases"]["matched_sr2"]
    st = json.load(open(os.path.join(here, "real_weight_stats_v1.json")))["checkpoints"]
    return O.matched_state(st[g["checkpoint"]], g["wseed"])


@pytest.mark.parametrize("weights", ["statistics_matched", "synthetic"])
def test_graphed_inference_at_batch_256(sifsr, weights):
    """BASELINE config 4 at its real batch: GraphedPredictor(m, 256) replays bit-equal to the eager predict_tiles(batch=256);
    every one of the 256 images on the network's own scale, (out - mean) / std against the float64 oracle's y, max error
    <= 1e-4 x max|y| of that image; a 200-image input through the same graph, its 200 images the same way."""
    sd = _weights(weights)
    stats = {"mean_lst": MEAN, "std_lst": STD}
    m = make_model(sifsr, sd).eval()
    gp = sifsr.predict.GraphedPredictor(m, 256, stats)
    for n, seed in ((256, 4256), (200, 4200)):
        lst, lst_up, ndvi = O.synthetic_batch(seed, n)
        out = gp(lst_up.cuda(), ndvi.cuda())
        assert out.shape == (n, 1, HR, HR)
        if n == 256:
            with torch.inference_mode():
                eager = sifsr.predict.predict_tiles(m, lst_up.cuda(), ndvi.cuda(), stats, batch=256)
            assert torch.equal(out, eager)
        err = normalised_per_image_err(out, oracle_eval_y(sd, lst_up, ndvi))
        line = f"[config 4, {weights} weights, n={n}] worst per-image error on y vs float64: HIP {float(err.max()):.2e}"
        if n == 256:
            err32 = per_image_rel_err(oracle_eval_y(sd, lst_up, ndvi, torch.float32), oracle_eval_y(sd, lst_up, ndvi))
            line += f" | fp32 CPU oracle {float(err32.max()):.2e}"
        print(line)
        assert err.shape == (n,) and float(err.max()) <= TOL, err
        gc.collect()
