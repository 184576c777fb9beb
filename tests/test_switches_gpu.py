"""The library's A/B switches select other kernels for the same maths: SIFSR_WGRAD_WINO=0 (tap-domain weight gradients),
SIFSR_NO_WINO8=1 (producer / consumer Winograd kernels for 32 / 64 output channels), SIFSR_NO_WINO=1 (tap-domain forward and
input gradients), SIFSR_NO_BWD16=1 / SIFSR_TAIL_APPLY=1 / SIFSR_HEAD_LINEAR=1 (round 3: the backward's fused kernels and their alternatives),
SIFSR_DBG_EARLY_REDUCE (when the weight-gradient slab reductions are issued), SIFSR_BF16_BWD16=1 (the fused kernel in bf16 mode).  The switches are read once per process, so each runs in its own process: the same seeded SR2 step must give
the same loss and gradients as the default configuration to fp32 rounding (the kernels differ in summation order only), and the
default itself is pinned to the oracle by tests/test_model_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, torch
sys.path.insert(0, os.environ["SIFSR_ROOT"])
import sifsr
torch.manual_seed(11)
dev = torch.device("cuda", 0)
model = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).to(dev)
model.compute_dtype = os.environ.get("SIFSR_TEST_COMPUTE", "fp32")
stats = dict(sifsr.dataset.DEFAULT_STATS)
lst, lst_up, ndvi = sifsr.dataset.synthetic_device_batch(3, dev, seed=21)
model.train()
sr = model(torch.cat((lst_up, ndvi), dim=1))
_, _, loss = sifsr.sif_loss("sr2", sr, lst, ndvi, stats["mean_lst"], stats["std_lst"], 0.5, -0.25)
loss.backward()
torch.cuda.synchronize()
torch.save({"loss": float(loss), "sr": sr.detach().cpu(), "grad": model.flat_grad().detach().cpu().clone(),
            "sizes": [p.numel() for p in model.parameters()]}, os.environ["SIFSR_OUT"])
'''


def _run(tmp_path, tag, extra_env):
    out = tmp_path / f"{tag}.pt"
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, SIFSR_ROOT=ROOT, SIFSR_OUT=str(out), **extra_env)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out, weights_only=True)


def test_kernel_switches_agree_with_the_default_configuration(tmp_path):
    ref = _run(tmp_path, "default", {})
    gmax = float(ref["grad"].abs().max())
    for tag, env in [("tap_wgrad", {"SIFSR_WGRAD_WINO": "0"}), ("no_wino8", {"SIFSR_NO_WINO8": "1"}),
                     ("no_wino", {"SIFSR_NO_WINO": "1"}), ("single_stream", {"SIFSR_WGRAD_STREAM": "0"}),
                     # round 3: separate input / weight gradient kernels for the 16 -> 16 layers; the tail's dL/dy stored by a
                     # second pass instead of recomputed in the fused kernel; the first layer's weight gradient in its linear form
                     ("no_bwd16", {"SIFSR_NO_BWD16": "1"}), ("tail_apply", {"SIFSR_TAIL_APPLY": "1"}),
                     ("head_linear", {"SIFSR_HEAD_LINEAR": "1"}), ("pool_stored", {"SIFSR_DBG_POOL_ON_LOAD": "0"})]:
        got = _run(tmp_path, tag, env)
        assert abs(got["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), tag
        assert float((got["sr"] - ref["sr"]).abs().max()) <= 1e-4 * float(ref["sr"].abs().max()), tag
        # gradients: a handful of ReLU decisions may flip when the forward kernels differ, so the bar is
        # on the bulk: relative L2 over all 282,705 parameters
        rel = float((got["grad"] - ref["grad"]).norm() / ref["grad"].norm())
        assert rel <= (1e-5 if tag in ("tap_wgrad", "single_stream", "no_bwd16", "tail_apply", "head_linear", "pool_stored") else 2e-3), (tag, rel)
        if tag == "single_stream":
            assert torch.equal(got["grad"], ref["grad"]), "the second stream must not change a bit"
        assert float((got["grad"] - ref["grad"]).abs().max()) <= 0.05 * gmax, tag


def test_early_reduce_schedules_are_bit_identical(tmp_path):
    """SIFSR_DBG_EARLY_REDUCE=0/1/2 move only WHEN the weight-gradient slab reductions are issued on the second stream (one batch
    at the end; + one before db1; + one after the decoder) against the default one per encoder stage: the same reductions of the
    same slabs, so loss and gradients must not change a bit.  The worker's batch 3 at 256 x 256 engages the second stream
    (B*H*W >= 2 * 65,536), which is what the schedules and their event waits act on."""
    ref = _run(tmp_path, "default", {})
    for v in ("0", "1", "2"):
        got = _run(tmp_path, f"early_reduce_{v}", {"SIFSR_DBG_EARLY_REDUCE": v})
        assert got["loss"] == ref["loss"], v
        assert torch.equal(got["sr"], ref["sr"]), v
        assert torch.equal(got["grad"], ref["grad"]), ("SIFSR_DBG_EARLY_REDUCE", v)


def test_bf16_fused_bwd16_switch(tmp_path):
    """bf16 mode with SIFSR_BF16_BWD16=1: the 16 -> 16 layers' backward in the fused kernel (fp32 Winograd arithmetic on the bf16
    values) instead of the separate bf16-MFMA kernels.  The forward is untouched, so loss and output must be bit-identical.  The
    gradients are two roundings of the same bf16 arithmetic, bounded as tests/test_bf16_gpu.py bounds the HIP bf16 step against
    its emulation: for each of the 53 parameter tensors, the relative L2 distance between the two bf16 runs is at most twice the
    distance of the default bf16 run from the fp32 run, + 2e-2."""
    f32 = _run(tmp_path, "fp32", {})
    ref = _run(tmp_path, "bf16", {"SIFSR_TEST_COMPUTE": "bf16"})
    got = _run(tmp_path, "bf16_bwd16", {"SIFSR_TEST_COMPUTE": "bf16", "SIFSR_BF16_BWD16": "1"})
    assert got["loss"] == ref["loss"] and torch.equal(got["sr"], ref["sr"])
    assert not torch.equal(ref["sr"], f32["sr"]), "the worker did not run the bf16 mode"
    sizes = ref["sizes"]
    assert len(sizes) == 53 and sum(sizes) == ref["grad"].numel()
    worst, worst_ref = 0.0, 0.0
    for a, b, c in zip(got["grad"].split(sizes), ref["grad"].split(sizes), f32["grad"].split(sizes)):
        e, e_r = float((a - b).norm() / b.norm()), float((b - c).norm() / c.norm())
        worst, worst_ref = max(worst, e), max(worst_ref, e_r)
        assert e < 2.0 * e_r + 2e-2, (e, e_r)
    print(f"bf16 fused 16 -> 16 backward: worst gradient relative L2 vs the default bf16 kernels {worst:.2e} | bf16 vs fp32 {worst_ref:.2e}")
