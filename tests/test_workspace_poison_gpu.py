"""GPU: the engine's workspace contract.  ModelB_2's forward and backward run through the C ABI ("sifsr_model_forward",
"sifsr_model_backward", "sifsr_model_forward_ex", "sifsr_model_backward_ex") in a guarded arena (tests/memcheck.py): the workspace is a
payload of exactly sifsr_model_workspace_bytes bytes, sr / grads / running / nbt live in the arena too, x / params / dsr are
registered inputs.  The whole workspace is poisoned before the forward; before the backward everything the forward is documented
not to need is poisoned AGAIN -- [workspace_bytes(training = 0), workspace_bytes(training = 1)) and the forward's statistic-partials
scratch, which runs from the 256-byte-aligned end of U[2] (region 25 of sifsr_model_workspace_regions, 16 channels at full
resolution) to workspace_bytes(training = 0).  (engine.hip: every use the backward makes of that scratch starts with a kernel of the
backward writing it -- the tail reduction, bn_bwd_reduce, the fused 16 -> 16 kernel's and the upsample adjoint's rows; the forward's
statistics live on in mean / invstd / scale / shift.  The workspace holds floating-point data only -- fp32, bf16, the float64
coefficients -- and, behind `shift`, the 1 + B + 1024 int flag words of non-finite data (include/sifsr_hip.h), which the first launch
of the forward clears or writes before anything reads them and which are only ever compared with zero; no counters, indices or
addresses, so a poisoned value cannot steer an access.)

sr, the running statistics, nbt and all 282,705 gradients must be bit-identical under zeros, NaN and N(0,1) poison and NaN-free, no
guard byte may change, and x, params, dsr must come back untouched.  No tolerance anywhere; none of this needs the oracle."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests.memcheck import Arena, bit_equal, same_under_all_poisons

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPARAMS = 282705
_STATE = {}


def _lib():
    import sifsr  # noqa: F401
    from sifsr import _lib as L
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return L


def _state():
    """seeded parameters / running statistics / counters of a ModelB_2, on the host"""
    if not _STATE:
        import sifsr
        torch.manual_seed(5)
        m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1).cuda().train()
        fp, fr, fn = m._flat_state(torch.device("cuda", 0))
        assert fp.numel() == NPARAMS and fn.dtype == torch.int64
        _STATE.update(params=fp.detach().cpu().clone(), running=fr.detach().cpu().clone(), nbt=fn.detach().cpu().clone())
    return _STATE


def _batch(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 2, H, W, generator=g)
    dsr = torch.randn(B, 1, H, W, generator=g) / (B * H * W)
    return x, dsr


def engine_run(L, poison, B, H, W, train=True, compute=0, warm=False):
    """One step (eval forward, or training forward + backward) on a poisoned workspace.  warm: a step with ANOTHER batch runs first
    in the same workspace, which is then NOT poisoned again (the production pattern: the caching allocator hands back last step's
    block); the running statistics and counters are reset in between so that both variants compute the same step."""
    st = _state()
    S = torch.cuda.current_stream().cuda_stream
    wsb = L.call("sifsr_model_workspace_bytes", B, H, W, 1 if train else 0)
    fwd_end = L.call("sifsr_model_workspace_bytes", B, H, W, 0)
    assert wsb > 0 and wsb % 256 == 0 and 0 < fwd_end <= wsb
    A = Arena("cuda", poison=poison, capacity=wsb + B * H * W * 4 * 8 + NPARAMS * 8 + (32 << 20))
    x_cpu, dsr_cpu = _batch(B, H, W, 1000 + B + H + W)
    x, params = A.input(x_cpu, "x"), A.input(st["params"], "params")
    running, nbt = A.inout(st["running"], "running"), A.inout(st["nbt"], "nbt")
    sr = A.output((B, 1, H, W), torch.float32, "sr")
    ws = A.scratch(wsb, "workspace")
    if train:
        dsr, grads = A.input(dsr_cpu, "dsr"), A.output((NPARAMS,), torch.float32, "grads")
        reg = (ctypes.c_size_t * 56)()
        assert L.call("sifsr_model_workspace_regions", B, H, W, reg, 56) == 56
        # regions are y[17], P[3], R[3], U[3], ...: index 25 = U[2], uc[2] = 16 channels at level 0 (engine.hip sifsr_layout:
        # `w.U[k] = take(uc[k] * N[2 - k])`), directly followed by `w.partials = take(maxpart)` and `w.fwd_end = off`
        part_lo = ((reg[25] + 16 * B * H * W) * 4 + 255) // 256 * 256       # the 256-byte-aligned end of U[2]
        assert reg[25] * 4 < part_lo < fwd_end and all(r * 4 < part_lo for r in list(reg)[:26])

    def step(xx, first):
        if compute == 0:
            L.call("sifsr_model_forward", xx, sr, params, running, nbt, ws, wsb, B, H, W, 1 if train else 0, 0.1, 1e-5, S)
        else:
            L.call("sifsr_model_forward_ex", xx, sr, params, running, nbt, ws, wsb, B, H, W, 1 if train else 0, 0.1, 1e-5, compute, S)
        torch.cuda.synchronize()
        A.check()
        if not train:
            return
        if first:
            A.repoison(ws, fwd_end, wsb)       # what a training forward without a backward is documented not to need ...
            A.repoison(ws, part_lo, fwd_end)   # ... and the forward's partials scratch
        if compute == 0:
            L.call("sifsr_model_backward", xx, dsr, params, grads, ws, wsb, B, H, W, S)
        else:
            L.call("sifsr_model_backward_ex", xx, dsr, params, grads, ws, wsb, B, H, W, compute, S)
        torch.cuda.synchronize()
        A.check()

    if warm:
        x_warm = A.input(_batch(B, H, W, 77)[0], "x_warm")
        step(x_warm, True)
        running.copy_(st["running"].cuda())
        nbt.copy_(st["nbt"].cuda())
        step(x, False)                         # same workspace, not poisoned again
    else:
        step(x, True)
    out = {"sr": sr.clone(), "running": running.clone(), "nbt": nbt.clone()}
    if train:
        out["grads"] = grads.clone()
    del A
    return out


def check_config(L, B, H, W, **kw):
    res = same_under_all_poisons(lambda p: engine_run(L, p, B, H, W, **kw))
    if kw.get("train", True):
        assert res["grads"].numel() == NPARAMS and float(res["grads"].abs().max()) > 0
        assert int(res["nbt"].min()) == int(_state()["nbt"].min()) + 1
    return res


@pytest.fixture(scope="module")
def L():
    return _lib()


@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (1, 24, 24), (3, 48, 80)])
def test_eval_forward(L, B, H, W):
    check_config(L, B, H, W, train=False)


# 256 x 256: batch 2 is below the two-stream threshold (2 * 65,536 pixels); 3 and 8 use the second stream, the fused 16 -> 16
# kernels and the early slab reductions.  The others are the DESIGN §5 shapes with partial tiles and odd deeper levels, where the
# tap-domain fallbacks run.
@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (3, 256, 256), (8, 256, 256), (2, 128, 384), (2, 64, 64), (2, 48, 80), (2, 40, 72),
                                   (2, 24, 24)])
def test_train_forward_backward(L, B, H, W):
    check_config(L, B, H, W)


@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (2, 48, 80)])
def test_bf16_mode(L, B, H, W):
    check_config(L, B, H, W, compute=1)
    check_config(L, B, H, W, compute=1, train=False)


@pytest.mark.parametrize("B,compute", [(2, 0), (3, 0), (2, 1)])
def test_second_step_into_the_same_workspace(L, B, compute):
    """last step's data at the same offsets: right to a few percent, so no parity test can see a kernel that reads it"""
    fresh = check_config(L, B, 256, 256, compute=compute)
    reused = check_config(L, B, 256, 256, compute=compute, warm=True)
    for k in fresh:
        assert bit_equal(fresh[k], reused[k]), f"{k}: a step depends on what the previous step left in the workspace"


# ---- the A/B switches (read once per process): the batch-3 comparison in a process of its own per switch ----------------------
WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["SIFSR_ROOT"])
import torch
from tests import test_workspace_poison_gpu as T
L = T._lib()
fresh = T.check_config(L, 3, 256, 256)
reused = T.check_config(L, 3, 256, 256, warm=True)
assert all(T.bit_equal(fresh[k], reused[k]) for k in fresh), "depends on the previous step's workspace"
print("POISON-OK")
'''

SWITCHES = [{"SIFSR_WGRAD_WINO": "0"}, {"SIFSR_NO_WINO8": "1"}, {"SIFSR_NO_WINO": "1"}, {"SIFSR_WGRAD_STREAM": "0"},
            {"SIFSR_NO_BWD16": "1"}, {"SIFSR_TAIL_APPLY": "1"}, {"SIFSR_HEAD_LINEAR": "1"}, {"SIFSR_DBG_POOL_ON_LOAD": "0"}]


def test_every_switch(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    report = {}
    for env in SWITCHES:
        tag = ",".join(f"{k}={v}" for k, v in env.items())
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, SIFSR_ROOT=ROOT, **env), capture_output=True,
                           text=True, timeout=600)
        ok = r.returncode == 0 and "POISON-OK" in r.stdout
        report[tag] = "pass" if ok else "FAIL: " + (r.stdout[-500:] + r.stderr[-1500:])
        print(f"[workspace poison] {tag}: {'pass' if ok else 'FAIL'}")
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            break                              # a crashed worker: start nothing more on the device
    failed = {k: v for k, v in report.items() if v != "pass"}
    assert not failed and len(report) == len(SWITCHES), failed
