"""Bit-level fingerprint of the core path on finite data: one `name sha256` line per tensor.  Run it on two trees (or with
SIFSR_LIB on two builds) on the same device and diff the output: a change that claims to leave finite results alone must leave
every line alone.

    python tools/hash_core.py > hashes.txt

Covers: the eval forward at three shapes; the three losses, flat_grad() and the parameters, Adam moments and running statistics
after three training steps, for the SR2 and the SR1 loss; one bf16 step; one frozen-BatchNorm step with the input gradient; the
fused losses, Huber, and PSNR / SSIM on their own.  Seeded inputs and the oracle's synthetic state only."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sifsr  # noqa: E402
from oracle import sif_oracle as O  # noqa: E402

MEAN, STD, ALPHA, GAMMA = 307.2378, 5.5698, 0.5, -0.25
STATS = {"mean_lst": MEAN, "std_lst": STD}


def line(name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    print(f"{name} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def model(mode, compute="fp32"):
    m = sifsr.ModelB_2(2, [16, 32, 64, 128], "replicate", "ReLU", 1, 1)
    m.load_state_dict(O.synthetic_state(23))
    m = m.cuda()
    m.compute_dtype = compute
    if mode == "eval":
        return m.eval()
    m.train()
    m.bn_frozen = mode == "frozen"
    return m


def main():
    torch.cuda.set_device(0)
    m = model("eval")
    for B, H, W in ((2, 256, 256), (3, 48, 80), (1, 24, 24)):
        x = torch.from_numpy(np.random.RandomState(B + H + W).standard_normal((B, 2, H, W)).astype(np.float32)).cuda()
        with torch.inference_mode():
            line(f"eval_sr_{B}x{H}x{W}", m(x))
    for kind, compute, hr, B in (("sr2", "fp32", 256, 3), ("sr1", "fp32", 64, 2), ("sr2", "bf16", 64, 2)):
        m = model("train", compute)
        opt = sifsr.FlatAdam(m.parameters(), lr=1e-4)
        tag = f"{kind}_{compute}_{B}x{hr}"
        for step in range(3 if compute == "fp32" else 1):
            lst, lst_up, ndvi = (t.cuda() for t in O.synthetic_batch(50 + step, B, hr))
            out = sifsr.train.train_step(m, opt, lst, lst_up, ndvi, STATS, ALPHA, GAMMA, kind, return_sr=True)
            for n, t in zip(("ds", "pl", "loss", "sr"), out):
                line(f"{tag}_step{step}_{n}", t)
            line(f"{tag}_step{step}_flat_grad", m.flat_grad())
        line(f"{tag}_params", m.flat_parameters())
        line(f"{tag}_exp_avg", opt._m)
        line(f"{tag}_exp_avg_sq", opt._v)
        line(f"{tag}_running", m._flat_state(torch.device("cuda", 0))[1])
    m = model("frozen")
    lst, lst_up, ndvi = (t.cuda() for t in O.synthetic_batch(60, 2, 64))
    x = torch.cat((lst_up, ndvi), 1).requires_grad_(True)
    sr = m(x)
    ds, pl, loss, dsr = sifsr.sif_ops.sif_loss_with_grad("sr2", sr, lst, ndvi, MEAN, STD, ALPHA, GAMMA)
    sr.backward(dsr)
    for n, t in (("sr", sr), ("loss", loss), ("dsr", dsr), ("dx", x.grad), ("flat_grad", m.flat_grad())):
        line(f"frozen_2x64_{n}", t)
    # the operators on their own
    g = torch.Generator().manual_seed(9)
    sr = (torch.randn(2, 1, 40, 56, generator=g) * 1.3).cuda()
    lst, ndvi = torch.randn(2, 1, 10, 14, generator=g).cuda(), torch.randn(2, 1, 40, 56, generator=g).clamp(-3, 3).cuda()
    for kind in ("sr2", "sr1"):
        for n, t in zip(("ds", "pl", "loss", "dsr"), sifsr.sif_ops.sif_loss_with_grad(kind, sr, lst, ndvi, MEAN, STD, ALPHA, GAMMA)):
            line(f"sif_loss_{kind}_{n}", t)
        valid = (torch.rand(2, 1, 10, 14, generator=g) > 0.3).to(torch.uint8).cuda()
        for n, t in zip(("ds", "pl", "loss", "dsr"), sifsr.sif_ops.masked_sif_loss_with_grad(kind, sr, lst, valid, int(valid.sum()), ndvi,
                                                                                             MEAN, STD, ALPHA, GAMMA)):
            line(f"masked_sif_loss_{kind}_{n}", t)
        lst_r = torch.randn(2, 1, 16, 22, generator=g).cuda()
        for n, t in zip(("losses", "dsr"), sifsr.rloss.sif_loss_with_grad(kind, sr, lst_r, ndvi, 2.5, MEAN, STD, ALPHA, GAMMA)):
            line(f"ratio_sif_loss_{kind}_{n}", t)
    a = sr.clone().requires_grad_(True)
    h = sifsr.sif_ops.huber_loss(a, ndvi)
    h.backward()
    line("huber_value", h)
    line("huber_grad", a.grad)
    for n, t in zip(("psnr", "ssim"), sifsr.metrics.psnr_ssim(sr, ndvi)):
        line(n, t)


if __name__ == "__main__":
    main()
