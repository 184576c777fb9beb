"""Float64 CPU restatement of LPIPS-VGG16 (lpips.py:226-292, :351-358 as called at model_perf_aster_formatds.py:134, :405-410) and a
closed-form generator of VGG16-shaped weights -- what tests/test_lpips_host.py and tests/test_lpips_gpu.py hold the device code to.

The restatement returns the five layer terms AND their sum: the deep layers are a few percent of the sum, so a test on the sum
alone would not see a broken 512-channel layer.  tests/golden/make_golden_lpips.py asserts that its sum equals the reference's own
ContentLoss on the same weights (to fp32 rounding) and stores the float64 terms.

The generator uses no library RNG: an integer hash (splitmix64 on the element index) -> U(-a, a) with a = sqrt(6 / (9 cin)) for the
conv weights (He scaling: the activations neither die nor explode over 13 layers), +-0.1 for the biases, (0, 10 / C) for the linear
weights.  The 59 MB of weights are rebuilt identically on any machine (WEIGHTS_SHA256) and never committed."""
import functools
import hashlib
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_lpips_v1.npz")
CONV_MODULES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
POOL_AFTER = (1, 3, 6, 9)                 # conv indices followed (after their ReLU) by MaxPool2d(2, 2)
TAP_AFTER = (1, 3, 6, 9, 12)              # conv indices whose ReLU output is a tap: modules 3, 8, 15, 22, 29
TAP_CHANNELS = (64, 128, 256, 512, 512)
EPS = 1e-10
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
WEIGHTS_SHA256 = "d6a59580303e9bac1a829463a0c51db82b31c7218a449626967cdeef2b4869a6"   # of vgg_flat() + lin_flat() as float32 bytes


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def hash_uniform(n, salt):
    """n values in (0, 1), float64: splitmix64 of (index + salt * golden ratio), the top 53 bits + 1/2 ulp"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


@functools.lru_cache(maxsize=1)
def weights():
    """-> ([(w (co,ci,3,3), b (co,)) x 13], [lin (C,) x 5]) float32 numpy"""
    vgg = []
    for l, (ci, co) in enumerate(CONV_CHANNELS):
        a = np.sqrt(6.0 / (9 * ci))
        w = ((2 * hash_uniform(co * ci * 9, 2 * l + 1) - 1) * a).astype(np.float32).reshape(co, ci, 3, 3)
        b = ((2 * hash_uniform(co, 2 * l + 2) - 1) * 0.1).astype(np.float32)
        vgg.append((w, b))
    lin = [(hash_uniform(c, 100 + k) * (10.0 / c)).astype(np.float32) for k, c in enumerate(TAP_CHANNELS)]
    return vgg, lin


def vgg_flat():
    return np.concatenate([np.concatenate((w.reshape(-1), b)) for w, b in weights()[0]])


def lin_flat():
    return np.concatenate(weights()[1])


def weights_sha256():
    return hashlib.sha256(vgg_flat().tobytes() + lin_flat().tobytes()).hexdigest()


def state_dicts(prefix="features."):
    """the weights as a torchvision-style state dict and piq's list of five (1,C,1,1) tensors"""
    vgg, lin = weights()
    sd = {}
    for m, (w, b) in zip(CONV_MODULES, vgg):
        sd[f"{prefix}{m}.weight"], sd[f"{prefix}{m}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    return sd, [torch.from_numpy(v).reshape(1, -1, 1, 1) for v in lin]


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def features(x, vgg=None, dtype=torch.float64):
    """x (N,3,H,W), already standardised -> the five tap tensors (ReLU outputs of modules 3, 8, 15, 22, 29)"""
    vgg = weights()[0] if vgg is None else vgg
    taps = []
    for l, (w, b) in enumerate(vgg):
        x = torch.relu(torch.nn.functional.conv2d(x, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), padding=1))
        if l in TAP_AFTER:
            taps.append(x)
        if l in POOL_AFTER:
            x = torch.nn.functional.max_pool2d(x, 2, 2)
    return taps


def terms(x, y, mean=IMAGENET_MEAN, std=IMAGENET_STD, vgg=None, lin=None, dtype=torch.float64):
    """x, y (N,3,H,W) float32 numpy -> (N,6) float64: d_1 .. d_5 and their sum.  dtype float32: what the reference does today."""
    lin = weights()[1] if lin is None else lin
    m = torch.tensor(mean, dtype=dtype).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=dtype).view(1, 3, 1, 1)
    with torch.no_grad():
        fx = features((torch.from_numpy(np.ascontiguousarray(x)).to(dtype) - m) / s, vgg, dtype)
        fy = features((torch.from_numpy(np.ascontiguousarray(y)).to(dtype) - m) / s, vgg, dtype)
        cols = []
        for a, b, w in zip(fx, fy, lin):
            a = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + EPS)
            b = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + EPS)
            cols.append((((a - b) ** 2) * torch.from_numpy(w).to(dtype).view(1, -1, 1, 1)).mean(dim=[2, 3]).sum(dim=1))
        d = torch.stack(cols, dim=1).double()
    return torch.cat((d, d.sum(dim=1, keepdim=True)), dim=1).numpy()


def normalise_pair(a, b):
    """model_perf_aster_formatds.py:373-374, :407-408 in float32: (N,H,W) x2 -> (N,3,H,W) x2, mini (N,), maxi (N,)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    mini = np.minimum(a.min(axis=(1, 2)), b.min(axis=(1, 2)))
    maxi = np.maximum(a.max(axis=(1, 2)), b.max(axis=(1, 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = [np.repeat(((v - mini[:, None, None]) / (maxi - mini)[:, None, None]).astype(np.float32)[:, None], 3, axis=1) for v in (a, b)]
    return t[0], t[1], mini, maxi


def pair_terms(a, b, **kw):
    x, y, _, _ = normalise_pair(a, b)
    return terms(x, y, mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], **kw)


# ---- closed-form test images -----------------------------------------------------------------------------------------------------
def smooth(N, H, W, seed):
    """(N,H,W) float64 in [0, 1]: a few sinusoids whose phases and frequencies come from the hash"""
    u = hash_uniform(N * 12, 1000 + seed).reshape(N, 3, 4)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((N, H, W))
    for k in range(3):
        fy, fx, ph, am = (u[:, k, j][:, None, None] for j in range(4))
        out += (0.5 + am) * np.sin(2 * np.pi * ((0.5 + 2.5 * fy) * yy / 16.0 + (0.5 + 2.5 * fx) * xx / 16.0 + ph))
    lo, hi = out.min(axis=(1, 2), keepdims=True), out.max(axis=(1, 2), keepdims=True)
    return (out - lo) / (hi - lo)


def images(N, H, W, seed, noise=0.05):
    """x, y (N,3,H,W) float32 in [0, 1]: smooth channels, y = x + 5 % uniform noise (clipped)"""
    x = smooth(3 * N, H, W, seed).reshape(N, 3, H, W)
    n = 2 * hash_uniform(x.size, 2000 + seed).reshape(x.shape) - 1
    return x.astype(np.float32), np.clip(x + noise * n, 0, 1).astype(np.float32)


def rasters(N, H, W, seed, noise=0.05):
    """a, b (N,H,W) float32, Kelvin-like: a = 290 + 20 smooth, b = a + noise of 5 % of the range"""
    a = 290.0 + 20.0 * smooth(N, H, W, 50 + seed)
    n = 2 * hash_uniform(a.size, 3000 + seed).reshape(a.shape) - 1
    return a.astype(np.float32), (a + 20.0 * noise * n).astype(np.float32)


# the value cases of tests/test_lpips_gpu.py: (N, H, W).  A feature map with min(h, w) < 16 runs through the direct kernel, so which
# layers reach the MFMA kernel -- and its slices of 128 output channels (cout = 256: 2 slices, 512: 4) -- follows from the size:
#   (1,16,16)    relu5_3 is 1 x 1; MFMA for conv1 only
#   (2,17,31)    odd; (1,41,43) the ASTER minimum, odd, floor pooling at every level; MFMA for conv1 (41 x 43: and conv2, 20 x 21)
#   (2,48,80)    several tiles per image on conv1 / conv2 (64 and 128 output channels, one launch each); conv3 .. conv5 (12 x 20, 6 x 10,
#                3 x 5) are direct: NO slice is taken at this size
#   (1,32,32)    the relu2_2 map is 16 x 16, exactly at the threshold (the smallest map the MFMA kernel takes); (1,30,34): 15 x 17, direct
#   (1,128,128)  conv3 at 32 x 32 (2 slices, 8 or 16 input-channel blocks) and conv4 at 16 x 16 (4 slices, 16 or 32 blocks) on MFMA
#   (1,256,256)  every layer on MFMA, conv5 (512 -> 512, 4 slices) at 16 x 16: the size of the reference's ASTER set
VALUE_SHAPES = ((1, 16, 16), (2, 17, 31), (1, 41, 43), (2, 48, 80), (1, 32, 32), (1, 30, 34), (1, 128, 128), (1, 256, 256))
FLOOR = 1e-7        # every term of every non-identical case is at least this (tests/test_lpips_host.py): no layer passes as 0 = 0


@functools.lru_cache(maxsize=None)
def value_case(shape):
    """-> (x, y, want (N,6)) for the three-channel call and (a, b, want) for the pairs call, computed once"""
    N, H, W = shape
    x, y = images(N, H, W, seed=H * 100 + W)
    a, b = rasters(N, H, W, seed=H * 100 + W)
    return (x, y, terms(x, y)), (a, b, pair_terms(a, b))
