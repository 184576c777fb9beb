"""From the raw integer rasters of a MODIS granule to training patches and ``statistics.json``, on the device:

    us.read_LST / us.read_NIRRED scaling, us.compute_NDVI                  utils.py:338, :428-435, :71; predict.py:76-78
    process_MOD21A1D / process_MOD11A1: the fill-pixel test per window     process_modis.py:88-112, :172-183
    find_corresponding_NDVI: zero-denominator rejection, NDVI, clip         process_modis.py:281-305
    the 60/40 split and statistics.json over the training split            data_preparation.py:32-39, :83-102

Reading the HDF files is not here (it needs GDAL): the entry points take the arrays ANY reader returns -- LST as uint16 (h,w), its
QC byte as uint8 (h,w), NIR and Red as int16 (4h,4w) -- as device tensors, or as NumPy arrays that are copied to the device.  The
data-sized work is four HIP kernels (include/sifsr_products.h, csrc/products.hip): decode, census, select, gather.  What is left is
64 bytes per patch and stays on the HOST in float64: the split labels and the merge of the per-patch moments with Chan's formula,
in patch order.

Transfers: `PatchMiner.add` has none (everything is enqueued on the current stream into buffers sized for the granule's full
windows); `PatchMiner.finish` reads each granule's accepted count, index and moment rows back once.  CPU-only use raises
SifsrError: there is no fallback.

Partly valid patches (`PatchMiner(coverage > 0)`; include/sifsr_masked.h): `fill_patches` / `MinedPatches.fill` mark
the valid pixels of every patch, fill the others with a neutral local mean (the fill of `gaps.fill_gaps`, per patch) and return the
moments of the valid pixels; `statistics(valid_only=True)` merges those, and `masked_loader` yields the filled input with the mask
and the count of valid pixels for `train.train_step(..., valid, n_valid)`.

At a ratio other than x4 the miner is `sifsr.rproducts.PatchMiner`; it returns the `MinedPatches` of this module
with `hr` set, and `statistics`, `fill`, `loader` and `masked_loader` follow `hr`: the NDVI count of a patch, the resampler of
`lst_up` (`ratio.prepare_tiles`) and, for masked batches, the (2,) counts of `rloss.valid_counts` in place of the one count.

Window order and `k` are the reference generator's (us.split), see the header: on a square raster column blocks are outer, row
blocks inner, and the ragged edge windows are counted but never accepted.
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch

from . import _lib, pipeline, ratio

QC_MODES = {"MOD21A1D": 0, "MOD11A1": 1}
STAT_KEYS = ("maxi", "mini", "mean_lst", "std_lst", "mean_ndvi", "std_ndvi")


def _raster(a, dtype, what, device=None):
    """a device tensor of `dtype`, from a device tensor (checked) or a NumPy array (copied)"""
    if isinstance(a, np.ndarray):
        if a.dtype != np.dtype(str(dtype).replace("torch.", "")):
            raise _lib.SifsrError(f"{what} must be {dtype}, got {a.dtype}")
        if not torch.cuda.is_available():
            raise _lib.SifsrError(f"{what}: this package only runs on a ROCm GPU (gfx950); there is no CPU path.")
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device or "cuda")
    if not isinstance(a, torch.Tensor):
        raise _lib.SifsrError(f"{what} must be a tensor or a NumPy array, got {type(a).__name__}")
    if not a.is_cuda:
        raise _lib.SifsrError(f"{what} is on {a.device}: this package only runs on a ROCm GPU (gfx950); there is no CPU path.")
    if a.dtype != dtype:
        raise _lib.SifsrError(f"{what} must be {dtype}, got {a.dtype}")
    if a.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D raster, got {tuple(a.shape)}")
    return a.contiguous()


def _rasters(lst_raw, nir, red, qc=None):
    lst_raw = _raster(lst_raw, torch.uint16, "lst_raw")
    nir = _raster(nir, torch.int16, "nir", lst_raw.device)
    red = _raster(red, torch.int16, "red", lst_raw.device)
    h, w = lst_raw.shape
    if tuple(nir.shape) != (4 * h, 4 * w) or tuple(red.shape) != (4 * h, 4 * w):
        raise ValueError(f"nir and red must be exactly 4x the LST raster ({4 * h}, {4 * w}); got {tuple(nir.shape)}, {tuple(red.shape)}")
    if qc is not None:
        qc = _raster(qc, torch.uint8, "qc", lst_raw.device)
        if tuple(qc.shape) != (h, w):
            raise ValueError(f"qc {tuple(qc.shape)} does not match lst_raw {(h, w)}")
    return lst_raw, nir, red, qc, h, w


def window_counts(h, w, window=64):
    """(nwin, nfull): the steps of the reference's generator over an (h, w) raster and the full windows among them."""
    no, ni = -(-h // window), -(-w // window)
    return no * ni, min(no, w // window) * min(ni, h // window)


def decode(lst_raw, nir, red, clip=False):
    """-> (lst_k (h,w), ndvi (4h,4w)) float32 device tensors: Kelvin and NDVI as us.read_LST / us.read_NIRRED /
    us.compute_NDVI give them (0 / 0 is NaN, x / 0 is +-inf; `clip` leaves NaN), ready for `predict.predict_granule`."""
    lst_raw, nir, red, _, h, w = _rasters(lst_raw, nir, red)
    lst_k = torch.empty((h, w), dtype=torch.float32, device=lst_raw.device)
    ndvi = torch.empty((4 * h, 4 * w), dtype=torch.float32, device=lst_raw.device)
    _lib.call("sifsrp_decode", lst_raw, nir, red, lst_k, ndvi, h, w, 1 if clip else 0, _lib.stream_ptr(lst_raw.device))
    return lst_k, ndvi


def _patch_counts(valid, window, hr):
    """valid (N,1,w,w) or (N,w,w) uint8 on the device -> (N,2) int64 on the device, row n = {n1, n2} of patch n under an hr x hr
    patch (`sifsrn_patch_counts`; nothing is read back)"""
    counts = torch.empty((valid.shape[0], 2), dtype=torch.int64, device=valid.device)
    _lib.call("sifsrn_patch_counts", valid.contiguous(), counts, valid.shape[0], int(window), int(hr), _lib.stream_ptr(valid.device))
    return counts


def fill_patches(lst):
    """lst (N,1,w,w) or (N,w,w) [K], 4 <= w <= 64, w % 4 == 0 -> (filled like lst float32, valid like lst uint8 of 0 / 1,
    moments (N,5) float64 device tensor [count, mean, M2, min, max] over the valid pixels of each patch; an empty patch:
    [0, 0, 0, +inf, -inf]).  valid: finite and not 0 K; filled[n] is `gaps.fill_gaps(lst[n])` bit for bit (`sifsrm_patches_fill`:
    one workgroup per patch, nothing read back)."""
    _lib.require_gpu(lst, "lst patches")
    if lst.dim() not in (3, 4) or (lst.dim() == 4 and lst.shape[1] != 1) or lst.shape[0] < 1 or lst.shape[-1] != lst.shape[-2]:
        raise _lib.SifsrError(f"lst patches: expected (N,1,w,w) or (N,w,w), got {tuple(lst.shape)}")
    n, w = int(lst.shape[0]), int(lst.shape[-1])
    if w < 4 or w > 64 or w % 4:
        raise _lib.SifsrError(f"lst patches: the window must be a multiple of 4 in [4, 64], got {w}")
    filled = torch.empty_like(lst)
    valid = torch.empty(lst.shape, dtype=torch.uint8, device=lst.device)
    moments = torch.empty((n, 5), dtype=torch.float64, device=lst.device)
    _lib.call("sifsrm_patches_fill", lst, filled, valid, moments, n, w, _lib.stream_ptr(lst.device))
    return filled, valid, moments


class PatchMiner:
    """Collects the accepted (LST 1x`window`x`window`, NDVI 1x4`window`x4`window`) pairs of any number of granules.

    coverage: the accepted share of bad LST pixels per window (process_modis.py --coverage); a window is accepted when
    bad <= coverage * window**2 and no fine pixel has nir + red == 0.  qc_mode: 'MOD21A1D' (bad: raw == 0) or 'MOD11A1' (bad:
    raw == 0 or the lowest QC bit set; `qc` is then required)."""

    def __init__(self, window=64, coverage=0.0, qc_mode="MOD21A1D"):
        if qc_mode not in QC_MODES:
            raise ValueError(f"qc_mode must be one of {sorted(QC_MODES)}, got {qc_mode!r}")
        if window < 4 or window % 4:
            raise ValueError(f"window must be a positive multiple of 4, got {window}")
        if not 0.0 <= coverage <= 1.0:
            raise ValueError(f"coverage must be in [0, 1], got {coverage}")
        self.window, self.coverage, self.qc_mode = int(window), float(coverage), qc_mode
        self.max_bad = int(math.floor(self.coverage * self.window ** 2))    # count <= coverage * window**2 on an integer count
        self._granules = []

    def add(self, lst_raw, nir, red, qc=None, granule_id=None):
        """Enqueue census, select and gather of one granule on the current stream.  Returns the granule's device buffers (counts
        (nwin,2), index (nfull,3), n_accepted (1)) for inspection; nothing is read back here."""
        lst_raw, nir, red, qc, h, w = _rasters(lst_raw, nir, red, qc)
        mode = QC_MODES[self.qc_mode]
        if mode == 1 and qc is None:
            raise ValueError("qc_mode 'MOD11A1' needs the QC raster")
        ws = self.window
        if h < ws or w < ws:
            raise ValueError(f"the raster ({h}, {w}) is smaller than one window ({ws})")
        nwin, cap = window_counts(h, w, ws)
        dev, s = lst_raw.device, _lib.stream_ptr(lst_raw.device)
        g = {"id": len(self._granules) if granule_id is None else int(granule_id),
             "counts": torch.empty((nwin, 2), dtype=torch.int32, device=dev),
             "index": torch.empty((cap, 3), dtype=torch.int32, device=dev),
             "n_accepted": torch.empty((1,), dtype=torch.int32, device=dev),
             "lst": torch.empty((cap, 1, ws, ws), dtype=torch.float32, device=dev),
             "ndvi": torch.empty((cap, 1, 4 * ws, 4 * ws), dtype=torch.float32, device=dev),
             "moments": torch.empty((cap, 8), dtype=torch.float64, device=dev)}
        _lib.call("sifsrp_census", lst_raw, qc, nir, red, g["counts"], h, w, ws, mode, s)
        _lib.call("sifsrp_select", g["counts"], g["index"], g["n_accepted"], h, w, ws, self.max_bad, cap, s)
        _lib.call("sifsrp_gather", lst_raw, nir, red, g["index"], g["n_accepted"], g["lst"], g["ndvi"], g["moments"], h, w, ws, cap, s)
        self._granules.append(g)
        return g

    def finish(self):
        """-> MinedPatches of everything added so far, in the order added (one read-back of the count, index and moments per
        granule); the miner is empty afterwards."""
        lst, ndvi, index, moments = [], [], [], []
        for g in self._granules:
            n = int(g["n_accepted"].item())
            idx = g["index"][:n].cpu().numpy().astype(np.int64)
            index.append(np.concatenate([np.full((n, 1), g["id"], dtype=np.int64), idx], 1))
            moments.append(g["moments"][:n].cpu().numpy())
            lst.append(g["lst"][:n])
            ndvi.append(g["ndvi"][:n])
        self._granules = []
        ws = self.window
        if not lst:
            raise _lib.SifsrError("PatchMiner.finish: no granule was added")
        return MinedPatches(torch.cat(lst).contiguous(), torch.cat(ndvi).contiguous(),
                            np.concatenate(index).reshape(-1, 4), np.concatenate(moments).reshape(-1, 8), ws)


def merge_moments(count, mean, m2):
    """Chan's pairwise update over the rows, in order, float64: -> (count, mean, M2) of the union."""
    n, mu, s = 0.0, 0.0, 0.0
    for nb, mb, sb in zip(np.asarray(count, np.float64), np.asarray(mean, np.float64), np.asarray(m2, np.float64)):
        if nb == 0:
            continue
        tot = n + nb
        d = mb - mu
        mu = mu + d * (nb / tot)
        s = s + sb + d * d * n * (nb / tot)
        n = tot
    return n, mu, s


class MinedPatches:
    """lst (N,1,w,w) Kelvin and ndvi (N,1,hr,hr) in [-1,1], float32 device tensors; index (N,4) int64 [granule id, k, row0, col0];
    moments (N,8) float64 (the rows of sifsrp_gather); split: None until `assign_split`, then an (N,) array of 'Train' / 'Val'.
    `hr`: the side of the NDVI patch, None = 4 w (what `PatchMiner` mines; `rproducts.PatchMiner` sets another).
    After `fill()`: filled (N,1,w,w) float32 and valid (N,1,w,w) uint8 device tensors, valid_moments (N,5) float64 on the host
    ([count, mean, M2, min, max] over the valid pixels of each patch)."""

    def __init__(self, lst, ndvi, index, moments, window=64, hr=None):
        self.lst, self.ndvi, self.index, self.moments, self.window = lst, ndvi, index, moments, int(window)
        self.hr = 4 * self.window if hr is None else int(hr)
        if self.hr < self.window:
            raise _lib.SifsrError(f"MinedPatches: hr {hr} is smaller than the window {window}")
        self.split = None
        self.filled = self.valid = self.valid_moments = self._valid_counts = self._patch_counts = None

    def fill(self):
        """`fill_patches` over all patches, once: sets and caches `.filled`, `.valid`, `.valid_moments` (one read-back of 40 bytes
        per patch; the counts also stay on the device for the masked loader).  The fill is LR-only, whatever `hr`.  Returns self."""
        if self.filled is None:
            filled, valid, moments = fill_patches(self.lst)
            self._valid_counts = moments[:, 0].to(torch.int64)
            self.valid_moments = moments.cpu().numpy()
            self.filled, self.valid = filled, valid
        return self

    def patch_counts(self):
        """(N,2) int64 on the device, row n = {n1, n2} of patch n: its valid cells and the HR pixels of its hr x hr patch under
        them -- `rloss.valid_counts` of that patch alone (`sifsrn_patch_counts`), formed once after `fill()` and kept."""
        if self._patch_counts is None:
            self._patch_counts = _patch_counts(self.fill().valid, self.window, self.hr)
        return self._patch_counts

    def __len__(self):
        return int(self.index.shape[0])

    def assign_split(self, seed=42, proportions=(0.6, 0.4)):
        """data_preparation.py:32-39: random.seed(seed), then one choices(['Train', 'Val'], proportions) per pair, in pair order
        (a private random.Random: the same stream, the global generator untouched)."""
        rng = random.Random(seed)
        self.split = np.array([rng.choices(["Train", "Val"], list(proportions))[0] for _ in range(len(self))], dtype=object)
        return self.split

    def rows(self, split=None):
        """the patch numbers of `split` ('Train' / 'Val'; None: all), ascending"""
        if split is None:
            return np.arange(len(self))
        if self.split is None:
            self.assign_split()
        return np.nonzero(self.split == split)[0]

    def statistics(self, split="Train", valid_only=False):
        """statistics.json of data_preparation.py:85-102 over the patches of `split`: maxi, mini, mean_lst, std_lst, mean_ndvi,
        std_ndvi (population standard deviations, as np.std), merged from the per-patch moments.  `valid_only`: the four LST
        numbers over the VALID pixels only (the moments of `fill()`, merged in patch order as the others are) -- what patches
        mined with coverage > 0 need, whose 0 K pixels would otherwise count; the NDVI numbers are unchanged."""
        rows = self.rows(split)
        m = self.moments[rows]
        if m.shape[0] == 0:
            raise _lib.SifsrError(f"statistics: no patch in split {split!r}")
        n, mean_l, m2_l = merge_moments(m[:, 0], m[:, 1], m[:, 2])
        maxi, mini = float(m[:, 4].max()), float(m[:, 3].min())
        if valid_only:
            v = self.fill().valid_moments[rows]
            n, mean_l, m2_l = merge_moments(v[:, 0], v[:, 1], v[:, 2])
            if n == 0:
                raise _lib.SifsrError(f"statistics: no valid LST pixel in split {split!r}")
            maxi, mini = float(v[:, 4].max()), float(v[:, 3].min())
        if self.hr == 4 * self.window:
            n_ndvi = 16.0 * m[:, 0]
        else:                                                            # (hr / window)^2 count: hr^2 for a patch, in integers
            n_ndvi = (m[:, 0] * float(self.hr * self.hr)) / float(self.window * self.window)
        nn, mean_n, m2_n = merge_moments(n_ndvi, m[:, 5], m[:, 6])
        return {"maxi": maxi, "mini": mini, "mean_lst": float(mean_l),
                "std_lst": float(math.sqrt(m2_l / n)), "mean_ndvi": float(mean_n), "std_ndvi": float(math.sqrt(m2_n / nn))}

    def loader(self, split, batch, stats, shuffle=True, seed=0):
        return PatchLoader(self, split, batch, stats, shuffle, seed)

    def masked_loader(self, split, batch, stats, shuffle=True, seed=0):
        """`loader` for partly valid patches: a `PatchLoader(masked=True)` (`stats` should be `statistics(valid_only=True)`)."""
        return PatchLoader(self, split, batch, stats, shuffle, seed, masked=True)


class PatchLoader:
    """An iterable of device batches (lst_norm (b,1,w,w), lst_up (b,1,4w,4w), ndvi_norm (b,1,4w,4w)) -- what `train.train_epoch` /
    `train.eval_epoch` iterate over: lst_norm = (lst - mean_lst) / std_lst, lst_up its bicubic x4 (`pipeline.prepare_tiles`, the
    resampler of the whole package) and ndvi_norm = (ndvi - mean_ndvi) / std_ndvi.  Every epoch (every `iter`) draws a new seeded permutation.

    `masked`: batches of five, (lst_norm, lst_up, ndvi_norm, valid (b,1,w,w) uint8, n_valid): lst_norm is the z-scored FILLED patch
    (`MinedPatches.fill`), lst_up its bicubic x4, and n_valid a 0-d int64 device tensor, the number of valid LST pixels of the batch
    -- the sum of the selected rows' counts, formed on the device without a host read.

    `mined.hr != 4 * mined.window` (patches of `rproducts.PatchMiner`): lst_up is (b,1,hr,hr), the bicubic resampling of
    `ratio.prepare_tiles` / `ratio.upsample` -- the operator `ratio.predict_granule` feeds the network with --, and the fifth item
    of a masked batch is the int64 (2,) sum of the selected rows of `MinedPatches.patch_counts()`, equal to
    `rloss.valid_counts(valid, (hr, hr))` of the batch: what `rloss.train_step(..., valid=, counts=)` takes."""

    def __init__(self, mined, split, batch, stats, shuffle=True, seed=0, masked=False):
        self.mined, self.rows, self.batch, self.stats = mined, mined.rows(split), int(batch), dict(stats)
        self.shuffle, self.seed, self.epoch, self.masked = bool(shuffle), int(seed), 0, bool(masked)
        if self.batch < 1:
            raise ValueError(f"batch must be positive, got {batch}")
        self.x4 = mined.hr == 4 * mined.window
        if self.masked:
            mined.fill()
            if not self.x4:
                mined.patch_counts()

    def __len__(self):
        return -(-len(self.rows) // self.batch)

    def order(self, epoch):
        return np.random.RandomState(self.seed + epoch).permutation(self.rows) if self.shuffle else self.rows

    def __iter__(self):
        rows = self.order(self.epoch)
        self.epoch += 1
        m, st = self.mined, self.stats
        for a in range(0, len(rows), self.batch):
            sel = torch.from_numpy(np.ascontiguousarray(rows[a:a + self.batch])).to(m.lst.device)
            src = m.filled if self.masked else m.lst
            lst = (src.index_select(0, sel) - float(st["mean_lst"])) / float(st["std_lst"])
            ndvi = (m.ndvi.index_select(0, sel) - float(st["mean_ndvi"])) / float(st["std_ndvi"])
            x = (pipeline if self.x4 else ratio).prepare_tiles(lst, ndvi)   # unit statistics: channel 0 = bicubic of lst to (hr, hr)
            if self.masked:
                n_valid = m._valid_counts.index_select(0, sel).sum() if self.x4 else m.patch_counts().index_select(0, sel).sum(0)
                yield lst, x[:, 0:1].contiguous(), ndvi, m.valid.index_select(0, sel), n_valid
            else:
                yield lst, x[:, 0:1].contiguous(), ndvi
