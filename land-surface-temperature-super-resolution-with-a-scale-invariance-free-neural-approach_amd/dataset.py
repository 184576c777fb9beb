"""Synthetic drop-in for the reference's ``dataset.ModisDatasetB`` (dataset.py:29-142).

The reference reads GeoTIFF pairs listed in ``data/ModisDatasetB.csv`` and ``data/statistics.json``
(neither is shipped, and GDAL/OpenCV are not installed here -- SURVEY.md §0), so this class keeps
the constructor signature, ``__len__``, the ``.stats`` dict and the ``__getitem__`` contract
  (lst (1,64,64), lst_up (1,256,256), ndvi (1,256,256)) float32 numpy, z-scored ('norm')
and fills them with seeded synthetic data of BASELINE.md §3: lst ~ N(0,1), ndvi ~ N(0,1) clipped to
+-3, lst_up = bicubic x4 of lst.  (The reference uses cv2.INTER_CUBIC for lst_up; OpenCV is absent,
so that resampler is 'parity unpinned' -- here lst_up is F.interpolate(bicubic, align_corners=False).)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from . import _lib

# statistics of the 83 shipped MODIS/ASTER test pairs (SURVEY.md §8 c), used as synthetic constants
DEFAULT_STATS = {"mean_lst": 307.2378, "std_lst": 5.5698, "mean_ndvi": 0.6452, "std_ndvi": 0.1683}


class ModisDatasetB(Dataset):
    def __init__(self, csv_path=None, transf="norm", split="Train", time="Both", length=16, seed=1234, hr=256):
        if transf != "norm":
            raise NotImplementedError("only transf='norm' (z-score, dataset.py:134-139) is provided")
        self.csv_path, self.transf, self.split, self.time = csv_path, transf, split, time
        self.stats = dict(DEFAULT_STATS)
        self.length, self.seed, self.hr = int(length), int(seed), int(hr)

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if idx < 0 or idx >= self.length:
            raise IndexError(idx)
        rs = np.random.RandomState(self.seed + 7919 * int(idx) + (0 if self.split == "Train" else 104729))
        lr = self.hr // 4
        lst = rs.standard_normal((lr, lr)).astype(np.float32)
        ndvi = np.clip(rs.standard_normal((self.hr, self.hr)), -3, 3).astype(np.float32)
        lst_up = F.interpolate(torch.from_numpy(lst)[None, None], scale_factor=4, mode="bicubic",
                               align_corners=False)[0, 0].numpy()
        return np.expand_dims(lst, 0), np.expand_dims(lst_up, 0), np.expand_dims(ndvi, 0)


class ModisDatasetB_scale_invariance(ModisDatasetB):
    """Synthetic drop-in for ``dataset.ModisDatasetB_scale_invariance`` (dataset.py:145-263): same constructor
    and ``.stats``; ``__getitem__`` returns (lst_4km_up (1,64,64), ndvi_1km (1,64,64), lst (1,64,64)) computed from
    the synthetic (lst, ndvi) pair exactly as dataset.py:256-263 does (bicubic /4 of NDVI without blur, norm-L4
    decimation of the de-normalised LST, bicubic x4 back, re-normalisation), with torch CPU ops."""

    def __getitem__(self, idx):
        lst, _, ndvi = super().__getitem__(idx)
        lst_t, ndvi_t = torch.from_numpy(lst)[None], torch.from_numpy(ndvi)[None]
        nd = F.interpolate(F.pad(ndvi_t, (4, 4, 4, 4), mode="reflect"), scale_factor=0.25, mode="bicubic")[:, :, 1:-1, 1:-1]
        k = lst_t * self.stats["std_lst"] + self.stats["mean_lst"]
        k = k.unfold(3, 4, 4).unfold(2, 4, 4).pow(4).sum((-1, -2)).div(16).pow(0.25)
        up = F.interpolate(k, scale_factor=4, mode="bicubic", align_corners=False)
        up = (up - self.stats["mean_lst"]) / self.stats["std_lst"]
        return up[0].numpy(), nd[0].numpy(), lst


class MinedDataset(Dataset):
    """The ``ModisDatasetB`` contract over patches mined from real granules (``sifsr.products.PatchMiner``): ``__len__``, the
    ``.stats`` dict (``statistics.json`` of the TRAINING split, data_preparation.py:69-105, whatever `split` this dataset serves)
    and ``__getitem__`` -> (lst (1,w,w), lst_up (1,4w,4w), ndvi (1,4w,4w)) float32 numpy, z-scored (dataset.py:134-142), so that
    ``train.fit`` takes it unchanged.  The patches are copied to the host once, here; lst_up is the same bicubic as the synthetic
    classes'.  For training at device rate use ``MinedPatches.loader`` instead.

    ``masked`` (patches mined with coverage > 0): items of five, (lst, lst_up, ndvi, valid (1,w,w) uint8, count
    int64) -- lst is the z-scored FILLED patch (``MinedPatches.fill``), count the number of its valid pixels; the default collate
    gives a (b,) count vector, which ``train.train_epoch`` / ``eval_epoch`` sum on the device.  The default ``stats`` are then
    ``mined.statistics("Train", valid_only=True)``."""

    def __init__(self, mined, split="Train", stats=None, masked=False):
        if getattr(mined, "hr", 4 * mined.window) != 4 * mined.window:
            raise _lib.SifsrError(f"MinedDataset is the host path at x4 (a CPU bicubic of scale 4): patches of window {mined.window} and "
                                  f"hr {mined.hr} go through MinedPatches.loader / masked_loader and rloss.train_epoch")
        self.split, self.masked = split, bool(masked)
        self.stats = dict(stats) if stats is not None else mined.statistics("Train", valid_only=self.masked)
        rows = mined.rows(split)
        sel = torch.from_numpy(np.ascontiguousarray(rows)).to(mined.lst.device)
        self.index = mined.index[rows]
        if self.masked:
            mined.fill()
            self._valid = mined.valid.index_select(0, sel).cpu()
            self._count = mined.valid_moments[rows, 0].astype(np.int64)
        self._lst = (mined.filled if self.masked else mined.lst).index_select(0, sel).cpu()
        self._ndvi = mined.ndvi.index_select(0, sel).cpu()

    def __len__(self):
        return int(self._lst.shape[0])

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        st = self.stats
        lst = (self._lst[idx:idx + 1] - st["mean_lst"]) / st["std_lst"]
        ndvi = (self._ndvi[idx] - st["mean_ndvi"]) / st["std_ndvi"]
        lst_up = F.interpolate(lst, scale_factor=4, mode="bicubic", align_corners=False)[0]
        if self.masked:
            return lst[0].numpy(), lst_up.numpy(), ndvi.numpy(), self._valid[idx].numpy(), self._count[idx]
        return lst[0].numpy(), lst_up.numpy(), ndvi.numpy()


def synthetic_device_batch(batch, device, seed=1234, hr=256):
    """BASELINE.md §3 bench inputs, generated once on the device: (lst, lst_up, ndvi)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    lr = hr // 4
    lst = torch.randn((batch, 1, lr, lr), generator=g)
    ndvi = torch.randn((batch, 1, hr, hr), generator=g).clamp_(-3, 3)
    lst_up = F.interpolate(lst, scale_factor=4, mode="bicubic", align_corners=False)
    return lst.to(device), lst_up.contiguous().to(device), ndvi.to(device)
