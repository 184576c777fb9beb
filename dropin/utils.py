"""``import utils as us`` (train_model_B_gradFTM.py:29, predict.py:16) -- an overlay with every ``us.*`` name the three
training scripts use, the hot-path ones on MI355X:

  us.downscale_LST_SR_to_LR, us.get_output_ftm     utils.py:1671, :1833   -> gfx950 kernels (autograd-capable)
  us.generate_psf_kernel                           utils.py:1615          -> host, float64 -> fp32 (as the reference)
  us.psnr_skimage, us.ssim_skimage                 utils.py:548-578       -> device kernel; accept the numpy arrays the
                                                                             scripts pass (.detach().cpu().numpy()) or tensors
  us.gssim                                         utils.py:1904-2005     -> device kernel (sifsr.metrics.aster_metrics)
  us.model_checkpoint                              utils.py:667-714       -> sifsr.train.ModelCheckpoint
  us.read_JsonA/B/C, us.save_model, us.load_model  utils.py:718-826       -> plain host code
  us.upsampling                                    utils.py:163-180       -> bicubic x scale, OpenCV INTER_CUBIC semantics
                                                                             (A = -0.75, half-pixel centres, edge clamp)
  us.TsHARP, us.ATPRK, us.AATPRK                   utils.py:1213-1253, :1588-1606 -> device kernels + host variogram fit
                                                                             (sifsr.baselines); 2-D numpy in, float64 numpy out
  us.downscale_Aster_to_coarse, us.downscale_Aster_to_fine, us.generic_downscale   utils.py:1759-1830, :1642-1668 -> device kernels
                                                                             (sifsr.degrade): the sensor model at any ratio
  us.DMS                                           data_mining_sharpener_modified.py as model_perf_aster_formatds.py:220-250
                                                                             calls it -> device kernels (sifsr.baselines.dms)

GeoTIFF / HDF I/O, the file interface of the DMS sharpener and the plotting helpers (GDAL, OpenCV, rasterio: not installed, out of scope --
SURVEY.md §2) raise ``NotImplementedError`` naming what was asked for.
"""
import json
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import sifsr  # noqa: E402
from sifsr import metrics as _metrics  # noqa: E402
from sifsr.sif_ops import downscale_LST_SR_to_LR, get_output_ftm, psf_taps_1d  # noqa: E402,F401
from sifsr.train import ModelCheckpoint as model_checkpoint  # noqa: E402,F401

json_load = json.load          # model_perf_aster_formatds.py uses us.json_load


def generate_psf_kernel(res, mtf_res, mtf_fc, half_kernel_width=None):
    """utils.py:1615-1639: the (2h+1)^2 Gaussian PSF as float32 (outer product of the normalised 1-D taps)."""
    t = psf_taps_1d(mtf_fc, mtf_res / res, half_kernel_width)
    return np.outer(t, t).astype(np.float32)


def _dev_pair(predictions, targets):
    dev = torch.device("cuda", torch.cuda.current_device())
    as_t = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float32).contiguous()
    return as_t(predictions), as_t(targets)


def psnr_skimage(predictions, targets):
    """utils.py:548-552 -> float (batch mean)."""
    return float(_metrics.psnr_ssim(*_dev_pair(predictions, targets))[0])


def ssim_skimage(predictions, targets):
    """utils.py:554-578 -> float (batch mean)."""
    return float(_metrics.psnr_ssim(*_dev_pair(predictions, targets))[1])


def gssim(im1, im2, win_size=7, data_range=None, grad_comp_type=1):
    """utils.py:1904-2005 -> float, computed on the GPU (the GSSIM column of sifsr.metrics.aster_metrics).  im1, im2: (H,W)
    float32 numpy arrays (or device tensors), H, W >= 16; ``grad_comp_type`` is accepted and ignored, as in the reference."""
    if data_range is None:
        raise TypeError("gssim: data_range=None is not supported (the reference computes K1 * None and fails)")
    if win_size != 7:
        raise NotImplementedError("gssim: only win_size=7 (the reference's default) has a gfx950 kernel")
    for name, im in (("im1", im1), ("im2", im2)):
        if isinstance(im, torch.Tensor) and not im.is_cuda:
            raise sifsr.SifsrError(f"gssim: {name} is on {im.device}; pass a numpy array or a device tensor")
    a, b = _dev_pair(im1, im2)
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"gssim: two 2-D images of the same shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return float(_metrics.aster_metrics(a[None, None], b[None, None], data_range=float(np.float32(data_range)))[0, 6])


def upsampling(img, scale):
    """utils.py:163-180 (``cv2.resize(..., INTER_CUBIC)``): numpy (h,w) -> numpy (h*scale[0], w*scale[1]), same dtype."""
    from sifsr import pipeline
    if scale[0] != 4 or scale[1] != 4:
        raise NotImplementedError("only the x4 bicubic of the hot path (dataset.py:140, predict.py:97) is implemented")
    a = np.asarray(img)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return pipeline.bicubic_up4(t[None, None])[0, 0].cpu().numpy().astype(a.dtype, copy=False)


def _sharpen_args(name, temp_coarse, index_coarse, index_fine, scale, block_size=5):
    if scale != 4:
        raise NotImplementedError(f"{name}: only scale=4 (the paper's 1 km -> 250 m) has a gfx950 kernel, got scale={scale}")
    if block_size != 5:
        raise NotImplementedError(f"{name}: only block_size=5 (the reference's default) has a gfx950 kernel, got block_size={block_size}")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = []
    for what, a in (("temp_coarse", temp_coarse), ("index_coarse", index_coarse), ("index_fine", index_fine)):
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError(f"{name}: {what} must be a 2-D array, got shape {a.shape}")
        out.append(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)[None, None])
    return out


def TsHARP(temp_coarse, index_coarse, index_fine, scale, min_T=285, path_image=False):
    """utils.py:1213-1231 -> (4h,4w) float64 numpy.  ``path_image`` is accepted and ignored (the reference's writer is commented out)."""
    from sifsr import baselines
    lst, nc, nf = _sharpen_args("TsHARP", temp_coarse, index_coarse, index_fine, scale)
    return baselines.tsharp(lst, nc, nf, min_T=min_T)[0, 0].cpu().numpy().astype(np.float64)


def ATPRK(temp_coarse, index_coarse, index_fine, scale, scc, block_size=5, sill=7, ran=1000, min_T=285, path_image=False):
    """utils.py:1234-1253 -> (4h,4w) float64 numpy; ``path_image`` accepted and ignored."""
    from sifsr import baselines
    lst, nc, nf = _sharpen_args("ATPRK", temp_coarse, index_coarse, index_fine, scale, block_size)
    return baselines.atprk(lst, nc, nf, scc=scc, sill=sill, ran=ran, min_T=min_T)[0, 0].cpu().numpy().astype(np.float64)


def AATPRK(temp_coarse, index_coarse, index_fine, scale, scc, b_radius=2, block_size=5, sill=7, ran=1000, min_T=285, path_image=False):
    """utils.py:1588-1606 -> (4h,4w) float64 numpy; ``path_image`` accepted and ignored."""
    from sifsr import baselines
    lst, nc, nf = _sharpen_args("AATPRK", temp_coarse, index_coarse, index_fine, scale, block_size)
    return baselines.aatprk(lst, nc, nf, scc=scc, b_radius=b_radius, sill=sill, ran=ran,
                            min_T=min_T)[0, 0].cpu().numpy().astype(np.float64)


def DMS(temp_coarse, index_fine, scale, n_estimators=10, seed=0):
    """The DMS sharpener on arrays instead of GeoTIFF files: global NDVI -> LST bagged trees with per-leaf ridge regression and
    the T^4 residual correction -> (4h,4w) float64 numpy.  Deterministic for a given ``seed`` (the reference's is not)."""
    from sifsr import baselines
    if scale != 4:
        raise NotImplementedError(f"DMS: only scale=4 (the paper's 1 km -> 250 m) has a gfx950 kernel, got scale={scale}")
    dev = torch.device("cuda", torch.cuda.current_device())
    args = []
    for what, a in (("temp_coarse", temp_coarse), ("index_fine", index_fine)):
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError(f"DMS: {what} must be a 2-D array, got shape {a.shape}")
        args.append(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)[None, None])
    return baselines.dms(*args, n_estimators=n_estimators, seed=seed)[0, 0].cpu().numpy().astype(np.float64)


def _same(name, padding):
    if padding != "same":
        raise NotImplementedError(f"{name}: only padding='same' (what the reference runs with) has a gfx950 kernel, got {padding!r}")


def _aster(name, data, factor, mtf, padding, hkw):
    from sifsr import degrade
    _same(name, padding)
    a = np.asarray(data)
    if a.ndim != 2:
        raise ValueError(f"{name}: data must be a 2-D array, got shape {a.shape}")
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    return degrade.degrade(t, factor, mtf=mtf, hkw=hkw).cpu().numpy()


def downscale_Aster_to_coarse(data, factor=926.25 / 90, mtf=0.1, padding="same", hkw=None):
    """utils.py:1759-1793: 2-D numpy (90 m) -> 2-D float32 numpy (926.25 m)."""
    return _aster("downscale_Aster_to_coarse", data, factor, mtf, padding, hkw)


def downscale_Aster_to_fine(data, factor=231.656 / 90, mtf=0.1, padding="same", hkw=None):
    """utils.py:1796-1830: 2-D numpy (90 m) -> 2-D float32 numpy (231.656 m)."""
    return _aster("downscale_Aster_to_fine", data, factor, mtf, padding, hkw)


def generic_downscale(data, factor=2.0, mtf=0.1, padding="same", hkw=3):
    """utils.py:1642-1668: (B,C,H,W) device tensor -> device tensor."""
    from sifsr import degrade
    _same("generic_downscale", padding)
    return degrade.degrade(data, factor, mtf=mtf, hkw=hkw)


def _read(file, keys):
    with open(file) as f:
        data = json.load(f)
    return tuple(data[k] for k in keys)


def read_JsonA(file):
    """utils.py:718-739."""
    return _read(file, ("dataset_parameter", "modelA_parameters", "hyperparameters", "save_parameters", "device"))


def read_JsonC(file):
    """utils.py:767-787."""
    return _read(file, ("dataset_parameter", "modelC_parameters", "hyperparameters", "save_parameters", "device"))


def read_JsonB(file):
    """utils.py:741-764: (dataset_parameter, modelA_parameters, modelB_parameters, hyperparameters, save_parameters, device)."""
    return _read(file, ("dataset_parameter", "modelA_parameters", "modelB_parameters", "hyperparameters", "save_parameters", "device"))


def save_model(model, path, model_name):
    """utils.py:802-826: the state_dict AND the whole module, as the reference does."""
    torch.save(model.state_dict(), os.path.join(path, model_name + "_state_dict.pt"))
    torch.save(model, os.path.join(path, model_name + ".pt"))


def load_model(model, state_dict_file, device="cpu"):
    """utils.py:791-800."""
    model.load_state_dict(torch.load(state_dict_file, map_location=torch.device(device), weights_only=True))


class OutOfScopeAttribute(AttributeError, NotImplementedError):
    """Raised for names of the reference's utils.py that the MI355X build does not provide.  An AttributeError, so that
    ``hasattr``, ``from utils import *`` (which probes ``__all__``) and ``inspect`` see an ordinary missing attribute; also a
    NotImplementedError, for callers that catch that."""


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    raise OutOfScopeAttribute(
        f"utils.{name}: not part of the SIF-CNN-SR hot path (GDAL / OpenCV / rasterio I/O, the file interface of DMS and plots "
        "are out of scope of the MI355X build, SURVEY.md §2); use the reference's own utils.py for it")
