"""MI355X-native (gfx950) implementation of the SIF-CNN-SR hot path.

Drop-in surface (SURVEY.md §8 b):
  model.ModelB_2                      <- reference model.py:533
  sif_ops.downscale_LST_SR_to_LR      <- reference utils.py:1671
  sif_ops.get_output_ftm              <- reference utils.py:1833
  sif_ops.sobel_bank / huber_loss / sif_loss  (fused forms of the train scripts' loss block)
  optim.FlatAdam                      <- torch.optim.Adam, train_model_B_gradFTM.py:453
  dataset.ModisDatasetB               <- reference dataset.py:29 (synthetic drop-in, same __getitem__)
  train.train_step / predict.predict_tiles  <- train_model_B_gradFTM.py:86-121 / predict.py:84-103
  pipeline.prepare_tiles / granule_to_tiles / tiles_to_granule, predict.predict_granule  <- dataset.py:134-142, predict.py:84-103
  metrics.psnr_skimage / ssim_skimage  <- utils.py:548-578 (on device)
  metrics.aster_metrics / gradient_strata  <- model_perf_aster_formatds.py:371-437 (per-pair table; us.gssim, utils.py:1904-2005)
  fourier.fft2_magnitude / attenuation_spectra / get_FRR / get_FRO / get_FRU  <- compare_methods.py:312-324, utils.py:598-662
  spectra.fft2_magnitude / attenuation_spectra / spectral_scores / summary_rows  <- compare_methods.py:305-417: the same for rasters
                                       of any size and lists of mixed sizes (chirp-z FFT, include/sifsr_spectra.h), the table's four
                                       spectral columns and the seven summary rows
  baselines.tsharp / atprk / aatprk    <- utils.py:1213-1253, :1588-1606 (the paper's comparison methods, on device)
  gaps.fill_gaps / select_tiles / predict_granule_gaps (also in predict)  <- no counterpart: cloud / ocean / fill pixels of a granule
                                       filled, all-gap tiles skipped, the output masked (include/sifsr_gaps.h)
  sif_ops.masked_sif_loss, products.fill_patches / MinedPatches.fill / masked_loader, train_step(valid=, n_valid=)  <- no counterpart:
                                       training on partly valid patches (PatchMiner(coverage > 0)): per-patch fill, statistics over
                                       valid pixels, a loss and gradient without the gap pixels (include/sifsr_masked.h)
  metrics.masked_aster_metrics / masked_psnr_ssim, train_epoch(masked_metrics=)  <- no counterpart: both metric sets over the valid
                                       pixels of rasters with gaps, a term counted iff its whole stencil is valid (include/sifsr_scores.h)
  lpips.LPIPS, metrics.aster_table     <- lpips.py:226-292, :351-358, model_perf_aster_formatds.py:134, :405-410: LPIPS-VGG16 on the device
                                       with weights the caller supplies (nothing is fetched), the table's ninth column (include/sifsr_lpips.h)
  conserve.consistency / conserve, predict_granule(conserve=) / predict_granule_gaps(conserve=) / GranulePredictor(conserve=)  <- no
                                       counterpart for the network (TsHARP's correction_linreg, utils.py:897, is the baselines' form):
                                       the residual LST - D(SR) over the valid cells and its correction (include/sifsr_conserve.h)
  degrade.degrade / aster_to_coarse / aster_to_fine / generic_downscale / simulate_pair / output_shape  <- utils.py:1642-1668,
                                       :1759-1830: the sensor model at any ratio (ASTER 90 m -> 250 m / 1 km), with the validity of
                                       every output (include/sifsr_degrade.h)
  adapt.frozen_bn / input_gradient / tile_targets / adapt_granule, ModelB_2.bn_frozen  <- no counterpart: fine-tuning a trained
                                       model on the granule it is about to predict -- BatchNorm backward with frozen running statistics,
                                       the gradient with respect to the network input, loss targets of active tiles (include/sifsr_adapt.h)
  sensor.downscale / lowpass / lr_shape / sif_loss / train_step  <- utils.py:1671-1706, :1833-1860 at any factor, as autograd ops
                                       (the adjoint of the banded sensor operator and the reflect-border MTF low-pass, forward
                                       and adjoint), the SIF loss and a training step at any ratio (include/sifsr_sensor.h)
  ratio.upsample / geometry / prepare_tiles / granule_to_tiles / blend_tiles / predict_granule / predict_granule_gaps  <- no
                                       counterpart: the bicubic resampler with an exact phase at any size, and whole-granule
                                       prediction (seamless, gap-aware) at any ratio hr / window (include/sifsr_ratio.h)
  rloss.valid_counts / sif_loss / sif_loss_with_grad / train_step / adapt_granule  <- no counterpart: the SIF loss at any ratio as
                                       two fused kernels, masked (cloudy patches at x3, x2.5, x2), and fine-tuning on a granule at
                                       any ratio hr / window (include/sifsr_rloss.h)
  rconserve.consistency / conserve, ratio.predict_granule(conserve=) / ratio.predict_granule_gaps(conserve=)  <- no counterpart:
                                       the residual LST - D(SR) and its correction at any ratio H / h <= 8, with the sensor model of
                                       degrade and the resampler of ratio (include/sifsr_rconserve.h)
  rproducts.decode / PatchMiner / patch_counts / expand_valid, MinedPatches(hr=), rloss.train_epoch / eval_epoch / fit  <- no
                                       counterpart: mining at any ratio hr / window with the reference's window and acceptance
                                       rules, loaders and the epoch loop on the patches (include/sifsr_rproducts.h)
  rloss.GraphedTrainStep, rloss.train_epoch / fit / adapt_granule(graphed=), adapt.adapt_granule(graphed=), ratio.GranulePredictor,
  predict.GranulePredictor(gaps=)      <- no counterpart: the training step at any ratio and both granule
                                       predictors as one hipGraph each; the gap-aware predictor forwards a fixed number of slots and
                                       keeps the active count on the device, so a stream of granules has no host synchronisation
                                       (host code only: no kernel, no header)
  rbaselines.tsharp / atprk / aatprk / dms / dms_model / dms_apply / dms_aggregate  <- utils.py:876-1606 with `iscale` other than 4
                                       (DESIGN.md §9 f24): the comparison methods for a fine raster at any ratio H / h <= 8 (kriging at
                                       integer scales 2..8), so that a model trained at x3, x2.5 or x2 can be ranked against them
                                       (csrc/rbaselines_api.h)
  products.decode / PatchMiner / MinedPatches, dataset.MinedDataset  <- process_modis.py:38-335, data_preparation.py:32-102
                                       (raw granule arrays -> patches + statistics.json, on device)

The directory name is the repository's mandated package name (it contains '-', so it is imported
through ``importlib`` or the ``sifsr`` alias: ``import sifsr`` at the repo root loads this package
and registers ``sifsr`` / ``sifsr.<submodule>`` as aliases of the same module objects).
"""
import importlib
import sys

_SUBMODULES = ("_lib", "model", "sif_ops", "optim", "dataset", "distributed", "train", "pipeline", "metrics", "fourier", "spectra", "gaps", "conserve", "degrade", "predict", "baselines", "products", "lpips", "adapt", "sensor", "rconserve", "ratio", "rloss", "rproducts", "rbaselines")
for _m in _SUBMODULES:
    importlib.import_module(__name__ + "." + _m)

sys.modules["sifsr"] = sys.modules[__name__]
for _m in _SUBMODULES:
    sys.modules.setdefault("sifsr." + _m, sys.modules[__name__ + "." + _m])

from .model import ModelB_2  # noqa: E402,F401
from .sif_ops import downscale_LST_SR_to_LR, get_output_ftm, sobel_bank, huber_loss, sif_loss, sif_loss_with_grad  # noqa: E402,F401
from .sif_ops import masked_sif_loss, masked_sif_loss_with_grad  # noqa: E402,F401
from .optim import FlatAdam  # noqa: E402,F401
from .dataset import ModisDatasetB, MinedDataset  # noqa: E402,F401
from ._lib import SifsrError  # noqa: E402,F401
# (`sifsr.degrade` stays the module: its function of the same name is `sifsr.degrade.degrade`)
from .degrade import aster_to_coarse, aster_to_fine, generic_downscale, simulate_pair  # noqa: E402,F401
