// Scoring rasters with gaps (C ABI: include/sifsr_scores.h): the valid-pixel forms of the per-pair evaluation
// table and of the train-time PSNR / SSIM.
//
// The kernels are the MASKED instantiations of eval_metrics.hip and pipeline.hip, as the masked SIF loss is the MASKED instantiation
// of loss.hip: one body serves both forms, so the all-valid case adds the same values in the same order as the unmasked entry
// points and equals them bit for bit -- the per-pair table with contraction off (eval_metrics.hip), the train-time pair with the
// contraction pipeline.hip is built with.  This file holds the C entry points: argument, shape and workspace checks, then the
// launch sequence of the unmasked call with the validity bytes threaded through it.
#include "../../include/sifsr_scores.h"

#include "edge_conv.h"

#pragma clang fp contract(off)

namespace {
bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

size_t sifsrv_eval_metrics_scratch_bytes(int B, int H, int W) { return eval_metrics_masked_scratch_bytes(B, H, W); }

int sifsrv_eval_metrics(const float* ref, const float* pred, const unsigned char* mask, int B, int H, int W, const float* taps9,
                        float data_range, void* scratch, size_t scratch_bytes, double* out8, int* counts5, void* stream) {
  if (!ref || !pred || !taps9 || !scratch || !out8 || !counts5 || !aligned(scratch, 256) || !aligned(out8, 8)) return SIFSR_ERR_ARG;
  const size_t need = eval_metrics_masked_scratch_bytes(B, H, W);
  if (need == 0) return SIFSR_ERR_SHAPE;
  if (scratch_bytes < need) return SIFSR_ERR_WORKSPACE;
  return launch_eval_metrics_masked(ref, pred, mask, B, H, W, taps9, data_range, scratch, out8, counts5, (hipStream_t)stream);
}

size_t sifsrv_psnr_ssim_scratch_bytes(int B, int H, int W) {
  if (B < 1 || H < 7 || W < 7) return 0;
  return psnr_ssim_masked_scratch_bytes(B, H, W);
}

int sifsrv_psnr_ssim(const float* pred, const float* targ, const unsigned char* valid, int scale, int B, int H, int W, void* scratch,
                     size_t scratch_bytes, float* out2, int* counts2, void* stream) {
  if (!pred || !targ || !valid || !scratch || !out2 || !counts2 || !aligned(scratch, 8)) return SIFSR_ERR_ARG;
  if (B < 1 || B > 65535 || H < 7 || W < 7 || (scale != 1 && scale != 4) || H % scale || W % scale) return SIFSR_ERR_SHAPE;
  if (scratch_bytes < psnr_ssim_masked_scratch_bytes(B, H, W)) return SIFSR_ERR_WORKSPACE;
  return launch_psnr_ssim_masked(pred, targ, valid, scale, B, H, W, scratch, out2, counts2, (hipStream_t)stream);
}
