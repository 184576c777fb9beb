/* sifsr_rloss.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): the scale-invariance-free loss at any ratio,
 * masked, with its gradient, as two fused kernels.  It is the loss block of the two training scripts
 * (train_model_B_gradFTM.py:99-117, train_model_B_predef_filters.py:111-133) with the sensor model of sifsr_degrade.h /
 * sifsr_sensor.h in the place of the /4 one, and the mask of sifsr_masked.h at a ratio.
 *
 * Conventions, error codes and "nothing is launched when an error is returned" are those of sifsr_sensor.h: every pointer is a
 * DEVICE pointer (dense, row-major; `float` fp32, `unsigned char` one byte per LR cell, `long long` int64), `stream` a hipStream_t
 * passed as void*; functions only enqueue work on `stream` and return 0, 1001 for a shape or limit error, 1002 for an argument
 * error, 1003 for a workspace that is too small, or the hipError_t of a failed launch.  The symbols carry the prefix `sifsrq_`,
 * live in the same library and have their own gate (tests/test_rloss_host.py, tests/test_rloss_gpu.py); sifsr_abi_version() is
 * unchanged.
 *
 * ---- definitions (those of sifsr_degrade.h and sifsr_sensor.h) ------------------------------------------------------------------
 * hw = ceil(factor) (the `hkw` argument of the sensor model is fixed at 0 here).
 * R (h x H, per axis): the banded operator of sifsrs_degrade for (H, factor, mtf = 0.1, hkw = 0, crop = 1).
 * L (H x H, per axis): the low-pass of sifsrt_lowpass_fwd for (factor, mtf = 0.25, hkw = 0).
 * Both weight tables are written by the table kernels of sifsrs_degrade / sifsrt_lowpass_fwd themselves (csrc/sensor_tables.h).
 * (h, w) = sifsrs_out_shape(H, W, factor, 0, 1).  lst and valid are (B, h, w); sr, ndvi and dsr are (B, H, W).
 * The LR cell of HR pixel (Y, X) is P = (floor(Y h / H), floor(X w / W)), in integers: cell i holds the HR rows
 * ceil(i H / h) .. ceil((i + 1) H / h) - 1, which are floor(H / h) or ceil(H / h) rows.
 *
 * V: the LR cells with valid != 0.  n1 = counts2[0] = |V|, n2 = counts2[1] = the number of HR pixels q with P(q) in V -- the exact
 * count, not n1 H W / (h w).  F = 1 for kind 2 (SR2), 4 for kind 1 (SR1, the Sobel bank of sifsr_sobel4_fwd, zero padding).
 *
 *     dn   = (Ry . (sr std + mean) . Rx^T - mean) / std
 *     ds   = 1 / n1       sum over p in V               huber(dn_p - lst_p)
 *     e2   = (sr - L sr) - gamma (ndvi - L ndvi)                      kind 2
 *            sobel_bank(sr) - gamma sobel_bank(ndvi)                  kind 1
 *     pl   = 1 / (F n2)   sum over q with P(q) in V, f  huber(e2_{q,f})
 *     loss = alpha ds + (1 - alpha) pl;   losses3 = {ds, pl, loss};   dsr (may be NULL) = d loss / d sr
 *
 * huber is nn.HuberLoss(delta = 1) per element.  valid == NULL and counts2 == NULL TOGETHER give the unmasked loss, n1 = B h w and
 * n2 = B H W, bit for bit what an all-ones mask with its counts gives; exactly one of them NULL is 1002.  The blur and the low-pass
 * read sr and ndvi at EVERY pixel, so a valid target still constrains the prediction in the rim of a gap.  lst[p] for p outside V is
 * never read: a NaN there changes no output bit.  n1 <= 0 or n2 <= 0: losses3 = {0, 0, 0} and dsr = 0, no NaN.  An image without a
 * valid cell has dsr exactly 0.  A NaN residual at a VALID cell is a NaN loss value and a NaN gradient wherever the operators' supports
 * carry it (sifsr_hip.h, "Non-finite data": clamp_d keeps a NaN); the other elements of dsr keep the bits of the repaired call.
 *
 * Arithmetic.  Weights, sums and residuals are float64.  By linearity dn = Ry sr Rx^T + (mean / std) (rowsum(Ry) rowsum(Rx) - 1):
 * nothing is rounded at the 300 K scale.  kind 2 applies ONE low-pass, e2 = (I - L)(sr - gamma ndvi), formed in float64.  The two
 * residual maps r1 = alpha / n1 clamp(e1) and r2 = (1 - alpha) / (F n2) clamp(e2) are stored as fp32; dsr is gathered from them in
 * float64 and rounded once.  No float atomics and a fixed order of every sum: the same inputs give the same bits, losses3 has the
 * same bits with dsr NULL, and an image gives the same dsr bits alone and inside a batch (with the same counts).
 *
 * Launches of sifsrq_sif_loss: a linear chain on `stream` -- the table kernel of R, for kind 2 the table kernel of L, with dsr the
 * range kernel of sifsrt_degrade_bwd, pass A (one workgroup per image and LR tile: r1, r2, the Huber partial sums), then pass B
 * (dsr = Ry^T r1 Rx + (I - L)^T r2, or the Sobel adjoint; its first workgroup finalises losses3) or, without dsr, one finalising
 * workgroup.  The scales alpha / n1 and (1 - alpha) / (F n2) are formed on the device from counts2 (or from B h w and B H W by the
 * same expressions).  No allocation, no host synchronisation, no host value that changes from step to step: the call can be
 * captured into a hipGraph.
 *
 * workspace: at least sifsrq_sif_loss_workspace_bytes bytes, 16-byte aligned (else 1002); its contents before the call do not matter
 * and are unspecified after it.  No buffer may overlap another.  sr, lst, valid, counts2 and ndvi are not written.
 *
 * Limits: kind 1 or 2 (else 1002; the size function returns 0), 1 <= B <= 65535, 1 < factor <= 8 (so that hw <= 8: the staged
 * tiles of both passes are sized for it), hw + 1 <= H, W <= 16384, both LR sides >= 1; otherwise (a NaN factor included) 1001.
 * Null sr / lst / ndvi / workspace / losses3, a pointer not aligned to its element (counts2: 8 bytes): 1002.
 *
 * ---- sifsrq_valid_counts --------------------------------------------------------------------------------------------------------
 * valid (B, h, w) -> counts2 = {n1, n2} as defined above, for any 1 <= h <= H <= 16384, 1 <= w <= W <= 16384, 1 <= B <= 65535 (else
 * 1001; null valid / counts2 or counts2 not 8-byte aligned: 1002).  Integer arithmetic only, exact; both elements are written.
 * Launches: a kernel that zeroes the two counters and the counting kernel (integer atomic adds of per-workgroup sums: exact in any
 * order); no memset node, so a captured graph holds kernels only.
 *
 * sifsrq_sif_loss_workspace_bytes is host only and returns 0 for an invalid shape or kind. */
#ifndef SIFSR_RLOSS_H
#define SIFSR_RLOSS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API size_t sifsrq_sif_loss_workspace_bytes(int kind, int B, int H, int W, double factor);
SIFSR_API int sifsrq_valid_counts(const unsigned char* valid, int B, int h, int w, int H, int W, long long* counts2, void* stream);
SIFSR_API int sifsrq_sif_loss(int kind, const float* sr, const float* lst, const unsigned char* valid, const long long* counts2,
                              const float* ndvi, int B, int H, int W, double factor, float mean, float std, float alpha, float gamma,
                              void* workspace, size_t workspace_bytes, float* losses3, float* dsr, void* stream);

#endif /* SIFSR_RLOSS_H */
