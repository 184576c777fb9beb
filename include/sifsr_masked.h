/* sifsr_masked.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): training on partly valid patches.
 *
 * sifsr_gaps.h makes PREDICTION work on granules with holes; this header does the same for TRAINING.  A patch mined with
 * PatchMiner(coverage > 0) (the reference's --coverage switch, process_modis.py) holds cloud / ocean / fill pixels as 0.0 K.
 * Left alone they pull the statistics down, enter the network at about -55 sigma, and the SIF loss asks the network to
 * reproduce 0 K there.  The entry points below
 *   patches_fill   mark the valid pixels of every patch of a batch, give the invalid ones a neutral local mean -- the fill of
 *                  sifsrg_fill, per patch -- and leave the moments of the valid pixels for the statistics,
 *   sif_loss       the fused SIF loss of sifsr_sif_loss and its gradient, to which an invalid LR pixel contributes nothing.
 * No reference counterpart.
 *
 * Conventions are those of sifsr_gaps.h: every pointer is a DEVICE pointer unless said otherwise (dense, row-major; `float` fp32,
 * `double` fp64, `unsigned char` one byte per pixel, `long long` 64 bit), `stream` a hipStream_t passed as void*; functions only
 * enqueue work on `stream` and return 0, 1001 for a shape error, 1002 for an argument error, 1003 for a workspace that is too
 * small, or the hipError_t of a failed launch.  Nothing is launched when an error is returned.  The symbols carry the prefix
 * `sifsrm_`, live in the same library and have their own declaration / export / memory-contract gate (tests/test_masked_host.py,
 * tests/test_masked_gpu.py); sifsr_abi_version() is unchanged.
 */
#ifndef SIFSR_MASKED_H
#define SIFSR_MASKED_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- per-patch fill and moments ---------------------------------------------------------------------------------------------
 * lst (N, w, w) [K] -> filled (N, w, w), valid (N, w, w), moments (N, 5) float64; EVERY element of the three outputs is written.
 * N >= 1, 4 <= w <= 64, w % 4 == 0; anything else: 1001.  Null lst / filled / valid / moments: 1002; moments 8-byte aligned.
 *
 * Validity is that of sifsrg_fill with mask == NULL:  valid[p] = isfinite(lst[p]) && lst[p] != 0, stored as 0 or 1.
 *
 * filled[n] is, bit for bit, what sifsrg_fill gives for patch n taken as a (w, w) raster of its own: the push-pull pyramid with
 * ceil halving (w = 20: 20 -> 10 -> 5 -> 3 -> 2 -> 1), a cell = the float64 sum and the count of the valid pixels under it, an
 * invalid pixel = (float)(S / c) of the smallest aligned dyadic block around it that holds a valid one; the cells are summed in
 * the order sifsrg_fill sums them (row-major within a 2 x 2 block at level 1, (a + b) + (c + d) above), so the two agree for any
 * values, not only where the sums are exact.  A patch without a valid pixel is filled with 0.
 *
 * moments[n] = [count, mean, M2, min, max] over the valid pixels of patch n:
 *   count     exact
 *   mean      S / count in float64, S the exact float64 sum (the argument of sifsr_gaps.h: temperatures in [128, 512) K are
 *             multiples of 2^-16 below 2^9, 4096 of them stay far below 2^53 units -- bit-defined)
 *   M2        sum (x - mean)^2 in float64, in a fixed order (a thread's pixels in order, then a fixed tree)
 *   min, max  exact
 * count == 0:  [0, 0, 0, +inf, -inf], so that a min / max merge over patches needs no special case.
 *
 * One workgroup per patch; the whole pyramid of a patch (at most 1365 cells of 12 B) lives in LDS: no workspace.  No atomics, and
 * nothing is shared between patches: patch n of a batch is bit-equal to its own N = 1 call. */
SIFSR_API int sifsrm_patches_fill(const float* lst, float* filled, unsigned char* valid, double* moments, int N, int w, void* stream);

/* ---- masked SIF loss --------------------------------------------------------------------------------------------------------
 * sifsr_sif_loss (sifsr_hip.h; same shapes, limits, kinds, host taps, workspace layout) with
 *   valid    (B, H/4, W/4), one byte per LR pixel, any non-zero byte = valid
 *   n_valid  DEVICE pointer to one int64: the number of valid LR pixels of the batch.  The caller supplies it (the sum of the
 *            `count` column of sifsrm_patches_fill over the batch) and the kernel trusts it.
 * With V the set of valid LR pixels, n = n_valid[0], P(q) the LR pixel of HR pixel q and F = 1 (kind 2), 4 (kind 1):
 *   ds   = 1 / n         * sum_{p in V}             huber(dn_p - lst_p)
 *   pl   = 1 / (16 F n)  * sum_{q: P(q) in V} sum_f huber(e2_{q,f})
 *   loss = alpha * ds + (1 - alpha) * pl          losses3 = {ds, pl, loss},  dsr (may be NULL) = d loss / d sr
 * dn and e2 are the quantities of the unmasked loss: the blur and the decimation read sr and ndvi at EVERY pixel, so a valid
 * target still constrains the prediction into the rim of a gap.  The high-frequency term is masked too: under a gap the network
 * input is the blocky fill, and texture trained on that input is not wanted.
 *   * lst[p] for p not in V is never read: a NaN there changes no output bit.
 *   * a NaN residual at a VALID pixel (lst[p], or sr / ndvi under it) is a NaN loss value and a NaN gradient wherever that residual
 *     reaches (sifsr_hip.h, "Non-finite data"); the other elements of dsr keep the bits of the call on the repaired input.
 *   * n <= 0: losses3 = {0, 0, 0} and dsr == 0 everywhere, no NaN.
 *   * every byte valid and n = B H W / 16: losses3 and dsr are bit-identical to sifsr_sif_loss on the same inputs (the weights and
 *     the finalisation scales are formed on the device by the IEEE double divisions and the one cast the host performs there).
 * Nothing of the call depends on a host value that changes from step to step: it can be captured into a hipGraph.  No atomics.
 * workspace: at least sifsrm_sif_loss_workspace_bytes(kind, B, H, W) bytes (the unmasked call's size), 4-byte aligned; a smaller
 * `workspace_bytes`: 1003.  Null sr / lst / valid / n_valid / ndvi / taps / workspace / losses3: 1002; kind not 1 or 2: 1002.
 * sifsrm_sif_loss_workspace_bytes is host only. */
SIFSR_API size_t sifsrm_sif_loss_workspace_bytes(int kind, int B, int H, int W);
SIFSR_API int sifsrm_sif_loss(int kind, const float* sr, const float* lst, const unsigned char* valid, const long long* n_valid,
                              const float* ndvi, int B, int H, int W, float mean, float std, float alpha, float gamma,
                              const float* taps_ds9, const float* taps_ftm9, void* workspace, size_t workspace_bytes,
                              float* losses3, float* dsr, void* stream);

#endif /* SIFSR_MASKED_H */
