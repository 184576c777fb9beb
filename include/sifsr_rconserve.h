/* sifsr_rconserve.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): does the super-resolved raster conserve the
 * observed one AT ANY RATIO, and the residual correction that makes it.  It is sifsr_conserve.h with the
 * sensor model of sifsr_degrade.h in the place of the /4 one and the exact-phase bicubic of sifsr_ratio.h in the place of the x4
 * one: the property a model trained with the loss of sifsr_rloss.h is trained on, measured and enforced on a whole granule with
 * gaps.  No reference counterpart.
 *
 * Conventions are those of sifsr_conserve.h: every pointer is a DEVICE pointer (dense, row-major; `float` fp32, `double` float64,
 * `unsigned char` one byte per LST pixel), `stream` a hipStream_t passed as void*; functions only enqueue work on `stream` and
 * return 0, 1001 for a shape or limit error, 1002 for an argument error, 1003 for a workspace that is too small, or the hipError_t
 * of a failed launch.  Nothing is launched when an error is returned.  The symbols carry the prefix `sifsrc_`, live in the same
 * library and are gated by tests/test_capi_gate.py (contract cases: tests/test_rconserve_gpu.py); sifsr_abi_version() is unchanged.
 *
 * ---- definitions ------------------------------------------------------------------------------------------------------------
 * Rasters: sr (H, W) [K], lst (h, w) [K], mask (h, w) bytes or NULL.  The ratio is H / h = W / w, checked as H w == W h in 64-bit
 * integers; factor = (double)H / (double)h with 1 < factor <= 8 (the limit of sifsr_rloss.h), hw = ceil(factor) <= 8.
 * A CELL is an LST pixel (i, j) and the sr pixels under it by the rule of sifsr_ratio.h / sifsr_rloss.h: the cell of sr pixel (Y, X)
 * is P = (floor(Y h / H), floor(X w / W)) in integers, so cell i holds the rows ceil(i H / h) .. ceil((i + 1) H / h) - 1 --
 * floor(factor) or ceil(factor) of them, 2 or 3 at x2.5 -- and likewise the columns.
 *
 *   D   the operator of sifsrs_degrade for (H, W, factor, mtf, hkw = 0, crop = 1): reflect pad by hw, the normalised Gaussian PSF
 *       with the zero ring, bicubic by 1 / factor, the cut of int(hw / factor) outputs on each side -- per axis ONE banded float64
 *       matrix R, D(sr) = Ry sr Rx^T.  Its weights and its stencil table (per output: the first pixel of the weight window, the
 *       first and last pixel with a weight, the ring flag) are written by the table kernel of sifsrs_degrade itself
 *       (csrc/sensor_tables.h).  The call is refused (1001) unless sifsrs_out_shape(H, W, factor, 0, 1) == (h, w): lst (16, 20) with
 *       sr (20, 25) gives 17 x 21 and is refused.  The reflection is at the raster edge only.
 *   U   bicubic (h, w) -> (H, W) as sifsrr_upsample computes it (A = -0.75, half-pixel centres, the phase of every output in
 *       integers, source indices clamped at the raster edge): U(r) is, bit for bit, what sifsrr_upsample gives for r (the device
 *       functions of csrc/ratio.h run in both).
 *   c   cell validity: c[i, j] = isfinite(lst) && lst != 0 && (mask == NULL || mask != 0)   -- the rule of sifsrg_fill --
 *       && every sr pixel of the cell is finite and non-zero   -- which covers fill_value = NaN and the 0 of an uncovered edge.
 *   r   the residual.  The stencil rectangle of output (i, j) is the pixels lo .. hi of each axis that carry a weight (the stencil
 *       table); the cells it touches are floor(lo h / H) .. floor(hi h / H), and likewise the columns.  r[i, j] = lst[i, j] - D(sr)[i, j]
 *       is COUNTED iff c holds on cell (i, j) and on every cell the rectangle touches, and neither axis has the ring flag set;
 *       otherwise r[i, j] = 0.  This is the validity rule of sifsrs_degrade(valid=) stated on cells.  Both are read from the tables;
 *       nothing is hard-wired.  At x4 it is the 3 x 3 rule of sifsr_conserve.h and no output touches the ring, nor does one at x3
 *       (the outermost output samples blurred entry hw + 1 alone); at x2, x2.5 and x8/3 the stencil reaches two cells to a side and
 *       outermost cells of the raster touch the zero ring -- the first and the last of an axis at x2, the first alone at x2.5 and
 *       x8/3 -- so they are never counted (tests/test_rconserve_host.py records this).  What an invalid pixel holds changes no
 *       output bit.
 *   one correction step   out[p] = fmaf(relax, U(r)[p], sr[p]) at every sr pixel p whose cell has c; every other pixel keeps its
 *       bits.  Uncounted cells carry r = 0, so the correction fades out towards a gap and never pulls in filled values.
 *   statistics   over the counted cells, in float64: {count, bias = mean r, RMSE = sqrt(mean r^2), max |r|}; a row with nothing
 *       counted holds count 0 and NaN in the other three.
 *
 * ---- sifsrc_conserve --------------------------------------------------------------------------------------------------------
 * stats (n_iter + 1, 4) float64: row 0 from sr as given, row k after the k-th step; n_iter = 0 is the pure check.
 * out (H, W): the corrected raster, EVERY element written when n_iter >= 1 (pixels of cells without c: the bits of sr); with
 * n_iter = 0 out is not touched and may be NULL.  out may alias sr (the residual and the correction are separate launches);
 * partial overlap is not allowed.  sr, lst and mask are not written (unless out aliases sr).
 *
 * Arithmetic.  D is applied in float64 over the float64 tables: a workgroup stages the sr pixels its tile of cells reaches, applies
 * Ry into a float64 intermediate, then Rx; r = (double)lst - D(sr) is formed in float64 and rounded to fp32 ONCE.  Weights that are
 * zero are skipped, not multiplied: what lies under them is not used.  The statistics are sums of the rounded r in float64, added
 * in a fixed order.  U and the step are fp32 fused multiply-adds in the order of sifsrr_upsample.  No float atomics: the same
 * inputs give the same bits on every run.
 *
 * Launches: the table kernel once, (n_iter + 1) residual kernels, n_iter correction kernels and one kernel that finishes the
 * statistics -- a linear chain on `stream`, no allocation, no host synchronisation: it can be captured into a hipGraph.
 *
 * workspace: at least sifsrc_workspace_bytes(h, w, H, W, n_iter) bytes, 16-byte aligned (else 1002); its contents before the call
 * do not matter.  After the call its first h * w floats hold r of the LAST statistics row (sifsr.rconserve.consistency reads it);
 * the rest is unspecified.
 *
 * Limits: H w == W h, 1 < factor <= 8, sifsrs_out_shape(H, W, factor, 0, 1) == (h, w) (which holds hw + 1 <= H, W <= 16384),
 * 0 <= n_iter <= 64, 0 < mtf < 1; otherwise (a NaN mtf included) 1001.  Null sr / lst / stats / workspace, null out with
 * n_iter >= 1, sr / lst / out not 4-byte or stats not 8-byte aligned, a non-finite relax: 1002.  A smaller `workspace_bytes`: 1003.
 * sifsrc_workspace_bytes is host only and returns 0 for a refused shape. */
#ifndef SIFSR_RCONSERVE_H
#define SIFSR_RCONSERVE_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API size_t sifsrc_workspace_bytes(int h, int w, int H, int W, int n_iter);
SIFSR_API int sifsrc_conserve(const float* sr, const float* lst, const unsigned char* mask, float* out, double* stats, void* workspace,
                              size_t workspace_bytes, int h, int w, int H, int W, double mtf, float relax, int n_iter, void* stream);

#endif /* SIFSR_RCONSERVE_H */
