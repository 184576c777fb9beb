/* sifsr_lpips.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): LPIPS-VGG16 on the device, the ninth column
 * of the per-pair ASTER table (model_perf_aster_formatds.py:405-410; the metric is the piq variant vendored in lpips.py:226-292,
 * :351-358 with distance = 'mse', normalize_features = True, max-pooling kept).
 *
 * The reference downloads the VGG16 and the LPIPS linear weights; this library never fetches anything: the caller supplies both
 * as flat fp32 buffers and sifsrl_pack rearranges them once per model.  For a pair (x, y) of (3, H, W) images
 *     x <- (x - mean) / std per channel; VGG16 `features` up to module 29 (13 convs 3x3, stride 1, ZERO padding 1, bias, ReLU;
 *     3 -> 64, 64 | 128, 128 | 256 x3 | 512 x3 | 512 x3; MaxPool2d(2, 2), floor, between the groups);
 *     taps: the ReLU outputs of modules 3, 8, 15, 22, 29 (64, 128, 256, 512, 512 channels);
 *     f <- f / (sqrt(sum_c f^2) + 1e-10);   d_l = sum_c lin_l[c] * mean_{h,w} (fx - fy)^2;   LPIPS = sum_l d_l.
 *
 * Conventions are those of sifsr_scores.h: every pointer is a DEVICE pointer unless said otherwise (dense, row-major; `float`
 * fp32, `double` fp64), `stream` a hipStream_t passed as void*; functions only enqueue work on `stream` and return 0, 1001 for a
 * shape error, 1002 for an argument error, 1003 for a workspace that is too small, or the hipError_t of a failed launch.  Nothing
 * is launched when an error is returned.  No float atomics, no allocation, no host synchronisation: every call can be captured
 * into a hipGraph (the launches form one linear chain).  The symbols carry the prefix `sifsrl_`, live in the same library and have
 * their own declaration / export / memory-contract gate (tests/test_lpips_host.py, tests/test_lpips_gpu.py); sifsr_abi_version()
 * is unchanged.
 *
 * How it runs: both images of every pair go through the network as one batch of 2N NHWC tensors.  A convolution whose feature map
 * has H >= 16 and W >= 16 runs on the fp32 matrix cores (the tap-domain kernel of conv_mfma.hip with zero padding, output
 * channels beyond 128 in slices of 128); a map with min(H, W) < 16 -- thinner than one 16 x 16 tile of that kernel, so that every
 * tile would be partial in that direction and no pixel an interior one -- runs through a plain direct convolution.  That is the
 * DIRECT / MFMA THRESHOLD: min(H, W) of the feature map < 16.  The rule looks at the thin side only, not at the pixel count: an
 * image that is thin but very long (30 x 2000: a 15 x 1000 map after the first pool) runs every later layer through the direct
 * kernel, one wave per 4 pixels and 16 output channels without the matrix cores -- correct, and several times slower per pixel
 * than the MFMA path.  The ASTER pairs (41 x 43 and larger, 256 x 256 in the reference's set) do not meet that case.
 * Bias + ReLU (+ the 2 x 2 max-pool) is a pass of its own, the channel norms and the lin-weighted squared differences are reduced
 * per pixel by one wave, and the spatial mean is accumulated in float64 in a fixed order (per-block partial sums, then one thread
 * per pair).
 *
 * Invariants:
 *   * Row i of a batch is bit-identical to its own N = 1 call.
 *   * Swapping x and y (a and b) changes no output bit.
 *   * Identical images give exactly 0.0 in all six columns.
 *   * If any pixel of a pair is not finite, that pair's row is NaN in all six columns and every other row is untouched by it.
 */
#ifndef SIFSR_LPIPS_H
#define SIFSR_LPIPS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- weights -----------------------------------------------------------------------------------------------------------------
 * vgg_params  the 13 (weight OIHW, bias) pairs of torchvision's vgg16().features, flat, in module order: 14,714,688 floats
 * lin         the LPIPS linear weights of the five taps, flat, in tap order: 64 + 128 + 256 + 512 + 512 = 1472 floats
 * packed      sifsrl_pack_floats() floats, 256-byte aligned: the 13 weight tensors in the forward MFMA fragment order
 *             wf[nb][q][tap][lane][j] = W[co = 16 nb + (lane & 15)][ci = 16 q + 4 (lane >> 4) + j][tap] (the 3 input channels of
 *             conv1_1 padded to 16 with zeros), then the 4224 biases, then lin.
 * Pack once per model; the LPIPS calls read `packed` only.  Null pointer: 1002.  sifsrl_pack_floats is host only. */
SIFSR_API size_t sifsrl_pack_floats(void);
SIFSR_API int sifsrl_pack(const float* vgg_params, const float* lin, float* packed, void* stream);

/* ---- workspace ---------------------------------------------------------------------------------------------------------------
 * Bytes an LPIPS call on N pairs of H x W images needs (three activation tensors of 2N x H x W x 64 floats and the partial sums).
 * 0 for an unsupported shape: N < 1, H < 16 or W < 16 (relu5_3 would be empty), or 2N x H x W x 64 floats at or beyond the
 * 4 GiB - 4 KiB limit of the convolution's 32-bit buffer addressing.  Host only. */
SIFSR_API size_t sifsrl_workspace_bytes(int N, int H, int W);

/* ---- LPIPS of N pairs of three-channel images ----------------------------------------------------------------------------------
 * x, y      (N, 3, H, W)
 * mean3, std3  HOST pointers to three floats each (lpips.py:133-134 for images in [0, 1])
 * out6      (N, 6): d_1 .. d_5 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) and their sum, the LPIPS of the pair
 * workspace at least sifsrl_workspace_bytes(N, H, W) bytes, 256-byte aligned; its contents before and after the call are private.
 * Unsupported shape: 1001.  Null x / y / mean3 / std3 / packed / workspace / out6: 1002.  workspace_bytes too small: 1003. */
SIFSR_API int sifsrl_lpips(const float* x, const float* y, int N, int H, int W, const float* mean3, const float* std3,
                           const float* packed, void* workspace, size_t workspace_bytes, double* out6, void* stream);

/* ---- the table path: N pairs of one-channel rasters (model_perf_aster_formatds.py:373-374, :407-408) ---------------------------
 * a, b      (N, H, W).  Per pair mini / maxi = min / max over both images, found on the device;
 *           t = (v - mini) / (maxi - mini) in fp32, repeated to three channels; mean = 0, std = 1.
 * The rows are bit-identical to sifsrl_lpips on those three-channel images.  maxi == mini (the reference divides by zero): the
 * row is NaN.  Errors as above. */
SIFSR_API int sifsrl_lpips_pairs(const float* a, const float* b, int N, int H, int W, const float* packed, void* workspace,
                                 size_t workspace_bytes, double* out6, void* stream);

#endif /* SIFSR_LPIPS_H */
