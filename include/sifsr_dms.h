/* sifsr_dms.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): DMS, the Data Mining Sharpener of Gao et al.
 * 2012 as the reference's evaluation calls it (data_mining_sharpener_modified.py through model_perf_aster_formatds.py:220-250):
 * one predictor (NDVI), the global regression only, a bagged ensemble of regression trees (max_leaf_nodes 30, min_samples_leaf 10)
 * with a ridge regression in every leaf, then the radiance (T^4) residual correction.
 *
 * With one feature every node of a tree is an interval of the samples sorted by the float32 feature, so scikit-learn's best-first
 * builder is prefix sums plus an arg-max per node, and a fitted tree is <= 29 ascending thresholds and <= 30 leaf records.  The
 * stages are separate entry points.  Two sorts (the cv values for the percentile, the samples by feature) and the bootstrap draw
 * are left to the caller (sifsr/baselines.py: torch.sort, torch.randint).
 *
 * Conventions are those of sifsr_baselines.h: every pointer is a DEVICE pointer to a dense array, `stream` a hipStream_t passed as
 * void*; functions only enqueue work on `stream` and return 0, a SIFSR_ERR_* code (1001 shape, 1002 argument) or the hipError_t of
 * a failed launch.  The symbols carry the prefix `sifsrd_`, live in the same library, and have their own declaration / export /
 * memory-contract gate (tests/test_dms_host.py, tests/test_dms_gpu.py); sifsr_abi_version() is unchanged.
 *
 * Shapes: lst is (B, h, w) float32 in Kelvin (coarse), ndvi_f, sr and out are (B, 4h, 4w) float32 (fine); N = h * w.  Only scale 4
 * is built.  Intermediate results are float64 with one rounding at a float32 store.  No atomics: every reduction runs in a fixed
 * order, so results are deterministic and the images of a batch do not depend on each other.  Every output is written in full.
 * Any other ratio H / h <= 8: sifsr/rbaselines.py, csrc/rbaselines_api.h.
 */
#ifndef SIFSR_DMS_H
#define SIFSR_DMS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

#define SIFSRD_MAX_LEAVES 30      /* thresholds are padded to 29 per tree with +inf, leaf records to 30 with zeros */
#define SIFSRD_MAX_ESTIMATORS 32

/* Stage 1 (_resampleHighResToLowRes on aligned grids): per coarse cell the NaN-ignoring mean and population standard deviation
 * of its 4 x 4 fine block (of fine^4 when pow4 != 0), the 16 values added row by row in float64; an all-NaN block gives NaN.
 * One thread per cell, four 16-byte loads.  std may be null (not computed). */
SIFSR_API int sifsrd_aggregate(const float* fine, double* mean, double* std, int B, int h, int w, int pow4, void* stream);

/* Stage 2a (trainSharpener :653-736, global window): per cell x = mean (1e-6 where mean == 0), cv = std / x (1000 where NaN),
 * good = isfinite(lst) and lst > 0 and isfinite(x) and 0 < cv < 1000 (lst <= 0 is this project's gap convention). */
SIFSR_API int sifsrd_trainset(const float* lst, const double* mean, const double* std, double* x, double* cv, unsigned char* good,
                              int B, int h, int w, void* stream);

/* Stage 2b: the sample weights.  stats (B, 3) = [the 80th percentile of cv over the good cells, their smallest cv, their largest
 * cv]; weight (B, N) = (1/cv - 1/cvmax) / (1/cvmin - 1/cvmax), halved where cv is not < the percentile, 0 where not good.  The
 * cell of largest cv gets exactly 0, as in the reference. */
SIFSR_API int sifsrd_weights(const double* cv, const unsigned char* good, const double* stats, double* weight, int B, int N,
                             void* stream);

/* Stage 3: one workgroup per (image, estimator).  xs, ys, ws (B, N): the image's n_train[b] training samples first, in ascending
 * order of (float)xs; cs (B, E, N) int32 the estimator's bootstrap multiplicities in the same order; n_train (B) int32, 0 = no
 * model.  The samples with ws * cs != 0 are compacted and their float64 prefix sums of w c, w c y, w c y^2 written to `scratch`
 * (sifsrd_fit_scratch_bytes(B, E, N) bytes, 8-byte aligned; written before it is read); best-first growth then follows
 * scikit-learn's BestFirstTreeBuilder with the MSE criterion: a node is a leaf if it holds fewer than 20 samples or its impurity
 * is <= DBL_EPSILON; split positions skip x[p] <= x[p-1] + 1e-7f (float32); both children hold >= 10 samples; the proxy
 * SL^2/WL + SR^2/WR is maximised with the lowest position winning ties; threshold = (double)x[p-1] / 2 + (double)x[p] / 2; the
 * frontier node of largest weighted impurity improvement is split next, at most 29 times.  Every leaf then gets a ridge regression
 * (alpha 1, with intercept, centred two-pass sums) over ALL the samples that predict into it, unweighted.
 * thresholds (B, E, 29) ascending, +inf padded; nleaf (B, E) int32 (0 where n_train == 0); leaves (B, E, 30, 4) =
 * [coef, intercept, min y - 0.25 range, max y + 0.25 range], zero padded. */
SIFSR_API size_t sifsrd_fit_scratch_bytes(int B, int E, int N);
SIFSR_API int sifsrd_fit(const double* xs, const double* ys, const double* ws, const int* cs, const int* n_train, void* scratch,
                         double* thresholds, int* nleaf, double* leaves, int B, int E, int N, void* stream);

/* Stage 4 (applySharpener :816-886): one thread owns 4 consecutive fine pixels; the image's E leaf tables sit in LDS.  Per
 * estimator the leaf by binary search with `x <= threshold -> left`, then clamp(intercept + coef x); the mean over the estimators
 * in index order, in float64.  A NaN index is stored as NaN; an image with nleaf[b, 0] == 0 is all NaN. */
SIFSR_API int sifsrd_predict(const float* ndvi_f, const double* thresholds, const int* nleaf, const double* leaves, float* sr,
                             int B, int E, int h, int w, void* stream);

/* Stage 5 (_calculateResidual, residualAnalysis with temperature): res = lst^4 - m4, m4 (B, h, w) = sifsrd_aggregate(sr, pow4 = 1);
 * res upsampled x4 in float64 with the INTER_CUBIC restatement of the pipeline (a = -0.75, replicate border, columns of a row
 * first), out = (res_hr + sr^4)^(1/4); a negative radicand gives NaN.  Upsample and root are one pass over the fine raster. */
SIFSR_API int sifsrd_correct(const float* lst, const float* sr, const double* m4, float* out, int B, int h, int w, void* stream);

#endif /* SIFSR_DMS_H */
