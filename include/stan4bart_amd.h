/* stan4bart_amd.h — C-ABI of the MI355X-native stan4bart Gibbs hot path.
 *
 * This is the drop-in boundary for the reference's `.Call` layer (reference
 * src/init.cpp:1215-1229 registration table).  Every entry point below names the reference
 * routine it replaces.  The reference passes R SEXPs (S4 dbarts objects + named lists); here the
 * same information travels as plain structs of scalars and pointers — no R, no torch types.
 * An R shim (`INTEGRATION.md`) unpacks the SEXPs into these structs and forwards.
 *
 * Conventions
 *   - all matrices are column-major (R layout); all pointers are host pointers unless the
 *     struct says otherwise; inputs are copied at create time (reference copies X, y, CSR parts:
 *     src/stan_sampler.cpp:35-65,197-249) except `offset`, which is copied too (the reference
 *     borrows it, src/init.cpp:1033 — copying removes the lifetime hazard).
 *   - every function returns 0 on success, non-zero on failure; `s4b_last_error()` returns the
 *     message the R shim would hand to Rf_error (reference: Rf_error longjmp, src/init.cpp:319).
 *   - one sampler == one chain == one GPU (reference: one chain per R worker process,
 *     R/stan4bart_fit.R:527-533).  A sampler is not thread-safe; different samplers are independent.
 *
 * The symbol prefix is configurable so the CPU oracle (oracle/, test infrastructure only) can
 * export the identical interface as `orc_*` for parity tests.
 */
#ifndef STAN4BART_AMD_H
#define STAN4BART_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifndef S4B_PREFIX
#define S4B_PREFIX s4b_
#endif
#define S4B_CAT_(a, b) a##b
#define S4B_CAT(a, b) S4B_CAT_(a, b)
#define S4B_FN(name) S4B_CAT(S4B_PREFIX, name)

#ifdef __cplusplus
extern "C" {
#endif

/* revision of the struct layouts below; s4b_bart_control.interface_version must carry it (checked by create()) */
#define S4B_INTERFACE_VERSION 6

typedef struct s4b_sampler s4b_sampler; /* reference: `Sampler`, src/init.cpp:124-173, held in an externalptr */

/* dbartsControl + dbartsModel fields the reference sets (R/stan4bart_fit.R:436-479) */
typedef struct {
  int32_t n_trees;      /* control@n.trees (bart_args$n.trees)                       */
  int32_t n_thin;       /* control@n.thin = skip.bart (R/stan4bart_fit.R:438)         */
  int32_t keep_trees;   /* control@keepTrees                                          */
  int32_t node_capacity;/* 0 = default (256): max node slots per tree on the device   */
  double base, power;   /* cgm(power = 2, base = 0.95)                                */
  double k;             /* normal(k = 2): the fixed k, or the value a modeled k starts from */
  double node_scale;    /* model@node.scale: 0.5 continuous, 3.0 binary (:477-479)    */
  double birth_or_death_prob, swap_prob, change_prob, birth_prob; /* dbarts: .5 .1 .4 .5 */
  const double* split_probs; /* cgm(split.probs = ): NULL (predictors equally likely) or one positive weight per predictor, any scale:
                              * a rule's predictor is drawn with probability weight / sum of the weights of the predictors still
                              * available at the node, and the tree prior carries the same term (R/stan4bart_fit.R:466-475;
                              * tests/testthat/test-09-bartArgs.R:20).  Tree updates then run on the persistent sweep's k_sweep_sp
                              * where that applies, else on the two-kernel path.                                                */
  int32_t use_quantiles;     /* dbartsControl(useQuantiles = ) through bart_args (R/stan4bart_fit.R:440-444): 0 uniform cut points
                              * between the column extremes, 1 cut points from the distinct values (n_cuts is then a maximum)    */
  int32_t interface_version; /* must be S4B_INTERFACE_VERSION: create() refuses anything else.  This struct and s4b_results have grown fields over the revisions
                              * (k_hyper_*, bart_k) and carry no size field: a caller compiled against an older header would pass short structs, and
                              * run() would read past their end.  The word was `reserved` (0) in those headers, so such a caller is refused at
                              * create() — before any of the newer fields is read — instead of being served garbage. */
  /* normal(k = chi(degreesOfFreedom, scale)) — reference R/stan4bart.R:202 ("allow calls like bart_args = list(k = chi(2, Inf))"),
   * R/stan4bart_fit.R:460-465, tests/testthat/test-09-bartArgs.R:32; model@node.hyperprior, `kPrior->isFixed` src/init.cpp:272,731.
   * k_hyper_df <= 0: k is fixed (`k` above).  k_hyper_df > 0: k is a parameter with prior density k^(df - 1) exp(-k^2 / (2 scale^2))
   * (k_hyper_scale may be +Inf) that is redrawn once per sweep, after the trees (and the latents of a binary response), from its
   * conditional given the leaf values (k^2 ~ Gamma((df + #leaves) / 2, rate (T sum mu^2 / node_scale^2 + 1 / scale^2) / 2), one rgamma from
   * R's stream); its draws come back in s4b_results.bart_k. */
  double k_hyper_df, k_hyper_scale;
} s4b_bart_control;

/* dbartsData slots (R/lme4_functions.R:176, R/stan4bart_fit.R:449-451) */
typedef struct {
  int64_t n;            /* numObservations                                            */
  int32_t p;            /* numPredictors                                              */
  int32_t reserved;
  const double* x;      /* n x p, data@x                                              */
  const int32_t* n_cuts;/* p, data@n.cuts (default 100 each)                          */
  int64_t n_test;       /* numTestObservations                                        */
  const double* x_test; /* n_test x p or NULL, data@x.test                            */
} s4b_bart_data;

/* the `stanData` list: same names as dataNames[] (reference src/stan_sampler.cpp:67-80) */
typedef struct {
  int64_t N; int32_t K;
  int32_t is_binary, has_intercept, has_weights;
  int32_t prior_dist, prior_dist_for_aux;           /* 0 none,1 normal,2 student_t,3 hs,4 hs_plus,5 laplace,6 lasso,7 product_normal / aux: 0..2, 3 exponential */
  const double* X;            /* N x K, column-centred fixed-effect design (R/rstanarm_functions.R:420-446) */
  const double* y;            /* N */
  const double* weights;      /* N or NULL */
  const double* prior_scale;  /* K */
  const double* prior_mean;   /* K */
  const double* prior_df;     /* K */
  double prior_scale_for_aux, prior_mean_for_aux, prior_df_for_aux;
  int32_t t;                  /* number of grouping terms */
  int32_t q;                  /* columns of Z */
  int32_t len_theta_L, len_concentration, len_regularization, reserved;
  const int32_t* p;           /* t */
  const int32_t* l;           /* t */
  const double* shape;        /* t */
  const double* scale;        /* t */
  const double* concentration;   /* len_concentration */
  const double* regularization;  /* len_regularization */
  int64_t num_non_zero;
  const double* w;            /* num_non_zero: CSR values of Z  */
  const int32_t* v;           /* num_non_zero: 0-based columns  */
  const int32_t* u;           /* N + 1: 0-based row starts      */
  /* coefficient prior families beyond normal / student_t (continuous.stan:124-144, 298-322, 382-414):
   * prior_dist 3 hs, 4 hs_plus, 5 laplace, 6 lasso, 7 product_normal */
  double global_prior_df, global_prior_scale, slab_df, slab_scale;   /* hs, hs_plus */
  const int32_t* num_normals; /* K (>= 2 each), product_normal only, else NULL */
} s4b_stan_data;

/* the `stanControl` list with the reference defaults (src/stan_sampler.cpp:395-458) */
typedef struct {
  uint32_t seed;              /* required */
  int32_t skip;               /* <=0 : NA -> max(1,(2000 - warmup)/1000) (src/init.cpp:206-209) */
  double init_r;              /* 2.0 */
  double adapt_gamma, adapt_delta, adapt_kappa, adapt_t0;   /* .05 .8 .75 10 */
  uint32_t adapt_init_buffer, adapt_term_buffer, adapt_window, reserved;  /* 75 50 25 */
  double stepsize, stepsize_jitter;  /* 1, 0 */
  int32_t max_treedepth;      /* 10 */
  int32_t hmc_mode;           /* extension: 0 = sufficient-statistic (Gram) gradient, 1 = per-leapfrog O(N) kernels */
} s4b_stan_control;

/* per-iteration callback (src/init.cpp:849-911); a non-zero return stops the run after that iteration (status 1, "stopped by the
 * per-iteration callback") — the reference's callback is R code whose error unwinds run() */
typedef int (*s4b_callback_fn)(void* user, const double* yhat_train, const double* yhat_test,
                               const double* stan_pars, int32_t num_pars);
/* progress / cancellation hook of run(): called before iteration `iter` (1-based) of `num_iter` for iter = 1 and whenever iter is
 * a multiple of common_control.refresh (every iteration when refresh <= 0); a non-zero return stops the run (status 1,
 * "interrupted ...").  With a hook installed run() prints nothing itself: the hook's owner prints the reference's
 * "starting warmup ..." and "iter k / n" lines (the R shim does, shim/init_shim.cpp).
 * Reference: "iter k / n" lines (src/init.cpp:752-754) and R_CheckUserInterrupt per transition (src/stan_sampler.hpp:44-48). */
typedef int (*s4b_progress_fn)(void* user, int32_t iter, int32_t num_iter, int32_t is_warmup);

/* the `commonControl` list (src/init.cpp:199-202, 1015-1051) */
typedef struct {
  int32_t warmup, iter, verbose, refresh;
  int32_t is_binary;
  int32_t offset_type;        /* 0 default,1 fixef,2 ranef,3 bart,4 parametric (src/init.cpp:83-97) */
  int32_t keep_fits;
  int32_t device;             /* extension: HIP device ordinal for this chain */
  const double* offset;       /* N or NULL: user offset */
  const double* bart_offset_init; /* N or NULL */
  double sigma_init;          /* > 0, default 1 */
  s4b_callback_fn callback;   /* NULL or per-iteration callback (src/init.cpp:849-911) */
  void* callback_user;
} s4b_common_control;

/* caller-allocated result buffers of one run() (layouts: src/stan_sampler.cpp:577-596, src/bart_util.cpp:13-81).
 * num_samples = keep_fits ? num_iter : 1; any pointer may be NULL to skip that output. */
typedef struct {
  double* stan;          /* num_pars x num_samples */
  double* bart_sigma;    /* num_samples            */
  double* bart_train;    /* n x num_samples        */
  double* bart_test;     /* n_test x num_samples   */
  int32_t* bart_varcount;/* p x num_samples        */
  double* bart_k;        /* num_samples: the draws of a modeled k (k_hyper_df > 0; reference result element "k", src/bart_util.cpp:17-26,60-64,75-76);
                          * with a fixed k the buffer, if given, is filled with that value */
} s4b_results;

/* R's generator state as 625 words {mti, mt[0..623]} == .Random.seed[2:626]
 * (reference brackets every entry with GetRNGstate/PutRNGstate: src/init.cpp:259,298,750,919) */
#define S4B_R_RNG_WORDS 625

const char* S4B_FN(last_error)(void);

/* stan4bart_create(bartControl, bartData, bartModel, stanData, stanControl, commonControl) — src/init.cpp:190-310 */
int S4B_FN(create)(const s4b_bart_control* bart_control, const s4b_bart_data* bart_data,
                   const s4b_stan_data* stan_data, const s4b_stan_control* stan_control,
                   const s4b_common_control* common_control, const uint32_t* r_rng_state,
                   s4b_sampler** out);

/* stan4bart_run(sampler, numIter, isWarmup, resultsType) — src/init.cpp:678-965; results_type 0 both,1 bart,2 stan */
int S4B_FN(run)(s4b_sampler* s, int32_t num_iter, int32_t is_warmup, int32_t results_type, s4b_results* out);

/* stan4bart_disengageAdaptation — src/init.cpp:995-1004 */
int S4B_FN(disengage_adaptation)(s4b_sampler* s);

/* stan4bart_printInitialSummary — src/init.cpp:971-993 (writes to stdout) */
int S4B_FN(print_initial_summary)(s4b_sampler* s);

/* stan4bart_getParametricMean — src/init.cpp:332-347: X beta + Z b of the last Stan draw, N doubles */
int S4B_FN(get_parametric_mean)(s4b_sampler* s, double* out);

/* stan4bart_getBARTDataRange — src/init.cpp:316-330: {min, max} of the response rescaling */
int S4B_FN(get_bart_data_range)(s4b_sampler* s, double out[2]);

/* PutRNGstate()/GetRNGstate() counterparts */
int S4B_FN(get_r_rng_state)(s4b_sampler* s, uint32_t* state);
int S4B_FN(set_r_rng_state)(s4b_sampler* s, const uint32_t* state);

/* sizes: num_pars (rows of the stan result), n, n_test, p, n_trees */
int S4B_FN(get_dims)(s4b_sampler* s, int64_t dims[5]);

/* row names of the stan result (src/stan_sampler.cpp:476-489): writes a '\n'-joined list */
int S4B_FN(get_stan_par_names)(s4b_sampler* s, char* buf, size_t cap);

/* stan4bart_getTrees(current = TRUE) — src/init.cpp:514-671 flattened-tree layout for the live trees:
 * preorder per tree; var >= 0: internal node (value = cut point), var = -1: leaf (value = mu on the
 * rescaled scale).  Returns the node count through *num_nodes; arrays may be NULL to query the size. */
int S4B_FN(get_trees)(s4b_sampler* s, int64_t cap, int32_t* tree, int32_t* n_obs, int32_t* var,
                      int32_t* split, double* value, int64_t* num_nodes);

/* stan4bart_getTrees(current = FALSE) — src/init.cpp:514-671 over the draws kept while sampling (keep_trees; also on a
 * stored sampler): sample < 0 selects every kept draw, otherwise that draw (0-based).  Same layout as get_trees plus
 * the draw index of every node. */
int S4B_FN(get_kept_trees)(s4b_sampler* s, int64_t sample, int64_t cap, int32_t* sample_index, int32_t* tree, int32_t* n_obs,
                           int32_t* var, int32_t* split, double* value, int64_t* num_nodes);

/* stan4bart_getTrees(chainIndices, sampleIndices, treeIndices, current = FALSE) — src/init.cpp:514-671 with its index vectors:
 * 0-based draw / tree indices (NULL = all).  A sampler is one chain; the R shim loops over chainIndices. */
int S4B_FN(get_kept_trees_indexed)(s4b_sampler* s, const int32_t* sample_idx, int64_t num_samples, const int32_t* tree_idx, int64_t num_trees,
                                   int64_t cap, int32_t* sample_index, int32_t* tree, int32_t* n_obs, int32_t* var, int32_t* split, double* value,
                                   int64_t* num_nodes);

/* stan4bart_printTrees(chainIndices, sampleIndices, treeIndices) — src/init.cpp:448-512: prints the selected kept trees to stdout.
 * The reference forwards to dbarts' printer, whose text format is not part of the reference tree: the layout here is this
 * library's own (one node per line, indented by depth). */
int S4B_FN(print_trees)(s4b_sampler* s, const int32_t* sample_idx, int64_t num_samples, const int32_t* tree_idx, int64_t num_trees);

/* progress / cancellation hook (see s4b_progress_fn); fn = NULL removes it */
int S4B_FN(set_progress)(s4b_sampler* s, s4b_progress_fn fn, void* user);

/* stan4bart_exportBARTState — src/init.cpp:409-416 (+ R/stan4bart_fit.R:572-580): the trees kept while sampling (keep_trees),
 * the cut points and the response scales as one relocatable byte string, so that a chain fitted in another process can be
 * predicted from.  Call with buf = NULL (or cap too small) to learn the size. */
int S4B_FN(export_bart_state)(s4b_sampler* s, void* buf, int64_t cap, int64_t* size);

/* stan4bart_createStoredBARTSampler — src/init.cpp:418-446: a sampler that only holds an exported state; it supports
 * predict_bart, export_bart_state, get_dims and free, everything else fails with a message. */
int S4B_FN(create_stored_bart_sampler)(const void* state, int64_t size, int32_t device, s4b_sampler** out);

/* stan4bart_predictBART(storedSampler, x_test, offset_test = NULL) — src/init.cpp:354-403, with the rescaling of
 * R/generics.R:671-674 folded in: BART fit of every kept draw at new predictor rows, on the data scale (probit: the
 * latent scale).  Trees are kept for the non-warmup runs of a sampler created with bart_control.keep_trees = 1
 * (reference: keepTrees is switched on only for the sampling phase, src/init.cpp:216-221,737-744).
 * out is n_test x num_samples (column-major); pass out = NULL to query num_samples. */
int S4B_FN(predict_bart)(s4b_sampler* s, const double* x_test, int64_t n_test, double* out, int64_t* num_samples);
/* the same with the reference's third argument: offset_test (n_test doubles, or NULL) is added to every draw's prediction */
int S4B_FN(predict_bart_offset)(s4b_sampler* s, const double* x_test, int64_t n_test, const double* offset_test, double* out, int64_t* num_samples);

/* extension (no reference counterpart; the reference forms these numbers in R from the full draws matrix of predictBART): SUMMARIES of the
 * predictions of the kept draws at new rows, formed on the device without the n_test x num_samples matrix.  For row i and kept draw k
 *     z(i,k) = bart(i,k) + offset[i] + sum_{j < n_dense} dense[i,j] dense_coef[k,j]                                   (j ascending)
 *                                    + sum_{e < n_ell, ell_index[i,e] >= 0} ell_value[i,e] ell_coef[k, ell_index[i,e]]  (e ascending)
 *     v(i,k) = z(i,k) (link 0) or Phi(z(i,k)), the standard normal cdf (link 1)
 * with bart(i,k) exactly predict_bart's value (no rescale for a binary response: the latent scale).  Per row: mean[i] and
 * m2[i] = sum_k (v(i,k) - mean[i])^2 over the draws (Welford's update in draw order; the variance is m2 / (num_samples - 1)).  Per draw:
 * average[k,g] = sum_i weights[g,i] v(i,k) for n_weights <= 8 weight vectors, used as given (1 / n_test: the sample average; an indicator over
 * its count: a subgroup's).  Two calls on one device return the same bits: no floating-point atomics, fixed orders.
 * Layouts: x_test (n_test x p), dense (n_test x n_dense), ell_index and ell_value (n_test x n_ell) are column-major over the rows, as every matrix
 * here; ell_index -1 marks padding (the entry is skipped), every other index lies in [0, n_ell_coef); the coefficient tables have ONE ROW PER DRAW:
 * dense_coef[k * n_dense + j], ell_coef[k * n_ell_coef + c]; weights[g * n_test + i]; average is draw-major: average[k * n_weights + g].
 * offset, dense*, ell_*, weights may be NULL when their count is 0 (offset: always).  Everything is checked before anything is launched.
 * Works on a sampler with kept trees (keep_trees, sampling runs) and on a stored sampler.  out->mean = m2 = average = NULL (or in = NULL): only
 * num_samples is set.  Device memory of a call: DESIGN.md 5.5 (no term grows with n_test x num_samples). */
typedef struct {
  const double* x_test; int64_t n_test;
  const double* offset;          /* n_test or NULL */
  int32_t n_dense, n_ell, n_ell_coef, link, n_weights;
  int32_t route;                 /* 0 automatic; 1 the LDS-staged kernel where the largest kept draw fits its staging buffers, else global; 2 the global-memory walk */
  int32_t stage_nodes;           /* 0, or an upper limit on the nodes per staging buffer below the library's own (less LDS per workgroup; a draw beyond it: global route) */
  int32_t max_workgroups;        /* 0, or an upper limit on the workgroups below the library's own (bounds the scratch of the per-draw sums) */
  const double* dense; const double* dense_coef;
  const int32_t* ell_index; const double* ell_value; const double* ell_coef;
  const double* weights;
} s4b_summary_in;
typedef struct {
  double* mean; double* m2;      /* n_test each */
  double* average;               /* num_samples x n_weights, draw-major; may be NULL when n_weights = 0 */
  int64_t num_samples;
  /* what the call did: [0] route taken (1 LDS-staged, 2 global; 0: nothing was launched), [1] rows per tile (= threads per workgroup), [2] workgroups,
   * [3] staging bytes per buffer (nodes and tree starts; 0 on the global route), [4] nodes of the largest kept draw, [5] kernel launches,
   * [6] bytes of device memory the call allocated, [7] nodes per staging buffer */
  int64_t info[8];
} s4b_summary_out;
int S4B_FN(predict_summary)(s4b_sampler* s, const s4b_summary_in* in, s4b_summary_out* out);

/* extension (dbarts' pdbart / pd2bart, formed on the device): the PARTIAL DEPENDENCE of the kept draws on one or two BART predictors.  For grid point g,
 * which assigns grid[g + w * n_grid] to predictor vars[w] (w < n_vars; two predictors: a joint grid, the caller lists the pairs), and kept draw k
 *     pd[k * n_grid + g] = sum_i weight[i] * v(i, g, k),     v = z (link 0) or Phi(z) (link 1),
 *     z(i, g, k) = bart(row i with x[vars[w]] replaced by the grid point's values; draw k) + the linear parts of predict_summary at row i, draw k
 * in ONE call that walks the trees without a rule on a varied predictor once per (row, draw) and only the others per grid point.
 * THE VARIED PREDICTORS ARE BART PREDICTORS ONLY: offset, dense and ELL parts stay at the rows' own values, whatever the grid.  `rows` is
 * predict_summary's input with n_weights 0 (weight 1 / n_test: the sample average) or 1 (weights[i]); route, stage_nodes and max_workgroups mean what
 * they mean there.  The grid is binned as rows are (+-inf allowed: the ends; a NaN is refused).  There are no per-row outputs: the individual curves
 * are predict_summary's mean per grid value.  The trees of a draw are added in another order than predict_bart adds them, so the BART term agrees with
 * it to rounding, not bit for bit; two calls, both routes, live and stored samplers return the same bits.  Everything is checked before anything is
 * launched.  out->pd = NULL (or in = NULL): only num_samples is set. */
typedef struct {
  s4b_summary_in rows;
  int32_t n_vars, vars[2], n_grid;   /* 1 or 2 distinct predictors in [0, p); 1 <= n_grid <= 64 */
  const double* grid;                /* n_grid x n_vars, column-major */
} s4b_pd_in;
typedef struct {
  double* pd;                        /* num_samples x n_grid, draw-major */
  int64_t num_samples;
  /* as s4b_summary_out.info, except: [3] staging bytes per buffer (nodes, tree starts and the tree order: 16 x nodes + 8 x trees), [4] nodes of the
   * largest kept draw (the staged route needs them in one buffer, with 16 KB of reduction space and both order tables inside the 160 KB of LDS),
   * [7] the trees with a rule on a varied predictor: (the most in one draw) << 32 | (their sum over the draws) */
  int64_t info[8];
} s4b_pd_out;
int S4B_FN(partial_dependence)(s4b_sampler* s, const s4b_pd_in* in, s4b_pd_out* out);

/* extension (R: apply(extract(fit), 1, quantile, probs), formed on the device): per-row QUANTILES of predict_summary's value v(i,k) — the same z, the
 * same order of the additions, link 0 or 1 — over the kept draws of `s` AND of n_peers further samplers, pooled in one call: quantiles do not merge
 * the way moments do, so the chains of a fit are handed to one call instead of one call each.  The pooled draws are those of `s`, then the peers' in
 * their order, S in all (S <= 16384); a handle may occur more than once.  R's type 7 (numpy's default) over the sorted values x(0) <= ... <= x(S-1)
 * of row i:     h = p (S - 1),  lo = floor(h),  hi = min(lo + 1, S - 1),  g = h - lo,  q = x(lo) + g (x(hi) - x(lo))     (g = 0: x(lo) unchanged)
 * `rows` is predict_summary's input with n_weights 0; its dense_coef / ell_coef are the tables of `s` (one row per draw of `s`), peer_dense_coef[x] /
 * peer_ell_coef[x] those of peer x (one row per draw of that peer).  The rows are binned once, with the cut points of `s`: every peer must have the
 * same number of predictors and of trees per draw, the same kind of response and bit-identical cut points (samplers of one fit do), and must hold kept
 * draws.  Everything is checked before anything is launched; a refused call leaves info all zero.  The rows are processed in chunks of C rows whose
 * values (C x S doubles) are the only rows-times-draws storage of the call: C = scratch / (8 S) rounded down to a multiple of 64, at least 64, at most
 * n_test, with scratch = scratch_bytes or the library's own limit.  Two calls, both routes, live and stored samplers, any order of
 * the peers return the same bits.  out->quantiles = NULL (or in = NULL): only num_samples is set, to the kept draws of `s` alone. */
typedef struct {
  s4b_summary_in rows;
  int32_t n_probs;                /* 1 .. 16 */
  const double* probs;            /* each in [0, 1], no NaN; duplicates and any order allowed */
  int32_t n_peers;                /* >= 0 */
  s4b_sampler* const* peers;      /* live (kept trees) or stored samplers */
  const double* const* peer_dense_coef;   /* [n_peers] tables (peer's draws x n_dense), NULL when n_dense = 0 */
  const double* const* peer_ell_coef;     /* [n_peers] tables (peer's draws x n_ell_coef), NULL when n_ell = 0 */
  int64_t scratch_bytes;          /* 0, or an upper limit below the library's own on the value scratch (fewer rows per chunk) */
} s4b_quantile_in;
typedef struct {
  double* quantiles;              /* n_probs x n_test, prob-major: quantiles[j * n_test + i] */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did: [0] route of the value kernel (1 LDS-staged, 2 global; 0: nothing was launched), [1] rows per chunk C, [2] chunks,
   * [3] (rows sorted side by side per workgroup) << 32 | draws padded to a power of two, [4] nodes of the largest pooled draw, [5] kernel launches
   * (2 per chunk), [6] bytes of device memory the call allocated, [7] pooled draws */
  int64_t info[8];
} s4b_quantile_out;
int S4B_FN(predict_quantiles)(s4b_sampler* s, const s4b_quantile_in* in, s4b_quantile_out* out);

/* extension (R: samples.icate <- (mu.train - mu.test) * (2 z - 1) and its row / column summaries, formed on the device): the PAIRED CONTRAST of two
 * arms over the same n_test rows and the same draws, pooled over `s` and its peers as predict_quantiles pools them.  For arm a = 1, 0
 *     z_a(i,k) = bart(x_a[i]; k) + offset_a[i] + sum_j dense_a[i,j] dense_coef[k,j] + sum_e ell_value_a[i,e] ell_coef[k, ell_index_a[i,e]]
 *     d(i,k)   = v(z_1) - v(z_0),      v = identity (link 0) or Phi (link 1)
 * The coefficient tables belong to the draw and are shared by the arms; only the row side differs.  `rows` is arm 1 (predict_summary's input, with
 * the weights: 0 <= n_weights <= 8).  x_test0 is arm 0's predictor matrix, column-major like x_test (NULL: arm 1's); offset0, dense0, ell_index0,
 * ell_value0 are arm 0's row side of the linear parts, each NULL (arm 1's) or shaped as the arm-1 part; an arm-0 part given where arm 1 has none is
 * refused.  Both arms are binned with the cut points of `s`; the BART columns whose BINS differ in at least one row — two raw values on the same side
 * of every cut do not differ — may number at most 2 (more: refused, the message names them).  Trees without a rule on such a column return the same
 * leaf in both arms: under link 0 they and every linear part whose arm-0 pointer is NULL cancel and are not evaluated at all; under link 1 they are
 * walked once for both arms.  Both arms go through the same arithmetic and d is (arm 1) - (arm 0): swapping the arms negates d bit for bit.
 * Outputs, none of which needs more rows-times-draws storage than a chunk's scratch (C x S doubles, C as predict_quantiles chooses it):
 *   mean[i], m2[i]      mean and sum of squared deviations of d(i, .) over the S pooled draws (two passes; variance m2 / (S - 1)); both or neither
 *   average[k, g]       sum_i weights[g,i] d(i,k), draw-major over the pooled draws (1 / n_test: the sample average effect; an indicator of the
 *                       treated over their count: the effect on the treated), rows added in row order within slabs of 64, slabs in order
 *   quantiles[j, i]     R's type 7 quantiles of d(i, .), 0 <= n_probs <= 16, prob-major
 * The peer rules, the pooled order, the limit of 16384 pooled draws, scratch_bytes and the query form (all outputs NULL or in = NULL: num_samples of
 * `s` alone) are predict_quantiles'.  Everything is checked before anything is launched; a refused call leaves info all zero.  Two calls, both routes,
 * live and stored samplers return the same bits; mean, m2 and quantiles do not depend on the chunking.  Device memory: DESIGN.md 5.8. */
typedef struct {
  s4b_summary_in rows;            /* arm 1, the coefficient tables of `s`, the weights */
  const double* x_test0;          /* n_test x p, or NULL */
  const double* offset0; const double* dense0; const int32_t* ell_index0; const double* ell_value0;   /* arm 0's row side, each NULL or as in `rows` */
  int32_t n_probs;                /* 0 .. 16 */
  const double* probs;
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  int64_t scratch_bytes;
} s4b_contrast_in;
typedef struct {
  double* mean; double* m2;       /* n_test each; both or neither */
  double* average;                /* num_samples x n_weights, draw-major; NULL when n_weights = 0 */
  double* quantiles;              /* n_probs x n_test, prob-major; NULL when n_probs = 0 */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did: [0] route of the value kernel (1 LDS-staged, 2 global, 0: no tree was walked — link 0 and no affected tree), [1] rows per chunk,
   * [2] chunks, [3] kernel launches (per chunk: values, + reduce with a per-row output or weights, + fold with weights, + sort with probs),
   * [4] bytes of device memory the call allocated, [5] pooled draws, [6] D, the differing BART columns, [7] the trees with a rule on one of them:
   * (the most in one draw) << 32 | (their sum over the pooled draws) */
  int64_t info[8];
} s4b_contrast_out;
int S4B_FN(predict_contrast)(s4b_sampler* s, const s4b_contrast_in* in, s4b_contrast_out* out);

/* extension (R: the group-by over the rows of extract(fit) or of samples.icate — the average fitted value of every school, the average treatment
 * effect of every site with its interval and the probability that it is positive — formed on the device): PER-LEVEL sums or means of the rows' values
 * per pooled draw, summarised over the draws.  Row i belongs to level level[i] in [0, n_levels) and carries the weight w_i >= 0 (every w_i = 1 with
 * arms.rows.n_weights = 0, weights[i] with n_weights = 1).  With the S pooled draws of `s` and its peers
 *     a(l,k) = sum_{i : level[i] = l} w_i x(i,k),     x = v(z_1) (n_arms 1: predict_quantiles' value) or v(z_1) - v(z_0) (n_arms 2: predict_contrast's d)
 *     A(l,k) = a(l,k) (statistic 0, the sum) or a(l,k) / W_l, W_l = sum_{i : level[i] = l} w_i (statistic 1, the mean)
 * THE ROWS OF A LEVEL ARE CONTIGUOUS: `level` is non-decreasing (a caller with labels in any order sorts its rows by a stable sort first; the Python
 * binding does).  The order of the additions is fixed and is part of the interface: the rows are cut into slabs of 64 (rows 0..63, 64..127, ...,
 * whatever the chunking); a(l,k) is the left fold, over the slabs the level touches in ascending order, of the slab's partial; a partial is the left
 * fold, over the level's rows in the slab in row order, of w_i x(i,k) (without weights: of x(i,k)); the first term of a fold is taken as it is.  No
 * floating-point atomics, no data-dependent order: the result does not depend on the chunking, the route, or live versus stored samplers, and a
 * level of one row with weight 1 is that row's value bit for bit.  W_l and count[l] are formed on the host in row order, in double.
 * `arms` is predict_contrast's input: the rows, arm 0, probs (0 .. 16), peers, scratch_bytes mean what they mean there; with n_arms 1 every arm-0
 * pointer must be NULL.  Per level:
 *   mean[l], m2[l]      mean and sum of squared deviations of A(l, .) over the S draws (two passes, as predict_contrast forms a row's)
 *   quantiles[j, l]     R's type 7 quantiles of A(l, .), prob-major: quantiles[j * n_levels + l]
 *   p_above[l]          #{k : A(l,k) > threshold} / S (strict; needs has_threshold; +-inf allowed, NaN refused)
 *   weight[l], count[l] W_l and the rows of the level
 *   draws[l, k]         A itself, level-major: draws[l * S + k]
 * A level without rows, or with W_l = 0 under statistic 1, gets NaN in every floating output (weight[l] stays 0); a level whose weights are all 0
 * under statistic 0 gets exact zeros.  The level matrix (8 n_levels S bytes) stays on the device for the call: it may be at most
 * S4B_GROUPS_LEVEL_BYTES_MAX, or level_bytes where that is given and smaller; a caller with more levels splits them into consecutive ranges (a range
 * of levels is a slice of the sorted rows).  Refused before anything is launched, info left all zero: a decreasing label, a label outside
 * [0, n_levels), a negative or non-finite weight, n_arms outside {1, 2}, an arm-0 pointer with n_arms 1, a statistic outside {0, 1}, 8 n_levels S
 * above the limit, and whatever predict_contrast refuses.  The peer rules, the limit of 16384 pooled draws and the query form (every output NULL, or
 * in = NULL: num_samples of `s` alone) are predict_quantiles'.  Device memory: DESIGN.md 5.12 (no term grows with n_test x S beyond a chunk). */
#define S4B_GROUPS_LEVEL_BYTES_MAX ((int64_t)1 << 30)   /* 1 GiB: the level matrix of one s4b_predict_groups call at most */
typedef struct {
  s4b_contrast_in arms;           /* rows (n_weights 0 or 1), arm 0, probs, peers, scratch_bytes: predict_contrast's meaning */
  int32_t n_arms;                 /* 1: x = v(z_1), every arm-0 pointer NULL; 2: the contrast */
  const int32_t* level;           /* n_test, non-decreasing, each in [0, n_levels) */
  int64_t n_levels;
  int32_t statistic;              /* 0 sum, 1 mean */
  int32_t has_threshold; double threshold;
  int64_t level_bytes;            /* 0, or a limit below the library's own on 8 n_levels S */
} s4b_groups_in;
typedef struct {
  double* mean; double* m2;       /* n_levels each, independently NULL where not wanted */
  double* quantiles;              /* n_probs x n_levels, prob-major; NULL when n_probs = 0 */
  double* p_above; double* weight; int64_t* count;   /* n_levels each */
  double* draws;                  /* n_levels x num_samples, level-major */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did: [0] route of the value kernel (as s4b_contrast_out.info[0]), [1] rows per chunk, [2] chunks, [3] kernel launches (per chunk:
   * values, k_level_reduce, + k_level_fold where a level of the chunk has edge partials; then k_level_rows, + the sort per 2^20 levels with probs),
   * [4] bytes of device memory the call allocated, [5] pooled draws, [6] levels with edge partials (those touching more than one slab), [7] levels
   * whose floating outputs are NaN (no rows, or W_l = 0 under statistic 1) */
  int64_t info[8];
} s4b_groups_out;
int S4B_FN(predict_groups)(s4b_sampler* s, const s4b_groups_in* in, s4b_groups_out* out);

/* extension (R: posterior summarisation — lm(effect ~ moderators, weights) of every row of t(samples.icate), or of the fitted values, and the posterior
 * of its coefficients and of its R^2 — formed on the device): the PROJECTION of the rows' values on a small design by weighted least squares PER POOLED
 * DRAW, summarised over the draws.  Row i carries the design row A(i, .) of n_columns = K entries, 1 <= K <= S4B_PROJECTION_COLUMNS_MAX, row-major
 * (design[i * K + j]), taken as given: no intercept is added.  Weights w_i >= 0 (every w_i = 1 with arms.rows.n_weights = 0, weights[i] with
 * n_weights = 1).  With the S pooled draws of `s` and its peers and x(i,k) = v(z_1) (n_arms 1: predict_quantiles' value) or v(z_1) - v(z_0) (n_arms 2:
 * predict_contrast's d)
 *     G(j,j') = sum_i w_i A(i,j) A(i,j')      b(j,k) = sum_i w_i A(i,j) x(i,k)      s(k) = sum_i w_i x(i,k)      t(k) = sum_i w_i x(i,k)^2
 *     W       = sum_i w_i, the host's sum in row order in double (part of the definition, returned as `weight`)
 *     G = L L' (Cholesky),   beta(., k) = G^-1 b(., k) by the two triangular solves,
 *     rss(k) = t(k) - sum_j beta(j,k) b(j,k),   tss(k) = t(k) - s(k)^2 / W,   r2(k) = 1 - rss(k) / tss(k)   (NaN where tss(k) == 0)
 * THE RANK RULE ACTS ON THE NORMAL EQUATIONS: the design is deficient where a pivot d_j = G(j,j) - sum_{p<j} L(j,p)^2 is not above tol G(j,j), before
 * its square root; tol in [0, 1), 0 meaning the default 1e-10.  G has the square of the design's condition number: columns whose scales differ by
 * orders of magnitude, or an intercept beside uncentred columns, lose pivots long before the design itself is deficient (the Python binding scales
 * every column by a power of two, which is exact; Stan4bartFit.predict_projection centres).  A deficient design (info[6] = 1), W == 0 (2) or
 * n_test == 0 (3) gives NaN in every floating output; nothing is partly filled.
 * THE ORDER OF THE ADDITIONS is fixed and part of the interface: the rows are cut into slabs of S4B_PROJECTION_SLAB = 128 (rows 0..127, 128..255, ...,
 * whatever the chunking: a chunk of this call is a multiple of 128 rows); with wx = w_i x(i,k) (x(i,k) itself without weights) a term of b is
 * A(i,j) wx, of s is wx, of t is wx x(i,k); a moment is the left fold, over the slabs in ascending order, of the slab's partial; a partial is the left
 * fold, over the slab's rows in row order, of the terms, begun from +0; the first partial of the fold over the slabs is taken as it is; a term and its
 * addition may be one fused multiply-add.  G is formed on the device by the same reduction with the design's own columns as the values, G(j,j') = sum_i A(i,j) (w_i A(i,j')),
 * and read for j >= j'.  The factorisation and the substitutions subtract their products in ascending index, rss subtracts beta(j,k) b(j,k) from t(k)
 * in ascending j.  No floating-point atomics, no data-dependent order: the result does not depend on scratch_bytes, the route, or live versus stored
 * samplers, bit for bit; multiplying a design column by a power of two divides its coefficient by it bit for bit and leaves everything else unchanged.
 * `arms` is predict_contrast's input: the rows, arm 0, probs (0 .. 16), peers, scratch_bytes mean what they mean there; with n_arms 1 every arm-0
 * pointer must be NULL.  Outputs; index K of the summaries is r2's:
 *   coef[j, k], r2[k]   beta and r2, coef[j * S + k]; small, always returned (both pointers are required)
 *   mean[l], m2[l]      mean and sum of squared deviations over the S draws (two passes, as predict_groups forms a level's), l <= K
 *   quantiles[q, l]     R's type 7 quantiles, prob-major: quantiles[q * (K + 1) + l]
 *   p_above[l]          #{k : value > threshold} / S (strict; needs has_threshold; +-inf allowed, NaN refused)
 *   weight              W
 * Refused before anything is launched, info left all zero: K outside [1, 32], K > n_test, a design entry or weight that is not finite, a negative
 * weight, n_arms outside {1, 2}, an arm-0 pointer with n_arms 1, tol outside [0, 1), a NULL coef or r2, and whatever predict_contrast refuses.  The
 * peer rules, the limit of 16384 pooled draws and the query form (every output NULL, or in = NULL: num_samples of `s` alone) are predict_quantiles'.
 * Device memory: DESIGN.md 5.13 (it grows with K S and n_test K; no term grows with n_test x S beyond a chunk). */
#define S4B_PROJECTION_COLUMNS_MAX 32
#define S4B_PROJECTION_SLAB 128
typedef struct {
  s4b_contrast_in arms;           /* rows (n_weights 0 or 1), arm 0, probs, peers, scratch_bytes: predict_contrast's meaning */
  int32_t n_arms;                 /* 1: x = v(z_1), every arm-0 pointer NULL; 2: the contrast */
  int32_t n_columns;              /* K */
  const double* design;           /* n_test x K, row-major */
  int32_t has_threshold; double threshold;
  double tol;                     /* pivot tolerance on the normal equations; 0: 1e-10 */
} s4b_projection_in;
typedef struct {
  double* coef; double* r2;       /* K x num_samples, num_samples: required */
  double* mean; double* m2;       /* K + 1 each, independently NULL where not wanted */
  double* quantiles;              /* n_probs x (K + 1), prob-major; NULL when n_probs = 0 */
  double* p_above;                /* K + 1 */
  double weight;                  /* W */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did: [0] route of the value kernel (as s4b_contrast_out.info[0]), [1] rows per chunk, [2] chunks, [3] kernel launches (per chunk:
   * k_proj_reduce and k_proj_fold for G; values, k_proj_reduce, k_proj_fold; then k_proj_solve, k_level_rows, + the sort with probs), [4] bytes of
   * device memory the call allocated, [5] pooled draws, [6] 0 answered, 1 deficient design, 2 W == 0, 3 no rows, [7] K */
  int64_t info[8];
} s4b_projection_out;
int S4B_FN(predict_projection)(s4b_sampler* s, const s4b_projection_in* in, s4b_projection_out* out);

/* extension (R: the heterogeneity of the effects — sd(icate), mean(icate > 0), range(icate) of every row of t(samples.icate) — and rstanarm's
 * bayes_R2, formed on the device): the SPREAD of the rows' values ACROSS THE ROWS within one pooled draw, summarised over the draws.  Every other
 * read-out summarises along the draws for a fixed row or adds rows linearly per draw; this one reads the distribution over the rows of one draw.
 * Row i carries the weight w_i >= 0 (every w_i = 1 with arms.rows.n_weights = 0, weights[i] with n_weights = 1).  thresholds[T],
 * 0 <= T <= S4B_SPREAD_THRESHOLDS_MAX, strictly ascending; +-inf allowed, NaN refused.  With the S pooled draws of `s` and its peers,
 * x(i,k) = v(z_1) (n_arms 1: predict_quantiles' value) or v(z_1) - v(z_0) (n_arms 2: predict_contrast's d) and
 * W = sum_i w_i, the host's sum in row order in double (part of the definition, returned as `weight`; W == 0 is refused), the call forms per pooled
 * draw k the matrix D[m, k] of M = 4 + 2 T statistics:
 *     m = 0          mean_k = sum_i w_i x(i,k) / W
 *     m = 1          sd_k = sqrt(M2_k / W),  M2_k = sum_i w_i (x(i,k) - mean_k)^2   (population form; exactly 0 for one row of positive weight)
 *     m = 2, 3       min_k, max_k over the rows with w_i > 0
 *     m = 4 + j      share_above[j] = (sum of w_i over the rows with x(i,k) > t_j) / W     (strict)
 *     m = 4 + T + j  part_above[j]  = (sum of w_i x(i,k) over the rows with x(i,k) > t_j) / W: the part of the mean contributed by the rows above t_j
 * part_above is always finite; the mean value among the rows above t_j is part_above / share_above, the gain of treating exactly those rows at cost
 * t_j is part_above - t_j share_above (callers form both; the matrix holds no NaN).  Over the draws, per statistic m:
 *   mean[m], m2[m]      mean and sum of squared deviations over the S draws (two passes, as predict_groups forms a level's)
 *   quantiles[q, m]     R's type 7 quantiles, prob-major: quantiles[q * M + m]
 *   draws[m, k]         D itself, statistic-major: draws[m * S + k] (at most 132 x 16384 doubles)
 *   weight              W
 * THE ORDER OF THE ADDITIONS is fixed and part of the interface: no floating-point atomics, no data-dependent order.  The rows are cut into slabs of
 * S4B_SPREAD_SLAB = 128 (rows 0..127, 128..255, ..., whatever the chunking: a chunk of this call is a multiple of 128 rows), so the result does not
 * depend on scratch_bytes, the route, or live versus stored samplers, bit for bit.
 *   Moments.  Per slab, with the shift c = the value of the slab's first row: W_s = fold of w_i, s1 = fold of w_i (x - c), s2 = fold of
 *   w_i (x - c)^2, left folds in row order from +0 (without weights the terms are 1, x - c, (x - c)^2); a term and its addition may be one fused
 *   multiply-add.  The slab's partial is (W_s, mean_s = c + s1 / W_s, M2_s = s2 - s1^2 / W_s, clamped at 0).  The partials combine over the slabs in
 *   ascending order by the pairwise update (Chan, Golub, LeVeque): delta = mean_b - mean_a, W_ab = W_a + W_b, mean = mean_a + delta W_b / W_ab,
 *   M2 = M2_a + M2_b + delta^2 W_a W_b / W_ab.  A partial with W_s = 0 is skipped; the first partial with positive weight is taken as it is.  The
 *   shift keeps the second moment from cancelling where the spread is small against the mean.  D divides by the host's W.
 *   Bins.  bin(x) = #{j : x > t_j} in [0, T].  Per slab and bin, cw[b] = fold of w_i and cs[b] = fold of w_i x in row order from +0; over the slabs
 *   they are added in ascending order; after the last chunk above_w[j] = sum_{b > j} cw[b] is added from b = T downward, above_s likewise.  Without
 *   weights cw are counts, exact in double: share_above is count / n_test exactly.
 *   Extremes are order-free.
 * Multiplying every weight by a power of two changes no output; one row gives mean = min = max = its value and sd = 0, bit for bit.
 * `arms` is predict_contrast's input: the rows, arm 0, probs (0 .. 16), peers, scratch_bytes mean what they mean there; with n_arms 1 every arm-0
 * pointer must be NULL.  Refused before anything is launched, info left all zero: T outside [0, 64], a NaN threshold, thresholds that are not
 * strictly ascending, n_weights > 1, a negative or non-finite weight, W == 0, n_arms outside {1, 2}, an arm-0 pointer with n_arms 1, bin_index
 * outside {0, 1, 2}, and whatever predict_contrast refuses.  The peer rules, the limit of 16384 pooled draws and the query form (every output NULL, or
 * in = NULL: num_samples of `s` alone) are predict_quantiles'.  Device memory: DESIGN.md 5.14 (no term grows with n_test x S beyond a chunk). */
#define S4B_SPREAD_THRESHOLDS_MAX 64
#define S4B_SPREAD_SLAB 128
typedef struct {
  s4b_contrast_in arms;           /* rows (n_weights 0 or 1), arm 0, probs, peers, scratch_bytes: predict_contrast's meaning */
  int32_t n_arms;                 /* 1: x = v(z_1), every arm-0 pointer NULL; 2: the contrast */
  int32_t n_thresholds;           /* T */
  const double* thresholds;       /* T, strictly ascending; NULL with T = 0 */
  int32_t bin_index;              /* how the kernel finds a value's bin: 0 the library's choice, 1 a count of compares, 2 a search (the same bin) */
} s4b_spread_in;
typedef struct {
  double* mean; double* m2;       /* 4 + 2 T each, independently NULL where not wanted */
  double* quantiles;              /* n_probs x (4 + 2 T), prob-major; NULL when n_probs = 0 */
  double* draws;                  /* (4 + 2 T) x num_samples, statistic-major */
  double weight;                  /* W */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did, in s4b_groups_out.info's layout: [0] route of the value kernel (as s4b_contrast_out.info[0]), [1] rows per chunk, [2] chunks,
   * [3] kernel launches (per chunk: values, k_spread_reduce, k_spread_fold; then k_spread_finish, + k_level_rows with mean or m2, + the sort with
   * probs), [4] bytes of device memory the call allocated, [5] pooled draws, [6] T, [7] slabs whose weight is 0 */
  int64_t info[8];
} s4b_spread_out;
int S4B_FN(predict_spread)(s4b_sampler* s, const s4b_spread_in* in, s4b_spread_out* out);

/* extension (R: quantiles and scores of extract(fit, "ppd") against held-out responses, formed on the device): the POSTERIOR PREDICTIVE read-out per row
 * over the draws of `s` and its peers, pooled as predict_quantiles pools them: prediction intervals for NEW OBSERVATIONS and the scores of held-out
 * responses y, without the rows-times-draws matrix.  Row i is a row of the call; k is the pooled draw index (the draws of `s`, then the peers' in peer
 * order); z(i,k) is predict_summary's z, the same additions in the same order.  `rows` is predict_summary's input with n_weights 0; rows.link names
 * the RESPONSE here: 0 continuous, 1 binary (probit).
 *   link 0   sd(i,k) = sigma[k] row_scale[i].  sigma holds one value per draw of `s`, peer_sigma[x] one per draw of peer x, each finite and > 0;
 *            row_scale has n_test values, finite and >= 0 (and > 0 when y is given), or is NULL: 1 (a fit with observation weights w passes
 *            1 / sqrt(w): the reference's sigma sqrt(1 / w)).
 *            y_rep(i,k) = z + sd e(i,k),   e(i,k) = sqrt(-2 log u1) cos(2 pi u2),   u1, u2 the two (0, 1] uniforms (53 bits each) of ONE block
 *            philox4x32_10({i low, i high, k, 0x50504431}, noise_key low, noise_key high).  The last counter word is a fixed tag ("PPD1") that no
 *            counter of the parallel probit latents carries (theirs is an attempt number below 4096), so the blocks differ even under one key.
 *            e is a pure function of (noise_key, i, k): chunking, route, scratch_bytes, live or stored samplers cannot change a bit of the result.
 *            quantiles[j, i]: R's type 7 of y_rep(i, .), 0 <= n_probs <= 16, prob-major.
 *            l(i,k) = -log(2 pi) / 2 - log sd - r^2 / 2,   r = (y_i - z) / sd
 *   link 1   no y_rep is formed: the predictive distribution of a row is Bernoulli(mean of ev), which predict_summary gives.  n_probs > 0 is refused.
 *            l(i,k) = log Phi(z) where y_i = 1, log Phi(-z) where y_i = 0 (the logarithm of Phi at the signed argument); every y is exactly 0 or 1;
 *            sigma, peer_sigma and row_scale are not read.
 * Scores, only when y (n_test values, finite) is given, S the pooled draw count:
 *   lpd[i]              m + log(sum_k exp(l - m)) - log S,  m = max_k l: the log pointwise predictive density
 *   lmean[i], lm2[i]    mean and sum of squared deviations of l(i, .) in two passes; both or neither.  The WAIC penalty is lm2 / (S - 1)
 *   pit[i]              (1 / S) sum_k Phi(r(i,k)); link 0 only: it must be NULL under link 1
 * A call that asks for nothing (no probs, no y with a score output) is refused.  The peer rules, the pooled order, the limit of 16384 pooled draws,
 * scratch_bytes, the rows per chunk and the query form (all outputs NULL or in = NULL: num_samples of `s` alone) are predict_quantiles'.  Everything
 * is checked before anything is launched; a refused call leaves info all zero.  Two calls return the same bits.  The draw reductions use a fixed
 * tree in pooled order and no floating-point atomics: a PERMUTED POOL may change the last bits of the scores, and it moves the noise (e belongs to
 * the pooled index k), so the quantiles of a permuted pool are those of another draw of the noise.  Device memory: DESIGN.md 5.9. */
typedef struct {
  s4b_summary_in rows;            /* n_weights 0; link: the response, 0 continuous, 1 binary */
  const double* y;                /* n_test held-out responses, or NULL: no scores */
  const double* sigma;            /* one per draw of `s` (link 0) */
  const double* row_scale;        /* n_test, or NULL: 1 */
  uint64_t noise_key;
  int32_t n_probs;                /* 0 .. 16; 0 under link 1 */
  const double* probs;
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  const double* const* peer_sigma;        /* [n_peers] vectors (one value per draw of that peer), link 0 */
  int64_t scratch_bytes;
} s4b_ppd_in;
typedef struct {
  double* quantiles;              /* n_probs x n_test, prob-major; NULL when n_probs = 0 */
  double* lpd;                    /* n_test, or NULL */
  double* lmean; double* lm2;     /* n_test each; both or neither */
  double* pit;                    /* n_test, or NULL; NULL under link 1 */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did, as s4b_quantile_out.info: [0] route of the value kernel (1 LDS-staged, 2 global; 0: nothing was launched), [1] rows per chunk C,
   * [2] chunks, [3] (rows per workgroup of k_ppd_rows) << 32 | draws padded to a power of two, [4] nodes of the largest pooled draw, [5] kernel
   * launches (2 per chunk), [6] bytes of device memory the call allocated, [7] pooled draws */
  int64_t info[8];
} s4b_ppd_out;
int S4B_FN(predict_ppd)(s4b_sampler* s, const s4b_ppd_in* in, s4b_ppd_out* out);

/* extension (R: rstanarm's pp_check / bayesplot's ppc_stat over posterior_predict's matrix, formed on the device): POSTERIOR PREDICTIVE CHECKS —
 * statistics of the replicate y_rep ACROSS THE ROWS within one pooled draw, each to be held against the same statistic of the observed y, summarised
 * over the draws.  predict_ppd forms y_rep and summarises it along the draws per row; predict_spread reads across the rows, but the expected value.
 * This call forms the replicate in registers, reduces it across the rows and never stores it.  `rows`, y, sigma, peer_sigma, row_scale, noise_key, the
 * peers and scratch_bytes are predict_ppd's and follow its rules (rows.n_weights 0; rows.link names the response); y is required.  Row i carries the
 * weight w_i >= 0 (row_weights, or NULL: every w_i = 1); W = sum_i w_i is the host's sum in row order in double (part of the definition, returned as
 * `weight`; W == 0 is refused).  thresholds[T], 0 <= T <= S4B_SPREAD_THRESHOLDS_MAX, strictly ascending, +-inf allowed; T must be 0 under link 1.
 * The replicate, z(i,k) being predict_ppd's z:
 *   link 0   y_rep(i,k) = z + sd e(i,k), sd = sigma[k] row_scale[i], e predict_ppd's deviate of (noise_key, i, k): THE SAME BITS predict_ppd sorts
 *            under the same key, so a check and an interval of one key speak of one replicate.
 *   link 1   y_rep(i,k) = 1 where u(i,k) <= Phi(z), else 0; u the (0, 1] uniform (53 bits) of the FIRST TWO words of the same Philox block
 *            (counter {i low, i high, k, 0x50504431}); Phi(z) = erfc(-z / sqrt 2) / 2.
 * Per pooled draw k the matrix D[m, k] of M = 7 + T statistics, x = y_rep:
 *     m = 0          mean_k = sum_i w_i x / W
 *     m = 1          sd_k = sqrt(M2_k / W),  M2_k = sum_i w_i (x - mean_k)^2       (population form)
 *     m = 2          m3_k = M3_k / W,        M3_k = sum_i w_i (x - mean_k)^3       (the skewness is m3 / sd^3: callers form it, NaN where sd = 0)
 *     m = 3, 4       min_k, max_k over the rows with w_i > 0
 *     m = 5 + j      share_above[j] = (sum of w_i over the rows with x > t_j) / W    (strict)
 *     m = 5 + T      disc_rep      m = 6 + T      disc_obs: the realised discrepancy of the replicate and of the observed y under draw k —
 *                    link 0 (chi^2 of Gelman, Meng and Stern): sum_i w_i e^2 / W  and  sum_i w_i ((y_i - z) / sd)^2 / W;
 *                    link 1 (the deviance): -2 sum_i w_i log Phi(+-z) / W, the sign + where y_rep (disc_rep) or y_i (disc_obs) is 1, - where it is 0.
 * The matrix holds no NaN (under link 1 a row WITH weight whose |z| lies beyond about 38 makes the deviance +inf, which is its value).  The posterior predictive p-value of a statistic is the share of draws with D[m, k] >= observed[m], of the discrepancy
 * the share with disc_rep >= disc_obs (callers form both from D).  Outputs:
 *   draws[m, k]         D itself, statistic-major: draws[m * S + k] (at most 71 x 16384 doubles); REQUIRED (NULL makes the call a query)
 *   observed[m]         m < 5 + T: the mean, sd, m3, min, max and share_above of y itself (x = y_i in the formulas above), formed on the host in the
 *                       same order of additions; or NULL
 *   mean[m], m2[m]      mean and sum of squared deviations of D[m, .] over the S draws (as predict_spread's); independently NULL
 *   quantiles[q, m]     R's type 7 quantiles, prob-major: quantiles[q * M + m]
 *   weight              W
 * THE ORDER OF THE ADDITIONS is fixed and part of the interface: no floating-point atomics, no data-dependent order.  The rows are cut into slabs
 * of S4B_SPREAD_SLAB = 128 (a chunk of this call is a multiple of 128 rows), and the deviate belongs to the row of the CALL, so the result does not
 * depend on scratch_bytes, the route, or live versus stored samplers, bit for bit.
 *   Moments.  Per slab, with the shift c = the replicate of the slab's first row and d_i = x_i - c: W_s = fold of w_i, s1 = fold of w_i d_i,
 *   s2 = fold of (w_i d_i) d_i, s3 = fold of ((w_i d_i) d_i) d_i, left folds in row order from +0; a term and its addition may be one fused
 *   multiply-add.  With d = s1 / W_s the slab's partial is (W_s, mean_s = c + d, M2_s = max(0, s2 - d s1), M3_s = (s3 - 3 d s2) + 2 d^2 s1).  The
 *   partials combine over the slabs in ascending order by the pairwise update: delta = mean_b - mean_a, W_ab = W_a + W_b,
 *       M3 = M3_a + M3_b + delta^3 W_a W_b (W_a - W_b) / W_ab^2 + 3 delta (W_a M2_b - W_b M2_a) / W_ab       (Pebay)
 *       M2 = M2_a + M2_b + delta^2 W_a W_b / W_ab,   mean = mean_a + delta W_b / W_ab                        (Chan, Golub, LeVeque)
 *   A partial with W_s = 0 is skipped; the first partial with positive weight is taken as it is.  D divides by the host's W.
 *   Bins.  bin(x) = #{j : x > t_j}.  Per slab and bin cw[b] = fold of w_i in row order from +0; over the slabs added in ascending order; after the
 *   last chunk above_w[j] = sum_{b > j} cw[b] is added from b = T downward.  Without weights cw are counts: share_above is count / n_test exactly.
 *   Discrepancies.  Per slab the fold of w_i (e e) and of w_i (r r), r = (y_i - z) / sd (link 0), or of w_i log Phi(+-z) (link 1), in row order
 *   from +0, a row with w_i = 0 adding no term (so a row without weight never brings 0 x -inf under link 1); over the slabs added in ascending
 *   order; D holds total / W (link 0), (-2 total) / W (link 1).
 *   Extremes are order-free.
 * Multiplying every weight by a power of two changes no output; multiplying sigma by a power of two and dividing row_scale by it changes none; one
 * row gives mean = min = max and sd = m3 = 0, bit for bit.  bin_index as predict_spread's.
 * Refused before anything is launched, info left all zero: T outside [0, 64], T > 0 under link 1, a NaN threshold, thresholds that are not strictly
 * ascending, a negative or non-finite weight, W == 0, bin_index outside {0, 1, 2}, NULL y, and whatever predict_ppd refuses of the rows, probs
 * (0 .. 16), y, sigma, row_scale and peers.  The limit of 16384 pooled draws and the query form (draws NULL, or in = NULL: num_samples of `s` alone)
 * are predict_quantiles'.  Device memory: DESIGN.md 5.15 (no term grows with n_test x S beyond a chunk). */
typedef struct {
  s4b_summary_in rows;            /* n_weights 0; link: the response, 0 continuous, 1 binary */
  const double* y;                /* n_test observed responses; required */
  const double* sigma;            /* one per draw of `s` (link 0) */
  const double* row_scale;        /* n_test, or NULL: 1 */
  uint64_t noise_key;
  const double* row_weights;      /* n_test, or NULL: 1 */
  int32_t n_thresholds;           /* T; 0 under link 1 */
  const double* thresholds;       /* T, strictly ascending; NULL with T = 0 */
  int32_t bin_index;              /* 0 the library's choice, 1 a count of compares, 2 a search (the same bin) */
  int32_t n_probs;                /* 0 .. 16 */
  const double* probs;
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  const double* const* peer_sigma;        /* [n_peers] vectors (one value per draw of that peer), link 0 */
  int64_t scratch_bytes;
} s4b_check_in;
typedef struct {
  double* mean; double* m2;       /* 7 + T each, independently NULL where not wanted */
  double* quantiles;              /* n_probs x (7 + T), prob-major; NULL when n_probs = 0 */
  double* draws;                  /* (7 + T) x num_samples, statistic-major; required */
  double* observed;               /* 5 + T, or NULL */
  double weight;                  /* W */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did, in s4b_spread_out.info's layout: [0] route of the value kernel (1 LDS-staged, 2 global), [1] rows per chunk, [2] chunks,
   * [3] kernel launches (per chunk: values, k_check_reduce, k_check_fold; then k_check_finish, + k_level_rows with mean or m2, + the sort with
   * probs), [4] bytes of device memory the call allocated, [5] pooled draws, [6] T, [7] slabs whose weight is 0 */
  int64_t info[8];
} s4b_check_out;
int S4B_FN(predict_check)(s4b_sampler* s, const s4b_check_in* in, s4b_check_out* out);

/* extension (R: the individual conditional expectation curves of pdbart's rows — ICE — and their summaries, formed on the device): PER-ROW RESPONSE
 * CURVES along one or two BART predictors.  For row i, grid point g (which assigns grid[g + w * n_grid] to predictor vars[w], as partial_dependence's
 * grid does) and pooled draw k
 *     v(i, g, k) = partial_dependence's v: z (link 0) or Phi(z) (link 1), z = bart(row i with x[vars[w]] replaced by the grid point's values; draw k)
 *                  + the linear parts of predict_summary at row i, draw k — THE VARIED PREDICTORS ARE BART PREDICTORS ONLY, the linear parts stay at
 *                  the row's own values,
 *     c(i, g, k) = v(i, g, k) - v(i, a, k)     with anchor = a in [0, n_grid): the curve centred at grid point a; anchor = -1: c = v.
 * The draws are those of `s` and its peers, pooled as predict_quantiles pools them (rows, peers, their coefficient tables, probs and scratch_bytes are
 * its input; rows.n_weights 0; n_probs may be 0).  in = NULL is the query form: num_samples of `s` alone.  Outputs, each NULL where it is not wanted
 * (a call with every output NULL asks for nothing and is refused):
 *   mean[i * n_grid + g], m2[...]             mean and sum of squared deviations of c(i, g, .) over the S pooled draws (two passes; variance m2 / (S - 1))
 *   quantiles[(j * n_test + i) * n_grid + g]  R's type 7 of c(i, g, .), 0 <= n_probs <= 16; required where n_probs > 0
 *   p_max[i * n_grid + g], p_min[...]         the share of the draws in which g is the LOWEST grid index that attains the row's maximum (minimum) of
 *                                             c(i, ., k) over the grid: an integer count divided by S, exact; the shares of a row add up to 1
 *   range_mean[i], range_m2[i], range_quantiles[j * n_test + i]     the same summaries of r(i, k) = max_g c(i, g, k) - min_g c(i, g, k)
 * THE ORDER OF THE ADDITIONS per (row, grid point, draw) is fixed and depends on nothing else — not on n_grid, the other grid points, the chunking,
 * the route or the kind of sampler.  With the trees of draw k ordered as partial_dependence orders them (those without a rule on a varied predictor in
 * ascending index, then the others in ascending index):
 *   anchor = -1, or link 1:  base = the leaf values of the first group added in that order from 0.0 with the row's own bins; f_g = base + the leaf values
 *       of the second group in that order under grid point g; z_g = (f_g, or (f_g + 0.5) * range_k + min_k for a continuous response) + lin, lin =
 *       offset[i] (or 0.0) + the dense and ELL terms in predict_summary's order; v_g = z_g or Phi(z_g) = erfc(-z_g / sqrt 2) / 2; c = v_g - v_a.
 *   anchor >= 0 under link 0:  s_g = the leaf values of the second group alone added in that order from 0.0; c = range_k * (s_g - s_a) (range_k = 1 for a
 *       binary response): predict_contrast's formula.  The first group and the linear parts cancel and are not evaluated.
 * Hence c(i, a, k) is exactly +0.0, two grid points with equal bins give bit-equal curves, and a call with one varied predictor, n_grid = 2 and anchor = 0
 * returns at g = 1 the bits predict_contrast returns for arm 1 = grid point 1, arm 0 = grid point 0 (link 0, no arm-0 linear part).
 * The rows are processed in chunks of C rows whose values (C x n_grid x S doubles) are the only rows-times-draws storage beside the ranges (C x S):
 * C = scratch / (8 S n_grid) rounded down to a multiple of 64, at least 64, at most n_test, scratch = scratch_bytes or the library's own limit (512 MiB: DESIGN.md 5.16), whichever is smaller.  A call
 * whose smallest scratch 8 x 64 x S x n_grid exceeds S4B_CURVES_SCRATCH_MAX is refused: the grid cannot be split, the extremes need all of it.
 * Refused before anything is launched, on every device layer, info left all zero: n_vars outside {1, 2}, a predictor outside [0, p), two equal
 * predictors, n_grid outside [1, 64], a NULL grid or a NaN in it (+-inf allowed), anchor outside [-1, n_grid), n_probs outside [0, 16] or a prob
 * outside [0, 1], n_probs > 0 without quantiles, range_quantiles without probs, rows.n_weights != 0, negative scratch_bytes, and whatever
 * predict_quantiles refuses of the rows and the peers (S <= 16384).  Two calls, both routes, live and stored samplers, any chunking return the same
 * bits.  Device memory: DESIGN.md 5.16. */
#define S4B_CURVES_SCRATCH_MAX ((int64_t)1 << 30)   /* 1 GiB: the smallest value scratch of one s4b_predict_curves call at most */
typedef struct {
  s4b_summary_in rows;            /* n_weights 0 */
  int32_t n_vars, vars[2], n_grid;   /* as s4b_pd_in */
  const double* grid;             /* n_grid x n_vars, column-major */
  int32_t anchor;                 /* -1, or the grid index the curves are centred at */
  int32_t n_probs;                /* 0 .. 16 */
  const double* probs;
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  int64_t scratch_bytes;
} s4b_curves_in;
typedef struct {
  double* mean; double* m2;       /* n_test x n_grid each, row-major; independently NULL */
  double* quantiles;              /* n_probs x n_test x n_grid; NULL when n_probs = 0 */
  double* p_max; double* p_min;   /* n_test x n_grid each; independently NULL */
  double* range_mean; double* range_m2;   /* n_test each; independently NULL */
  double* range_quantiles;        /* n_probs x n_test, prob-major; or NULL */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did: [0] route of the value kernel (1 LDS-staged, 2 global; 0: no tree was walked — link 0, an anchor and no affected tree),
   * [1] rows per chunk C, [2] chunks, [3] (rows sorted side by side per workgroup) << 32 | draws padded to a power of two, [4] nodes of the largest
   * pooled draw, [5] kernel launches, [6] bytes of device memory the call allocated, [7] the trees with a rule on a varied predictor: (the most in one
   * draw) << 32 | (their sum over the pooled draws) */
  int64_t info[8];
} s4b_curves_out;
int S4B_FN(predict_curves)(s4b_sampler* s, const s4b_curves_in* in, s4b_curves_out* out);

/* extension (R: bayestestR::describe_posterior / HDInterval::hdi applied to every row of extract(fit) or of samples.icate, formed on the device): the
 * PER-ROW DESCRIPTION of the posterior — the highest-density interval, the draws above and below thresholds (from which the probability of direction,
 * the probability of exceeding a cost and the ROPE share follow), the median and the median absolute deviation.  Every output is a function of ONE
 * thing, the row's draws in sorted order.  For row i let x(0) <= ... <= x(S-1) be its S pooled values in ascending order: x = v(z_1) (n_arms 1:
 * predict_quantiles' value) or v(z_1) - v(z_0) (n_arms 2: predict_contrast's d), over the draws of `s` and its peers pooled as predict_quantiles pools
 * them.  The order is that of the usual monotone map of a double's bits to an unsigned integer: -0.0 stands before +0.0.  The values are finite.
 *   quantiles[q, i]     R's type 7 as predict_quantiles forms it, prob-major: the bits are predict_quantiles' (n_arms 1) / predict_contrast's (n_arms 2)
 *   median[i]           type 7 at 0.5: x((S-1)/2) for odd S, x(S/2-1) + 0.5 (x(S/2) - x(S/2-1)) for even S; the bits of quantiles at prob 0.5
 *   hdi[c, 0 / 1, i], hdi_start[c, i]
 *                       the host hands down an integer hdi_count[c] = m, 1 <= m <= S.  Among the windows j = 0 .. S - m the width is x(j + m - 1) - x(j),
 *                       one double subtraction; the smallest width wins, on an exact tie the LOWEST j.  hdi = x(j), x(j + m - 1) at
 *                       hdi[(2 c + e) * n_test + i], hdi_start = j at hdi_start[c * n_test + i].  This is the shortest interval that holds at least m
 *                       of the draws.  It is restated here from that definition; it is NOT pinned against HDInterval::hdi or bayestestR::hdi (no R in
 *                       the test environment), which differ from it and from each other by one point of the window, only against the numpy model of
 *                       tests/describe_cases.py.  The caller chooses m for a mass (the Python binding: ceil(mass S) in exact rational arithmetic).
 *   n_above[t, i], n_below[t, i]
 *                       #{k : x(k) > thresholds[t]} and #{k : x(k) < thresholds[t]}, both strict, both in DOUBLE comparison: -0.0 and +0.0 are equal to
 *                       a threshold of either zero; a draw equal to the threshold counts on neither side.  +-inf allowed, NaN refused.  At [t * n_test + i].
 *   mad[i]              the type-7 median of |x(k) - median[i]| over the S draws, unscaled (R's mad() multiplies by 1.4826)
 * Every output may be NULL.  n_hdi <= S4B_DESCRIBE_HDI_MAX, n_thresholds <= S4B_DESCRIBE_THRESHOLDS_MAX, n_probs <= 16, S <= 16384.  The sorted row
 * alone determines every output: the result does not depend on the chunking, the route, live versus stored samplers, the rows sorted side by side per
 * workgroup or the order of the peers, hdi_start included.  `arms` is predict_contrast's input with n_weights 0 (there are no row weights: every output
 * is per row); with n_arms 1 every arm-0 pointer must be NULL.  Refused before anything is launched, info left all zero: n_hdi, n_thresholds or
 * n_probs outside their range, a hdi_count outside [1, S], a NaN threshold, n_arms outside {1, 2}, an arm-0 pointer with n_arms 1, n_weights != 0,
 * an output whose count is 0 (quantiles with n_probs 0, hdi or hdi_start with n_hdi 0, n_above or n_below with n_thresholds 0), and whatever
 * predict_contrast refuses.  The query forms: in = NULL sets num_samples to the kept draws of `s` alone; in given and EVERY output NULL runs all the
 * checks, sets num_samples to the pooled draws and info to the plan of the call (launches and device bytes 0), and launches nothing.  Per chunk of rows
 * (C as predict_quantiles chooses it) two launches; device memory: DESIGN.md 5.17 (no term grows with n_test x S beyond a chunk). */
#define S4B_DESCRIBE_HDI_MAX 8
#define S4B_DESCRIBE_THRESHOLDS_MAX 32
typedef struct {
  s4b_contrast_in arms;           /* rows (n_weights 0), arm 0, probs, peers, scratch_bytes: predict_contrast's meaning */
  int32_t n_arms;                 /* 1: x = v(z_1), every arm-0 pointer NULL; 2: the contrast */
  int32_t n_hdi;                  /* 0 .. S4B_DESCRIBE_HDI_MAX */
  const int32_t* hdi_count;       /* [n_hdi], each in [1, S] */
  int32_t n_thresholds;           /* 0 .. S4B_DESCRIBE_THRESHOLDS_MAX */
  const double* thresholds;       /* [n_thresholds], any order, duplicates allowed, no NaN */
} s4b_describe_in;
typedef struct {
  double* quantiles;              /* n_probs x n_test, prob-major */
  double* median;                 /* n_test */
  double* hdi;                    /* n_hdi x 2 x n_test */
  int32_t* hdi_start;             /* n_hdi x n_test */
  int32_t* n_above; int32_t* n_below;   /* n_thresholds x n_test each */
  double* mad;                    /* n_test */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did, in s4b_groups_out.info's layout where the entries have a meaning: [0] route of the value kernel (as s4b_contrast_out.info[0]),
   * [1] rows per chunk, [2] chunks, [3] kernel launches (2 per chunk; 0 for the query), [4] bytes of device memory the call allocated (0 for the query),
   * [5] pooled draws, [6] (rows sorted side by side per workgroup) << 32 | draws padded to a power of two, [7] bytes of LDS of a sort workgroup */
  int64_t info[8];
} s4b_describe_out;
int S4B_FN(predict_describe)(s4b_sampler* s, const s4b_describe_in* in, s4b_describe_out* out);

/* extension (R: apply(samples.icate, 2, quantile) and the classification analysis of the sorted effects of Chernozhukov, Fernandez-Val and Luo, formed
 * on the device): ORDER STATISTICS ACROSS THE ROWS within every pooled draw — the distribution of the individual values over the units, with a
 * posterior band — and for every row how often it lies beyond a per-draw order statistic (membership of the most and least affected group).
 * Rows i < n = n_test; pooled draws k < S, over the draws of `s` and its peers pooled as predict_quantiles pools them, S <= 16384.
 * x(i,k) = v(z_1) (n_arms 1: predict_quantiles' value, k_predict_values' v) or v(z_1) - v(z_0) (n_arms 2: predict_contrast's d).  The values are
 * finite.  There are no row weights: n_weights must be 0.  For draw k let y_k(0) <= ... <= y_k(n-1) be the column x(., k) in the order of the usual
 * monotone map of a double's bits to an unsigned 64-bit integer, under which -0.0 stands before +0.0.
 *   sorted[j, k]        for row_probs[j], j < n_row_probs <= S4B_SORTED_PROBS_MAX, each in [0, 1]: R's type 7 ACROSS THE ROWS.  h = p (n - 1),
 *                       lo = floor(h), hi = min(lo + 1, n - 1), g = h - lo, formed on the host in double exactly as predict_quantiles forms them over
 *                       the draws; y(lo) when g = 0, else y(lo) + g (y(hi) - y(lo)) (the product and the sum may contract to one fused multiply-add).
 *   cut[c, k]           for cut_rank[c], c < n_cuts <= S4B_SORTED_CUTS_MAX, integers in [0, n - 1] in any order, duplicates allowed:
 *                       y_k(cut_rank[c]), the order statistic itself, bit for bit.
 *   D                   the matrix [(n_row_probs + n_cuts) x S], statistic-major: the sorted rows, then the cut rows.  Returned as `draws`;
 *                       mean[m], m2[m] (the sum of squared deviations) and quantiles[q, m] at [q * (n_row_probs + n_cuts) + m] for arms.probs are
 *                       formed over the draws as predict_spread forms them over its matrix.
 *   n_above[c, i], n_below[c, i]
 *                       #{k : x(i,k) > cut[c,k]} and #{k : x(i,k) < cut[c,k]}, int32 at [c * n_test + i], both strict, both in DOUBLE comparison: a
 *                       value equal to the cut, or a zero of either sign against a zero cut, counts on neither side.
 * Every output may be NULL.  The result depends on nothing but the multisets of the columns: two calls, both routes, live and stored samplers and any
 * scratch_bytes (which only sets how many draws are held at once) return the same bits.  Another order of the peers permutes the columns of D and
 * changes nothing else: n_above, n_below and quantiles are the same bits, mean and m2 add the same numbers in another order.  `arms` is predict_contrast's input;
 * with n_arms 1 every arm-0 pointer must be NULL.  arms.scratch_bytes limits the values held at once, 8 n_test x (draws of a block): a block is a
 * multiple of 8 draws, at least 8 (64 n_test bytes where the limit is below that), at most 1024, by default what 64 MiB hold.
 * Refused before anything is launched, info left all zero: n_row_probs or n_cuts outside their range, a row prob outside [0, 1] or NaN, a cut_rank
 * outside [0, n_test - 1], n_arms outside {1, 2}, an arm-0 pointer with n_arms 1, n_weights != 0, n_test >= 2^31, an output whose count is 0 (mean,
 * m2 or draws with n_row_probs + n_cuts = 0, quantiles with that or with n_probs = 0, n_above or n_below with n_cuts = 0), and whatever
 * predict_contrast refuses.  The query forms: in = NULL sets num_samples to the kept draws of `s` alone; in given and EVERY output NULL runs all the
 * checks, sets num_samples to the pooled draws and info to the plan of the call (launches and device bytes 0), and launches nothing.  Per block of
 * draws the value kernel once, 16 launches of the selection and one of the counts (where there are cuts and an output for them); then one launch for D
 * and the summary's.  Device memory: DESIGN.md 5.18 (8 n_test x draws of a block, and at most 32 MiB of counting tables). */
#define S4B_SORTED_PROBS_MAX 12
#define S4B_SORTED_CUTS_MAX 8
typedef struct {
  s4b_contrast_in arms;           /* rows (n_weights 0), arm 0, probs (over the draws), peers, scratch_bytes: predict_contrast's meaning */
  int32_t n_arms;                 /* 1: x = v(z_1), every arm-0 pointer NULL; 2: the contrast */
  int32_t n_row_probs;            /* 0 .. S4B_SORTED_PROBS_MAX */
  const double* row_probs;        /* [n_row_probs], each in [0, 1]: across the rows */
  int32_t n_cuts;                 /* 0 .. S4B_SORTED_CUTS_MAX */
  const int32_t* cut_rank;        /* [n_cuts], each in [0, n_test - 1] */
} s4b_sorted_in;
typedef struct {
  double* mean; double* m2;       /* n_row_probs + n_cuts each */
  double* quantiles;              /* n_probs x (n_row_probs + n_cuts), prob-major */
  double* draws;                  /* D: (n_row_probs + n_cuts) x num_samples, statistic-major */
  int32_t* n_above; int32_t* n_below;   /* n_cuts x n_test each */
  int64_t num_samples;            /* pooled draws S */
  /* what the call did, in s4b_spread_out.info's layout where the entries have a meaning: [0] route of the value kernel (as s4b_contrast_out.info[0]),
   * [1] draws per block, [2] blocks, [3] kernel launches (0 for the query), [4] bytes of device memory the call allocated (0 for the query),
   * [5] pooled draws, [6] targets: the distinct ranks selected per draw, [7] selection passes per block (8) */
  int64_t info[8];
} s4b_sorted_out;
int S4B_FN(predict_sorted)(s4b_sampler* s, const s4b_sorted_in* in, s4b_sorted_out* out);

/* extension (R: loo::loo() on the rows-times-draws log-likelihood matrix, formed on the device): PSIS-LOO, Pareto-smoothed importance-sampling
 * leave-one-out, per row over the draws of `s` and its peers, pooled as predict_quantiles pools them (the draws of `s`, then the peers' in their order,
 * S in all, S <= 16384).  It follows loo's do_psis_i / psis_smooth_tail / gpdfit (Vehtari, Simpson, Gelman, Yao, Gabry; the fit: Zhang & Stephens
 * 2009), restated here from the published algorithm; it is NOT pinned against the R package (no R in the test environment), only against the numpy
 * model of tests/loo_cases.py.  l(i,k) is exactly predict_ppd's log-likelihood of y_i under pooled draw k, link 0 or 1: the same
 * sd = sigma[k] row_scale[i], the same log Phi at the signed argument.  lr_k = -l(i,k) is the log importance ratio; lr(0) <= ... <= lr(S-1) the
 * sorted row, mx = lr(S-1), lw(j) = lr(j) - mx.
 *   1  tail length M = tail_len; tail_len = 0: min(ceil(S / 5), ceil(3 sqrt S)) — loo's ceiling(min(0.2 S, 3 sqrt(S / r_eff))) at r_eff = 1 —,
 *      ceil(3 sqrt S) being the smallest m with m m >= 9 S, formed in integers on the host.  A given tail_len must lie in [5, min(S - 1, 1024)].
 *   2  no smoothing where M < 5 (every pool below 21 draws under the default) or lw(S-1) - lw(S-M) < 2^-52 / 100: khat = +inf, raw weights (loo's choice).
 *   3  else the generalised-Pareto fit: ec = exp(lw(S-M-1)); x_j = exp(lw(S-M+j)) - ec, j = 0 .. M-1 ascending; N = M; G = 30 + floor(sqrt N);
 *      xs = x[floor(N / 4 + 0.5) - 1]; theta_g = 1 / x_{N-1} + (1 - sqrt(G / (g - 0.5))) / (3 xs), g = 1 .. G; kappa_g = mean_j log1p(-theta_g x_j);
 *      L_g = N (log(-theta_g / kappa_g) - kappa_g - 1); w_g = exp(L_g - max L) / sum exp(L - max L); theta^ = sum theta_g w_g;
 *      k0 = mean_j log1p(-theta^ x_j); sigma = -k0 / theta^; khat = k0 N / (N + 10) + 5 / (N + 10).  khat or sigma not finite: khat = +inf, no
 *      smoothing.  Else, p_j = (j + 0.5) / N:  lw'(S-M+j) = min(0, log(sigma expm1(-khat log1p(-p_j)) / khat + ec)).
 *   4  outputs per row, lw' the smoothed weights on the tail and lw elsewhere; n_test doubles each, each may be NULL, at least one is wanted:
 *        elpd_loo[i]   log sum_j exp(lw'(j) - lr(j)) - log sum_j exp(lw'(j)), both log-sum-exps with the maximum taken out
 *        pareto_k[i]   khat
 *        lpd[i]        log sum_j exp(-lr(j)) - log S: predict_ppd's lpd, summed here in SORTED order — it agrees within its bound, not bit for bit
 *        ess[i]        (sum_j e^{lw'(j)})^2 / sum_j e^{2 lw'(j)}
 * The smoothed weight belongs to the RANK of its draw, and outside the tail lw + l = -mx whichever draw it is: the sorted row alone determines every
 * output, ties included.  `rows`, y (required), sigma, row_scale, the peers with peer_sigma, scratch_bytes, the chunking and the query
 * form (all outputs NULL or in = NULL: num_samples of `s` alone) are predict_ppd's; there is no noise key and there are no probs.  Everything is
 * checked before anything is launched; a refused call leaves info all zero.  Two calls return the same bits, on both routes, with live or stored
 * samplers, under any chunking.  Device memory: DESIGN.md 5.10. */
typedef struct {
  s4b_summary_in rows;            /* n_weights 0; link: the response, 0 continuous, 1 binary */
  const double* y;                /* n_test responses */
  const double* sigma;            /* one per draw of `s` (link 0) */
  const double* row_scale;        /* n_test, or NULL: 1 */
  int32_t tail_len;               /* 0: the default; else 5 .. min(S - 1, 1024) */
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  const double* const* peer_sigma;        /* [n_peers] vectors (one value per draw of that peer), link 0 */
  int64_t scratch_bytes;
} s4b_loo_in;
typedef struct {
  double* elpd_loo;               /* n_test each, or NULL */
  double* pareto_k;
  double* lpd;
  double* ess;
  int64_t num_samples;            /* pooled draws S */
  int32_t tail_len;               /* the M the call used (0 after a query or a refusal) */
  /* what the call did, s4b_quantile_out.info's layout: [0] route of the value kernel (1 LDS-staged, 2 global; 0: nothing was launched), [1] rows per
   * chunk C, [2] chunks, [3] (rows per workgroup of k_loo_rows) << 32 | draws padded to a power of two, [4] nodes of the largest pooled draw,
   * [5] kernel launches (2 per chunk), [6] bytes of device memory the call allocated, [7] pooled draws */
  int64_t info[8];
} s4b_loo_out;
int S4B_FN(predict_loo)(s4b_sampler* s, const s4b_loo_in* in, s4b_loo_out* out);

/* extension (R: Rhat and n_eff of rstan's summary, for every row instead of the handful of Stan parameters): split R-hat and the effective sample
 * size per row, with the chains KEPT APART.  The estimators are Stan's compute_potential_scale_reduction / compute_effective_sample_size (Gelman et
 * al., BDA3 11.4 - 11.5; Geyer 1992), restated here; tests/conv_cases.py holds the numpy model they are tested against.
 *   chains    every pooled sampler is one chain: `s`, then the peers in their order, each OCCURRENCE of a handle a chain of its own, n_c draws each.
 *             N0 = min n_c; every chain keeps its FIRST N0 draws.  split = 0: C chains of N = N0 draws.  split = 1 (what the Python layer asks for):
 *             h = floor(N0 / 2), chain c gives chains 2c (its draws 0 .. h-1) and 2c+1 (its draws N0-h .. N0-1; the middle draw of an odd N0 belongs
 *             to neither): C chains of N = h draws.  D = C N draws are used.  C <= 256 and at most 16384 pooled draws, else the call is refused.
 *   series    quantity 0: x(i,k) = predict_summary's v(i,k), link 0 or 1.  quantity 1: x(i,k) = exp(l(i,k) - max_k l(i,k)), l predict_ppd's
 *             log-likelihood of y_i (rows.link: the response; y, sigma, row_scale, peer_sigma under predict_ppd's rules), the maximum over all
 *             pooled draws: the likelihood up to a factor, which no output depends on — the series of loo::relative_eff.
 *   per row   mu_c the chain means, d_c[i] = x - mu_c, q_c = sum_i d_c[i]^2, W = sum_c q_c / (C (N-1)), B' = sum_c (mu_c - mean)^2 / (C-1) (0 for
 *             C = 1), mean = sum_c mu_c / C, var+ = W (N-1) / N + B'.
 *               rhat = sqrt(var+ / W), NaN for C = 1
 *             a_c(t) = sum_{i < N-t} d_c[i] d_c[i+t] / N — divisor N at EVERY lag, Geyer's biased estimator: what the autocovariance of Stan's
 *             analyze/mcmc headers computes —, rho(0) = 1, rho(t) = 1 - (W - sum_c a_c(t) / C) / var+.  Pairs (e_j, o_j) = (rho(2j), rho(2j+1)),
 *             P_j = e_j + o_j.  J = the first j with 2j + 1 >= N - 4 or not P_j > 0.  P'_0 = P_0, P'_j = min(P'_{j-1}, P_j) for 0 < j < J.
 *             e'_J = 1 for J = 0, else e_J where P_J >= 0 and 0 otherwise; r = e_J where e_J > 0 and 0 otherwise (the raw value, J = 0: 1).
 *               tau = -1 + 2 (sum_{j<J} P'_j + e'_J) + r,  ess = min(D / tau, D log10 D)
 *               mean = the mean of the D draws used,  mcse = sd / sqrt(ess), sd^2 = (sum_c q_c + N sum_c (mu_c - mean)^2) / (D - 1)
 *               n_pairs = J
 *             Every output of a row is NaN (n_pairs: -1) where N < 4, where a value used is not finite, or where W = 0 (every chain exactly
 *             constant: Stan tests approximately, this is the exact rule).
 * Outputs: n_test values each, each may be NULL, at least one is wanted.  Pooling, scratch_bytes, the chunking and the query form (all outputs NULL
 * or in = NULL: num_samples of `s` alone) are predict_quantiles'.  Everything is checked before anything is launched; a refused call leaves info all
 * zero.  Two calls return the same bits, on both routes, with live or stored samplers, under any chunking.  DESIGN.md 5.11. */
typedef struct {
  s4b_summary_in rows;            /* n_weights 0; link: quantity 0 the link of v, quantity 1 the response (0 continuous, 1 binary) */
  int32_t quantity;               /* 0: the fitted value; 1: the likelihood of y */
  int32_t split;                  /* 0: the chains as they are; 1: every chain in two halves */
  const double* y;                /* quantity 1: n_test responses; quantity 0: NULL */
  const double* sigma;            /* quantity 1, link 0: one per draw of `s` */
  const double* row_scale;        /* quantity 1: n_test, or NULL: 1 */
  int32_t n_peers;
  s4b_sampler* const* peers;
  const double* const* peer_dense_coef;
  const double* const* peer_ell_coef;
  const double* const* peer_sigma;        /* quantity 1, link 0: [n_peers] vectors (one value per draw of that peer) */
  int64_t scratch_bytes;
} s4b_conv_in;
typedef struct {
  double* rhat;                   /* n_test each, or NULL */
  double* ess;
  double* mean;
  double* mcse;
  int32_t* n_pairs;               /* n_test, or NULL */
  int64_t num_samples;            /* pooled draws S (of which D = n_chains chain_len are used) */
  int32_t n_chains;               /* C (0 after a query or a refusal) */
  int32_t chain_len;              /* N */
  /* what the call did, s4b_quantile_out.info's layout: [0] route of the value kernel (1 LDS-staged, 2 global; 0: nothing was launched), [1] rows per
   * chunk, [2] chunks, [3] (rows per workgroup of k_chain_rows) << 32 | draws padded to a power of two, [4] nodes of the largest pooled draw,
   * [5] kernel launches (2 per chunk), [6] bytes of device memory the call allocated, [7] pooled draws */
  int64_t info[8];
} s4b_conv_out;
int S4B_FN(predict_convergence)(s4b_sampler* s, const s4b_conv_in* in, s4b_conv_out* out);

/* The state of a chain BETWEEN TWO GIBBS ITERATIONS as one relocatable byte string: what the next iteration starts from.  It is
 * the hook of the teacher-forced parity tests (state of one implementation injected into the other before every compared
 * transition) and lets a chain continue in another sampler created from the same data; it is not an archive of a fit: the
 * kept trees of keep_trees (export_bart_state carries those), the draws already returned, the tree-move trace and the
 * counters of get_counters / get_nuts_stats stay with the sampler that produced them.  set_state validates the blob
 * (dimensions, tree shapes, rule ranges, finite values, positive scales) before anything is changed.  No reference routine
 * does this: the reference can only re-run a chain from its seed (R/stan4bart_fit.R:33-60); what the blob holds is the
 * state the reference keeps between two iterations of src/init.cpp:752-917 —
 *   NUTS: current point, step size, dual-averaging scalars (stepsize_adaptation.hpp:10-65), window counters
 *   (windowed_adaptation.hpp:29-110), Welford accumulators and inverse metric (var_adaptation.hpp:17-46), ecuyer1988 state;
 *   BART: trees + leaf values, total fit per observation, offset, response scale, sigma, probit latents, R's generator.
 * Layout (native endianness, every block 8-byte aligned), in this order:
 *   s4b_state_header
 *   double  q[D], inv_metric[D], welford_mean[D], welford_m2[D]
 *   double  nuts[6]     = {stepsize, da_mu, da_counter, da_s_bar, da_x_bar, welford_n}
 *   double  last_row[7] = lp__, accept_stat__, stepsize__, treedepth__, n_leapfrog__, divergent__, energy__ of the last draw
 *   uint32  win[8]      = {num_warmup, init_buffer, term_buffer, base_window, window_counter, next_window, window_size, adapting}
 *   uint32  ecuyer[2]
 *   uint32  r_rng[626]  = {mti, mt[624], 0}
 *   double  scale[4]    = {min, max, range, sigma on the data scale}
 *   double  offset[n], total_fits[n] (sum of the tree fits on the rescaled scale), then latents[n] (probit only: latent
 *           response with the offset removed)
 *   per tree: int32 num_nodes, num_leaves; int32 node[num_nodes][2] in preorder ({var, split} internal, {-1, n_obs} leaf);
 *             double mu[num_leaves] in DFS order
 *   latent mode 1 only: uint64 key, uint64 draw index of the parallel latents (s4b_set_latent_mode)
 * get_state: call with buf = NULL (or cap too small) to learn the size. */
#define S4B_STATE_MAGIC 0x53423453u /* "S4BS" */
typedef struct {
  uint32_t magic, version;   /* S4B_STATE_MAGIC, 1 */
  int64_t n;
  int32_t n_trees, num_unconstrained, is_binary, p;
  int64_t reserved[2];       /* [0]: bit pattern of the current k (a double) when k is modeled, else 0; [1]: latent mode (set_latent_mode) */
} s4b_state_header;
int S4B_FN(get_state)(s4b_sampler* s, void* buf, int64_t cap, int64_t* size);
int S4B_FN(set_state)(s4b_sampler* s, const void* buf, int64_t size);

/* diagnostics used by the parity tests: per-tree-update trace records of 5 int32
 * {type 0 birth 1 death 2 swap 3 change, status 1/0/-1, var, split, num_leaves} */
int S4B_FN(set_trace)(s4b_sampler* s, int32_t enable);
int S4B_FN(get_trace)(s4b_sampler* s, int64_t cap_records, int32_t* out, int64_t* num_records);
/* DFS leaf rank of every training observation in tree t (n int32) */
int S4B_FN(get_leaf_assignment)(s4b_sampler* s, int32_t tree, int32_t* out);
/* Not a reference routine.  Hint that `chains` samplers share this sampler's device (R/stan4bart_fit.R:515-533 runs the chains of
 * one fit in parallel workers; here they can be host threads on one GPU).  Where the persistent sweep applies (set_tree_path) the hint
 * changes nothing since round 5: samplers of one process take turns on the device, launches of other processes are sorted out by the
 * roll call at the start of every persistent launch, and the aggregate rate is higher than on the per-tree kernels.
 * Elsewhere — n > 1.04e6, observation weights together with cgm(split.probs) — the fused launch keeps every CU busy with one register-heavy workgroup,
 * which is fastest for a chain that has the device to itself; with three or more chains per device the sampler switches to the
 * two-kernel tree update, which leaves room for the other chains' kernels (higher aggregate rate).  The
 * same chain either way: identical tree moves and generator stream, floating-point values equal up to the summation order of the
 * per-bin sums (1e-15 relative).  May be called at any time between runs. */
int S4B_FN(set_device_sharing)(s4b_sampler* s, int32_t chains);
/* Not a reference routine.  Which device code runs a tree update: 0 automatic (default), 1 two kernels per tree (k_tree + k_control),
 * 2 one fused launch per tree (k_step), 4 persistent (k_sweep: ONE launch per sweep, the residual in the registers of the pass waves, bin
 * partials exchanged through order-free integer atomics), 5 persistent with a streaming pass (k_sweep_stream: the same launch, the pass
 * waves read and write the residual per tree; measured slower than 1 / 2 at every size and never chosen automatically).  The automatic
 * choice is 4 wherever it applies — at most 16 observations per pass thread (n <= 1 044 480 on 256 compute units); observation weights
 * and cgm(split.probs) have their own instantiations of the launch since round 6 (k_sweep_w, k_sweep_sp), the two together do not —,
 * else 2 up to n ~ 4e6, else 1 (with split.probs always 1).  A request the sampler cannot honour
 * (more than 255 quads per thread for 2, the conditions above for 4 / 5) falls back to the next path down; get_tree_path reports the path
 * in effect.  The same chain on every path (see set_device_sharing).  May be called at any time between runs.
 * get_tree_path: out[0] = the request, out[1] = the path in effect (1, 2, 4 or 5).  (3 was the lagged launch of an earlier revision:
 * removed, the value is rejected.) */
int S4B_FN(set_tree_path)(s4b_sampler* s, int32_t path);
int S4B_FN(get_tree_path)(s4b_sampler* s, int32_t out[2]);
/* counters: {log-density gradient evaluations, tree updates, device kernel launches} */
int S4B_FN(get_counters)(s4b_sampler* s, int64_t out[3]);
/* diagnostics of the one-launch O(N) sums of the Stan block (k_stan_fused): out = {evaluations, evaluations repeated in plain
 * doubles because the fixed-point range check failed (first evaluation, rescaled response, trajectory far outside the typical set)} */
int S4B_FN(get_fused_stats)(s4b_sampler* s, int64_t out[2]);
/* persistent tree path only (zeros otherwise): out = {sweeps run while the persistent path was in effect — the ones a busy device sent to
 * k_step launches (get_sweep_busy and the back-off after it) included —, of which handed over to k_step launches part-way because a
 * tree outgrew the 64 node slots of the wave-register control path} since creation */
int S4B_FN(get_sweep_stats)(s4b_sampler* s, int64_t out[2]);
/* persistent tree path only (zeros otherwise), since creation: out = {persistent launches that ran (roll call passed), tree updates
 * decided inside them, steps whose bin statistics were published BEFORE the verdict of the tree before (speculation), steps
 * of those whose verdict bore the speculation out} */
int S4B_FN(get_sweep_spec)(s4b_sampler* s, int64_t out[4]);
/* persistent tree path only (zero otherwise): persistent launches that found the device shared (not every workgroup of the launch became
 * resident within 200 us: somebody else's kernels held compute units).  Such a launch changes nothing; its sweep ran as k_step launches and
 * so do the next 16, 32, ... sweeps before the persistent launch is tried again.  (The reference's chain fan-out starts one worker process
 * per chain, R/stan4bart_fit.R:498-533: on a box with fewer GPUs than chains those processes share devices.) */
int S4B_FN(get_sweep_busy)(s4b_sampler* s, int64_t* out);
/* extension: how the Stan block evaluates the O(N) part of the log density (stan_control.hmc_mode): 0 = sufficient statistics
 * gathered once per Gibbs iteration, 1 = one device evaluation per leapfrog (the reference's cost model).  A sampler created
 * with mode 0 may be switched to 1 and back between runs (same posterior, same draws up to rounding); one created with mode 1
 * has no Gram matrix and stays in mode 1. */
int S4B_FN(set_hmc_mode)(s4b_sampler* s, int32_t mode);
int S4B_FN(get_hmc_mode)(s4b_sampler* s, int32_t* mode);
/* extension: how the probit latents of a binary response are drawn.  0 = exact (default): dbarts' truncated normals from R's stream, the
 * reference's chain bit for bit.  1 = parallel: every latent drawn independently and exactly from N(mean, 1) truncated by y, one device thread
 * per observation, from Philox4x32-10 under a 64-bit key derived from the generator state and seed given to create (R's stream is not used
 * for it; tree proposals and a modeled k still are).  A different chain with the same stationary distribution, not the reference's chain;
 * it is identical on every tree path, in sweep groups and from run to run.  Set it after create and before the first run (the initial sweep
 * inside create draws its latents exactly); mode 1 is refused for a continuous response and by a device layer without the parallel draw.
 * The state of get_state carries the mode (header reserved[1]) and, in mode 1, 16 more bytes at its end: uint64 key, uint64 draw index;
 * set_state refuses a state of the other mode.  DESIGN.md 5.4b. */
int S4B_FN(set_latent_mode)(s4b_sampler* s, int32_t mode);
int S4B_FN(get_latent_mode)(s4b_sampler* s, int32_t* mode);

/* NUTS totals over all transitions since creation: {transitions, sum of treedepth__, sum of n_leapfrog__, divergent transitions}
 * (the per-draw values are columns 4-6 of the stan result; the totals let a caller that keeps no per-iteration output, keep_fits =
 * FALSE, report mean tree depth and leapfrogs per iteration) */
int S4B_FN(get_nuts_stats)(s4b_sampler* s, double out[4]);

/* extension: run-ahead helpers of the NUTS transition.  The leapfrog states of a transition are a function of its start point, momentum draw,
 * step size and metric alone; a helper thread integrates one direction ahead while the sampler's thread builds the tree and consumes the
 * finished states in the order the doublings ask for them; a state the helper has not finished when it is asked for is computed by the
 * sampler's thread itself, as without a helper.  The chain is the same bit for bit with and without helpers.  n = 0: none; 1: the
 * backward direction; 2: both directions.  (TEST HOOK, not part of the contract and not reachable through the environment: n + 16 makes the
 * sampler's thread wait for a helper's state instead of computing it, so that a test sees every state of a helper's direction come from the helper.)
 * The default is the environment variable S4B_NUTS_HELPERS at create (0 / 1 / 2).  Where that is unset and this function is not called, the count is
 * automatic: one helper, and a second one for the forward direction as long as the CPUs a helper of the sampler's thread can be put on (same
 * last-level cache, another core, allowed to the process) span at least two cores, the CPUs the process may use span at least three cores for
 * every live sampler that may run ahead, and the process's helper budget has room.  Cores, not hardware threads: a single chain with eight cores
 * gets both helpers, a rank bound to two cores keeps one whether or not the cores have two hardware threads each.
 * Helpers exist only for a model whose gradient is closed-form host arithmetic (normal or flat coefficient prior, at most two coefficients per
 * grouping term) in hmc_mode 0; every other sampler integrates inline whatever n says.  A process has at most 8 helper threads in all; a
 * sampler that gets none integrates inline, and so does one whose thread may use no core but its own (a process bound to one core).  On Linux a
 * helper is kept on the cores that share the last-level cache of the sampler's thread (its own affinity only, never the caller's).  A helper is created at the first transition that uses it, sleeps between transitions and is
 * joined by free (or by a smaller n). */
int S4B_FN(set_nuts_helpers)(s4b_sampler* s, int32_t n);
/* {leapfrogs taken from a helper, leapfrogs of a helper's direction that the helper had not finished in time (computed by the sampler's
 * thread itself; in the waiting mode: waited for, and counted as taken too), leapfrogs a helper computed that no tree consumed, transitions
 * that ran without a helper} since creation */
int S4B_FN(get_nuts_runahead)(s4b_sampler* s, int64_t out[4]);
/* extension (process-wide): the host loops of a leapfrog (dense Gram product, leaf and merge loops) in their AVX2 form (on != 0) or their scalar
 * form (0); both give the same bits.  Default: AVX2 where the CPU has it, unless the environment variable S4B_HOST_VECTOR is 0.  *effective
 * (may be NULL) receives what is in force: 0 on a CPU without AVX2 whatever was asked.  on < 0 changes nothing and only reports. */
int S4B_FN(set_host_vector)(int32_t on, int32_t* effective);

/* measurement hook (no reference counterpart): runs `n_sweeps` extra BART sweeps with HIP events recorded on the
 * sampler's own stream around every kernel launch and returns, per kernel class
 * {stats, control, apply}: out[0..2] = average launch duration in microseconds, out[3..5] = launches timed,
 * out[6] = wall microseconds per sweep (events around the whole sweep, no per-launch events), out[7] = n. */
int S4B_FN(profile_sweep)(s4b_sampler* s, int32_t n_sweeps, double out[8]);
/* extension (measurement): plain streaming kernels over n_doubles doubles on `device` — out[0] GB/s of a read-only pass,
 * out[1] GB/s of an in-place read + write pass (the residual's access pattern), out[2..3] their best times in us */
int S4B_FN(stream_probe)(int32_t device, int64_t n_doubles, int32_t reps, double out[4]);

/* extension (measurement): HIP-event timing of the per-leapfrog O(N) sums of the hmc_mode 1 path at the current draw.
 * out[0] us per evaluation (kernels), out[1] us including the result fetch, out[2] launches per evaluation, out[3] N,
 * out[4] algorithmic bytes per evaluation N (8K + 12z + 20) (SURVEY §8d B_lf) */
int S4B_FN(profile_leapfrog)(s4b_sampler* s, int32_t n_evals, double out[8]);

/* TEST HOOK (no reference counterpart; off by default): hook 1, value k > 0 — every k-th persistent launch of this sampler finds the roll call
 * of its launch already decided "device busy" (what a launch sees that shares the device with another process's kernels), so that the busy
 * fallback of the persistent path runs under the parity tests without a second process; value 0 switches it off.  Other hooks are rejected. */
int S4B_FN(set_test_hook)(s4b_sampler* s, int32_t hook, int64_t value);

/* TEST ENTRY (no reference counterpart): ONE draw of the probit latents from the state as it stands, and nothing else of a sweep — the exact
 * draw of the sampler's latent mode, then a wait and the check of the device error word.  Mode 0: dbarts' sequential truncated normals from R's
 * stream (k_latents2 + k_latents_finish on the device).  Mode 1: k_latents_par under the key and draw index of the state's tail; the draw index
 * advances by one, R's stream stays.  With set_state before it (r_rng, offset, total_fits, latents; in mode 1 key and draw index) and get_state
 * after it, a test chooses the 624 state words, mti, fits, offsets and previous latents the draw sees, which run() cannot offer: its tree sweep
 * consumes a data-dependent number of stream positions first.  Refused for a continuous response and on a stored sampler.  Domain of the device
 * draw, mode 0: an observation that needs more than 256 stream positions fails with "internal error" (DESIGN.md 5.4, 7); mode 1: a mean whose
 * square overflows (|mean| above about 1.3e154) fails with "parallel latents: no proposal was accepted" (DESIGN.md 5.4b). */
int S4B_FN(test_draw_latents)(s4b_sampler* s);

/* TEST ENTRY (no reference counterpart): the Stan -> BART hand-off of ONE Gibbs iteration and nothing else — exactly what run() does between
 * the Stan transition and the tree sweep (reference src/init.cpp:762-821), for coefficients the caller chooses: BART's offset from beta (K) and
 * b (q) with the terms of the sampler's own offset type (the same dispatch run() goes through), sigma (a continuous response only; ignored for a
 * binary one) and the rescaling of the response, with a new response scale when update_scale != 0; then the check of the device error word.  No
 * transition, no sweep, no latent draw, no refresh of the Stan block's inputs: Stan's position, its adaptation state and both generators are left
 * alone, so a get_state after the call differs from one before it in the BART block's scale, offset, total fits, leaf values and latents only,
 * and a test can compare exactly those.  The coefficients need not be a draw of the model (they are not stored: get_parametric_mean keeps
 * answering from the last transition).  Refused on a stored sampler, for non-finite coefficients and for a sigma that is not positive. */
int S4B_FN(test_hand_off)(s4b_sampler* s, const double* beta, const double* b, double sigma, int32_t update_scale);

/* TEST ENTRY (no reference counterpart): ONE evaluation of the Stan block's O(N) sums (ss = e'We, X'We, Z'We) from the state as it stands, through the
 * members run() itself uses, and nothing else.  mode -1: the evaluation of one leapfrog of hmc_mode 1 — e = e0 - X beta - Z b with the e0 the last
 * evaluation of the other kind left on the device; beta (K) and b (q) may hold non-finite values (ordinary arithmetic: the evaluation is then
 * rejected by the device's flag and repeated in plain doubles).  mode 0..3: the evaluation of one Gibbs iteration with that Stan-offset mode
 * (0: e = y; 1: y - fit; 2: y - user offset; 3: y - fit - user offset; 2 and 3 are refused without a user offset); beta and b are ignored; e0 is
 * rewritten on the device as run() rewrites it, nothing else of the chain moves.  set_exp: NULL (the power-of-two scales of the fixed-point sums are
 * what the history left them) or three binary exponents in [-900, 900] for |e|^2, X'e, Z'e that replace them before the launch; the memory of
 * consecutive failures is cleared with them, so {0, 0, 0} is what run() and set_state start from.  sums[1 + K + q]: ss, X'e, Z'e as the sampler would
 * have used them (after a rejected fixed-point evaluation: the plain-double values).  info[S4B_STAN_SUMS_INFO]: [0] 1 = the fixed-point result was
 * accepted; [1] why not, a sum of 1 = the device's flag (something non-finite or of 2^42 and more after scaling), 2 = a magnitude word of 2^32 and
 * more, 4 = an exponent word below 4 (resolution); [2..4] the exponents of this launch; [5..7] the exponents after it; [8..10] the magnitude words;
 * [11..13] the exponent words as the device wrote them (0: nothing but zeros went in, else 4000 + the binary exponent of the largest workgroup
 * magnitude); [14] workgroups of the launch; [15] 1 = this shape has the fixed-point path at all; [16], [17] the counters of s4b_get_fused_stats.
 * A shape without that path (K > 16 or q > 4096) and the emulated device layer evaluate in plain doubles: info is all 0.  Refused on a stored sampler. */
#define S4B_STAN_SUMS_INFO 18
int S4B_FN(test_stan_sums)(s4b_sampler* s, int32_t mode, const double* beta, const double* b, const int32_t* set_exp, double* sums, int64_t* info);

/* TEST ENTRY (no reference counterpart): the selection and the count kernels of s4b_predict_sorted ALONE, on a caller's matrix values [n x S] row-major
 * (values[i * S + k], finite), in blocks of block_draws columns read in place — no tree is walked, the sampler only lends its device and stream (a
 * stored sampler will do).  order_stats[r * S + k] = the ranks[r]-th smallest of column k in the key order (-0.0 before +0.0), bit for bit, for
 * n_ranks ranks in [0, n - 1] in any order, duplicates allowed; n_above / n_below [c * n + i] count the columns in which values[i, k] lies strictly
 * above / below the cut_rank[c]-th smallest of column k, in double comparison, for n_cuts <= S4B_SORTED_CUTS_MAX cuts.  Any output may be NULL.
 * Refused: n < 1 or >= 2^31, S outside [1, 16384], block_draws < 1, min(block_draws, S) > 1024, n_ranks outside [0, 32], n_cuts outside
 * [0, S4B_SORTED_CUTS_MAX], neither ranks nor cuts, more than 32 DISTINCT ranks among ranks and cut_rank together, a rank outside [0, n - 1], NULL
 * values or info.  info[8]: [0] draws per counting workgroup, [1] draws per block, [2] blocks, [3] launches (17 per block with counts, 16 without, and
 * one for order_stats), [4] device bytes, [5] S, [6] distinct ranks, [7] passes (8).  The emulated device layer refuses the call. */
int S4B_FN(test_sorted_select)(s4b_sampler* s, const double* values, int64_t n, int64_t S, int64_t block_draws, int32_t n_ranks, const int32_t* ranks,
                               double* order_stats, int32_t n_cuts, const int32_t* cut_rank, int32_t* n_above, int32_t* n_below, int64_t* info);

/* finalizer of the externalptr — src/init.cpp:1152-1165 */
void S4B_FN(free)(s4b_sampler* s);

/* extension (no reference counterpart): SWEEP GROUP — samplers on one device whose tree sweeps are launched together, one workgroup per
 * member, while each runs in the solo regime of the persistent path (n <= 4 096).  Samplers driven from different host threads join one
 * group; a member's sweep then waits (bounded: s4b_sweep_group_set_timeout, default 30 s) for the other members that are inside run()
 * at the moment and one of them launches all the sweeps at once.  Draws are identical to the ungrouped run.  A member whose sweep
 * is not in the solo regime (more observations, another tree path) launches on its own as before and is never waited for.
 * stats: {batched launches, member sweeps inside them, member sweeps launched on their own, launches that left a straggler behind}. */
typedef struct s4b_sweep_group s4b_sweep_group;
int S4B_FN(sweep_group_create)(int32_t device, int32_t max_members, s4b_sweep_group** out);
int S4B_FN(sweep_group_join)(s4b_sweep_group* g, s4b_sampler* s);     /* refused: a sampler on another device, one already in a group, a full group */
int S4B_FN(sweep_group_leave)(s4b_sampler* s);                        /* no-op for a sampler in no group */
int S4B_FN(sweep_group_stats)(s4b_sweep_group* g, int64_t out[4]);
int S4B_FN(sweep_group_set_timeout)(s4b_sweep_group* g, double seconds);
int S4B_FN(sweep_group_free)(s4b_sweep_group* g);                     /* refused while samplers are joined */

#ifdef __cplusplus
}
#endif
#endif /* STAN4BART_AMD_H */
