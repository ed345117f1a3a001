/*
 * blhip.h -- C-ABI of libblhip.so: the MI355X (gfx950) implementation of bayesloop's grid-based
 * forward-backward inference loop.
 *
 * The reference (christophmark/bayesloop v1.5.7) is pure Python and has NO FFI for this path; its boundary is the
 * duck-typed method level.  Each entry point below names the reference interface it stands in for
 * (file:line relative to the reference checkout):
 *
 *   blhip_fit            Study.fit                        bayesloop/core.py:330-486
 *                        (+ the per-hyper-point loop of   bayesloop/core.py:1349-1366 / 1473-1489 when n_chains > 1)
 *   blhip_set_series     the user's loop `for d in series: S.loadData(d); S.fit()` around Study.fit   bayesloop/core.py:330-486
 *   blhip_accum_*        the evidence-weighted average    bayesloop/core.py:1295, 1362-1366, 1339, 1375-1382, 1416-1419
 *   blhip_posterior_*    the posteriorSequence attribute  bayesloop/core.py:356, 408, 436-441
 *   blhip_posterior_query / _bins   Parser.__call__ over a loop of time stamps   bayesloop/parser.py:256-440 (probabilities; :399-418 distributions)
 *   blhip_carry_*        OnlineStudy.step                bayesloop/core.py:2062-2226 (with BLHIP_RESUME / BLHIP_CARRY fits)
 *   blhip_comm_*         HyperStudy.fit(nJobs > 1):       bayesloop/core.py:1307-1340 (pool.map fan-out and the merge of the
 *                        sub-studies), _parallelFit       bayesloop/core.py:1443-1495 -- one process per GPU, RCCL over xGMI
 *
 * inside which the library evaluates
 *   ObservationModel.processedPdf + Poisson/Gaussian/GaussianMean.pdf   observationModels.py:35-56, 502, 566-567, 705-706
 *   Bernoulli / Laplace / WhiteNoise / AR1 / ScaledAR1.pdf               observationModels.py:428-430, 635, 767, 830-831, 893-896
 *   GaussianRandomWalk / CombinedTransitionModel / ChangePoint / Static  transitionModels.py:49-63, 96-118, 289-317, 632-662
 *   RegimeSwitch / Independent / SerialTransitionModel + BreakPoint      transitionModels.py:339-363, 394-415, 756-818
 *   NotEqual / AlphaStable- / BivariateRandomWalk / Deterministic        transitionModels.py:450-474, 158-260, 872-911, 548-606
 *   (scipy.ndimage.gaussian_filter1d, mode='reflect', truncate=4.0, called at transitionModels.py:111;
 *    scipy.signal.fftconvolve / convolve2d at :258, :889; scipy.ndimage.shift(order=3, mode='nearest') at :581, :600).
 *
 * Conventions
 *   - plain C, no C++ / torch types; every array is float64 (double) or the integer type shown, C-contiguous.
 *   - the caller owns every host buffer and keeps it alive for the duration of the call; the library owns all
 *     device memory inside the opaque context.  No callbacks.  Nothing throws across the ABI.
 *   - return value: 0 = ok, < 0 = hard error (message via blhip_last_error).  Numerical failure of a chain (a zero
 *     normaliser, core.py:390-400 / 442-452) is NOT an error: it is reported per chain in abort_step/abort_phase and
 *     the caller mirrors the reference (logEvidence = -inf, early return).
 *   - one context per device; calls on one context must be serialised by the caller.
 */
#ifndef BLHIP_H
#define BLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLHIP_ABI_VERSION 15

typedef struct blhip_ctx blhip_ctx;

/* observation models (likelihood evaluated on the device from the data point and the grid) */
enum {
    BLHIP_OM_POISSON       = 1,   /* observationModels.py:502      1 parameter  (rate)            */
    BLHIP_OM_GAUSSIAN      = 2,   /* observationModels.py:566-567  2 parameters (mean, std)       */
    BLHIP_OM_GAUSSIAN_MEAN = 3,   /* observationModels.py:705-706  1 parameter  (mean); data (T,1,2) = (value, std) */
    /* closed-form models whose likelihood table (T,G) is built ON THE DEVICE from the data (no host pdf, no upload): */
    BLHIP_OM_BERNOULLI     = 4,   /* observationModels.py:419-439  1 parameter  (p)                               */
    BLHIP_OM_LAPLACE       = 5,   /* observationModels.py:624-635  2 parameters (mean, scale)                     */
    BLHIP_OM_WHITE_NOISE   = 6,   /* observationModels.py:756-767  1 parameter  (sigma)                           */
    BLHIP_OM_AR1           = 7,   /* observationModels.py:819-831  2 parameters (rho, sigma); seg_len 2           */
    BLHIP_OM_SCALED_AR1    = 8,   /* observationModels.py:881-896  2 parameters (rho, sigma); seg_len 2           */
    /* (ABI v9) the density as a postfix program the caller compiled from an expression (bl.om.SymPy, bl.om.SciPy): the (T,G) table is
     * built ON THE DEVICE by one interpreter kernel from the program armed with blhip_set_lik_program; lik stays NULL, seg_len is 1.
     * Grids of 1 .. BLHIP_MAX_DIM parameters. */
    BLHIP_OM_PROGRAM       = 9,   /* observationModels.py:35-56 over a density written as a program                */
    BLHIP_OM_TABLE         = 100  /* likelihood evaluated by the caller (any ObservationModel.pdf): lik (T,G) */
};

/* transition-model ops, applied in list order in both directions (transitionModels.py:645-649, 656-660) */
enum {
    BLHIP_OP_STATIC       = 0,    /* transitionModels.py:49-63    no hyper-parameter                           */
    BLHIP_OP_GRW          = 1,    /* transitionModels.py:96-118   value = sigma, axis = target parameter index  */
    BLHIP_OP_CHANGEPOINT  = 2,    /* transitionModels.py:289-317  value = tChange (flags bit 0: see below)      */
    BLHIP_OP_REGIMESWITCH = 3,    /* transitionModels.py:394-415  value = log10 pMin: clamp from below, renormalise */
    BLHIP_OP_INDEPENDENT  = 4,    /* transitionModels.py:339-363  restart from the normalised prior at every step */
    BLHIP_OP_BREAKPOINT   = 5,    /* transitionModels.py:821-840  value = tBreak: boundary between two sub-models of a
                                     SerialTransitionModel (transitionModels.py:756-786) */
    BLHIP_OP_NOTEQUAL     = 6,    /* transitionModels.py:450-474  value = log10 pMin: max(p) - p, renormalise, clamp from
                                     below, renormalise */
    BLHIP_OP_BIVARIATE    = 7,    /* transitionModels.py:872-911  value = sigma1; MUST be followed by two BIVARIATE_ARG ops
                                     carrying sigma2 and rho: dense 2-D convolution with the bivariate normal kernel on
                                     |x| <= 3 ceil(sigma / lattice), zero boundary, renormalised (2-D grids only) */
    BLHIP_OP_BIVARIATE_ARG = 8,   /* value = sigma2 (first) / rho (second) of the BIVARIATE op before it */
    BLHIP_OP_ALPHASTABLE  = 9,    /* transitionModels.py:158-260  value = scale c, axis = target parameter; MUST be followed
                                     by one ALPHASTABLE_ARG op carrying alpha: convolution along the axis with the symmetric
                                     alpha-stable density (inverse FFT of exp(-|c w|^alpha)), zero boundary, renormalised */
    BLHIP_OP_ALPHASTABLE_ARG = 10,/* value = alpha of the ALPHASTABLE op before it */
    BLHIP_OP_DETERMINISTIC = 11,  /* transitionModels.py:548-606  axis = target parameter; no value of its own; MUST be
                                     followed by 2 T DETERMINISTIC_ARG ops whose values are the shifts (in parameter units)
                                     the caller evaluated from the model's function: first T: f(t'+1) - f(t') of the
                                     transition INTO forward step i (t' = time stamp of step i-1; entry 0 is used with
                                     BLHIP_RESUME only), next T: f(t'-1) - f(t') of the backward transition into step i
                                     (t' = time stamp of step i+1; entry T-1 unused).  Cubic-spline shift as
                                     scipy.ndimage.shift(order=3, mode='nearest'), renormalised.  Shifts beyond 12 grid cells
                                     per step: 1-D grids of up to 16000 points, 2-D grids along axes of up to 16384 points */
    BLHIP_OP_DETERMINISTIC_ARG = 12
};

/* A SerialTransitionModel (transitionModels.py:665-818) is flattened into the same program: the ops of its n sub-models
 * carry segment = 0..n-1, its n-1 boundaries are BREAKPOINT ops or CHANGEPOINT ops with flags bit 0 set (in list order).
 * At time stamp t the active segment is the number of boundary values <= t (:768); ops with segment >= 0 act only
 * while their segment is active; a boundary change-point additionally restarts from the prior at t == value (:801-813). */
typedef struct {
    int32_t kind;                 /* BLHIP_OP_* */
    int32_t axis;                 /* GRW: index of the target parameter (0 .. ndim-1) */
    int32_t segment;              /* -1: always active; >= 0: sub-model index of the serial model */
    int32_t flags;                /* CHANGEPOINT: bit 0 = boundary of the serial model */
} blhip_op;

#define BLHIP_MAX_DIM 4

/* The fit problem: grid, data, prior, transition program (shared by all chains of a call). */
typedef struct {
    int32_t        ndim;          /* number of observation-model parameters = grid dimensions (core.py:130-176 builds a
                                     meshgrid over any number): 1 .. BLHIP_MAX_DIM.  3 and more: BLHIP_OM_TABLE / BLHIP_OM_PROGRAM
                                     models (the reference's SciPy / SymPy / NumPy plug-ins) with every op but REGIMESWITCH /
                                     ALPHASTABLE / BIVARIATE; DETERMINISTIC shifts of at most 12 grid cells per step */
    int32_t        obs_model;     /* BLHIP_OM_*                                                                  */
    int64_t        n[BLHIP_MAX_DIM];          /* grid size per parameter (core.py:157)                           */
    const double  *marginal[BLHIP_MAX_DIM];   /* marginal grid values per parameter, n[k] doubles (core.py:156)  */
    double         lattice[BLHIP_MAX_DIM];    /* lattice constants (core.py:161-166)                             */
    int64_t        T;             /* number of formatted time steps                                              */
    int32_t        seg_len;       /* segment length of the observation model (1 for the device-side models)      */
    int32_t        data_dim;      /* trailing data dimension d (1 for scalar series); GAUSSIAN_MEAN: 2           */
    const double  *data;          /* formatted data (T, seg_len, data_dim), NaN = missing (observationModels.py:53) */
    const double  *timestamps;    /* formatted timestamps (T,) (core.py:350)                                     */
    const double  *prior;         /* alpha_0: Study._computePrior() on the grid, (G,) (core.py:363)              */
    const double  *reset_prior;   /* what a change-point resets to, (G,) (transitionModels.py:300-312); NULL if no CHANGEPOINT op */
    const double  *indep_prior;   /* what INDEPENDENT restarts from, (G,) (transitionModels.py:351-360); NULL if no such op */
    const double  *lik;           /* BLHIP_OM_TABLE only: likelihood (T, G) evaluated by the caller; else NULL   */
    int32_t        n_ops;         /* length of the transition program                                            */
    const blhip_op *ops;
    /* streaming use (OnlineStudy.step, core.py:2062-2226): see BLHIP_RESUME / BLHIP_CARRY */
    double         resume_time;   /* BLHIP_RESUME: the time stamp the transition into step 0 is evaluated at
                                     (OnlineStudy passes len(formattedData) - 1 = -1, core.py:2164-2165)         */
    int32_t        carry_slot;    /* which carried state (one per transition model of an OnlineStudy), >= 0      */
    int32_t        reserved0;
    /* (ABI v7) the backward message entering the LAST time step, (G,); NULL: uniform 1 / G (core.py:424-425).  Lets a caller that
     * applies the transition model ITSELF -- the reference's plug-in boundary TransitionModel.computeBackwardPrior(posterior, t),
     * transitionModels.py:49-63, for models the library has no op for -- run the backward recursion one step per call: the
     * likelihood products, normalisations, sums and means of core.py:434-470 stay on the device (bayesloop_amd/core.py:
     * Study._fitHostTransition).  Fits with a backward_init take the launch-per-step kernels. */
    const double  *backward_init;
    /* (ABI v8) 0, or the caller's name for the CONTENT of `prior`: a caller that passes the same non-zero token again promises that the
     * array holds the same values as when it last passed that token.  The library then skips the upload when the context still holds
     * that prior (same token, same grid, nothing uploaded over it since) -- the prior of a 2048 x 2048 grid is 32 MiB, 0.6 ms of PCIe per
     * fit of a study that is fitted again and again (Study.optimize, core.py:488-565; repeated fit() calls).  bayesloop_amd passes a
     * token for the read-only prior arrays it caches per study (bayesloop_amd/core.py: _computePrior). */
    uint64_t       prior_token;
} blhip_problem;

/* Flags of blhip_fit */
#define BLHIP_FORWARD_ONLY   1u   /* Study.fit(forwardOnly=True)   core.py:422                                   */
#define BLHIP_EVIDENCE_ONLY  2u   /* Study.fit(evidenceOnly=True)  core.py:355, 407, 422, 477                    */
#define BLHIP_KEEP_POSTERIOR 4u   /* keep each chain's normalised posterior sequence on the device (blhip_posterior_read) */
#define BLHIP_ACCUMULATE     8u   /* fold each finite chain into the context's average-posterior accumulator (blhip_accum_*) */
#define BLHIP_RESUME         16u  /* step 0 consumes T_fwd(carried state of carry_slot, resume_time) of every chain instead of
                                     the prior (core.py:2164-2165); the slot must hold n_chains states of this grid  */
#define BLHIP_CARRY          32u  /* keep every chain's filtered, normalised distribution of the LAST step in carry_slot
                                     (core.py:2173 parameterPosterior[i][j]); forward-only / evidence-only fits      */

/* Per-chain results; every pointer may be NULL. */
typedef struct {
    double  *log_evidence;        /* (n_chains,)          Study.logEvidence (core.py:403, 417); -inf on abort    */
    double  *local_evidence;      /* (n_chains, T)        Study.localEvidence (core.py:404, 463-464)             */
    double  *posterior_mean;      /* (n_chains, ndim, T)  Study.posteriorMeanValues (core.py:480-483)            */
    int64_t *abort_step;          /* (n_chains,)          -1, or the step i at which the normaliser was zero     */
    int32_t *abort_phase;         /* (n_chains,)          0 = forward (core.py:390-400), 1 = backward (442-452)  */
} blhip_result;

/* Timing of the last blhip_fit, measured with HIP events on the library's stream. */
typedef struct {
    double  forward_ms;           /* all forward-step launches                                                   */
    double  backward_ms;          /* all backward-step launches                                                  */
    double  accumulate_ms;        /* hyper-average accumulation launches                                         */
    double  total_ms;             /* whole call on the device timeline                                           */
    int64_t forward_launches;
    int64_t backward_launches;
    int64_t accumulate_launches;
    int64_t cells_per_launch;     /* grid cells x chains processed by one step launch (largest batch)            */
    int64_t batches;              /* number of chain batches the call was split into                             */
    int32_t fwd_kernel_variant;   /* which step kernel ran (library-internal id)                   */
    int32_t bwd_kernel_variant;
    /* what the launches of the call move and compute BY CONSTRUCTION (totals over all batches; the launch-per-step kernels
     * stream the state, the resident kernels keep it in LDS and touch HBM only for what the fit keeps + halo strips): the
     * figures bench.py turns into real HBM GB/s and fp64 TFLOP/s next to the streaming-equivalent rate of SURVEY 8(d) */
    double  fwd_hbm_bytes;        /* HBM bytes of all forward launches                                           */
    double  bwd_hbm_bytes;        /* HBM bytes of all backward launches (incl. a fold fused into them)           */
    double  fwd_flops;            /* fp64 flop of all forward launches, as executed (band products of the matrix-pipe
                                     kernels incl. their structural zeros, FMA = 2)                              */
    double  bwd_flops;
    int32_t resident_fallbacks;   /* batches of this call a resident launch gave up on (repeated launch-per-step) */
    int32_t resident_armed;       /* 1: the context will try the resident paths on its next eligible fit          */
    int32_t resident_fallback_reason;   /* (ABI v7) why the LAST such batch fell back: BLHIP_FALLBACK_*             */
    int32_t peer_copy_path;       /* (ABI v7) how blhip_accum_peer_reduce / _gather fetched the other contexts' slices since the
                                     last blhip_fit of THIS context: BLHIP_PEER_* (0: no peer merge)                   */
    int32_t resident_probe;       /* (ABI v8) the co-residency probe of this call: 0 = none ran (it runs on a context's first fit, when
                                     the resident paths are re-armed and at most once per second), 1 = every block of a one-block-per-CU
                                     grid with the resident kernels' footprint was on the chip at once, 2 = not (another process holds
                                     CUs, a partitioned GPU): the resident paths are parked WITHOUT paying a launch's time-out     */
    int32_t xcd_order;            /* (ABI v8) 1: the probe saw block b on XCD b % 8 (the both-axes kernels publish their exchange with
                                     plain stores that stay in that XCD's L2); 0: it did not -- write-through exchange instead    */
} blhip_timing;

/* blhip_timing.peer_copy_path */
#define BLHIP_PEER_NONE         0
#define BLHIP_PEER_SAME_DEVICE  1   /* both contexts on one GPU (test configuration): device-to-device copy                       */
#define BLHIP_PEER_DIRECT       2   /* hipMemcpyPeerAsync over xGMI with peer access                                                */
#define BLHIP_PEER_HOST_STAGED  3   /* no peer access / a failed peer copy / option peer_copy_mode = 1: through page-locked host memory */

/* blhip_timing.resident_fallback_reason */
#define BLHIP_FALLBACK_NONE       0
#define BLHIP_FALLBACK_GAVE_UP    1   /* a block waited longer than the bound for a peer block (blocks not all co-resident: a
                                         shared or partitioned GPU); the context parks the resident paths (resident_armed = 0) */
#define BLHIP_FALLBACK_RANGE      2   /* a lagged sum left (1e-150, 1e150) or was not finite (extreme outliers, a zero normaliser) */
#define BLHIP_FALLBACK_PREDICTION 3   /* the predicted posterior sums did not reproduce the reduced ones                          */
#define BLHIP_FALLBACK_FORCED     4   /* option resident_force_abort (tests)                                                      */
#define BLHIP_FALLBACK_BUSY       5   /* (ABI v8) no launch was tried: the co-residency probe found the chip shared (resident_probe = 2) */

/* ---- context ------------------------------------------------------------------------------------------------- */
int         blhip_abi_version(void);
int         blhip_device_count(void);
/* Diagnostics / test infrastructure (needs no GPU, no context): the kernel instantiations this library holds -- every __global__
 * function it can launch registers itself when the library is loaded -- and how often THIS PROCESS has launched each.  Text, one
 * line per instantiation, sorted by name: "<launches>\t<kernel name with its template arguments>\n".  Writes at most cap - 1 bytes
 * + NUL into buf (buf may be NULL); returns the length of the whole text (call again with a larger buffer if >= cap), < 0 on error.
 * The -m gpu suite asserts that no line starts with "0": every kernel that ships has been compared with the oracle. */
int64_t     blhip_kernel_census(char *buf, int64_t cap);
blhip_ctx  *blhip_create(int device);
void        blhip_destroy(blhip_ctx *ctx);
const char *blhip_last_error(blhip_ctx *ctx);        /* ctx may be NULL for errors of blhip_create              */
int         blhip_device_name(blhip_ctx *ctx, char *buf, int buflen);
int         blhip_set_option(blhip_ctx *ctx, const char *key, double value);   /* tuning knobs, see DESIGN.md    */
int         blhip_synchronize(blhip_ctx *ctx);

/* ---- the hot path --------------------------------------------------------------------------------------------- */
/* Runs n_chains independent forward(-backward) passes that share `problem` and differ in the hyper-parameter value
 * of each op: op_values is (n_chains, n_ops), row-major; entries of STATIC ops are ignored.
 * log_chain_weight (n_chains,) is only read with BLHIP_ACCUMULATE: log of the hyper-prior value of each chain
 * (core.py:1366); the library adds the chain's log-evidence itself.
 * Threads: a call with several batches of chains starts ONE helper thread that prepares the next batch's per-step programs
 * from `problem` / `op_values` (read-only, no HIP call) and is joined before the call returns -- also on errors; option
 * build_ahead = 0 keeps everything on the calling thread.  One context must not be used by two threads at once. */
int blhip_fit(blhip_ctx *ctx, const blhip_problem *problem, int64_t n_chains, const double *op_values,
              const double *log_chain_weight, uint32_t flags, blhip_result *result);

int blhip_last_timing(blhip_ctx *ctx, blhip_timing *out);

/* Calibration of the attainable HBM rate on THIS device ("calibrate the attainable peak on the box"): a 16-B-per-
 * lane streaming copy of `bytes` (read + write counted), `iterations` launches timed with HIP events -> GB/s. */
int blhip_bandwidth_probe(blhip_ctx *ctx, int64_t bytes, int iterations, double *gb_per_s);

/* ---- page-locked host memory for the big read-backs -------------------------------------------------------------------------------
 * posteriorSequence is a HOST array in the reference (core.py:356, 408): (T, G) doubles, 16 GiB for BASELINE C3.  Into pageable
 * memory the copy is staged by the runtime (23 GB/s measured); into page-locked memory it is ONE DMA at the PCIe rate.  The host
 * side allocates its result arrays here (bayesloop_amd/engine.py keeps one freed block for the next fit).  NULL on failure. */
void *blhip_host_alloc(size_t bytes);
void  blhip_host_free(void *p);

/* ---- posterior sequence of the last blhip_fit(..., BLHIP_KEEP_POSTERIOR) ---------------------------------------- */
/* Copies the normalised posteriors of steps [t0, t1) of one chain to host memory ((t1-t0) * G doubles). */
int blhip_posterior_read(blhip_ctx *ctx, int64_t chain, int64_t t0, int64_t t1, double *host_out);
/* Device address of chain 0 / step 0 and the strides in doubles (device-side consumers, e.g. RCCL). */
int blhip_posterior_devptr(blhip_ctx *ctx, void **devptr, int64_t *chain_stride, int64_t *step_stride);
int blhip_posterior_release(blhip_ctx *ctx);

/* ---- reductions of a device-resident posterior sequence (consumers of posteriorSequence: marginal parameter
 *      distributions, bayesloop/core.py:915, 979-980; time average, core.py:588, 886) -------------------------------
 * source: 0 = posterior of `chain` kept by the last blhip_fit(BLHIP_KEEP_POSTERIOR), 1 = the finalised accumulator.
 * keep_axis: the parameter whose marginal is wanted; host_out is (T, n[keep_axis]) probabilities (sums, no density). */
int blhip_posterior_marginal(blhip_ctx *ctx, int source, int64_t chain, int keep_axis, double *host_out);
/* host_out is (G,): mean over time steps of the posterior. */
int blhip_posterior_time_average(blhip_ctx *ctx, int source, int64_t chain, double *host_out);

/* ---- posterior predictive (ABI v10; Study.simulate, bayesloop/core.py:566-597) ------------------------------------------------------
 *   host_out[t - t0][j] = sum over the grid cells of  L(x_j | cell) * sequence[t][cell]          t0 <= t < t1,  0 <= j < n_x
 * or, with average != 0, ONE row: the same sum against the mean of the rows [t0, t1) of the sequence (the whole sequence: t0 = 0, t1 = T).
 * Probabilities times likelihood values: no lattice constant, no normalisation over x -- the caller's, as in the reference.
 * source / chain: as blhip_posterior_marginal.  The contraction runs on the fp64 matrix pipe (blhip_predictive.hpp), split over slabs of
 * cells whose partial results are added in a fixed order: two calls on the same inputs return the same bits.
 * model: only obs_model, ndim, n[] and marginal[] are read (and the program the context is armed with, for BLHIP_OM_PROGRAM); the product
 * of n[] must be the number of cells of the sequence.  Where the likelihood rows L(x_j | .) come from:
 *   host_rows != NULL                      the caller's, (n_x, G) doubles on the host (any ObservationModel.pdf); uploaded chunk by chunk
 *   BLHIP_OM_GAUSSIAN, BLHIP_OM_POISSON    tabulated on the device from the formulas of observationModels.py:502 / :566-567.  Poisson: x_step
 *                                          holds k! of every value as a double, (n_x); values whose k! is no finite double, that are
 *                                          negative or no whole numbers belong to host_rows (the call refuses them)
 *   BLHIP_OM_BERNOULLI / _LAPLACE / _WHITE_NOISE   the kernel that builds their likelihood table for a fit, with x as the data
 *   BLHIP_OM_PROGRAM                       the armed program with x as the data; x_step: its STEP values, (n_x, n_step) (NULL: n_step = 0)
 *   anything else                          host_rows is required
 * The rows of a chunk of x values and the partial results live in a workspace of the context that stays within option mem_budget_bytes
 * (blhip_host_predictive_plan); x itself must be finite unless host_rows is given (then it is not read and may be NULL).
 * Errors (return -1, blhip_last_error; the context stays usable): no posterior kept / chain out of range / accumulator not finalised,
 * t0 < 0 or t1 > T or t0 >= t1, n_x < 1, a grid that does not match the sequence, a NULL model / x / host_out, a model that needs
 * host_rows, a budget below the plan's minimum. */
int blhip_posterior_predictive(blhip_ctx *ctx, int source, int64_t chain, int64_t t0, int64_t t1, int average, const blhip_problem *model,
                               const double *x, int64_t n_x, const double *x_step, const double *host_rows, double *host_out);
/* The plan of such a call, host-only (no GPU, no context): G cells, T output rows (1 with average), X values, `budget` bytes.
 * plan_out (6 values): cells per slab of the split over the cell axis, slabs (= blocks along it), x values per chunk, chunks, workspace
 * bytes (<= budget), the smallest budget accepted.  Slab s covers the cells [s * slab, min(G, (s + 1) * slab)), chunk c the values
 * [c * rows, min(X, (c + 1) * rows)).  Returns 0; -1 for bad arguments; 1 for a budget below the minimum (plan_out[5] is still written). */
int blhip_host_predictive_plan(int64_t G, int64_t T, int64_t X, int average, double budget, int64_t *plan_out);

/* ---- evidence-weighted average posterior (HyperStudy) ----------------------------------------------------------- */
/* The accumulator holds  A[t, cell] = sum_h exp(logE_h + log prior_h - log_ref) * max(post_h[t, cell], 1e-300)
 * in linear space with a running reference exponent `log_ref` (equal to the reference's log-space logaddexp
 * accumulation, core.py:1362-1366, up to rounding).  external_devptr, if not NULL, is caller-owned device memory of
 * T*G doubles (e.g. a torch tensor handed to RCCL); otherwise the library allocates it. */
int blhip_accum_begin(blhip_ctx *ctx, int64_t T, int64_t G, void *external_devptr);
int blhip_accum_state(blhip_ctx *ctx, double *log_ref, void **devptr, int64_t *n_folded);
/* Re-express the accumulator against a new reference exponent (>= current), e.g. the maximum over ranks, so that
 * accumulators of several GPUs can be summed (core.py:1339). */
int blhip_accum_rescale(blhip_ctx *ctx, double new_log_ref);
/* (ABI v8) Folds ONE chain whose posterior sequence the CALLER holds -- a hyper-grid point fitted through the transition-model plug-in
 * interface, where the state crosses the host at every step anyway (bayesloop_amd/core.py: Study._fitHostTransition) -- into the open
 * accumulator: posterior is (T, G) on the host, every row normalised; log_weight = logEvidence + log(hyper-prior value) of the chain
 * (core.py:1358-1366: acc = logaddexp(acc, log(max(post, 1e-300)) + log_weight); a non-finite log_weight contributes nothing).  The
 * sequence is uploaded and folded by the kernels that fold a stored batch. */
int blhip_accum_fold_host(blhip_ctx *ctx, const double *posterior, double log_weight);
/* Per-step normalisation (core.py:1379-1382) and posterior means (core.py:1416-1419); the normalised average stays
 * on the device and is read with blhip_accum_read.  posterior_mean: (ndim, T) or NULL. */
int blhip_accum_finalize(blhip_ctx *ctx, const blhip_problem *problem, double *posterior_mean);
int blhip_accum_read(blhip_ctx *ctx, int64_t t0, int64_t t1, double *host_out);
int blhip_accum_end(blhip_ctx *ctx);
/* Per-step sums of the (not yet finalised) accumulator, relative to its current reference exponent:
 * host_out (T, 1 + ndim) = [sum A, sum A grid_0, (sum A grid_1)] per step.  Sums of several ranks, each scaled by
 * exp(log_ref_rank - max log_ref), add up to the normalisers / posterior means of the merged average (core.py:1379-1382,
 * 1416-1419), so every rank can form them from ONE gather.  All zeros if nothing was folded. */
int blhip_accum_row_stats(blhip_ctx *ctx, const blhip_problem *problem, double *host_out);

/* ---- host-side algebra of the resident kernels, callable without a GPU (unit tests) ------------------------------------------------
 * The time-resident kernels divide step k not by the sum of step k - 1 but by something older (their sums cross the chip through
 * HBM); the host reconstructs the reference's normalisers (core.py:385) from the sums S_k they report:
 *   scheme 0 (blhip_resident.hpp):  s_k = 1 / S_(k-lag)                              norm_k = S_k / (S_(k-1) s_k)
 *   scheme 1 (blhip_chainres.hpp):  s_k = S_(k-lag-1) s_(k-lag) / S_(k-lag)          (s_k = 1 while k < lag, S_(-1) = 1)
 *   scheme 2 (blhip_chainclamp.hpp): scheme 1, except that a step whose kind has bit 6 (0x40) set -- a clamped step, RegimeSwitch -- ran at
 *                                    the exact scale s_k = 1 / S_(k-1); the lagged rule of later steps reads that scale like any other.
 *                                    The low six bits of a kind are the source kind as in scheme 1.
 * sums: (T) in, the normalisers out (in place).  kinds (scheme 1, may be NULL): (T) source kinds, a step whose kind is not 0
 * (blk::SRC_PREV) restarted from a distribution of known mass: norm_k = S_k / s_k.  scales_out (may be NULL): (T) the scales s_k.
 * Returns 0, or 1 if a sum left (1e-150, 1e150) -- the fit then repeats the batch with the launch-per-step kernels. */
int blhip_host_unlag(int scheme, double *sums, int64_t T, int lag, const unsigned char *kinds, double *scales_out);

/* Whether a two-parameter Gaussian fit takes the likelihood RECURRENCE along the rows (1) or one exponential per cell (0); -1: not such a
 * problem.  The recurrence carries exp() as mantissa * 2^exponent with the exponents added in int and its anchors clamped to +-1.4e9, so
 * it is used only while  dn (D^2 cA + |cB|) + 32 |d1| + 512 |d2| <= 1e9  for the largest cA = 1 / (2 s^2), |cB| = |log(2 pi s^2)| / 2 of
 * the std grid, the most values dn of a record, the largest distance D of a datum from the mean lattice continued 256 rows beyond either
 * end, and first / second differences d1, d2 of the argument over 4 rows.  bound_out (may be NULL): the left-hand side.  Reads
 * marginal[0..1], n, data, T, seg_len, data_dim of the problem. */
int blhip_host_rec_envelope(const blhip_problem *problem, double *bound_out);

/* Which records of a Poisson problem the step kernels evaluate DIRECTLY, lambda^k exp(-lambda) / k! factor by factor
 * (observationModels.py:502), and which in log space, exp(k ln(lambda) - lambda - ln k!) with ln k! from lgammal_r (long double, rounded once).  A record is in the direct
 * domain when every count is at most 170 (171! is inf), max count * ln(max rate) <= 700 (lambda^k overflows at 709.78) and the largest
 * rate of the grid is at most 708 (exp(-lambda) is a normal number); NaN counts are ignored.  Inside it the arithmetic is the one the
 * library has always used; outside it the factors would be inf, 0 or subnormal where the likelihood is an ordinary number.  direct_out
 * (may be NULL): (T) 1 / 0 per record.  Returns the number of direct records, or -1: not such a problem.  Reads marginal[0], n, data, T,
 * seg_len, data_dim of the problem. */
int blhip_host_poisson_direct(const blhip_problem *problem, int *direct_out);

/* The weights the host builds for a transition model's kernel, as the step kernels read them (unit tests hold them to the reference's
 * formulas without a GPU).  kind: 0 GaussianRandomWalk, params = {sigma in cells}: the 2 r + 1 weights of SciPy's gaussian_filter1d,
 * r = int(4 sigma + 0.5) (transitionModels.py:107-115); 1 Deterministic shift of |d| <= 12 cells, params = {d}: the 2 r + 1 stencil
 * weights K[m], m = -r .. r, r = ceil|d| + 34 (out[i] = sum_m K[m] ext[i + m]); 2 AlphaStableRandomWalk, params = {c in cells, alpha}: k[0 .. n-1]
 * (:196-240); 3 BivariateRandomWalk, params = {sigma1, sigma2 in cells, rho}: the (2 r0 + 1) x (2 r1 + 1) kernel, row-major (:898-911).
 * n: the axis length (kind 2 only; 2 .. 16384, c > 0, 0 < alpha <= 2).  out (may be NULL): `cap` doubles; radius_out (may be NULL): {r, r1} (r1 = 0 for 1-D sets).
 * Returns the number of weights (nothing is written beyond `cap`: call with out = NULL to size the buffer), or -1 for arguments
 * no builder takes. */
int64_t blhip_host_taps(int kind, int64_t n, const double *params, int n_params, double *out, int64_t cap, int *radius_out);

/* ---- likelihood programs (ABI v9; bayesloop_amd/likprogram.py compiles them from SymPy expressions) ---------------------------------
 * The density of an observation model as a postfix program over the data point and the grid's parameters: one {int32 code, int32 arg}
 * record per op, at most 256 ops, stack depth at most 16, exactly one value left at the end.
 *   pushes      CONST i: consts[i];  PARAM k: the marginal grid value of parameter k at the cell;  DATA: the datum of the current data
 *               dimension;  STEP j: step_values[t][dimension][j], a data-only subtree the caller evaluated (factorial(x), binomial(10, x));
 *               AXIS a: consts[(a >> 2) + index of the cell along parameter (a & 3)], a function of ONE parameter the caller tabulated
 *               along that parameter's axis inside `consts`
 *   arithmetic  ADD MUL DIV NEG ABS SQRT EXP LOG POW COS SIN;  POWI n: integer exponent |n| <= 64 by multiplications (x**2 is x * x)
 *   logic       LT LE EQ (1.0 / 0.0), AND, SELECT (a b c -> c != 0 ? a : b)
 * The likelihood of a step is the product over the data dimensions of the density; a NaN datum contributes the factor 1
 * (observationModels.py:35-56). */
enum {
    BLHIP_LP_CONST = 0, BLHIP_LP_PARAM = 1, BLHIP_LP_DATA = 2, BLHIP_LP_STEP = 3, BLHIP_LP_AXIS = 4,
    BLHIP_LP_ADD = 5, BLHIP_LP_MUL = 6, BLHIP_LP_DIV = 7, BLHIP_LP_NEG = 8, BLHIP_LP_ABS = 9, BLHIP_LP_SQRT = 10, BLHIP_LP_EXP = 11,
    BLHIP_LP_LOG = 12, BLHIP_LP_POW = 13, BLHIP_LP_COS = 14, BLHIP_LP_SIN = 15, BLHIP_LP_POWI = 16,
    BLHIP_LP_LT = 17, BLHIP_LP_LE = 18, BLHIP_LP_EQ = 19, BLHIP_LP_AND = 20, BLHIP_LP_SELECT = 21
};
/* Arms the context: the next blhip_fit / blhip_accum_* problems whose obs_model is BLHIP_OM_PROGRAM evaluate THIS program (the arrays are
 * copied; it stays armed until the next call).  ops: n_ops records (2 n_ops int32); consts: n_consts doubles; step_values:
 * (T, data_dim, n_step) doubles (NULL when n_step = 0).  The program is validated here (blhip_host_lik_program_check, with the 4
 * parameters an ABI grid can have at most) and again against the problem: a fit with BLHIP_OM_PROGRAM and no armed program fails, so does
 * one whose T * data_dim * n_step differs from n_step_values, the number of doubles passed here. */
int blhip_set_lik_program(blhip_ctx *ctx, const int32_t *ops, int64_t n_ops, const double *consts, int64_t n_consts,
                          const double *step_values, int64_t n_step, int64_t n_step_values);
/* Host-only validation (no GPU, no context): the stack discipline (no underflow, depth <= 16, one value left), n_ops <= 256, every CONST /
 * STEP / PARAM / AXIS index in range, |n| of POWI <= 64.  Returns 0, or -1 with the reason in err (errlen bytes, may be NULL). */
int blhip_host_lik_program_check(const int32_t *ops, int64_t n_ops, int64_t n_consts, int64_t n_step, int ndim, char *err, int errlen);
/* Runs the SAME kernel a fit runs for the armed program on the grid marginal[0 .. ndim-1] (n[k] values each) and the data (T, data_dim),
 * and copies the (T, G) table to host memory `out`: what the cell-by-cell tests read. */
int blhip_lik_program_eval(blhip_ctx *ctx, int ndim, const int64_t *n, const double *const *marginal, int64_t T, int data_dim,
                           const double *data, double *out);

/* ---- series fits (ABI v14; Study.fitMany of bayesloop_amd: the user's loop `for d in series: S.loadData(d); S.fit()` around Study.fit,
 *      bayesloop/core.py:330-486, as ONE blhip_fit) ---------------------------------------------------------------------------------------
 * Many short data series on a one-parameter grid -- one Poisson rate per neuron, one Bernoulli rate per subject -- are many single chains,
 * none of which fills the chip.  blhip_set_series arms the context: in the NEXT blhip_fit chain c observes series c.
 *   data: (S, T, seg_len, data_dim) on the host, T / seg_len / data_dim those of that fit's problem; NOT copied: the caller keeps it alive
 *         until that fit has returned.  Series shorter than T are padded with NaN at the end by the caller (a NaN step has likelihood 1).
 *   The next blhip_fit must be called with n_chains == S; chain c's row of op_values is still its own; problem->data is ignored.  The
 *   call disarms itself with that fit, whether it succeeds or fails.  BLHIP_RESUME, BLHIP_CARRY and BLHIP_ACCUMULATE are refused.
 * Every batch of such a fit runs on the chain-resident 1-D kernel (one block per chain, the whole pass in LDS) over a (B, T, n) likelihood
 * table built in one launch from the series' data by the device functions a single fit evaluates; a fit the kernel's envelope does not
 * take (row length, radius against the LDS of a CU, options chain1d / chain1d_long / chain1d_shift / chain1d_clamp / fuse1d, option
 * series_fit = 0) fails with the reason, and the caller runs its loop.
 * blhip_host_series_check (host only, no GPU, no context): 0 when the path admits the problem -- a 1-D grid, BLHIP_OM_POISSON /
 * _GAUSSIAN_MEAN / _BERNOULLI / _WHITE_NOISE, seg_len 1, a row of at most 8192 cells, no backward_init, no AlphaStable / Bivariate op, none
 * of the three flags above (flags: those of blhip_fit) --, else 1 with the reason in err (errlen bytes, may be NULL).  With
 * BLHIP_SERIES_RAGGED in flags (this function only: the series differ in length or in their time stamps) the program must be
 * time-independent as well: Static, GRW and REGIMESWITCH ops outside serial models only.
 * blhip_host_series_plan (host only): plan_out (4 values) = chains per batch (at most 4096), batches, bytes of such a batch, the smallest
 * budget accepted; a chain counts its state ping-pong, stored sequence and partial sums as in any fit plus its (T, n) likelihood table,
 * T n 8 bytes.  Batch b covers the chains [b * per, min(S, (b + 1) * per)).  Returns 0; -1 for bad arguments or a problem the check
 * refuses; 1 for a budget below the minimum (plan_out[3] is still written).
 *
 * Two-parameter grids (same functions, same signatures; ABI v14 still): the batches run on the chain-resident kernels blc::chain_kernel (Static,
 * a GaussianRandomWalk on the first parameter, change- and break-points; BLHIP_OM_GAUSSIAN with the likelihood recurrence, or a likelihood
 * table per chain for BLHIP_OM_LAPLACE / _AR1 / _SCALED_AR1) and blc::chainax_kernel (walks on both parameters; BLHIP_OM_GAUSSIAN only), one
 * launch per pass and round of chains; every chain reads its own records, anchors or table through a per-chain stride.  A batch those
 * kernels do not take -- a radius beyond their bands, options chain_resident / chain_table / chain_ax1 / chain_depad, a recurrence outside
 * its envelope over ANY series, memory -- or whose pass gives up or fails its host check fails with "series fit: ..." and the caller runs
 * its loop: no other kernel reads per-chain data.
 * blhip_host_series_check admits there: BLHIP_OM_GAUSSIAN (data_dim <= 4) / _LAPLACE / _AR1 / _SCALED_AR1; 32 .. 1024 rows (table models:
 * <= 512, and no padded geometry of 384 / 512 rows), 1 .. 1024 columns; Static / GRW / CHANGEPOINT / BREAKPOINT ops only (RegimeSwitch,
 * NotEqual, Deterministic, AlphaStable, Bivariate: refused); walks on both parameters for BLHIP_OM_GAUSSIAN on grids of 32 .. 512 rows and
 * columns; no backward_init; a padded grid of 513 .. 1024 rows only with BLHIP_FORWARD_ONLY or BLHIP_EVIDENCE_ONLY in flags (a full fit of it
 * has no storing backward kernel).  BLHIP_SERIES_RAGGED is refused.  Every refusal there contains "a grid of 2 parameters".
 * blhip_host_series_plan counts a chain there on the padded geometry Gk of the kernels (rows a multiple of 128, 1024 beyond 512; columns a
 * multiple of 16; walks on both parameters: the next square of 128 / 256 / 512): (T + 2) Gk 8 bytes of states and stored sequence (2 Gk 8
 * evidence-only), the partial sums, T G 8 for the de-padding copy where the grid is padded or both parameters walk (not evidence-only),
 * its data, and its anchors T x 8 x (columns / 16) x 64 x 32 bytes (BLHIP_OM_GAUSSIAN without a walk on the second parameter) or its
 * (T, G) table (the table models).  At most 1024 chains per batch; a count of 16 or more that memory limits is cut to a multiple of 8. */
#define BLHIP_SERIES_RAGGED 0x10000
int blhip_set_series(blhip_ctx *ctx, const double *data /* (S, T, seg_len, data_dim), host */, int64_t S);
int blhip_host_series_check(const blhip_problem *problem, int64_t S, int flags, char *err, int errlen);
int blhip_host_series_plan(const blhip_problem *problem, int64_t S, int flags, double budget, int64_t *plan_out);

/* ---- series in groups (ABI v15; HyperStudy.fitMany / ChangepointStudy.fitMany of bayesloop_amd: the user's loop `for d in series:
 *      H.loadData(d); H.fit()` around HyperStudy.fit, bayesloop/core.py:1247-1441, as ONE blhip_fit per batch of series) ----------------------
 * blhip_set_series_groups arms the context as blhip_set_series does, with H chains per series: the next blhip_fit must be called with
 * n_chains == S * H, chain c observes series c / H with the op values of its own row (the caller repeats the H rows of its hyper-grid S
 * times).  One-parameter grids only; blhip_set_series is H = 1, with its behaviour and messages unchanged.  The (T, n) likelihood table
 * is built once per SERIES of a batch and shared by the chains of its group; a batch of an evidence-only fit may begin and end inside a
 * group.  Every batch runs on the chain-resident 1-D kernel or fails with "series fit: ...", as above.
 * BLHIP_ACCUMULATE (with log_chain_weight and BLHIP_KEEP_POSTERIOR; forward-only or full fits) is admitted for groups and means the GROUPED
 * FOLD: behind the passes each group is folded into its own average
 *     A[s][t][cell] = sum_h w[s, h] * max(post[s, h][t][cell] / rowsum[s, h][t], 1e-300),   w = exp(logE + log_chain_weight - ref_s),
 * ref_s the maximum over the group's valid chains (an aborted chain, a non-finite evidence or a -inf weight contributes nothing), in one
 * launch of blk::series_group_fold_kernel; the averages are row-normalised and become the context's kept posterior: S chains of T rows,
 * blhip_posterior_read / _marginal / _query / _bins / _predictive with chain = s then read series s's average.  A series no chain
 * contributed to is all NaN.  The context's accumulator (blhip_accum_*) is neither used nor changed and need not be begun.  All groups
 * of such a fit are one batch (blhip_host_series_group_plan says how many fit).
 * Results of a grouped fold: log_evidence, local_evidence, abort_step, abort_phase are per CHAIN (S * H entries) as in any fit;
 * posterior_mean, where given, holds the means of the AVERAGES in its first S entries -- posterior_mean[(s * ndim + k) * T + t] for series
 * s, the layout chain s's means would have -- and the chains' own means are not formed (the rest of the array is not written).
 * blhip_host_series_group_check (host only): blhip_host_series_check's rules for H = 1; for H > 1 a one-parameter grid, H <= 4096, and
 * those rules without the refusal of BLHIP_ACCUMULATE.
 * blhip_host_series_group_plan (host only): plan_out (4 values) = groups per batch, batches, bytes of such a batch, the smallest budget
 * accepted (one group).  A group counts H chains as blhip_host_series_plan counts them, less the H - 1 likelihood tables they do not own,
 * plus (not evidence-only) one (T, n) average.  max_batch: the cap in chains, at most and by default (<= 0) the 1-D batch cap of 4096
 * (the caller's option max_batch).  Returns 0; -1 for bad arguments or a problem the check refuses; 1 when one group exceeds the cap or
 * the budget, with the reason in err (plan_out[3] is still written): the caller runs its loop.  H = 1 gives blhip_host_series_plan's
 * figures under the same cap. */
int blhip_set_series_groups(blhip_ctx *ctx, const double *data /* (S, T, seg_len, data_dim), host */, int64_t S, int64_t H);
int blhip_host_series_group_check(const blhip_problem *problem, int64_t S, int64_t H, int flags, char *err, int errlen);
int blhip_host_series_group_plan(const blhip_problem *problem, int64_t S, int64_t H, int flags, double budget, int64_t max_batch,
                                 int64_t *plan_out, char *err, int errlen);

/* ---- multi-GPU exchange of a sharded hyper-study (HyperStudy.fit(nJobs > 1), core.py:1307-1340, 1443-1495) -------------
 * One process per GPU, one context per process; each rank fits its share of the hyper-grid points with blhip_fit and
 * no communication, then the ranks exchange results through RCCL (xGMI inside a node), which this library binds
 * directly: librccl.so.1 is dlopen'ed by the first blhip_comm_* call (override the path with BLHIP_RCCL_LIBRARY).
 *   rank 0:      blhip_comm_unique_id(id)  ->  the caller hands the 128 bytes to the other ranks (file, socket, ...)
 *   every rank:  blhip_comm_init(ctx, id, world, rank)                      (collective; ncclCommInitRank on ctx's device)
 *   after the fits, the ONE exchange:
 *                blhip_comm_allgather   packed rows [logEvidence | localEvidence (T) | abort step] per chain + a trailer
 *                                       [accumulator log_ref | row stats], `count` doubles per rank, host in / host out
 *                                       (staged through HBM; host_out is (world, count) in rank order)     core.py:1335-1337
 *                blhip_comm_reduce_accum  only when posteriors are wanted, after blhip_accum_rescale(max log_ref):
 *                                       ncclReduce(sum) of the (T, G) accumulators to `root`, in place       core.py:1338-1340
 *   blhip_comm_allreduce: small host vectors (barriers, max-over-ranks timing of bench.py). */
#define BLHIP_UNIQUE_ID_BYTES 128
enum { BLHIP_SUM = 0, BLHIP_MAX = 1, BLHIP_MIN = 2 };
int blhip_comm_unique_id(void *id_out /* BLHIP_UNIQUE_ID_BYTES */);      /* errors: blhip_last_error(NULL) */
int blhip_comm_init(blhip_ctx *ctx, const void *unique_id, int world, int rank);
int blhip_comm_info(blhip_ctx *ctx, int *world, int *rank, int *rccl_version);   /* world = 1 without a communicator */
int blhip_comm_allgather(blhip_ctx *ctx, const double *host_in, int64_t count, double *host_out);
int blhip_comm_allreduce(blhip_ctx *ctx, double *host_inout, int64_t count, int op);
int blhip_comm_reduce_accum(blhip_ctx *ctx, int root);
int blhip_comm_timing(blhip_ctx *ctx, double *reduce_ms);     /* HIP-event time of the last blhip_comm_reduce_accum (ms) */
int blhip_comm_destroy(blhip_ctx *ctx);

/* ---- the same merge inside ONE process that drives several GPUs (HyperStudy.fit(nJobs = N), core.py:1307-1340: one context per
 * device, one host thread per context; no RCCL): peer copies over xGMI.  Every accumulator involved must be open, of the same shape
 * and at the same reference exponent (blhip_accum_rescale), every context idle (blhip_synchronize); the caller orders the calls of
 * its threads with host barriers.  The merge is a reduce-scatter over time slices followed by a gather:
 *   blhip_accum_peer_reduce   dst.acc[row0:row1] += sum_i srcs[i].acc[row0:row1]   (rows fetched concurrently, one stream -- one
 *                             xGMI link -- per source; summed in list order: the same result on every run)
 *   blhip_accum_peer_gather   dst.acc[row0[i]:row1[i]] = srcs[i].acc[row0[i]:row1[i]]   for every i (concurrent copies)
 * at most NBS = 18 sources per call. */
int blhip_accum_peer_reduce(blhip_ctx *dst, blhip_ctx *const *srcs, int n_srcs, int64_t row0, int64_t row1);
int blhip_accum_peer_gather(blhip_ctx *dst, blhip_ctx *const *srcs, int n_srcs, const int64_t *row0, const int64_t *row1);

/* ---- carried states (OnlineStudy.step, core.py:2062-2226) ------------------------------------------------------------
 * A blhip_fit with BLHIP_CARRY leaves every chain's normalised filtered distribution of its last step in slot
 * `carry_slot` of the context; the next call with BLHIP_RESUME continues from it.  What the online study does with these
 * states after each step (core.py:2196-2212) are evidence-weighted sums over chains:
 *   mix = (accumulate ? mix : 0) + sum_j weights[j] * state_j      (transitionModelPosterior / marginalizedPosterior)
 * blhip_carry_read copies one chain's state (chain >= 0) or the mix buffer (chain = -1, slot ignored) to the host, (G,). */
int blhip_carry_mix(blhip_ctx *ctx, int slot, int64_t n_chains, const double *weights, int accumulate);
int blhip_carry_read(blhip_ctx *ctx, int slot, int64_t chain, double *host_out);
/* Restores carried states saved with blhip_carry_read (a pickled OnlineStudy that continues in another process / context,
 * reference fileIO.py:10-37): host_in is (n_chains, G), every row a normalised distribution. */
int blhip_carry_write(blhip_ctx *ctx, int slot, int64_t n_chains, int64_t G, const double *host_in);
int blhip_carry_release(blhip_ctx *ctx, int slot);   /* slot < 0: all slots and the mix buffer */

/* ---- blocks of an online study (ABI v11; OnlineStudy.stepMany of bayesloop_amd: N data points of a recorded series in one call) -------
 * Every chain of an online study is an independent forward filter, so a block of N points is, per transition model, ONE blhip_fit of N
 * steps with BLHIP_RESUME | BLHIP_CARRY (every time stamp and resume_time = -1: OnlineStudy evaluates each transition there,
 * core.py:2164-2165) -- evidence-only, or BLHIP_FORWARD_ONLY | BLHIP_KEEP_POSTERIOR when the study stores its history.  What the
 * reference forms once per data point (core.py:2194-2211) is then a mixture over chains whose weights change with the time step:
 *   H[plane][t][cell] = (accumulate ? H[plane][t][cell] : 0) + sum_b weights[t][b] * seq[b][t][cell]      (b ascending, no atomics:
 *                                                                                     two calls on the same inputs return the same bits)
 * into a history of n_planes planes of (T, G) cells the context owns.  source 0: seq = the normalised sequence the last forward-only
 * BLHIP_KEEP_POSTERIOR fit left in the context (n_chains and T must be its chains and steps); source 1: seq = the planes 1 .. n_planes - 1
 * of the history itself, mixed into plane 0 (n_chains = n_planes - 1) -- a study of M > 1 transition models keeps one plane per model
 * (weights: the model's hyper-parameter distribution, known once ITS fit is done) and mixes them with the transition-model distribution
 * when the last model is done.  weights: (T, n_chains) on the host.  A call whose n_planes, T or grid differ from the history's starts a
 * new one (then accumulate must be 0 and source 0).
 * blhip_mix_means: host_out (T, ndim) = sum over the cells of plane 0 of H * grid_k (only ndim, n[] and marginal[] of the problem are read).
 * blhip_mix_read: the rows [t0, t1) of a plane, one ranged copy.
 * blhip_carry_copy: the carried states of src_slot -> dst_slot on the device (the states a block resumed from, kept until the block is done).
 * blhip_mem_budget: the bytes a fit's memory plan works with on this context right now (0.9 x min(free + reusable buffers, option
 * mem_budget_bytes)): what blhip_host_online_block_plan is asked with.
 * blhip_host_online_block_plan (host only, no GPU, no context): a resumed fit needs all chains of a model in one batch, so a long block is
 * cut along TIME.  plan_out (4 values): the largest number of steps per chunk for which the kept sequence of a model of `chains` chains
 * (as a fit's memory plan counts it) plus `planes` history planes fit in `budget` bytes, the number of chunks of a block of N steps, the
 * bytes of such a chunk, the bytes of a one-step chunk.  Returns 0; -1 for bad arguments; 1 for a budget below one step (plan_out[3] is
 * still written). */
int blhip_mix_sequence(blhip_ctx *ctx, int source, int64_t plane, int64_t n_planes, int64_t n_chains, int64_t T, const double *weights,
                       int accumulate);
int blhip_mix_means(blhip_ctx *ctx, const blhip_problem *problem, double *host_out);
int blhip_mix_read(blhip_ctx *ctx, int64_t plane, int64_t t0, int64_t t1, double *host_out);
int blhip_carry_copy(blhip_ctx *ctx, int src_slot, int dst_slot);
int blhip_mem_budget(blhip_ctx *ctx, double *bytes_out);
int blhip_host_online_block_plan(int ndim, const int64_t *n, int64_t chains, int64_t planes, int64_t N, double budget, int64_t *plan_out);

/* ---- probability queries at many time steps (ABI v12; bl.Parser / Study.eval with a vector of time stamps, bayesloop/parser.py:256-440,
 *      core.py:604-621) ----------------------------------------------------------------------------------------------------------------
 *   one space  (n_b = 0):  host_out[s] = sum over the cells c of A with  f(c, s) REL 0  of  sequence[steps[s]][c]
 *   two spaces (n_b > 0):  host_out[s] = sum over the pairs (c, j) with  f(c, j, s) REL 0  of  sequence[steps[s]][c] * b_prob[s][j]
 *                                        divided by  (sum_c sequence[steps[s]][c]) (sum_j b_prob[s][j])        (parser.py:239-243)
 * A is the parameter grid of the sequence (source / chain: as blhip_posterior_marginal), B a second, independent quantity the caller holds.
 * f is a postfix program in the instruction set of the likelihood programs (BLHIP_LP_*; no DATA, AND, SELECT) that leaves one value:
 *   PARAM k   the marginal grid value of parameter k of A at the cell          AXIS   as in a likelihood program: a table along ONE axis of A
 *   STEP j    series[s][j], the value of the step                               CONST  consts[i]
 *   BLHIP_QP_BCOL k   b_values[k][j]: a value column of B, or a function of B alone the caller tabulated
 * One IEEE operation per op, nothing contracted; a NaN compares false.  relation: BLHIP_QR_*.  steps: rows of the sequence in any order,
 * repeats allowed.  The uploads and the per-slab partial sums live in a workspace of the context that stays within option
 * mem_budget_bytes (blhip_host_query_plan); a call that does not fit is cut along the steps.  Partial sums are added in a fixed order: two
 * calls on the same inputs return the same bits.
 * Validation happens on the host before anything is launched (blhip_host_query_check: the same checks without a context).
 * Errors (return -1, blhip_last_error; the context stays usable): no posterior kept / chain out of range / accumulator not finalised, a
 * step out of range, a grid that does not match the sequence, stack or index violations of the program, a NULL pointer, a series value
 * that is not finite, a budget below the plan's minimum. */
#define BLHIP_QP_BCOL 32
enum { BLHIP_QR_LT = 0, BLHIP_QR_LE = 1, BLHIP_QR_EQ = 2, BLHIP_QR_GT = 3, BLHIP_QR_GE = 4 };
typedef struct blhip_query {
    int32_t        n_ops, n_consts, n_series, relation;
    const int32_t *ops;                       /* (n_ops, 2) {code, arg}                                          */
    const double  *consts;                    /* (n_consts) constants and AXIS tables                            */
    const double  *series;                    /* (n_steps, n_series) STEP values (NULL: n_series = 0)            */
    int32_t        ndim, b_const;             /* b_const != 0: b_prob is ONE row, the same at every step         */
    int64_t        n[BLHIP_MAX_DIM];          /* the grid of A; the product must be the cells of the sequence    */
    const double  *marginal[BLHIP_MAX_DIM];
    int64_t        n_b;                       /* cells of B; 0: one space                                        */
    int32_t        n_bcols, reserved0;
    const double  *b_values;                  /* (n_bcols, n_b)                                                  */
    const double  *b_prob;                    /* (b_const ? 1 : n_steps, n_b)                                    */
} blhip_query;
int blhip_posterior_query(blhip_ctx *ctx, int source, int64_t chain, const int64_t *steps, int64_t n_steps, const blhip_query *query,
                          double *host_out);
/* The checks of a query that need no sequence, host-only (no GPU, no context): 0, or -1 with the message in err. */
int blhip_host_query_check(const blhip_query *query, int64_t n_steps, char *err, int errlen);
/* The plan of such a call, host-only: G cells of A, n_steps steps, n_series STEP values per step, n_b cells of B (0: one space), b_const,
 * fixed_bytes of uploads that do not depend on the step (program, constants, grids, B's columns, a constant b_prob), `budget` bytes.
 * plan_out (6 values): cells of A per slab, slabs (= blocks along the cells), steps per chunk, chunks, workspace bytes (<= budget), the
 * smallest budget accepted.  Slab k covers the cells [k * slab, min(G, (k + 1) * slab)), chunk c the steps [c * spc, min(n_steps,
 * (c + 1) * spc)).  Returns 0; -1 for bad arguments; 1 for a budget below the minimum (plan_out[5] is still written). */
int blhip_host_query_plan(int64_t G, int64_t n_steps, int64_t n_series, int64_t n_b, int b_const, int64_t fixed_bytes, double budget,
                          int64_t *plan_out);

/* ---- derived distributions at many time steps (ABI v13; bl.Parser / Study.eval WITHOUT a relation and with a vector of time stamps,
 *      bayesloop/parser.py:399-418: the binned distribution of a derived quantity) ----------------------------------------------------
 *   host_out[s][b] = sum of sequence[steps[s]][c] over the cells c with bin[c] == b          (n_steps, n_bins), C order
 * bin (G): the bin of every cell of the sequence's grid, -1 = the cell is left out; the caller bins the grid (for a query over the
 * parameters of one study the map does not depend on the step).  source / chain: as blhip_posterior_marginal.  steps: rows of the
 * sequence in any order, repeats allowed.  n_bins: 1 .. 2^31 - 1.  No floating-point atomics: the order of the additions is fixed by
 * the map (bayesloop_amd/csrc/blhip_bins.hpp), two calls on the same inputs return the same bits, and so does a call the budget cuts
 * into chunks.  The order of the map, the steps of a chunk, the partial sums and the result live in a workspace of the context within
 * 0.9 * option mem_budget_bytes (blhip_host_bins_plan); a call that does not fit is cut along the steps.
 * Validation happens on the host before anything is launched (blhip_host_bins_check: the checks of the map without a context).
 * Errors (return -1, blhip_last_error; the context stays usable): no posterior kept / chain out of range / accumulator not finalised, a
 * step out of range, a map whose length does not match the sequence, a bin outside -1 .. n_bins - 1, a NULL pointer, a budget below
 * the plan's minimum. */
int blhip_posterior_bins(blhip_ctx *ctx, int source, int64_t chain, const int64_t *steps, int64_t n_steps, const int32_t *bin, int64_t G,
                         int64_t n_bins, double *host_out);
/* The checks of a map, host-only (no GPU, no context): 0, or -1 with the message in err. */
int blhip_host_bins_check(const int32_t *bin, int64_t G, int64_t n_bins, char *err, int errlen);
/* The plan of such a call, host-only.  bin: the map, or NULL for the shape alone (no runs, no tables).  plan_out (12 values): cells per
 * slab, slabs, steps per block, group width chosen for the map, runs (pairs of a slab and a bin it touches), groups, bytes of the
 * map's tables, steps per chunk, chunks, workspace bytes (<= budget), the smallest budget accepted, bytes of LDS per block.
 * Returns 0; -1 for bad arguments; 1 for a budget below the minimum (plan_out is still written). */
int blhip_host_bins_plan(const int32_t *bin, int64_t G, int64_t n_bins, int64_t n_steps, double budget, int64_t *plan_out);

#ifdef __cplusplus
}
#endif
#endif /* BLHIP_H */
