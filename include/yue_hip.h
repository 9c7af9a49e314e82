/*
 * yue_hip.h -- C ABI of libyue_hip.so: the MI355X (gfx950) BPR training + top-N scoring path
 * that replaces the NumPy loop of 0411tony/Yue behind its Recommender plugin surface.
 *
 * Plain pointers and sizes only; all pointers are HOST pointers owned by the caller and are
 * borrowed for the duration of the call (NumPy owns P/Q).  Device memory lives
 * behind the opaque context.  Every function returns 0 on success; otherwise a negative
 * status and yue_last_error() holds a thread-local message (the reference's convention is
 * print + exit(-1): tool/config.py:9-11, base/IterativeRecommender.py:64-66 -- the Python
 * shim does exactly that with the message).
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   yue_set_factors / yue_get_factors   state contract of IterativeRecommender.initModel
 *                                       (base/IterativeRecommender.py:36-39): P[m,k], Q[n,k] fp32 C-order
 *   yue_set_interactions                userListen + userRecord iteration of BPR.buildModel
 *                                       (recommender/cf/BPR.py:32-35,42-45; data/record.py:138-163)
 *   yue_bpr_replay                      the epoch body recommender/cf/BPR.py:42-58 on an explicit
 *                                       (u,i,j) stream, exact sequential semantics
 *   yue_cune_steps                      the two-level BPR loop of recommender/advanced/CUNE.py:126-172
 *   yue_bpr_rounds / yue_bpr_epoch      the same triplet update in rounds (DESIGN.md "S-round"),
 *                                       yue_bpr_epoch fuses the negative sampler of BPR.py:46-48
 *   yue_sumsq                           the regulariser sums of BPR.py:59
 *   yue_scores                          BPR.predict / IterativeRecommender.predict
 *                                       (recommender/cf/BPR.py:131-134, base/IterativeRecommender.py:58-60)
 *   yue_topn_scan                       the per-user mask + seed + overwrite-scan of
 *                                       IterativeRecommender.evalRanking (base/IterativeRecommender.py:96-145)
 *                                       and ranking_performance (:186-228)
 */
#ifndef YUE_HIP_H
#define YUE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yue_ctx yue_ctx;

#define YUE_OK              0
#define YUE_ERR_ARG        -1   /* bad argument / call order */
#define YUE_ERR_HIP        -2   /* HIP runtime error */
#define YUE_ERR_FEW_ITEMS  -3   /* a user has fewer than N candidates (reference: IndexError) */
#define YUE_ERR_COMM       -4   /* RCCL error */
#define YUE_ERR_SATURATED  -5   /* yue_cdae_step: a sampled output rounds to 1.0f; nothing was updated */

#define YUE_MAX_ATTEMPTS   64   /* negative-sampler attempts before a triplet is skipped */
#define YUE_UNIQUE_ID_BYTES 128

const char *yue_last_error(void);
int yue_version(void);

/* device = HIP ordinal.  HIP is initialised here, never earlier (fork-safety: yue.py:94-105). */
int yue_ctx_create(int device, yue_ctx **out);
int yue_ctx_destroy(yue_ctx *ctx);
int yue_sync(yue_ctx *ctx);

/* Factor matrices, fp32 row-major.  k <= 256, m and n below 2^31 rows, any size in bytes: item matrices of 2 GiB and more per GPU
 * are taken by yue_bpr_epoch's default path and by the scoring calls; yue_bpr_rounds, yue_bpr_replay, the option epoch_exact and
 * round_meta = 0 refuse them (their kernels address item rows with 31-bit byte offsets). */
int yue_set_factors(yue_ctx *ctx, const float *P, int64_t m, const float *Q, int64_t n, int k);
int yue_get_factors(yue_ctx *ctx, float *P, float *Q);

/*
 * Training interactions of this context's item range (all items on one GPU).
 *   indptr[m+1], indices[nnz]  sorted-unique listened items per user (negative rejection)
 *   ev_ptr[m+1], ev_i[E]       events in userRecord order: user-major, users by ascending id,
 *                              duplicates kept (one triplet per event, BPR.py:44)
 */
int yue_set_interactions(yue_ctx *ctx, const int64_t *indptr, const int32_t *indices,
                         const int64_t *ev_ptr, const int32_t *ev_i);

/* Exact sequential semantics of BPR.py:42-58 on explicit triplets, any order of users: one dataflow launch in which every
 * triplet waits for exactly the earlier triplets that share a row with it (chain_kernels.hpp; row ordinals and runs of
 * equal users are computed on the device, the host only copies the stream up).  j[t] < 0 skips the triplet.
 * nll_out = sum of -log(s).  Ids are checked on the device before anything is written. */
int yue_bpr_replay(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T,
                   double lr, double regU, double regI, double *nll_out);

/* The reference's LIVE path (recommender/cf/BPR.py:83-129, a TensorFlow-1 graph): one minibatch step on the fed triplets
 * (the reference feeds 512 events x 100 negatives, :65-81) -- loss = sum softplus(-(U[u].V[i] - U[u].V[j])) + reg * (l2_loss of
 * the three gathered row sets), then Adam (beta1 0.9, beta2 0.999, epsilon 1e-8, TF-1 sparse apply = dense Adam with zero
 * gradients on untouched rows) on both factor matrices, all in float32.  step = 1, 2, ... (Adam's bias correction).
 * yue_adam_reset clears the moments (also done implicitly when the factor shapes change).  PARITY UNPINNED: no TensorFlow
 * here; the checker is oracle/numpy_adam.py, a restatement of the graph as written. */
int yue_adam_reset(yue_ctx *ctx);
/* The moments of the uploaded factors' Adam state, [m][k] / [n][k] float32 each (any may be NULL). */
int yue_adam_get_moments(yue_ctx *ctx, float *mU, float *vU, float *mV, float *vV);
int yue_adam_step(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T,
                  double lr, double reg, int64_t step, double *loss_out);

/* CUNE's two-level BPR steps (reference recommender/advanced/CUNE.py:126-172) on explicit (u, i, k, j) steps, exact
 * sequential semantics in the given order: k[t] >= 0 is the step with a friends' item k ((i over k), then (k over j) with
 * margin and step scaled by 1/s, then the decays :156-159), k[t] < 0 the plain (i over j) step of :166-172.
 * loss_out[T] = every step's -log sigmoid term(s) on its final rows (the caller adds them up the way :161 / :175 do).
 * The user network / Word2Vec stage that produces the friends' items (CUNE.py:34-118) is not part of this library. */
int yue_cune_steps(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *k, const int32_t *j, int64_t T,
                   double s, double lr, double regU, double regI, double *loss_out);

/* Explicit triplets, S-round semantics: rounds are round_ptr[r]..round_ptr[r+1] (n_rounds+1 entries). */
int yue_bpr_rounds(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j,
                   const int64_t *round_ptr, int64_t n_rounds,
                   double lr, double regU, double regI, double *nll_out);

/*
 * One epoch over the uploaded events; negatives from the device's counter-based sampler.
 * Rounds are blocks of whole users holding about round_events events (0 = the device's default,
 * yue_default_round_events): users per block = floor(round_events / (events per user) + 1/2) from the
 * job-wide event count, the same blocks on every rank of a communicator, where the blocks' user-factor
 * differences are all-reduced.  (yue_amd/dist.py: epoch_round_ptr restates the rule.)
 * Outputs: nll (sum of -log s over this rank's triplets), sums of squares of P and of this
 * rank's Q after the epoch (for BPR.py:59).  Any output pointer may be NULL.
 */
int yue_bpr_epoch(yue_ctx *ctx, uint64_t seed, uint32_t epoch, int64_t round_events,
                  double lr, double regU, double regI,
                  double *nll_out, double *sumsqP_out, double *sumsqQ_out);

/* The host-side schedule of yue_bpr_epoch, as a pure function (no device, no context): users per round
 * (user_block = floor(round_events / (events_total / nranks / m) + 1/2), at least 1), rounds per apply / all-reduce
 * group (at least ~8 MB of user-factor differences per collective) and the number of rounds.  Every rank computes
 * the same values from job-wide counts; tests check it against yue_amd/dist.py: epoch_block_plan. */
int yue_epoch_plan(int64_t m, int k, int64_t round_events, double events_total, int nranks,
                   int64_t *user_block, int64_t *blocks_per_group, int64_t *n_blocks);

/* The default round size of yue_bpr_epoch for the uploaded factors on this device.  One resident set of waves of the
 * round kernel takes 57,344 events on MI355X at k = 128 (49,152 for the kernels that finish contended rows inside
 * the launch: option round_meta = 0, and yue_bpr_rounds); the default is up to 6 such sets, as long as
 * a round holds at most four events per item row of this rank (job-wide average on a communicator: the call is then
 * collective), at most 4 sets for rounds with fewer than two touches per item row -- 344,064 on BASELINE config 3,
 * 172,032 on config 2.  Results depend on the round size (DESIGN.md section 3 tabulates the distance from the
 * sequential loop against it): pass an explicit value where runs must be comparable across devices. */
int yue_default_round_events(yue_ctx *ctx, int64_t *out);

/* Negatives the device sampler draws for (seed, epoch): j_out[E], -1 where all attempts were rejected. */
int yue_sample_negatives(yue_ctx *ctx, uint64_t seed, uint32_t epoch, int32_t *j_out);

int yue_sumsq(yue_ctx *ctx, double *sumsqP_out, double *sumsqQ_out);

/* predict(user): scores of all n items in id order, fp32, k-ascending fused-multiply-add chain. */
int yue_scores(yue_ctx *ctx, int32_t user, float *out_n);

/*
 * evalRanking's selection for nu users.  Masked items per user come from mask_indptr[nu+1] /
 * mask_indices (rows sorted ascending, indexed by position in users[]); pass NULL for both to
 * mask the uploaded training items (evalRanking).  out_ids[nu*N], out_scores[nu*N], 1 <= N <= 100 (the
 * reference caps N at 100, :84-86).  Scores are the exact fp32 fma chain of yue_scores; for
 * k in {16,32,64,128} a bf16 MFMA tile pre-filters the pairs that can matter (same results).
 * Returns YUE_ERR_FEW_ITEMS if some user has fewer than N candidates (their rows are -1 / -inf).
 */
int yue_topn_scan(yue_ctx *ctx, const int32_t *users, int64_t nu, int N,
                  const int64_t *mask_indptr, const int32_t *mask_indices,
                  int32_t *out_ids, float *out_scores);

/* Timing of the dominant training kernel with HIP events on the library's stream: stride = 0 disables; any other
 * value brackets ALL round launches of each yue_bpr_epoch / yue_bpr_rounds call with one event pair (launch
 * boundaries and the interleaved user-row apply launches included).  yue_get_kernel_timing returns the summed
 * time, the round launches and the triplets inside the brackets since the last call. */
int yue_set_kernel_timing(yue_ctx *ctx, int stride);
int yue_get_kernel_timing(yue_ctx *ctx, double *total_ms, int64_t *launches_timed, int64_t *triplets_timed);
/* Last yue_topn_scan: time of its scoring kernel (HIP events), state-machine events, exact re-scores
 * done behind the bf16 pre-filter, and whether the bf16 pre-filter kernel ran (k in 16/32/64/128). */
int yue_get_scan_stats(yue_ctx *ctx, double *kernel_ms, int64_t *events, int64_t *rescored, int *used_bf16);
/* Last yue_topn_scan: 32-user x 32-item tiles the kernel actually scored, and the tiles of the full user x item product.  The
 * bf16 kernel skips a tile -- and stops a workgroup -- when a norm bound shows that none of its exact scores can reach any of the
 * users' thresholds (||P_u|| * max ||Q_i|| <= threshold; exact: the lists do not change). */
int yue_get_scan_work(yue_ctx *ctx, int64_t *tiles_scored, int64_t *tiles_total);

/* Tuning / diagnostic knobs (results do not depend on them, except that round_stage changes the order of some fp32 sums):
 *   "scan_f32"  1 = always score with the exact f32-MFMA kernel instead of bf16 pre-filter + exact re-score
 *   "scan_batch" bf16 scoring kernel: 0 (default) two item tiles per loop iteration and 256 users per workgroup, 1 one tile and 128 users
 *   "round_tpw" events per wave in the training round kernel: 0 = default (8 for k <= 128 -- 16 for k <= 64 in yue_bpr_rounds --, else 4), 2, 4, 8, 16 (k <= 64 only)
 *   "round_stage" 1 (default): item rows touched a few times in a round collect their differences in staging rows,
 *               summed in ticket / event order when the row is rewritten -- up to 4 touches in yue_bpr_rounds; in the
 *               epoch path up to a bound sized from the round's mean touches per item row (2x the mean at k > 64,
 *               4x at k <= 64, between 4 and 64; read it back as "round_last_stage_max"); 2..64: that bound chosen
 *               explicitly (epoch path); 0: every contended row goes through float atomics
 *   "round_meta" 1 (default): yue_bpr_epoch takes the touch metadata of all rounds from one pre-pass per epoch
 *               (k_round_meta), round launches without a retire phase (k_round_m) and a fold launch behind each
 *               (k_round_fold) -- item shards of up to 8.4M rows (above 454,656: touches bucketed by item range first); 0: touches counted and contended rows finished
 *               inside the round launches (k_round, the kernel of yue_bpr_rounds).  Also moves yue_default_round_events.
 *   "round_bucket" 1: the bucketed pre-pass also for small catalogues (tests)
 *   "fold_blocks" workgroups of the fold launch (default 1536)
 *   "scan_two_phase" 1 (default): yue_topn_scan on catalogues of >= 16,384 items (k in {16,32,64,128}, N <= 64, bf16 path) scores
 *               the first 512 items with the fused kernel and the rest in chunks through k_scan_filter + k_scan_select; 0: the
 *               fused kernel for everything (same lists and scores)
 *   "scan_growth" 0 (default): each chunk of the two-phase scan ends at 2x or 8x the items scanned so far, chosen from the
 *               list-update rate of the first 512 items; 2..64: that factor
 *   "scan_filter_ub" form of k_scan_filter: 3 (default) = two blocks of 32 users per wave in workgroups of four waves, item rows by
 *               LDS-DMA (k = 64 / 128; other k: as 2); 2 = the same blocking, rows staged through registers; 1 = one block per
 *               wave, eight waves (round 3).  Same lists and scores
 *   "scan_streams" 2 (default): calls of at least "scan_streams_min_users" users (262,144) split them into four or more slabs that
 *               alternate between two streams -- one slab's selection beside the next slab's filter; 1: one stream
 *   "fism_lds"   1 (default): yue_fism_rounds keeps a user's working rows in LDS when they fit (k_fism_round_lds); 0: always the
 *               form with working rows in global memory and host-built item lists
 *   "fism_inplace" 1 (default): in k_fism_round_lds a row only ONE user of the round touches goes back to the model in place
 *               (no second read of the round-start row, no atomic adds; the round in front counts the users per row);
 *               0: every row through the difference buffers
 *   "chain_waves" exact path: workgroups per CU of the dataflow launch, 1..8 (0 = default: 1; 2 with chain_xcd)
 *   "chain_split" exact path: 1 = a run is walked by a GROUP of five waves (k_bpr_chain3: two keep the memory side -- headers,
 *               prefetch rings, version checks, polling; even / odd triplets --, one the dependency chain margin -> sigmoid ->
 *               user row, two store the updated item rows; hand-over through LDS; same results bit for bit); 0 = by one wave
 *               (k_bpr_chain); -1 (default) = the group for streams of at least 16 triplets per run (BASELINE config 3: 940 ->
 *               607 ms per epoch), one wave otherwise (short runs: the group's hand-offs and run starts cost more than they save)
 *   "chain_fast"  exact path: 1 = the step's coefficient fp32(lr (1 - sigmoid(x))) in single precision and the margin as one
 *               64-lane sum -- the reference's ORDER of updates, not its last bit: factors within BASELINE.json's 1e-5 of the
 *               sequential loop (measured 3e-7..6e-7 on full configs 2, 3 and config 4's shard), 1.26e8 instead of 8.2e7 triplets/s
 *               on config 3; 0 (default) = every operation as the reference rounds it (bit-equal to the oracle)
 *   "chain_xcd"   exact path, wave group only: 1 = every working wave on ONE XCD (the other XCDs' workgroups leave at once), item rows
 *               handed over through that XCD's L2 instead of the memory side; same results; default 0
 *   "chain_ring"  exact path, wave group: triplets whose rows a loading wave keeps in flight, 8 (default) or 16 (k <= 128)
 *   "chain_spin"  exact path: polls a wave spends on one wait before it gives up with an error (0 = default: 2^22)
 *   "round_user_seq" epoch path on one GPU: 1 (default) = a wave owns a user and applies the user's triplets in the reference's
 *               order with P[u] in registers (k_round_u), only the item rows keep round semantics; 0 = user rows under round
 *               semantics too (k_round_m, differences through dP: the form a communicator always runs)
 *   "round_fast"  k_round_u: 1 (default) = the step's coefficient in single precision (as chain_fast); 0 = double precision
 *   "comm_group_mb" communicator: MB of user-factor differences per ncclAllReduce (groups of user blocks), 1..4096, default 8
 *               (what yue_epoch_plan announces); RCCL reaches its bus bandwidth at tens of MB
 *   "round_cus_reserved" CUs the compute stream leaves free (the stream is re-created with a CU mask) for RCCL's kernels beside
 *               round launches that otherwise fill the chip exactly; default 0
 * Behaviour switches:
 *   "epoch_exact" 1 = yue_bpr_epoch applies the epoch's triplets (device sampler's negatives) with the reference's exact
 *               sequential semantics (recommender/cf/BPR.py:42-58) instead of S-rounds: round_events is ignored, one GPU only
 *   "replay_levels" 1 = yue_bpr_replay by host-computed dependency levels, one launch per level (the round-1 path, kept for
 *               comparison; same results)
 * Read-only (yue_get_option): "chain_last_runs" / "chain_last_waves" (runs walked / waves launched by the last exact launch),
 *   "scan_last_few_users" (users of the last two-phase scan whose first 512 items held fewer than N candidates: they alone went
 *   through the fused kernel over all items), "chain_last_us" (HIP-event time of that launch alone, microseconds), "round_last_user_seq" (1: the last epoch ran k_round_u),
 *   "comm_last_compute_waits" (times the compute stream waited for the collective stream in the last epoch: 1),
 *   "replay_last_levels" (dependency levels of the last levelled replay), "scan_last_chunks" (filter + select launches of the
 *   last two-phase scan; 0: the fused kernel ran), "scan_last_settle" (1: most sampled users were settled against the catalogue's
 *   tail after the first chunk, the filter ran in the variant whose workgroups stop then), "round_last_stage_max" (largest staged block of the last epoch's pre-pass)
 * Behaviour switch (off by default = the reference's behaviour):
 *   "topn_true" 1 = yue_topn_scan returns a real top-N (descending, ties: lower item id first) instead of
 *               the reference's order-dependent overwrite-scan */
int yue_set_option(yue_ctx *ctx, const char *name, int64_t value);
/* Reads an option back; "round_path" = the kernels yue_bpr_epoch runs for the uploaded factors: 0 k_round,
 * 1 k_round_meta + k_round_m + k_round_fold. */
int yue_get_option(yue_ctx *ctx, const char *name, int64_t *value);

/*
 * FISM (reference recommender/cf/FISM.py) -- parity path: the reference's strictly
 * sequential epoch on the device, in the reference's types (item-history factors P float64 [n,k],
 * item factors Q float32 [n,k], item bias Bi float64 [n]).
 *   yue_fism_set_model / yue_fism_get_model   replace FISM.initModel's arrays (FISM.py:15-18) on / from the device
 *   yue_fism_epoch   replaces one pass of FISM.buildModel's loop (FISM.py:38-69): users in user_ptr order, users
 *                    with one event skipped; negs = the accepted negatives in processing order (rho per event,
 *                    drawn by the caller as FISM.py:50-53 does); coef[u] = pow(nu - 1, -alpha) (FISM.py:42).
 *                    Outputs: sum of 0.5*error^2 (:58) and {sum(P*P), sum(Q*Q), Bi.Bi} after the pass (:70).
 *   yue_fism_rounds  the throughput form of the same pass (ours; DESIGN.md section 10, oracle/numpy_fism.py: fism_rounds):
 *                    rounds of round_users consecutive users; every user of a round runs the reference's whole per-user
 *                    loop on the model as it was when the round started plus its own changes, the per-row differences of
 *                    the round's users are summed and added once.  round_users = 1 is yue_fism_epoch.  Same arguments
 *                    and outputs otherwise.  Read-only option "fism_last_form": the form the last call took -- 0 k_fism_round
 *                    (working rows in global memory), 1 k_fism_round_lds<KR, false>, 2 k_fism_round_lds<KR, true> (round-start
 *                    rows in LDS beside the working rows).
 *   Negatives (both calls): a draw whose negative equals its OWN event's item is refused with YUE_ERR_ARG (the message names
 *                    the draw) before anything is uploaded or changed: the reference rejects the user's items when it draws
 *                    (FISM.py:50-53) and cannot produce it, and the device forms would not follow the reference's sequential
 *                    update for it (Bi[i], then Bi[j] from the updated value; likewise Q).  A negative equal to ANOTHER item
 *                    of the same user is accepted and shares that item's row, as in the reference's arithmetic.
 *   yue_fism_scores  replaces FISM.predict (FISM.py:75-83) for a user whose training events are `items`.
 *   yue_fism_topn_scan  predict + the selection of base/IterativeRecommender.py:98-145 for nu users given as a
 *                    CSR of their training events (mask = those items).  YUE_ERR_FEW_ITEMS as yue_topn_scan.
 */
int yue_fism_set_model(yue_ctx *ctx, const double *P, const float *Q, const double *Bi, int64_t n, int k);
int yue_fism_get_model(yue_ctx *ctx, double *P, float *Q, double *Bi);
int yue_fism_epoch(yue_ctx *ctx, const int64_t *user_ptr, int64_t m, const int32_t *ev_i, const int32_t *negs, int64_t n_negs, int rho,
                   const double *coef, double lr, double regI, double regB, double *half_sq_out, double *sumsq3_out);
int yue_fism_rounds(yue_ctx *ctx, const int64_t *user_ptr, int64_t m, const int32_t *ev_i, const int32_t *negs, int64_t n_negs, int rho,
                    const double *coef, int64_t round_users, double lr, double regI, double regB, double *half_sq_out, double *sumsq3_out);
int yue_fism_scores(yue_ctx *ctx, const int32_t *items, int64_t n_items, double *out_n);
int yue_fism_topn_scan(yue_ctx *ctx, const int64_t *row_ptr, const int32_t *row_items, int64_t nu, int N, int32_t *out_ids, double *out_scores);

/*
 * WRMF (reference recommender/cf/WRMF.py; Hu, Koren and Volinsky's implicit-feedback MF) -- ALS half-sweeps on the
 * context's factors: X = P (users), Y = Q (items), as uploaded by yue_set_factors, so yue_scores / yue_topn_scan rank
 * with X and Y unchanged.  Needs 1 <= k <= 128 (larger k: YUE_ERR_ARG, nothing launched).
 *   yue_wrmf_set_pairs  the distinct (user, item) pairs both ways with their event counts r >= 1: user-major (u_ptr[m+1],
 *                    items ascending within a user) and item-major (i_ptr[n+1], users ascending), the transpose of each
 *                    other; sizes are those of yue_set_factors.  Builds the longest-row-first solve schedule and the
 *                    chunks of the long rows (option "wrmf_long_pairs", default 2048 pairs).
 *   yue_wrmf_half_sweep side 0: every X[u] from Y; side 1: every Y[i] from X.  Per row, over its pairs f_j with counts r_j:
 *                    A = fp32(F^T F) + sum alpha*r_j f_j f_j^T + reg*I,  b = sum (1 + alpha*r_j) f_j,  x = A^-1 b by an fp64
 *                    Cholesky factorisation, rounded to fp32 once; rows without pairs become 0.  loss_out (side 0, may be
 *                    NULL): sum over the pairs of (1 - x_old . y)^2, the dot rounded to fp32, the sum in fp64.  A
 *                    non-positive pivot returns YUE_ERR_ARG naming the (smallest such) row.  Bit-reproducible (no float
 *                    atomics).  Read-only options: "wrmf_last_ns" / "wrmf_last_long_ns" (device time of the last half-sweep /
 *                    of its long-row chunks), "wrmf_long_rows_user" / "wrmf_long_rows_item".
 */
int yue_wrmf_set_pairs(yue_ctx *ctx, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                       const int64_t *i_ptr, const int32_t *i_users, const int32_t *i_counts, int64_t nnz);
int yue_wrmf_half_sweep(yue_ctx *ctx, int side, double alpha, double reg, double *loss_out);

/*
 * ExpoMF (reference recommender/advanced/ExpoMF.py; Liang et al., "Modeling User Exposure in Recommendation") -- exposure-
 * weighted ALS on the context's factors: theta = P (users), beta = Q (items), so yue_scores / yue_topn_scan rank with
 * beta . theta[u] unchanged.  Needs 1 <= k <= 128 and m, n < 2^26 (otherwise YUE_ERR_ARG, nothing launched).
 *   yue_expo_set_pairs   the arguments and the upload of yue_wrmf_set_pairs (pairs both ways with counts, the longest-row-first
 *                        schedule, the long rows' chunks: option "wrmf_long_pairs"); the two solvers share that state.
 *   yue_expo_set_mu / yue_expo_get_mu   the exposure prior, one fp32 value per item, each inside (0, 1).
 *   yue_expo_half_sweep  side 0: every theta[u] from beta; side 1: every beta[i] from theta.  Per row r with old value x_r, over
 *                        every row f_j of the fixed side: s_j = x_r . f_j, pEX_j = sqrt(lam_y pi / 2) exp(-lam_y s_j^2 / 2),
 *                        A_j = (pEX_j + 1e-8) / (pEX_j + 1e-8 + (1 - mu) / mu), A_j = 1 on the row's pairs;
 *                        B = sum_j A_j f_j f_j^T + lam*I, a = sum over the pairs of r_j f_j, x = B^-1 a by an fp64 Cholesky
 *                        factorisation, rounded to fp32 once; rows without pairs become 0.  mu is taken per column j
 *                        (mu_per_column = 1: required on side 0, allowed on side 1 only when m == n, where the reference does
 *                        exactly that) or per row r (side 1).  The dense sum runs on the matrix cores in fp32
 *                        (v_mfma_f32_32x32x2_f32, exact fp32 products and sums) in row batches whose Gram workspace fits option
 *                        "expo_gram_mb" (default 512 MiB); the pairs' correction, lam*I, a and the solve are fp64.  A
 *                        non-positive pivot returns YUE_ERR_ARG naming the (smallest such) row.  Bit-reproducible (no float
 *                        atomics; every order of summation depends on the shapes only).
 *   yue_expo_update_mu   mu[i] = (a + A_sum[i] - 1) / (a + b + m - 2), A_sum[i] = sum over all users of A_ui from the current
 *                        theta, beta and mu (per item); the sums in fp64, mu rounded to fp32 once.
 * Read-only options: "expo_last_ns" / "expo_last_gram_ns" (device time of the last half-sweep or mu update / of its dense
 * Gram launches), "expo_last_batches".
 *   yue_expo_gram_rows   diagnostic, like those options: the dense stage of a half-sweep alone, for the tests.  For each of the
 *                        nrows listed rows r of the side (any order, repeats allowed) the packed lower triangle
 *                        out[t][p(p+1)/2 + q] (p >= q) of sum over ALL columns j of A~_j f_j f_j^T, A~ the posterior WITHOUT the
 *                        A = 1 overwrite on the pairs, no lam*I.  Runs the half-sweep's own Gram kernel with the pair-block
 *                        shape and the column splits of a half-sweep over all the side's rows; the list takes the place of the
 *                        schedule and the splits are summed in order in fp64, as the solve sums them.  Refuses what the
 *                        half-sweep refuses, and a list whose Grams exceed "expo_gram_mb".  Changes no factor.
 */
int yue_expo_set_pairs(yue_ctx *ctx, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                       const int64_t *i_ptr, const int32_t *i_users, const int32_t *i_counts, int64_t nnz);
int yue_expo_set_mu(yue_ctx *ctx, const float *mu, int64_t n);
int yue_expo_get_mu(yue_ctx *ctx, float *mu, int64_t n);
int yue_expo_half_sweep(yue_ctx *ctx, int side, double lam, double lam_y, int mu_per_column);
int yue_expo_update_mu(yue_ctx *ctx, double a, double b, double lam_y);
int yue_expo_gram_rows(yue_ctx *ctx, int side, int mu_per_column, double lam_y, const int32_t *rows, int64_t nrows, double *out);

/*
 * CoFactor (reference recommender/advanced/CoFactor.py; Liang et al., "Factorization Meets the Item Embedding") -- WRMF's ALS
 * with the items' shifted positive PMI factorised jointly.  The factors are X = P (users), Y = Q (items) of yue_set_factors, the
 * pairs those of yue_wrmf_set_pairs, the user sweep and the loss yue_wrmf_half_sweep(0, ...).  Needs 1 <= k <= 128.
 *   yue_cof_cooccur      the item x item co-occurrence counts as a symmetric CSR without diagonal: count(i, j) = common users;
 *                        items with fewer than `filter` training events (the sum of their counts) take no part, a pair is kept
 *                        when count > filter (filter >= 0).  Posting-list counting in passes over item ranges (option
 *                        "cof_pass_items", default 8192), integer atomics only, count then fill: exact and reproducible.  The
 *                        CSR is bounded by option "cof_cooccur_mb" (default 1024 MiB at 8 bytes per entry): beyond it the call
 *                        returns YUE_ERR_ARG naming the option and keeps nothing.  nnz_out: the number of entries.
 *   yue_cof_get_cooccur  ptr[n+1], idx ascending within a row, cnt (int32), as many entries as yue_cof_cooccur reported.
 *   yue_cof_set_sppmi    the contexts S_i of every item with their values s_ij: a symmetric CSR, rows ascending, no diagonal,
 *                        finite values (otherwise YUE_ERR_ARG, the previous SPPMI is kept).  Builds the level schedule:
 *                        level(i) = 1 + max(level(j): j in S_i, j < i), else 0.
 *   yue_cof_set_state / yue_cof_get_state   the context embeddings G [n][k], the item bias w [n] and the context bias c [n], fp64.
 *   yue_cof_item_sweep   the reference's sequential item sweep (items in id order, each reading the current rows of its
 *                        contexts), run level by level -- the rows of a level share no context edge, so the result is that of
 *                        the sequential sweep.  Per item i, every right-hand side before any write, contexts in ascending id:
 *                          Y[i] = (fp32(X^T X) + sum_u alpha r x_u x_u^T + regU I + sum_j G_j G_j^T)^-1
 *                                 (sum_u (1 + alpha r) x_u + sum_j (s_ij - w_i - c_j) G_j)                     rounded to fp32 once
 *                          G[i] = (sum_j Y_j Y_j^T + regR I)^-1 sum_j (s_ij - w_j - c_i) Y_j   (products of Y_j Y_j^T rounded to fp32)
 *                          w[i] = mean_j (s_ij - Y_i . G_j - c_j),   c[i] = mean_j (s_ij - Y_j . G_i - w_j)
 *                        the last three only where S_i is not empty; an item without pairs and without contexts becomes 0.
 *                        Both systems by an fp64 Cholesky factorisation.  A non-positive pivot returns YUE_ERR_ARG naming the
 *                        (smallest such) row.  Bit-reproducible (no float atomics).
 * Read-only options: "cof_last_ns" (device time of the last co-occurrence build or item sweep), "cof_last_small_ns" (of the
 * sweep's levels of fewer than 256 rows; measured only with option "cof_level_timing" = 1, which records an event per level), "cof_levels", "cof_cooccur_nnz".
 */
int yue_cof_cooccur(yue_ctx *ctx, int filter, int64_t *nnz_out);
int yue_cof_get_cooccur(yue_ctx *ctx, int64_t *ptr, int32_t *idx, int32_t *cnt);
int yue_cof_set_sppmi(yue_ctx *ctx, const int64_t *ptr, const int32_t *idx, const double *val_f64, int64_t nnz);
int yue_cof_set_state(yue_ctx *ctx, const double *G, const double *w, const double *c);
int yue_cof_get_state(yue_ctx *ctx, double *G, double *w, double *c);
int yue_cof_item_sweep(yue_ctx *ctx, double alpha, double regU, double regR);

/*
 * UserKNN (reference recommender/cf/UserKNN.py) -- exact user neighbours and neighbourhood ranking.  Needs no factors.
 * A_u is the set of distinct training items of user u; sim(u, v) = 2|A_u & A_v| / |A_u | A_v| (not Jaccard: in [0, 2]).
 *   yue_knn_set_pairs  the distinct (user, item) pairs both ways: user-major (u_ptr[m+1], items ascending within a user,
 *                    with their event counts >= 1) and item-major (i_ptr[n+1], users ascending), the transpose of each
 *                    other.  Needs n < 2^26 (similarities are ordered as exact integer ratios).
 *   yue_knn_neighbors  for every user the first K (1 <= K <= 256) other users with positive similarity by (sim descending,
 *                    user id ascending), as m x K arrays: neighbour id, |A_u & A_v|, |A_u | A_v|, padded with -1 / 0 / 0
 *                    behind the positive neighbours; any output may be NULL.  The lists stay on the device for the two
 *                    calls below.  No m x m matrix: per-row posting-list counting in passes of "knn_range" users.
 *   yue_knn_predict    the full ranked list of one user: every item some positive neighbour holds, score = sum_r sim_r *
 *                    count_r(i) / sum_r sim_r over the neighbours in rank order (fp64, no fused multiply-add), ordered by
 *                    (score descending, item ascending), the user's own items included.  Writes min(len, cap) entries;
 *                    *len_out = the full length.
 *   yue_knn_topn       the same lists for `users` without each user's own training items, cut at N (1 <= N <= 100): ids_out /
 *                    scores_out [nu][N] padded with -1 / 0, len_out[nu] the real lengths (a list may be shorter than N).
 *                    Neighbour sets of more than "knn_gather" entries are scored in item-range chunks.
 * Options: "knn_range" (64..4096, candidate users per counting pass), "knn_gather" (256..2048, entries per scoring chunk);
 * read-only "knn_last_ns" (device time of the last neighbours / topn / predict call), "knn_last_chunked_users".
 */
int yue_knn_set_pairs(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                      const int64_t *i_ptr, const int32_t *i_users, int64_t nnz);
int yue_knn_neighbors(yue_ctx *ctx, int K, int32_t *nbr_out, int32_t *inter_out, int32_t *union_out);
int yue_knn_predict(yue_ctx *ctx, int32_t user, int64_t cap, int32_t *items_out, double *scores_out, int64_t *len_out);
int yue_knn_topn(yue_ctx *ctx, const int32_t *users, int64_t nu, int N, int32_t *ids_out, double *scores_out, int32_t *len_out);

/*
 * IPF (reference recommender/cf/IPF.py) -- ranking by four typed 3-hop paths over the session temporal graph.  Needs no
 * factors.  UL[u] is u's training events in order (duplicates kept), S[u] = UL[u][-10:] its session.
 *   yue_ipf_set_graph  the graph and its weights, computed by the caller as the reference writes them:
 *                    u_ptr[m+1] / u_items   each user's distinct items of UL[u] in first-occurrence order (< 2^18 per user)
 *                    s_ptr[m+1] / s_items   each user's distinct items of S[u] in first-occurrence order
 *                    hu_ptr[n+1] / hu_users item -> its distinct users in listened (insertion) order; pos = index in the row
 *                    hs_ptr[n+1] / hs_users / hs_pos  item -> the distinct users whose session holds it, in user order, with
 *                                           each one's first position in the list that keeps duplicates (< 2^26)
 *                    w_user[m] = 1/L^rho, w_sess[m] = 1/min(10, L)^rho, p_i2u[n] = (eta/(eta nU + nS))^rho,
 *                    p_i2s[n] = (1/(eta nU + nS))^rho; r_user = beta, r_sess = 1 - beta.  Needs m, n < 2^26.
 *   yue_ipf_predict    the full list of one user: every item some path reaches, score = the fp64 sum over the paths in order,
 *                    ordered by (score descending, first insertion ascending), the user's own items included.  Writes
 *                    min(len, cap) entries; *len_out = the full length.
 *   yue_ipf_topn       the same lists for `users` without each user's own training items, cut at N (1 <= N <= 100): ids_out /
 *                    scores_out [nu][N] padded with -1 / 0, len_out[nu] the real lengths (a list may be shorter than N).
 * Options: "ipf_slots" (1..4096, queries in flight per launch, default 1024, capped so that the work arrays stay within
 * 4 GiB); read-only "ipf_last_ns" (device time of the last predict / topn launch).
 */
int yue_ipf_set_graph(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int64_t *s_ptr,
                      const int32_t *s_items, const int64_t *hu_ptr, const int32_t *hu_users, const int64_t *hs_ptr,
                      const int32_t *hs_users, const int32_t *hs_pos, const double *w_user, const double *w_sess,
                      const double *p_i2u, const double *p_i2s, double r_user, double r_sess);
int yue_ipf_predict(yue_ctx *ctx, int32_t user, int64_t cap, int32_t *items_out, double *scores_out, int64_t *len_out);
int yue_ipf_topn(yue_ctx *ctx, const int32_t *users, int64_t nu, int N, int32_t *ids_out, double *scores_out, int32_t *len_out);

/*
 * CUNE's user-network stage (reference recommender/advanced/CUNE.py:34-118) -- collaborative user network, random walks,
 * CBOW user embedding, cosine top-K friends.  Needs no factors.  Contract: tests/helpers/numpy_cune_net.py, DESIGN.md 18.
 * Every random number is cnet_hash(seed ^ tag, a, b, c, d) (csrc/counter_hash.hpp: the mix64 chain of the BPR sampler).
 *   yue_cnet_set_pairs     the distinct (user, item) pairs both ways, as yue_knn_set_pairs takes them (no counts).  The
 *                        network CUNet[a] = every other user b repeated |items(a) & items(b)| times is never built: entry
 *                        r of it is found from the prefix sums of deg(item) - 1 over a's item row.  A user whose total is 0
 *                        is not in the network: no walks, no embedding row, no friends.
 *   yue_cnet_walks         T walks of length L (2 <= L <= 64, T (L - 1) <= 15360) from every network user, one wave per
 *                        start user; draw (start, t, step, attempt) picks entry mulhi(hash, total) of CUNet[last].  Up to
 *                        10 re-draws while the candidate is in visited[start] (:64-69) -- consulted only where the walk
 *                        stands on its start user; for any other node the set counts as empty (the reference reads there
 *                        what walks from that node have stored so far, which depends on dict order: stated deviation).
 *                        The walks (user ascending, t ascending) are stored in the order of (hash(seed ^ shuffle, walk),
 *                        walk) -- shuffle(self.walks), :74 -- and stay on the device.  walks_out [nw][L] may be NULL.
 *   yue_cnet_set_walks     uploads walks of the caller's (ids below m) in training order instead.
 *   yue_cnet_set_sentences uploads ns sentences of unequal length instead (ptr[ns + 1] from 0 to the words, ids below m; Song2vec:
 *                        ids are tracks, a sentence is a user's play list).  yue_cnet_embed cuts every sentence into
 *                        consecutive segments of at most S words, the last one shorter; S is the largest value <= 64 for
 *                        which S (negative + 2) rows of dim floats fit 60 KiB (S = 64 at dim 20, 34 at dim 64, 17 at dim 128
 *                        with 5 negatives); S < 2 window + 1 is refused.  A segment is trained as a walk of its own length:
 *                        windows do not cross a cut (stated deviation: gensim cuts sentences at 10,000 words only).  Alpha
 *                        runs over the words passed (the words of the segments before); counts, subsampling thresholds and
 *                        the negative table run over the real words.  Sentences that all have one length L <= S give the
 *                        embedding of the same rows as walks, bit for bit.
 *   yue_cnet_embed         Word2Vec(walks, size=dim, window, min_count=0, iter=epochs) as gensim documents it, with this
 *                        stream: CBOW with the mean of the context, `negative` negatives from the unigram^0.75 table of the
 *                        walks' user counts (a draw equal to the word is skipped), window shrink b uniform in [0, window)
 *                        per position, subsampling at 1e-3, alpha from 0.025 to 1e-4 linear in the words passed (one value
 *                        per walk), no update where |logit| >= 6, syn0 = (U - 0.5) / dim, syn1neg = 0; float32.  A round
 *                        is round_walks consecutive walks (0: the default, 64): each walk reads the rows as the round began
 *                        plus its own changes; its row differences are rounded to multiples of 2^-36 and summed as 64-bit
 *                        integers (order-free), then row = fp32(fp64(row) + sum 2^-36).  Bit-reproducible; round_walks = 1
 *                        is the sequential algorithm.  1 <= dim <= 128; L (negative + 2) rows of dim floats must fit
 *                        60 KiB.  W_out [m][dim] (may be NULL): rows of users outside the walks are 0.
 *   yue_cnet_set_embedding uploads an embedding of the caller's; `users` (ascending, or NULL: all m) have rows.
 *   yue_cnet_friends       for every user with a row the K (1 <= K <= 100) others with the largest cosine(W[a], W[b]) =
 *                        dot / sqrt(n_a n_b), dots and norms in fp64 over the float32 values (tool/qmath.py:36-45; 0 where
 *                        a norm is 0, the reference's ZeroDivisionError branch), by (cosine descending, id ascending).
 *                        friends_out [m][K] padded with -1, sims_out [m][K] padded with 0; either may be NULL.
 * Read-only option "cnet_last_ns": device time of the last walks / embed / friends call.
 */
int yue_cnet_set_pairs(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int64_t *i_ptr,
                       const int32_t *i_users, int64_t nnz);
int yue_cnet_walks(yue_ctx *ctx, int T, int L, uint64_t seed, int32_t *walks_out, int64_t *nw_out);
int yue_cnet_set_walks(yue_ctx *ctx, int64_t m, int64_t nw, int L, const int32_t *walks);
int yue_cnet_set_sentences(yue_ctx *ctx, int64_t m, int64_t ns, const int64_t *ptr, const int32_t *ids);
int yue_cnet_embed(yue_ctx *ctx, int dim, int window, int epochs, int negative, int64_t round_walks, uint64_t seed, float *W_out);
int yue_cnet_set_embedding(yue_ctx *ctx, int64_t m, int dim, const float *W, const int32_t *users, int64_t nu);
int yue_cnet_friends(yue_ctx *ctx, int K, int32_t *friends_out, double *sims_out);

/*
 * Song2vec's iteration (reference recommender/advanced/Song2vec.py:162-189) -- a biased matrix factorisation by sequential
 * SGD over (user, item, count) steps, then a similarity regulariser over (track, similar track) pairs.  The factors are
 * X = P (users), Y = Q (items) of yue_set_factors (float32, k <= 128); the embedding and the similar tracks come from
 * yue_cnet_set_sentences / yue_cnet_embed / yue_cnet_friends.  Contract: tests/helpers/numpy_song2vec.py, DESIGN.md 19.
 *   yue_s2v_set_state / yue_s2v_get_state   the biases Bu [m], Bi [n], fp64.
 *   yue_s2v_set_steps   the rating steps in the reference's order (users in id order, a user's items in first-listen order,
 *                       count = the user's events of the item).  A user's steps must be contiguous, otherwise the call is
 *                       refused: the reference reads bu = Bu[u] once per user, and every step of the user uses that value in
 *                       its regulariser.  Builds the dependency schedule.
 *   yue_s2v_set_pairs   the similarity pairs in visiting order, sim in fp64 (rounded to float32 where NumPy rounds it: it
 *                       meets a float32 dot).  t1 == t2 is refused.  Builds the dependency schedule.
 *   yue_s2v_epoch       one iteration: the rating pass, then the pair pass (the arithmetic, call by call as NumPy 2 rounds
 *                       it: csrc/s2v_kernels.hpp).  err2_steps [T] and err2_pairs [Pn] (either may be NULL) take the squared
 *                       error of every step and pair, so that the caller adds them in the reference's order and composes the
 *                       loss of :190 itself.
 * Schedule: level(step) = 1 + max(level of the previous step of the same user, ... of the same item); for pairs, of either
 * track.  Two steps of a level share no row and every step finds what the sequential loop would hand it, so one launch per
 * level with one wave per step gives the sequential loop's result bit for bit, without atomics.  Option "s2v_schedule":
 * 1 = levels (default), 0 = one wave walks all steps in order in one launch (the yardstick).  Read-only options
 * "s2v_levels_steps", "s2v_levels_pairs" (launches per pass) and "s2v_last_ns" (device time of the last yue_s2v_epoch).
 */
int yue_s2v_set_state(yue_ctx *ctx, const double *Bu, const double *Bi);
int yue_s2v_get_state(yue_ctx *ctx, double *Bu, double *Bi);
int yue_s2v_set_steps(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *count, int64_t T);
int yue_s2v_set_pairs(yue_ctx *ctx, const int32_t *t1, const int32_t *t2, const double *sim, int64_t Pn);
int yue_s2v_epoch(yue_ctx *ctx, double lr, double regU, double regI, double regB, double alpha, double globalMean, double *err2_steps,
                  double *err2_pairs);

/*
 * LightGCN (reference recommender/advanced/LightGCN.py) -- embeddings propagated over the user-item graph, trained by Adam on
 * a pairwise loss.  U = P, V = Q of yue_set_factors (float32, k <= 128); Adam's moments are those of yue_adam_step
 * (yue_adam_reset clears them).  Contract: tests/helpers/numpy_lightgcn.py, DESIGN.md 20.  Parity with TensorFlow unpinned.
 *   A  [(m + n)^2], symmetric: A[u][m + i] = A[m + i][u] = the pair's weight (the reference's is the squared event count).
 *   E_0 = [U; V], E_l = A E_{l-1}, F = E_0 + sum_{l = 1..layers} E_l * rsqrt(max(|E_l row|^2, 1e-12)).
 *   loss = sum_t -log sigmoid(F_u.F_i - F_u.F_j) + reg / 2 (|F_u|^2 + |F_i|^2 + |F_j|^2) over the T triplets.
 *   yue_lgcn_set_graph   both sides of the pair list: u_ptr [m + 1] / u_items / u_w and i_ptr [n + 1] / i_users / i_w, ids sorted
 *                        and unique within a row.  Ids, order and symmetry (same pairs, same weights) are checked before
 *                        anything is stored; a refused call leaves the previous graph in place.
 *   yue_lgcn_propagate   raw_layers_out [layers][m + n][k] (E_1 .. E_layers, may be NULL), F_out [m + n][k] (may be NULL).
 *   yue_lgcn_grad        loss and dLoss / dU [m][k], dLoss / dV [n][k] of one minibatch, no step (outputs may be NULL).
 *   yue_lgcn_step        the same, then dense Adam (beta 0.9 / 0.999, eps 1e-8, lr_t of `step` = 1, 2, ...) on U and V.
 * Refused with YUE_ERR_ARG: k > 128, layers < 1 (or > 64), T < 1, an id out of range, no graph, a graph set for another m, n.
 * Every sum has a fixed order and no atomic is used: two calls on the same input return the same bits.  Option "lgcn_hub"
 * (default 1024): rows with more neighbours are cut into parts of that many, one wave per part, combined in ascending order.
 * Read-only options "lgcn_last_hubs", "lgcn_last_parts", "lgcn_last_forward_ns", "lgcn_last_batch_ns",
 * "lgcn_last_backward_ns", "lgcn_last_adam_ns" (device time of the last call's phases).
 */
int yue_lgcn_set_graph(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const float *u_w, const int64_t *i_ptr,
                       const int32_t *i_users, const float *i_w);
int yue_lgcn_propagate(yue_ctx *ctx, int layers, float *raw_layers_out, float *F_out);
int yue_lgcn_grad(yue_ctx *ctx, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out,
                  float *gU_out, float *gV_out);
int yue_lgcn_step(yue_ctx *ctx, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double reg, int64_t step,
                  double *loss_out);

/* NGCF (reference recommender/advanced/NGCF.py).  U [m][k] and V [n][k] are the factors of
 * yue_set_factors; the Adam moments of U and V are those of yue_adam_step (yue_adam_reset clears them).  With N = m + n:
 *   A  [N][N], a general CSR (the reference's graph is not symmetric as written); the transpose is built on the host.
 *   Per layer l = 0 .. layers-1, E_0 = [U; V]:  S = A E;  Z = (S + E) W_l_1 + (E o S) W_l_2;  H = Z > 0 ? Z : 0.2 Z;
 *   D = training ? H / keep where the mask keeps the element, 0 elsewhere : H;  E_{l+1} = D;  N_{l+1} = D * rsqrt(max(|D row|^2, 1e-12)).
 *   F = [E_0 | N_1 | .. | N_layers], (layers + 1) k wide.  The loss is yue_lgcn_grad's on F.
 *   The mask keeps element (row, column) of layer l when the top 24 bits of hash(seed ^ 0x4E474346, step, l, row, column) lie
 *   below floor(keep * 2^24); the hash is the user-network stage's counter hash.  It is recomputed in the backward pass.
 *   yue_ngcf_set_graph    ptr [N + 1], col, w: columns ascending and unique within a row and below N, finite weights; checked
 *                         before anything is stored (a refused call leaves the previous graph in place).
 *   yue_ngcf_set_weights  W [layers][2][k][k] (W_l_1 then W_l_2, input index major); clears the weights' Adam moments.
 *   yue_ngcf_get_weights  W and, where asked for, the weights' moments (any pointer may be NULL).
 *   yue_ngcf_propagate    S_out, Z_out, D_out [layers][N][k], F_out [N][(layers + 1) k] (any may be NULL).
 *   yue_ngcf_grad         loss, dLoss / dU [m][k], dLoss / dV [n][k], dLoss / dW [layers][2][k][k]; no step (outputs may be NULL).
 *   yue_ngcf_step         the same, then dense Adam (beta 0.9 / 0.999, eps 1e-8, lr_t of `step` = 1, 2, ...) on U, V and the
 *                         weights; the mask is that of `step`.
 * Refused with YUE_ERR_ARG: k > 128, (layers + 1) k > 256, layers < 1, keep outside (0, 1], T < 1, an id out of range, no graph or
 * no weights, a graph or weights set for other shapes.
 * Every sum has a fixed order and no atomic is used: two calls on the same input return the same bits.  The weight gradients
 * are summed over chunks of 512 rows in ascending order.  Option "ngcf_hub" (default 1024) as "lgcn_hub", for A and its
 * transpose.  Read-only options "ngcf_last_hubs", "ngcf_last_parts" (both matrices together), "ngcf_last_gather_ns",
 * "ngcf_last_dense_ns", "ngcf_last_batch_ns", "ngcf_last_backward_ns", "ngcf_last_wgrad_ns", "ngcf_last_adam_ns".
 */
int yue_ngcf_set_graph(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *ptr, const int32_t *col, const float *w);
int yue_ngcf_set_weights(yue_ctx *ctx, int layers, int k, const float *W);
int yue_ngcf_get_weights(yue_ctx *ctx, float *W, float *mW, float *vW);
int yue_ngcf_propagate(yue_ctx *ctx, int layers, int training, double keep, uint64_t seed, int64_t step, float *S_out, float *Z_out, float *D_out,
                       float *F_out);
int yue_ngcf_grad(yue_ctx *ctx, int layers, int training, double keep, uint64_t seed, int64_t step, const int32_t *u, const int32_t *i,
                  const int32_t *j, int64_t T, double reg, double *loss_out, float *gU_out, float *gV_out, float *gW_out);
int yue_ngcf_step(yue_ctx *ctx, int layers, int training, double keep, uint64_t seed, const int32_t *u, const int32_t *i, const int32_t *j,
                  int64_t T, double lr, double reg, int64_t step, double *loss_out);

/* CDAE (reference recommender/advanced/CDAE.py): a denoising autoencoder over the item axis, worked as
 * sparse-in / sampled-out.  The five variables live in a state of their own (not the factors of yue_set_factors): U [m][h],
 * encoder W [n][h], decoder W' [h][n] (kept transposed on the device), b [h], b' [n], each with Adam moments.
 *   A batch is B slots: users[B] (a user may repeat) and per slot the sampled items as a CSR (sample_ptr [B + 1], sample_items
 *   ascending and distinct within a slot).  The input row of a slot holds the user's event counts c at the user's items.
 *   Input entry (slot, item) of `step` is KEPT when the top 24 bits of hash(seed ^ 0x43444145, step, slot, item, 0) lie below
 *   floor(co * 2^24); the hash is the user-network stage's counter hash.
 *   hid = sigmoid(sum over kept entries of c W[item] + b + U[u]);  logit = hid . W'[:, item] + b'[item] at the sampled entries;
 *   y_pred = max(1e-6, sigmoid(logit));  y_true = c where the item is a kept input entry of the slot, else 0.
 *   loss = (sum over sampled entries of -y_true log y_pred - (1 - y_true) log(1 - y_pred) + (B n - entries) * -log(1 - 1e-6))
 *          / (B n) + reg / 2 (|W|^2 + |W'|^2 + |b|^2 + |b'|^2 + sum over slots |U[u]|^2).
 *   yue_cdae_set_data     the user CSR: ptr [m + 1], items ascending and distinct within a user, counts >= 1.
 *   yue_cdae_set_params   U, W, W' [h][n], b, b' for the data's m and n; clears the moments.
 *   yue_cdae_get_params   params / m_out / v_out: each NULL or five pointers (U, W, W' [h][n], b, b'; any may be NULL).
 *   yue_cdae_forward      hid_out [B][h], kept_out (one flag per input entry, slot by slot in the user's item order),
 *                         logit_out and ypred_out per sampled entry, the loss (any output may be NULL).
 *   yue_cdae_grad         the loss and the five gradients, dense, in the shapes of set_params; no step (outputs may be NULL).
 *                         A sampled entry whose y_pred equals 1.0f is counted, makes the loss inf and contributes no gradient.
 *   yue_cdae_step         the same gradients, then Adam (beta 0.9 / 0.999, eps 1e-8, lr_t of `step` = 1, 2, ...) on EVERY row of
 *                         all five variables (TF-1 applies Adam densely: moments decay and rows move with a zero gradient).
 *                         When a sampled y_pred equals 1.0f the loss is returned as inf, nothing is updated and the call
 *                         returns YUE_ERR_SATURATED (option "cdae_last_saturated": how many).
 *   yue_cdae_load_factors encodes all m users with a mask of ones and fills the context's factor matrices on the device with
 *                         P[u] = [hid(u) | 1], Q[i] = [W'[:, i] | b'[i]] (k = h + 1), as yue_set_factors would: yue_scores,
 *                         yue_topn_scan and yue_get_factors then serve the decoder's logits (upload the interactions again).
 *   yue_cdae_times        ns_out [4]: device time of the last call's encode, decode, regroup and adam phases.
 * Refused with YUE_ERR_ARG before any launch: h outside 1 .. 128, B < 1, an id out of range, a slot's items not ascending and
 * distinct, co outside (0, 1], no data or no parameters.  Every sum has a fixed order (items ascending, slots ascending) and no
 * atomic is used: two calls on the same input return the same bits.  Option "cdae_hub" (default 1024, inherited from "lgcn_hub"):
 * encoder rows and regrouped segments with more entries are cut into parts of that many, one wave per part, combined in
 * ascending order.  Read-only options "cdae_last_hubs", "cdae_last_parts", "cdae_last_saturated".
 */
int yue_cdae_set_data(yue_ctx *ctx, int64_t m, int64_t n, const int64_t *ptr, const int32_t *items, const int32_t *counts);
int yue_cdae_set_params(yue_ctx *ctx, int h, const float *U, const float *W, const float *Wd, const float *b, const float *bd);
int yue_cdae_get_params(yue_ctx *ctx, float *const *params, float *const *m_out, float *const *v_out);
int yue_cdae_forward(yue_ctx *ctx, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                     int64_t step, double reg, float *hid_out, int32_t *kept_out, float *logit_out, float *ypred_out, double *loss_out);
int yue_cdae_grad(yue_ctx *ctx, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                  int64_t step, double reg, double *loss_out, float *gU_out, float *gW_out, float *gWd_out, float *gb_out, float *gbd_out);
int yue_cdae_step(yue_ctx *ctx, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                  double lr, double reg, int64_t step, double *loss_out);
int yue_cdae_load_factors(yue_ctx *ctx);
int yue_cdae_times(yue_ctx *ctx, int64_t *ns_out);

/* APR (reference recommender/advanced/APR.py): declared in a header of its own, which sees the types above. */
#include "yue_apr.h"

/* Multi-GPU (one process per GPU, RCCL over xGMI).  Rank 0 creates the id, the caller ships
 * the 128 bytes to the other ranks (any side channel), every rank calls yue_comm_init. */
int yue_comm_unique_id(void *id128_out);
int yue_comm_init(yue_ctx *ctx, const void *id128, int rank, int nranks);
/* Sum a double across ranks (loss terms); identity without a communicator. */
int yue_allreduce_f64(yue_ctx *ctx, double *vals, int count);
/* The last yue_bpr_epoch on a communicator: bytes this rank handed to ncclAllReduce (user-factor differences, fp32), the
 * number of collectives, the time the compute stream had to wait for the second stream (all-reduce + apply of the last
 * group) after its own last round launch had finished (HIP events), the communicator's rank count as RCCL reports it and
 * the RCCL version (ncclGetVersion).  Zeros / 1 without a communicator. */
int yue_get_comm_stats(yue_ctx *ctx, double *allreduce_bytes, int64_t *collectives, double *wait_ms, int *nranks, int *rccl_version);

#ifdef __cplusplus
}
#endif
#endif
