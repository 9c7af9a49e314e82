/* libyue_hip.so -- the C ABI of APR.  Included by yue_hip.h, inside its extern "C" block and after its typedef of yue_ctx and
 * its status codes; not meant to be included alone.  Python binding: APR_SIGNATURES of yue_amd/_shim.py
 * (tests/test_apr_signatures.py holds that table against this file type by type). */
#ifndef YUE_APR_H
#define YUE_APR_H

/* APR (reference recommender/advanced/APR.py): BPR's live minibatch path (yue_adam_step) with an adversarial
 * perturbation D of the embeddings.  U [m][k] and V [n][k] are the factors of yue_set_factors (k <= 256); Adam's moments are those
 * of yue_adam_step (yue_adam_reset clears them), so the step count runs on from phase 1 into phase 2.  Contract:
 * tests/helpers/numpy_apr.py.  Parity with TensorFlow unpinned.  With x = U_u.V_i - U_u.V_j over the T triplets (u, i, j) and
 * x_adv the same on U + D_U, V + D_V:
 *   phase 1       loss = sum softplus(-x) + reg / 2 (2 |U_u|^2 + |V_i|^2) per triplet: the user rows are regularised twice, the
 *                 negative rows not at all (APR.py:61-67)
 *   adversarial   loss_adv = sum softplus(-x) + regA sum softplus(-x_adv), no l2 term
 * The perturbation is kept compact: the distinct rows of the batch that set it.  Every other row is 0, which is what the
 * reference's whole-variable assign leaves behind.
 *   yue_apr_reset         clears the perturbation.
 *   yue_apr_pre_step      one phase-1 step: gradient of the phase-1 loss, then dense Adam (lr_t of `step` = 1, 2, ...) on U and V.
 *   yue_apr_adv_step      one phase-2 step: yue_apr_delta_update's work, then the gradient of loss_adv with respect to U and V at the
 *                         new perturbation and dense Adam.  loss_out = loss_adv at the new perturbation, before the step.
 *   yue_apr_set_delta     for tests: the perturbation's rows -- users ascending and distinct with rows_u [n_users][k], items
 *                         likewise with rows_v [n_items][k]; every other row is 0.
 *   yue_apr_get_delta     for tests: the perturbation, dense: dU_out [m][k], dV_out [n][k] (either may be NULL).
 *   yue_apr_delta_update  for tests, the first half of a phase-2 step alone: g = d loss_adv / d (D_U, D_V) at the standing
 *                         perturbation, returned dense (gU_raw_out [m][k], gV_raw_out [n][k], either may be NULL), then
 *                         D <- g * rsqrt(max(|g row|^2, 1e-12)) * eps on the batch's distinct rows and 0 on every other row.
 *   yue_apr_grad          for tests: the loss and its gradient with respect to U and V, dense (outputs may be NULL), no step.
 *                         adversarial = 0: the phase-1 loss with `reg`; 1: loss_adv at the standing perturbation with regA = `reg`.
 *   yue_apr_times         ns_out [4]: device time of the last call's coefficient, parameter-row, perturbation-row (gradient and
 *                         normalisation) and adam phases.
 * Refused with YUE_ERR_ARG before any launch: no factors, T < 1, an id out of range, step < 1, eps < 0, reg or regA < 0.  i == j is
 * accepted: its terms cancel exactly.  Every sum has a fixed order (a row's terms in triplet order, the positive role before the
 * negative one; the loss in triplet order in double) and no atomic is used: two calls on the same input return the same bits.
 * Read-only option "apr_last_longest_row": the longest list of terms one wave added in the last batch.
 */
int yue_apr_reset(yue_ctx *ctx);
int yue_apr_pre_step(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double reg, int64_t step, double *loss_out);
int yue_apr_adv_step(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double eps, double regA, int64_t step,
                     double *loss_out);
int yue_apr_set_delta(yue_ctx *ctx, const int32_t *users, int64_t n_users, const float *rows_u, const int32_t *items, int64_t n_items, const float *rows_v);
int yue_apr_get_delta(yue_ctx *ctx, float *dU_out, float *dV_out);
int yue_apr_delta_update(yue_ctx *ctx, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double eps, double regA, float *gU_raw_out,
                         float *gV_raw_out);
int yue_apr_grad(yue_ctx *ctx, int adversarial, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out,
                 float *gU_out, float *gV_out);
int yue_apr_times(yue_ctx *ctx, int64_t *ns_out);

#endif
