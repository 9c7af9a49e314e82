// Host side of libyue_hip.so, shared by its translation units: the opaque context (device buffers, streams, options),
// error plumbing, and the few helpers more than one subsystem uses.  The C ABI is include/yue_hip.h.
//   core_host.hip   context, factors, interactions            bpr_host.hip   replay levels, S-rounds, epochs, CUNE, Adam, kernel timing
//   chain_host.hip  exact sequential semantics as dataflow    scan_host.hip  predict + evalRanking's selection, scan statistics
//   fism_host.hip   FISM                                      comm.hip       RCCL
//   options_host.hip  yue_get_option / yue_set_option: one table row per option, every subsystem's included (no device code)
//   wrmf_host.hip   WRMF (ALS half-sweeps)                     knn_host.hip   UserKNN (neighbours, ranking)
//   ipf_host.hip    IPF (session-graph ranking)                expo_host.hip  ExpoMF (exposure-weighted ALS, MFMA Gram)
//   cof_host.hip    CoFactor (co-occurrence, level-scheduled item sweep)
//   cnet_host.hip   CUNE's user-network stage (walks, embedding, friends); Song2vec's track embedding (sentences)
//   s2v_host.hip    Song2vec's iteration (level-scheduled rating steps and similarity pairs)
//   lgcn_host.hip   LightGCN (graph propagation forward and backward, minibatch, Adam step)
//   ngcf_host.hip   NGCF (weighted graph convolution: gather, MFMA layers forward and backward, weight gradients, Adam step)
//   cdae_host.hip   CDAE (sparse encoder, sampled decoder, gradients regrouped by item, dense Adam on five variables)
//   apr_host.hip    APR (pairwise minibatch gradient in fixed order, compact adversarial perturbation, Adam step)
//   gcn_host.hpp    what those two share (header only): the graph on the device and its hub parts, a product's launches, the
//                   minibatch, the phase timer
//   input_checks.hpp  what a caller uploads as row lists, checked before a kernel indexes with it (header only, no HIP call):
//                   check_rows (the whole pointer, then the ids), check_transpose, check_ids, and fail()'s declaration
// Ownership: every device allocation is a DevBuf, every event an Event, every subsystem's state a StatePtr
// member of the context made by state(); each frees itself with its owner, so yue_ctx_destroy ends in `delete c` and no unit
// keeps a list of things to release.  The raw HIP calls for both stand in this header and nowhere else, as do upload / download
// (blocking copies into and out of a DevBuf) and elapsed (the time between two events) -- tests/test_host_ownership.py.
#pragma once
#include "../../include/yue_hip.h"
#include "input_checks.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

struct ncclComm;
struct yue_wrmf;                                     // wrmf_host.hip: pairs, schedules, workspaces of the WRMF half-sweeps
struct yue_knn;                                      // knn_host.hip: pair lists, neighbour lists, ranking buffers of UserKNN
struct yue_expo;                                     // expo_host.hip: mu, Gram workspace, partial sums of ExpoMF
struct yue_cof;                                      // cof_host.hip: co-occurrence CSR, SPPMI, level schedule, G / w / c of CoFactor
struct yue_cnet;                                     // cnet_host.hip: pairs, walks, embedding, friends of CUNE's user-network stage
struct yue_s2v;                                      // s2v_host.hip: biases, steps, pairs and their level schedules of Song2vec's iteration
struct yue_lgcn;                                     // lgcn_host.hip: the graph (gcn_host.hpp), layers and gradients of LightGCN
struct yue_ngcf;                                     // ngcf_host.hip: the graph and its transpose (gcn_host.hpp), weights, layers and gradients of NGCF
struct yue_cdae;                                     // cdae_host.hip: user CSR, the five variables with their moments, the batch's index arrays of CDAE
struct yue_apr;                                      // apr_host.hip: the compact perturbation and the batch's index arrays of APR
struct yue_ipf;                                      // ipf_host.hip: session temporal graph, weights, per-slot work arrays of IPF

namespace yue_host {

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return yue_host::fail(YUE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// One device allocation, freed with its owner (move-only; an empty one makes no HIP call, also not when it is destroyed).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t resize(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; n = 0; if (e != hipSuccess) return e; }
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// blocking copies of `count` elements: up into a buffer that holds max(count, 1), so that its pointer is never null
// afterwards; down only where the caller wants them (dst may be null)
template <typename T>
int upload(DevBuf<T> &buf, const T *src, int64_t count) {
    HIPCHK(buf.resize((size_t)std::max<int64_t>(count, 1)));
    if (count > 0) HIPCHK(hipMemcpy(buf.p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
    return YUE_OK;
}
template <typename T>
int upload(DevBuf<T> &buf, const std::vector<T> &src) { return upload(buf, src.data(), (int64_t)src.size()); }
template <typename T>
int download(T *dst, const DevBuf<T> &src, size_t count) {
    if (dst && count > 0) HIPCHK(hipMemcpy(dst, src.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return YUE_OK;
}

// One event, destroyed with its owner (move-only, so that a std::vector of them works).  record() creates it the first time;
// an event something may wait for before its first record (the context's ev_rounds / ev_comm) is created by name.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    hipError_t record(hipStream_t s) {
        const hipError_t rc = create();
        return rc != hipSuccess ? rc : hipEventRecord(e, s);
    }
    operator hipEvent_t() const { return e; }
};

// The time between two recorded events whose stream has been waited for: in milliseconds as a double (for sums of several
// intervals, converted once), or in nanoseconds as every *_ns field holds one interval.
inline hipError_t elapsed(hipEvent_t from, hipEvent_t to, double *ms) {
    float f = 0.0f;
    const hipError_t rc = hipEventElapsedTime(&f, from, to);
    if (rc == hipSuccess) *ms = (double)f;
    return rc;
}
inline int64_t ns_of(double ms) { return (int64_t)(1e6 * ms); }
inline hipError_t elapsed(hipEvent_t from, hipEvent_t to, int64_t *ns) {
    double ms = 0.0;
    const hipError_t rc = elapsed(from, to, &ms);
    if (rc == hipSuccess) *ns = ns_of(ms);
    return rc;
}

constexpr int kNllSlotsHost = 1024;   // == yue::kNllSlots (bpr_device.hpp; checked where both are visible)
constexpr int kHeaderSlackHost = 16;  // == yue::kHeaderSlack (round_kernels.hpp)
constexpr int kMetaStageMaxHost = 64; // == yue::kMetaStageMax (round_kernels.hpp)
// ends of option ranges (options_host.hip includes no kernel header), each checked in the subsystem's own unit
constexpr int kWrmfStageHost = 32;    // == yue::kWrmfStage (wrmf_kernels.hpp)
constexpr int kKnnRangeHost = 4096, kKnnMaxKHost = 256, kKnnGatherHost = 2048;   // == yue::kKnnRange, kKnnMaxK, kKnnGather (knn_kernels.hpp)
constexpr int kCofRangeHost = 8192;   // == yue::kCofRange (cof_kernels.hpp)

// A subsystem's state as the context holds it: yue_host::state() in the subsystem's own unit creates it and supplies the
// deleter, so that whoever sees only the declaration (options_host.hip) can still destroy a context.
template <class T>
using StatePtr = std::unique_ptr<T, void (*)(T *)>;

inline int kr_of(int k) { return k <= 64 ? 1 : k <= 128 ? 2 : 4; }   // registers per lane per row (64 lanes)

// f(std::integral_constant<int, KR>{}) with KR = kr_of(k): picks the <1> / <2> / <4> instance of a kernel template
template <class F>
auto with_kr(int k, F &&f) {
    switch (kr_of(k)) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

}  // namespace yue_host

using yue_host::DevBuf;
using yue_host::Event;
using yue_host::Order;
using yue_host::check_ids;
using yue_host::check_rows;
using yue_host::check_transpose;

struct yue_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t m = 0, n = 0, E = 0, nnz = 0;
    int k = 0;
    bool have_factors = false, have_inter = false;
    DevBuf<float> P, Q, dP, dQ;
    DevBuf<float> margins;                       // [E] the events' margins of the running epoch (k_round_u -> k_loss_margins)
    DevBuf<double> psq_slots;                    // [kNllSlots] sum P*P of the users k_round_u stored (the epoch's P pass when every user has events)
    DevBuf<unsigned long long> cnt0, cnt1;       // item-row touch counters of the even / odd round (total | remaining)
    DevBuf<uint32_t> cntp0, cntp1;               // user-row flushes of the even / odd round
    DevBuf<uint32_t> tab0, tab1;                 // staging-slot tables of the even / odd round (kStageMax words per item row)
    // staged item rows (2 per event of the widest round) live behind the n item rows in the Q allocation,
    // so that "new row in place" and "new row to my staging row" are the same store with another offset
    bool staged = false;                         // the running call uses the staging rows
    bool bigq = false;                           // ... and addresses item / staging rows through 64-bit pointers (2 GiB and more)
    // epoch path: touch metadata of all rounds from one pre-pass (round_kernels.hpp)
    DevBuf<uint32_t> meta_i, meta_j;
    DevBuf<unsigned long long> round_rows;
    DevBuf<uint2> fold, bk_touch;
    DevBuf<uint32_t> bk_ptr;
    DevBuf<int64_t> d_bounds;
    std::vector<int64_t> h_bounds;               // outlives the asynchronous upload
#ifdef YUE_STAMPS
    DevBuf<unsigned long long> stamps;           // diagnostic build: phase stamps of one chosen round launch
    int64_t stamp_launch = -1, update_launches = 0, stamp_waves = 0;
#endif
    DevBuf<int32_t> ev_u, ev_i, ev_j, indices;
    DevBuf<int64_t> indptr;
    DevBuf<int32_t> xu, xi, xj, xk;      // explicit triplets (replay / rounds), CUNE's fourth row
    DevBuf<double> x_loss;               // per-step losses (CUNE)
    DevBuf<float> aU_m, aU_v, aV_m, aV_v;  // Adam moments of the live TF-style path (yue_adam_step); gradients use dP / dQ
    int64_t adam_m = 0, adam_n = 0; int adam_k = 0;
    DevBuf<double> scal;                 // [kNllSlots] nll slots + [8] scalars
    std::vector<int64_t> h_ev_ptr;       // host copy: user -> first event
    bool all_users_have_events = false;  // every user of h_ev_ptr has at least one event
    bool psq_in_rounds = false;          // yue_bpr_epoch: k_round_u sums P*P into psq_slots
    // scoring scratch
    DevBuf<int32_t> s_users, s_ids, s_mask_idx, s_flags;
    DevBuf<int32_t> s_few, s_few_ids;   // two-phase scoring: positions / ids of the users with fewer than N candidates in the first chunk, their lists
    DevBuf<float> s_few_scores;
    int64_t scan_few_users = 0;         // such users of the last scan (read-only option scan_last_few_users)
    DevBuf<int64_t> s_mask_ptr;
    DevBuf<float> s_scores, s_row, s_norms;
    double scan_ms = 0.0;
    int64_t scan_events = 0, scan_rescored = 0, scan_tiles_done = 0, scan_tiles_total = 0;
    DevBuf<unsigned long long> s_work;
    DevBuf<unsigned short> s_qb;         // two-phase scoring: bf16 copy of the item factors
    DevBuf<uint32_t> s_masks;            // ... and the survivor words of a chunk
    int opt_scan_two_phase = 1;          // 0: always the fused kernels (k_topn_scan*)
    int64_t opt_scan_streams_min_users = 262144;   // ... from this many users of a call on (tests lower it)
    int opt_scan_slabs = 4;              // ... slabs of users at least, with two streams
    int opt_scan_streams = 2;            // two-phase path, 262,144 users and more: slabs of users alternate between two streams (1: one stream)
    int opt_scan_filter_ub = 3;          // two-phase path: form of k_scan_filter (scan_host.hip): 3 = two blocks of 32 users per wave, rows by DMA into LDS; 2 = rows through registers; 1 = one block, 8 waves
    int opt_scan_growth = 0;             // two-phase path: a chunk ends at this many times the items scanned so far (0: 2 or 8 by the first items' update rate)
    int scan_chunks = 0;                 // chunks the last scan ran through the filter / select pair
    int scan_used_bf16 = 0;
    // options (yue_set_option)
    int opt_scan_f32 = 0;                // 1: always the exact-f32-MFMA scoring kernel
    int opt_scan_batch = 0;              // bf16 scoring kernel: 0 = two tiles per iteration, 256 users per workgroup (default); 1 = one tile, 128 users
    int opt_round_tpw = 0;               // 0: default events per wave in the round kernel
    int opt_topn_true = 0;               // 1: yue_topn_scan returns a real top-N instead of the reference's overwrite-scan
    int scan_settle = 0;                 // the last two-phase scan used the filter variant that stops settled workgroups (read-only option scan_last_settle)
    int last_stage_max = 0;              // largest staged block of the last pre-pass (read-only option round_last_stage_max)
    int opt_round_stage = 1;             // 0: every contended item row goes through float atomics (no staging rows); 1: sized from the round's mean touches per row; 2..64: rows with up to that many touches are staged (epoch path)
    int opt_round_bucket = 0;            // 1: the bucketed pre-pass also for small catalogues (tests)
    int opt_fold_blocks = 1536;           // workgroups of k_round_fold
    int opt_round_user_seq = 1;          // epoch path on one GPU: 1 = a wave owns a user and walks the user's events in order (k_round_u); 0 = user rows with round semantics (k_round_m + dP)
    int opt_round_fast = 1;              // k_round_u: the step's coefficient in single precision (0: the reference's double-precision sigmoid)
    int last_round_user_seq = 0;         // the last epoch ran k_round_u (read-only option round_last_user_seq)
    int opt_comm_group_mb = 8;           // communicator: user-factor differences per all-reduce (groups of user blocks), MB (8 = what yue_epoch_plan announces; RCCL reaches its bus bandwidth at tens of MB: try 32..64 on a real node)
    int opt_round_cus_reserved = 0;      // CUs the compute stream leaves free (CU mask of the stream) for RCCL's kernels beside the round launches
    int64_t comm_compute_waits = 0;      // times the compute stream waited for the collective stream in the last epoch (read-only option comm_last_compute_waits)
    int opt_round_meta = 1;              // 0: the epoch path counts touches inside the round launches (k_round) as the explicit-rounds path does
    // kernel timing
    int timing_stride = 0;
    std::vector<std::pair<Event, Event>> ev_pool;
    std::vector<int64_t> ev_triplets, ev_launches;
    size_t ev_used = 0;
    // FISM (parity path): item-history factors (f64), item factors (f32), item bias (f64)
    DevBuf<double> fP, fBi, f_coef, f_x, f_hist, f_scores, f_out_sc;
    DevBuf<float> fQ;
    DevBuf<int64_t> f_ptr;
    DevBuf<int32_t> f_items, f_negs, f_ids, f_flags;
    // FISM rounds: touched-item lists, positions, working copies, difference buffers
    DevBuf<int64_t> f_uq_ptr, f_neg_ptr;
    DevBuf<int32_t> f_uq_items, f_loc_i, f_loc_j;
    DevBuf<float> f_wq, f_dQ;
    DevBuf<double> f_wp, f_wb, f_dP, f_dB;
    DevBuf<unsigned> f_cnt;              // [2][n] users of a round touching an item (k_fism_round_lds)
    int64_t fn = 0;
    int fk = 0;
    int opt_fism_inplace = 1;            // 0: every row a round's users touch goes through the difference buffers (round 3's form)
    int opt_fism_lds = 1;                // 0: yue_fism_rounds always through k_fism_round (working rows in global memory, item lists from the host)
    int64_t fism_form = 0;               // form the last yue_fism_rounds took: 0 k_fism_round, 1 k_fism_round_lds<KR, false>, 2 <KR, true> (read-only option fism_last_form)
    // exact path (chain_host.hip): touch keys / ordinals, runs, granule copies of the factor rows, control words
    DevBuf<uint32_t> ch_key, ch_val, ch_key2, ch_val2, ch_seg, ch_ord_i, ch_ord_j, ch_head, ch_incl, ch_ord_u, ch_rkey, ch_rval;
    DevBuf<int64_t> ch_run_ptr, d_ev_ptr;
    DevBuf<int32_t> ch_run_u;
    DevBuf<unsigned char> ch_tmp;
    DevBuf<unsigned> ch_Qv, ch_Pv;
    DevBuf<unsigned long long> ch_ctl;   // [0] run claim counter, [1] validation flags, [2] wait status
    DevBuf<unsigned long long> ch_stats; // diagnostic build (make chainstats) only
    bool d_ev_ptr_valid = false;
    int opt_epoch_exact = 0;             // 1: yue_bpr_epoch applies the epoch's triplets with exact sequential semantics (k_bpr_chain)
    int opt_replay_levels = 0;           // 1: yue_bpr_replay by host-computed dependency levels, one launch per level (the round-1 path)
    int opt_chain_split = -1;            // 1: a run is walked by a group of five waves (k_bpr_chain3: 2 x loads / dependency chain / 2 x stores); 0: by one wave (k_bpr_chain); -1: by the stream's mean run length
    int opt_chain_ring = 0;              // wave-group kernel: triplets whose rows a loading wave keeps in flight (0 = 8; 16 for k <= 128)
    int opt_chain_xcd = 0;               // wave-group kernel: 1 = all working waves on ONE XCD, rows handed over through its L2
    int opt_chain_fast = 0;              // 1: single-precision coefficient, one 64-lane sum per triplet (within 1e-5, not bit-equal)
    int opt_chain_waves = 0;             // workgroups per CU of the persistent launch (0: what fits, at most 8)
    int64_t opt_chain_spin = 0;          // polls per wait before a wave gives up (0: 2^22)
    int64_t chain_runs = 0, chain_waves = 0, chain_groups = 0, chain_kernel_us = 0, replay_levels = 0;
    Event ev_chain0, ev_chain1;   // brackets of the dataflow launch (read-only option chain_last_us)
    // RCCL
    ncclComm *comm = nullptr;              // ncclComm_t (comm.hip)
    int rank = 0, nranks = 1;
    hipStream_t comm_stream = nullptr;   // (all-reduce +) user-row apply of yue_bpr_epoch run here, beside the next rounds
    Event ev_rounds, ev_comm;
    Event ev_t_rounds, ev_t_comm;   // timing pair of the last epoch on a communicator: end of its round launches / end of its last apply
    // TEST SEAM (libyue_hip_seam.so only, make test-seam: the product library has no way to set these): the collective of
    // reduce_user_block / yue_allreduce_f64 as a host-staged sum through a callback, so that the 2-rank block / group /
    // stream logic of yue_bpr_epoch runs on a one-GPU box (tests/test_gpu_multi.py).  dtype 0 = float, 1 = double.
    int (*seam_reduce)(void *host, int64_t count, int dtype, void *user) = nullptr;
    void *seam_user = nullptr;
    std::vector<float> seam_buf;
    // communicator statistics of the last yue_bpr_epoch (yue_get_comm_stats)
    int64_t comm_collectives = 0;
    double comm_bytes = 0.0, comm_wait_ms = 0.0;
    int comm_version = 0, comm_nranks_reported = 0;
    Event ev_scan0, ev_scan1;      // brackets of the scoring kernel (yue_get_scan_stats)
    yue_host::StatePtr<yue_wrmf> wrmf{nullptr, nullptr};   // WRMF state (yue_wrmf_set_pairs), owned by wrmf_host.hip
    int64_t opt_wrmf_long_pairs = 2048;  // WRMF: rows with more pairs are summed by several workgroups (chunks of this many pairs) before their solve; read by yue_wrmf_set_pairs and by CoFactor's schedule
    int64_t wrmf_ns[2] = {0, 0};         // device time of the last half-sweep, of its long-row chunks (read-only options wrmf_last_ns / wrmf_last_long_ns)
    yue_host::StatePtr<yue_knn> knn{nullptr, nullptr};   // UserKNN state (yue_knn_set_pairs), owned by knn_host.hip
    int opt_knn_range = yue_host::kKnnRangeHost, opt_knn_gather = yue_host::kKnnGatherHost;   // UserKNN: candidate users per counting pass, entries per scoring chunk (tests lower them to reach the multi-pass paths)
    int64_t knn_ns = 0, knn_chunked_users = 0;   // device time of the last neighbours / topn / predict call; users of the last topn scored in item-range chunks (read-only options knn_last_*)
    yue_host::StatePtr<yue_ipf> ipf{nullptr, nullptr};   // IPF state (yue_ipf_set_graph), owned by ipf_host.hip
    int opt_ipf_slots = 1024;            // IPF: workgroups (queries in flight) of one yue_ipf_topn launch
    int64_t ipf_ns = 0;                  // device time of the last topn / predict launch (read-only option ipf_last_ns)
    yue_host::StatePtr<yue_expo> expo{nullptr, nullptr};   // ExpoMF state (yue_expo_set_mu), owned by expo_host.hip
    int64_t opt_expo_gram_mb = 512;      // ExpoMF: budget of the per-row Gram workspace, MiB: a half-sweep runs in batches of rows that fit
    int64_t expo_ns[2] = {0, 0};         // device time of the last half-sweep / mu update, of its dense MFMA kernel(s) (read-only options expo_last_ns / expo_last_gram_ns)
    int64_t expo_batches = 0;            // row batches of the last half-sweep (read-only option expo_last_batches)
    yue_host::StatePtr<yue_cof> cof{nullptr, nullptr};   // CoFactor state (yue_cof_*), owned by cof_host.hip
    int64_t opt_cof_cooccur_mb = 1024;   // CoFactor: bound of the co-occurrence CSR (idx + cnt: 8 bytes per entry), MiB
    int64_t opt_cof_pass_items = yue_host::kCofRangeHost;   // ... items counted per pass
    int opt_cof_level_timing = 0;        // ... 1: time every level's launch (tools/cofactor_bench.py)
    int64_t cof_ns[2] = {0, 0};          // device time of the last co-occurrence build / item sweep, of the sweep's levels of fewer than 256 rows (0 unless timed) (read-only options cof_last_ns / cof_last_small_ns)
    yue_host::StatePtr<yue_cnet> cnet{nullptr, nullptr};   // CUNE user-network state (yue_cnet_*), owned by cnet_host.hip
    int64_t cnet_ns = 0;                 // device time of the last walks / embed / friends call (read-only option cnet_last_ns)
    yue_host::StatePtr<yue_s2v> s2v{nullptr, nullptr};   // Song2vec state (yue_s2v_*), owned by s2v_host.hip
    int opt_s2v_schedule = 1;            // Song2vec: 0 = one wave walks all steps, 1 = one launch per dependency level
    int64_t s2v_ns = 0;                  // device time of the last yue_s2v_epoch (read-only option s2v_last_ns)
    yue_host::StatePtr<yue_lgcn> lgcn{nullptr, nullptr};   // LightGCN state (yue_lgcn_*), owned by lgcn_host.hip
    int64_t opt_lgcn_hub = 1024;         // LightGCN: rows with more neighbours are cut into parts of this many, one wave each (lgcn_kernels.hpp)
    int64_t lgcn_hubs = 0, lgcn_parts = 0;   // ... such rows and their parts in the last call (read-only options lgcn_last_hubs / lgcn_last_parts)
    int64_t lgcn_ns[4] = {0, 0, 0, 0};   // device time of the last call's forward, minibatch, backward and Adam phases (read-only options lgcn_last_*_ns)
    yue_host::StatePtr<yue_ngcf> ngcf{nullptr, nullptr};   // NGCF state (yue_ngcf_*), owned by ngcf_host.hip
    int64_t opt_ngcf_hub = 1024;         // NGCF: as lgcn_hub, for the graph and its transpose
    int64_t ngcf_hubs = 0, ngcf_parts = 0;   // ... hub rows and parts of both matrices in the last call (read-only options ngcf_last_hubs / ngcf_last_parts)
    int64_t ngcf_ns[6] = {0, 0, 0, 0, 0, 0};   // device time of the last call's gather, dense, batch, backward, wgrad and adam phases (read-only options ngcf_last_*_ns)
    yue_host::StatePtr<yue_cdae> cdae{nullptr, nullptr};   // CDAE state (yue_cdae_*), owned by cdae_host.hip
    int64_t opt_cdae_hub = 1024;         // CDAE: encoder rows and regrouped segments with more entries are cut into parts of this many (the default is lgcn_hub's, unmeasured here)
    int64_t cdae_hubs = 0, cdae_parts = 0;   // ... such rows / segments and their parts in the last call (read-only options cdae_last_hubs / cdae_last_parts)
    int64_t cdae_saturated = 0;          // sampled outputs with y_pred == 1.0f in the last call (read-only option cdae_last_saturated)
    int64_t cdae_ns[4] = {0, 0, 0, 0};   // device time of the last call's encode, decode, regroup and adam phases (yue_cdae_times)
    yue_host::StatePtr<yue_apr> apr{nullptr, nullptr};   // APR state (yue_apr_*), owned by apr_host.hip
    int64_t apr_longest = 0;             // longest (triplet, role) list of a row in the last batch (read-only option apr_last_longest_row)
    int64_t apr_ns[4] = {0, 0, 0, 0};    // device time of the last call's coefficient, row, normalise and adam phases (yue_apr_times)
};

namespace yue_host {
inline bool on_communicator(const yue_ctx *c) { return c->comm != nullptr || c->seam_reduce != nullptr; }
// bpr_host.hip: yue_bpr_epoch runs k_round_meta + k_round_m / k_round_u + k_round_fold for the uploaded factors (else k_round)
bool fold_path(const yue_ctx *c);
// bpr_host.hip: loss / scalar scratch shared by the training entry points
int zero_scalars(yue_ctx *c);
int read_scalars(yue_ctx *c, double *nll, double *sp, double *sq);
int sumsq_async(yue_ctx *c, const double *p_slots = nullptr);   // p_slots: sum P*P from these kNllSlots partial sums instead of a pass over P
int upload_triplets(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, bool validate);
int adam_apply(yue_ctx *c, double lr, int64_t step);            // k_adam on P and Q with the gradients in dP / dQ, lr_t of `step`
// ... the same step on any dense parameter with moments and gradient of its own (NGCF's weights)
int adam_apply_dense(yue_ctx *c, float *var, float *m, float *v, float *grad, int64_t count, double lr, int64_t step);
// comm.hip: sum dP[first .. first + count) over the ranks on `stream` (in place); identity without a communicator
int reduce_user_block(yue_ctx *c, int64_t first, int64_t count, hipStream_t stream);
// chain_host.hip: exact sequential semantics over the uploaded events (negatives in ev_j) / over the stream in xu, xi, xj
int chain_epoch(yue_ctx *c, double lr, double regU, double regI);
int chain_stream(yue_ctx *c, int64_t T, double lr, double regU, double regI);
// The subsystem's state for an entry point of its own unit (the only place that sees the type whole): made on the context's
// device when there is none yet, and destroyed with the context.
template <class T>
int state(yue_ctx *c, StatePtr<T> &slot, T **out) {
    if (!slot) {
        HIPCHK(hipSetDevice(c->device));
        slot = StatePtr<T>(new T(), [](T *s) { delete s; });
    }
    *out = slot.get();
    return YUE_OK;
}
// The subsystems below: what yue_get_option reads from one of them without a state is 0.
// wrmf_host.hip: a side's long rows (read-only options wrmf_long_rows_user / _item)
int64_t wrmf_long_rows(const yue_ctx *c, int side);
// ... the uploaded pairs of one side (0: user rows, 1: item rows) for the other ALS solver (expo_host.hip); false when
// yue_wrmf_set_pairs has not run for the context's current factors
struct WrmfPairsView {
    const int64_t *ptr, *cptr, *cbeg, *cend;
    const int32_t *idx, *cnt, *sched, *cpos;
    int64_t rows, n_long, chunks, n_nonempty;       // n_nonempty: rows with pairs, the first positions of sched
    int64_t generation;                             // counts the uploads of yue_wrmf_set_pairs
};
bool wrmf_pairs_view(const yue_ctx *c, int side, WrmfPairsView *v);
// ... and the fp32-rounded F^T F of the side's fixed factors (0: Y^T Y, 1: X^T X), queued on the context's stream into the
// WRMF state's slot-major buffer (cof_host.hip)
int wrmf_gram(yue_ctx *c, int side, const double **G);
// cof_host.hip: levels of the uploaded SPPMI, entries of the co-occurrence CSR (read-only options cof_levels / cof_cooccur_nnz)
int64_t cof_levels(const yue_ctx *c);
int64_t cof_cooccur_nnz(const yue_ctx *c);
// s2v_host.hip: dependency levels of the steps (which = 0) / the pairs (1) (read-only options s2v_levels_steps / s2v_levels_pairs)
int64_t s2v_levels(const yue_ctx *c, int which);
}  // namespace yue_host
