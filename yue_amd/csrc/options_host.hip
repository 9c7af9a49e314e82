// libyue_hip.so -- yue_get_option / yue_set_option (include/yue_hip.h): one table row per option, walked by both entry
// points.  Every option is a member of the context, or a fact that a subsystem's own reader returns (0 without a state), so
// no call here allocates or touches a subsystem.  No kernel header is included: this unit holds no device code.
#include "host_common.hpp"

#include <limits>

using yue_host::fail;

namespace {

struct Option {
    const char *name;
    int64_t (*get)(yue_ctx *);                           // none: the option cannot be read
    void (*put)(yue_ctx *, int64_t);
    int (*set)(const Option &, yue_ctx *, int64_t);      // set_flag, set_ranged or a setter of the option's own; none: read-only
    int64_t lo, hi;                                      // set_ranged: the accepted interval,
    const char *refusal;                                 // ... what the message says after the name for any other value
    std::vector<int64_t> also;                           // ... unless it is one of these
};
// get and put of an option kept in a member of the context (int and int64_t members both occur)
#define YUE_AT(member) [](yue_ctx *c) -> int64_t { return c->member; }, [](yue_ctx *c, int64_t v) { c->member = (decltype(c->member))v; }
// get of a fact a subsystem keeps for its own logic
#define YUE_FROM(reader) [](yue_ctx *c) -> int64_t { return yue_host::reader; }

int set_flag(const Option &o, yue_ctx *c, int64_t value) { o.put(c, value != 0); return YUE_OK; }

int set_ranged(const Option &o, yue_ctx *c, int64_t value) {
    if ((value < o.lo || value > o.hi) && std::find(o.also.begin(), o.also.end(), value) == o.also.end())
        return fail(YUE_ERR_ARG, std::string("yue_set_option: ") + o.name + " " + o.refusal);
    o.put(c, value);
    return YUE_OK;
}

// which kernels yue_bpr_epoch runs for the uploaded factors: 0 k_round, 1 k_round_meta + k_round_m + k_round_fold
int64_t round_path(yue_ctx *c) { return yue_host::fold_path(c) ? 1 : 0; }

int set_round_cus_reserved(const Option &, yue_ctx *c, int64_t value) {
    // the compute stream is re-created with a CU mask that leaves the LAST `value` CUs of the device free: RCCL's kernels
    // (collective stream, no mask) find room beside round launches that would otherwise fill the chip exactly
    int cus = 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    if (value < 0 || value >= cus) return fail(YUE_ERR_ARG, "yue_set_option: round_cus_reserved must be 0 .. CUs - 1");
    HIPCHK(hipStreamSynchronize(c->stream));
    hipStream_t fresh = nullptr;
    if (value == 0) HIPCHK(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
    else {
        std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
        for (int cu = 0; cu < cus - (int)value; ++cu) mask[(size_t)cu / 32] |= 1u << (cu % 32);
        HIPCHK(hipExtStreamCreateWithCUMask(&fresh, (uint32_t)mask.size(), mask.data()));
    }
    (void)hipStreamDestroy(c->stream);
    c->stream = fresh;
    c->opt_round_cus_reserved = (int)value;
    return YUE_OK;
}

// Not derived from the list of round-kernel instances (bpr_host.hip): this rule sees the k uploaded at the time of the call
// only (none yet: every listed value passes), and it lets 2 events per wave through for k > 128, which the list does not
// hold -- the launch refuses that pair.  A rule derived from the list would refuse it here, with another message.
int set_round_tpw(const Option &, yue_ctx *c, int64_t value) {
    if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16) return fail(YUE_ERR_ARG, "yue_set_option: round_tpw must be 0, 2, 4, 8 or 16");
    if (value == 8 && yue_host::kr_of(c->k) == 4) return fail(YUE_ERR_ARG, "yue_set_option: round_tpw 8 needs k <= 128");
    if (value == 16 && yue_host::kr_of(c->k) != 1) return fail(YUE_ERR_ARG, "yue_set_option: round_tpw 16 needs k <= 64");
    c->opt_round_tpw = (int)value;
    return YUE_OK;
}

#ifdef YUE_STAMPS
int set_stamp_launch(const Option &, yue_ctx *c, int64_t value) { c->stamp_launch = value; c->update_launches = 0; return YUE_OK; }
#endif

constexpr int64_t kNoEnd = std::numeric_limits<int64_t>::max();

const Option kOptions[] = {
    // scoring (scan_host.hip)
    {"scan_f32", YUE_AT(opt_scan_f32), set_flag},
    {"scan_batch", YUE_AT(opt_scan_batch), set_ranged, 0, 1, "must be 0 or 1"},
    {"scan_two_phase", YUE_AT(opt_scan_two_phase), set_flag},
    {"scan_growth", YUE_AT(opt_scan_growth), set_ranged, 2, 64, "must be 0 (automatic) or 2..64", {0}},
    {"scan_filter_ub", YUE_AT(opt_scan_filter_ub), set_ranged, 1, 3, "must be 1, 2 or 3"},
    {"scan_streams", YUE_AT(opt_scan_streams), set_ranged, 1, 2, "must be 1 or 2"},
    {"scan_slabs", YUE_AT(opt_scan_slabs), set_ranged, 2, 64, "must be 2..64"},
    {"scan_streams_min_users", YUE_AT(opt_scan_streams_min_users), set_ranged, 1024, kNoEnd, "must be at least 1024"},
    {"scan_last_chunks", YUE_AT(scan_chunks)},
    {"scan_last_few_users", YUE_AT(scan_few_users)},
    {"scan_last_settle", YUE_AT(scan_settle)},
    {"topn_true", YUE_AT(opt_topn_true), set_flag},
    // FISM (fism_host.hip)
    {"fism_lds", YUE_AT(opt_fism_lds), set_flag},
    {"fism_inplace", YUE_AT(opt_fism_inplace), set_flag},
    {"fism_last_form", YUE_AT(fism_form)},
    // S-rounds and epochs (bpr_host.hip), the communicator (comm.hip)
    {"round_stage", YUE_AT(opt_round_stage), set_ranged, 0, yue_host::kMetaStageMaxHost, "must be 0, 1 or 2..64"},
    {"round_last_stage_max", YUE_AT(last_stage_max)},
    {"round_meta", YUE_AT(opt_round_meta), set_flag},
    {"comm_group_mb", YUE_AT(opt_comm_group_mb), set_ranged, 1, 4096, "must be 1..4096"},
    {"round_cus_reserved", YUE_AT(opt_round_cus_reserved), set_round_cus_reserved},
    {"comm_last_compute_waits", YUE_AT(comm_compute_waits)},
    {"round_user_seq", YUE_AT(opt_round_user_seq), set_flag},
    {"round_fast", YUE_AT(opt_round_fast), set_flag},
    {"round_last_user_seq", YUE_AT(last_round_user_seq)},
    {"round_bucket", YUE_AT(opt_round_bucket), set_flag},
    {"fold_blocks", YUE_AT(opt_fold_blocks), set_ranged, 1, 65536, "out of range"},
    {"round_tpw", YUE_AT(opt_round_tpw), set_round_tpw},
    {"round_path", round_path},
#ifdef YUE_STAMPS
    {"debug_stamp_launch", nullptr, nullptr, set_stamp_launch},
#endif
    // exact sequential semantics (chain_host.hip), levelled replay
    {"epoch_exact", YUE_AT(opt_epoch_exact), set_flag},
    {"replay_levels", YUE_AT(opt_replay_levels), set_flag},
    {"chain_waves", YUE_AT(opt_chain_waves), set_ranged, 0, 8, "must be 0..8"},
    {"chain_split", YUE_AT(opt_chain_split), set_ranged, -1, 1, "must be -1, 0 or 1"},
    {"chain_fast", YUE_AT(opt_chain_fast), set_flag},
    {"chain_xcd", YUE_AT(opt_chain_xcd), set_flag},
    {"chain_ring", YUE_AT(opt_chain_ring), set_ranged, 0, 0, "must be 0, 8 or 16", {8, 16}},
    {"chain_spin", YUE_AT(opt_chain_spin), set_ranged, 0, 0x7fffffff, "out of range"},
    {"chain_last_us", YUE_AT(chain_kernel_us)},
    {"chain_last_runs", YUE_AT(chain_runs)},          // last exact launch: runs walked, waves launched
    {"chain_last_waves", YUE_AT(chain_waves)},
    {"replay_last_levels", YUE_AT(replay_levels)},    // last levelled replay: dependency levels = launches
    // LightGCN (lgcn_host.hip)
    {"lgcn_hub", YUE_AT(opt_lgcn_hub), set_ranged, 1, 0x7fffffff, "must be 1 .. 2^31 - 1"},
    {"lgcn_last_hubs", YUE_AT(lgcn_hubs)},
    {"lgcn_last_parts", YUE_AT(lgcn_parts)},
    {"lgcn_last_forward_ns", YUE_AT(lgcn_ns[0])},
    {"lgcn_last_batch_ns", YUE_AT(lgcn_ns[1])},
    {"lgcn_last_backward_ns", YUE_AT(lgcn_ns[2])},
    {"lgcn_last_adam_ns", YUE_AT(lgcn_ns[3])},
    // NGCF (ngcf_host.hip)
    {"ngcf_hub", YUE_AT(opt_ngcf_hub), set_ranged, 1, 0x7fffffff, "must be 1 .. 2^31 - 1"},
    {"ngcf_last_hubs", YUE_AT(ngcf_hubs)},
    {"ngcf_last_parts", YUE_AT(ngcf_parts)},
    {"ngcf_last_gather_ns", YUE_AT(ngcf_ns[0])},
    {"ngcf_last_dense_ns", YUE_AT(ngcf_ns[1])},
    {"ngcf_last_batch_ns", YUE_AT(ngcf_ns[2])},
    {"ngcf_last_backward_ns", YUE_AT(ngcf_ns[3])},
    {"ngcf_last_wgrad_ns", YUE_AT(ngcf_ns[4])},
    {"ngcf_last_adam_ns", YUE_AT(ngcf_ns[5])},
    // CDAE (cdae_host.hip)
    {"cdae_hub", YUE_AT(opt_cdae_hub), set_ranged, 1, 0x7fffffff, "must be 1 .. 2^31 - 1"},
    {"cdae_last_hubs", YUE_AT(cdae_hubs)},
    {"cdae_last_parts", YUE_AT(cdae_parts)},
    {"cdae_last_saturated", YUE_AT(cdae_saturated)},
    // APR (apr_host.hip)
    {"apr_last_longest_row", YUE_AT(apr_longest)},
    // WRMF (wrmf_host.hip)
    {"wrmf_long_pairs", YUE_AT(opt_wrmf_long_pairs), set_ranged, yue_host::kWrmfStageHost, kNoEnd, "must be >= 32"},   // takes effect at the next yue_wrmf_set_pairs
    {"wrmf_last_ns", YUE_AT(wrmf_ns[0])},
    {"wrmf_last_long_ns", YUE_AT(wrmf_ns[1])},
    {"wrmf_long_rows_user", YUE_FROM(wrmf_long_rows(c, 0))},
    {"wrmf_long_rows_item", YUE_FROM(wrmf_long_rows(c, 1))},
    // UserKNN (knn_host.hip)
    {"knn_range", YUE_AT(opt_knn_range), set_ranged, 64, yue_host::kKnnRangeHost, "must be 64..4096"},
    {"knn_gather", YUE_AT(opt_knn_gather), set_ranged, yue_host::kKnnMaxKHost, yue_host::kKnnGatherHost, "must be 256..2048"},
    {"knn_last_ns", YUE_AT(knn_ns)},
    {"knn_last_chunked_users", YUE_AT(knn_chunked_users)},
    // IPF (ipf_host.hip)
    {"ipf_slots", YUE_AT(opt_ipf_slots), set_ranged, 1, 4096, "must be 1..4096"},
    {"ipf_last_ns", YUE_AT(ipf_ns)},
    // ExpoMF (expo_host.hip)
    {"expo_gram_mb", YUE_AT(opt_expo_gram_mb), set_ranged, 1, 65536, "must be in [1, 65536]"},
    {"expo_last_ns", YUE_AT(expo_ns[0])},
    {"expo_last_gram_ns", YUE_AT(expo_ns[1])},
    {"expo_last_batches", YUE_AT(expo_batches)},
    // CoFactor (cof_host.hip)
    {"cof_cooccur_mb", YUE_AT(opt_cof_cooccur_mb), set_ranged, 1, 65536, "must be in [1, 65536]"},
    {"cof_level_timing", YUE_AT(opt_cof_level_timing), set_ranged, 0, 1, "must be 0 or 1"},
    {"cof_pass_items", YUE_AT(opt_cof_pass_items), set_ranged, 64, yue_host::kCofRangeHost, "must be in [64, 8192]"},
    {"cof_last_ns", YUE_AT(cof_ns[0])},
    {"cof_last_small_ns", YUE_AT(cof_ns[1])},
    {"cof_levels", YUE_FROM(cof_levels(c))},
    {"cof_cooccur_nnz", YUE_FROM(cof_cooccur_nnz(c))},
    // CUNE's user-network stage (cnet_host.hip)
    {"cnet_last_ns", YUE_AT(cnet_ns)},
    // Song2vec (s2v_host.hip)
    {"s2v_schedule", YUE_AT(opt_s2v_schedule), set_ranged, 0, 1, "must be 0 (one wave walks all steps) or 1 (levels)"},
    {"s2v_levels_steps", YUE_FROM(s2v_levels(c, 0))},
    {"s2v_levels_pairs", YUE_FROM(s2v_levels(c, 1))},
    {"s2v_last_ns", YUE_AT(s2v_ns)},
};
#undef YUE_AT
#undef YUE_FROM

const Option *find_option(const std::string &key) {
    for (const Option &o : kOptions) if (key == o.name) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

int yue_get_option(yue_ctx *c, const char *name, int64_t *value) {
    if (!c || !name || !value) return fail(YUE_ERR_ARG, "yue_get_option: null argument");
    const std::string key(name);
    const Option *o = find_option(key);
    if (o && o->get) { *value = o->get(c); return YUE_OK; }
    return fail(YUE_ERR_ARG, "yue_get_option: unknown option " + key);
}

int yue_set_option(yue_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return fail(YUE_ERR_ARG, "yue_set_option: null argument");
    const std::string key(name);
    const Option *o = find_option(key);
    if (o && o->set) return o->set(*o, c, value);          // (a read-only name answers as one the table does not hold)
    return fail(YUE_ERR_ARG, "yue_set_option: unknown option " + key);
}

}  // extern "C"
