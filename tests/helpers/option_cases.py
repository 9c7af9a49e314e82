"""What yue_get_option / yue_set_option must answer: every option's default, what it accepts, what it refuses and with which
words.  Shared by tests/test_gpu_options.py (through the C ABI on a device) and tests/test_option_table.py (the table alone, on
the CPU).  The expectations are written out by hand from the context's defaults (csrc/host_common.hpp) and the documented
ranges (include/yue_hip.h); they are not read from the library's own option table."""

# name -> default; set to 0, 1 and 7 they read back 0, 1, 1
FLAGS = {'scan_f32': 0, 'scan_two_phase': 1, 'topn_true': 0, 'fism_lds': 1, 'fism_inplace': 1, 'round_meta': 1, 'round_user_seq': 1,
         'round_fast': 1, 'round_bucket': 0, 'epoch_exact': 0, 'replay_levels': 0, 'chain_fast': 0, 'chain_xcd': 0}
FLAG_VALUES = ((0, 0), (1, 1), (7, 1), (0, 0), (-3, 1))      # (set, read back)

# name -> (default, accepted boundary values, refused values, the refusal's words)
RANGES = {
    'scan_batch': (0, [0, 1], [-1, 2], 'scan_batch must be 0 or 1'),
    'scan_growth': (0, [0, 2, 64], [-1, 1, 65], 'scan_growth must be 0 (automatic) or 2..64'),
    'scan_filter_ub': (3, [1, 3], [0, 4], 'scan_filter_ub must be 1, 2 or 3'),
    'scan_streams': (2, [1, 2], [0, 3], 'scan_streams must be 1 or 2'),
    'scan_slabs': (4, [2, 64], [1, 65], 'scan_slabs must be 2..64'),
    'scan_streams_min_users': (262144, [1024, 1 << 40], [1023, -1], 'scan_streams_min_users must be at least 1024'),     # (no upper end)
    'round_stage': (1, [0, 1, 2, 64], [-1, 65], 'round_stage must be 0, 1 or 2..64'),
    'comm_group_mb': (8, [1, 4096], [0, 4097], 'comm_group_mb must be 1..4096'),
    'fold_blocks': (1536, [1, 65536], [0, 65537], 'fold_blocks out of range'),
    'chain_waves': (0, [0, 8], [-1, 9], 'chain_waves must be 0..8'),
    'chain_split': (-1, [-1, 0, 1], [-2, 2], 'chain_split must be -1, 0 or 1'),
    'chain_ring': (0, [0, 8, 16], [-1, 4, 12, 17], 'chain_ring must be 0, 8 or 16'),
    'chain_spin': (0, [0, 0x7fffffff], [-1, 1 << 31], 'chain_spin out of range'),
    # the subsystems' tunables: members of the context like the rest, read and set before the subsystem has any state
    'wrmf_long_pairs': (2048, [32, 1 << 40], [31, -1], 'wrmf_long_pairs must be >= 32'),                                # (no upper end)
    'knn_range': (4096, [64, 4096], [63, 4097], 'knn_range must be 64..4096'),
    'knn_gather': (2048, [256, 2048], [255, 2049], 'knn_gather must be 256..2048'),
    'ipf_slots': (1024, [1, 4096], [0, 4097], 'ipf_slots must be 1..4096'),
    'expo_gram_mb': (512, [1, 65536], [0, 65537], 'expo_gram_mb must be in [1, 65536]'),
    'cof_cooccur_mb': (1024, [1, 65536], [0, 65537], 'cof_cooccur_mb must be in [1, 65536]'),
    'cof_level_timing': (0, [0, 1], [-1, 2, 7], 'cof_level_timing must be 0 or 1'),                                      # (a range, not a flag)
    'cof_pass_items': (8192, [64, 8192], [63, 8193], 'cof_pass_items must be in [64, 8192]'),
    's2v_schedule': (1, [0, 1], [-1, 2], 's2v_schedule must be 0 (one wave walks all steps) or 1 (levels)'),
}

# name -> value on a fresh context (round_path: no factors yet, the epoch path's metadata form is the default; the
# subsystems' reports and facts: no subsystem has any state yet)
READ_ONLY = {'scan_last_chunks': 0, 'scan_last_few_users': 0, 'scan_last_settle': 0, 'round_last_stage_max': 0, 'comm_last_compute_waits': 0,
             'round_last_user_seq': 0, 'fism_last_form': 0, 'chain_last_us': 0, 'chain_last_runs': 0, 'chain_last_waves': 0, 'replay_last_levels': 0, 'round_path': 1,
             'wrmf_last_ns': 0, 'wrmf_last_long_ns': 0, 'wrmf_long_rows_user': 0, 'wrmf_long_rows_item': 0,
             'knn_last_ns': 0, 'knn_last_chunked_users': 0, 'ipf_last_ns': 0,
             'expo_last_ns': 0, 'expo_last_gram_ns': 0, 'expo_last_batches': 0,
             'cof_last_ns': 0, 'cof_last_small_ns': 0, 'cof_levels': 0, 'cof_cooccur_nnz': 0,
             'cnet_last_ns': 0, 's2v_levels_steps': 0, 's2v_levels_pairs': 0, 's2v_last_ns': 0}

# options with a setter of their own
OTHER = {'round_cus_reserved': 0, 'round_tpw': 0}

# names no table row carries: the get answers 'yue_get_option: unknown option NAME', the set 'yue_set_option: unknown option NAME'
UNKNOWN = ('', 'scan_slab', 'scan_slabs ', 'wrmf_nonsense', 'knn_', 'cof')

# round_tpw before any factors are uploaded: the whole set passes
TPW_ACCEPTED = (2, 4, 8, 16, 0)
TPW_REFUSED = (-2, 1, 3, 6, 12, 32)
TPW_WORDS = 'yue_set_option: round_tpw must be 0, 2, 4, 8 or 16'


def defaults():
    """name -> value on a fresh context, of all 67 options"""
    want = dict(FLAGS)
    want.update({name: row[0] for name, row in RANGES.items()})
    want.update(READ_ONLY)
    want.update(OTHER)
    assert len(want) == len(FLAGS) + len(RANGES) + len(READ_ONLY) + len(OTHER) == 67
    return want
