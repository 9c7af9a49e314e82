"""yue_get_option / yue_set_option through the C ABI: every option's default, what it accepts, what it refuses and with which
words.  The expectations below are written out by hand from the context's defaults (csrc/host_common.hpp) and the documented
ranges (include/yue_hip.h); they are not read from the library's own option table."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# name -> default; set to 0, 1 and 7 they read back 0, 1, 1
FLAGS = {'scan_f32': 0, 'scan_two_phase': 1, 'topn_true': 0, 'fism_lds': 1, 'fism_inplace': 1, 'round_meta': 1, 'round_user_seq': 1,
         'round_fast': 1, 'round_bucket': 0, 'epoch_exact': 0, 'replay_levels': 0, 'chain_fast': 0, 'chain_xcd': 0}

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
}

# name -> value on a fresh context (round_path: no factors yet, the epoch path's metadata form is the default)
READ_ONLY = {'scan_last_chunks': 0, 'scan_last_few_users': 0, 'scan_last_settle': 0, 'round_last_stage_max': 0, 'comm_last_compute_waits': 0,
             'round_last_user_seq': 0, 'fism_last_form': 0, 'chain_last_us': 0, 'chain_last_runs': 0, 'chain_last_waves': 0, 'replay_last_levels': 0, 'round_path': 1}

# options with a setter of their own
OTHER = {'round_cus_reserved': 0, 'round_tpw': 0}

# options of the subsystems that own them (routed by prefix), read before the subsystem has any state
ROUTED = {'wrmf_long_pairs': 2048, 'knn_range': 4096, 'ipf_slots': 1024, 'expo_gram_mb': 512, 'cof_cooccur_mb': 1024}


@pytest.fixture
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def _refused(dev, name, value, words):
    from yue_amd._shim import YueHipError
    with pytest.raises(YueHipError, match=re.escape(words)):
        dev.set_option(name, value)


def test_every_option_reads_its_default_on_a_fresh_context(dev):
    want = dict(FLAGS)
    want.update({name: row[0] for name, row in RANGES.items()})
    want.update(READ_ONLY)
    want.update(OTHER)
    assert len(want) == len(FLAGS) + len(RANGES) + len(READ_ONLY) + len(OTHER) == 40
    for name, value in want.items():
        assert dev.get_option(name) == value, name


def test_flags_read_back_zero_or_one(dev):
    for name, default in FLAGS.items():
        for value, back in ((0, 0), (1, 1), (7, 1), (0, 0), (-3, 1)):
            dev.set_option(name, value)
            assert dev.get_option(name) == back, (name, value)
        dev.set_option(name, default)


def test_ranges_accept_their_ends_and_refuse_the_values_beside_them(dev):
    for name, (default, accepted, refused, words) in RANGES.items():
        for value in accepted:
            dev.set_option(name, value)
            assert dev.get_option(name) == value, (name, value)
            for bad in refused:
                _refused(dev, name, bad, 'yue_set_option: ' + words)
                assert dev.get_option(name) == value, (name, bad)       # a refused value changes nothing
        dev.set_option(name, default)


def test_read_only_and_unknown_names_are_refused(dev):
    from yue_amd._shim import YueHipError
    for name in READ_ONLY:
        for value in (0, 1):
            _refused(dev, name, value, 'yue_set_option: unknown option ' + name)
        assert dev.get_option(name) == READ_ONLY[name]
    _refused(dev, 'round_nonsense', 1, 'yue_set_option: unknown option round_nonsense')
    with pytest.raises(YueHipError, match=re.escape('yue_get_option: unknown option round_nonsense')):
        dev.get_option('round_nonsense')
    for name in ('', 'scan_slab', 'scan_slabs ', 'wrmf_nonsense', 'knn_', 'cof'):
        with pytest.raises(YueHipError, match='unknown option'):
            dev.get_option(name)


def test_routed_options_give_their_defaults_without_subsystem_state(dev):
    for name, value in ROUTED.items():
        assert dev.get_option(name) == value, name


def test_round_tpw_follows_the_uploaded_factor_width(dev):
    words = 'yue_set_option: round_tpw must be 0, 2, 4, 8 or 16'

    def check(refused_8, refused_16):
        for value in (2, 4, 8, 16, 0):
            if value == 8 and refused_8:
                _refused(dev, 'round_tpw', 8, 'yue_set_option: round_tpw 8 needs k <= 128')
            elif value == 16 and refused_16:
                _refused(dev, 'round_tpw', 16, 'yue_set_option: round_tpw 16 needs k <= 64')
            else:
                dev.set_option('round_tpw', value)
                assert dev.get_option('round_tpw') == value
        for bad in (-2, 1, 3, 6, 12, 32):
            _refused(dev, 'round_tpw', bad, words)
        assert dev.get_option('round_tpw') == 0

    check(False, False)                                    # no factors uploaded: the whole set passes
    for k, refused_8, refused_16 in ((64, False, False), (128, False, True), (130, True, True)):
        dev.set_factors(np.zeros((3, k), np.float32), np.zeros((5, k), np.float32))
        check(refused_8, refused_16)


def test_round_cus_reserved_recreates_the_stream_and_is_restored(dev):
    _refused(dev, 'round_cus_reserved', -1, 'yue_set_option: round_cus_reserved must be 0 .. CUs - 1')
    _refused(dev, 'round_cus_reserved', 1 << 20, 'yue_set_option: round_cus_reserved must be 0 .. CUs - 1')
    assert dev.get_option('round_cus_reserved') == 0
    dev.set_option('round_cus_reserved', 1)
    assert dev.get_option('round_cus_reserved') == 1
    dev.set_option('round_cus_reserved', 0)
    assert dev.get_option('round_cus_reserved') == 0
    # the re-created stream serves the context
    P0 = np.arange(12, dtype=np.float32).reshape(3, 4)
    Q0 = np.arange(20, dtype=np.float32).reshape(5, 4)
    dev.set_factors(P0, Q0)
    P, Q = dev.get_factors()
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)
