"""yue_get_option / yue_set_option through the C ABI: every option's default, what it accepts, what it refuses and with which
words.  The expectations are the hand-written tables of tests/helpers/option_cases.py, which tests/test_option_table.py
drives through the table alone on the CPU; here they meet a context on a device."""
import re

import numpy as np
import pytest

from helpers.option_cases import FLAGS, FLAG_VALUES, RANGES, READ_ONLY, UNKNOWN, TPW_ACCEPTED, TPW_REFUSED, TPW_WORDS, defaults

pytestmark = pytest.mark.gpu


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
    # (the subsystems' options among them: no subsystem has any state when they are read)
    for name, value in defaults().items():
        assert dev.get_option(name) == value, name


def test_flags_read_back_zero_or_one(dev):
    for name, default in FLAGS.items():
        for value, back in FLAG_VALUES:
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
    for name in UNKNOWN:
        with pytest.raises(YueHipError, match=re.escape('yue_get_option: unknown option ' + name) + '$'):
            dev.get_option(name)
        _refused(dev, name, 1, 'yue_set_option: unknown option ' + name)


def test_routed_options_give_their_defaults_without_subsystem_state(dev):
    # (once routed to their subsystems by prefix, rows of the table now: the same five values as RANGES holds)
    for name, value in {'wrmf_long_pairs': 2048, 'knn_range': 4096, 'ipf_slots': 1024, 'expo_gram_mb': 512, 'cof_cooccur_mb': 1024}.items():
        assert dev.get_option(name) == value == RANGES[name][0], name


def test_round_tpw_follows_the_uploaded_factor_width(dev):
    def check(refused_8, refused_16):
        for value in TPW_ACCEPTED:
            if value == 8 and refused_8:
                _refused(dev, 'round_tpw', 8, 'yue_set_option: round_tpw 8 needs k <= 128')
            elif value == 16 and refused_16:
                _refused(dev, 'round_tpw', 16, 'yue_set_option: round_tpw 16 needs k <= 64')
            else:
                dev.set_option('round_tpw', value)
                assert dev.get_option('round_tpw') == value
        for bad in TPW_REFUSED:
            _refused(dev, 'round_tpw', bad, TPW_WORDS)
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
