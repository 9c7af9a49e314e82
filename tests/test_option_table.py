"""CPU: the option table (yue_amd/csrc/options_host.hip) needs no device and no subsystem, so it runs here on its own, in a
stand-alone program (tests/helpers/option_table_main.cpp) built with the host's address and undefined-behaviour sanitizers:
the defaults, flags, ranges, read-only and unknown names of tests/helpers/option_cases.py, the same tables that
tests/test_gpu_options.py drives through the C ABI.  Left out: round_cus_reserved (its setter asks the device for its CUs)
and round_tpw's cases that depend on the uploaded width (yue_set_factors)."""
import os
import shutil
import subprocess

import pytest

from helpers.option_cases import FLAGS, FLAG_VALUES, RANGES, READ_ONLY, UNKNOWN, TPW_ACCEPTED, TPW_REFUSED, TPW_WORDS, defaults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('option_table') / 'option_table')
    out = subprocess.run([hipcc, '--offload-host-only', '-x', 'hip', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-o', exe,
                          os.path.join(ROOT, 'tests', 'helpers', 'option_table_main.cpp'),
                          os.path.join(ROOT, 'yue_amd', 'csrc', 'options_host.hip')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


class Table:
    """One run of the program = one fresh context.  get / set queue a command with what it must answer; the with-block's
    end runs them all and compares, and a sanitizer report fails the run."""

    def __init__(self, exe):
        self.exe, self.lines, self.want = exe, [], []

    def get(self, name, value):
        self.lines.append('g\t%s' % name)
        self.want.append((0, str(value)))

    def get_refused(self, name):
        self.lines.append('g\t%s' % name)
        self.want.append((ERR_ARG, 'yue_get_option: unknown option ' + name))

    def set(self, name, value):
        self.lines.append('s\t%s\t%d' % (name, value))
        self.want.append((0, ''))

    def set_refused(self, name, value, message):
        self.lines.append('s\t%s\t%d' % (name, value))
        self.want.append((ERR_ARG, message))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            return False
        out = subprocess.run([self.exe], input=''.join(line + '\n' for line in self.lines), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stderr == '', out.stderr[-3000:]
        got = [tuple(line.split('\t', 1)) for line in out.stdout.split('\n')[:-1]]
        assert len(got) == len(self.want)
        for command, (rc, text), want in zip(self.lines, got, self.want):
            assert (int(rc), text) == want, command
        return False


def test_every_option_reads_its_default_on_a_value_initialised_context(program):
    with Table(program) as t:
        for name, value in defaults().items():
            if name != 'round_cus_reserved':
                t.get(name, value)


def test_flags_read_back_zero_or_one(program):
    with Table(program) as t:
        for name, default in FLAGS.items():
            for value, back in FLAG_VALUES:
                t.set(name, value)
                t.get(name, back)
            t.set(name, default)


def test_ranges_accept_their_ends_and_refuse_the_values_beside_them(program):
    with Table(program) as t:
        for name, (default, accepted, refused, words) in RANGES.items():
            for value in accepted:
                t.set(name, value)
                t.get(name, value)
                for bad in refused:
                    t.set_refused(name, bad, 'yue_set_option: ' + words)
                    t.get(name, value)                                  # a refused value changes nothing
            t.set(name, default)


def test_read_only_and_unknown_names_are_refused(program):
    with Table(program) as t:
        for name, value in READ_ONLY.items():
            for v in (0, 1):
                t.set_refused(name, v, 'yue_set_option: unknown option ' + name)
            t.get(name, value)
        for name in ('round_nonsense',) + UNKNOWN:
            t.set_refused(name, 1, 'yue_set_option: unknown option ' + name)
            t.get_refused(name)


def test_round_tpw_without_factors_takes_the_whole_set(program):
    with Table(program) as t:
        for value in TPW_ACCEPTED:
            t.set('round_tpw', value)
            t.get('round_tpw', value)
        for bad in TPW_REFUSED:
            t.set_refused('round_tpw', bad, TPW_WORDS)
        t.get('round_tpw', 0)
