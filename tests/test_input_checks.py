"""CPU: the checks of uploaded row lists (yue_amd/csrc/input_checks.hpp) need no device, so they run here
in a stand-alone program (tests/helpers/input_checks_main.cpp) built with the host's address and undefined-behaviour
sanitizers.  Every array the program hands them is a heap allocation of exactly its stated length: a check that reads an id
before the whole pointer has been walked is reported by the sanitizer, and any sanitizer output fails the run.  The lists
hold at most three rows and six ids."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('input_checks') / 'input_checks')
    out = subprocess.run([hipcc, '--offload-host-only', '-x', 'hip', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-o', exe,
                          os.path.join(ROOT, 'tests', 'helpers', 'input_checks_main.cpp')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def text(v):
    if isinstance(v, (list, tuple)):
        return ','.join(str(x) for x in v) if len(v) else '-'
    return '-' if v is None else str(v)                           # (a null array is the string 'null')


class Checks:
    """One run of the program.  rows / transpose / ids queue a command with what it must answer: None for accepted, else the
    words the refusal must hold (all of them, and the text must start with the entry's name).  The with-block's end runs them
    all and compares; a sanitizer report fails the run."""

    def __init__(self, exe):
        self.exe, self.lines, self.want = exe, [], []

    def rows(self, want, ptr, ids, bound, total=None, order='ascending', max_row=None, rule=None):
        rows = 1 if ptr == 'null' else len(ptr) - 1
        self.lines.append('\t'.join(['rows', text(ptr), str(rows), text(ids), str(bound), text(total), order, text(max_row), text(rule)]))
        self.want.append(want)

    def transpose(self, want, u_ptr, u_items, i_ptr, i_users, differ=None):
        self.lines.append('\t'.join(['transpose', str(len(u_ptr) - 1), text(u_ptr), text(u_items), str(len(i_ptr) - 1), text(i_ptr), text(i_users),
                                     '-' if differ is None else '%d:%d' % differ]))
        self.want.append(want)

    def ids(self, want, ids, bound):
        self.lines.append('\t'.join(['ids', text(ids), str(bound)]))
        self.want.append(want)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            return False
        out = subprocess.run([self.exe], input=''.join(line + '\n' for line in self.lines), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stderr == '', out.stderr[-3000:]
        got = [line.split('\t', 1) for line in out.stdout.split('\n')[:-1]]
        assert len(got) == len(self.want)
        for command, (rc, message), want in zip(self.lines, got, self.want):
            if want is None:
                assert (int(rc), message) == (0, ''), command
            else:
                assert int(rc) == ERR_ARG and message.startswith('entry') and all(w in message for w in want), (command, message)
        return False


ORDERS = ('any', 'distinct', 'ascending')


def test_accepted_lists(program):
    with Checks(program) as c:
        for order in ORDERS:
            for total in (None, 0):
                c.rows(None, [0, 0], 'null', 3, total, order)                       # the empty list: one row, no ids at all
                c.rows(None, [0, 0, 0, 0], 'null', 3, total, order)
            for ptr in ([0, 0, 1, 2], [0, 1, 1, 2], [0, 1, 2, 2]):                 # an empty first, middle, last row
                for total in (None, 2):
                    c.rows(None, ptr, [1, 2], 3, total, order)
            c.rows(None, [0, 4], [0, 1, 2, 3], 4, 4, order)                         # one row holds every id; the last is bound - 1
            c.rows(None, [0, 1, 3], [3, 0, 3], 4, None, order)                      # bound - 1 twice, in two rows
        c.rows(None, [0, 3], [1, 0, 1], 2, None, 'any')                             # a repeat is in order where no order is asked
        c.rows(None, [0, 2, 4], [2, 0, 0, 2], 3, None, 'distinct')                  # distinct in any order, the same ids in the next row


def test_refused_ids(program):
    with Checks(program) as c:
        for order in ORDERS:
            c.rows(['id out of range', '(row 1)'], [0, 1, 3], [0, 1, 4], 4, None, order)        # id == bound
            c.rows(['id out of range', '(row 0)'], [0, 1, 3], [-1, 1, 2], 4, None, order)
            c.rows(['id out of range', '(row 2)'], [0, 0, 0, 1], [1], 1, 1, order)
        c.rows(['sorted and unique', '(row 1)'], [0, 2, 4], [0, 1, 2, 2], 4)                    # equal neighbours
        c.rows(['sorted and unique', '(row 0)'], [0, 2, 4], [1, 0, 2, 3], 4)                    # a descending pair
        c.rows(None, [0, 2, 4], [2, 3, 0, 1], 4)                                                # ... but every row starts afresh
        c.rows(['distinct', '(row 0)'], [0, 3], [1, 0, 1], 2, None, 'distinct')                 # a repeat two positions apart
        c.rows(['distinct', '(row 1)'], [0, 1, 4], [1, 1, 0, 1], 2, None, 'distinct')


def test_a_falling_pointer_is_refused_before_any_id_is_read(program):
    five = [0, 1, 2, 3, 4]
    with Checks(program) as c:
        for order in ORDERS:
            c.rows(['non-decreasing', '(row 1)'], [0, 100, 5], five, 5, 5, order)               # row 0 alone looks fine: ids[5 .. 99] do not exist
            c.rows(['non-decreasing', '(row 1)'], [0, 100, 5], five, 5, None, order)
            c.rows(['non-decreasing', '(row 1)'], [0, 3, 2, 5], five, 5, None, order)
            c.rows(['non-decreasing', '(row 1)'], [0, 3, 2, 5], five, 5, 5, order)
            c.rows(['non-decreasing', '(row 0)'], [0, -1], 'null', 5, None, order)
        c.rows(['non-decreasing'], [0, 100, 5], five, 5, 5, 'ascending', None, 0)               # nor does the rule see an entry


def test_other_pointer_and_argument_faults(program):
    with Checks(program) as c:
        for total in (None, 3):
            c.rows(['must start at 0'], [1, 2, 3], [0, 1, 2], 3, total)
            c.rows(['null pointer array'], 'null', [0, 1, 2], 3, total)
            c.rows(['null id array'], [0, 1, 3], 'null', 3, total)
        c.rows(['must run from 0 to nnz'], [0, 1, 3], [0, 1, 2], 3, 2)                          # ids beyond the total are the caller's, unread
        c.rows(['must run from 0 to nnz'], [0, 1, 2], [0, 1], 3, 3)                             # ... and a total beyond the pointer names no id
        c.rows(['must run from 0 to nnz'], [0, 0], 'null', 3, 1)
        c.rows(['row 1 is too long', 'limit 2'], [0, 2, 5], [0, 1, 0, 1, 2], 3, None, 'ascending', 2)
        c.rows(None, [0, 2, 5], [0, 1, 0, 1, 2], 3, None, 'ascending', 3)                       # exactly at the limit
        c.rows(['non-decreasing', '(row 1)'], [0, 100, 5], [0, 1, 2, 3, 4], 5, 5, 'any', 99)    # a fall is said before a length
        c.rows(['row 0 is too long', 'limit 1'], [0, 2, 5], [0, 1, 0, 1, 2], 3, None, 'ascending', 1)   # the first of two such rows
        for e, row in ((0, 0), (2, 1), (4, 2)):
            c.rows(['row %d: the rule\'s words' % row], [0, 2, 3, 5], [0, 1, 2, 0, 1], 3, 5, 'ascending', None, e)
        c.rows(None, [0, 2, 3, 5], [0, 1, 2, 0, 1], 3, 5, 'ascending', None, 5)                 # the rule is asked about entries 0 .. 4 only
        c.rows(['id out of range'], [0, 2, 3, 5], [0, 3, 2, 0, 1], 3, 5, 'ascending', None, 1)  # the id's fault comes before the rule's


def test_transpose(program):
    # users 0: {0, 1}, 1: {1}, 2: {0}; items 0: {0, 2}, 1: {0, 1}
    u_ptr, u_items, i_ptr, i_users = [0, 2, 3, 4], [0, 1, 1, 0], [0, 2, 4], [0, 2, 0, 1]
    words = 'not the transpose'
    with Checks(program) as c:
        c.transpose(None, u_ptr, u_items, i_ptr, i_users)
        c.transpose(None, [0, 0], 'null', [0, 0, 0], 'null')
        c.transpose([words, '(item 1)'], u_ptr, u_items, i_ptr, [0, 2, 0, 2])                   # item 1 names user 2 where user 1 stands
        c.transpose([words, '(item 0)'], u_ptr, u_items, i_ptr, [0, 1, 0, 1])
        # item 0 one short and item 1 one long: user 2's pair finds item 0's row full
        c.transpose([words, '(item 0)'], u_ptr, u_items, [0, 1, 4], [0, 0, 1, 2])
        # item 1 one short, item 0 one long: user 1's pair finds item 1's row full
        c.transpose([words, '(item 1)'], u_ptr, u_items, [0, 3, 4], [0, 2, 2, 0])
        c.transpose([words, '(item 1)'], u_ptr, u_items, i_ptr, i_users, differ=(2, 3))         # user 1's pair with item 1 differs in its value
        c.transpose([words, '(item 0)'], u_ptr, u_items, i_ptr, i_users, differ=(3, 1))
        c.transpose(None, u_ptr, u_items, i_ptr, i_users, differ=(3, 0))                        # pairs the walk never compares


def test_flat_ids(program):
    with Checks(program) as c:
        c.ids(None, [], 3)
        c.ids(None, [2, 0, 2], 3)
        c.ids(['id out of range', '(position 1)'], [0, 3], 3)
        c.ids(['id out of range', '(position 2)'], [0, 1, -1], 3)
