"""CPU: device buffers, events and subsystem states are owned by RAII types of yue_amd/csrc/host_common.hpp and by nothing
else.  Read from the sources: a new subsystem cannot bring back a hand-written list of things to free."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'yue_amd', 'csrc')
OWNER = 'host_common.hpp'


def code(path):
    """The file without its comments (no string of these sources holds a comment marker)."""
    with open(path) as f:
        text = f.read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.hpp')))
    assert len(paths) > 30 and any(os.path.basename(p) == OWNER for p in paths)
    return {os.path.basename(p): code(p) for p in paths}


def test_raw_allocation_and_event_calls_live_in_one_header():
    calls = ('hipMalloc(', 'hipFree(', 'hipEventCreate', 'hipEventCreateWithFlags', 'hipEventDestroy')
    src = sources()
    for call in calls:
        assert call in src[OWNER], call
    found = [(name, call) for name, text in src.items() if name != OWNER for call in calls if call in text]
    assert not found, found


def test_nothing_releases_by_hand():
    src = sources()
    # a member function named release: its definition, `void release(` or `release() {`, inside a class or out of it
    definition = re.compile(r'\brelease\s*\([^;{)]*\)\s*(const\s*)?\{')
    assert definition.search(src[OWNER])
    found = [name for name, text in src.items() if name != OWNER and definition.search(text)]
    assert not found, found
    core = src['core_host.hip']
    start = core.index('int yue_ctx_destroy(')
    body = core[start:core.index('\n}\n', start)]
    assert 'delete c;' in body and 'hipStreamDestroy' in body and '.release()' not in body and '->release()' not in body


def test_upload_and_download_are_defined_once():
    src = sources()
    for name, overloads in (('upload', 2), ('download', 1)):
        definition = re.compile(r'^(?:inline\s+)?int\s+%s\s*\(' % name, re.M)
        counts = {f: len(definition.findall(text)) for f, text in src.items() if definition.search(text)}
        assert counts == {OWNER: overloads}, (name, counts)


def test_row_lists_are_checked_in_one_place():
    # the hand-written row-list checks are gone for good, and the transpose walk is written once
    src = sources()
    definition = re.compile(r'\b(check_csr|check_lists|check_side|fism_check_rows)\s*\([^;{)]*\)\s*\{')
    found = [(name, m.group(1)) for name, text in src.items() if name != 'input_checks.hpp' for m in definition.finditer(text)]
    assert not found, found
    assert re.search(r'\bint\s+check_rows\s*\(', src['input_checks.hpp'])
    assert [name for name, text in src.items() if 'not the transpose' in text] == ['input_checks.hpp']
