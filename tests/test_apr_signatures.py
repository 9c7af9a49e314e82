"""CPU: APR's C ABI stands in a header of its own (include/yue_apr.h, which include/yue_hip.h includes) and its signatures in a table
of their own (APR_SIGNATURES of yue_amd/_shim.py).  What tests/test_shim_signatures.py and tests/test_abi.py hold for yue_hip.h and
SIGNATURES is held here for that pair, with the same reader: the table equals the header type by type, the comparison sees one
retyped parameter, the library exports every function, and load_library() sets restype and argtypes from the table."""
import ctypes
import os
import re
import types

from test_shim_signatures import ROOT, declared, differing


def header():
    with open(os.path.join(ROOT, 'include', 'yue_apr.h')) as f:
        return f.read()


def table():
    from yue_amd import _shim
    return types.SimpleNamespace(SIGNATURES=_shim.APR_SIGNATURES)


def test_the_apr_table_equals_its_header_type_by_type():
    from yue_amd import _shim
    want = declared(header())
    assert len(want) == 8 and all(name.startswith('yue_apr_') for name in want)
    assert want['yue_apr_times'] == ('int', ['ctx', 'i64*']) and want['yue_apr_grad'][1][:2] == ['ctx', 'int']
    assert differing(table(), header()) == []
    assert not set(_shim.APR_SIGNATURES) & set(_shim.SIGNATURES)
    # the main header includes this one after its types, and declares none of these functions itself
    with open(os.path.join(ROOT, 'include', 'yue_hip.h')) as f:
        main = f.read()
    assert main.count('#include "yue_apr.h"') == 1 and main.index('typedef struct yue_ctx yue_ctx;') < main.index('#include "yue_apr.h"')
    assert not re.search(r'\byue_apr_\w+\s*\(', main)


def test_the_comparison_sees_one_retyped_parameter():
    old = 'int yue_apr_times(yue_ctx *ctx, int64_t *ns_out);'
    assert old in header()
    assert differing(table(), header().replace(old, old.replace('int64_t *', 'int32_t *'))) == ['yue_apr_times']
    assert differing(table(), header().replace(old, '')) == ['yue_apr_times']


def test_the_library_exports_the_header_and_load_library_types_every_call():
    import __graft_entry__
    __graft_entry__.build()
    from yue_amd import _shim
    lib = _shim.load_library()
    raw = ctypes.CDLL(_shim.LIB_PATH)
    for name, (returns, params) in declared(header()).items():
        assert hasattr(raw, name), 'libyue_hip.so lacks ' + name
        fn = getattr(lib, name)
        assert fn.restype is _shim.TYPES[returns], name
        assert len(fn.argtypes) == len(params) and all(a is _shim.TYPES[p] for a, p in zip(fn.argtypes, params)), name
