"""CPU: yue_amd/_shim.py declares every library call's C signature once (SIGNATURES), the table equals include/yue_hip.h type
by type, load_library() turns it into restype / argtypes, the pointer argument types refuse what the library must not be
handed, and no call site marshals by hand any more (read from the source, as tests/test_host_ownership.py does)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's parameter types, const dropped and blanks removed -> the table's spelling
C_TYPES = {'yue_ctx*': 'ctx', 'yue_ctx**': 'ctx*', 'char*': 'str', 'void*': 'void*',
           'int': 'int', 'int32_t': 'i32', 'uint32_t': 'u32', 'int64_t': 'i64', 'uint64_t': 'u64', 'double': 'f64',
           'float*': 'f32*', 'double*': 'f64*', 'int32_t*': 'i32*', 'int64_t*': 'i64*', 'int*': 'int*', 'float**': 'f32**'}


def header():
    with open(os.path.join(ROOT, 'include', 'yue_hip.h')) as f:
        return f.read()


def spelled(ctype):
    return C_TYPES[re.sub(r'\bconst\b|\s', '', ctype)]


def declared(text):
    """{function: (return type, [parameter types])} of every prototype of the header, in the table's spelling."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = {}
    for returns, name, params in re.findall(r'^((?:const\s+)?\w+\s*\*?)\s*(yue_\w+)\s*\(([^)]*)\)\s*;', text, re.M):
        params = [] if params.strip() == 'void' else [re.sub(r'\w+$', '', p.strip()) for p in params.split(',')]
        out[name] = (spelled(returns), [spelled(p) for p in params])
    return out


def table(shim):
    """The same of the shim's table: a missing '-> type' means int."""
    out = {}
    for name, signature in shim.SIGNATURES.items():
        params, _, returns = signature.partition('->')
        out[name] = (returns.strip() or 'int', params.split())
    return out


def differing(shim, text):
    want, have = declared(text), table(shim)
    return sorted(name for name in set(want) | set(have) if want.get(name) != have.get(name))


def test_the_table_equals_the_header_type_by_type():
    from yue_amd import _shim
    want = declared(header())
    assert len(want) == 88 and want['yue_last_error'] == ('str', []) and want['yue_cdae_get_params'][1] == ['ctx'] + ['f32**'] * 3
    assert differing(_shim, header()) == []
    assert _shim.SYMBOLS == list(_shim.SIGNATURES)


def test_the_comparison_sees_one_retyped_parameter():
    from yue_amd import _shim
    old = 'int yue_scores(yue_ctx *ctx, int32_t user, float *out_n);'
    assert old in header()
    assert differing(_shim, header().replace(old, old.replace('int32_t user', 'int64_t user'))) == ['yue_scores']
    assert differing(_shim, header().replace(old, old.replace('float *', 'double *'))) == ['yue_scores']
    assert differing(_shim, header().replace(old, old.replace('int32_t user, ', ''))) == ['yue_scores']


def test_load_library_sets_restype_and_argtypes_from_the_table():
    import __graft_entry__
    __graft_entry__.build()
    from yue_amd import _shim
    lib = _shim.load_library()
    for name, (returns, params) in declared(header()).items():
        fn = getattr(lib, name)
        assert fn.restype is _shim.TYPES[returns], name
        assert len(fn.argtypes) == len(params) and all(a is _shim.TYPES[p] for a, p in zip(fn.argtypes, params)), name


POINTERS = [('f32*', C.c_float, np.float32, C.c_double, np.float64), ('f64*', C.c_double, np.float64, C.c_float, np.float32),
            ('i32*', C.c_int32, np.int32, C.c_int64, np.int64), ('i64*', C.c_int64, np.int64, C.c_int32, np.int32),
            ('int*', C.c_int, np.intc, C.c_int64, np.int64)]


@pytest.mark.parametrize('code, elem, dtype, other_elem, other_dtype', POINTERS, ids=[p[0] for p in POINTERS])
def test_pointer_types_take_their_own_element_type_and_nothing_else(code, elem, dtype, other_elem, other_dtype):
    from yue_amd import _shim
    ptr = _shim.TYPES[code]
    assert ptr.from_param(None) is None
    for good in (C.byref(elem()), (elem * 3)(), np.zeros(4, dtype), np.zeros((2, 3), dtype), np.zeros(0, dtype)):
        assert ptr.from_param(good) is not None
    a = np.arange(8).astype(dtype)
    assert C.cast(ptr.from_param(a), C.POINTER(elem))[5] == 5            # the array's own memory
    bad = (np.zeros(4, other_dtype), np.zeros(8, dtype)[::2], np.zeros((4, 4), dtype).T, np.asfortranarray(np.zeros((2, 3), dtype)),
           C.byref(other_elem()), (other_elem * 3)(), [0, 1, 2], 0)
    for x in bad:
        with pytest.raises(TypeError):
            ptr.from_param(x)


def test_a_call_refuses_a_wrong_array_before_the_library_sees_it():
    # yue_epoch_plan needs no device: its three outputs are int64_t *
    import __graft_entry__
    __graft_entry__.build()
    from yue_amd import _shim
    lib = _shim.load_library()
    out = np.zeros(3, np.int64)
    assert lib.yue_epoch_plan(1000, 16, 64, 5000.0, 1, out[0:], out[1:], out[2:]) == 0 and out[0] > 0
    with pytest.raises(C.ArgumentError):
        lib.yue_epoch_plan(1000, 16, 64, 5000.0, 1, np.zeros(1, np.int32), out[1:], out[2:])
    with pytest.raises(C.ArgumentError):
        lib.yue_epoch_plan(1000.5, 16, 64, 5000.0, 1, out[0:], out[1:], out[2:])


def source():
    with open(os.path.join(ROOT, 'yue_amd', '_shim.py')) as f:
        return f.read()


def test_call_sites_do_not_marshal_by_hand():
    src = source()
    # an array's address is taken in the pointer type; one more place builds the arrays of pointers of yue_cdae_get_params
    start = src.index('class _Pointer')
    end = re.compile(r'^\S', re.M).search(src, src.index('\n', start) + 1).start()      # the next line that is not indented
    assert 'from_param' in src[start:end] and 'from_param' not in src[:start] + src[end:]
    assert src[:start].count('data_as(') + src[end:].count('data_as(') <= 1
    # no ctypes scalar is built from a value: the only ones are the empty output cells handed over by byref
    assert re.findall(r'\bC\.c_\w+\(\s*[^)\s]', src) == []
    cells = set(re.findall(r'\bC\.(c_\w+)\(\)', src))
    assert cells and cells <= {'c_double', 'c_int64', 'c_int', 'c_void_p'}, cells
    assert src.count('np.zeros(1') == 1
    assert 'getattr(self, ' not in src
