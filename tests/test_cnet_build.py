"""CPU: the library exports the user-network stage (yue_cnet_*), and its kernels (yue_amd/csrc/cnet_kernels.hpp) compile
for gfx950 without scratch, within 64 KiB of static LDS, with no float atomics."""
import ctypes
import os
import re
import shutil
import subprocess

from helpers.resource_usage import has_device_assert, kernel_sources, parse_resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['yue_cnet_set_pairs', 'yue_cnet_walks', 'yue_cnet_set_walks', 'yue_cnet_embed', 'yue_cnet_set_embedding', 'yue_cnet_friends']


def test_library_exports_the_cnet_symbols():
    import __graft_entry__
    __graft_entry__.build()
    from yue_amd import _shim
    lib = ctypes.CDLL(_shim.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _shim.SYMBOLS, name


def test_cnet_kernels_no_scratch_lds_budget_no_float_atomics(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'cnet_host.hip')
    asm = tmp_path / 'cnet_host.s'
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(asm), src],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    usage = parse_resource_usage(out.stderr)
    kernels = {fn: u for fn, u in usage.items() if 'k_cnet_' in fn}
    # prefix, walk, count, embed_init, embed_round<1>, embed_round<2>, embed_apply, norms, friends
    assert len(kernels) == 9, sorted(usage)
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
        assert u['LDS Size [bytes/block]'] <= 64 * 1024, (fn, u)
    wide = [u for fn, u in kernels.items() if 'k_cnet_embed_roundILi2EE' in fn]
    assert len(wide) == 1 and wide[0]['ScratchSize [bytes/lane]'] == 0 and wide[0]['VGPRs'] + wide[0].get('AGPRs', 0) <= 128, wide
    text = open(str(asm)).read()
    assert not re.search(r'atomic_(add|pk_add|min|max|fadd|fmin|fmax)_(f32|f64|pk)', text)
    assert not re.search(r'atomic_add_f|atomic_pk_add', text)
    src_text = kernel_sources(ROOT, 'cnet_kernels.hpp')
    assert 'wg_bitonic' in src_text
    assert '__builtin_trap' not in src_text and not has_device_assert(src_text)
    assert 'cnet_host' in open(os.path.join(os.path.dirname(src), 'Makefile')).read().split('UNITS')[1].splitlines()[0]
