"""CPU: the UserKNN kernels (yue_amd/csrc/knn_kernels.hpp) compile for gfx950 without scratch, and their LDS fits the
residency the host assumes: two workgroups of 256 threads per CU, i.e. at most 80 KB of LDS each (160 KB per CU)."""
import os
import re
import shutil
import subprocess

from helpers.resource_usage import has_device_assert, kernel_sources, parse_resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_kernels_no_scratch_and_lds_budget(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'knn_host.hip')
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'knn_host.s'), src],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    usage = parse_resource_usage(out.stderr)
    kernels = {fn: u for fn, u in usage.items() if 'k_knn_' in fn}
    assert len(kernels) == 3, sorted(usage)
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
        assert u['LDS Size [bytes/block]'] <= 80 * 1024, (fn, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (fn, u)
    # no float atomics, no traps, no device asserts in the UserKNN sources (the kernels' header and the shared workgroup helpers)
    text = kernel_sources(ROOT, 'knn_kernels.hpp')
    assert 'wg_reform' in text
    assert has_device_assert('  assert(x);') and has_device_assert('__assert(x)') and not has_device_assert('static_assert(x, "")')
    assert not re.search(r'atomicAdd\(\s*&?\s*(ss|sim|sum|den)', text) and '__builtin_trap' not in text and not has_device_assert(text)
