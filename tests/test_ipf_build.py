"""CPU: the IPF kernel (yue_amd/csrc/ipf_kernels.hpp) compiles for gfx950 without scratch, within the LDS budget the host
assumes (a 1,024-workgroup launch keeps four 256-thread workgroups per CU: at most 40 KB of LDS each), with no float
atomics, no traps and no device asserts."""
import os
import re
import shutil
import subprocess

from helpers.resource_usage import has_device_assert, kernel_sources, parse_resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ipf_kernel_no_scratch_lds_budget_no_float_atomics(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'ipf_host.hip')
    asm = tmp_path / 'ipf_host.s'
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(asm), src],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    usage = parse_resource_usage(out.stderr)
    kernels = {fn: u for fn, u in usage.items() if 'k_ipf_' in fn}
    assert len(kernels) == 1, sorted(usage)
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
        assert u['LDS Size [bytes/block]'] <= 40 * 1024, (fn, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (fn, u)
    text = asm.read_text()
    atomics = set(re.findall(r'\b(global_atomic_\w+|flat_atomic_\w+|buffer_atomic_\w+|ds_\w*(?:add|max|min)\w*)', text))
    assert 'global_atomic_umax_x2' in atomics, atomics                      # the level-2 / level-3 64-bit integer max
    assert not [a for a in atomics if re.search(r'f32|f64|bf16|pk_add|cmpswap', a)], atomics
    assert 's_trap' not in text
    src_text = kernel_sources(ROOT, 'ipf_kernels.hpp')
    assert 'wg_reform' in src_text
    assert '__builtin_trap' not in src_text and not has_device_assert(src_text)
