"""CPU: the CoFactor kernels (yue_amd/csrc/cof_kernels.hpp) compile for gfx950 without scratch, the solve kernel's LDS fits the
occupancy its host code assumes, and the translation unit holds no float atomics."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cof_kernels_no_scratch_lds_budget_no_float_atomics(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'cof_host.hip')
    asm = tmp_path / 'cof_host.s'
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(asm), src],
                         capture_output=True, text=True, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)', line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kernels = {fn: u for fn, u in usage.items() if 'k_cof_' in fn}
    assert len(kernels) == 4, sorted(usage)                      # events, cooccur, chunk, solve
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 512, (fn, u)
    # __launch_bounds__(256, 2): two workgroups per CU share its 160 KiB of LDS and each wave may hold 256 registers
    solve = [u for fn, u in kernels.items() if 'k_cof_solve' in fn][0]
    assert solve['LDS Size [bytes/block]'] + 128 * 129 // 2 * 8 <= 80 * 1024 and solve['VGPRs'] + solve.get('AGPRs', 0) <= 256, solve
    cooccur = [u for fn, u in kernels.items() if 'k_cof_cooccur' in fn][0]
    assert cooccur['LDS Size [bytes/block]'] <= 64 * 1024, cooccur
    text = open(str(asm)).read()
    assert not re.search(r'atomic_(add|pk_add|min|max|fadd|fmin|fmax)_(f32|f64|pk)', text)
    assert not re.search(r'atomic_add_f|atomic_pk_add', text)
    # the shared library's unit list holds the unit
    assert 'cof_host' in open(os.path.join(os.path.dirname(src), 'Makefile')).read().split('UNITS')[1].splitlines()[0]
