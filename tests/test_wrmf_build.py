"""CPU: the WRMF kernels (yue_amd/csrc/wrmf_kernels.hpp) compile for gfx950 without scratch, and k_wrmf_solve fits the
residency the host assumes: two workgroups of 256 threads per CU, i.e. static + dynamic LDS <= 80 KB (160 KB per CU) and
at most 256 VGPRs (two waves per SIMD)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wrmf_kernels_no_scratch_and_lds_budget(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'wrmf_host.hip')
    out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
                          '-Rpass-analysis=kernel-resource-usage', '-o', str(tmp_path / 'wrmf_host.s'), src],
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
    kernels = {fn: u for fn, u in usage.items() if 'k_wrmf_' in fn}
    assert len(kernels) == 5, sorted(usage)
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
    solve = [u for fn, u in kernels.items() if 'k_wrmf_solve' in fn][0]
    packed_l = 128 * 129 // 2 * 8                                   # wrmf_dyn_lds(128): the packed fp64 factor
    assert solve['LDS Size [bytes/block]'] + packed_l <= 80 * 1024, solve
    assert solve['VGPRs'] + solve.get('AGPRs', 0) <= 256, solve
