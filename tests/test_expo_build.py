"""CPU: the ExpoMF kernels (yue_amd/csrc/expo_kernels.hpp) compile for gfx950 without scratch, the dense Gram kernel runs on
the f32-input MFMA, and the translation unit holds no float atomics."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expo_kernels_no_scratch_f32_mfma_no_float_atomics(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'yue_amd', 'csrc', 'expo_host.hip')
    asm = tmp_path / 'expo_host.s'
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
    kernels = {fn: u for fn, u in usage.items() if 'k_expo_' in fn}
    assert len(kernels) == 7, sorted(usage)                      # gram<2>, gram<4>, gram<6>, chunk, solve, asum, mu
    for fn, u in kernels.items():
        assert u['ScratchSize [bytes/lane]'] == 0, (fn, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 512, (fn, u)
    solve = [u for fn, u in kernels.items() if 'k_expo_solve' in fn][0]
    assert solve['LDS Size [bytes/block]'] + 128 * 129 // 2 * 8 <= 80 * 1024 and solve['VGPRs'] + solve.get('AGPRs', 0) <= 256, solve
    # per kernel: the Gram kernels multiply on the f32-input MFMA; nothing in the unit uses a float atomic
    text = open(str(asm)).read()
    bodies = {}
    for m in re.finditer(r'^(_ZN3yue\w+):[^\n]*\n(.*?)^\s*s_endpgm', text, re.S | re.M):
        bodies[m.group(1)] = m.group(2)
    grams = [b for fn, b in bodies.items() if 'k_expo_gram' in fn]
    assert len(grams) == 3
    for b in grams:
        assert b.count('v_mfma_f32_32x32x2_f32') >= 3
        assert 'bf16' not in b and 'f16' not in b.replace('v_mfma_f32_32x32x2_f32', '')
    assert not re.search(r'atomic_(add|pk_add|min|max|fadd|fmin|fmax)_(f32|f64|pk)', text)
    assert not re.search(r'atomic_add_f|atomic_pk_add', text)
    src_text = open(src).read() + open(os.path.join(os.path.dirname(src), 'expo_kernels.hpp')).read()
    assert 'atomicAdd' not in src_text
