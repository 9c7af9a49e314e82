"""The compiler's per-kernel resource report (-Rpass-analysis=kernel-resource-usage), as the build tests read it."""
import os
import re


def parse_resource_usage(stderr):
    """{mangled function name: {'VGPRs' | 'AGPRs' | 'ScratchSize [bytes/lane]' | 'LDS Size [bytes/block]': int}}"""
    usage, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)', line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return usage


def kernel_sources(root, header):
    """The text of a ranking kernel's own header and of the workgroup helpers it calls (yue_amd/csrc/wg_rank.hpp)."""
    return ''.join(open(os.path.join(root, 'yue_amd', 'csrc', f)).read() for f in (header, 'wg_rank.hpp'))


def has_device_assert(text):
    """`assert(` in device source; a compile-time `static_assert(` is not one."""
    return re.search(r'(?<!static_)assert\(', text) is not None
