#!/usr/bin/env python3
"""Do the adversarial scoring tests bite?  python tools/scan_margin_probe.py   (YUE_LIB=path of another build of the library)

Runs the factors of tests/helpers/bf16_adversary.py through every form of every bf16 pre-filter kernel and prints, per form,
how many users' lists (ids or scores) differ from the oracle's.  The product library must show 0 everywhere; the diagnostic
build of `make -C yue_amd/csrc margin-probe` (the margin at 0.90 of the proven bound instead of 1.01) must show differences in
EVERY form -- a form without any is one the cases do not reach.  Wrong lists are the point of that build; nothing else is.

Forms: the fused kernels (scan_batch 0 = k_topn_scan_bf16p, 1 = k_topn_scan_bf16) on catalogues below 16,384 items; on longer
ones the first chunk (k_topn_scan_bf16p over items 0 .. 511: users whose list lacks an oracle item below 512) and k_scan_filter
with one / two user blocks per wave and the DMA rows (scan_filter_ub 1 / 2 / 3; 3 is the DMA form at k = 64 and 128), without
and with the settle check (users whose list lacks an oracle item from 512 on)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import oracle  # noqa: E402
from helpers import bf16_adversary as adv  # noqa: E402
from yue_amd import _shim  # noqa: E402
from yue_amd._shim import Device  # noqa: E402

if os.environ.get('YUE_LIB'):
    _shim.LIB_PATH = os.environ['YUE_LIB']
print('library: %s' % os.path.basename(_shim.LIB_PATH))
orc = oracle.Oracle()
dev = Device(0, raise_errors=True)
totals = {}


def lacking(ids, oid, lo, hi):
    """users whose list lacks an oracle item with lo <= id < hi"""
    return int(sum(1 for a, b in zip(ids, oid) if set(x for x in b.tolist() if lo <= x < hi) - set(a.tolist())))


def report(form, fam, n, k, N, count, extra=''):
    totals[form] = totals.get(form, 0) + count
    print('%-46s %-8s n=%-6d k=%-4d N=%-3d users differing: %4d%s' % (form, fam, n, k, N, count, extra), flush=True)


for k in adv.KS:
    for fam, n, N in (('under', 4096, 5), ('spikes', 4099, 20), ('mixed', 4099, 64)):
        m = adv.M_FUSED
        P, Q, mp, mi = adv.make(fam, m, n, k)
        users = np.arange(m, dtype=np.int32)
        oid, osc, _ = orc.topn_scan(P, Q, users, N, mp, mi)
        dev.set_factors(P, Q)
        for batch in (0, 1):
            dev.set_option('scan_batch', batch)
            ids, sc = dev.topn_scan(users, N, mp, mi)
            dev.set_option('scan_batch', 0)
            report('fused, scan_batch %d' % batch, fam, n, k, N, int(((ids != oid) | (sc != osc)).any(axis=1).sum()))
    for fam, N in (('under', 20), ('spikes', 5), ('settling', 5)):
        m, n = adv.M_TWO_PHASE, adv.N_TWO_PHASE
        P, Q, mp, mi = adv.make(fam, m, n, k)
        users = np.arange(m, dtype=np.int32)
        oid, osc, _ = orc.topn_scan(P, Q, users, N, mp, mi)
        dev.set_factors(P, Q)
        for ub in (3, 2, 1):
            dev.set_option('scan_filter_ub', ub)
            ids, sc = dev.topn_scan(users, N, mp, mi)
            dev.set_option('scan_filter_ub', 3)
            settle = dev.get_option('scan_last_settle')
            assert dev.get_option('scan_last_chunks') >= 2
            dma = ub == 3 and k in (64, 128)
            form = 'k_scan_filter ub %d%s, settle %d' % (min(ub, 2), ' DMA' if dma else '', settle)
            if ub == 3 and not dma:
                form += ' (ub 3 asked)'
            report(form, fam, n, k, N, lacking(ids, oid, 512, n), '   (any difference: %d)' % int(((ids != oid) | (sc != osc)).any(axis=1).sum()))
            if ub == 3:
                report('first chunk, k_topn_scan_bf16p', fam, n, k, N, lacking(ids, oid, 0, 512))
dev.close()
print()
for form in sorted(totals):
    print('TOTAL %-46s %6d' % (form, totals[form]))
print('forms without a difference: %d of %d' % (sum(1 for v in totals.values() if v == 0), len(totals)))
