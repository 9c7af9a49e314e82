#!/usr/bin/env python3
"""How long NGCF's float32 training stays with fp64 (CPU only; DESIGN.md section 21, tests/helpers/ngcf_e2e.py).

For both end-to-end problems, at batch_size 128 and two epochs, and for several seeds of the start values and the sampler: the
float32 contract (tests/helpers/numpy_ngcf.py) and the fp64 contract are trained side by side for 1, 2, 3, 5, 10 and 30 steps
and propagated once; printed are the largest |F32 - F64| (absolute and relative) and how many test users the near-tie rule of
tests/helpers/lightgcn_e2e.py leaves out at that distance (cap: 5 %).  One JSON line per (problem, seed, steps).

    python tools/ngcf_e2e_drift.py [--seeds 4] [--steps 1,2,3,5,10,30] [--batch 128]
"""
import argparse
import contextlib
import io
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import ngcf_e2e as ne             # noqa: E402
from helpers import numpy_ngcf as ng           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=4)
    ap.add_argument('--steps', default='1,2,3,5,10,30')
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    tmp = pathlib.Path(tempfile.mkdtemp())
    for name in sorted(ne.PROBLEMS):
        p = ne.PROBLEMS[name]
        ne.PROBLEMS[name] = p[:6] + (2, args.batch) + p[8:]
        for seed in range(p[4], p[4] + args.seeds):
            with contextlib.redirect_stdout(io.StringIO()):
                rec, _ = ne.plugin_on_cpu(tmp, name, seed)
            N = max(rec._top_list())
            names, uids, mp, mi = ne.ranked_users(rec)
            for steps in (int(x) for x in args.steps.split(',')):
                F64, batches = ne.contract_F(rec, rec.U, rec.V, rec.W, seed, np.float64, steps)
                F32, _ = ne.contract_F(rec, rec.U, rec.V, rec.W, seed, np.float32, steps)
                keep, dist = ne.compared_users(F64, rec.m, uids, mp, mi, N, F32)
                print(json.dumps({'problem': name, 'k': rec.k, 'seed': seed, 'steps': len(batches), 'F_abs': dist, 'F_rel': ng.rel(F32, F64),
                                  'test_users': len(uids), 'left_out': int((~keep).sum())}), flush=True)


if __name__ == '__main__':
    main()
