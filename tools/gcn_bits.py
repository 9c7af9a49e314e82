#!/usr/bin/env python3
"""The bits LightGCN's and NGCF's device paths give on a few small cases, as SHA-256 digests: one JSON object on stdout.

    python tools/gcn_bits.py > tests/golden/g19_gcn_bits.json      (YUE_LIB=path of another build of the library)

A digest is over the raw little-endian bytes of an output array, or over float.hex() of a loss.  The cases are existing ones of
tests/helpers/lightgcn_cases.py and tests/helpers/ngcf_cases.py, chosen for the paths they take:
  LightGCN  k20 (KR 1), k65 (KR 2 with a row tail), deg_k64 at lgcn_hub 96 (hubs, uneven parts, degrees 95 / 96 / 97), T1 (a one-triplet batch)
  NGCF      k33 (KP 64, k odd), k85 (2 layers, width 255: the minibatch's KR 4 instances), deg_written at ngcf_hub 96 (A != A^T, hubs
            on both), eval (no dropout)
and one LightGCN case run after an NGCF case on the same Device.  Per case: the propagation's outputs, the loss and gradients
of one minibatch, and the state after adam_reset and two steps.  tests/test_gpu_gcn_bits.py compares with the committed file:
the kernels promise fixed summation orders (DESIGN.md sections 20 and 21), so a change that moves no sum moves no digest.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import lightgcn_cases as lc       # noqa: E402
from helpers import ngcf_cases as nc           # noqa: E402
from yue_amd import _shim                      # noqa: E402
from yue_amd._shim import Device               # noqa: E402
if os.environ.get('YUE_LIB'):
    _shim.LIB_PATH = os.environ['YUE_LIB']

LIGHTGCN = ['k20', 'k65', 'deg_k64', 'T1']
NGCF = ['k33', 'k85', 'deg_written', 'eval']
AFTER = ('k32', 'k64')                         # the NGCF case, then the LightGCN case on the same Device
LR = 0.002


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder('<'), copy=False).tobytes()).hexdigest()


def sha_loss(x):
    return hashlib.sha256(float(x).hex().encode()).hexdigest()


def lightgcn_upload(dev, c):
    g = c['g']
    dev.set_option('lgcn_hub', c['hub'] if c['hub'] else 1024)
    dev.set_factors(c['U'], c['V'])
    dev.lgcn_set_graph(c['m'], c['n'], g['u_ptr'], g['u_items'], g['u_w'], g['i_ptr'], g['i_users'], g['i_w'])


def ngcf_upload(dev, c):
    g = c['g']
    dev.set_option('ngcf_hub', c['hub'] if c['hub'] else 1024)
    dev.set_factors(c['U'], c['V'])
    dev.ngcf_set_graph(c['m'], c['n'], g['ptr'], g['col'], g['w'])
    dev.ngcf_set_weights(c['W'])


def lightgcn_grad(dev, c):
    loss, gU, gV = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    return {'loss': sha_loss(loss), 'gU': sha(gU), 'gV': sha(gV)}


def lightgcn_digests(dev, name):
    c = lc.build(name)
    lightgcn_upload(dev, c)
    E, F = dev.lgcn_propagate(c['layers'], raw=True)
    out = {'E': sha(E), 'F': sha(F)}
    out.update(lightgcn_grad(dev, c))
    lightgcn_upload(dev, c)
    dev.adam_reset()
    for t in (1, 2):
        out['step%d_loss' % t] = sha_loss(dev.lgcn_step(c['layers'], c['u'], c['i'], c['j'], LR, lc.REG, t))
    for key, a in zip(('U', 'V'), dev.get_factors()):
        out['step2_' + key] = sha(a)
    for key, a in zip(('mU', 'vU', 'mV', 'vV'), dev.adam_get_moments()):
        out['step2_' + key] = sha(a)
    return out


def ngcf_grad(dev, c):
    loss, gU, gV, gW = dev.ngcf_grad(c['layers'], c['training'], c['keep'], c['mask_seed'], c['step'], c['u'], c['i'], c['j'], nc.REG)
    return {'loss': sha_loss(loss), 'gU': sha(gU), 'gV': sha(gV), 'gW': sha(gW)}


def ngcf_digests(dev, name):
    c = nc.build(name)
    ngcf_upload(dev, c)
    S, Z, D, F = dev.ngcf_propagate(c['layers'], c['training'], c['keep'], c['mask_seed'], c['step'], parts=True)
    out = {'S': sha(S), 'Z': sha(Z), 'D': sha(D), 'F': sha(F)}
    out.update(ngcf_grad(dev, c))
    ngcf_upload(dev, c)
    dev.adam_reset()
    for t in (1, 2):
        out['step%d_loss' % t] = sha_loss(dev.ngcf_step(c['layers'], c['training'], c['keep'], c['mask_seed'], c['u'], c['i'], c['j'], LR, nc.REG, t))
    for key, a in zip(('U', 'V'), dev.get_factors()):
        out['step2_' + key] = sha(a)
    for key, a in zip(('W', 'mW', 'vW'), dev.ngcf_get_weights(moments=True)):
        out['step2_' + key] = sha(a)
    for key, a in zip(('mU', 'vU', 'mV', 'vV'), dev.adam_get_moments()):
        out['step2_' + key] = sha(a)
    return out


def after_ngcf_digests(dev):
    c = nc.build(AFTER[0])
    ngcf_upload(dev, c)
    ngcf_grad(dev, c)
    c = lc.build(AFTER[1])
    lightgcn_upload(dev, c)
    return lightgcn_grad(dev, c)


def main():
    dev = Device(0, raise_errors=True)
    out = {'lightgcn': {name: lightgcn_digests(dev, name) for name in LIGHTGCN}, 'ngcf': {name: ngcf_digests(dev, name) for name in NGCF},
           'lightgcn_after_ngcf': after_ngcf_digests(dev)}
    dev.close()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
