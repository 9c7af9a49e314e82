"""GPU: the bits of LightGCN's and NGCF's device paths on eight small cases (tools/gcn_bits.py), against the SHA-256 digests
recorded in tests/golden/g19_gcn_bits.json.  The digests pin the summation orders of DESIGN.md sections 20 and 21 -- the four
accumulators of a gathered row and their (a0 + a1) + (a2 + a3), the hub parts in ascending order, a minibatch row's entries in
triplet order, the loss in triplet order, the dense layers' chains, the weight gradients' chunks -- as the compiler of this ROCm
turns them into instructions: the other GPU tests bound each model against its fp64 contract, which a reordered sum still meets.
A later change that reorders a sum on purpose, or another compiler that contracts or schedules a chain differently, regenerates
the file with the tool (python tools/gcn_bits.py > tests/golden/g19_gcn_bits.json) and says so."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location('gcn_bits', os.path.join(ROOT, 'tools', 'gcn_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bits = _load_tool()


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


@pytest.fixture(scope='module')
def want(golden_dir):
    with open(os.path.join(golden_dir, 'g19_gcn_bits.json')) as f:
        return json.load(f)


def differing(got, want):
    return sorted(key for key in set(got) | set(want) if got.get(key) != want.get(key))


def test_the_golden_file_holds_the_tools_cases(want):
    assert sorted(want) == ['lightgcn', 'lightgcn_after_ngcf', 'ngcf']
    assert sorted(want['lightgcn']) == sorted(bits.LIGHTGCN) and sorted(want['ngcf']) == sorted(bits.NGCF)


@pytest.mark.parametrize('name', bits.LIGHTGCN)
def test_lightgcn_bits(dev, want, name):
    assert differing(bits.lightgcn_digests(dev, name), want['lightgcn'][name]) == []


@pytest.mark.parametrize('name', bits.NGCF)
def test_ngcf_bits(dev, want, name):
    assert differing(bits.ngcf_digests(dev, name), want['ngcf'][name]) == []


def test_lightgcn_bits_after_ngcf_calls_on_the_same_device(dev, want):
    assert differing(bits.after_ngcf_digests(dev), want['lightgcn_after_ngcf']) == []
