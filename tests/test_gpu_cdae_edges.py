"""GPU: CDAE's kernels at their chunk, part, width and grid-stride edges, on the cases EDGE_CASES of
tests/helpers/cdae_cases.py, which set degrees, batch users and sample sizes instead of drawing them: encoder rows and sample sets of
0, 1, 63, 64, 65, 128 and 129 entries (the 64-entry chunk loops of k_cdae_enc_parts and k_cdae_dec); a batch that samples nothing and
holds no input; h = 1, 63, 65, 127; rows and segments of hub - 1, hub, hub + 1, 2 hub and 2 hub + 1 entries in each of the five part
families at cdae_hub 4, and cdae_hub 1; a keep probability whose threshold is 0; a variable of more than 8192 x 256 elements (the
second trip of k_cdae_dense's grid-stride loop).  tests/test_cdae_golden.py asserts on the CPU that every case reaches its edge and
meets the conditioning statement.  The checks and their bounds are those of tests/test_gpu_cdae.py (4 x the case's d32 with the floor
L 2^-24; a step within 1e-6 lr of the contract's Adam, moments within 1e-6), with exact ones where the contract gives exact values."""
import numpy as np
import pytest

from helpers import cdae_cases as cc
from helpers import numpy_cdae as cd
from test_gpu_cdae import batch, check_factors, check_gradients, check_steps, dev, upload  # noqa: F401 (dev: the module's fixture)

pytestmark = pytest.mark.gpu

REG32 = np.float32(cc.REG)
LR = 0.002


@pytest.mark.parametrize('name', cc.EDGE_NAMES)
def test_forward_mask_loss_and_gradients_at_the_edge(dev, name):
    c = cc.build(name)
    p, users = c['p'], c['users']
    g, out = check_gradients(dev, c)
    hid = out[0]
    if name == 'nothing':                                            # no data term at all: every gradient is the decay, bit for bit
        for k in ('W', 'Wd', 'b', 'bd'):
            assert np.array_equal(g[k], REG32 * p[k]), k
        want = np.zeros_like(p['U'])
        want[0] = REG32 * p['U'][0] + REG32 * p['U'][0]              # reg U[u] once per slot, and user 0 holds both slots
        assert np.array_equal(g['U'], want)
        assert len(out[1]) == len(out[2]) == len(out[3]) == 0
    if name == 'all_dropped':                                        # thr = 0: no input reaches the encoder or gW
        assert not out[1].any() and np.array_equal(g['W'], REG32 * p['W'])
        want = 1 / (1 + np.exp(-(p['b'].astype(np.float64)[None, :] + p['U'].astype(np.float64)[users])))
        assert cd.rel(hid, want) <= cc.bound(c, 'hid')
    if c['kind'] == 'dec':                                           # the slot with the empty sample: dz = 0, so its user's row is reg U[u] alone
        assert c['sptr'][0] == c['sptr'][1] and users.count(users[0]) == 1
        assert np.array_equal(g['U'][users[0]], REG32 * p['U'][users[0]])


def _decay_rows(c):
    """Item rows in no sample and no batch user's list (map < 0), below and from the first row of k_cdae_dense's second trip."""
    fam = cc.families(c)
    rows = np.setdiff1d(np.arange(c['n']), sorted(set(fam['sampled']) | set(fam['inputs'])))
    first = cc.GRID // c['h']
    assert (rows < first).any() and (rows >= first).any()
    return rows


@pytest.mark.parametrize('name', ['stride', 'parts', 'hub1', 'h1', 'h65', 'nothing'])
def test_step_is_the_contracts_adam_at_the_edge(dev, name):
    c = cc.build(name)
    data, users, sptr, sitems, co, seed = c['data'], c['users'], c['sptr'], c['sitems'], c['co'], c['mask_seed']
    rows = _decay_rows(c) if name == 'stride' else None

    def after(t, loss, g, before, got):
        # the loss of the step (the sums of squares of W and W' take their second addends from the loop's second trip) against the
        # fp64 contract at the parameters the device held before it
        p64 = {k: before[k].astype(np.float64) for k in cd.NAMES}
        want = float(cd.loss_and_grad(p64, data, users, sptr, sitems, co, seed, t, cc.REG, dtype=np.float64)[0])
        print(name, 'step', t, 'loss %.3g from fp64 (bound %.3g)' % (abs(loss - want) / abs(want), cc.bound(c, 'loss')))
        assert abs(loss - want) / abs(want) <= cc.bound(c, 'loss')
        if rows is None:
            return
        # a row outside the batch moves by decay alone: its gradient is reg w bit for bit, and Adam on that gradient gives its new value
        for k, pick in (('W', lambda a: a[rows]), ('Wd', lambda a: a[:, rows].T), ('bd', lambda a: a[rows][:, None])):
            w, mo, ve = pick(before[k]).copy(), pick(before['m' + k]).copy(), pick(before['v' + k]).copy()
            assert np.array_equal(pick(g[k]), REG32 * w), k
            cd.adam(w, REG32 * w.copy(), mo, ve, LR, t, np.float32)
            moved = np.abs(pick(got[k]) - w).max(axis=1)
            assert (moved <= 1e-6 * LR).all(), (k, rows[moved > 1e-6 * LR])
            assert (np.abs(pick(got[k]) - pick(before[k])).max(axis=1) > 0).all(), k          # and every one of them did move

    check_steps(dev, c, lr=LR, after=after)


@pytest.mark.parametrize('name', ['h1', 'h63', 'h65', 'h127', 'enc_chunks', 'enc_chunks_hub96'])
def test_load_factors_then_scores_at_the_edge(dev, name):
    c = cc.build(name)
    check_factors(dev, c, c['layout']['score_users'])                # every user, row_user null; ld = h + 1 (64 at h = 63)
    deg = np.diff(c['data'][0])
    hub = c['hub'] if c['hub'] else 1024
    assert dev.get_option('cdae_last_hubs') == int((deg > hub).sum()) and dev.get_option('cdae_last_parts') == int(sum(-(-d // hub) for d in deg if d > hub))


@pytest.mark.parametrize('name', ['enc_chunks', 'parts'])
def test_another_hub_gives_other_sums_within_the_bound_and_the_first_hub_the_first_bits(dev, name):
    c = cc.build(name)
    first = check_gradients(dev, c)[1]
    again = check_gradients(dev, c)[1]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    other = check_gradients(dev, c, hub=7)[1]                        # every bound again, and the host's counts at hub 7
    assert dev.get_option('cdae_last_hubs') > 0
    print(name, 'outputs whose bits differ at hub 7:', sum(not np.array_equal(a, b) for a, b in zip(first, other)), 'of', len(first))
    back = check_gradients(dev, c)[1]
    for a, b in zip(first, back):
        assert np.array_equal(a, b)
