"""GPU: a context's whole life, every family once -- create a Device, run one smallest call of BPR's epoch, Adam, FISM, the
exact replay, WRMF, UserKNN, IPF, ExpoMF, CoFactor, CUNE's network stage, Song2vec, LightGCN, NGCF and CDAE, close it -- in one
process, a warm-up cycle and then a second one, and a fresh context afterwards still trains.  There is no assertion on free
device memory: the runtime takes device memory in blocks far larger than the 8 KiB buffer a context used to forget, and four
such contexts in a row left torch.cuda.mem_get_info() where it was (DESIGN.md 5.00000 has the figures), so that reading
cannot tell a leak of that size from none.  The shapes are the test helpers' smallest, not the workload's."""
import gc

import numpy as np
import pytest

from helpers import cdae_cases, fism_cases, lightgcn_cases, ngcf_cases
from helpers import numpy_cofactor, numpy_cune_net, numpy_expomf, numpy_userknn, numpy_wrmf

pytestmark = pytest.mark.gpu

M, N, K, D = 64, 64, 16, 4                                       # every user has D events: the epoch sums P*P in its rounds


def epoch(dev, data, P0, Q0):
    dev.set_factors(P0, Q0)
    dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
    nll, sp, sq = dev.bpr_epoch(42, 0, 128, 0.02, 0.01, 0.01)
    assert dev.get_option('round_last_user_seq') == 1 and np.isfinite([nll, sp, sq]).all()
    return nll


def cycle():
    """One context from yue_ctx_create to yue_ctx_destroy with every subsystem's state in it."""
    from test_cofactor_golden import load as cof_load
    from test_song2vec_golden import load as s2v_load, start as s2v_start
    from yue_amd import synth
    from yue_amd._shim import Device
    from yue_amd.recommender.cf.IPF import ipf_graph
    data = synth.make_arrays(M, N, D, seed=5)
    ev_u = np.repeat(np.arange(M, dtype=np.int32), D)
    P0, Q0 = synth.init_factors(M, N, K, 6)
    rs = np.random.RandomState(7)
    j = ((data['ev_i'] + 1 + rs.randint(0, N - 1, M * D)) % N).astype(np.int32)
    dev = Device(0, raise_errors=True)
    try:
        epoch(dev, data, P0, Q0)
        dev.adam_step(ev_u[:32], data['ev_i'][:32], j[:32], 0.001, 0.01, 1)
        c = fism_cases.build('S9_k1')
        dev.fism_set_model(c['P0'], c['Q0'], c['B0'])
        dev.fism_rounds(c['user_ptr'], c['ev_i'], c['negs'], c['rho'], c['coef'], 5, c['lr'], fism_cases.REG_I, fism_cases.REG_B)
        dev.set_factors(P0, Q0)
        dev.bpr_replay(ev_u, data['ev_i'], j, 0.02, 0.01, 0.01)
        # WRMF, ExpoMF (on WRMF's pairs), UserKNN, IPF and the user network on the same small log
        um, im = numpy_wrmf.pairs_from_events(ev_u, data['ev_i'], M, N)
        dev.wrmf_set_pairs(*(um + im))
        dev.wrmf_half_sweep(0, numpy_wrmf.ALPHA, 1.0)
        dev.expo_set_pairs(*(um + im))
        dev.expo_set_mu(np.full(N, 0.01, np.float32))
        dev.expo_half_sweep(0, numpy_expomf.LAM_THETA / numpy_expomf.LAM_Y, numpy_expomf.LAM_Y, True)
        (up, ui, uc), (ip, iu) = numpy_userknn.pairs_from_events(data['ev_ptr'], data['ev_i'], N)
        dev.knn_set_pairs(M, N, up, ui, uc, ip, iu)
        dev.knn_neighbors(4)
        dev.ipf_set_graph(ipf_graph(data['ev_ptr'], data['ev_i'], N, 0.5, 0.7, 0.3))
        dev.ipf_topn(np.arange(8, dtype=np.int32), 5)
        (up, ui), (ip, iu) = numpy_cune_net.pairs_from_events(ev_u, data['ev_i'], M, N)
        dev.cnet_set_pairs(M, N, up, ui, ip, iu)
        dev.cnet_walks(2, 5, 3)
        # CoFactor and Song2vec from their smallest goldens
        z, _, _, um, im, _, sp = cof_load('c1_k20')
        X0, Y0, G0, w0, c0 = numpy_cofactor.init_from_seed(int(z['seed']), int(z['m']), int(z['n']), int(z['k']))
        dev.set_factors(X0, Y0)
        dev.wrmf_set_pairs(*(um + im))
        dev.cof_set_sppmi(*sp)
        dev.cof_set_state(G0, w0, c0)
        dev.cof_item_sweep(numpy_wrmf.ALPHA, 1.0, 1.0)
        z, _, _, _, _, steps, pairs, h = s2v_load('c1_k20')
        S = s2v_start(z)
        dev.set_factors(S[0], S[1])
        dev.s2v_set_state(S[2], S[3])
        dev.s2v_set_steps(*steps)
        dev.s2v_set_pairs(*pairs)
        dev.s2v_epoch(h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0.0)
        # the graph models and the autoencoder: one step each
        c = lightgcn_cases.build('layers1')
        g = c['g']
        dev.set_factors(c['U'], c['V'])
        dev.lgcn_set_graph(c['m'], c['n'], g['u_ptr'], g['u_items'], g['u_w'], g['i_ptr'], g['i_users'], g['i_w'])
        dev.lgcn_step(c['layers'], c['u'], c['i'], c['j'], 0.001, lightgcn_cases.REG, 1)
        c = ngcf_cases.build('N31')
        g = c['g']
        dev.set_factors(c['U'], c['V'])
        dev.ngcf_set_graph(c['m'], c['n'], g['ptr'], g['col'], g['w'])
        dev.ngcf_set_weights(c['W'])
        dev.ngcf_step(c['layers'], c['training'], c['keep'], c['mask_seed'], c['u'], c['i'], c['j'], 0.001, ngcf_cases.REG, 1)
        c = cdae_cases.build('B1')
        ptr, items, cnt = c['data']
        p = c['p']
        dev.cdae_set_data(c['m'], c['n'], ptr, items, cnt)
        dev.cdae_set_params(p['U'], p['W'], p['Wd'], p['b'], p['bd'])
        dev.cdae_step(c['users'], c['sptr'], c['sitems'], c['co'], c['mask_seed'], 0.01, cdae_cases.REG, 1)
    finally:
        dev.close()
    del dev
    gc.collect()


def test_contexts_come_and_go():
    cycle()                                                      # warm-up: code objects, the runtime's own pools
    cycle()
    # ... and the process is as good as new: a fresh context trains
    from yue_amd import synth
    from yue_amd._shim import Device
    dev = Device(0, raise_errors=True)
    try:
        epoch(dev, synth.make_arrays(M, N, D, seed=5), *synth.init_factors(M, N, K, 6))
    finally:
        dev.close()
