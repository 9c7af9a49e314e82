"""ctypes binding of libyue_hip.so (include/yue_hip.h).

This is the only route from the Python plugin surface to the numeric hot path: there is no
CPU fallback.  If the library is missing or no MI355X is visible, calls fail loudly in the
reference's style -- print the message, exit(-1) (tool/config.py:9-11,
base/IterativeRecommender.py:64-66) -- or raise YueHipError when ``raise_errors`` is set
(tests use that).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libyue_hip.so')

OK, ERR_ARG, ERR_HIP, ERR_FEW_ITEMS, ERR_COMM, ERR_SATURATED = 0, -1, -2, -3, -4, -5
UNIQUE_ID_BYTES = 128

# every symbol include/yue_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = ['yue_last_error', 'yue_version', 'yue_ctx_create', 'yue_ctx_destroy', 'yue_sync',
           'yue_set_factors', 'yue_get_factors', 'yue_set_interactions', 'yue_bpr_replay',
           'yue_bpr_rounds', 'yue_bpr_epoch', 'yue_cune_steps', 'yue_adam_reset', 'yue_adam_get_moments', 'yue_adam_step', 'yue_sample_negatives', 'yue_sumsq', 'yue_scores',
           'yue_topn_scan', 'yue_set_kernel_timing', 'yue_get_kernel_timing', 'yue_get_scan_stats', 'yue_get_scan_work', 'yue_set_option', 'yue_get_option',
           'yue_comm_unique_id', 'yue_comm_init', 'yue_allreduce_f64', 'yue_get_comm_stats',
           'yue_default_round_events', 'yue_epoch_plan',
           'yue_fism_set_model', 'yue_fism_get_model', 'yue_fism_epoch', 'yue_fism_rounds', 'yue_fism_scores', 'yue_fism_topn_scan',
           'yue_wrmf_set_pairs', 'yue_wrmf_half_sweep',
           'yue_expo_set_pairs', 'yue_expo_set_mu', 'yue_expo_get_mu', 'yue_expo_half_sweep', 'yue_expo_update_mu', 'yue_expo_gram_rows',
           'yue_cof_cooccur', 'yue_cof_get_cooccur', 'yue_cof_set_sppmi', 'yue_cof_set_state', 'yue_cof_get_state', 'yue_cof_item_sweep',
           'yue_knn_set_pairs', 'yue_knn_neighbors', 'yue_knn_predict', 'yue_knn_topn',
           'yue_ipf_set_graph', 'yue_ipf_predict', 'yue_ipf_topn',
           'yue_cnet_set_pairs', 'yue_cnet_walks', 'yue_cnet_set_walks', 'yue_cnet_set_sentences', 'yue_cnet_embed', 'yue_cnet_set_embedding',
           'yue_cnet_friends',
           'yue_s2v_set_state', 'yue_s2v_get_state', 'yue_s2v_set_steps', 'yue_s2v_set_pairs', 'yue_s2v_epoch',
           'yue_lgcn_set_graph', 'yue_lgcn_propagate', 'yue_lgcn_grad', 'yue_lgcn_step',
           'yue_ngcf_set_graph', 'yue_ngcf_set_weights', 'yue_ngcf_get_weights', 'yue_ngcf_propagate', 'yue_ngcf_grad', 'yue_ngcf_step',
           'yue_cdae_set_data', 'yue_cdae_set_params', 'yue_cdae_get_params', 'yue_cdae_forward', 'yue_cdae_grad', 'yue_cdae_step',
           'yue_cdae_load_factors', 'yue_cdae_times']


class YueHipError(RuntimeError):
    def __init__(self, code, msg):
        super(YueHipError, self).__init__('libyue_hip error %d: %s' % (code, msg))
        self.code = code


_lib = None


def load_library():
    """dlopen libyue_hip.so; never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YueHipError(ERR_HIP, 'HIP library not built: %s (run `make -C yue_amd/csrc` or __graft_entry__.build())' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.yue_last_error.restype = C.c_char_p
        for name in SYMBOLS[1:]:
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(C.POINTER(C.c_int64))


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def comm_unique_id():
    lib = load_library()
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    rc = lib.yue_comm_unique_id(buf)
    if rc != OK:
        raise YueHipError(rc, lib.yue_last_error().decode())
    return bytes(buf)


def epoch_plan(m, k, round_events, events_total, nranks):
    """(user_block, blocks_per_group, n_blocks) of yue_bpr_epoch's schedule -- pure host arithmetic inside the library."""
    lib = load_library()
    ub, grp, nb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.yue_epoch_plan(C.c_int64(m), C.c_int(k), C.c_int64(round_events), C.c_double(events_total), C.c_int(nranks),
                            C.byref(ub), C.byref(grp), C.byref(nb))
    if rc != OK:
        raise YueHipError(rc, lib.yue_last_error().decode())
    return ub.value, grp.value, nb.value


class Device(object):
    """One HIP context = one GPU (one process per GPU)."""

    def __init__(self, device=0, raise_errors=False):
        self._lib = load_library()
        self._raise = raise_errors
        self._ctx = C.c_void_p()
        self.m = self.n = self.k = self.E = 0
        self.fn = self.fk = 0
        self.knn_m = self.knn_n = 0
        self.ipf_m = self.ipf_n = 0
        self.cnet_m = self.cnet_dim = 0
        self._chk(self._lib.yue_ctx_create(C.c_int(device), C.byref(self._ctx)))

    # reference convention: print, exit(-1)
    def _chk(self, rc):
        if rc == OK:
            return
        msg = self._lib.yue_last_error().decode()
        if self._raise:
            raise YueHipError(rc, msg)
        print(msg)
        exit(-1)

    def close(self):
        if self._ctx:
            self._lib.yue_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self._lib.yue_sync(self._ctx))

    # -- state ------------------------------------------------------------------------
    def set_factors(self, P, Q):
        P, pp = _f32(P)
        Q, qp = _f32(Q)
        assert P.ndim == 2 and Q.ndim == 2 and P.shape[1] == Q.shape[1]
        self.m, self.k = P.shape
        self.n = Q.shape[0]
        self._chk(self._lib.yue_set_factors(self._ctx, pp, C.c_int64(self.m), qp, C.c_int64(self.n), C.c_int(self.k)))

    def get_factors(self, P=None, Q=None):
        """Copies the device factors into P, Q (allocated when None) and returns them."""
        if P is None:
            P = np.empty((self.m, self.k), np.float32)
        if Q is None:
            Q = np.empty((self.n, self.k), np.float32)
        assert P.dtype == np.float32 and Q.dtype == np.float32 and P.flags.c_contiguous and Q.flags.c_contiguous
        self._chk(self._lib.yue_get_factors(self._ctx, P.ctypes.data_as(C.POINTER(C.c_float)), Q.ctypes.data_as(C.POINTER(C.c_float))))
        return P, Q

    def set_interactions(self, indptr, indices, ev_ptr, ev_i):
        indptr, a = _i64(indptr)
        indices, b = _i32(indices if len(indices) else np.zeros(1, np.int32))
        ev_ptr, c = _i64(ev_ptr)
        ev_i, d = _i32(ev_i if len(ev_i) else np.zeros(1, np.int32))
        assert len(indptr) == self.m + 1 and len(ev_ptr) == self.m + 1
        self.E = int(ev_ptr[-1])
        self._chk(self._lib.yue_set_interactions(self._ctx, a, b, c, d))

    # -- training -----------------------------------------------------------------------
    def bpr_replay(self, u, i, j, lr, regU, regI):
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        nll = C.c_double()
        self._chk(self._lib.yue_bpr_replay(self._ctx, a, b, c, C.c_int64(len(u)), C.c_double(lr), C.c_double(regU), C.c_double(regI), C.byref(nll)))
        return nll.value

    def bpr_rounds(self, u, i, j, round_ptr, lr, regU, regI):
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        rp, d = _i64(round_ptr)
        nll = C.c_double()
        self._chk(self._lib.yue_bpr_rounds(self._ctx, a, b, c, d, C.c_int64(len(rp) - 1), C.c_double(lr), C.c_double(regU), C.c_double(regI), C.byref(nll)))
        return nll.value

    def cune_steps(self, u, i, k, j, s, lr, regU, regI):
        """CUNE's two-level BPR steps in order (k < 0: plain step).  Returns the per-step losses (float64[T])."""
        u, a = _i32(u)
        i, b = _i32(i)
        k, c = _i32(k)
        j, d = _i32(j)
        loss = np.empty(len(u), np.float64)
        self._chk(self._lib.yue_cune_steps(self._ctx, a, b, c, d, C.c_int64(len(u)), C.c_double(s), C.c_double(lr), C.c_double(regU), C.c_double(regI),
                                           loss.ctypes.data_as(C.POINTER(C.c_double))))
        return loss

    def adam_reset(self):
        self._chk(self._lib.yue_adam_reset(self._ctx))

    def adam_step(self, u, i, j, lr, reg, step):
        """One minibatch step of the reference's live TF-style path (softplus loss + l2 terms, Adam).  Returns total_loss."""
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        loss = C.c_double()
        self._chk(self._lib.yue_adam_step(self._ctx, a, b, c, C.c_int64(len(u)), C.c_double(lr), C.c_double(reg), C.c_int64(step), C.byref(loss)))
        return loss.value

    def adam_get_moments(self):
        """(mU, vU, mV, vV) of the uploaded factors' Adam state."""
        out = [np.empty((r, self.k), np.float32) for r in (self.m, self.m, self.n, self.n)]
        self._chk(self._lib.yue_adam_get_moments(self._ctx, *[x.ctypes.data_as(C.POINTER(C.c_float)) for x in out]))
        return tuple(out)

    # -- LightGCN (U = P, V = Q of set_factors) -------------------------
    def lgcn_set_graph(self, m, n, u_ptr, u_items, u_w, i_ptr, i_users, i_w):
        """Both sides of the (user, item, weight) pair list, ids sorted and unique within a row; checked for symmetry."""
        u_ptr, a = _i64(u_ptr)
        i_ptr, d = _i64(i_ptr)
        assert len(u_ptr) == m + 1 and len(i_ptr) == n + 1, 'lgcn_set_graph: u_ptr [m + 1], i_ptr [n + 1]'
        assert len(u_items) == len(u_w) and len(i_users) == len(i_w), 'lgcn_set_graph: one weight per id'
        assert len(u_items) >= u_ptr[-1] and len(i_users) >= i_ptr[-1], 'lgcn_set_graph: ptr runs past the id lists'
        u_items, b = _i32(u_items if len(u_items) else np.zeros(1, np.int32))
        u_w, c = _f32(u_w if len(u_w) else np.zeros(1, np.float32))
        i_users, e = _i32(i_users if len(i_users) else np.zeros(1, np.int32))
        i_w, f = _f32(i_w if len(i_w) else np.zeros(1, np.float32))
        self._chk(self._lib.yue_lgcn_set_graph(self._ctx, C.c_int64(m), C.c_int64(n), a, b, c, d, e, f))

    def lgcn_propagate(self, layers, raw=False):
        """F [m + n][k]; with raw also the unnormalised layers E_1 .. E_layers [layers][m + n][k]."""
        N = self.m + self.n
        F = np.empty((N, self.k), np.float32)
        E = np.empty((max(layers, 0), N, self.k), np.float32) if raw else None
        self._chk(self._lib.yue_lgcn_propagate(self._ctx, C.c_int(layers), E.ctypes.data_as(C.POINTER(C.c_float)) if raw else None,
                                               F.ctypes.data_as(C.POINTER(C.c_float))))
        return (E, F) if raw else F

    def lgcn_grad(self, layers, u, i, j, reg):
        """(loss, dLoss / dU, dLoss / dV) of one minibatch of triplets; nothing moves."""
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        assert len(u) == len(i) == len(j), 'lgcn_grad: one u, i, j per triplet'
        loss = C.c_double()
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        self._chk(self._lib.yue_lgcn_grad(self._ctx, C.c_int(layers), a, b, c, C.c_int64(len(u)), C.c_double(reg), C.byref(loss),
                                          gU.ctypes.data_as(C.POINTER(C.c_float)), gV.ctypes.data_as(C.POINTER(C.c_float))))
        return loss.value, gU, gV

    def lgcn_step(self, layers, u, i, j, lr, reg, step):
        """One minibatch step: propagation, loss, backward pass, Adam on U and V.  Returns the loss."""
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        assert len(u) == len(i) == len(j), 'lgcn_step: one u, i, j per triplet'
        loss = C.c_double()
        self._chk(self._lib.yue_lgcn_step(self._ctx, C.c_int(layers), a, b, c, C.c_int64(len(u)), C.c_double(lr), C.c_double(reg), C.c_int64(step),
                                          C.byref(loss)))
        return loss.value

    # -- NGCF (U = P, V = Q of set_factors) ------------------------------
    def ngcf_set_graph(self, m, n, ptr, col, w):
        """The (m + n)-row graph as a general CSR: columns ascending and unique within a row."""
        ptr, a = _i64(ptr)
        assert len(ptr) == m + n + 1 and len(col) == len(w) and len(col) >= ptr[-1], 'ngcf_set_graph: ptr [m + n + 1], one weight per column'
        col, b = _i32(col if len(col) else np.zeros(1, np.int32))
        w, c = _f32(w if len(w) else np.zeros(1, np.float32))
        self._chk(self._lib.yue_ngcf_set_graph(self._ctx, C.c_int64(m), C.c_int64(n), a, b, c))

    def ngcf_set_weights(self, W):
        """W [layers][2][k][k]; the weights' Adam moments are cleared."""
        W, a = _f32(W)
        assert W.ndim == 4 and W.shape[1] == 2 and W.shape[2] == W.shape[3], 'ngcf_set_weights: W [layers][2][k][k]'
        self.ngcf_w_shape = W.shape
        self._chk(self._lib.yue_ngcf_set_weights(self._ctx, C.c_int(W.shape[0]), C.c_int(W.shape[2]), a))

    def ngcf_get_weights(self, moments=False):
        """W, or (W, mW, vW) with the weights' Adam moments."""
        out = [np.empty(self.ngcf_w_shape, np.float32) for _ in range(3 if moments else 1)]
        ptrs = [x.ctypes.data_as(C.POINTER(C.c_float)) for x in out] + [None] * (3 - len(out))
        self._chk(self._lib.yue_ngcf_get_weights(self._ctx, *ptrs))
        return tuple(out) if moments else out[0]

    def ngcf_propagate(self, layers, training=False, keep=1.0, seed=0, step=0, parts=False):
        """F [m + n][(layers + 1) k]; with parts (S, Z, D, F), the first three [layers][m + n][k]."""
        N = self.m + self.n
        F = np.empty((N, (max(layers, 0) + 1) * self.k), np.float32)
        P = [np.empty((max(layers, 0), N, self.k), np.float32) for _ in range(3)] if parts else []
        ptrs = [x.ctypes.data_as(C.POINTER(C.c_float)) for x in P] if parts else [None] * 3
        self._chk(self._lib.yue_ngcf_propagate(self._ctx, C.c_int(layers), C.c_int(int(bool(training))), C.c_double(keep), C.c_uint64(seed),
                                               C.c_int64(step), ptrs[0], ptrs[1], ptrs[2], F.ctypes.data_as(C.POINTER(C.c_float))))
        return tuple(P) + (F,) if parts else F

    def ngcf_grad(self, layers, training, keep, seed, step, u, i, j, reg):
        """(loss, dLoss / dU, dLoss / dV, dLoss / dW) of one minibatch of triplets; nothing moves."""
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        assert len(u) == len(i) == len(j), 'ngcf_grad: one u, i, j per triplet'
        loss = C.c_double()
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        gW = np.empty((max(layers, 0), 2, self.k, self.k), np.float32)
        self._chk(self._lib.yue_ngcf_grad(self._ctx, C.c_int(layers), C.c_int(int(bool(training))), C.c_double(keep), C.c_uint64(seed), C.c_int64(step),
                                          a, b, c, C.c_int64(len(u)), C.c_double(reg), C.byref(loss), gU.ctypes.data_as(C.POINTER(C.c_float)),
                                          gV.ctypes.data_as(C.POINTER(C.c_float)), gW.ctypes.data_as(C.POINTER(C.c_float))))
        return loss.value, gU, gV, gW

    def ngcf_step(self, layers, training, keep, seed, u, i, j, lr, reg, step):
        """One minibatch step: propagation, loss, backward pass, Adam on U, V and the weights.  Returns the loss."""
        u, a = _i32(u)
        i, b = _i32(i)
        j, c = _i32(j)
        assert len(u) == len(i) == len(j), 'ngcf_step: one u, i, j per triplet'
        loss = C.c_double()
        self._chk(self._lib.yue_ngcf_step(self._ctx, C.c_int(layers), C.c_int(int(bool(training))), C.c_double(keep), C.c_uint64(seed), a, b, c,
                                          C.c_int64(len(u)), C.c_double(lr), C.c_double(reg), C.c_int64(step), C.byref(loss)))
        return loss.value

    # -- CDAE (a state of its own: U, W, W', b, b') ----------------------
    def cdae_set_data(self, m, n, ptr, items, counts):
        """The user CSR: items ascending and distinct within a user, with their event counts."""
        ptr, a = _i64(ptr)
        assert len(ptr) == m + 1 and len(items) == len(counts) and len(items) >= ptr[-1], 'cdae_set_data: ptr [m + 1], one count per item'
        self.cdae_nnz_ptr = ptr
        items, b = _i32(items if len(items) else np.zeros(1, np.int32))
        counts, c = _i32(counts if len(counts) else np.zeros(1, np.int32))
        self._chk(self._lib.yue_cdae_set_data(self._ctx, C.c_int64(m), C.c_int64(n), a, b, c))
        self.cdae_m, self.cdae_n = int(m), int(n)

    def cdae_set_params(self, U, W, Wd, b, bd):
        """U [m, h], encoder W [n, h], decoder Wd [h, n], b [h], bd [n]; the Adam moments are cleared."""
        arrs = [_f32(x) for x in (U, W, Wd, b, bd)]
        h = arrs[0][0].shape[1]
        assert [x[0].shape for x in arrs] == [(self.cdae_m, h), (self.cdae_n, h), (h, self.cdae_n), (h,), (self.cdae_n,)], \
            'cdae_set_params: U [m, h], W [n, h], Wd [h, n], b [h], bd [n] for the m, n of cdae_set_data'
        self._chk(self._lib.yue_cdae_set_params(self._ctx, C.c_int(h), *[x[1] for x in arrs]))
        self.cdae_h = int(h)

    def _cdae_shapes(self):
        m, n, h = self.cdae_m, self.cdae_n, self.cdae_h
        return ((m, h), (n, h), (h, n), (h,), (n,))

    def cdae_get_params(self, moments=False):
        """{'U', 'W', 'Wd', 'b', 'bd'}; with moments also 'mU' .. 'vbd'."""
        out, sets = {}, []
        for prefix in ('', 'm', 'v') if moments else ('',):
            arrs = [np.empty(shape, np.float32) for shape in self._cdae_shapes()]
            out.update({prefix + key: a for key, a in zip(('U', 'W', 'Wd', 'b', 'bd'), arrs)})
            sets.append((C.POINTER(C.c_float) * 5)(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs]))
        sets += [None] * (3 - len(sets))
        self._chk(self._lib.yue_cdae_get_params(self._ctx, *sets))
        return out

    def _cdae_batch(self, users, sptr, sitems):
        users, a = _i32(users)
        sptr, b = _i64(sptr)
        assert len(sptr) == len(users) + 1 and len(sitems) >= sptr[-1], 'cdae: sample_ptr [B + 1] over sample_items'
        sitems, c = _i32(sitems if len(sitems) else np.zeros(1, np.int32))
        return (users, sptr, sitems), (a, C.c_int64(len(users)), b, c)

    def cdae_forward(self, users, sptr, sitems, co, seed, step, reg):
        """(hid [B, h], kept flags per input entry, logits and y_pred per sampled entry, loss)."""
        keep, args = self._cdae_batch(users, sptr, sitems)
        B, S = len(keep[0]), int(keep[1][-1])
        ptr = self.cdae_nnz_ptr
        q_in = int(sum(ptr[u + 1] - ptr[u] for u in keep[0] if 0 <= u < self.cdae_m))
        hid = np.empty((B, self.cdae_h), np.float32)
        kept = np.empty(max(q_in, 1), np.int32)
        logit, ypred = np.empty(max(S, 1), np.float32), np.empty(max(S, 1), np.float32)
        loss = C.c_double()
        self._chk(self._lib.yue_cdae_forward(self._ctx, *args, C.c_double(co), C.c_uint64(seed), C.c_int64(step), C.c_double(reg),
                                             hid.ctypes.data_as(C.POINTER(C.c_float)), kept.ctypes.data_as(C.POINTER(C.c_int32)),
                                             logit.ctypes.data_as(C.POINTER(C.c_float)), ypred.ctypes.data_as(C.POINTER(C.c_float)), C.byref(loss)))
        return hid, kept[:q_in].astype(bool), logit[:S], ypred[:S], loss.value

    def cdae_grad(self, users, sptr, sitems, co, seed, step, reg):
        """(loss, {'U', 'W', 'Wd', 'b', 'bd'}: the dense gradients); nothing moves."""
        keep, args = self._cdae_batch(users, sptr, sitems)
        g = [np.empty(shape, np.float32) for shape in self._cdae_shapes()]
        loss = C.c_double()
        self._chk(self._lib.yue_cdae_grad(self._ctx, *args, C.c_double(co), C.c_uint64(seed), C.c_int64(step), C.c_double(reg), C.byref(loss),
                                          *[x.ctypes.data_as(C.POINTER(C.c_float)) for x in g]))
        return loss.value, dict(zip(('U', 'W', 'Wd', 'b', 'bd'), g))

    def cdae_step(self, users, sptr, sitems, co, seed, lr, reg, step):
        """One minibatch step.  Returns (loss, saturated): with saturated > 0 the loss is inf and nothing was updated."""
        keep, args = self._cdae_batch(users, sptr, sitems)
        loss = C.c_double()
        rc = self._lib.yue_cdae_step(self._ctx, *args, C.c_double(co), C.c_uint64(seed), C.c_double(lr), C.c_double(reg), C.c_int64(step), C.byref(loss))
        if rc == ERR_SATURATED:
            return loss.value, self.get_option('cdae_last_saturated')
        self._chk(rc)
        return loss.value, 0

    def cdae_load_factors(self):
        """Fills the context's factor matrices on the device with [hid(u) | 1] and [Wd[:, i] | bd[i]] (k = h + 1) for the scan."""
        self._chk(self._lib.yue_cdae_load_factors(self._ctx))
        self.m, self.n, self.k = self.cdae_m, self.cdae_n, self.cdae_h + 1

    def cdae_times(self):
        """Device ns of the last call's (encode, decode, regroup, adam) phases."""
        ns = (C.c_int64 * 4)()
        self._chk(self._lib.yue_cdae_times(self._ctx, ns))
        return tuple(ns)

    def default_round_events(self):
        out = C.c_int64()
        self._chk(self._lib.yue_default_round_events(self._ctx, C.byref(out)))
        return out.value

    def bpr_epoch(self, seed, epoch, round_events, lr, regU, regI):
        """Returns (nll, sumsqP, sumsqQ) after one epoch (device sampler + S-rounds; round_events 0 = the device default)."""
        nll, sp, sq = C.c_double(), C.c_double(), C.c_double()
        self._chk(self._lib.yue_bpr_epoch(self._ctx, C.c_uint64(seed), C.c_uint32(epoch), C.c_int64(round_events), C.c_double(lr), C.c_double(regU),
                                          C.c_double(regI), C.byref(nll), C.byref(sp), C.byref(sq)))
        return nll.value, sp.value, sq.value

    def sample_negatives(self, seed, epoch):
        j = np.empty(max(self.E, 1), np.int32)
        self._chk(self._lib.yue_sample_negatives(self._ctx, C.c_uint64(seed), C.c_uint32(epoch), j.ctypes.data_as(C.POINTER(C.c_int32))))
        return j[:self.E]

    def sumsq(self):
        sp, sq = C.c_double(), C.c_double()
        self._chk(self._lib.yue_sumsq(self._ctx, C.byref(sp), C.byref(sq)))
        return sp.value, sq.value

    # -- scoring ------------------------------------------------------------------------
    def scores(self, user):
        out = np.empty(self.n, np.float32)
        self._chk(self._lib.yue_scores(self._ctx, C.c_int32(user), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def topn_scan(self, users, N, mask_indptr=None, mask_indices=None):
        """(ids[nu,N] int32, scores[nu,N] float32).  Raises IndexError like the reference
        (base/IterativeRecommender.py:126) when a user has fewer than N candidates."""
        users, up = _i32(users)
        ids = np.empty((len(users), N), np.int32)
        sc = np.empty((len(users), N), np.float32)
        if mask_indptr is None:
            mp = mi = None
        else:
            mask_indptr, mp = _i64(mask_indptr)
            mask_indices, mi = _i32(mask_indices if len(mask_indices) else np.zeros(1, np.int32))
        rc = self._lib.yue_topn_scan(self._ctx, up, C.c_int64(len(users)), C.c_int(N), mp, mi,
                                     ids.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_float)))
        if rc == ERR_FEW_ITEMS:
            raise IndexError('list index out of range')
        self._chk(rc)
        return ids, sc

    def scan_stats(self):
        """(kernel ms, state-machine events, exact re-scores, used_bf16) of the last topn_scan."""
        ms, ev, rs, bf = C.c_double(), C.c_int64(), C.c_int64(), C.c_int()
        self._chk(self._lib.yue_get_scan_stats(self._ctx, C.byref(ms), C.byref(ev), C.byref(rs), C.byref(bf)))
        return ms.value, ev.value, rs.value, bool(bf.value)

    def scan_work(self):
        """(tiles scored, tiles of the full product) of the last topn_scan (32 users x 32 items each)."""
        done, total = C.c_int64(), C.c_int64()
        self._chk(self._lib.yue_get_scan_work(self._ctx, C.byref(done), C.byref(total)))
        return done.value, total.value

    def set_option(self, name, value):
        self._chk(self._lib.yue_set_option(self._ctx, name.encode(), C.c_int64(value)))

    def get_option(self, name):
        out = C.c_int64()
        self._chk(self._lib.yue_get_option(self._ctx, name.encode(), C.byref(out)))
        return out.value

    # -- measurement ----------------------------------------------------------------------
    def set_kernel_timing(self, stride):
        self._chk(self._lib.yue_set_kernel_timing(self._ctx, C.c_int(stride)))

    def get_kernel_timing(self):
        ms, nl, nt = C.c_double(), C.c_int64(), C.c_int64()
        self._chk(self._lib.yue_get_kernel_timing(self._ctx, C.byref(ms), C.byref(nl), C.byref(nt)))
        return ms.value, nl.value, nt.value

    # -- multi-GPU ----------------------------------------------------------------------
    # -- FISM (parity path) ---------------------------------------------------------------
    def fism_set_model(self, P, Q, Bi):
        P, a = _f64(P)
        Q, b = _f32(Q)
        Bi, c = _f64(Bi)
        assert P.shape == Q.shape and len(Bi) == P.shape[0]
        self._chk(self._lib.yue_fism_set_model(self._ctx, a, b, c, C.c_int64(P.shape[0]), C.c_int(P.shape[1])))
        self.fn, self.fk = P.shape                       # (after the check: a refused upload leaves the earlier model and its shape)

    def fism_get_model(self, P, Q, Bi):
        """Copies the device model into the given arrays (float64 [n,k], float32 [n,k], float64 [n])."""
        assert P.dtype == np.float64 and Q.dtype == np.float32 and Bi.dtype == np.float64
        assert P.flags.c_contiguous and Q.flags.c_contiguous and Bi.flags.c_contiguous
        self._chk(self._lib.yue_fism_get_model(self._ctx, P.ctypes.data_as(C.POINTER(C.c_double)), Q.ctypes.data_as(C.POINTER(C.c_float)),
                                               Bi.ctypes.data_as(C.POINTER(C.c_double))))

    def fism_epoch(self, user_ptr, ev_i, negs, rho, coef, lr, regI, regB):
        """One sequential pass (FISM.py:38-69).  Returns (sum of 0.5*error^2, sum(P*P), sum(Q*Q), Bi.Bi)."""
        user_ptr, a = _i64(user_ptr)
        ev_i, b = _i32(ev_i if len(ev_i) else np.zeros(1, np.int32))
        n_negs = len(negs)
        negs, c = _i32(negs if n_negs else np.zeros(1, np.int32))
        coef, d = _f64(coef)
        half = C.c_double()
        sums = (C.c_double * 3)()
        self._chk(self._lib.yue_fism_epoch(self._ctx, a, C.c_int64(len(user_ptr) - 1), b, c, C.c_int64(n_negs), C.c_int(rho), d,
                                           C.c_double(lr), C.c_double(regI), C.c_double(regB), C.byref(half), sums))
        return half.value, sums[0], sums[1], sums[2]

    def fism_rounds(self, user_ptr, ev_i, negs, rho, coef, round_users, lr, regI, regB):
        """The same pass in rounds of `round_users` users (throughput form).  Returns (sum of 0.5*error^2, sum(P*P), sum(Q*Q), Bi.Bi)."""
        user_ptr, a = _i64(user_ptr)
        ev_i, b = _i32(ev_i if len(ev_i) else np.zeros(1, np.int32))
        n_negs = len(negs)
        negs, c = _i32(negs if n_negs else np.zeros(1, np.int32))
        coef, d = _f64(coef)
        half = C.c_double()
        sums = (C.c_double * 3)()
        self._chk(self._lib.yue_fism_rounds(self._ctx, a, C.c_int64(len(user_ptr) - 1), b, c, C.c_int64(n_negs), C.c_int(rho), d, C.c_int64(round_users),
                                            C.c_double(lr), C.c_double(regI), C.c_double(regB), C.byref(half), sums))
        return half.value, sums[0], sums[1], sums[2]

    def fism_scores(self, items):
        n_items = len(items)                             # (an empty row is passed as a placeholder of one element and a length of 0)
        items, a = _i32(items if n_items else np.zeros(1, np.int32))
        out = np.empty(self.fn, np.float64)
        self._chk(self._lib.yue_fism_scores(self._ctx, a, C.c_int64(n_items), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def fism_topn_scan(self, row_ptr, row_items, N):
        """(ids[nu,N] int32, scores[nu,N] float64) for users given by the CSR of their training events."""
        row_ptr, a = _i64(row_ptr)
        nu = len(row_ptr) - 1
        row_items, b = _i32(row_items if len(row_items) else np.zeros(1, np.int32))
        ids = np.empty((nu, N), np.int32)
        sc = np.empty((nu, N), np.float64)
        rc = self._lib.yue_fism_topn_scan(self._ctx, a, b, C.c_int64(nu), C.c_int(N), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                          sc.ctypes.data_as(C.POINTER(C.c_double)))
        if rc == ERR_FEW_ITEMS:
            raise IndexError(self._lib.yue_last_error().decode())
        self._chk(rc)
        return ids, sc

    # -- WRMF (ALS half-sweeps on the factors of set_factors) ----------------------------------
    def wrmf_set_pairs(self, u_ptr, u_items, u_counts, i_ptr, i_users, i_counts):
        """Distinct pairs both ways with their counts: user-major (items ascending) and item-major (users ascending)."""
        u_ptr, a = _i64(u_ptr)
        i_ptr, d = _i64(i_ptr)
        assert len(u_ptr) == self.m + 1 and len(i_ptr) == self.n + 1, 'wrmf_set_pairs: pointer sizes must match set_factors (m + 1, n + 1)'
        nnz = int(u_ptr[-1])
        assert int(i_ptr[-1]) == nnz and len(u_items) == nnz and len(u_counts) == nnz and len(i_users) == nnz and len(i_counts) == nnz, \
            'wrmf_set_pairs: both directions must hold nnz pairs'
        u_items, b = _i32(u_items if nnz else np.zeros(1, np.int32))
        u_counts, c = _i32(u_counts if nnz else np.zeros(1, np.int32))
        i_users, e = _i32(i_users if nnz else np.zeros(1, np.int32))
        i_counts, f = _i32(i_counts if nnz else np.zeros(1, np.int32))
        self._chk(self._lib.yue_wrmf_set_pairs(self._ctx, a, b, c, d, e, f, C.c_int64(nnz)))

    def wrmf_half_sweep(self, side, alpha, reg):
        """side 0: every user row from the item factors (returns the loss over the pairs, from the rows before the sweep);
        side 1: every item row from the user factors (returns 0.0)."""
        assert side in (0, 1)
        loss = C.c_double()
        self._chk(self._lib.yue_wrmf_half_sweep(self._ctx, C.c_int(side), C.c_double(alpha), C.c_double(reg), C.byref(loss)))
        return loss.value

    # -- ExpoMF (factors: theta = P, beta = Q) ---------------------------------------------------
    def expo_set_pairs(self, u_ptr, u_items, u_counts, i_ptr, i_users, i_counts):
        """The pairs of wrmf_set_pairs (the two ALS solvers share the upload, the schedule and the long rows' chunks)."""
        u_ptr, a = _i64(u_ptr)
        i_ptr, d = _i64(i_ptr)
        assert len(u_ptr) == self.m + 1 and len(i_ptr) == self.n + 1, 'expo_set_pairs: pointer sizes must match set_factors (m + 1, n + 1)'
        nnz = int(u_ptr[-1])
        assert int(i_ptr[-1]) == nnz and len(u_items) == nnz and len(u_counts) == nnz and len(i_users) == nnz and len(i_counts) == nnz, \
            'expo_set_pairs: both directions must hold nnz pairs'
        u_items, b = _i32(u_items if nnz else np.zeros(1, np.int32))
        u_counts, c = _i32(u_counts if nnz else np.zeros(1, np.int32))
        i_users, e = _i32(i_users if nnz else np.zeros(1, np.int32))
        i_counts, f = _i32(i_counts if nnz else np.zeros(1, np.int32))
        self._chk(self._lib.yue_expo_set_pairs(self._ctx, a, b, c, d, e, f, C.c_int64(nnz)))

    def expo_set_mu(self, mu):
        mu, p = _f32(mu)
        self._chk(self._lib.yue_expo_set_mu(self._ctx, p, C.c_int64(len(mu))))

    def expo_get_mu(self):
        mu = np.empty(self.n, np.float32)
        self._chk(self._lib.yue_expo_get_mu(self._ctx, mu.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(self.n)))
        return mu

    def expo_half_sweep(self, side, lam, lam_y, mu_per_column):
        """side 0: every user row from the item factors; side 1: every item row from the user factors."""
        self._chk(self._lib.yue_expo_half_sweep(self._ctx, C.c_int(side), C.c_double(lam), C.c_double(lam_y), C.c_int(1 if mu_per_column else 0)))

    def expo_update_mu(self, a, b, lam_y):
        self._chk(self._lib.yue_expo_update_mu(self._ctx, C.c_double(a), C.c_double(b), C.c_double(lam_y)))

    def expo_gram_rows(self, side, mu_per_column, lam_y, rows):
        """Diagnostic: the dense stage of a half-sweep alone.  fp64 [len(rows), k(k+1)/2]: per listed row the packed lower
        triangle of sum over all columns of A~ f f^T (no A = 1 on the pairs, no lam*I), from the half-sweep's own Gram kernel."""
        rows, p = _i32(rows)
        out = np.empty((len(rows), self.k * (self.k + 1) // 2), np.float64)
        self._chk(self._lib.yue_expo_gram_rows(self._ctx, C.c_int(side), C.c_int(1 if mu_per_column else 0), C.c_double(lam_y), p,
                                               C.c_int64(len(rows)), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # -- CoFactor (factors: X = P, Y = Q; pairs: wrmf_set_pairs; user sweep: wrmf_half_sweep(0, ...)) ----------------
    def cof_cooccur(self, filt):
        """Builds the co-occurrence CSR on the device; returns (ptr int64 [n+1], idx int32 ascending, cnt int32)."""
        nnz = C.c_int64()
        self._chk(self._lib.yue_cof_cooccur(self._ctx, C.c_int(int(filt)), C.byref(nnz)))
        ptr = np.empty(self.n + 1, np.int64)
        idx = np.empty(max(nnz.value, 1), np.int32)
        cnt = np.empty(max(nnz.value, 1), np.int32)
        self._chk(self._lib.yue_cof_get_cooccur(self._ctx, ptr.ctypes.data_as(C.POINTER(C.c_int64)), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                cnt.ctypes.data_as(C.POINTER(C.c_int32))))
        return ptr, idx[:nnz.value], cnt[:nnz.value]

    def cof_set_sppmi(self, ptr, idx, val):
        ptr, a = _i64(ptr)
        assert len(ptr) == self.n + 1, 'cof_set_sppmi: the pointer must hold n + 1 entries'
        nnz = int(ptr[-1])
        assert len(idx) == nnz and len(val) == nnz, 'cof_set_sppmi: idx and val must hold nnz entries'
        idx, b = _i32(idx if nnz else np.zeros(1, np.int32))
        val, c = _f64(val if nnz else np.zeros(1, np.float64))
        self._chk(self._lib.yue_cof_set_sppmi(self._ctx, a, b, c, C.c_int64(nnz)))

    def cof_set_state(self, G, w, c):
        G, a = _f64(G)
        w, b = _f64(w)
        c, d = _f64(c)
        assert G.shape == (self.n, self.k) and w.shape == (self.n,) and c.shape == (self.n,), 'cof_set_state: G [n, k], w [n], c [n]'
        self._chk(self._lib.yue_cof_set_state(self._ctx, a, b, d))

    def cof_get_state(self):
        G = np.empty((self.n, self.k), np.float64)
        w = np.empty(self.n, np.float64)
        c = np.empty(self.n, np.float64)
        self._chk(self._lib.yue_cof_get_state(self._ctx, G.ctypes.data_as(C.POINTER(C.c_double)), w.ctypes.data_as(C.POINTER(C.c_double)),
                                              c.ctypes.data_as(C.POINTER(C.c_double))))
        return G, w, c

    def cof_item_sweep(self, alpha, regU, regR):
        self._chk(self._lib.yue_cof_item_sweep(self._ctx, C.c_double(alpha), C.c_double(regU), C.c_double(regR)))

    # -- UserKNN (needs no factors) ------------------------------------------------------------
    def knn_set_pairs(self, m, n, u_ptr, u_items, u_counts, i_ptr, i_users):
        """Distinct pairs both ways: user-major (items ascending, with event counts) and item-major (users ascending)."""
        u_ptr, a = _i64(u_ptr)
        i_ptr, e = _i64(i_ptr)
        assert len(u_ptr) == m + 1 and len(i_ptr) == n + 1, 'knn_set_pairs: pointer sizes must be m + 1, n + 1'
        nnz = int(u_ptr[-1])
        assert int(i_ptr[-1]) == nnz and len(u_items) == nnz and len(u_counts) == nnz and len(i_users) == nnz, \
            'knn_set_pairs: both directions must hold nnz pairs'
        u_items, b = _i32(u_items if nnz else np.zeros(1, np.int32))
        u_counts, c = _i32(u_counts if nnz else np.zeros(1, np.int32))
        i_users, f = _i32(i_users if nnz else np.zeros(1, np.int32))
        self._chk(self._lib.yue_knn_set_pairs(self._ctx, C.c_int64(m), C.c_int64(n), a, b, c, e, f, C.c_int64(nnz)))
        self.knn_m, self.knn_n = int(m), int(n)

    def knn_neighbors(self, K):
        """(nbr, inter, union), each int32 [m, K]: the first K positive-similarity users by (sim desc, id asc), -1 / 0 / 0 padded."""
        out = [np.empty((self.knn_m, max(int(K), 0)), np.int32) for _ in range(3)]
        ptrs = [o.ctypes.data_as(C.POINTER(C.c_int32)) for o in out]
        self._chk(self._lib.yue_knn_neighbors(self._ctx, C.c_int(K), *ptrs))
        return tuple(out)

    def knn_predict(self, user):
        """(items int32, scores float64): the full list of one user by (score desc, item asc), own items included."""
        items = np.empty(self.knn_n, np.int32)
        scores = np.empty(self.knn_n, np.float64)
        length = C.c_int64()
        self._chk(self._lib.yue_knn_predict(self._ctx, C.c_int32(int(user)), C.c_int64(self.knn_n), items.ctypes.data_as(C.POINTER(C.c_int32)),
                                            scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(length)))
        return items[:length.value], scores[:length.value]

    def knn_topn(self, users, N):
        """(ids int32 [nu, N] -1 padded, scores float64 [nu, N] 0 padded, lens int32 [nu]) without each user's own items."""
        users, up = _i32(users)
        nu = len(users)
        ids = np.empty((nu, max(int(N), 0)), np.int32)
        scores = np.empty((nu, max(int(N), 0)), np.float64)
        lens = np.empty(nu, np.int32)
        self._chk(self._lib.yue_knn_topn(self._ctx, up, C.c_int64(nu), C.c_int(N), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                         scores.ctypes.data_as(C.POINTER(C.c_double)), lens.ctypes.data_as(C.POINTER(C.c_int32))))
        return ids, scores, lens

    # -- IPF (needs no factors) -----------------------------------------------------------------
    def ipf_set_graph(self, g):
        """Upload the session temporal graph ``g`` (yue_amd/recommender/cf/IPF.py: ipf_graph): per-user distinct lists
        u_ptr/u_items and s_ptr/s_items, holder lists hu_ptr/hu_users and hs_ptr/hs_users/hs_pos, the weights w_user,
        w_sess, p_i2u, p_i2s and r_user = beta, r_sess = 1 - beta."""
        m, n = int(g['m']), int(g['n'])
        keep = []

        def arr(key, conv, size=None):
            a, p = conv(g[key] if len(g[key]) else np.zeros(1, np.int32))
            assert size is None or len(a) == size, 'ipf_set_graph: %s must hold %d entries' % (key, size)
            keep.append(a)
            return p
        ptrs = [arr('u_ptr', _i64, m + 1), arr('u_items', _i32), arr('s_ptr', _i64, m + 1), arr('s_items', _i32),
                arr('hu_ptr', _i64, n + 1), arr('hu_users', _i32), arr('hs_ptr', _i64, n + 1), arr('hs_users', _i32),
                arr('hs_pos', _i32)]
        assert len(g['u_items']) == g['u_ptr'][-1] and len(g['s_items']) == g['s_ptr'][-1] and len(g['hu_users']) == g['hu_ptr'][-1] \
            and len(g['hs_users']) == g['hs_ptr'][-1] == len(g['hs_pos']), 'ipf_set_graph: list lengths must match their pointers'
        weights = []
        for key, size in (('w_user', m), ('w_sess', m), ('p_i2u', n), ('p_i2s', n)):
            a, p = _f64(g[key])
            assert len(a) == size, 'ipf_set_graph: %s must hold %d entries' % (key, size)
            keep.append(a)
            weights.append(p)
        self._chk(self._lib.yue_ipf_set_graph(self._ctx, C.c_int64(m), C.c_int64(n), *ptrs, *weights,
                                              C.c_double(g['r_user']), C.c_double(g['r_sess'])))
        self.ipf_m, self.ipf_n = m, n

    def ipf_predict(self, user):
        """(items int32, scores float64): the full list of one user by (score desc, first insertion asc), own items included."""
        items = np.empty(max(self.ipf_n, 1), np.int32)
        scores = np.empty(max(self.ipf_n, 1), np.float64)
        length = C.c_int64()
        self._chk(self._lib.yue_ipf_predict(self._ctx, C.c_int32(int(user)), C.c_int64(self.ipf_n), items.ctypes.data_as(C.POINTER(C.c_int32)),
                                            scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(length)))
        return items[:length.value], scores[:length.value]

    def ipf_topn(self, users, N):
        """(ids int32 [nu, N] -1 padded, scores float64 [nu, N] 0 padded, lens int32 [nu]) without each user's own items."""
        users, up = _i32(users)
        nu = len(users)
        ids = np.empty((nu, max(int(N), 0)), np.int32)
        scores = np.empty((nu, max(int(N), 0)), np.float64)
        lens = np.empty(nu, np.int32)
        self._chk(self._lib.yue_ipf_topn(self._ctx, up, C.c_int64(nu), C.c_int(N), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                         scores.ctypes.data_as(C.POINTER(C.c_double)), lens.ctypes.data_as(C.POINTER(C.c_int32))))
        return ids, scores, lens

    # -- CUNE's user-network stage (needs no factors) --------------------------------------------
    # -- Song2vec ---------------------------------------------------------------------------
    def s2v_set_state(self, Bu, Bi):
        Bu, a = _f64(Bu)
        Bi, b = _f64(Bi)
        assert Bu.shape == (self.m,) and Bi.shape == (self.n,), 's2v_set_state: Bu [m], Bi [n]'
        self._chk(self._lib.yue_s2v_set_state(self._ctx, a, b))

    def s2v_get_state(self):
        Bu, Bi = np.empty(self.m, np.float64), np.empty(self.n, np.float64)
        self._chk(self._lib.yue_s2v_get_state(self._ctx, Bu.ctypes.data_as(C.POINTER(C.c_double)), Bi.ctypes.data_as(C.POINTER(C.c_double))))
        return Bu, Bi

    def s2v_set_steps(self, u, i, count):
        u, a = _i32(u)
        i, b = _i32(i)
        count, d = _i32(count)
        assert len(u) == len(i) == len(count), 's2v_set_steps: u, i and count must hold one entry per step'
        self._s2v_T = len(u)
        self._chk(self._lib.yue_s2v_set_steps(self._ctx, a, b, d, C.c_int64(len(u))))

    def s2v_set_pairs(self, t1, t2, sim):
        t1, a = _i32(t1)
        t2, b = _i32(t2)
        sim, d = _f64(sim)
        assert len(t1) == len(t2) == len(sim), 's2v_set_pairs: t1, t2 and sim must hold one entry per pair'
        self._s2v_P = len(t1)
        self._chk(self._lib.yue_s2v_set_pairs(self._ctx, a, b, d, C.c_int64(len(t1))))

    def s2v_epoch(self, lr, regU, regI, regB, alpha, globalMean=0.0):
        """One iteration of Song2vec.py:163-189.  Returns the squared errors per step and per pair (float64)."""
        e1 = np.zeros(getattr(self, '_s2v_T', 0), np.float64)
        e2 = np.zeros(getattr(self, '_s2v_P', 0), np.float64)
        self._chk(self._lib.yue_s2v_epoch(self._ctx, C.c_double(lr), C.c_double(regU), C.c_double(regI), C.c_double(regB), C.c_double(alpha),
                                          C.c_double(globalMean), e1.ctypes.data_as(C.POINTER(C.c_double)), e2.ctypes.data_as(C.POINTER(C.c_double))))
        return e1, e2

    def cnet_set_pairs(self, m, n, u_ptr, u_items, i_ptr, i_users):
        """Distinct pairs both ways: user-major (items ascending) and item-major (users ascending)."""
        u_ptr, a = _i64(u_ptr)
        i_ptr, e = _i64(i_ptr)
        assert len(u_ptr) == m + 1 and len(i_ptr) == n + 1, 'cnet_set_pairs: pointer sizes must be m + 1, n + 1'
        nnz = int(u_ptr[-1])
        assert int(i_ptr[-1]) == nnz and len(u_items) == nnz and len(i_users) == nnz, 'cnet_set_pairs: both directions must hold nnz pairs'
        u_items, b = _i32(u_items if nnz else np.zeros(1, np.int32))
        i_users, f = _i32(i_users if nnz else np.zeros(1, np.int32))
        self._chk(self._lib.yue_cnet_set_pairs(self._ctx, C.c_int64(m), C.c_int64(n), a, b, e, f, C.c_int64(nnz)))
        self.cnet_m = int(m)

    def cnet_walks(self, T, L, seed):
        """int32 [nw, L]: T walks per network user in training (shuffled) order; they stay on the device for cnet_embed."""
        out = np.empty((self.cnet_m * max(int(T), 0), max(int(L), 0)), np.int32)
        nw = C.c_int64()
        self._chk(self._lib.yue_cnet_walks(self._ctx, C.c_int(T), C.c_int(L), C.c_uint64(seed), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nw)))
        return out.reshape(-1)[:nw.value * int(L)].reshape(nw.value, int(L))

    def cnet_set_walks(self, m, walks):
        walks, p = _i32(walks)
        assert walks.ndim == 2
        self._chk(self._lib.yue_cnet_set_walks(self._ctx, C.c_int64(m), C.c_int64(walks.shape[0]), C.c_int(walks.shape[1]), p))
        self.cnet_m = int(m)

    def cnet_set_sentences(self, m, ptr, ids):
        """Sentences of unequal length (ids below m; ptr [ns + 1]); cnet_embed cuts them into segments."""
        ptr, a = _i64(ptr)
        ids, b = _i32(ids)
        assert len(ptr) >= 2 and int(ptr[-1]) == len(ids), 'cnet_set_sentences: the pointer must run from 0 to the number of words'
        self._chk(self._lib.yue_cnet_set_sentences(self._ctx, C.c_int64(m), C.c_int64(len(ptr) - 1), a, b))
        self.cnet_m = int(m)

    def cnet_embed(self, dim, window, epochs, seed, negative=5, round_walks=0):
        """float32 [m, dim]: the CBOW user embedding of the walks on the device (rows of users outside the walks are 0)."""
        W = np.empty((self.cnet_m, max(int(dim), 0)), np.float32)
        self._chk(self._lib.yue_cnet_embed(self._ctx, C.c_int(dim), C.c_int(window), C.c_int(epochs), C.c_int(negative), C.c_int64(round_walks),
                                           C.c_uint64(seed), W.ctypes.data_as(C.POINTER(C.c_float))))
        self.cnet_dim = int(dim)
        return W

    def cnet_set_embedding(self, W, users=None):
        W, p = _f32(W)
        assert W.ndim == 2
        up, nu = None, 0
        if users is not None:
            users, up = _i32(users)
            nu = len(users)
        self._chk(self._lib.yue_cnet_set_embedding(self._ctx, C.c_int64(W.shape[0]), C.c_int(W.shape[1]), p, up, C.c_int64(nu)))
        self.cnet_m, self.cnet_dim = W.shape

    def cnet_friends(self, K):
        """(friends int32 [m, K] -1 padded, cosines float64 [m, K] 0 padded) by (cosine desc, id asc)."""
        friends = np.empty((self.cnet_m, max(int(K), 0)), np.int32)
        sims = np.empty((self.cnet_m, max(int(K), 0)), np.float64)
        self._chk(self._lib.yue_cnet_friends(self._ctx, C.c_int(K), friends.ctypes.data_as(C.POINTER(C.c_int32)), sims.ctypes.data_as(C.POINTER(C.c_double))))
        return friends, sims

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._chk(self._lib.yue_comm_init(self._ctx, buf, C.c_int(rank), C.c_int(nranks)))

    def comm_stats(self):
        """Last bpr_epoch on a communicator: dict(allreduce_bytes, collectives, wait_ms, nranks, rccl_version)."""
        b, n, w, r, v = C.c_double(), C.c_int64(), C.c_double(), C.c_int(), C.c_int()
        self._chk(self._lib.yue_get_comm_stats(self._ctx, C.byref(b), C.byref(n), C.byref(w), C.byref(r), C.byref(v)))
        return {'allreduce_bytes': b.value, 'collectives': n.value, 'wait_ms': w.value, 'nranks': r.value, 'rccl_version': v.value}

    def allreduce_f64(self, vals):
        arr = (C.c_double * len(vals))(*vals)
        self._chk(self._lib.yue_allreduce_f64(self._ctx, arr, C.c_int(len(vals))))
        return list(arr)
