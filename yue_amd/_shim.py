"""ctypes binding of libyue_hip.so (include/yue_hip.h, and include/yue_apr.h, which it includes).

This is the only route from the Python plugin surface to the numeric hot path: there is no
CPU fallback.  If the library is missing or no MI355X is visible, calls fail loudly in the
reference's style -- print the message, exit(-1) (tool/config.py:9-11,
base/IterativeRecommender.py:64-66) -- or raise YueHipError when ``raise_errors`` is set
(tests use that).

Every exported function's C signature stands once, in SIGNATURES (APR's in APR_SIGNATURES, beside its own header); load_library() turns it into
``restype`` and ``argtypes``, so a call site passes Python numbers and NumPy arrays as they are and
ctypes converts or refuses each argument (tests/test_shim_signatures.py holds the table against the header).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libyue_hip.so')

OK, ERR_ARG, ERR_HIP, ERR_FEW_ITEMS, ERR_COMM, ERR_SATURATED = 0, -1, -2, -3, -4, -5
UNIQUE_ID_BYTES = 128


class _Pointer(object):
    """The argument type of an `elem *` parameter: None (where the header lets the pointer be NULL), a byref or a ctypes
    array of elem, or a C-contiguous ndarray of exactly elem's dtype.  Anything else is a TypeError before the call."""

    def __init__(self, elem):
        self.ctype, self.dtype = C.POINTER(elem), np.dtype(elem)

    def from_param(self, obj):
        if isinstance(obj, np.ndarray):
            if obj.dtype != self.dtype or not obj.flags.c_contiguous:
                raise TypeError('a C-contiguous %s array is expected, not %s%s'
                                % (self.dtype, obj.dtype, '' if obj.flags.c_contiguous else ' (not contiguous)'))
            return obj.ctypes                                # (holds the array; ctypes reads its _as_parameter_)
        return self.ctype.from_param(obj)


# the parameter types of include/yue_hip.h, const dropped
TYPES = {'ctx': C.c_void_p, 'ctx*': C.POINTER(C.c_void_p), 'str': C.c_char_p, 'void*': C.c_void_p,
         'int': C.c_int, 'i32': C.c_int32, 'u32': C.c_uint32, 'i64': C.c_int64, 'u64': C.c_uint64, 'f64': C.c_double,
         'f32*': _Pointer(C.c_float), 'f64*': _Pointer(C.c_double), 'i32*': _Pointer(C.c_int32), 'i64*': _Pointer(C.c_int64),
         'int*': _Pointer(C.c_int), 'f32**': C.POINTER(C.POINTER(C.c_float))}

_PAIRS = 'ctx i64* i32* i32* i64* i32* i32* i64'
_PREDICT = 'ctx i32 i64 i32* f64* i64*'
_TOPN = 'ctx i32* i64 int i32* f64* i32*'

# every function include/yue_hip.h declares: its parameters in order, and '-> type' where it does not return int
SIGNATURES = {
    'yue_last_error': '-> str',
    'yue_version': '',
    'yue_ctx_create': 'int ctx*',
    'yue_ctx_destroy': 'ctx',
    'yue_sync': 'ctx',
    'yue_set_factors': 'ctx f32* i64 f32* i64 int',
    'yue_get_factors': 'ctx f32* f32*',
    'yue_set_interactions': 'ctx i64* i32* i64* i32*',
    'yue_bpr_replay': 'ctx i32* i32* i32* i64 f64 f64 f64 f64*',
    'yue_adam_reset': 'ctx',
    'yue_adam_get_moments': 'ctx f32* f32* f32* f32*',
    'yue_adam_step': 'ctx i32* i32* i32* i64 f64 f64 i64 f64*',
    'yue_cune_steps': 'ctx i32* i32* i32* i32* i64 f64 f64 f64 f64 f64*',
    'yue_bpr_rounds': 'ctx i32* i32* i32* i64* i64 f64 f64 f64 f64*',
    'yue_bpr_epoch': 'ctx u64 u32 i64 f64 f64 f64 f64* f64* f64*',
    'yue_epoch_plan': 'i64 int i64 f64 int i64* i64* i64*',
    'yue_default_round_events': 'ctx i64*',
    'yue_sample_negatives': 'ctx u64 u32 i32*',
    'yue_sumsq': 'ctx f64* f64*',
    'yue_scores': 'ctx i32 f32*',
    'yue_topn_scan': 'ctx i32* i64 int i64* i32* i32* f32*',
    'yue_set_kernel_timing': 'ctx int',
    'yue_get_kernel_timing': 'ctx f64* i64* i64*',
    'yue_get_scan_stats': 'ctx f64* i64* i64* int*',
    'yue_get_scan_work': 'ctx i64* i64*',
    'yue_set_option': 'ctx str i64',
    'yue_get_option': 'ctx str i64*',
    'yue_fism_set_model': 'ctx f64* f32* f64* i64 int',
    'yue_fism_get_model': 'ctx f64* f32* f64*',
    'yue_fism_epoch': 'ctx i64* i64 i32* i32* i64 int f64* f64 f64 f64 f64* f64*',
    'yue_fism_rounds': 'ctx i64* i64 i32* i32* i64 int f64* i64 f64 f64 f64 f64* f64*',
    'yue_fism_scores': 'ctx i32* i64 f64*',
    'yue_fism_topn_scan': 'ctx i64* i32* i64 int i32* f64*',
    'yue_wrmf_set_pairs': _PAIRS,
    'yue_wrmf_half_sweep': 'ctx int f64 f64 f64*',
    'yue_expo_set_pairs': _PAIRS,
    'yue_expo_set_mu': 'ctx f32* i64',
    'yue_expo_get_mu': 'ctx f32* i64',
    'yue_expo_half_sweep': 'ctx int f64 f64 int',
    'yue_expo_update_mu': 'ctx f64 f64 f64',
    'yue_expo_gram_rows': 'ctx int int f64 i32* i64 f64*',
    'yue_cof_cooccur': 'ctx int i64*',
    'yue_cof_get_cooccur': 'ctx i64* i32* i32*',
    'yue_cof_set_sppmi': 'ctx i64* i32* f64* i64',
    'yue_cof_set_state': 'ctx f64* f64* f64*',
    'yue_cof_get_state': 'ctx f64* f64* f64*',
    'yue_cof_item_sweep': 'ctx f64 f64 f64',
    'yue_knn_set_pairs': 'ctx i64 i64 i64* i32* i32* i64* i32* i64',
    'yue_knn_neighbors': 'ctx int i32* i32* i32*',
    'yue_knn_predict': _PREDICT,
    'yue_knn_topn': _TOPN,
    'yue_ipf_set_graph': 'ctx i64 i64 i64* i32* i64* i32* i64* i32* i64* i32* i32* f64* f64* f64* f64* f64 f64',
    'yue_ipf_predict': _PREDICT,
    'yue_ipf_topn': _TOPN,
    'yue_cnet_set_pairs': 'ctx i64 i64 i64* i32* i64* i32* i64',
    'yue_cnet_walks': 'ctx int int u64 i32* i64*',
    'yue_cnet_set_walks': 'ctx i64 i64 int i32*',
    'yue_cnet_set_sentences': 'ctx i64 i64 i64* i32*',
    'yue_cnet_embed': 'ctx int int int int i64 u64 f32*',
    'yue_cnet_set_embedding': 'ctx i64 int f32* i32* i64',
    'yue_cnet_friends': 'ctx int i32* f64*',
    'yue_s2v_set_state': 'ctx f64* f64*',
    'yue_s2v_get_state': 'ctx f64* f64*',
    'yue_s2v_set_steps': 'ctx i32* i32* i32* i64',
    'yue_s2v_set_pairs': 'ctx i32* i32* f64* i64',
    'yue_s2v_epoch': 'ctx f64 f64 f64 f64 f64 f64 f64* f64*',
    'yue_lgcn_set_graph': 'ctx i64 i64 i64* i32* f32* i64* i32* f32*',
    'yue_lgcn_propagate': 'ctx int f32* f32*',
    'yue_lgcn_grad': 'ctx int i32* i32* i32* i64 f64 f64* f32* f32*',
    'yue_lgcn_step': 'ctx int i32* i32* i32* i64 f64 f64 i64 f64*',
    'yue_ngcf_set_graph': 'ctx i64 i64 i64* i32* f32*',
    'yue_ngcf_set_weights': 'ctx int int f32*',
    'yue_ngcf_get_weights': 'ctx f32* f32* f32*',
    'yue_ngcf_propagate': 'ctx int int f64 u64 i64 f32* f32* f32* f32*',
    'yue_ngcf_grad': 'ctx int int f64 u64 i64 i32* i32* i32* i64 f64 f64* f32* f32* f32*',
    'yue_ngcf_step': 'ctx int int f64 u64 i32* i32* i32* i64 f64 f64 i64 f64*',
    'yue_cdae_set_data': 'ctx i64 i64 i64* i32* i32*',
    'yue_cdae_set_params': 'ctx int f32* f32* f32* f32* f32*',
    'yue_cdae_get_params': 'ctx f32** f32** f32**',
    'yue_cdae_forward': 'ctx i32* i64 i64* i32* f64 u64 i64 f64 f32* i32* f32* f32* f64*',
    'yue_cdae_grad': 'ctx i32* i64 i64* i32* f64 u64 i64 f64 f64* f32* f32* f32* f32* f32*',
    'yue_cdae_step': 'ctx i32* i64 i64* i32* f64 u64 f64 f64 i64 f64*',
    'yue_cdae_load_factors': 'ctx',
    'yue_cdae_times': 'ctx i64*',
    'yue_comm_unique_id': 'void*',
    'yue_comm_init': 'ctx void* int int',
    'yue_allreduce_f64': 'ctx f64* int',
    'yue_get_comm_stats': 'ctx f64* i64* f64* int* int*',
}
SYMBOLS = list(SIGNATURES)                                   # (checked against the header by tests/test_abi.py)

# ... and every function include/yue_apr.h declares, which yue_hip.h includes (tests/test_apr_signatures.py)
APR_SIGNATURES = {
    'yue_apr_reset': 'ctx',
    'yue_apr_pre_step': 'ctx i32* i32* i32* i64 f64 f64 i64 f64*',
    'yue_apr_adv_step': 'ctx i32* i32* i32* i64 f64 f64 f64 i64 f64*',
    'yue_apr_set_delta': 'ctx i32* i64 f32* i32* i64 f32*',
    'yue_apr_get_delta': 'ctx f32* f32*',
    'yue_apr_delta_update': 'ctx i32* i32* i32* i64 f64 f64 f32* f32*',
    'yue_apr_grad': 'ctx int i32* i32* i32* i64 f64 f64* f32* f32*',
    'yue_apr_times': 'ctx i64*',
}


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
        for name, signature in list(SIGNATURES.items()) + list(APR_SIGNATURES.items()):
            params, _, returns = signature.partition('->')
            fn = getattr(lib, name)
            fn.restype = TYPES[returns.strip() or 'int']
            fn.argtypes = [TYPES[t] for t in params.split()]
        _lib = lib
    return _lib


def _in(a, dtype, placeholder=False):
    """An input list as a C-contiguous array of dtype.  With `placeholder` an empty list becomes one element, passed with a
    length of 0: the library asks for a pointer it may not read."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if not placeholder or len(a) else np.zeros(1, dtype)


def _triplets(u, i, j, who=None):
    u, i, j = _in(u, np.int32), _in(i, np.int32), _in(j, np.int32)
    assert who is None or len(u) == len(i) == len(j), '%s: one u, i, j per triplet' % who
    return u, i, j


def _pairs(who, m, n, sizes, u_ptr, u_lists, i_ptr, i_lists):
    """(u_ptr, *u_lists, i_ptr, *i_lists, nnz): the arguments of an upload of the distinct pairs both ways."""
    u_ptr, i_ptr = _in(u_ptr, np.int64), _in(i_ptr, np.int64)
    assert len(u_ptr) == m + 1 and len(i_ptr) == n + 1, '%s: pointer sizes must %s' % (who, sizes)
    nnz = int(u_ptr[-1])
    assert int(i_ptr[-1]) == nnz and all(len(x) == nnz for x in u_lists + i_lists), '%s: both directions must hold nnz pairs' % who
    return (u_ptr, *[_in(x, np.int32, True) for x in u_lists], i_ptr, *[_in(x, np.int32, True) for x in i_lists], nnz)


def _raise_unless_ok(lib, rc):
    if rc != OK:
        raise YueHipError(rc, lib.yue_last_error().decode())


def comm_unique_id():
    lib = load_library()
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    _raise_unless_ok(lib, lib.yue_comm_unique_id(buf))
    return bytes(buf)


def epoch_plan(m, k, round_events, events_total, nranks):
    """(user_block, blocks_per_group, n_blocks) of yue_bpr_epoch's schedule -- pure host arithmetic inside the library."""
    lib = load_library()
    ub, grp, nb = C.c_int64(), C.c_int64(), C.c_int64()
    _raise_unless_ok(lib, lib.yue_epoch_plan(m, k, round_events, events_total, nranks, C.byref(ub), C.byref(grp), C.byref(nb)))
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
        self._s2v_T = self._s2v_P = 0
        self.ngcf_w_shape = (0, 2, 0, 0)
        self.cdae_m = self.cdae_n = self.cdae_h = 0
        self.cdae_nnz_ptr = np.zeros(self.cdae_m + 1, np.int64)
        self._chk(self._lib.yue_ctx_create(device, C.byref(self._ctx)))

    # reference convention: print, exit(-1)
    def _chk(self, rc):
        if rc == OK:
            return
        msg = self._lib.yue_last_error().decode()
        if self._raise:
            raise YueHipError(rc, msg)
        print(msg)
        exit(-1)

    def _status(self, name, *args):
        """The status of library function `name` on this context, for the callers that treat one themselves."""
        return getattr(self._lib, name)(self._ctx, *args)

    def _call(self, name, *args):
        self._chk(getattr(self._lib, name)(self._ctx, *args))

    def _read(self, name, count, *args):
        """Calls `name` with an output cell behind args for each of its last `count` parameters; returns the cells' values."""
        fn = getattr(self._lib, name)
        cells = [pointer.ctype._type_() for pointer in fn.argtypes[-count:]]
        self._chk(fn(self._ctx, *args, *[C.byref(cell) for cell in cells]))
        return [cell.value for cell in cells]

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
        self._call('yue_sync')

    # -- state ------------------------------------------------------------------------
    def set_factors(self, P, Q):
        P, Q = _in(P, np.float32), _in(Q, np.float32)
        assert P.ndim == 2 and Q.ndim == 2 and P.shape[1] == Q.shape[1]
        self.m, self.k = P.shape
        self.n = Q.shape[0]
        self._call('yue_set_factors', P, self.m, Q, self.n, self.k)

    def get_factors(self, P=None, Q=None):
        """Copies the device factors into P, Q (allocated when None) and returns them."""
        if P is None:
            P = np.empty((self.m, self.k), np.float32)
        if Q is None:
            Q = np.empty((self.n, self.k), np.float32)
        assert P.dtype == np.float32 and Q.dtype == np.float32 and P.flags.c_contiguous and Q.flags.c_contiguous
        self._call('yue_get_factors', P, Q)
        return P, Q

    def set_interactions(self, indptr, indices, ev_ptr, ev_i):
        indptr, indices = _in(indptr, np.int64), _in(indices, np.int32, True)
        ev_ptr, ev_i = _in(ev_ptr, np.int64), _in(ev_i, np.int32, True)
        assert len(indptr) == self.m + 1 and len(ev_ptr) == self.m + 1
        self.E = int(ev_ptr[-1])
        self._call('yue_set_interactions', indptr, indices, ev_ptr, ev_i)

    # -- training -----------------------------------------------------------------------
    def bpr_replay(self, u, i, j, lr, regU, regI):
        u, i, j = _triplets(u, i, j)
        return self._read('yue_bpr_replay', 1, u, i, j, len(u), lr, regU, regI)[0]

    def adam_reset(self):
        self._call('yue_adam_reset')

    def adam_get_moments(self):
        """(mU, vU, mV, vV) of the uploaded factors' Adam state."""
        out = [np.empty((r, self.k), np.float32) for r in (self.m, self.m, self.n, self.n)]
        self._call('yue_adam_get_moments', *out)
        return tuple(out)

    def adam_step(self, u, i, j, lr, reg, step):
        """One minibatch step of the reference's live TF-style path (softplus loss + l2 terms, Adam).  Returns total_loss."""
        u, i, j = _triplets(u, i, j)
        return self._read('yue_adam_step', 1, u, i, j, len(u), lr, reg, step)[0]

    def cune_steps(self, u, i, k, j, s, lr, regU, regI):
        """CUNE's two-level BPR steps in order (k < 0: plain step).  Returns the per-step losses (float64[T])."""
        u, i, j = _triplets(u, i, j)
        k = _in(k, np.int32)
        loss = np.empty(len(u), np.float64)
        self._call('yue_cune_steps', u, i, k, j, len(u), s, lr, regU, regI, loss)
        return loss

    def bpr_rounds(self, u, i, j, round_ptr, lr, regU, regI):
        u, i, j = _triplets(u, i, j)
        round_ptr = _in(round_ptr, np.int64)
        return self._read('yue_bpr_rounds', 1, u, i, j, round_ptr, len(round_ptr) - 1, lr, regU, regI)[0]

    def bpr_epoch(self, seed, epoch, round_events, lr, regU, regI):
        """Returns (nll, sumsqP, sumsqQ) after one epoch (device sampler + S-rounds; round_events 0 = the device default)."""
        return tuple(self._read('yue_bpr_epoch', 3, seed, epoch, round_events, lr, regU, regI))

    def default_round_events(self):
        return self._read('yue_default_round_events', 1)[0]

    def sample_negatives(self, seed, epoch):
        j = np.empty(max(self.E, 1), np.int32)
        self._call('yue_sample_negatives', seed, epoch, j)
        return j[:self.E]

    def sumsq(self):
        return tuple(self._read('yue_sumsq', 2))

    # -- scoring ------------------------------------------------------------------------
    def scores(self, user):
        out = np.empty(self.n, np.float32)
        self._call('yue_scores', user, out)
        return out

    def topn_scan(self, users, N, mask_indptr=None, mask_indices=None):
        """(ids[nu,N] int32, scores[nu,N] float32).  Raises IndexError like the reference
        (base/IterativeRecommender.py:126) when a user has fewer than N candidates."""
        users = _in(users, np.int32)
        ids = np.empty((len(users), N), np.int32)
        sc = np.empty((len(users), N), np.float32)
        if mask_indptr is None:
            mask_indices = None
        else:
            mask_indptr, mask_indices = _in(mask_indptr, np.int64), _in(mask_indices, np.int32, True)
        rc = self._status('yue_topn_scan', users, len(users), N, mask_indptr, mask_indices, ids, sc)
        if rc == ERR_FEW_ITEMS:
            raise IndexError('list index out of range')
        self._chk(rc)
        return ids, sc

    # -- measurement and options ----------------------------------------------------------
    def set_kernel_timing(self, stride):
        self._call('yue_set_kernel_timing', stride)

    def get_kernel_timing(self):
        return tuple(self._read('yue_get_kernel_timing', 3))

    def scan_stats(self):
        """(kernel ms, state-machine events, exact re-scores, used_bf16) of the last topn_scan."""
        ms, ev, rs, bf = self._read('yue_get_scan_stats', 4)
        return ms, ev, rs, bool(bf)

    def scan_work(self):
        """(tiles scored, tiles of the full product) of the last topn_scan (32 users x 32 items each)."""
        return tuple(self._read('yue_get_scan_work', 2))

    def set_option(self, name, value):
        self._call('yue_set_option', name.encode(), value)

    def get_option(self, name):
        return self._read('yue_get_option', 1, name.encode())[0]

    # -- FISM (parity path) ---------------------------------------------------------------
    def fism_set_model(self, P, Q, Bi):
        P, Q, Bi = _in(P, np.float64), _in(Q, np.float32), _in(Bi, np.float64)
        assert P.shape == Q.shape and len(Bi) == P.shape[0]
        self._call('yue_fism_set_model', P, Q, Bi, P.shape[0], P.shape[1])
        self.fn, self.fk = P.shape                       # (after the check: a refused upload leaves the earlier model and its shape)

    def fism_get_model(self, P, Q, Bi):
        """Copies the device model into the given arrays (float64 [n,k], float32 [n,k], float64 [n])."""
        assert P.dtype == np.float64 and Q.dtype == np.float32 and Bi.dtype == np.float64
        assert P.flags.c_contiguous and Q.flags.c_contiguous and Bi.flags.c_contiguous
        self._call('yue_fism_get_model', P, Q, Bi)

    def _fism_pass(self, name, user_ptr, ev_i, negs, rho, coef, *rates):
        """yue_fism_epoch or yue_fism_rounds: `rates` is what follows coef, up to regB."""
        user_ptr = _in(user_ptr, np.int64)
        half = C.c_double()
        sums = (C.c_double * 3)()
        self._call(name, user_ptr, len(user_ptr) - 1, _in(ev_i, np.int32, True), _in(negs, np.int32, True), len(negs), rho,
                   _in(coef, np.float64), *rates, C.byref(half), sums)
        return half.value, sums[0], sums[1], sums[2]

    def fism_epoch(self, user_ptr, ev_i, negs, rho, coef, lr, regI, regB):
        """One sequential pass (FISM.py:38-69).  Returns (sum of 0.5*error^2, sum(P*P), sum(Q*Q), Bi.Bi)."""
        return self._fism_pass('yue_fism_epoch', user_ptr, ev_i, negs, rho, coef, lr, regI, regB)

    def fism_rounds(self, user_ptr, ev_i, negs, rho, coef, round_users, lr, regI, regB):
        """The same pass in rounds of `round_users` users (throughput form).  Returns (sum of 0.5*error^2, sum(P*P), sum(Q*Q), Bi.Bi)."""
        return self._fism_pass('yue_fism_rounds', user_ptr, ev_i, negs, rho, coef, round_users, lr, regI, regB)

    def fism_scores(self, items):
        out = np.empty(self.fn, np.float64)
        self._call('yue_fism_scores', _in(items, np.int32, True), len(items), out)
        return out

    def fism_topn_scan(self, row_ptr, row_items, N):
        """(ids[nu,N] int32, scores[nu,N] float64) for users given by the CSR of their training events."""
        row_ptr = _in(row_ptr, np.int64)
        nu = len(row_ptr) - 1
        ids = np.empty((nu, N), np.int32)
        sc = np.empty((nu, N), np.float64)
        rc = self._status('yue_fism_topn_scan', row_ptr, _in(row_items, np.int32, True), nu, N, ids, sc)
        if rc == ERR_FEW_ITEMS:
            raise IndexError(self._lib.yue_last_error().decode())
        self._chk(rc)
        return ids, sc

    # -- WRMF (ALS half-sweeps on the factors of set_factors) ----------------------------------
    def wrmf_set_pairs(self, u_ptr, u_items, u_counts, i_ptr, i_users, i_counts):
        """Distinct pairs both ways with their counts: user-major (items ascending) and item-major (users ascending)."""
        self._call('yue_wrmf_set_pairs', *_pairs('wrmf_set_pairs', self.m, self.n, 'match set_factors (m + 1, n + 1)',
                                                 u_ptr, [u_items, u_counts], i_ptr, [i_users, i_counts]))

    def wrmf_half_sweep(self, side, alpha, reg):
        """side 0: every user row from the item factors (returns the loss over the pairs, from the rows before the sweep);
        side 1: every item row from the user factors (returns 0.0)."""
        assert side in (0, 1)
        return self._read('yue_wrmf_half_sweep', 1, side, alpha, reg)[0]

    # -- ExpoMF (factors: theta = P, beta = Q) ---------------------------------------------------
    def expo_set_pairs(self, u_ptr, u_items, u_counts, i_ptr, i_users, i_counts):
        """The pairs of wrmf_set_pairs (the two ALS solvers share the upload, the schedule and the long rows' chunks)."""
        self._call('yue_expo_set_pairs', *_pairs('expo_set_pairs', self.m, self.n, 'match set_factors (m + 1, n + 1)',
                                                 u_ptr, [u_items, u_counts], i_ptr, [i_users, i_counts]))

    def expo_set_mu(self, mu):
        mu = _in(mu, np.float32)
        self._call('yue_expo_set_mu', mu, len(mu))

    def expo_get_mu(self):
        mu = np.empty(self.n, np.float32)
        self._call('yue_expo_get_mu', mu, self.n)
        return mu

    def expo_half_sweep(self, side, lam, lam_y, mu_per_column):
        """side 0: every user row from the item factors; side 1: every item row from the user factors."""
        self._call('yue_expo_half_sweep', side, lam, lam_y, 1 if mu_per_column else 0)

    def expo_update_mu(self, a, b, lam_y):
        self._call('yue_expo_update_mu', a, b, lam_y)

    def expo_gram_rows(self, side, mu_per_column, lam_y, rows):
        """Diagnostic: the dense stage of a half-sweep alone.  fp64 [len(rows), k(k+1)/2]: per listed row the packed lower
        triangle of sum over all columns of A~ f f^T (no A = 1 on the pairs, no lam*I), from the half-sweep's own Gram kernel."""
        rows = _in(rows, np.int32)
        out = np.empty((len(rows), self.k * (self.k + 1) // 2), np.float64)
        self._call('yue_expo_gram_rows', side, 1 if mu_per_column else 0, lam_y, rows, len(rows), out)
        return out

    # -- CoFactor (factors: X = P, Y = Q; pairs: wrmf_set_pairs; user sweep: wrmf_half_sweep(0, ...)) ----------------
    def cof_cooccur(self, filt):
        """Builds the co-occurrence CSR on the device; returns (ptr int64 [n+1], idx int32 ascending, cnt int32)."""
        nnz, = self._read('yue_cof_cooccur', 1, int(filt))
        ptr = np.empty(self.n + 1, np.int64)
        idx = np.empty(max(nnz, 1), np.int32)
        cnt = np.empty(max(nnz, 1), np.int32)
        self._call('yue_cof_get_cooccur', ptr, idx, cnt)
        return ptr, idx[:nnz], cnt[:nnz]

    def cof_set_sppmi(self, ptr, idx, val):
        ptr = _in(ptr, np.int64)
        assert len(ptr) == self.n + 1, 'cof_set_sppmi: the pointer must hold n + 1 entries'
        nnz = int(ptr[-1])
        assert len(idx) == nnz and len(val) == nnz, 'cof_set_sppmi: idx and val must hold nnz entries'
        self._call('yue_cof_set_sppmi', ptr, _in(idx, np.int32, True), _in(val, np.float64, True), nnz)

    def cof_set_state(self, G, w, c):
        G, w, c = _in(G, np.float64), _in(w, np.float64), _in(c, np.float64)
        assert G.shape == (self.n, self.k) and w.shape == (self.n,) and c.shape == (self.n,), 'cof_set_state: G [n, k], w [n], c [n]'
        self._call('yue_cof_set_state', G, w, c)

    def cof_get_state(self):
        G = np.empty((self.n, self.k), np.float64)
        w = np.empty(self.n, np.float64)
        c = np.empty(self.n, np.float64)
        self._call('yue_cof_get_state', G, w, c)
        return G, w, c

    def cof_item_sweep(self, alpha, regU, regR):
        self._call('yue_cof_item_sweep', alpha, regU, regR)

    # -- UserKNN (needs no factors) ------------------------------------------------------------
    def knn_set_pairs(self, m, n, u_ptr, u_items, u_counts, i_ptr, i_users):
        """Distinct pairs both ways: user-major (items ascending, with event counts) and item-major (users ascending)."""
        self._call('yue_knn_set_pairs', m, n, *_pairs('knn_set_pairs', m, n, 'be m + 1, n + 1', u_ptr, [u_items, u_counts], i_ptr, [i_users]))
        self.knn_m, self.knn_n = int(m), int(n)

    def knn_neighbors(self, K):
        """(nbr, inter, union), each int32 [m, K]: the first K positive-similarity users by (sim desc, id asc), -1 / 0 / 0 padded."""
        out = [np.empty((self.knn_m, max(int(K), 0)), np.int32) for _ in range(3)]
        self._call('yue_knn_neighbors', K, *out)
        return tuple(out)

    def _predict(self, name, user, n):
        """One user's full (items, scores) list of yue_knn_predict or yue_ipf_predict over n items."""
        items = np.empty(max(n, 1), np.int32)
        scores = np.empty(max(n, 1), np.float64)
        length, = self._read(name, 1, int(user), n, items, scores)
        return items[:length], scores[:length]

    def _topn(self, name, users, N):
        """The padded (ids, scores, lens) of yue_knn_topn or yue_ipf_topn."""
        users = _in(users, np.int32)
        nu = len(users)
        ids = np.empty((nu, max(int(N), 0)), np.int32)
        scores = np.empty((nu, max(int(N), 0)), np.float64)
        lens = np.empty(nu, np.int32)
        self._call(name, users, nu, N, ids, scores, lens)
        return ids, scores, lens

    def knn_predict(self, user):
        """(items int32, scores float64): the full list of one user by (score desc, item asc), own items included."""
        return self._predict('yue_knn_predict', user, self.knn_n)

    def knn_topn(self, users, N):
        """(ids int32 [nu, N] -1 padded, scores float64 [nu, N] 0 padded, lens int32 [nu]) without each user's own items."""
        return self._topn('yue_knn_topn', users, N)

    # -- IPF (needs no factors) -----------------------------------------------------------------
    def ipf_set_graph(self, g):
        """Upload the session temporal graph ``g`` (yue_amd/recommender/cf/IPF.py: ipf_graph): per-user distinct lists
        u_ptr/u_items and s_ptr/s_items, holder lists hu_ptr/hu_users and hs_ptr/hs_users/hs_pos, the weights w_user,
        w_sess, p_i2u, p_i2s and r_user = beta, r_sess = 1 - beta."""
        m, n = int(g['m']), int(g['n'])

        def arr(key, dtype, size=None, placeholder=True):
            a = _in(g[key], dtype, placeholder)
            assert size is None or len(a) == size, 'ipf_set_graph: %s must hold %d entries' % (key, size)
            return a
        lists = [arr('u_ptr', np.int64, m + 1), arr('u_items', np.int32), arr('s_ptr', np.int64, m + 1), arr('s_items', np.int32),
                 arr('hu_ptr', np.int64, n + 1), arr('hu_users', np.int32), arr('hs_ptr', np.int64, n + 1), arr('hs_users', np.int32),
                 arr('hs_pos', np.int32)]
        assert len(g['u_items']) == g['u_ptr'][-1] and len(g['s_items']) == g['s_ptr'][-1] and len(g['hu_users']) == g['hu_ptr'][-1] \
            and len(g['hs_users']) == g['hs_ptr'][-1] == len(g['hs_pos']), 'ipf_set_graph: list lengths must match their pointers'
        weights = [arr(key, np.float64, size, False) for key, size in (('w_user', m), ('w_sess', m), ('p_i2u', n), ('p_i2s', n))]
        self._call('yue_ipf_set_graph', m, n, *lists, *weights, g['r_user'], g['r_sess'])
        self.ipf_m, self.ipf_n = m, n

    def ipf_predict(self, user):
        """(items int32, scores float64): the full list of one user by (score desc, first insertion asc), own items included."""
        return self._predict('yue_ipf_predict', user, self.ipf_n)

    def ipf_topn(self, users, N):
        """(ids int32 [nu, N] -1 padded, scores float64 [nu, N] 0 padded, lens int32 [nu]) without each user's own items."""
        return self._topn('yue_ipf_topn', users, N)

    # -- CUNE's user-network stage (needs no factors) --------------------------------------------
    def cnet_set_pairs(self, m, n, u_ptr, u_items, i_ptr, i_users):
        """Distinct pairs both ways: user-major (items ascending) and item-major (users ascending)."""
        self._call('yue_cnet_set_pairs', m, n, *_pairs('cnet_set_pairs', m, n, 'be m + 1, n + 1', u_ptr, [u_items], i_ptr, [i_users]))
        self.cnet_m = int(m)

    def cnet_walks(self, T, L, seed):
        """int32 [nw, L]: T walks per network user in training (shuffled) order; they stay on the device for cnet_embed."""
        out = np.empty((self.cnet_m * max(int(T), 0), max(int(L), 0)), np.int32)
        nw, = self._read('yue_cnet_walks', 1, T, L, seed, out)
        return out.reshape(-1)[:nw * int(L)].reshape(nw, int(L))

    def cnet_set_walks(self, m, walks):
        walks = _in(walks, np.int32)
        assert walks.ndim == 2
        self._call('yue_cnet_set_walks', m, walks.shape[0], walks.shape[1], walks)
        self.cnet_m = int(m)

    def cnet_set_sentences(self, m, ptr, ids):
        """Sentences of unequal length (ids below m; ptr [ns + 1]); cnet_embed cuts them into segments."""
        ptr, ids = _in(ptr, np.int64), _in(ids, np.int32)
        assert len(ptr) >= 2 and int(ptr[-1]) == len(ids), 'cnet_set_sentences: the pointer must run from 0 to the number of words'
        self._call('yue_cnet_set_sentences', m, len(ptr) - 1, ptr, ids)
        self.cnet_m = int(m)

    def cnet_embed(self, dim, window, epochs, seed, negative=5, round_walks=0):
        """float32 [m, dim]: the CBOW user embedding of the walks on the device (rows of users outside the walks are 0)."""
        W = np.empty((self.cnet_m, max(int(dim), 0)), np.float32)
        self._call('yue_cnet_embed', dim, window, epochs, negative, round_walks, seed, W)
        self.cnet_dim = int(dim)
        return W

    def cnet_set_embedding(self, W, users=None):
        W = _in(W, np.float32)
        assert W.ndim == 2
        if users is not None:
            users = _in(users, np.int32)
        self._call('yue_cnet_set_embedding', W.shape[0], W.shape[1], W, users, 0 if users is None else len(users))
        self.cnet_m, self.cnet_dim = W.shape

    def cnet_friends(self, K):
        """(friends int32 [m, K] -1 padded, cosines float64 [m, K] 0 padded) by (cosine desc, id asc)."""
        friends = np.empty((self.cnet_m, max(int(K), 0)), np.int32)
        sims = np.empty((self.cnet_m, max(int(K), 0)), np.float64)
        self._call('yue_cnet_friends', K, friends, sims)
        return friends, sims

    # -- Song2vec ---------------------------------------------------------------------------
    def s2v_set_state(self, Bu, Bi):
        Bu, Bi = _in(Bu, np.float64), _in(Bi, np.float64)
        assert Bu.shape == (self.m,) and Bi.shape == (self.n,), 's2v_set_state: Bu [m], Bi [n]'
        self._call('yue_s2v_set_state', Bu, Bi)

    def s2v_get_state(self):
        Bu, Bi = np.empty(self.m, np.float64), np.empty(self.n, np.float64)
        self._call('yue_s2v_get_state', Bu, Bi)
        return Bu, Bi

    def s2v_set_steps(self, u, i, count):
        u, i, count = _in(u, np.int32), _in(i, np.int32), _in(count, np.int32)
        assert len(u) == len(i) == len(count), 's2v_set_steps: u, i and count must hold one entry per step'
        self._s2v_T = len(u)
        self._call('yue_s2v_set_steps', u, i, count, len(u))

    def s2v_set_pairs(self, t1, t2, sim):
        t1, t2, sim = _in(t1, np.int32), _in(t2, np.int32), _in(sim, np.float64)
        assert len(t1) == len(t2) == len(sim), 's2v_set_pairs: t1, t2 and sim must hold one entry per pair'
        self._s2v_P = len(t1)
        self._call('yue_s2v_set_pairs', t1, t2, sim, len(t1))

    def s2v_epoch(self, lr, regU, regI, regB, alpha, globalMean=0.0):
        """One iteration of Song2vec.py:163-189.  Returns the squared errors per step and per pair (float64)."""
        e1 = np.zeros(self._s2v_T, np.float64)
        e2 = np.zeros(self._s2v_P, np.float64)
        self._call('yue_s2v_epoch', lr, regU, regI, regB, alpha, globalMean, e1, e2)
        return e1, e2

    # -- LightGCN (U = P, V = Q of set_factors) -------------------------
    def lgcn_set_graph(self, m, n, u_ptr, u_items, u_w, i_ptr, i_users, i_w):
        """Both sides of the (user, item, weight) pair list, ids sorted and unique within a row; checked for symmetry."""
        u_ptr, i_ptr = _in(u_ptr, np.int64), _in(i_ptr, np.int64)
        assert len(u_ptr) == m + 1 and len(i_ptr) == n + 1, 'lgcn_set_graph: u_ptr [m + 1], i_ptr [n + 1]'
        assert len(u_items) == len(u_w) and len(i_users) == len(i_w), 'lgcn_set_graph: one weight per id'
        assert len(u_items) >= u_ptr[-1] and len(i_users) >= i_ptr[-1], 'lgcn_set_graph: ptr runs past the id lists'
        self._call('yue_lgcn_set_graph', m, n, u_ptr, _in(u_items, np.int32, True), _in(u_w, np.float32, True),
                   i_ptr, _in(i_users, np.int32, True), _in(i_w, np.float32, True))

    def lgcn_propagate(self, layers, raw=False):
        """F [m + n][k]; with raw also the unnormalised layers E_1 .. E_layers [layers][m + n][k]."""
        N = self.m + self.n
        F = np.empty((N, self.k), np.float32)
        E = np.empty((max(layers, 0), N, self.k), np.float32) if raw else None
        self._call('yue_lgcn_propagate', layers, E, F)
        return (E, F) if raw else F

    def lgcn_grad(self, layers, u, i, j, reg):
        """(loss, dLoss / dU, dLoss / dV) of one minibatch of triplets; nothing moves."""
        u, i, j = _triplets(u, i, j, 'lgcn_grad')
        loss = C.c_double()
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        self._call('yue_lgcn_grad', layers, u, i, j, len(u), reg, C.byref(loss), gU, gV)
        return loss.value, gU, gV

    def lgcn_step(self, layers, u, i, j, lr, reg, step):
        """One minibatch step: propagation, loss, backward pass, Adam on U and V.  Returns the loss."""
        u, i, j = _triplets(u, i, j, 'lgcn_step')
        return self._read('yue_lgcn_step', 1, layers, u, i, j, len(u), lr, reg, step)[0]

    # -- NGCF (U = P, V = Q of set_factors) ------------------------------
    def ngcf_set_graph(self, m, n, ptr, col, w):
        """The (m + n)-row graph as a general CSR: columns ascending and unique within a row."""
        ptr = _in(ptr, np.int64)
        assert len(ptr) == m + n + 1 and len(col) == len(w) and len(col) >= ptr[-1], 'ngcf_set_graph: ptr [m + n + 1], one weight per column'
        self._call('yue_ngcf_set_graph', m, n, ptr, _in(col, np.int32, True), _in(w, np.float32, True))

    def ngcf_set_weights(self, W):
        """W [layers][2][k][k]; the weights' Adam moments are cleared."""
        W = _in(W, np.float32)
        assert W.ndim == 4 and W.shape[1] == 2 and W.shape[2] == W.shape[3], 'ngcf_set_weights: W [layers][2][k][k]'
        self.ngcf_w_shape = W.shape
        self._call('yue_ngcf_set_weights', W.shape[0], W.shape[2], W)

    def ngcf_get_weights(self, moments=False):
        """W, or (W, mW, vW) with the weights' Adam moments."""
        out = [np.empty(self.ngcf_w_shape, np.float32) for _ in range(3 if moments else 1)]
        self._call('yue_ngcf_get_weights', *(out + [None] * (3 - len(out))))
        return tuple(out) if moments else out[0]

    def ngcf_propagate(self, layers, training=False, keep=1.0, seed=0, step=0, parts=False):
        """F [m + n][(layers + 1) k]; with parts (S, Z, D, F), the first three [layers][m + n][k]."""
        N = self.m + self.n
        F = np.empty((N, (max(layers, 0) + 1) * self.k), np.float32)
        P = [np.empty((max(layers, 0), N, self.k), np.float32) for _ in range(3)] if parts else [None] * 3
        self._call('yue_ngcf_propagate', layers, int(bool(training)), keep, seed, step, *P, F)
        return tuple(P) + (F,) if parts else F

    def ngcf_grad(self, layers, training, keep, seed, step, u, i, j, reg):
        """(loss, dLoss / dU, dLoss / dV, dLoss / dW) of one minibatch of triplets; nothing moves."""
        u, i, j = _triplets(u, i, j, 'ngcf_grad')
        loss = C.c_double()
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        gW = np.empty((max(layers, 0), 2, self.k, self.k), np.float32)
        self._call('yue_ngcf_grad', layers, int(bool(training)), keep, seed, step, u, i, j, len(u), reg, C.byref(loss), gU, gV, gW)
        return loss.value, gU, gV, gW

    def ngcf_step(self, layers, training, keep, seed, u, i, j, lr, reg, step):
        """One minibatch step: propagation, loss, backward pass, Adam on U, V and the weights.  Returns the loss."""
        u, i, j = _triplets(u, i, j, 'ngcf_step')
        return self._read('yue_ngcf_step', 1, layers, int(bool(training)), keep, seed, u, i, j, len(u), lr, reg, step)[0]

    # -- CDAE (a state of its own: U, W, W', b, b') ----------------------
    def cdae_set_data(self, m, n, ptr, items, counts):
        """The user CSR: items ascending and distinct within a user, with their event counts."""
        ptr = _in(ptr, np.int64)
        assert len(ptr) == m + 1 and len(items) == len(counts) and len(items) >= ptr[-1], 'cdae_set_data: ptr [m + 1], one count per item'
        self.cdae_nnz_ptr = ptr
        self._call('yue_cdae_set_data', m, n, ptr, _in(items, np.int32, True), _in(counts, np.int32, True))
        self.cdae_m, self.cdae_n = int(m), int(n)

    def cdae_set_params(self, U, W, Wd, b, bd):
        """U [m, h], encoder W [n, h], decoder Wd [h, n], b [h], bd [n]; the Adam moments are cleared."""
        arrs = [_in(x, np.float32) for x in (U, W, Wd, b, bd)]
        h = arrs[0].shape[1]
        assert [x.shape for x in arrs] == [(self.cdae_m, h), (self.cdae_n, h), (h, self.cdae_n), (h,), (self.cdae_n,)], \
            'cdae_set_params: U [m, h], W [n, h], Wd [h, n], b [h], bd [n] for the m, n of cdae_set_data'
        self._call('yue_cdae_set_params', h, *arrs)
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
            sets.append((C.POINTER(C.c_float) * 5)(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs]))    # (`out` holds the arrays)
        self._call('yue_cdae_get_params', *(sets + [None] * (3 - len(sets))))
        return out

    def _cdae_batch(self, users, sptr, sitems):
        """(users, B, sample_ptr, sample_items): the arguments every batch call begins with."""
        users, sptr = _in(users, np.int32), _in(sptr, np.int64)
        assert len(sptr) == len(users) + 1 and len(sitems) >= sptr[-1], 'cdae: sample_ptr [B + 1] over sample_items'
        return users, len(users), sptr, _in(sitems, np.int32, True)

    def cdae_forward(self, users, sptr, sitems, co, seed, step, reg):
        """(hid [B, h], kept flags per input entry, logits and y_pred per sampled entry, loss)."""
        batch = users, B, sptr, _ = self._cdae_batch(users, sptr, sitems)
        S = int(sptr[-1])
        ptr = self.cdae_nnz_ptr
        q_in = int(sum(ptr[u + 1] - ptr[u] for u in users if 0 <= u < self.cdae_m))
        hid = np.empty((B, self.cdae_h), np.float32)
        kept = np.empty(max(q_in, 1), np.int32)
        logit, ypred = np.empty(max(S, 1), np.float32), np.empty(max(S, 1), np.float32)
        loss, = self._read('yue_cdae_forward', 1, *batch, co, seed, step, reg, hid, kept, logit, ypred)
        return hid, kept[:q_in].astype(bool), logit[:S], ypred[:S], loss

    def cdae_grad(self, users, sptr, sitems, co, seed, step, reg):
        """(loss, {'U', 'W', 'Wd', 'b', 'bd'}: the dense gradients); nothing moves."""
        batch = self._cdae_batch(users, sptr, sitems)
        g = [np.empty(shape, np.float32) for shape in self._cdae_shapes()]
        loss = C.c_double()
        self._call('yue_cdae_grad', *batch, co, seed, step, reg, C.byref(loss), *g)
        return loss.value, dict(zip(('U', 'W', 'Wd', 'b', 'bd'), g))

    def cdae_step(self, users, sptr, sitems, co, seed, lr, reg, step):
        """One minibatch step.  Returns (loss, saturated): with saturated > 0 the loss is inf and nothing was updated."""
        loss = C.c_double()
        rc = self._status('yue_cdae_step', *self._cdae_batch(users, sptr, sitems), co, seed, lr, reg, step, C.byref(loss))
        if rc == ERR_SATURATED:
            return loss.value, self.get_option('cdae_last_saturated')
        self._chk(rc)
        return loss.value, 0

    def cdae_load_factors(self):
        """Fills the context's factor matrices on the device with [hid(u) | 1] and [Wd[:, i] | bd[i]] (k = h + 1) for the scan."""
        self._call('yue_cdae_load_factors')
        self.m, self.n, self.k = self.cdae_m, self.cdae_n, self.cdae_h + 1

    def cdae_times(self):
        """Device ns of the last call's (encode, decode, regroup, adam) phases."""
        ns = (C.c_int64 * 4)()
        self._call('yue_cdae_times', ns)
        return tuple(ns)

    # -- APR (U = P, V = Q of set_factors, the moments of adam_reset) -----
    def apr_reset(self):
        """Clears the adversarial perturbation."""
        self._call('yue_apr_reset')

    def apr_pre_step(self, u, i, j, lr, reg, step):
        """One phase-1 step (softplus loss, the user rows regularised twice, the negative rows not), Adam.  Returns total_loss."""
        u, i, j = _triplets(u, i, j, 'apr_pre_step')
        return self._read('yue_apr_pre_step', 1, u, i, j, len(u), lr, reg, step)[0]

    def apr_adv_step(self, u, i, j, lr, eps, regA, step):
        """One phase-2 step: the perturbation from the batch's normalised gradient, then Adam on loss_adv.  Returns loss_adv."""
        u, i, j = _triplets(u, i, j, 'apr_adv_step')
        return self._read('yue_apr_adv_step', 1, u, i, j, len(u), lr, eps, regA, step)[0]

    def apr_set_delta(self, users, rows_u, items, rows_v):
        """The perturbation's rows: ascending distinct ids with one row [k] each; every other row is 0."""
        users, items = _in(users, np.int32, True), _in(items, np.int32, True)
        rows_u, rows_v = _in(rows_u, np.float32).reshape(-1, self.k), _in(rows_v, np.float32).reshape(-1, self.k)
        nu, ni = len(rows_u), len(rows_v)
        assert nu <= len(users) and ni <= len(items), 'apr_set_delta: one id per row'
        self._call('yue_apr_set_delta', users, nu, rows_u if nu else None, items, ni, rows_v if ni else None)

    def apr_get_delta(self):
        """(dU [m, k], dV [n, k]): the perturbation, dense."""
        dU, dV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        self._call('yue_apr_get_delta', dU, dV)
        return dU, dV

    def apr_delta_update(self, u, i, j, eps, regA):
        """The first half of a phase-2 step: returns the raw gradients (gU [m, k], gV [n, k]) with respect to the standing
        perturbation and installs the new one."""
        u, i, j = _triplets(u, i, j, 'apr_delta_update')
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        self._call('yue_apr_delta_update', u, i, j, len(u), eps, regA, gU, gV)
        return gU, gV

    def apr_grad(self, adversarial, u, i, j, reg):
        """(loss, dLoss / dU, dLoss / dV) of the phase-1 loss (reg) or of loss_adv at the standing perturbation (reg = regA);
        nothing moves."""
        u, i, j = _triplets(u, i, j, 'apr_grad')
        loss = C.c_double()
        gU, gV = np.empty((self.m, self.k), np.float32), np.empty((self.n, self.k), np.float32)
        self._call('yue_apr_grad', 1 if adversarial else 0, u, i, j, len(u), reg, C.byref(loss), gU, gV)
        return loss.value, gU, gV

    def apr_times(self):
        """Device ns of the last call's (coefficient, parameter-row, perturbation-row, adam) phases."""
        ns = (C.c_int64 * 4)()
        self._call('yue_apr_times', ns)
        return tuple(ns)

    # -- multi-GPU ----------------------------------------------------------------------
    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._call('yue_comm_init', buf, rank, nranks)

    def allreduce_f64(self, vals):
        arr = (C.c_double * len(vals))(*vals)
        self._call('yue_allreduce_f64', arr, len(vals))
        return list(arr)

    def comm_stats(self):
        """Last bpr_epoch on a communicator: dict(allreduce_bytes, collectives, wait_ms, nranks, rccl_version)."""
        return dict(zip(('allreduce_bytes', 'collectives', 'wait_ms', 'nranks', 'rccl_version'), self._read('yue_get_comm_stats', 5)))
