"""The smallest pair list that tells a swapped bound or row count at a call site of yue_host::check_rows:
m = 5 users, n = 3 items (m != n), eight pairs; the user side holds the item n - 1 and the item side the user m - 1, each
at the end of a row, so that the valid upload proves `bound - 1` accepted and one step further is refused on that side only.
None of the refused inputs reaches a kernel: a refused upload launches nothing."""
import numpy as np
import pytest

M, N = 5, 3
U_PTR = np.array([0, 2, 3, 5, 6, 8], np.int64)
U_ITEMS = np.array([0, 2, 1, 0, 1, 2, 0, 2], np.int32)
I_PTR = np.array([0, 3, 5, 8], np.int64)
I_USERS = np.array([0, 2, 4, 1, 2, 0, 3, 4], np.int32)
NNZ = 8
BIG = 10 ** 6                                                     # where the falling pointer points: far past every id array


def lists():
    return {'u_ptr': U_PTR.copy(), 'u_items': U_ITEMS.copy(), 'i_ptr': I_PTR.copy(), 'i_users': I_USERS.copy()}


def not_the_transpose():
    """The item side with user 3 where user 2 stands in item 1's row: sorted, in range, eight pairs, and another pair list."""
    users = I_USERS.copy()
    assert users[4] == 2
    users[4] = 3
    return users


def faults(ptr, ids, bound, ordered):
    """(words, ptr, ids) of the refusals one list must give: an id one past its bound, an unsorted row where the order is
    asked for, the pointer {0, BIG, ...} that falls after its first row."""
    at = int(np.flatnonzero(ids == bound - 1)[0])
    bad = ids.copy(); bad[at] = bound
    yield 'out of range', ptr, bad
    if ordered:
        row = int(np.flatnonzero(np.diff(ptr) >= 2)[0])
        bad = ids.copy(); a = int(ptr[row]); bad[a], bad[a + 1] = bad[a + 1], bad[a]
        yield 'sorted and unique', ptr, bad
    down = ptr.copy(); down[1] = BIG
    assert down[2] < BIG and down[-1] == ptr[-1]
    yield 'non-decreasing', down, ids


def check_wiring(entry, upload, base, sides):
    """upload(**base) is the valid call of the entry point `entry`.  sides: (ptr key, ids key, bound, ordered) per list of the
    entry point.  Every fault of every side is refused with its words, the entry point's name and its error code, and the
    valid call is answered after each."""
    from yue_amd._shim import ERR_ARG, YueHipError
    upload(**base)
    for ptr_key, ids_key, bound, ordered in sides:
        assert base[ids_key].max() == bound - 1
        for words, ptr, ids in faults(base[ptr_key], base[ids_key], bound, ordered):
            with pytest.raises(YueHipError, match=words) as err:
                upload(**dict(base, **{ptr_key: ptr, ids_key: ids}))
            assert err.value.code == ERR_ARG and entry + ':' in str(err.value), (ptr_key, words, str(err.value))
            upload(**base)
