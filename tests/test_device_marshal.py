"""CPU tests of the marshalling vocabulary behind carbonado_amd.device
(carbonado_amd/_marshal.py): what no GPU test can see when it goes wrong, a
column of the wrong length, a NULL pointer for an empty one, a bounds check
that wraps.  Only the two layout cases at the end call the built library."""
import ctypes

import numpy as np
import pytest

from carbonado_amd import _marshal as M


def test_empty_column_has_count_zero_and_a_pointer():
    (a,), (p,), n = M._cols("Q", [])
    assert n == 0 and a.size == 0
    assert ctypes.cast(p, ctypes.c_void_p).value   # not NULL: the library may form &p[0]


def test_mismatched_columns_are_refused():
    with pytest.raises(AssertionError):
        M._cols("QI", [1, 2, 3], [1, 2])


def test_fits_does_not_wrap():
    def fits(off, ln):
        return M._fits(np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint64), 100)
    assert fits([2**64 - 1], [2]) is False
    assert fits([96], [4]) is True
    assert fits([97], [4]) is False


def test_optional_column():
    assert M._opt(None, 3) == (None, None)
    a, p = M._opt([0, 5, 17], 3)
    assert a.dtype == np.uint32 and a.tolist() == [0, 5, 17] and p
    with pytest.raises(AssertionError):
        M._opt([0, 5], 3)


def test_gcm_keys_of_bytes_bytearray_and_numpy():
    keys, ivs = bytes(range(64)), bytes(range(100, 132))
    forms = [(keys, ivs), (bytearray(keys), bytearray(ivs)),
             (np.frombuffer(keys, dtype=np.uint8).reshape(2, 32), np.frombuffer(ivs, dtype=np.uint8).reshape(2, 16))]
    for k, v in forms:
        for count in (2, None):
            (kk, vv), (pk, pv), n = M._gcm_keys(k, v, count)
            assert n == 2 and kk.tobytes() == keys and vv.tobytes() == ivs
            assert ctypes.string_at(pk, 64) == keys and ctypes.string_at(pv, 32) == ivs
    for k, v, count in ((keys[:63], ivs, 2), (keys, ivs[:31], 2), (keys + b"\0", ivs, None), (keys, ivs + b"\0", None)):
        with pytest.raises(AssertionError):
            M._gcm_keys(k, v, count)


def test_read_layout_across_a_shard_boundary():
    from carbonado_amd import device as D
    assert D.read_layout([1024], [0], [0, 0], [1000, 5], [100, 0]) == ([0, 112], [100, 0], 112, 2)


def test_plain_read_layout_clips_at_the_plaintext():
    from carbonado_amd import device as D
    assert D.plain_read_layout([1024], [0], [0, 0], [3990, 0], [100, 3999]) == ([0, 16], [9, 3999], 4016, 5)
