"""The marshalling vocabulary of device.py: host sequences to arrays and
pointers, output arrays, the checks of device tensors, and the argument groups
that the extension headers share (stream set, request set, ragged triple, keys).

THE RULE: a pointer handed to the library is only as good as the array behind
it.  Every helper here returns the arrays beside their pointers; the caller
binds the whole return value to local names and keeps them until the library
call has returned.  Never take a pointer from a temporary
(`_cols(...)[1][0]` inside a call's argument list is a bug).
"""
from __future__ import annotations

import ctypes

import numpy as np

import torch

from . import _lib

# kinds of a host column, as struct spells them
_KIND = {"B": np.uint8, "I": np.uint32, "Q": np.uint64}
_PTR = {np.uint8: _lib.c_u8p, np.uint32: _lib.c_u32p, np.uint64: _lib.c_u64p, np.int32: ctypes.c_void_p}


# ---- host columns

def _arr(xs, dtype=np.uint64):
    """(array, its pointer, its length) of a host sequence or numpy array.  The
    pointer is never NULL: an empty column points at one spare entry, which
    the returned (empty) array keeps alive."""
    a = np.ascontiguousarray(xs, dtype=dtype).reshape(-1)
    keep = a if a.size else np.zeros(1, dtype=dtype)
    return keep[:a.size], keep.ctypes.data_as(_PTR[dtype]), int(a.size)


def _cols(kinds: str, *xs):
    """Several host columns of one length: kinds[i] in "BIQ" is the type of
    xs[i] (B, I, Q: uint8, uint32, uint64).  Returns (arrays, pointers, count) and asserts the equal lengths."""
    assert len(kinds) == len(xs)
    cols = [_arr(x, _KIND[k]) for k, x in zip(kinds, xs)]
    count = cols[0][2]
    assert all(c[2] == count for c in cols)
    return [c[0] for c in cols], [c[1] for c in cols], count


def _opt(xs, n: int, dtype=np.uint32):
    """An optional column of n entries: (None, None) for None, else (array, pointer)."""
    if xs is None:
        return None, None
    a, p, m = _arr(xs, dtype)
    assert m == n
    return a, p


def _out(n: int, dtype=np.uint64, width=None):
    """An output column the library fills: (array of n entries [x width], its
    pointer).  The array is a view of max(n, 1) zeroed entries, so it is what
    the caller returns (as it is, or .tolist())."""
    keep = np.zeros(max(n, 1) if width is None else (max(n, 1), width), dtype=dtype)
    return keep[:n], keep.ctypes.data_as(_PTR[dtype])


def _fits(off, length, numel: int) -> bool:
    """every range [off[r], off[r] + length[r]) lies inside a buffer of numel bytes"""
    o, m = off[:length.size], np.uint64(numel)
    return bool((o <= m).all() and (length <= m - np.minimum(o, m)).all())


# ---- device tensors

def _resident(*ts) -> None:
    """tensors of which a call asks no more than that they are on the device (a scratch)"""
    for t in ts:
        assert t.is_cuda


def _flat(*ts, one_dim=True) -> None:
    """flat byte buffers on the device"""
    for t in ts:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and (t.dim() == 1 or not one_dim)


def _words(n: int, *ts, size=4, contiguous=True) -> None:
    """per-request or per-stream words on the device: n entries of `size` bytes
    (size None: any)"""
    for t in ts:
        assert t.is_cuda and t.numel() >= n and (t.is_contiguous() or not contiguous)
        assert size is None or t.element_size() == size


def _hashes(hashes, n: int) -> None:
    assert hashes.is_cuda and hashes.is_contiguous() and hashes.numel() >= 32 * n


def _scratch(size: int, device=None) -> torch.Tensor:
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


# ---- the argument groups

def _stream_args(streams, in_off, in_len, hashes, padding, chunk_len, one_dim=True):
    """The stream set of the read headers: (ioff, ilen, pad, cl), their
    pointers, nstreams."""
    _flat(streams, one_dim=one_dim)
    cols, ptrs, nstreams = _cols("QQII", in_off, in_len, padding, chunk_len)
    _hashes(hashes, nstreams)
    assert _fits(cols[0], cols[1], streams.numel())
    return cols, ptrs, nstreams


def _request_args(req_stream, start, length, content_off, content, words, nstreams, want):
    """The request set of a read call: (rs, st, ln, coff, clen), their
    pointers, nreq; clen is the output column the call returns.  `words` are
    the status words; want(rs, st, ln) gives the content length per request
    (the layout's), and the content buffer is checked against it before the
    call where every stream index is valid (else: the call reports it)."""
    _flat(content)
    cols, ptrs, nreq = _cols("IQQQ", req_stream, start, length, content_off)
    rs, st, ln, coff = cols
    _words(nreq, *words)
    if nreq and int(rs.max()) < nstreams:
        assert _fits(coff, np.asarray(want(rs, st, ln), dtype=np.uint64), content.numel())
    clen, pclen = _out(nreq)
    return cols + [clen], ptrs + [pclen], nreq


def _ragged(inp, in_off, n, out, out_off, *more, kinds="", room=lambda ln, *more: ln):
    """The (in_off, n, out_off) triple of a ragged call, with further columns
    of the same length (`kinds` as _cols): arrays, pointers, count.  Object o
    is inp[in_off[o] : in_off[o] + n[o]]; out[out_off[o] :] must hold
    room(n, *more)[o] bytes (room None: only known after the call)."""
    cols, ptrs, count = _cols("QQQ" + kinds, in_off, n, out_off, *more)
    assert _fits(cols[0], cols[1], inp.numel())
    if room is not None:
        assert _fits(cols[2], room(cols[1], *cols[3:]), out.numel())
    return cols, ptrs, count


def _gcm_keys(keys, ivs, count=None):
    """keys (32 B each) and ivs (16 B each) as bytes, bytearray or numpy:
    (arrays, pointers, count), the count taken from keys where None."""
    k, v = (x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8) for x in (keys, ivs))
    if count is None:
        count = k.size // 32
    (kk, pk, nk), (vv, pv, nv) = _arr(k, np.uint8), _arr(v, np.uint8)
    assert nk == 32 * count and nv == 16 * count
    return (kk, vv), (pk, pv), count
