"""Device-resident batch API over torch tensors (the throughput path).

torch provides HBM allocations and the stream; every byte of work is done by
the HIP kernels behind the C-ABI batch entry points.  All functions enqueue
on torch's current stream and return without synchronising.
"""
from __future__ import annotations

import ctypes

import numpy as np

import torch

from . import _lib
from ._buf import check
from .constants import FEC_K, FEC_M


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def zfec_encode_batch(inp: torch.Tensor, n: int, out: torch.Tensor, k: int = FEC_K, m: int = FEC_M) -> None:
    """inp: uint8 [count, in_stride] (first n bytes of each row are data);
    out: uint8 [count, >= m*chunk_len]."""
    assert inp.dtype == torch.uint8 and out.dtype == torch.uint8 and inp.is_cuda and out.is_cuda
    assert inp.is_contiguous() and out.is_contiguous() and inp.shape[0] == out.shape[0]
    count = inp.shape[0]
    need = _lib.lib().chip_zfec_encoded_len(n, k, m)
    assert out.shape[1] >= need and inp.shape[1] >= n
    check(_lib.lib().chip_zfec_encode_batch_dev(k, m, _p(inp), inp.shape[1], n, count, _p(out), out.shape[1],
                                                _stream()))


def hbm_pattern_batch(inp: torch.Tensor, n: int, out: torch.Tensor, k: int = FEC_K, m: int = FEC_M) -> None:
    """Diagnostic: zfec_encode_batch's memory pattern (same loads, stores,
    grid and run queue) without the GF arithmetic — `out` receives the data
    shards and, per computed row q, their XOR with every byte XOR q; not
    parity (chip_hbm_pattern_batch_dev)."""
    assert inp.is_cuda and out.is_cuda and inp.is_contiguous() and out.is_contiguous()
    assert inp.shape[0] == out.shape[0] and inp.data_ptr() != out.data_ptr()
    need = _lib.lib().chip_zfec_encoded_len(n, k, m)
    assert out.shape[1] >= need and inp.shape[1] >= n
    check(_lib.lib().chip_hbm_pattern_batch_dev(k, m, _p(inp), inp.shape[1], n, inp.shape[0], _p(out),
                                                out.shape[1], _stream()))


def zfec_decode_batch(enc: torch.Tensor, chunk_len: int, indices, out: torch.Tensor,
                      k: int = FEC_K, m: int = FEC_M) -> None:
    """enc: uint8 [count, >= m*chunk_len] (shard i at i*chunk_len); `indices`
    lists the surviving shares; out: uint8 [count, >= k*chunk_len]."""
    assert enc.is_contiguous() and out.is_contiguous() and enc.shape[0] == out.shape[0]
    idx = list(indices)
    cidx = (ctypes.c_uint32 * len(idx))(*idx)
    check(_lib.lib().chip_zfec_decode_batch_dev(k, m, _p(enc), enc.shape[1], chunk_len, cidx, len(idx),
                                                enc.shape[0], _p(out), out.shape[1], _stream()))


_pools = {}


def batch_pool(device=None):
    """A torch MemPool whose segments come from chip_device_alloc (physically
    contiguous HBM where available), for multi-GiB batch buffers."""
    dev = torch.device(device or "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _pools:
        alloc = torch.cuda.memory.CUDAPluggableAllocator(str(_lib.LIB_PATH), "chip_torch_alloc", "chip_torch_free")
        with torch.cuda.device(idx):
            _pools[idx] = (alloc, torch.cuda.MemPool(alloc.allocator()))
    return _pools[idx][1]


def empty_batch(shape, device=None) -> torch.Tensor:
    """uint8 tensor for a batch buffer, allocated in batch_pool()."""
    dev = torch.device(device or "cuda")
    with torch.cuda.device(dev), torch.cuda.use_mem_pool(batch_pool(dev)):
        return torch.empty(shape, dtype=torch.uint8, device=dev)


def bao_scratch(n: int, count: int, device=None) -> torch.Tensor:
    size = _lib.lib().chip_bao_scratch_len(n, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def bao_encode_batch(inp: torch.Tensor, n: int, out: torch.Tensor | None, hashes: torch.Tensor,
                     scratch: torch.Tensor, out_offset: int = 0) -> None:
    """out: uint8 [count, >= out_offset + bao_len(n)] or None (hash only), each
    stream `out_offset` bytes into its row (8-B multiple; 56: every chunk and
    node on a 64-B boundary); hashes: uint8 [count, 32]."""
    assert inp.is_contiguous() and inp.shape[1] >= n  # the row stride is inp.shape[1]
    count = inp.shape[0]
    check(_lib.lib().chip_bao_encode_batch_dev(
        _p(inp), inp.shape[1], n, count,
        ctypes.c_void_p(out.data_ptr() + out_offset) if out is not None else ctypes.c_void_p(0),
        out.shape[1] if out is not None else 0, _p(hashes), _p(scratch), _stream()))


def encode_scratch(fmt: int, n: int, count: int, device=None) -> torch.Tensor:
    size = _lib.lib().chip_encode_scratch_len(fmt, n, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def encode_batch(fmt: int, inp: torch.Tensor, n: int, out: torch.Tensor, hashes: torch.Tensor,
                 scratch: torch.Tensor, out_offset: int = 0):
    """encode() of device-resident objects at a level without host stages
    (Bao and/or Zfec bits): inp uint8 [count, in_stride] (first n bytes of each
    row), out uint8 [count, >= out_offset + encoded length], hashes uint8
    [count, 32]; each encoding starts `out_offset` bytes into its row (56 with
    a 256-B multiple row: STREAM_OFFSET, the fast layout of Zfec|Bao streams,
    include/carbonado_hip.h).  Zfec|Bao runs fused (shards hashed on chip,
    written into their bao slots).  Returns (encoded length, EncodeInfoC)."""
    assert inp.is_cuda and out.is_cuda and inp.is_contiguous() and out.is_contiguous()
    assert inp.shape[0] == out.shape[0] == hashes.shape[0] and inp.shape[1] >= n
    olen = ctypes.c_uint64()
    info = _lib.EncodeInfoC()
    check(_lib.lib().chip_encode_batch_dev(fmt, _p(inp), inp.shape[1], n, inp.shape[0],
                                           ctypes.c_void_p(out.data_ptr() + out_offset), out.shape[1],
                                           ctypes.byref(olen), _p(hashes), ctypes.byref(info), _p(scratch),
                                           _stream()))
    assert out_offset + olen.value <= out.shape[1]
    return olen.value, info


# Where a Zfec|Bao stream starts in a row of 256-B multiple pitch for the fast
# layout: its 8-byte header fills the end of a 64-B segment, so every chunk and
# parent node after it starts on a 64-B boundary (include/carbonado_hip.h).
STREAM_OFFSET = 56


def decode_scratch(fmt: int, in_len: int, count: int, device=None) -> torch.Tensor:
    size = _lib.lib().chip_decode_scratch_len(fmt, in_len, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def decode_batch(fmt: int, enc: torch.Tensor, in_len: int, hashes: torch.Tensor, padding: int, out: torch.Tensor,
                 status: torch.Tensor, scratch: torch.Tensor, in_offset: int = 0) -> int:
    """decode() of device-resident encodings at a level without host stages:
    enc uint8 [count, in_stride] (in_len bytes of each row from in_offset:
    STREAM_OFFSET where encode_batch put them), hashes uint8 [count, 32], out
    uint8 [count, >= decoded length], status int32 [count] (0, or the
    chip_status of that object).  Returns the decoded length."""
    assert enc.is_cuda and out.is_cuda and enc.is_contiguous() and out.is_contiguous()
    assert enc.shape[0] == out.shape[0] == status.shape[0] and enc.shape[1] >= in_offset + in_len
    olen = ctypes.c_uint64()
    check(_lib.lib().chip_decode_batch_dev(fmt, ctypes.c_void_p(enc.data_ptr() + in_offset), enc.shape[1], in_len,
                                           enc.shape[0], _p(hashes), padding,
                                           _p(out), out.shape[1], ctypes.byref(olen), _p(status), _p(scratch),
                                           _stream()))
    return olen.value


def bao_decode_batch(enc: torch.Tensor, n: int, hashes: torch.Tensor, out: torch.Tensor,
                     status: torch.Tensor, scratch: torch.Tensor, in_offset: int = 0) -> None:
    """status: int32/uint32 [count]; 0 = verified, 5 = hash mismatch.  Each
    stream `in_offset` bytes into its row of enc (8-B multiple)."""
    count = enc.shape[0]
    check(_lib.lib().chip_bao_decode_batch_dev(ctypes.c_void_p(enc.data_ptr() + in_offset), enc.shape[1], n, count,
                                               _p(hashes), _p(out), out.shape[1], _p(status), _p(scratch),
                                               _stream()))


def scrub_scratch(length: int, count: int, device=None) -> torch.Tensor:
    size = _lib.lib().chip_scrub_scratch_len(length, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def scrub_batch(enc: torch.Tensor, length: int, hashes: torch.Tensor, padding: int, chunk_len: int,
                out: torch.Tensor, scratch: torch.Tensor, offset: int = 0) -> np.ndarray:
    """scrub() (decoding.rs:159-212) of device-resident Bao|Zfec streams
    enc uint8 [count, >= length] with one EncodeInfo; repaired streams go to
    the rows of `out`.  Returns the per-object statuses (int32 numpy):
    0 = repaired, CHIP_ERR_UNNECESSARY_SCRUB = intact, else scrub's error.
    A row of `out` is written only where the status is 0 (its repaired
    stream's hash matched); every other row is left untouched.  The streams
    sit `offset` bytes into their rows of enc and out (8-B multiple)."""
    assert enc.is_cuda and out.is_cuda and enc.is_contiguous() and out.is_contiguous()
    count = enc.shape[0]
    assert out.shape[0] == count and hashes.shape[0] == count
    status = np.zeros(count, dtype=np.int32)
    check(_lib.lib().chip_scrub_batch_dev(ctypes.c_void_p(enc.data_ptr() + offset), enc.shape[1], length, count,
                                          _p(hashes), padding, chunk_len, ctypes.c_void_p(out.data_ptr() + offset),
                                          out.shape[1], status.ctypes.data_as(ctypes.c_void_p), _p(scratch),
                                          _stream()))
    return status


def encode_host_batch(fmt: int, inp: torch.Tensor, n: int, out: torch.Tensor, hashes: torch.Tensor,
                      nslots: int = 3, slice_bytes: int = 256 << 20, pubkey: bytes = b"",
                      ephemeral_sk=None, nonce=None, host_threads: int = 0):
    """End-to-end encode() of `count` objects held in HOST memory (pinned
    tensors reach the full PCIe rate): inp uint8 [count, >= n], out uint8
    [count, >= chip_encode_max_len(n)], hashes uint8 [count, 32].  The
    Snappy/Ecies host stages of a slice run on `host_threads` threads while
    earlier slices are on the device.  `ephemeral_sk` [count, 32] / `nonce`
    [count, 16] (uint8 tensors or arrays) inject the ECIES randomness (tests).
    Synchronous.  Returns (encoded length per object, EncodeInfo per object)."""
    import numpy as np
    from .structs import EncodeInfo
    assert not inp.is_cuda and not out.is_cuda and not hashes.is_cuda
    assert inp.is_contiguous() and out.is_contiguous() and hashes.is_contiguous()
    count = inp.shape[0]
    olen = (ctypes.c_uint64 * max(count, 1))()
    info = (_lib.EncodeInfoC * max(count, 1))()
    keep = [np.ascontiguousarray(np.asarray(x, dtype=np.uint8)) if x is not None else None
            for x in (ephemeral_sk, nonce)]
    inj = None
    if any(k is not None for k in keep):
        inj = _lib.EciesInjectC(*[k.ctypes.data if k is not None else None for k in keep])
    pk = np.frombuffer(bytes(pubkey), dtype=np.uint8)
    check(_lib.lib().chip_encode_host_batch(fmt, pk.ctypes.data if pk.size else None, pk.size,
                                            ctypes.byref(inj) if inj is not None else None, _p(inp), n, count,
                                            inp.shape[1], _p(out), out.shape[1], olen, _p(hashes), info,
                                            nslots, slice_bytes, host_threads))
    # field tuples through numpy (one C-speed pass), then EncodeInfo(*t): half
    # the cost of from_c per object at 16384 objects
    rows = np.ctypeslib.as_array(info)[:count].tolist() if count else []
    return list(olen)[:count], [EncodeInfo(*r) for r in rows]


def decode_host_batch(fmt: int, enc: torch.Tensor, in_len, hashes: torch.Tensor, padding, out: torch.Tensor,
                      secret_key: bytes = b"", nslots: int = 3, slice_bytes: int = 256 << 20,
                      host_threads: int = 0, raise_first: bool = True):
    """End-to-end decode() of `count` encoded objects held in HOST memory:
    enc uint8 [count, >= max in_len], in_len / padding per object, hashes
    uint8 [count, 32], out uint8 [count, out_stride].  Synchronous.  Returns
    (decoded length per object, status per object); with raise_first the
    first failing object's status is raised as its CarbonadoError."""
    import numpy as np
    from .error import status_to_error
    assert not enc.is_cuda and not out.is_cuda and not hashes.is_cuda
    assert enc.is_contiguous() and out.is_contiguous() and hashes.is_contiguous()
    count = enc.shape[0]
    n = max(count, 1)
    lens = (ctypes.c_uint64 * n)(*[int(x) for x in in_len])
    pads = (ctypes.c_uint32 * n)(*[int(x) for x in padding])
    olen = (ctypes.c_uint64 * n)()
    st = (ctypes.c_int32 * n)()
    sk = np.frombuffer(bytes(secret_key), dtype=np.uint8)
    rc = _lib.lib().chip_decode_host_batch(fmt, sk.ctypes.data if sk.size else None, sk.size, _p(hashes), _p(enc),
                                           lens, count, enc.shape[1], pads, _p(out), out.shape[1], olen, st,
                                           nslots, slice_bytes, host_threads)
    statuses = [st[o] for o in range(count)]
    if rc and (raise_first or not any(statuses)):
        raise status_to_error(rc)
    return [olen[o] for o in range(count)], statuses


# ---- ragged batches (include/carbonado_hip_ext.h): objects of different
# lengths in one call; `inp` / `out` / `enc` are flat uint8 buffers and each
# object has its own offset and length (host sequences of ints)

# Everything below marshals through one vocabulary (_marshal.py).  Its rule:
# bind what a helper returns and keep it until the library call has returned;
# the arrays are what keeps the pointers valid.
from ._marshal import (_arr, _cols, _fits, _flat, _gcm_keys, _hashes, _opt, _out, _ragged,  # noqa: E402
                       _request_args, _resident, _scratch, _stream_args, _words)


def _encode_outputs(count: int):
    """(encoded lengths, their pointer, EncodeInfoC array) for an encode call to fill"""
    olen, polen = _out(count)
    return olen, polen, (_lib.EncodeInfoC * max(count, 1))()


def _encoded(olen, info, ooff, out):
    """what a ragged encode returns, once the encodings are known to lie inside out"""
    from .structs import EncodeInfo
    assert _fits(ooff, olen, out.numel())
    return olen.tolist(), [EncodeInfo.from_c(info[o]) for o in range(olen.size)]


def ragged_layout(fmt: int, sizes, align: int = 256, stream_offset: int = STREAM_OFFSET):
    """Where encode_ragged's caller should put each object in one output
    buffer (host only): rows rounded up to `align`, each encoding
    `stream_offset` bytes into its row.  Returns (out_off, out_len, total)."""
    n, pn, count = _arr(sizes)
    (off, poff), (ln, pln), total = _out(count), _out(count), ctypes.c_uint64()
    check(_lib.lib().chipx_ragged_layout(fmt, pn, count, align, stream_offset, poff, pln, ctypes.byref(total)))
    return off.tolist(), ln.tolist(), total.value


def ragged_scratch(fmt: int, lens, decode: bool = False, device=None) -> torch.Tensor:
    """Scratch of a ragged call over objects of these lengths (input lengths
    of encode_ragged, encoded lengths of decode_ragged)."""
    ln, pln, count = _arr(lens)
    return _scratch(_lib.lib().chipx_ragged_scratch_len(fmt, pln, count, int(decode)), device)


def encode_ragged(fmt: int, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off, hashes: torch.Tensor,
                  scratch: torch.Tensor):
    """encode() at Bao (4), Zfec (8) or both (12) of object o =
    inp[in_off[o] : in_off[o] + sizes[o]] into out[out_off[o] :] (offsets as
    ragged_layout gives them), its hash to hashes[o] (uint8 [count, 32]).
    Returns (encoded length per object, EncodeInfo per object)."""
    _flat(inp, out)
    _resident(scratch)
    (ioff, n, ooff), (pioff, pn, pooff), count = _ragged(inp, in_off, sizes, out, out_off, room=None)
    _hashes(hashes, count)
    olen, polen, info = _encode_outputs(count)
    check(_lib.lib().chipx_encode_ragged_dev(fmt, _p(inp), pioff, pn, count, _p(out), pooff, polen, _p(hashes), info,
                                             _p(scratch), _stream()))
    return _encoded(olen, info, ooff, out)


def decode_ragged(fmt: int, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, out: torch.Tensor,
                  out_off, status: torch.Tensor, scratch: torch.Tensor):
    """decode() of the encodings enc[in_off[o] : in_off[o] + in_len[o]] with
    hashes[o] and padding[o] into out[out_off[o] :]; status int32 / uint32
    [count] on the device (0, or 5 = that object's hash mismatch).  Returns
    the decoded length per object."""
    _flat(enc, out)
    _resident(scratch)
    (ioff, ilen, ooff, pad), (pioff, pilen, pooff, ppad), count = _ragged(enc, in_off, in_len, out, out_off, padding,
                                                                          kinds="I", room=None)
    _hashes(hashes, count)
    _words(count, status, size=None, contiguous=False)
    olen, polen = _out(count)
    check(_lib.lib().chipx_decode_ragged_dev(fmt, _p(enc), pioff, pilen, count, _p(hashes), ppad, _p(out), pooff, polen,
                                             _p(status), _p(scratch), _stream()))
    assert _fits(ooff, olen, out.numel())
    return olen.tolist()


# ---- slice audits (include/carbonado_hip_audit.h): extract_slice /
# verify_slice for a batch of requests over device-resident bao streams.
# `streams`, `proofs` and `content` are flat uint8 buffers; a request r is
# (req_stream[r], index[r], count[r]) in units of 1024 bytes, as
# decoding.verify_slice takes them

def _stream_content_lens(in_len):
    """Content bytes of bao streams of in_len bytes: x = len - 8 = n + 64 (N - 1)
    with N = ceil(n / 1024) chunks, so N - 1 = (x - 1) // 1088.  (A length no
    stream has gives some number here: the call itself reports it.)"""
    x = np.maximum(in_len, np.uint64(8)) - np.uint64(8)
    return x - np.uint64(64) * ((np.maximum(x, np.uint64(1)) - np.uint64(1)) // np.uint64(1088))


def _content_lens(ns, idx, cnt):
    """min(n, start + len) - start where start < n, else 0, per request (the
    content-buffer check made before a verify call; chipa_slice_layout's rule)"""
    N = np.maximum((ns + np.uint64(1023)) // np.uint64(1024), np.uint64(1))
    start = np.minimum(np.minimum(idx, N) * np.uint64(1024), ns)
    end = np.minimum(np.minimum(idx + cnt, N) * np.uint64(1024), ns)
    return np.where(end > start, end - start, np.uint64(0))


def slice_layout(content_lens, index, count, align: int = 16):
    """Sizes and places of every request's proof and content (host only):
    content_lens[r] = the content length of request r's stream.  Returns
    (proof_off, proof_len, content_off, content_len, proof_total,
    content_total): offsets into one proof and one content buffer, each range
    on a multiple of `align` (a multiple of 16)."""
    cols, (pn, pidx, pcnt), nreq = _cols("QQQ", content_lens, index, count)
    outs = [_out(nreq) for _ in range(4)]
    pt, ct = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().chipa_slice_layout(pn, pidx, pcnt, nreq, align, *[p for _, p in outs],
                                        ctypes.byref(pt), ctypes.byref(ct)))
    return (*[o.tolist() for o, _ in outs], pt.value, ct.value)


def audit_scratch(nstreams: int, nreq: int, device=None) -> torch.Tensor:
    """Scratch of an extract_slices / verify_slices / verify_slice_proofs call."""
    return _scratch(_lib.lib().chipa_audit_scratch_len(nstreams, nreq), device)


def extract_slices(streams: torch.Tensor, in_off, in_len, req_stream, index, count, proofs: torch.Tensor,
                   proof_off, proof_len, scratch: torch.Tensor) -> None:
    """extract_slice of every request: the proof of request r (what
    decoding.extract_slice(stream, index[r], count[r] * 1024) returns for stream
    req_stream[r] = streams[in_off[s] : in_off[s] + in_len[s]]) into
    proofs[proof_off[r] : proof_off[r] + proof_len[r]], the offsets and exact
    lengths as slice_layout gives them.  No hashing, no status.  The per-stream
    and per-request numbers are host sequences or numpy arrays."""
    _flat(streams, proofs)
    _resident(scratch)
    (ioff, ilen), (pioff, pilen), nstreams = _cols("QQ", in_off, in_len)
    (rs, idx, cnt, poff, plen), (prs, pidx, pcnt, ppoff, pplen), nreq = _cols("IQQQQ", req_stream, index, count,
                                                                              proof_off, proof_len)
    assert _fits(ioff, ilen, streams.numel()) and _fits(poff, plen, proofs.numel())
    assert scratch.numel() >= _lib.lib().chipa_audit_scratch_len(nstreams, nreq)
    check(_lib.lib().chipa_extract_slices_dev(_p(streams), pioff, pilen, nstreams, prs, pidx, pcnt, nreq, _p(proofs),
                                              ppoff, pplen, _p(scratch), _stream()))


def verify_slices(streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, req_stream, index, count,
                  content: torch.Tensor, content_off, status: torch.Tensor, scratch: torch.Tensor):
    """verify_slice of every request straight from the resident streams;
    hashes uint8 [nstreams, 32].  status int32 / uint32 [nreq] on the device:
    0, or 5 where a node on the request's walk (or the stream's header, or its
    hash) disagrees.  content[content_off[r] :] receives the request's content
    where the status is 0 and zeros otherwise (offsets as slice_layout gives
    them).  Returns the content length per request."""
    _flat(streams, content)
    _resident(scratch)
    (ioff, ilen), (pioff, pilen), nstreams = _cols("QQ", in_off, in_len)
    (rs, idx, cnt, coff), (prs, pidx, pcnt, pcoff), nreq = _cols("IQQQ", req_stream, index, count, content_off)
    _hashes(hashes, nstreams)
    _words(nreq, status, contiguous=False)
    assert _fits(ioff, ilen, streams.numel())
    assert scratch.numel() >= _lib.lib().chipa_audit_scratch_len(nstreams, nreq)
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        assert _fits(coff, _content_lens(_stream_content_lens(ilen)[rs], idx, cnt), content.numel())
    clen, pclen = _out(nreq)
    check(_lib.lib().chipa_verify_slices_dev(_p(streams), pioff, pilen, _p(hashes), nstreams, prs, pidx, pcnt, nreq,
                                             _p(content), pcoff, pclen, _p(status), _p(scratch), _stream()))
    return clen.tolist()


def verify_slice_proofs(proofs: torch.Tensor, proof_off, proof_len, content_lens, hashes: torch.Tensor, index, count,
                        content: torch.Tensor, content_off, status: torch.Tensor, scratch: torch.Tensor):
    """The auditor's side: verify_slice from extracted proofs alone.  Request
    r's proof is proofs[proof_off[r] : proof_off[r] + proof_len[r]],
    content_lens[r] the content length of the stream it came from, hashes
    uint8 [nreq, 32] that stream's hash (one per request).  status and content
    as verify_slices.  Returns the content length per request."""
    _flat(proofs, content)
    _resident(scratch)
    (poff, plen, n, idx, cnt, coff), (ppoff, pplen, pn, pidx, pcnt, pcoff), nreq = _cols(
        "QQQQQQ", proof_off, proof_len, content_lens, index, count, content_off)
    _hashes(hashes, nreq)
    _words(nreq, status, contiguous=False)
    assert _fits(poff, plen, proofs.numel())
    assert scratch.numel() >= _lib.lib().chipa_audit_scratch_len(nreq, nreq)
    assert _fits(coff, _content_lens(n, idx, cnt), content.numel())  # before the call
    clen, pclen = _out(nreq)
    check(_lib.lib().chipa_verify_proofs_dev(_p(proofs), ppoff, pplen, pn, _p(hashes), pidx, pcnt, nreq, _p(content),
                                             pcoff, pclen, _p(status), _p(scratch), _stream()))
    return clen.tolist()


# ---- ragged scrub (include/carbonado_hip_repair.h): shard verdicts and repair
# of device-resident Bao|Zfec streams of different lengths in one call.  `enc`
# and `out` are flat uint8 buffers; stream o is enc[in_off[o] : in_off[o] +
# in_len[o]] with its own padding[o] and chunk_len[o] (EncodeInfo's)

def scrub_ragged_scratch(in_len, nrepair=None, device=None) -> torch.Tensor:
    """Scratch of a scrub_ragged / shard_masks_ragged call over streams of
    these lengths that repairs any `nrepair` of them per pass (None: all of
    them, one pass; 1: the least a call accepts)."""
    ln, pl, count = _arr(in_len)
    size = _lib.lib().chipr_scrub_ragged_scratch_len(pl, count, count if nrepair is None else int(nrepair))
    return _scratch(size, device)


def shard_masks_ragged(enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, chunk_len,
                       scratch: torch.Tensor, masks: torch.Tensor | None = None) -> torch.Tensor:
    """The authentic zfec shards of every stream (decoding.rs:172-183): returns
    masks int32 [count] on the device, bit i set when shard i of stream o
    verifies against hashes[o] (uint8 [count, 32]); 255 = intact, 0 also for a
    damaged header or a chunk_len that does not fit the stream.  Enqueued on
    the current stream, not synchronised."""
    _flat(enc)
    _resident(scratch)
    (ioff, ilen, cl), (pioff, pilen, pcl), count = _cols("QQI", in_off, in_len, chunk_len)
    _hashes(hashes, count)
    assert _fits(ioff, ilen, enc.numel())
    if masks is None:
        masks = torch.empty(count, dtype=torch.int32, device=enc.device)
    _words(count, masks)
    check(_lib.lib().chipr_shard_masks_ragged_dev(_p(enc), pioff, pilen, count, _p(hashes), pcl, _p(masks), _p(scratch),
                                                  scratch.numel(), _stream()))
    return masks


def scrub_ragged(enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len, out: torch.Tensor,
                 out_off, scratch: torch.Tensor) -> np.ndarray:
    """scrub() (decoding.rs:151-212) of device-resident Bao|Zfec streams of
    different lengths in one call: stream o = enc[in_off[o] : in_off[o] +
    in_len[o]] with hashes[o] (uint8 [count, 32]), padding[o] and chunk_len[o];
    a repaired stream goes to out[out_off[o] : out_off[o] + in_len[o]].
    Returns the per-object statuses (int32 numpy), what scrub_batch gives for
    that stream alone: 0 = repaired, CHIP_ERR_UNNECESSARY_SCRUB = intact, else
    scrub's error (a chunk_len that does not fit its stream is that object's
    ZfecError, not the call's).  An output range is written only where the
    status is 0 (its repaired stream's hash matched), and then completely;
    nothing else of `out` is touched.  `out` may be `enc` with out_off[o] ==
    in_off[o]: the stream is repaired where it lies.  The repairs run in as
    many passes as `scratch` requires (scrub_ragged_scratch); the results do
    not depend on it.  Synchronous."""
    _flat(enc, out)
    _resident(scratch)
    (ioff, ilen, ooff, pad, cl), (pioff, pilen, pooff, ppad, pcl), count = _ragged(
        enc, in_off, in_len, out, out_off, padding, chunk_len, kinds="II")
    _hashes(hashes, count)
    status, pstatus = _out(count, np.int32)
    check(_lib.lib().chipr_scrub_ragged_dev(_p(enc), pioff, pilen, count, _p(hashes), ppad, pcl, _p(out), pooff,
                                            pstatus, _p(scratch), scratch.numel(), _stream()))
    return status


# ---- ranged reads (include/carbonado_hip_read.h): byte ranges of resident
# Zfec|Bao objects, rebuilt from other shards where the primary's chunks are
# damaged.  A request r is (req_stream[r], start[r], len[r]) in object bytes

def _read_layout(layout, chunk_len, padding, req_stream, start, length, align):
    """read_layout and plain_read_layout: `layout` is the header's call"""
    (cl, pad), (pcl, ppad), nstreams = _cols("II", chunk_len, padding)
    (rs, st, ln), (prs, pst, pln), nreq = _cols("IQQ", req_stream, start, length)
    (off, poff), (clen, pclen) = _out(nreq), _out(nreq)
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    check(layout(pcl, ppad, nstreams, prs, pst, pln, nreq, align, poff, pclen, ctypes.byref(total), ctypes.byref(nseg)))
    return off.tolist(), clen.tolist(), total.value, nseg.value


def read_layout(chunk_len, padding, req_stream, start, length, align: int = 16):
    """Where read_ranges' caller should put every request's content (host
    only).  Returns (content_off, content_len, content_total, nseg): offsets
    into one content buffer, each range on a multiple of `align` (a multiple of
    16), and the segments of the call for read_scratch."""
    return _read_layout(lambda *args: _lib.lib().chipd_read_layout(*args), chunk_len, padding, req_stream, start, length,
                        align)


def read_scratch(nreq: int, nseg: int, device=None) -> torch.Tensor:
    """Scratch of a read_ranges call of nreq requests in nseg segments (read_layout)."""
    return _scratch(_lib.lib().chipd_read_scratch_len(nreq, nseg), device)


def read_ranges(streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len, req_stream, start,
                length, content: torch.Tensor, content_off, status: torch.Tensor, used: torch.Tensor,
                scratch: torch.Tensor):
    """Object bytes [start[r], start[r] + length[r]) of stream req_stream[r] =
    streams[in_off[s] : in_off[s] + in_len[s]] (hashes uint8 [nstreams, 32],
    padding[s] and chunk_len[s] its EncodeInfo's) into content[content_off[r] :]
    (offsets as read_layout gives them).  A range whose primary chunks verify
    is copied; one whose chunks are damaged is rebuilt from the first four
    shards whose chunks at the same place verify.  status int32 / uint32 [nreq]
    on the device: 0, or 7 where fewer than four do (zeros are written);
    used [nreq]: the shards each request was served from (bit p alone: copied
    from primary p).  Enqueued on the current stream, not synchronised.
    Returns the content length per request."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len)
    _resident(scratch)
    (rs, st, ln, coff, clen), (prs, pst, pln, pcoff, pclen), nreq = _request_args(
        req_stream, start, length, content_off, content, (status, used), nstreams,
        lambda *req: read_layout(cl, pad, *req)[1])
    check(_lib.lib().chipd_read_ranges_dev(_p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs, pst, pln,
                                           nreq, _p(content), pcoff, pclen, _p(status), _p(used), _p(scratch),
                                           scratch.numel(), _stream()))
    return clen.tolist()


# ---- vouched ranged reads (include/carbonado_hip_vread.h): read_ranges with
# every rebuilt chunk hashed against the CV the stream's tree stores for it

VOUCHED, UNVOUCHED, CONTRADICTED = 1, 2, 4  # bits of a request's vouch word
VREAD_STRICT = 1                            # flag: a request with an unvouched segment fails with 7


def vread_scratch(nreq: int, nseg: int, device=None) -> torch.Tensor:
    """Scratch of a read_ranges_vouched call of nreq requests in nseg segments (read_layout)."""
    return _scratch(_lib.lib().chipv_read_scratch_len(nreq, nseg), device)


def read_ranges_vouched(streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len, req_stream,
                        start, length, content: torch.Tensor, content_off, status: torch.Tensor, used: torch.Tensor,
                        vouch: torch.Tensor, scratch: torch.Tensor, flags: int = 0):
    """read_ranges with the same arguments, layout (read_layout) and bytes,
    plus a check and its verdict: every chunk of a rebuilt range is rebuilt in
    full, hashed as that chunk of the stream and compared with the CV its
    parent stores for it.  vouch int32 / uint32 [nreq] on the device: the OR
    over the request's segments of VOUCHED (rebuilt, hashes agree), UNVOUCHED
    (rebuilt, but the path from the chunk's parent to the root is damaged too,
    so nothing can be compared: read_ranges' guarantee) and CONTRADICTED (the
    hashes differ).  status: 5 for a request with a contradicted segment
    (zeros are written), else 7 as read_ranges gives it, and with flags =
    VREAD_STRICT also for a request with an unvouched segment, else 0.  With
    status 0 and no UNVOUCHED bit every byte is hashed against the root.
    status, used and vouch are filled on the device; enqueued on the current
    stream, not synchronised.  Returns the content length per request."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len)
    _resident(scratch)
    (rs, st, ln, coff, clen), (prs, pst, pln, pcoff, pclen), nreq = _request_args(
        req_stream, start, length, content_off, content, (status, used, vouch), nstreams,
        lambda *req: read_layout(cl, pad, *req)[1])
    check(_lib.lib().chipv_read_ranges_dev(_p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs, pst, pln,
                                           nreq, _p(content), pcoff, pclen, _p(status), _p(used), _p(vouch), flags,
                                           _p(scratch), scratch.numel(), _stream()))
    return clen.tolist()


# ---- ranged reads planned on the device (include/carbonado_hip_qread.h): the
# requests are device tensors, a kernel plans them, nothing is uploaded per call

class StreamTable:
    """The resident description of a set of streams (stream_table): the device
    table and what the planned reads know of it on the host."""

    def __init__(self, table: torch.Tensor, info: "_lib.TableInfo"):
        self.table, self.info = table, info

    nstreams = property(lambda self: self.info.nstreams)
    max_chunks = property(lambda self: self.info.max_chunks)
    min_shard = property(lambda self: self.info.min_shard)


def stream_table(streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len) -> StreamTable:
    """Describe resident streams once (the stream arguments of read_ranges):
    one record per stream and the share-selection table, uploaded on the
    current stream.  The table serves every later read_ranges_planned call
    while the streams and hashes stay where they are; an in-place scrub does not
    invalidate it."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len)
    table = torch.empty(_lib.lib().chipq_stream_table_len(nstreams), dtype=torch.uint8, device=streams.device)
    info = _lib.TableInfo()
    check(_lib.lib().chipq_stream_table_dev(_p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, _p(table),
                                            table.numel(), ctypes.byref(info), _stream()))
    return StreamTable(table, info)


def planned_read_scratch(table: StreamTable, nreq: int, max_len: int, vouched: bool = False,
                         device=None) -> torch.Tensor:
    """Scratch of a read_ranges_planned (vouched: read_ranges_vouched_planned)
    call of capacity (nreq, max_len) over `table`."""
    size = _lib.lib().chipq_read_scratch_len(ctypes.byref(table.info), nreq, max_len, 1 if vouched else 0)
    if nreq and not size:
        raise ValueError("the call would refuse this capacity")
    return _scratch(size, device or table.table.device)


def _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len, words, scratch):
    nreq = req_stream.numel()
    assert start.numel() == length.numel() == content_len.numel() == nreq
    assert req_stream.element_size() == 4 and start.element_size() == length.element_size() == 8
    assert content_len.element_size() == 8 and content.dtype == torch.uint8 and content.dim() == 1
    for t in (req_stream, start, length, content, content_len, scratch, table.table):
        assert t.is_cuda and t.is_contiguous()
    _words(nreq, *words)
    assert nreq == 0 or content.numel() >= (nreq - 1) * content_stride + min(content_stride, (max_len + 15) // 16 * 16)
    return nreq


def read_ranges_planned(table: StreamTable, req_stream: torch.Tensor, start: torch.Tensor, length: torch.Tensor,
                        max_len: int, content: torch.Tensor, content_stride: int, content_len: torch.Tensor,
                        status: torch.Tensor, used: torch.Tensor, scratch: torch.Tensor) -> None:
    """read_ranges for requests that live on the device: req_stream (int32 /
    uint32), start and length (int64 / uint64) are device tensors of nreq
    entries, read by the GPU only; nreq and max_len are the capacity of the
    call (spare requests: length 0).  Request r's content goes to
    content[r * content_stride :], its length to content_len[r] (device int64 /
    uint64).  status: 1 for a request the device refuses (stream index, range
    above 2^53, content longer than max_len), else read_ranges' status, used
    word and bytes.  The host work is O(1) and nothing is uploaded: after one
    warm-up call the call can be captured into a graph and replayed with the
    request tensors rewritten in place.  Enqueued on the current stream."""
    nreq = _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len,
                         (status, used), scratch)
    check(_lib.lib().chipq_read_ranges_dev(_p(table.table), ctypes.byref(table.info), _p(req_stream), _p(start),
                                           _p(length), nreq, max_len, _p(content), content_stride, _p(content_len),
                                           _p(status), _p(used), _p(scratch), scratch.numel(), _stream()))


def read_ranges_vouched_planned(table: StreamTable, req_stream: torch.Tensor, start: torch.Tensor,
                                length: torch.Tensor, max_len: int, content: torch.Tensor, content_stride: int,
                                content_len: torch.Tensor, status: torch.Tensor, used: torch.Tensor,
                                vouch: torch.Tensor, scratch: torch.Tensor, flags: int = 0) -> None:
    """read_ranges_vouched for requests that live on the device: the arguments
    of read_ranges_planned, the vouch word per request and flags (0 or
    VREAD_STRICT) as there."""
    nreq = _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len,
                         (status, used, vouch), scratch)
    check(_lib.lib().chipq_read_ranges_vouched_dev(_p(table.table), ctypes.byref(table.info), _p(req_stream),
                                                   _p(start), _p(length), nreq, max_len, _p(content), content_stride,
                                                   _p(content_len), _p(status), _p(used), _p(vouch), flags,
                                                   _p(scratch), scratch.numel(), _stream()))


# ---- slice audits planned on the device (include/carbonado_hip_paudit.h): the
# requests (and, for the auditor, the proofs) are device tensors, a kernel plans
# them, nothing is uploaded per call.  The holder's calls take the StreamTable
# of stream_table, the auditor's a RootTable

NO_REQUEST = 0xFFFFFFFF  # req_stream of a spare slot (CHIPP_NO_REQUEST)


class RootTable:
    """The auditor's resident description of the streams it audits
    (root_table): the device table and what the planned check knows of it."""

    def __init__(self, table: torch.Tensor, info: "_lib.RootInfo"):
        self.table, self.info = table, info

    nroots = property(lambda self: self.info.nroots)
    max_chunks = property(lambda self: self.info.max_chunks)


def root_table(content_lens, hashes: torch.Tensor) -> RootTable:
    """Describe audited streams once: content_lens[s] content bytes (host) and
    hashes uint8 [nroots, 32] on the device, which must stay where they are.
    Uploaded on the current stream."""
    (n,), (pn,), nroots = _cols("Q", content_lens)
    _hashes(hashes, nroots)
    table = torch.empty(max(_lib.lib().chipp_root_table_len(nroots), 16), dtype=torch.uint8, device=hashes.device)
    info = _lib.RootInfo()
    check(_lib.lib().chipp_root_table_dev(pn, _p(hashes), nroots, _p(table), table.numel(), ctypes.byref(info),
                                          _stream()))
    return RootTable(table, info)


def proof_bound(max_chunks: int, max_count: int) -> int:
    """The most bytes a proof of max_count chunks of a stream of max_chunks chunks can have."""
    return _lib.lib().chipp_proof_bound(max_chunks, max_count)


def planned_audit_scratch(table, nreq: int, max_count: int, device=None) -> torch.Tensor:
    """Scratch of a verify_slices_planned / extract_slices_planned /
    verify_slice_proofs_planned call of capacity (nreq, max_count) over `table`
    (a StreamTable or a RootTable)."""
    size = _lib.lib().chipp_audit_scratch_len(table.max_chunks, nreq, max_count)
    if nreq and not size:
        raise ValueError("the call would refuse this capacity")
    return _scratch(size, device or table.table.device)


def _planned_audit_args(table, req_stream, index, count, slots, lens, status, scratch):
    """The checks of a planned audit's tensors; slots = [(buffer, stride, min bytes of a slot)]."""
    nreq = req_stream.numel()
    assert index.numel() == count.numel() == nreq
    assert req_stream.element_size() == 4 and index.element_size() == count.element_size() == 8
    for t in (req_stream, index, count, scratch, table.table, *lens):
        assert t.is_cuda and t.is_contiguous()
    for t in lens:
        assert t.numel() >= nreq and t.element_size() == 8
    _words(nreq, status)
    for buf, stride, least in slots:
        _flat(buf)
        assert nreq == 0 or buf.numel() >= (nreq - 1) * stride + min(stride, least)
    return nreq


def verify_slices_planned(table: StreamTable, req_stream: torch.Tensor, index: torch.Tensor, count: torch.Tensor,
                          max_count: int, content: torch.Tensor, content_stride: int, content_len: torch.Tensor,
                          status: torch.Tensor, scratch: torch.Tensor) -> None:
    """verify_slices for requests that live on the device: req_stream (int32 /
    uint32; NO_REQUEST: a spare slot), index and count (int64 / uint64) are
    device tensors of nreq entries, read by the GPU only; nreq and max_count
    (selected chunks per request) are the capacity of the call.  Request r's
    content goes to content[r * content_stride :], its length to content_len[r]
    (device int64 / uint64).  status: 1 for a request the device refuses
    (stream index, index or count above 2^53, more than max_count chunks), else
    verify_slices' status and bytes.  The host work is O(1) and nothing is
    uploaded: after one warm-up call the call can be captured into a graph and
    replayed with the request tensors rewritten in place.  Enqueued on the
    current stream."""
    nreq = _planned_audit_args(table, req_stream, index, count, [(content, content_stride, 1024 * max_count)],
                               [content_len], status, scratch)
    check(_lib.lib().chipp_verify_slices_dev(_p(table.table), ctypes.byref(table.info), _p(req_stream), _p(index),
                                             _p(count), nreq, max_count, _p(content), content_stride, _p(content_len),
                                             _p(status), _p(scratch), scratch.numel(), _stream()))


def extract_slices_planned(table: StreamTable, req_stream: torch.Tensor, index: torch.Tensor, count: torch.Tensor,
                           max_count: int, proofs: torch.Tensor, proof_stride: int, proof_len: torch.Tensor,
                           status: torch.Tensor, scratch: torch.Tensor) -> None:
    """extract_slices for requests that live on the device (as
    verify_slices_planned): request r's proof goes to proofs[r * proof_stride :],
    its exact length to proof_len[r]; proof_stride is at least
    proof_bound(table.max_chunks, max_count).  status: 0, or 1 for a request the
    device refuses."""
    nreq = _planned_audit_args(table, req_stream, index, count,
                               [(proofs, proof_stride, proof_bound(table.max_chunks, max_count))], [proof_len], status,
                               scratch)
    check(_lib.lib().chipp_extract_slices_dev(_p(table.table), ctypes.byref(table.info), _p(req_stream), _p(index),
                                              _p(count), nreq, max_count, _p(proofs), proof_stride, _p(proof_len),
                                              _p(status), _p(scratch), scratch.numel(), _stream()))


def verify_slice_proofs_planned(roots: RootTable, req_stream: torch.Tensor, index: torch.Tensor, count: torch.Tensor,
                                max_count: int, proofs: torch.Tensor, proof_stride: int, proof_len: torch.Tensor,
                                content: torch.Tensor, content_stride: int, content_len: torch.Tensor,
                                status: torch.Tensor, scratch: torch.Tensor) -> None:
    """The auditor's side for requests and proofs that live on the device:
    req_stream[r] names the audited stream of `roots` whose proof sits in
    proofs[r * proof_stride :], proof_len[r] (device, read) the bytes that
    arrived.  status: 6 where proof_len[r] is not the proof's exact length
    (content zeros), else as verify_slices_planned."""
    nreq = _planned_audit_args(roots, req_stream, index, count,
                               [(proofs, proof_stride, proof_bound(roots.max_chunks, max_count)),
                                (content, content_stride, 1024 * max_count)], [proof_len, content_len], status, scratch)
    check(_lib.lib().chipp_verify_proofs_dev(_p(roots.table), ctypes.byref(roots.info), _p(req_stream), _p(index),
                                             _p(count), nreq, max_count, _p(proofs), proof_stride, _p(proof_len),
                                             _p(content), content_stride, _p(content_len), _p(status), _p(scratch),
                                             scratch.numel(), _stream()))


# ---- AES-256-GCM over resident messages (include/carbonado_hip_ecies.h): the
# data half of the Ecies stage, one ragged batch per call

ECIES_FAILED = 17  # status of a message whose tag does not verify (CHIP_ERR_ECIES)


def gcm_scratch(n, device=None) -> torch.Tensor:
    """Scratch of a gcm_seal_ragged / gcm_open_ragged call over messages of n[o] bytes."""
    ln, pln, count = _arr(n)
    return _scratch(_lib.lib().chipe_gcm_scratch_len(pln, count), device)


def gcm_seal_ragged(keys, ivs, inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off, tags: torch.Tensor,
                    scratch: torch.Tensor) -> None:
    """AES-256-GCM (16-byte nonce, no AAD) of message o = inp[in_off[o] :
    in_off[o] + n[o]] (16-B aligned) under keys[32 o : 32 o + 32] and
    ivs[16 o : 16 o + 16] (host bytes): the ciphertext to out[out_off[o] :] at
    any byte offset, the tag to tags[16 o : 16 o + 16].  Bitsliced AES and a
    table-free GHASH on the device; the key region of the scratch is zeroed by
    the call's last operation.  Enqueued on the current stream, not
    synchronised."""
    _flat(inp, out, tags, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, n, out, out_off)
    assert tags.numel() >= 16 * count
    kv, (pk, pv), _ = _gcm_keys(keys, ivs, count)
    check(_lib.lib().chipe_gcm_seal_ragged_dev(pk, pv, _p(inp), pioff, pln, count, _p(out), pooff, _p(tags),
                                               _p(scratch), scratch.numel(), _stream()))


def gcm_open_ragged(keys, ivs, inp: torch.Tensor, in_off, n, tags: torch.Tensor, out: torch.Tensor, out_off,
                    status: torch.Tensor, scratch: torch.Tensor) -> None:
    """The reverse: ciphertext o = inp[in_off[o] : in_off[o] + n[o]] (any byte
    offset) with its tag tags[16 o : 16 o + 16]; the plaintext to
    out[out_off[o] :] (16-B aligned).  The tags are checked first; the CTR pass
    is gated on the verdicts on the device, so a message whose tag fails gets
    status[o] = ECIES_FAILED and zeros over its whole range, the others 0 and
    their plaintext.  status int32 / uint32 [count] on the device.  Enqueued on
    the current stream, not synchronised."""
    _flat(inp, out, tags, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, n, out, out_off)
    assert tags.numel() >= 16 * count
    _words(count, status)
    kv, (pk, pv), _ = _gcm_keys(keys, ivs, count)
    check(_lib.lib().chipe_gcm_open_ragged_dev(pk, pv, _p(inp), pioff, pln, count, _p(tags), _p(out), pooff,
                                               _p(status), _p(scratch), scratch.numel(), _stream()))


def ecies_seal_ragged(pubkey: bytes, inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off,
                      scratch: torch.Tensor, inject=None) -> None:
    """encoding::ecies of every object inp[in_off[o] : in_off[o] + n[o]]
    (16-B aligned) to the receiver `pubkey` (33 or 65 bytes): the envelope
    eph_pub65 || nonce16 || tag16 || ciphertext, n[o] + 97 bytes, to
    out[out_off[o] :].  The key agreement of every object runs on the host
    before anything is enqueued; the bytes are sealed on the device.  inject:
    None, or a list of (ephemeral_sk 32 B, nonce 16 B) per object for bit-exact
    tests.  scratch: gcm_scratch(n).  Enqueued on the current stream, not
    synchronised."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, n, out, out_off,
                                                           room=lambda ln: ln + np.uint64(97))
    assert scratch.numel() >= _lib.lib().chipe_gcm_scratch_len(pln, count)
    inj, keep = _inject_array(inject, count)
    check(_lib.lib().chipe_seal_ragged_dev(bytes(pubkey), len(pubkey), inj, _p(inp), pioff, pln, count, _p(out), pooff,
                                           _p(scratch), _stream()))


def ecies_open_ragged(secret_key: bytes, inp: torch.Tensor, in_off, in_len, out: torch.Tensor, out_off,
                      status: torch.Tensor, scratch: torch.Tensor):
    """decoding::ecies of every envelope inp[in_off[o] : in_off[o] + in_len[o]]
    (any byte offset): the plaintext, in_len[o] - 97 bytes, to out[out_off[o] :]
    (16-B aligned), status[o] = 0; or ECIES_FAILED and zeros for a tag that
    does not verify, an envelope shorter than 97 bytes or an ephemeral key that
    does not parse.  The call waits once, for the envelopes' header bytes (the
    keys depend on them); the rest is enqueued on the current stream.  scratch:
    gcm_scratch of the plaintext lengths.  Returns the plaintext length per
    object."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, in_len, out, out_off, room=_plain_lens)
    _words(count, status)
    pl, ppl, _ = _arr(_plain_lens(ln))
    assert scratch.numel() >= _lib.lib().chipe_gcm_scratch_len(ppl, count)
    olen, polen = _out(count)
    check(_lib.lib().chipe_open_ragged_dev(bytes(secret_key), len(secret_key), _p(inp), pioff, pln, count, _p(out),
                                           pooff, polen, _p(status), _p(scratch), _stream()))
    return olen.tolist()


def _plain_lens(ln):
    """plaintext bytes of envelopes of ln bytes (eph_pub65 || nonce16 || tag16 come off)"""
    return np.where(ln >= 97, ln - np.uint64(97), np.uint64(0)).astype(np.uint64)


def _inject_array(inject, count):
    if inject is None:
        return None, []
    assert len(inject) == count
    inj, keep = (_lib.EciesInjectC * max(count, 1))(), []
    for o, (sk, nonce) in enumerate(inject):
        bs, bn = ctypes.create_string_buffer(bytes(sk), 32), ctypes.create_string_buffer(bytes(nonce), 16)
        keep += [bs, bn]
        inj[o].ephemeral_sk, inj[o].nonce = ctypes.addressof(bs), ctypes.addressof(bn)
    return inj, keep


def ecies_ragged_scratch(fmt: int, lens, decode: bool = False, device=None) -> torch.Tensor:
    """Scratch of encode_ragged_ecies (object lengths) / decode_ragged_ecies (stream lengths)."""
    ln, pln, count = _arr(lens)
    fn = _lib.lib().chipe_decode_scratch_len if decode else _lib.lib().chipe_encode_scratch_len
    return _scratch(fn(fmt, pln, count), device)


def encode_ragged_ecies(fmt: int, pubkey: bytes, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off,
                        hashes: torch.Tensor, scratch: torch.Tensor, inject=None):
    """encode() at Ecies with Bao and / or Zfec (5, 9, 13) of resident objects
    in one call: sealed into envelopes in the scratch, then encoded as
    encode_ragged does at fmt & 12 (offsets: ragged_layout(fmt & 12, sizes +
    97)).  Stream bytes, hash and EncodeInfo are those of encode() at fmt.
    Returns (encoded length per object, EncodeInfo per object)."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, sizes, out, out_off, room=None)
    _hashes(hashes, count)
    assert scratch.numel() >= _lib.lib().chipe_encode_scratch_len(fmt, pln, count)
    inj, keep = _inject_array(inject, count)
    olen, polen, info = _encode_outputs(count)
    check(_lib.lib().chipe_encode_ragged_dev(fmt, bytes(pubkey), len(pubkey), inj, _p(inp), pioff, pln, count, _p(out),
                                             pooff, polen, _p(hashes), info, _p(scratch), _stream()))
    return _encoded(olen, info, ooff, out)


def decode_ragged_ecies(fmt: int, secret_key: bytes, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding,
                        out: torch.Tensor, out_off, status: torch.Tensor, scratch: torch.Tensor):
    """decode() at 5, 9 or 13 of resident streams in one call: decode_ragged at
    fmt & 12 into envelopes in the scratch, then ecies_open_ragged.  status[o]:
    0, the bao status of a damaged stream (not opened, zeros), or ECIES_FAILED.
    Returns the plaintext length per object."""
    _flat(enc, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff, pad), (pioff, pln, pooff, ppad), count = _ragged(enc, in_off, in_len, out, out_off, padding,
                                                                      kinds="I", room=None)
    _words(count, status)
    assert scratch.numel() >= _lib.lib().chipe_decode_scratch_len(fmt, pln, count)
    olen, polen = _out(count)
    check(_lib.lib().chipe_decode_ragged_dev(fmt, bytes(secret_key), len(secret_key), _p(enc), pioff, pln, count,
                                             _p(hashes) if hashes is not None else None, ppad, _p(out), pooff,
                                             polen, _p(status), _p(scratch), _stream()))
    assert _fits(ooff, olen, out.numel())
    return olen.tolist()


# ---- the Ecies key agreement on the device (include/carbonado_hip_agree.h):
# secp256k1 and HKDF-SHA256 kernels, and the envelope and one-call forms above
# with no host key agreement, no copy back and no wait

def agree_scratch(count: int, device=None) -> torch.Tensor:
    """Scratch of a seal_keys / open_keys call over count objects."""
    return _scratch(_lib.lib().chipy_keys_scratch_len(count), device)


def envelope_scratch(n, device=None) -> torch.Tensor:
    """Scratch of ecies_seal_ragged_dev_keys / ecies_open_ragged_dev_keys over plaintexts of n[o] bytes."""
    ln, pln, count = _arr(n)
    return _scratch(_lib.lib().chipy_envelope_scratch_len(pln, count), device)


def _pitched(buf: torch.Tensor, pitch: int, width: int, count: int) -> None:
    """count slots of `width` bytes at a pitch lie inside a flat device buffer"""
    _flat(buf)
    assert count == 0 or (pitch >= width and buf.numel() >= (count - 1) * pitch + width)


def seal_keys(pubkey: bytes, count: int, pub: torch.Tensor, pub_pitch: int, keys: torch.Tensor, key_pitch: int,
              scratch: torch.Tensor, eph_sk=None) -> None:
    """Per object o: the ephemeral public key k_o G (0x04 || x || y) to
    pub[o * pub_pitch :][:65] and the AES key HKDF(E65 || (k_o P)65) to
    keys[o * key_pitch :][:32], P the receiver `pubkey` (33 or 65 bytes).
    eph_sk: None (the library's RNG) or 32 * count host bytes.  The keys stay
    in `keys`: the caller wipes them.  Enqueued on the current stream, not
    synchronised."""
    _pitched(pub, pub_pitch, 65, count)
    _pitched(keys, key_pitch, 32, count)
    _resident(scratch)
    sk, psk, nsk = _arr(np.frombuffer(bytes(eph_sk or b""), dtype=np.uint8), np.uint8)
    assert eph_sk is None or nsk == 32 * count
    check(_lib.lib().chipy_seal_keys_dev(bytes(pubkey), len(pubkey),
                                         ctypes.cast(psk, ctypes.c_void_p) if eph_sk is not None else None, count,
                                         _p(pub), pub_pitch, _p(keys), key_pitch, _p(scratch), scratch.numel(),
                                         _stream()))


def open_keys(secret_key: bytes, eph: torch.Tensor, eph_pitch: int, count: int, keys: torch.Tensor, key_pitch: int,
              status: torch.Tensor, scratch: torch.Tensor) -> None:
    """Per object o: the AES key HKDF(R65 || (sk R)65) of the ephemeral key
    R = eph[o * eph_pitch :][:65] to keys[o * key_pitch :][:32], status[o] = 0;
    or ECIES_FAILED and a key of zeros for an R that does not parse.  The keys
    stay in `keys`: the caller wipes them.  Enqueued on the current stream, not
    synchronised."""
    _pitched(eph, eph_pitch, 65, count)
    _pitched(keys, key_pitch, 32, count)
    _resident(scratch)
    _words(count, status)
    check(_lib.lib().chipy_open_keys_dev(bytes(secret_key), len(secret_key), _p(eph), eph_pitch, count, _p(keys),
                                         key_pitch, _p(status), _p(scratch), scratch.numel(), _stream()))


def ecies_seal_ragged_dev_keys(pubkey: bytes, inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off,
                               scratch: torch.Tensor, inject=None) -> None:
    """ecies_seal_ragged with the key agreement on the device: the same
    envelopes for the same injected values, no host elliptic-curve work.
    scratch: envelope_scratch(n)."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, n, out, out_off,
                                                           room=lambda ln: ln + np.uint64(97))
    assert scratch.numel() >= _lib.lib().chipy_envelope_scratch_len(pln, count)
    inj, keep = _inject_array(inject, count)
    check(_lib.lib().chipy_seal_ragged_dev(bytes(pubkey), len(pubkey), inj, _p(inp), pioff, pln, count, _p(out), pooff,
                                           _p(scratch), _stream()))


def ecies_open_ragged_dev_keys(secret_key: bytes, inp: torch.Tensor, in_off, in_len, out: torch.Tensor, out_off,
                               status: torch.Tensor, scratch: torch.Tensor):
    """ecies_open_ragged with the key agreement on the device: no copy back
    and no wait.  scratch: envelope_scratch of the plaintext lengths.  Returns
    the plaintext length per object."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, in_len, out, out_off, room=_plain_lens)
    _words(count, status)
    pl, ppl, _ = _arr(_plain_lens(ln))
    assert scratch.numel() >= _lib.lib().chipy_envelope_scratch_len(ppl, count)
    olen, polen = _out(count)
    check(_lib.lib().chipy_open_ragged_dev(bytes(secret_key), len(secret_key), _p(inp), pioff, pln, count, _p(out),
                                           pooff, polen, _p(status), _p(scratch), _stream()))
    return olen.tolist()


def ecies_ragged_scratch_dev_keys(fmt: int, lens, decode: bool = False, device=None) -> torch.Tensor:
    """Scratch of encode_ragged_ecies_dev_keys (object lengths) / decode_ragged_ecies_dev_keys (stream lengths)."""
    ln, pln, count = _arr(lens)
    fn = _lib.lib().chipy_decode_scratch_len if decode else _lib.lib().chipy_encode_scratch_len
    return _scratch(fn(fmt, pln, count), device)


def encode_ragged_ecies_dev_keys(fmt: int, pubkey: bytes, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off,
                                 hashes: torch.Tensor, scratch: torch.Tensor, inject=None):
    """encode_ragged_ecies with the key agreement on the device.  Returns
    (encoded length per object, EncodeInfo per object)."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, sizes, out, out_off, room=None)
    _hashes(hashes, count)
    assert scratch.numel() >= _lib.lib().chipy_encode_scratch_len(fmt, pln, count)
    inj, keep = _inject_array(inject, count)
    olen, polen, info = _encode_outputs(count)
    check(_lib.lib().chipy_encode_ragged_dev(fmt, bytes(pubkey), len(pubkey), inj, _p(inp), pioff, pln, count, _p(out),
                                             pooff, polen, _p(hashes), info, _p(scratch), _stream()))
    return _encoded(olen, info, ooff, out)


def decode_ragged_ecies_dev_keys(fmt: int, secret_key: bytes, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor,
                                 padding, out: torch.Tensor, out_off, status: torch.Tensor, scratch: torch.Tensor):
    """decode_ragged_ecies with the key agreement on the device: the call no
    longer blocks.  Returns the plaintext length per object."""
    _flat(enc, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff, pad), (pioff, pln, pooff, ppad), count = _ragged(enc, in_off, in_len, out, out_off, padding,
                                                                      kinds="I", room=None)
    _words(count, status)
    assert scratch.numel() >= _lib.lib().chipy_decode_scratch_len(fmt, pln, count)
    olen, polen = _out(count)
    check(_lib.lib().chipy_decode_ragged_dev(fmt, bytes(secret_key), len(secret_key), _p(enc), pioff, pln, count,
                                             _p(hashes) if hashes is not None else None, ppad, _p(out), pooff,
                                             polen, _p(status), _p(scratch), _stream()))
    assert _fits(ooff, olen, out.numel())
    return olen.tolist()


# ---- plaintext ranged reads of level-13 streams (include/carbonado_hip_cread.h):
# the keystream over ranges, the keys of resident streams, the read

def ctr_scratch(nkeys: int, nitems: int, device=None) -> torch.Tensor:
    """Scratch of a ctr_ranges call over nitems items under nkeys keys."""
    return _scratch(_lib.lib().chipc_ctr_scratch_len(nkeys, nitems), device)


def ctr_ranges(keys, ivs, item_key, pos, n, buf: torch.Tensor, buf_off, scratch: torch.Tensor,
               gate: torch.Tensor | None = None) -> None:
    """Item i XORs buf[buf_off[i] : buf_off[i] + n[i]] (16-B aligned) in place
    with keystream bytes [pos[i], pos[i] + n[i]) of AES-256-GCM (16-byte nonce)
    under keys[32 k : 32 k + 32] and ivs[16 k : 16 k + 16], k = item_key[i]
    (host bytes).  The same call encrypts and decrypts.  gate: None, or int32 /
    uint32 [nitems] on the device: item i is skipped where gate[i] != 0.  The
    key region of the scratch is zeroed by the call's last operation.  Enqueued
    on the current stream, not synchronised."""
    _flat(buf, one_dim=False)
    _resident(scratch)
    (ik, ps, ln, off), (pik, pps, pln, poff), nitems = _cols("IQQQ", item_key, pos, n, buf_off)
    assert _fits(off, ln, buf.numel())
    kv, (pk, pv), nkeys = _gcm_keys(keys, ivs)
    if gate is not None:
        _words(nitems, gate)
    check(_lib.lib().chipc_ctr_ranges_dev(pk, pv, nkeys, pik, pps, pln, nitems, _p(buf), poff,
                                          _p(gate) if gate is not None else None, _p(scratch), scratch.numel(),
                                          _stream()))


def stream_keys_scratch(nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a stream_keys call over nstreams streams."""
    return _scratch(_lib.lib().chipc_stream_keys_scratch_len(nstreams), device)


def stream_keys(secret_key: bytes, streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len,
                scratch: torch.Tensor):
    """The AES key and nonce of every level-13 stream, from envelope bytes
    [0, 81) read by a strict vouched read (so only from bytes hashed against
    the root) and one key agreement per stream on the host.  The call waits
    once, for the header bytes.  Returns (keys uint8 [nstreams, 32], ivs uint8
    [nstreams, 16], key_status uint32 [nstreams]) as numpy arrays: status 0, 5
    or 7 for a header that cannot be served, ECIES_FAILED for an object shorter
    than 97 bytes or an ephemeral key that does not parse (key and nonce are
    zeros then).  The keys are the caller's to hold and wipe."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len)
    _resident(scratch)
    (keys, pkeys), (ivs, pivs) = _out(nstreams, np.uint8, 32), _out(nstreams, np.uint8, 16)
    status, pstatus = _out(nstreams, np.uint32)
    check(_lib.lib().chipc_stream_keys_dev(bytes(secret_key), len(secret_key), _p(streams), pioff, pilen, _p(hashes),
                                           ppad, pcl, nstreams, pkeys, pivs, pstatus, _p(scratch), scratch.numel(),
                                           _stream()))
    return keys, ivs, status


def plain_read_layout(chunk_len, padding, req_stream, start, length, align: int = 16):
    """read_layout for requests in plaintext bytes of level-13 streams: (content_off,
    content_len, content_total, nseg) of plaintext [start, min(P, start +
    length)), P = 4 chunk_len - padding - 97."""
    return _read_layout(lambda *args: _lib.lib().chipc_read_layout(*args), chunk_len, padding, req_stream, start, length,
                        align)


def plain_read_scratch(nreq: int, nseg: int, nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a read_plain_ranges call of nreq requests in nseg segments (plain_read_layout)."""
    return _scratch(_lib.lib().chipc_read_scratch_len(nreq, nseg, nstreams), device)


def read_plain_ranges(keys, ivs, key_status, streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding,
                      chunk_len, req_stream, start, length, content: torch.Tensor, content_off, status: torch.Tensor,
                      used: torch.Tensor, vouch: torch.Tensor, scratch: torch.Tensor, flags: int = 0):
    """Plaintext bytes [start[r], start[r] + length[r]) of level-13 stream
    req_stream[r] into content[content_off[r] :] (plain_read_layout), with keys,
    ivs and key_status as stream_keys gave them (key_status may be None): the
    vouched read of the envelope bytes behind the range, then the keystream
    taken off in place, gated on the read's status.  status, used and vouch as
    read_ranges_vouched fills them; a request whose stream has a non-zero
    key_status gets that status, zeros, used 0 and vouch 0.  The GCM tag is NOT
    checked: the ciphertext is vouched for by the root hash, and a wrong key
    gives status 0 and bytes that are not the plaintext.  Enqueued on the
    current stream, not synchronised.  Returns the content length per request."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len)
    _resident(scratch)
    (rs, st, ln, coff, clen), (prs, pst, pln, pcoff, pclen), nreq = _request_args(
        req_stream, start, length, content_off, content, (status, used, vouch), nstreams,
        lambda *req: plain_read_layout(cl, pad, *req)[1])
    kv, (pk, pv), _ = _gcm_keys(keys, ivs, nstreams)
    ks, pks = _opt(key_status, nstreams)
    check(_lib.lib().chipc_read_ranges_dev(pk, pv, pks, _p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs,
                                           pst, pln, nreq, _p(content), pcoff, pclen, _p(status), _p(used), _p(vouch),
                                           flags, _p(scratch), scratch.numel(), _stream()))
    return clen.tolist()


# ---- plaintext reads of level-13 streams planned on the device
# (include/carbonado_hip_kread.h): the keys are expanded once into a resident
# table, the requests are device tensors, nothing is uploaded per call

class KeyTable:
    """The resident keys of a set of level-13 streams (key_table): round keys,
    J0 and the key_status word of every stream, in device memory until
    wipe_key_table."""

    def __init__(self, table: torch.Tensor, nstreams: int):
        self.table, self.nstreams = table, nstreams


def key_table(keys, ivs, key_status, device=None) -> KeyTable:
    """Expand the keys of resident level-13 streams once (keys, ivs and
    key_status as stream_keys gave them; key_status may be None): one record of
    round keys and J0 per stream, zeros for a stream whose key_status is not 0.
    The raw keys are uploaded into a staging part of the table, which is zeros
    again once the enqueued work is done.  The round keys STAY on the device, in
    the returned table, until wipe_key_table.  Enqueued on the current stream."""
    kv, (pk, pv), nstreams = _gcm_keys(keys, ivs)
    ks, pks = _opt(key_status, nstreams)
    table = torch.empty(_lib.lib().chipk_key_table_len(nstreams), dtype=torch.uint8, device=device or "cuda")
    check(_lib.lib().chipk_key_table_dev(pk, pv, pks, nstreams, _p(table), table.numel(), _stream()))
    return KeyTable(table, nstreams)


def wipe_key_table(table: KeyTable) -> None:
    """Zeros over the whole key table, enqueued on the current stream behind the reads that use it."""
    check(_lib.lib().chipk_key_table_wipe_dev(_p(table.table), table.table.numel(), _stream()))


def planned_plain_read_scratch(table: StreamTable, nreq: int, max_len: int, device=None) -> torch.Tensor:
    """Scratch of a read_plain_ranges_planned call of capacity (nreq, max_len) over `table`."""
    size = _lib.lib().chipk_read_scratch_len(ctypes.byref(table.info), nreq, max_len)
    if nreq and not size:
        raise ValueError("the call would refuse this capacity")
    return _scratch(size, device or table.table.device)


def read_plain_ranges_planned(table: StreamTable, key_table: KeyTable, req_stream: torch.Tensor, start: torch.Tensor,
                              length: torch.Tensor, max_len: int, content: torch.Tensor, content_stride: int,
                              content_len: torch.Tensor, status: torch.Tensor, used: torch.Tensor, vouch: torch.Tensor,
                              scratch: torch.Tensor, flags: int = 0) -> None:
    """read_plain_ranges for requests that live on the device: the arguments of
    read_ranges_vouched_planned with requests in PLAINTEXT bytes of level-13
    streams, over the stream table and a key table of the same streams.
    status: 1 for a request the device refuses (as read_ranges_planned; a start
    above 2^53 - 97; a range that ends above 2^36 - 32), the stream's key_status
    where that is not 0 (zeros over the clipped range, used 0, vouch 0), else
    read_plain_ranges' status, words and bytes.  Kernel launches only: after one
    warm-up call the call can be captured into a graph and replayed with the
    request tensors rewritten in place.  Enqueued on the current stream."""
    nreq = _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len,
                         (status, used, vouch), scratch)
    assert key_table.table.is_cuda and key_table.table.is_contiguous() and key_table.nstreams == table.nstreams
    check(_lib.lib().chipk_read_ranges_dev(_p(table.table), ctypes.byref(table.info), _p(key_table.table),
                                           key_table.table.numel(), _p(req_stream), _p(start), _p(length), nreq,
                                           max_len, _p(content), content_stride, _p(content_len), _p(status),
                                           _p(used), _p(vouch), flags, _p(scratch), scratch.numel(), _stream()))


def key_table_from_streams(table: StreamTable, secret_key: bytes, scratch: torch.Tensor | None = None) -> KeyTable:
    """The key table of the resident level-13 streams `table` describes, made
    without the host seeing a header or a key: what stream_keys followed by
    key_table produce, byte for byte, from a strict vouched planned read of
    every envelope's first 81 bytes and the key agreement kernels
    (include/carbonado_hip_agree.h).  No copy back, no wait; the only upload is
    the secret.  Enqueued on the current stream; the scratch (made here unless
    given) must outlive the enqueued work."""
    need = _lib.lib().chipy_key_table_scratch_len(ctypes.byref(table.info))
    if table.nstreams and not need:
        raise ValueError("the call would refuse this table")
    if scratch is None:
        scratch = _scratch(need, table.table.device)
    _resident(scratch)
    kt = torch.empty(_lib.lib().chipk_key_table_len(table.nstreams), dtype=torch.uint8, device=table.table.device)
    check(_lib.lib().chipy_key_table_dev(_p(table.table), ctypes.byref(table.info), bytes(secret_key), len(secret_key),
                                         _p(kt), kt.numel(), _p(scratch), scratch.numel(), _stream()))
    return KeyTable(kt, table.nstreams)


# ---- snappy on the device (include/carbonado_hip_snap.h): the framing format
# of encoding::snap / decoding::snap over ragged batches, bit-exact with
# chip_snap_compress, and the one-call forms of formats 6, 7, 10, 11, 14, 15

SNAP_FAILED = 16        # status of a stream that is not a valid frame stream (CHIP_ERR_SNAP)
SNAP_TOO_SMALL = 2      # its content does not fit the capacity (CHIP_ERR_BUFFER_TOO_SMALL)
SNAP_TOO_MANY = 11      # more data chunks than the capacity's slots (CHIP_ERR_UNSUPPORTED_FORMAT)


def snap_max_len(n: int) -> int:
    return int(_lib.lib().chip_snap_max_len(int(n)))


def snap_scratch(n, out_cap=None, device=None) -> torch.Tensor:
    """Scratch of a snap_ragged call over objects of n[o] bytes, or (with
    out_cap) of an unsnap_ragged call over streams of n[o] bytes."""
    ln, pln, count = _arr(n)
    if out_cap is None:
        size = _lib.lib().chips_snap_scratch_len(pln, count)
    else:
        cap, pcap, _ = _arr(out_cap)
        size = _lib.lib().chips_unsnap_scratch_len(pln, pcap, count)
    return _scratch(size, device)


def snap_ragged(inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off, out_len: torch.Tensor,
                scratch: torch.Tensor) -> None:
    """encoding::snap of every object inp[in_off[o] : in_off[o] + n[o]] (16-B
    aligned): its frame stream, the bytes chip_snap_compress gives, to
    out[out_off[o] :] at any byte offset (capacity snap_max_len(n[o])), its
    length to out_len[o] (int64 [count] on the device).  Enqueued on the
    current stream, not synchronised."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(
        inp, in_off, n, out, out_off, room=lambda ln: np.array([snap_max_len(x) for x in ln], dtype=np.uint64))
    _words(count, out_len, size=8)
    check(_lib.lib().chips_snap_ragged_dev(_p(inp), pioff, pln, count, _p(out), pooff, _p(out_len), _p(scratch),
                                           scratch.numel(), _stream()))


def unsnap_ragged(inp: torch.Tensor, in_off, in_len, out: torch.Tensor, out_off, out_cap, out_len: torch.Tensor,
                  status: torch.Tensor, scratch: torch.Tensor) -> None:
    """decoding::snap of every frame stream inp[in_off[o] : in_off[o] +
    in_len[o]] (any byte offset) into out[out_off[o] :] (16-B aligned, capacity
    out_cap[o]); status[o] (int32 / uint32) and out_len[o] (int64) on the
    device are what chip_snap_decompress gives.  A stream that fails leaves no
    decompressed byte: untouched for a framing error or a small capacity, zeros
    for a block that does not decode or whose CRC disagrees.  Enqueued on the
    current stream, not synchronised."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff, cap), (pioff, pln, pooff, pcap), count = _ragged(inp, in_off, in_len, out, out_off, out_cap,
                                                                      kinds="Q", room=lambda ln, cap: cap)
    _words(count, out_len, size=8)
    _words(count, status)
    check(_lib.lib().chips_unsnap_ragged_dev(_p(inp), pioff, pln, count, _p(out), pooff, pcap, _p(out_len), _p(status),
                                             _p(scratch), scratch.numel(), _stream()))


def snap_encode_layout(fmt: int, sizes, align: int = 256, stream_offset: int = STREAM_OFFSET):
    """Where encode_ragged_snap's caller should put each object (host only):
    ragged_layout over the worst-case lengths, since the encoded length depends
    on the data.  Returns (out_off, out_cap, total)."""
    n, pn, count = _arr(sizes)
    (off, poff), (cap, pcap), total = _out(count), _out(count), ctypes.c_uint64()
    check(_lib.lib().chips_encode_layout(fmt, pn, count, align, stream_offset, poff, pcap, ctypes.byref(total)))
    return off.tolist(), cap.tolist(), total.value


def snap_ragged_scratch(fmt: int, lens, out_cap=None, device=None) -> torch.Tensor:
    """Scratch of encode_ragged_snap (object lengths) or, with out_cap, of
    decode_ragged_snap (stream lengths and output capacities)."""
    ln, pln, count = _arr(lens)
    if out_cap is None:
        size = _lib.lib().chips_encode_scratch_len(fmt, pln, count)
    else:
        cap, pcap, _ = _arr(out_cap)
        size = _lib.lib().chips_decode_scratch_len(fmt, pln, pcap, count)
    return _scratch(size, device)


def encode_ragged_snap(fmt: int, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off, hashes: torch.Tensor,
                       scratch: torch.Tensor, pubkey: bytes = None, inject=None):
    """encode() at a format with the Snappy bit and Bao and / or Zfec (6, 7,
    10, 11, 14, 15) of resident objects in one call: compressed into rows of
    the scratch, then (sealed and) encoded as encode_ragged does at fmt & 12.
    The call waits once, for the compressed lengths.  Offsets:
    snap_encode_layout(fmt, sizes).  Stream bytes, hash and EncodeInfo are
    those of encode() at fmt.  Returns (encoded length per object, EncodeInfo
    per object)."""
    _flat(inp, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff), (pioff, pln, pooff), count = _ragged(inp, in_off, sizes, out, out_off, room=None)
    _hashes(hashes, count)
    assert scratch.numel() >= _lib.lib().chips_encode_scratch_len(fmt, pln, count)
    inj, keep = _inject_array(inject, count)
    olen, polen, info = _encode_outputs(count)
    pk = bytes(pubkey) if pubkey is not None else None
    check(_lib.lib().chips_encode_ragged_dev(fmt, pk, len(pk) if pk else 0, inj, _p(inp), pioff, pln, count, _p(out),
                                             pooff, polen, _p(hashes), info, _p(scratch), _stream()))
    return _encoded(olen, info, ooff, out)


def decode_ragged_snap(fmt: int, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, out: torch.Tensor,
                       out_off, out_cap, out_len: torch.Tensor, status: torch.Tensor, scratch: torch.Tensor,
                       secret_key: bytes = None) -> None:
    """decode() at 6, 7, 10, 11, 14 or 15 of resident streams in one call:
    decode_ragged (or decode_ragged_ecies) into rows of the scratch, then
    unsnap_ragged into out[out_off[o] :] (capacity out_cap[o]).  status[o]: 0,
    the bao / ecies status of an object that failed there (not decompressed,
    nothing written), or a snappy status; out_len[o] (int64 on the device): the
    decoded length.  Without the Ecies bit nothing is waited for."""
    _flat(enc, out, one_dim=False)
    _resident(scratch)
    (ioff, ln, ooff, cap, pad), (pioff, pln, pooff, pcap, ppad), count = _ragged(
        enc, in_off, in_len, out, out_off, out_cap, padding, kinds="QI", room=lambda ln, cap, pad: cap)
    _words(count, status)
    _words(count, out_len, size=8)
    assert scratch.numel() >= _lib.lib().chips_decode_scratch_len(fmt, pln, pcap, count)
    sk = bytes(secret_key) if secret_key is not None else None
    check(_lib.lib().chips_decode_ragged_dev(fmt, sk, len(sk) if sk else 0, _p(enc), pioff, pln, count,
                                             _p(hashes) if hashes is not None else None, ppad, _p(out), pooff, pcap,
                                             _p(out_len), _p(status), _p(scratch), _stream()))


# ---- plaintext ranged reads of level-14 / level-15 streams
# (include/carbonado_hip_fread.h): the frame index of resident streams, its
# proof against the stream, the read

def _frame_keys(fmt, keys, ivs, key_status, nstreams):
    """(keep-alive, keys pointer, ivs pointer, key_status pointer): looked at for format 15 only"""
    if fmt != 15 or keys is None:
        return None, None, None, None
    kv, (pk, pv), _ = _gcm_keys(keys, ivs, nstreams)
    ks, pks = _opt(key_status, nstreams)
    return (kv, ks), pk, pv, pks


def _index_args(frame_off, idx_off, nframes, *more, kinds=""):
    """The index of every stream, frame_off[idx_off[s] : idx_off[s] + nframes[s]
    + 1], with further per-stream columns: (fo, (io, nf, ...)), their pointers
    alike, nstreams."""
    fo, pfo, nfo = _arr(frame_off)
    cols, ptrs, nstreams = _cols("QQ" + kinds, idx_off, nframes, *more)
    assert not nstreams or (nfo and _fits(cols[0], cols[1], nfo - 1))  # idx_off + nframes + 1 <= len(frame_off)
    return (fo, cols), (pfo, ptrs), nstreams


def frame_index_scratch(nstreams: int, nentries: int, device=None) -> torch.Tensor:
    """Scratch of a frame_index or verify_frame_index call over nstreams streams
    and nentries index entries in all (the capacities, or nframes + 1 each)."""
    return _scratch(_lib.lib().chipf_index_scratch_len(nstreams, nentries), device)


def frame_index(fmt: int, streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len, idx_off,
                idx_cap, scratch: torch.Tensor, keys=None, ivs=None, key_status=None):
    """The frame index of every resident level-14 / level-15 stream, built by a
    serial walk over the chunk headers of the primary copy (decrypted hop by hop
    at 15, with keys, ivs and key_status as stream_keys gave them) and proven by
    verify_frame_index's work.  Stream s may write idx_cap[s] entries from entry
    idx_off[s] of one offsets array.  The call waits twice.  Returns numpy
    arrays (frame_off, nframes, index_status, plain_len, index_vouch):
    index_status 0 for a proven index of nframes + 1 entries; 2 where idx_cap
    is below nframes + 1; 11 for a valid stream that is not canonical; 16, 5 or
    7 with a vouch bit for a stream whose header's primary copy is damaged
    (scrub_ragged, then call again)."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len, one_dim=False)
    _resident(scratch)
    (io, cap), (pio, pcap), nidx = _cols("QQ", idx_off, idx_cap)
    assert nidx == nstreams
    (frame_off, pfo), (nframes, pnf) = _out(int((io + cap).max()) if nstreams else 0), _out(nstreams)
    (status, pstatus), (vouch, pvouch) = _out(nstreams, np.uint32), _out(nstreams, np.uint32)
    plain, pplain = _out(nstreams)
    keep, pk, pv, pks = _frame_keys(fmt, keys, ivs, key_status, nstreams)
    check(_lib.lib().chipf_frame_index_dev(fmt, pk, pv, pks, _p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams,
                                           pfo, pio, pcap, pnf, pstatus, pplain, pvouch, _p(scratch), scratch.numel(),
                                           _stream()))
    return frame_off, nframes, status, plain, vouch


def verify_frame_index(fmt: int, streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len,
                       frame_off, idx_off, nframes, index_status: torch.Tensor, plain_len: torch.Tensor,
                       index_vouch: torch.Tensor, scratch: torch.Tensor, keys=None, ivs=None, key_status=None) -> None:
    """Proves the index frame_off[idx_off[s] : idx_off[s] + nframes[s] + 1] of
    every stream against the stream: a strict vouched read of the identifier and
    of every chunk header, the keystream over them at 15, the chain check.
    index_status (int32 / uint32), plain_len (int64) and index_vouch (int32 /
    uint32), one entry per stream on the device: 0 and the plaintext's length
    for an index whose every link holds; the read's 5 or 7; 16 for a wrong
    link; 11 for a chain that is not canonical.  Enqueued on the current stream,
    not synchronised."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len, one_dim=False)
    _resident(scratch)
    (fo, (io, nf)), (pfo, (pio, pnf)), nidx = _index_args(frame_off, idx_off, nframes)
    assert nidx == nstreams
    _words(nstreams, index_status, index_vouch)
    _words(nstreams, plain_len, size=8)
    keep, pk, pv, pks = _frame_keys(fmt, keys, ivs, key_status, nstreams)
    check(_lib.lib().chipf_verify_index_dev(fmt, pk, pv, pks, _p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams,
                                            pfo, pio, pnf, _p(index_status), _p(plain_len), _p(index_vouch),
                                            _p(scratch), scratch.numel(), _stream()))


def frame_read_layout(fmt: int, chunk_len, padding, frame_off, idx_off, nframes, plain_len, req_stream, start, length,
                      align: int = 16, index_status=None):
    """Where read_frame_ranges puts plaintext [start, min(plain_len, start +
    length)) of every request and what its scratch depends on (host only):
    (content_off, content_len, content_total, nseg, stage_total, vseg).
    index_status: as read_frame_ranges takes it."""
    (fo, (io, nf, pl, cl, pad)), (pfo, (pio, pnf, ppl, pcl, ppad)), nstreams = _index_args(
        frame_off, idx_off, nframes, plain_len, chunk_len, padding, kinds="QII")
    (rs, st, ln), (prs, pst, pln), nreq = _cols("IQQ", req_stream, start, length)
    ist, pis = _opt(index_status, nstreams)
    (off, poff), (clen, pclen) = _out(nreq), _out(nreq)
    total, nseg, stage, vseg = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().chipf_read_layout(fmt, pcl, ppad, pis, pfo, pio, pnf, ppl, nstreams, prs, pst, pln, nreq, align,
                                       poff, pclen, ctypes.byref(total), ctypes.byref(nseg), ctypes.byref(stage),
                                       ctypes.byref(vseg)))
    return off.tolist(), clen.tolist(), total.value, nseg.value, stage.value, vseg.value


def frame_read_scratch(nreq: int, nseg: int, stage_total: int, vseg: int, nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a read_frame_ranges call (the numbers of frame_read_layout)."""
    return _scratch(_lib.lib().chipf_read_scratch_len(nreq, nseg, stage_total, vseg, nstreams), device)


def read_frame_ranges(fmt: int, streams: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, chunk_len,
                      frame_off, idx_off, nframes, plain_len, req_stream, start, length, content: torch.Tensor,
                      content_off, status: torch.Tensor, used: torch.Tensor, vouch: torch.Tensor, scratch: torch.Tensor,
                      flags: int = 0, keys=None, ivs=None, index_status=None):
    """Plaintext bytes [start[r], start[r] + length[r]) of level-14 / level-15
    stream req_stream[r] into content[content_off[r] :] (any byte offset), with
    an index as frame_index or verify_frame_index proved it: the vouched read of
    the compressed frames behind the range, the keystream taken off them at 15,
    one block decode per frame with header and CRC checked, only the wanted
    bytes stored.  status: 0, the read's 5 or 7, 16 for a frame that does not
    agree with the index or its CRC (a wrong key at 15 among them), or the
    stream's index_status where that is non-zero; content is the exact plaintext
    for 0 and zeros otherwise.  used and vouch as read_ranges_vouched fills
    them.  The GCM tag is NOT checked.  Enqueued on the current stream, not
    synchronised.  Returns the content length per request."""
    (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams = _stream_args(streams, in_off, in_len, hashes, padding,
                                                                              chunk_len, one_dim=False)
    _resident(scratch)
    (fo, (io, nf, pl)), (pfo, (pio, pnf, ppl)), nidx = _index_args(frame_off, idx_off, nframes, plain_len, kinds="Q")
    assert nidx == nstreams
    (rs, st, ln, coff, clen), (prs, pst, pln, pcoff, pclen), nreq = _request_args(
        req_stream, start, length, content_off, content, (status, used, vouch), nstreams,
        lambda rs, st, ln: np.minimum(np.where(pl[rs] > st, pl[rs] - st, np.uint64(0)), ln))
    keep, pk, pv, _ = _frame_keys(fmt, keys, ivs, None, nstreams)
    ist, pis = _opt(index_status, nstreams)
    check(_lib.lib().chipf_read_ranges_dev(fmt, pk, pv, pis, pfo, pio, pnf, ppl, _p(streams), pioff, pilen, _p(hashes),
                                           ppad, pcl, nstreams, prs, pst, pln, nreq, _p(content), pcoff, pclen,
                                           _p(status), _p(used), _p(vouch), flags, _p(scratch), scratch.numel(),
                                           _stream()))
    return clen.tolist()


# ---- plaintext reads of level-14 / level-15 streams planned on the device
# (include/carbonado_hip_gread.h): the frame indexes are checked and uploaded
# once into a resident table, the requests are device tensors, nothing is
# uploaded per call

class FrameTable:
    """The resident frame indexes of a set of level-14 / level-15 streams
    (frame_table): the device table and what the planned reads know of it on
    the host."""

    def __init__(self, table: torch.Tensor, info: "_lib.FrameInfo"):
        self.table, self.info = table, info

    nstreams = property(lambda self: self.info.nstreams)
    nentries = property(lambda self: self.info.nentries)
    max_frame = property(lambda self: self.info.max_frame)
    format = property(lambda self: self.info.format)


def frame_table(fmt: int, chunk_len, padding, frame_off, idx_off, nframes, plain_len, index_status=None,
                device=None) -> FrameTable:
    """Describe the frame indexes of resident streams once (the index arguments
    of read_frame_ranges, as frame_index or verify_frame_index proved them):
    the checks read_frame_ranges makes on every call, one record per stream and
    the entries of the streams whose index_status is 0, uploaded on the current
    stream.  The table serves every later read_frame_ranges_planned call while
    the streams are not re-encoded."""
    (fo, (io, nf, pl, cl, pad)), (pfo, (pio, pnf, ppl, pcl, ppad)), nstreams = _index_args(
        frame_off, idx_off, nframes, plain_len, chunk_len, padding, kinds="QII")
    ist, pis = _opt(index_status, nstreams)
    size = _lib.lib().chipg_frame_table_len(nstreams, int(nf.sum()) + nstreams)
    if nstreams and not size:
        raise ValueError("too many streams or index entries for one frame table")
    table = torch.empty(size, dtype=torch.uint8, device=device or "cuda")
    info = _lib.FrameInfo()
    check(_lib.lib().chipg_frame_table_dev(fmt, pcl, ppad, pis, pfo, pio, pnf, ppl, nstreams, _p(table), table.numel(),
                                           ctypes.byref(info), _stream()))
    return FrameTable(table, info)


def planned_frame_read_scratch(table: StreamTable, frames: FrameTable, nreq: int, max_len: int,
                               device=None) -> torch.Tensor:
    """Scratch of a read_frame_ranges_planned call of capacity (nreq, max_len)
    over `table` and `frames`: the inner planned read's scratch and one staging
    slot per request for the compressed frames a range of max_len bytes can
    touch."""
    size = _lib.lib().chipg_read_scratch_len(ctypes.byref(table.info), ctypes.byref(frames.info), nreq, max_len)
    if nreq and not size:
        raise ValueError("the call would refuse this capacity")
    return _scratch(size, device or table.table.device)


def read_frame_ranges_planned(table: StreamTable, frames: FrameTable, key_table, req_stream: torch.Tensor,
                              start: torch.Tensor, length: torch.Tensor, max_len: int, content: torch.Tensor,
                              content_stride: int, content_len: torch.Tensor, status: torch.Tensor,
                              used: torch.Tensor, vouch: torch.Tensor, scratch: torch.Tensor, flags: int = 0) -> None:
    """read_frame_ranges for requests that live on the device: the arguments of
    read_ranges_vouched_planned with requests in PLAINTEXT bytes of level-14 /
    level-15 streams, over the stream table, the frame table and, at 15, a key
    table of the same streams (key_table: None at 14).  status: 1 for a request
    the device refuses (as read_ranges_planned; a frame record that contradicts
    the frame table's info), the stream's index_status or, at 15, key_status
    where that is not 0 (zeros over the clipped range, used 0, vouch 0), else
    read_frame_ranges' status, words and bytes.  Kernel launches only: after one
    warm-up call the call can be captured into a graph and replayed with the
    request tensors rewritten in place.  Enqueued on the current stream."""
    nreq = _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len,
                         (status, used, vouch), scratch)
    assert frames.table.is_cuda and frames.table.is_contiguous()
    ktab, klen = None, 0
    if frames.format == 15:
        assert key_table is not None and key_table.table.is_cuda and key_table.table.is_contiguous()
        assert key_table.nstreams == table.nstreams
        ktab, klen = _p(key_table.table), key_table.table.numel()
    check(_lib.lib().chipg_read_ranges_dev(_p(table.table), ctypes.byref(table.info), _p(frames.table),
                                           ctypes.byref(frames.info), ktab, klen, _p(req_stream), _p(start),
                                           _p(length), nreq, max_len, _p(content), content_stride, _p(content_len),
                                           _p(status), _p(used), _p(vouch), flags, _p(scratch), scratch.numel(),
                                           _stream()))


def host_topology() -> dict:
    """Where this process's host-copy path sits (chip_host_topology): the
    GPU's NUMA node, the calling thread's staging ring node and the copy
    workers' nodes (diagnostic)."""
    import json
    L = _lib.lib()
    n = ctypes.c_uint64(0)
    L.chip_host_topology(None, 0, ctypes.byref(n))
    buf = ctypes.create_string_buffer(max(1, n.value))
    check(L.chip_host_topology(buf, n.value, ctypes.byref(n)))
    return json.loads(buf.value.decode())
