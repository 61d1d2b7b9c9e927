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

def _u64(xs):
    xs = [int(x) for x in xs]
    return (ctypes.c_uint64 * max(len(xs), 1))(*xs), len(xs)


def ragged_layout(fmt: int, sizes, align: int = 256, stream_offset: int = STREAM_OFFSET):
    """Where encode_ragged's caller should put each object in one output
    buffer (host only): rows rounded up to `align`, each encoding
    `stream_offset` bytes into its row.  Returns (out_off, out_len, total)."""
    n, count = _u64(sizes)
    off, ln, total = (ctypes.c_uint64 * max(count, 1))(), (ctypes.c_uint64 * max(count, 1))(), ctypes.c_uint64()
    check(_lib.lib().chipx_ragged_layout(fmt, n, count, align, stream_offset, off, ln, ctypes.byref(total)))
    return list(off)[:count], list(ln)[:count], total.value


def ragged_scratch(fmt: int, lens, decode: bool = False, device=None) -> torch.Tensor:
    """Scratch of a ragged call over objects of these lengths (input lengths
    of encode_ragged, encoded lengths of decode_ragged)."""
    ln, count = _u64(lens)
    size = _lib.lib().chipx_ragged_scratch_len(fmt, ln, count, int(decode))
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def encode_ragged(fmt: int, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off, hashes: torch.Tensor,
                  scratch: torch.Tensor):
    """encode() at Bao (4), Zfec (8) or both (12) of object o =
    inp[in_off[o] : in_off[o] + sizes[o]] into out[out_off[o] :] (offsets as
    ragged_layout gives them), its hash to hashes[o] (uint8 [count, 32]).
    Returns (encoded length per object, EncodeInfo per object)."""
    from .structs import EncodeInfo
    assert inp.is_cuda and out.is_cuda and hashes.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.dim() == out.dim() == 1
    assert inp.is_contiguous() and out.is_contiguous() and hashes.is_contiguous()
    ioff, count = _u64(in_off)
    n, _ = _u64(sizes)
    ooff, _ = _u64(out_off)
    assert len(sizes) == count == len(out_off) and hashes.numel() >= 32 * count
    assert all(int(a) + int(b) <= inp.numel() for a, b in zip(in_off, sizes))
    olen = (ctypes.c_uint64 * max(count, 1))()
    info = (_lib.EncodeInfoC * max(count, 1))()
    check(_lib.lib().chipx_encode_ragged_dev(fmt, _p(inp), ioff, n, count, _p(out), ooff, olen, _p(hashes), info,
                                             _p(scratch), _stream()))
    assert all(int(a) + b <= out.numel() for a, b in zip(out_off, list(olen)[:count]))
    return list(olen)[:count], [EncodeInfo.from_c(info[o]) for o in range(count)]


def decode_ragged(fmt: int, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, out: torch.Tensor,
                  out_off, status: torch.Tensor, scratch: torch.Tensor):
    """decode() of the encodings enc[in_off[o] : in_off[o] + in_len[o]] with
    hashes[o] and padding[o] into out[out_off[o] :]; status int32 / uint32
    [count] on the device (0, or 5 = that object's hash mismatch).  Returns
    the decoded length per object."""
    assert enc.is_cuda and out.is_cuda and hashes.is_cuda and status.is_cuda and scratch.is_cuda
    assert enc.dtype == out.dtype == torch.uint8 and enc.dim() == out.dim() == 1
    assert enc.is_contiguous() and out.is_contiguous() and hashes.is_contiguous()
    ioff, count = _u64(in_off)
    ilen, _ = _u64(in_len)
    ooff, _ = _u64(out_off)
    pads = (ctypes.c_uint32 * max(count, 1))(*[int(x) for x in padding])
    assert len(in_len) == count == len(out_off) == len(padding) and status.numel() >= count
    assert all(int(a) + int(b) <= enc.numel() for a, b in zip(in_off, in_len))
    olen = (ctypes.c_uint64 * max(count, 1))()
    check(_lib.lib().chipx_decode_ragged_dev(fmt, _p(enc), ioff, ilen, count, _p(hashes), pads, _p(out), ooff, olen,
                                             _p(status), _p(scratch), _stream()))
    assert all(int(a) + b <= out.numel() for a, b in zip(out_off, list(olen)[:count]))
    return list(olen)[:count]


# ---- slice audits (include/carbonado_hip_audit.h): extract_slice /
# verify_slice for a batch of requests over device-resident bao streams.
# `streams`, `proofs` and `content` are flat uint8 buffers; a request r is
# (req_stream[r], index[r], count[r]) in units of 1024 bytes, as
# decoding.verify_slice takes them

def _arr(xs, dtype=np.uint64):
    """(array, its pointer, its length) of a host sequence or numpy array; the
    array stays referenced by the caller for the duration of the call."""
    a = np.ascontiguousarray(xs, dtype=dtype).reshape(-1)
    keep = a if a.size else np.zeros(1, dtype=dtype)
    return keep, keep.ctypes.data_as(_lib.c_u64p if dtype == np.uint64 else _lib.c_u32p), int(a.size)


def _fits(off, length, numel: int) -> bool:
    """every range [off[r], off[r] + length[r]) lies inside a buffer of numel bytes"""
    o, m = off[:length.size], np.uint64(numel)
    return bool((o <= m).all() and (length <= m - np.minimum(o, m)).all())


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
    n, pn, nreq = _arr(content_lens)
    idx, pidx, ni = _arr(index)
    cnt, pcnt, nc = _arr(count)
    assert ni == nreq == nc
    outs = [np.zeros(max(nreq, 1), dtype=np.uint64) for _ in range(4)]
    pt, ct = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().chipa_slice_layout(pn, pidx, pcnt, nreq, align, *[o.ctypes.data_as(_lib.c_u64p) for o in outs],
                                        ctypes.byref(pt), ctypes.byref(ct)))
    return (*[o[:nreq].tolist() for o in outs], pt.value, ct.value)


def audit_scratch(nstreams: int, nreq: int, device=None) -> torch.Tensor:
    """Scratch of an extract_slices / verify_slices / verify_slice_proofs call."""
    size = _lib.lib().chipa_audit_scratch_len(nstreams, nreq)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def extract_slices(streams: torch.Tensor, in_off, in_len, req_stream, index, count, proofs: torch.Tensor,
                   proof_off, proof_len, scratch: torch.Tensor) -> None:
    """extract_slice of every request: the proof of request r (what
    decoding.extract_slice(stream, index[r], count[r] * 1024) returns for stream
    req_stream[r] = streams[in_off[s] : in_off[s] + in_len[s]]) into
    proofs[proof_off[r] : proof_off[r] + proof_len[r]], the offsets and exact
    lengths as slice_layout gives them.  No hashing, no status.  The per-stream
    and per-request numbers are host sequences or numpy arrays."""
    assert streams.is_cuda and proofs.is_cuda and scratch.is_cuda
    assert streams.dtype == proofs.dtype == torch.uint8 and streams.dim() == proofs.dim() == 1
    assert streams.is_contiguous() and proofs.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    idx, pidx, ni = _arr(index)
    cnt, pcnt, nc = _arr(count)
    poff, ppoff, npo = _arr(proof_off)
    plen, pplen, npl = _arr(proof_len)
    assert nl == nstreams and ni == nreq == nc == npo == npl
    assert _fits(ioff, ilen[:nstreams], streams.numel()) and _fits(poff, plen[:nreq], proofs.numel())
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
    assert streams.is_cuda and content.is_cuda and hashes.is_cuda and status.is_cuda and scratch.is_cuda
    assert streams.dtype == content.dtype == torch.uint8 and streams.dim() == content.dim() == 1
    assert streams.is_contiguous() and content.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    idx, pidx, ni = _arr(index)
    cnt, pcnt, nc = _arr(count)
    coff, pcoff, nco = _arr(content_off)
    assert nl == nstreams and ni == nreq == nc == nco
    assert hashes.numel() >= 32 * nstreams and status.numel() >= nreq and status.element_size() == 4
    assert _fits(ioff, ilen[:nstreams], streams.numel())
    assert scratch.numel() >= _lib.lib().chipa_audit_scratch_len(nstreams, nreq)
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        assert _fits(coff, _content_lens(_stream_content_lens(ilen)[rs[:nreq]], idx[:nreq], cnt[:nreq]), content.numel())
    check(_lib.lib().chipa_verify_slices_dev(_p(streams), pioff, pilen, _p(hashes), nstreams, prs, pidx, pcnt, nreq,
                                             _p(content), pcoff, clen.ctypes.data_as(_lib.c_u64p), _p(status),
                                             _p(scratch), _stream()))
    return clen[:nreq].tolist()


def verify_slice_proofs(proofs: torch.Tensor, proof_off, proof_len, content_lens, hashes: torch.Tensor, index, count,
                        content: torch.Tensor, content_off, status: torch.Tensor, scratch: torch.Tensor):
    """The auditor's side: verify_slice from extracted proofs alone.  Request
    r's proof is proofs[proof_off[r] : proof_off[r] + proof_len[r]],
    content_lens[r] the content length of the stream it came from, hashes
    uint8 [nreq, 32] that stream's hash (one per request).  status and content
    as verify_slices.  Returns the content length per request."""
    assert proofs.is_cuda and content.is_cuda and hashes.is_cuda and status.is_cuda and scratch.is_cuda
    assert proofs.dtype == content.dtype == torch.uint8 and proofs.dim() == content.dim() == 1
    assert proofs.is_contiguous() and content.is_contiguous() and hashes.is_contiguous()
    poff, ppoff, nreq = _arr(proof_off)
    plen, pplen, npl = _arr(proof_len)
    n, pn, nn = _arr(content_lens)
    idx, pidx, ni = _arr(index)
    cnt, pcnt, nc = _arr(count)
    coff, pcoff, nco = _arr(content_off)
    assert npl == nreq == nn == ni == nc == nco
    assert hashes.numel() >= 32 * nreq and status.numel() >= nreq and status.element_size() == 4
    assert _fits(poff, plen[:nreq], proofs.numel())
    assert scratch.numel() >= _lib.lib().chipa_audit_scratch_len(nreq, nreq)
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    assert _fits(coff, _content_lens(n[:nreq], idx[:nreq], cnt[:nreq]), content.numel())  # before the call
    check(_lib.lib().chipa_verify_proofs_dev(_p(proofs), ppoff, pplen, pn, _p(hashes), pidx, pcnt, nreq, _p(content),
                                             pcoff, clen.ctypes.data_as(_lib.c_u64p), _p(status), _p(scratch),
                                             _stream()))
    return clen[:nreq].tolist()


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
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def shard_masks_ragged(enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, chunk_len,
                       scratch: torch.Tensor, masks: torch.Tensor | None = None) -> torch.Tensor:
    """The authentic zfec shards of every stream (decoding.rs:172-183): returns
    masks int32 [count] on the device, bit i set when shard i of stream o
    verifies against hashes[o] (uint8 [count, 32]); 255 = intact, 0 also for a
    damaged header or a chunk_len that does not fit the stream.  Enqueued on
    the current stream, not synchronised."""
    assert enc.is_cuda and hashes.is_cuda and scratch.is_cuda
    assert enc.dtype == torch.uint8 and enc.dim() == 1 and enc.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    assert nl == count == ncl and hashes.numel() >= 32 * count
    assert _fits(ioff, ilen[:count], enc.numel())
    if masks is None:
        masks = torch.empty(count, dtype=torch.int32, device=enc.device)
    assert masks.is_cuda and masks.numel() >= count and masks.element_size() == 4 and masks.is_contiguous()
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
    assert enc.is_cuda and out.is_cuda and hashes.is_cuda and scratch.is_cuda
    assert enc.dtype == out.dtype == torch.uint8 and enc.dim() == out.dim() == 1
    assert enc.is_contiguous() and out.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    ooff, pooff, no = _arr(out_off)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    assert nl == count == no == npad == ncl and hashes.numel() >= 32 * count
    assert _fits(ioff, ilen[:count], enc.numel()) and _fits(ooff, ilen[:count], out.numel())
    status = np.zeros(max(count, 1), dtype=np.int32)
    check(_lib.lib().chipr_scrub_ragged_dev(_p(enc), pioff, pilen, count, _p(hashes), ppad, pcl, _p(out), pooff,
                                            status.ctypes.data_as(ctypes.c_void_p), _p(scratch), scratch.numel(),
                                            _stream()))
    return status[:count]


# ---- ranged reads (include/carbonado_hip_read.h): byte ranges of resident
# Zfec|Bao objects, rebuilt from other shards where the primary's chunks are
# damaged.  A request r is (req_stream[r], start[r], len[r]) in object bytes

def read_layout(chunk_len, padding, req_stream, start, length, align: int = 16):
    """Where read_ranges' caller should put every request's content (host
    only).  Returns (content_off, content_len, content_total, nseg): offsets
    into one content buffer, each range on a multiple of `align` (a multiple of
    16), and the segments of the call for read_scratch."""
    cl, pcl, nstreams = _arr(chunk_len, np.uint32)
    pad, ppad, npad = _arr(padding, np.uint32)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nl = _arr(length)
    assert npad == nstreams and ns == nreq == nl
    off, clen = np.zeros(max(nreq, 1), dtype=np.uint64), np.zeros(max(nreq, 1), dtype=np.uint64)
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().chipd_read_layout(pcl, ppad, nstreams, prs, pst, pln, nreq, align, off.ctypes.data_as(_lib.c_u64p),
                                       clen.ctypes.data_as(_lib.c_u64p), ctypes.byref(total), ctypes.byref(nseg)))
    return off[:nreq].tolist(), clen[:nreq].tolist(), total.value, nseg.value


def read_scratch(nreq: int, nseg: int, device=None) -> torch.Tensor:
    """Scratch of a read_ranges call of nreq requests in nseg segments (read_layout)."""
    size = _lib.lib().chipd_read_scratch_len(nreq, nseg)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
    assert streams.is_cuda and content.is_cuda and hashes.is_cuda and status.is_cuda and used.is_cuda and scratch.is_cuda
    assert streams.dtype == content.dtype == torch.uint8 and streams.dim() == content.dim() == 1
    assert streams.is_contiguous() and content.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nln = _arr(length)
    coff, pcoff, nco = _arr(content_off)
    assert nl == nstreams == npad == ncl and ns == nreq == nln == nco
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
    for t in (status, used):
        assert t.numel() >= nreq and t.element_size() == 4 and t.is_contiguous()
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        _, want, _, _ = read_layout(cl[:nstreams], pad[:nstreams], rs[:nreq], st[:nreq], ln[:nreq])
        assert _fits(coff, np.asarray(want, dtype=np.uint64), content.numel())
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    check(_lib.lib().chipd_read_ranges_dev(_p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs, pst, pln,
                                           nreq, _p(content), pcoff, clen.ctypes.data_as(_lib.c_u64p), _p(status),
                                           _p(used), _p(scratch), scratch.numel(), _stream()))
    return clen[:nreq].tolist()


# ---- vouched ranged reads (include/carbonado_hip_vread.h): read_ranges with
# every rebuilt chunk hashed against the CV the stream's tree stores for it

VOUCHED, UNVOUCHED, CONTRADICTED = 1, 2, 4  # bits of a request's vouch word
VREAD_STRICT = 1                            # flag: a request with an unvouched segment fails with 7


def vread_scratch(nreq: int, nseg: int, device=None) -> torch.Tensor:
    """Scratch of a read_ranges_vouched call of nreq requests in nseg segments (read_layout)."""
    size = _lib.lib().chipv_read_scratch_len(nreq, nseg)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
    assert streams.is_cuda and content.is_cuda and hashes.is_cuda and status.is_cuda and used.is_cuda and scratch.is_cuda
    assert vouch.is_cuda
    assert streams.dtype == content.dtype == torch.uint8 and streams.dim() == content.dim() == 1
    assert streams.is_contiguous() and content.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nln = _arr(length)
    coff, pcoff, nco = _arr(content_off)
    assert nl == nstreams == npad == ncl and ns == nreq == nln == nco
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
    for t in (status, used, vouch):
        assert t.numel() >= nreq and t.element_size() == 4 and t.is_contiguous()
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        _, want, _, _ = read_layout(cl[:nstreams], pad[:nstreams], rs[:nreq], st[:nreq], ln[:nreq])
        assert _fits(coff, np.asarray(want, dtype=np.uint64), content.numel())
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    check(_lib.lib().chipv_read_ranges_dev(_p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs, pst, pln,
                                           nreq, _p(content), pcoff, clen.ctypes.data_as(_lib.c_u64p), _p(status),
                                           _p(used), _p(vouch), flags, _p(scratch), scratch.numel(), _stream()))
    return clen[:nreq].tolist()


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
    assert streams.is_cuda and hashes.is_cuda and streams.dtype == torch.uint8 and streams.dim() == 1
    assert streams.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    assert nl == nstreams == npad == ncl
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
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
    return torch.empty(size, dtype=torch.uint8, device=device or table.table.device)


def _planned_args(table, req_stream, start, length, max_len, content, content_stride, content_len, words, scratch):
    nreq = req_stream.numel()
    assert start.numel() == length.numel() == content_len.numel() == nreq
    assert req_stream.element_size() == 4 and start.element_size() == length.element_size() == 8
    assert content_len.element_size() == 8 and content.dtype == torch.uint8 and content.dim() == 1
    for t in (req_stream, start, length, content, content_len, scratch, table.table) + tuple(words):
        assert t.is_cuda and t.is_contiguous()
    for t in words:
        assert t.numel() >= nreq and t.element_size() == 4
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


# ---- AES-256-GCM over resident messages (include/carbonado_hip_ecies.h): the
# data half of the Ecies stage, one ragged batch per call

ECIES_FAILED = 17  # status of a message whose tag does not verify (CHIP_ERR_ECIES)


def gcm_scratch(n, device=None) -> torch.Tensor:
    """Scratch of a gcm_seal_ragged / gcm_open_ragged call over messages of n[o] bytes."""
    ln, pln, count = _arr(n)
    size = _lib.lib().chipe_gcm_scratch_len(pln, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def _gcm_keys(keys, ivs, count):
    k = np.frombuffer(bytes(keys), dtype=np.uint8) if not isinstance(keys, np.ndarray) else keys
    v = np.frombuffer(bytes(ivs), dtype=np.uint8) if not isinstance(ivs, np.ndarray) else ivs
    k, v = np.ascontiguousarray(k, dtype=np.uint8).reshape(-1), np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)
    assert k.size == 32 * count and v.size == 16 * count
    keep_k = k if k.size else np.zeros(1, dtype=np.uint8)
    keep_v = v if v.size else np.zeros(1, dtype=np.uint8)
    return keep_k, keep_k.ctypes.data_as(_lib.c_u8p), keep_v, keep_v.ctypes.data_as(_lib.c_u8p)


def gcm_seal_ragged(keys, ivs, inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off, tags: torch.Tensor,
                    scratch: torch.Tensor) -> None:
    """AES-256-GCM (16-byte nonce, no AAD) of message o = inp[in_off[o] :
    in_off[o] + n[o]] (16-B aligned) under keys[32 o : 32 o + 32] and
    ivs[16 o : 16 o + 16] (host bytes): the ciphertext to out[out_off[o] :] at
    any byte offset, the tag to tags[16 o : 16 o + 16].  Bitsliced AES and a
    table-free GHASH on the device; the key region of the scratch is zeroed by
    the call's last operation.  Enqueued on the current stream, not
    synchronised."""
    assert inp.is_cuda and out.is_cuda and tags.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == tags.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(n)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and tags.numel() >= 16 * count and tags.is_contiguous()
    assert _fits(ioff, ln[:count], inp.numel()) and _fits(ooff, ln[:count], out.numel())
    kk, pk, vv, pv = _gcm_keys(keys, ivs, count)
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
    assert inp.is_cuda and out.is_cuda and tags.is_cuda and scratch.is_cuda and status.is_cuda
    assert inp.dtype == out.dtype == tags.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(n)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and tags.numel() >= 16 * count and tags.is_contiguous()
    assert status.numel() >= count and status.element_size() == 4 and status.is_contiguous()
    assert _fits(ioff, ln[:count], inp.numel()) and _fits(ooff, ln[:count], out.numel())
    kk, pk, vv, pv = _gcm_keys(keys, ivs, count)
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
    assert inp.is_cuda and out.is_cuda and scratch.is_cuda and inp.dtype == out.dtype == torch.uint8
    assert inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(n)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no
    assert _fits(ioff, ln[:count], inp.numel()) and _fits(ooff, ln[:count] + np.uint64(97), out.numel())
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
    assert inp.is_cuda and out.is_cuda and scratch.is_cuda and status.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(in_len)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and _fits(ioff, ln[:count], inp.numel())
    assert status.numel() >= count and status.element_size() == 4 and status.is_contiguous()
    plain = np.where(ln[:count] >= 97, ln[:count] - np.uint64(97), np.uint64(0)).astype(np.uint64)
    assert _fits(ooff, plain, out.numel())
    pl, ppl, _ = _arr(plain)
    assert scratch.numel() >= _lib.lib().chipe_gcm_scratch_len(ppl, count)
    olen = np.zeros(max(count, 1), dtype=np.uint64)
    check(_lib.lib().chipe_open_ragged_dev(bytes(secret_key), len(secret_key), _p(inp), pioff, pln, count, _p(out),
                                           pooff, olen.ctypes.data_as(_lib.c_u64p), _p(status), _p(scratch), _stream()))
    return olen[:count].tolist()


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
    return torch.empty(fn(fmt, pln, count), dtype=torch.uint8, device=device or "cuda")


def encode_ragged_ecies(fmt: int, pubkey: bytes, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off,
                        hashes: torch.Tensor, scratch: torch.Tensor, inject=None):
    """encode() at Ecies with Bao and / or Zfec (5, 9, 13) of resident objects
    in one call: sealed into envelopes in the scratch, then encoded as
    encode_ragged does at fmt & 12 (offsets: ragged_layout(fmt & 12, sizes +
    97)).  Stream bytes, hash and EncodeInfo are those of encode() at fmt.
    Returns (encoded length per object, EncodeInfo per object)."""
    from .structs import EncodeInfo
    assert inp.is_cuda and out.is_cuda and hashes.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(sizes)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and hashes.numel() >= 32 * count and hashes.is_contiguous()
    assert _fits(ioff, ln[:count], inp.numel())
    assert scratch.numel() >= _lib.lib().chipe_encode_scratch_len(fmt, pln, count)
    inj, keep = _inject_array(inject, count)
    olen = (ctypes.c_uint64 * max(count, 1))()
    info = (_lib.EncodeInfoC * max(count, 1))()
    check(_lib.lib().chipe_encode_ragged_dev(fmt, bytes(pubkey), len(pubkey), inj, _p(inp), pioff, pln, count, _p(out),
                                             pooff, olen, _p(hashes), info, _p(scratch), _stream()))
    assert all(int(a) + b <= out.numel() for a, b in zip(ooff[:count], list(olen)[:count]))
    return list(olen)[:count], [EncodeInfo.from_c(info[o]) for o in range(count)]


def decode_ragged_ecies(fmt: int, secret_key: bytes, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding,
                        out: torch.Tensor, out_off, status: torch.Tensor, scratch: torch.Tensor):
    """decode() at 5, 9 or 13 of resident streams in one call: decode_ragged at
    fmt & 12 into envelopes in the scratch, then ecies_open_ragged.  status[o]:
    0, the bao status of a damaged stream (not opened, zeros), or ECIES_FAILED.
    Returns the plaintext length per object."""
    assert enc.is_cuda and out.is_cuda and status.is_cuda and scratch.is_cuda
    assert enc.dtype == out.dtype == torch.uint8 and enc.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(in_len)
    ooff, pooff, no = _arr(out_off)
    pad, ppad, npad = _arr(padding, np.uint32)
    assert nl == count == no == npad and _fits(ioff, ln[:count], enc.numel())
    assert status.numel() >= count and status.element_size() == 4 and status.is_contiguous()
    assert scratch.numel() >= _lib.lib().chipe_decode_scratch_len(fmt, pln, count)
    olen = np.zeros(max(count, 1), dtype=np.uint64)
    check(_lib.lib().chipe_decode_ragged_dev(fmt, bytes(secret_key), len(secret_key), _p(enc), pioff, pln, count,
                                             _p(hashes) if hashes is not None else None, ppad, _p(out), pooff,
                                             olen.ctypes.data_as(_lib.c_u64p), _p(status), _p(scratch), _stream()))
    assert _fits(ooff, olen[:count], out.numel())
    return olen[:count].tolist()


# ---- plaintext ranged reads of level-13 streams (include/carbonado_hip_cread.h):
# the keystream over ranges, the keys of resident streams, the read

def ctr_scratch(nkeys: int, nitems: int, device=None) -> torch.Tensor:
    """Scratch of a ctr_ranges call over nitems items under nkeys keys."""
    size = _lib.lib().chipc_ctr_scratch_len(nkeys, nitems)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def ctr_ranges(keys, ivs, item_key, pos, n, buf: torch.Tensor, buf_off, scratch: torch.Tensor,
               gate: torch.Tensor | None = None) -> None:
    """Item i XORs buf[buf_off[i] : buf_off[i] + n[i]] (16-B aligned) in place
    with keystream bytes [pos[i], pos[i] + n[i]) of AES-256-GCM (16-byte nonce)
    under keys[32 k : 32 k + 32] and ivs[16 k : 16 k + 16], k = item_key[i]
    (host bytes).  The same call encrypts and decrypts.  gate: None, or int32 /
    uint32 [nitems] on the device: item i is skipped where gate[i] != 0.  The
    key region of the scratch is zeroed by the call's last operation.  Enqueued
    on the current stream, not synchronised."""
    assert buf.is_cuda and scratch.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()
    ik, pik, nitems = _arr(item_key, np.uint32)
    ps, pps, npos = _arr(pos)
    ln, pln, nl = _arr(n)
    off, poff, no = _arr(buf_off)
    assert npos == nitems == nl == no and _fits(off, ln[:nitems], buf.numel())
    nkeys = len(bytes(keys)) // 32 if not isinstance(keys, np.ndarray) else keys.size // 32
    kk, pk, vv, pv = _gcm_keys(keys, ivs, nkeys)
    if gate is not None:
        assert gate.is_cuda and gate.numel() >= nitems and gate.element_size() == 4 and gate.is_contiguous()
    check(_lib.lib().chipc_ctr_ranges_dev(pk, pv, nkeys, pik, pps, pln, nitems, _p(buf), poff,
                                          _p(gate) if gate is not None else None, _p(scratch), scratch.numel(),
                                          _stream()))


def stream_keys_scratch(nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a stream_keys call over nstreams streams."""
    size = _lib.lib().chipc_stream_keys_scratch_len(nstreams)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
    assert streams.is_cuda and hashes.is_cuda and scratch.is_cuda and streams.dtype == torch.uint8
    assert streams.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    assert nl == nstreams == npad == ncl
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
    keys = np.zeros((max(nstreams, 1), 32), dtype=np.uint8)
    ivs = np.zeros((max(nstreams, 1), 16), dtype=np.uint8)
    status = np.zeros(max(nstreams, 1), dtype=np.uint32)
    check(_lib.lib().chipc_stream_keys_dev(bytes(secret_key), len(secret_key), _p(streams), pioff, pilen, _p(hashes),
                                           ppad, pcl, nstreams, keys.ctypes.data_as(_lib.c_u8p),
                                           ivs.ctypes.data_as(_lib.c_u8p), status.ctypes.data_as(_lib.c_u32p),
                                           _p(scratch), scratch.numel(), _stream()))
    return keys[:nstreams], ivs[:nstreams], status[:nstreams]


def plain_read_layout(chunk_len, padding, req_stream, start, length, align: int = 16):
    """read_layout for requests in plaintext bytes of level-13 streams: (content_off,
    content_len, content_total, nseg) of plaintext [start, min(P, start +
    length)), P = 4 chunk_len - padding - 97."""
    cl, pcl, nstreams = _arr(chunk_len, np.uint32)
    pad, ppad, npad = _arr(padding, np.uint32)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nl = _arr(length)
    assert npad == nstreams and ns == nreq == nl
    off, clen = np.zeros(max(nreq, 1), dtype=np.uint64), np.zeros(max(nreq, 1), dtype=np.uint64)
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().chipc_read_layout(pcl, ppad, nstreams, prs, pst, pln, nreq, align, off.ctypes.data_as(_lib.c_u64p),
                                       clen.ctypes.data_as(_lib.c_u64p), ctypes.byref(total), ctypes.byref(nseg)))
    return off[:nreq].tolist(), clen[:nreq].tolist(), total.value, nseg.value


def plain_read_scratch(nreq: int, nseg: int, nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a read_plain_ranges call of nreq requests in nseg segments (plain_read_layout)."""
    size = _lib.lib().chipc_read_scratch_len(nreq, nseg, nstreams)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
    assert streams.is_cuda and content.is_cuda and hashes.is_cuda and status.is_cuda and used.is_cuda and scratch.is_cuda
    assert vouch.is_cuda
    assert streams.dtype == content.dtype == torch.uint8 and streams.dim() == content.dim() == 1
    assert streams.is_contiguous() and content.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nln = _arr(length)
    coff, pcoff, nco = _arr(content_off)
    assert nl == nstreams == npad == ncl and ns == nreq == nln == nco
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
    for t in (status, used, vouch):
        assert t.numel() >= nreq and t.element_size() == 4 and t.is_contiguous()
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        _, want, _, _ = plain_read_layout(cl[:nstreams], pad[:nstreams], rs[:nreq], st[:nreq], ln[:nreq])
        assert _fits(coff, np.asarray(want, dtype=np.uint64), content.numel())
    kk, pk, vv, pv = _gcm_keys(keys, ivs, nstreams)
    pks = None
    if key_status is not None:
        ks, pks, nks = _arr(key_status, np.uint32)
        assert nks == nstreams
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    check(_lib.lib().chipc_read_ranges_dev(pk, pv, pks, _p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams, prs,
                                           pst, pln, nreq, _p(content), pcoff, clen.ctypes.data_as(_lib.c_u64p),
                                           _p(status), _p(used), _p(vouch), flags, _p(scratch), scratch.numel(),
                                           _stream()))
    return clen[:nreq].tolist()


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
    k = np.ascontiguousarray(np.frombuffer(bytes(keys), dtype=np.uint8) if not isinstance(keys, np.ndarray) else keys,
                             dtype=np.uint8).reshape(-1)
    nstreams = k.size // 32
    kk, pk, vv, pv = _gcm_keys(k, ivs, nstreams)
    pks = None
    if key_status is not None:
        ks, pks, nks = _arr(key_status, np.uint32)
        assert nks == nstreams
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
    return torch.empty(size, dtype=torch.uint8, device=device or table.table.device)


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
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def snap_ragged(inp: torch.Tensor, in_off, n, out: torch.Tensor, out_off, out_len: torch.Tensor,
                scratch: torch.Tensor) -> None:
    """encoding::snap of every object inp[in_off[o] : in_off[o] + n[o]] (16-B
    aligned): its frame stream, the bytes chip_snap_compress gives, to
    out[out_off[o] :] at any byte offset (capacity snap_max_len(n[o])), its
    length to out_len[o] (int64 [count] on the device).  Enqueued on the
    current stream, not synchronised."""
    assert inp.is_cuda and out.is_cuda and out_len.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(n)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and out_len.numel() >= count and out_len.element_size() == 8 and out_len.is_contiguous()
    worst = np.array([snap_max_len(x) for x in ln[:count]], dtype=np.uint64)
    assert _fits(ioff, ln[:count], inp.numel()) and _fits(ooff, worst, out.numel())
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
    assert inp.is_cuda and out.is_cuda and out_len.is_cuda and status.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(in_len)
    ooff, pooff, no = _arr(out_off)
    cap, pcap, nc = _arr(out_cap)
    assert nl == count == no == nc
    assert out_len.numel() >= count and out_len.element_size() == 8 and out_len.is_contiguous()
    assert status.numel() >= count and status.element_size() == 4 and status.is_contiguous()
    assert _fits(ioff, ln[:count], inp.numel()) and _fits(ooff, cap[:count], out.numel())
    check(_lib.lib().chips_unsnap_ragged_dev(_p(inp), pioff, pln, count, _p(out), pooff, pcap, _p(out_len), _p(status),
                                             _p(scratch), scratch.numel(), _stream()))


def snap_encode_layout(fmt: int, sizes, align: int = 256, stream_offset: int = STREAM_OFFSET):
    """Where encode_ragged_snap's caller should put each object (host only):
    ragged_layout over the worst-case lengths, since the encoded length depends
    on the data.  Returns (out_off, out_cap, total)."""
    n, pn, count = _arr(sizes)
    off, cap = np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
    total = ctypes.c_uint64()
    check(_lib.lib().chips_encode_layout(fmt, pn, count, align, stream_offset, off.ctypes.data_as(_lib.c_u64p),
                                         cap.ctypes.data_as(_lib.c_u64p), ctypes.byref(total)))
    return off[:count].tolist(), cap[:count].tolist(), total.value


def snap_ragged_scratch(fmt: int, lens, out_cap=None, device=None) -> torch.Tensor:
    """Scratch of encode_ragged_snap (object lengths) or, with out_cap, of
    decode_ragged_snap (stream lengths and output capacities)."""
    ln, pln, count = _arr(lens)
    if out_cap is None:
        size = _lib.lib().chips_encode_scratch_len(fmt, pln, count)
    else:
        cap, pcap, _ = _arr(out_cap)
        size = _lib.lib().chips_decode_scratch_len(fmt, pln, pcap, count)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


def encode_ragged_snap(fmt: int, inp: torch.Tensor, in_off, sizes, out: torch.Tensor, out_off, hashes: torch.Tensor,
                       scratch: torch.Tensor, pubkey: bytes = None, inject=None):
    """encode() at a format with the Snappy bit and Bao and / or Zfec (6, 7,
    10, 11, 14, 15) of resident objects in one call: compressed into rows of
    the scratch, then (sealed and) encoded as encode_ragged does at fmt & 12.
    The call waits once, for the compressed lengths.  Offsets:
    snap_encode_layout(fmt, sizes).  Stream bytes, hash and EncodeInfo are
    those of encode() at fmt.  Returns (encoded length per object, EncodeInfo
    per object)."""
    from .structs import EncodeInfo
    assert inp.is_cuda and out.is_cuda and hashes.is_cuda and scratch.is_cuda
    assert inp.dtype == out.dtype == torch.uint8 and inp.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(sizes)
    ooff, pooff, no = _arr(out_off)
    assert nl == count == no and hashes.numel() >= 32 * count and hashes.is_contiguous()
    assert _fits(ioff, ln[:count], inp.numel())
    assert scratch.numel() >= _lib.lib().chips_encode_scratch_len(fmt, pln, count)
    inj, keep = _inject_array(inject, count)
    olen = (ctypes.c_uint64 * max(count, 1))()
    info = (_lib.EncodeInfoC * max(count, 1))()
    pk = bytes(pubkey) if pubkey is not None else None
    check(_lib.lib().chips_encode_ragged_dev(fmt, pk, len(pk) if pk else 0, inj, _p(inp), pioff, pln, count, _p(out),
                                             pooff, olen, _p(hashes), info, _p(scratch), _stream()))
    assert all(int(a) + b <= out.numel() for a, b in zip(ooff[:count], list(olen)[:count]))
    return list(olen)[:count], [EncodeInfo.from_c(info[o]) for o in range(count)]


def decode_ragged_snap(fmt: int, enc: torch.Tensor, in_off, in_len, hashes: torch.Tensor, padding, out: torch.Tensor,
                       out_off, out_cap, out_len: torch.Tensor, status: torch.Tensor, scratch: torch.Tensor,
                       secret_key: bytes = None) -> None:
    """decode() at 6, 7, 10, 11, 14 or 15 of resident streams in one call:
    decode_ragged (or decode_ragged_ecies) into rows of the scratch, then
    unsnap_ragged into out[out_off[o] :] (capacity out_cap[o]).  status[o]: 0,
    the bao / ecies status of an object that failed there (not decompressed,
    nothing written), or a snappy status; out_len[o] (int64 on the device): the
    decoded length.  Without the Ecies bit nothing is waited for."""
    assert enc.is_cuda and out.is_cuda and status.is_cuda and scratch.is_cuda and out_len.is_cuda
    assert enc.dtype == out.dtype == torch.uint8 and enc.is_contiguous() and out.is_contiguous()
    ioff, pioff, count = _arr(in_off)
    ln, pln, nl = _arr(in_len)
    ooff, pooff, no = _arr(out_off)
    cap, pcap, nc = _arr(out_cap)
    pad, ppad, npad = _arr(padding, np.uint32)
    assert nl == count == no == npad == nc and _fits(ioff, ln[:count], enc.numel())
    assert _fits(ooff, cap[:count], out.numel())
    assert status.numel() >= count and status.element_size() == 4 and status.is_contiguous()
    assert out_len.numel() >= count and out_len.element_size() == 8 and out_len.is_contiguous()
    assert scratch.numel() >= _lib.lib().chips_decode_scratch_len(fmt, pln, pcap, count)
    sk = bytes(secret_key) if secret_key is not None else None
    check(_lib.lib().chips_decode_ragged_dev(fmt, sk, len(sk) if sk else 0, _p(enc), pioff, pln, count,
                                             _p(hashes) if hashes is not None else None, ppad, _p(out), pooff, pcap,
                                             _p(out_len), _p(status), _p(scratch), _stream()))


# ---- plaintext ranged reads of level-14 / level-15 streams
# (include/carbonado_hip_fread.h): the frame index of resident streams, its
# proof against the stream, the read

def _stream_args(streams, in_off, in_len, hashes, padding, chunk_len):
    assert streams.is_cuda and hashes.is_cuda and streams.dtype == torch.uint8
    assert streams.is_contiguous() and hashes.is_contiguous()
    ioff, pioff, nstreams = _arr(in_off)
    ilen, pilen, nl = _arr(in_len)
    pad, ppad, npad = _arr(padding, np.uint32)
    cl, pcl, ncl = _arr(chunk_len, np.uint32)
    assert nl == nstreams == npad == ncl
    assert hashes.numel() >= 32 * nstreams and _fits(ioff, ilen[:nstreams], streams.numel())
    return (ioff, ilen, pad, cl), (pioff, pilen, ppad, pcl), nstreams


def _frame_keys(fmt, keys, ivs, key_status, nstreams):
    """(keep-alive, keys pointer, ivs pointer, key_status pointer): looked at for format 15 only"""
    if fmt != 15 or keys is None:
        return None, None, None, None
    kk, pk, vv, pv = _gcm_keys(keys, ivs, nstreams)
    ks, pks = None, None
    if key_status is not None:
        ks, pks, nks = _arr(key_status, np.uint32)
        assert nks == nstreams
    return (kk, vv, ks), pk, pv, pks


def frame_index_scratch(nstreams: int, nentries: int, device=None) -> torch.Tensor:
    """Scratch of a frame_index or verify_frame_index call over nstreams streams
    and nentries index entries in all (the capacities, or nframes + 1 each)."""
    size = _lib.lib().chipf_index_scratch_len(nstreams, nentries)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
                                                                              chunk_len)
    io, pio, nio = _arr(idx_off)
    cap, pcap, ncap = _arr(idx_cap)
    assert nio == nstreams == ncap and scratch.is_cuda
    total = int((io[:nstreams] + cap[:nstreams]).max()) if nstreams else 0
    frame_off = np.zeros(max(total, 1), dtype=np.uint64)
    nframes = np.zeros(max(nstreams, 1), dtype=np.uint64)
    status = np.zeros(max(nstreams, 1), dtype=np.uint32)
    plain = np.zeros(max(nstreams, 1), dtype=np.uint64)
    vouch = np.zeros(max(nstreams, 1), dtype=np.uint32)
    keep, pk, pv, pks = _frame_keys(fmt, keys, ivs, key_status, nstreams)
    check(_lib.lib().chipf_frame_index_dev(fmt, pk, pv, pks, _p(streams), pioff, pilen, _p(hashes), ppad, pcl, nstreams,
                                           frame_off.ctypes.data_as(_lib.c_u64p), pio, pcap,
                                           nframes.ctypes.data_as(_lib.c_u64p), status.ctypes.data_as(_lib.c_u32p),
                                           plain.ctypes.data_as(_lib.c_u64p), vouch.ctypes.data_as(_lib.c_u32p),
                                           _p(scratch), scratch.numel(), _stream()))
    return frame_off[:total], nframes[:nstreams], status[:nstreams], plain[:nstreams], vouch[:nstreams]


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
                                                                              chunk_len)
    fo, pfo, nfo = _arr(frame_off)
    io, pio, nio = _arr(idx_off)
    nf, pnf, nnf = _arr(nframes)
    assert nio == nstreams == nnf and scratch.is_cuda
    assert all(int(io[s]) + int(nf[s]) + 1 <= nfo for s in range(nstreams))
    for t, size in ((index_status, 4), (plain_len, 8), (index_vouch, 4)):
        assert t.is_cuda and t.numel() >= nstreams and t.element_size() == size and t.is_contiguous()
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
    cl, pcl, nstreams = _arr(chunk_len, np.uint32)
    pad, ppad, npad = _arr(padding, np.uint32)
    fo, pfo, nfo = _arr(frame_off)
    io, pio, nio = _arr(idx_off)
    nf, pnf, nnf = _arr(nframes)
    pl, ppl, npl = _arr(plain_len)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nl = _arr(length)
    assert npad == nstreams == nio == nnf == npl and ns == nreq == nl
    assert all(int(io[s]) + int(nf[s]) + 1 <= nfo for s in range(nstreams))
    off, clen = np.zeros(max(nreq, 1), dtype=np.uint64), np.zeros(max(nreq, 1), dtype=np.uint64)
    total, nseg, stage, vseg = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    pis = None
    if index_status is not None:
        ist, pis, nis = _arr(index_status, np.uint32)
        assert nis == nstreams
    check(_lib.lib().chipf_read_layout(fmt, pcl, ppad, pis, pfo, pio, pnf, ppl, nstreams, prs, pst, pln, nreq, align,
                                       off.ctypes.data_as(_lib.c_u64p), clen.ctypes.data_as(_lib.c_u64p),
                                       ctypes.byref(total), ctypes.byref(nseg), ctypes.byref(stage), ctypes.byref(vseg)))
    return off[:nreq].tolist(), clen[:nreq].tolist(), total.value, nseg.value, stage.value, vseg.value


def frame_read_scratch(nreq: int, nseg: int, stage_total: int, vseg: int, nstreams: int, device=None) -> torch.Tensor:
    """Scratch of a read_frame_ranges call (the numbers of frame_read_layout)."""
    size = _lib.lib().chipf_read_scratch_len(nreq, nseg, stage_total, vseg, nstreams)
    return torch.empty(size, dtype=torch.uint8, device=device or "cuda")


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
                                                                              chunk_len)
    assert content.is_cuda and status.is_cuda and used.is_cuda and vouch.is_cuda and scratch.is_cuda
    assert content.dtype == torch.uint8 and content.dim() == 1 and content.is_contiguous()
    fo, pfo, nfo = _arr(frame_off)
    io, pio, nio = _arr(idx_off)
    nf, pnf, nnf = _arr(nframes)
    pl, ppl, npl = _arr(plain_len)
    rs, prs, nreq = _arr(req_stream, np.uint32)
    st, pst, ns = _arr(start)
    ln, pln, nln = _arr(length)
    coff, pcoff, nco = _arr(content_off)
    assert nio == nstreams == nnf == npl and ns == nreq == nln == nco
    assert all(int(io[s]) + int(nf[s]) + 1 <= nfo for s in range(nstreams))
    for t in (status, used, vouch):
        assert t.numel() >= nreq and t.element_size() == 4 and t.is_contiguous()
    if nreq and int(rs.max()) < nstreams:  # the content buffer is checked before the call (else: the call reports it)
        want = np.array([min(max(int(pl[s]) - int(a), 0), int(n)) for s, a, n in zip(rs[:nreq], st[:nreq], ln[:nreq])],
                        dtype=np.uint64)
        assert _fits(coff, want, content.numel())
    keep, pk, pv, _ = _frame_keys(fmt, keys, ivs, None, nstreams)
    pis = None
    if index_status is not None:
        ist, pis, nis = _arr(index_status, np.uint32)
        assert nis == nstreams
    clen = np.zeros(max(nreq, 1), dtype=np.uint64)
    check(_lib.lib().chipf_read_ranges_dev(fmt, pk, pv, pis, pfo, pio, pnf, ppl, _p(streams), pioff, pilen, _p(hashes),
                                           ppad, pcl, nstreams, prs, pst, pln, nreq, _p(content), pcoff,
                                           clen.ctypes.data_as(_lib.c_u64p), _p(status), _p(used), _p(vouch), flags,
                                           _p(scratch), scratch.numel(), _stream()))
    return clen[:nreq].tolist()


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
