#!/usr/bin/env python3
"""Slice audits of device-resident streams against what the library offered
before them (GPU only; not bench.py).

Workload: 1024 resident bao streams of 1 MiB of content each, at the fast
layout (56 bytes into rows of 256-B multiple pitch).  Request shapes:
  1. one random 1 KiB slice per stream          (1024 requests)
  2. 16 random 1 KiB slices per stream          (16384 requests)
  3. one run of 64 slices per stream            (1024 requests, 64 KiB each)
For each shape, in alternating rounds on the same box:
  verify          chipa_verify_slices_dev (device.verify_slices)
  extract+proofs  chipa_extract_slices_dev then chipa_verify_proofs_dev
  full decode     chip_bao_decode_batch_dev of all 1024 streams: the only
                  device-side check there was
and, once, the per-request host call decoding.verify_slice on a sample of 32
requests (each uploads and re-hashes its whole stream).  A time is the host
clock around `--calls` back-to-back calls ending in a device synchronise,
divided by the calls: it includes the host-side planning and the table upload
of every call.  Every request's status is checked, and the content against the
streams' input.

Writes one JSON document (default profiles/audit_bench_mi355x.json); the one
hard condition, shape 1 faster than the full decode, is recorded in it and
decides the exit status.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--content", type=int, default=1 << 20, help="content bytes per stream")
    ap.add_argument("--rounds", type=int, default=15, help="alternating rounds per shape")
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timing")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "audit_bench_mi355x.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from carbonado_amd import _lib, decoding
    from carbonado_amd import device as D

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc}): {L.chip_last_device_error().decode()}")

    S, n = a.streams, a.content
    N = max(1, -(-n // 1024))
    blen = L.chip_bao_encoded_len(n)
    pitch = -(-(D.STREAM_OFFSET + blen) // 256) * 256
    gen = torch.Generator(device="cuda").manual_seed(1)
    inp = torch.randint(0, 256, (S, n), dtype=torch.uint8, device="cuda", generator=gen)
    enc = torch.zeros((S, pitch), dtype=torch.uint8, device="cuda")
    hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
    D.bao_encode_batch(inp, n, enc, hashes, D.bao_scratch(n, S), out_offset=D.STREAM_OFFSET)
    torch.cuda.synchronize()
    flat = enc.view(-1)
    in_off = np.arange(S, dtype=np.uint64) * np.uint64(pitch) + np.uint64(D.STREAM_OFFSET)
    in_len = np.full(S, blen, dtype=np.uint64)

    # the full decode (what there was): all streams, content written out
    dec_out = torch.empty((S, n), dtype=torch.uint8, device="cuda")
    dec_status = torch.zeros(S, dtype=torch.int32, device="cuda")
    dec_scratch = D.bao_scratch(n, S)

    def full_decode():
        D.bao_decode_batch(enc, n, hashes, dec_out, dec_status, dec_scratch, in_offset=D.STREAM_OFFSET)

    rng = np.random.default_rng(2)
    shapes = {
        "1_one_slice_per_stream": (np.arange(S), rng.integers(0, N, S), np.ones(S, dtype=np.int64)),
        "2_sixteen_slices_per_stream": (np.repeat(np.arange(S), 16), rng.integers(0, N, 16 * S),
                                        np.ones(16 * S, dtype=np.int64)),
        "3_one_run_of_64_slices_per_stream": (np.arange(S), rng.integers(0, max(1, N - 64), S),
                                              np.full(S, min(64, N), dtype=np.int64)),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.calls * 1e3  # ms per call

    def stats(xs):
        return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
                "max_ms": round(max(xs), 4)}

    result = {"device": torch.cuda.get_device_name(0), "streams": S, "content_bytes": n, "stream_bytes": blen,
              "rounds": a.rounds, "calls_per_timing": a.calls,
              "timing": "host clock around back-to-back calls ending in a device synchronise, per call; "
                        "host planning and table upload included; one box, one run",
              "shapes": {}}
    for name, (rs, idx, cnt) in shapes.items():
        rs, idx, cnt = rs.astype(np.uint32), idx.astype(np.uint64), cnt.astype(np.uint64)
        nreq = rs.size
        poff, plen, coff, clen, ptotal, ctotal = D.slice_layout(np.full(nreq, n, dtype=np.uint64), idx, cnt, 16)
        poff, plen, coff = (np.array(x, dtype=np.uint64) for x in (poff, plen, coff))
        proofs = torch.empty(ptotal + 16, dtype=torch.uint8, device="cuda")
        content = torch.empty(ctotal + 16, dtype=torch.uint8, device="cuda")
        status = torch.empty(nreq, dtype=torch.int32, device="cuda")
        scratch = D.audit_scratch(S, nreq)
        req_hashes = hashes[torch.from_numpy(rs.astype(np.int64)).cuda()].contiguous()
        ns = np.full(nreq, n, dtype=np.uint64)

        def verify():
            D.verify_slices(flat, in_off, in_len, hashes, rs, idx, cnt, content, coff, status, scratch)

        def extract():
            D.extract_slices(flat, in_off, in_len, rs, idx, cnt, proofs, poff, plen, scratch)

        def proofs_verify():
            D.verify_slice_proofs(proofs, poff, plen, ns, req_hashes, idx, cnt, content, coff, status, scratch)

        def extract_then_proofs():
            extract()
            proofs_verify()

        # every verdict and the content, for both paths, before any timing
        def check(tag):
            torch.cuda.synchronize()
            assert int((status != 0).sum()) == 0, f"{name}/{tag}: a clean request failed"
            got = content.cpu().numpy()
            host_in = None
            for r in np.linspace(0, nreq - 1, min(nreq, 256)).astype(int):
                if host_in is None or host_in[0] != rs[r]:
                    host_in = (rs[r], inp[int(rs[r])].cpu().numpy())
                s0 = int(idx[r]) * 1024
                want = host_in[1][s0:s0 + int(cnt[r]) * 1024]
                assert clen[r] == want.size and (got[int(coff[r]):int(coff[r]) + want.size] == want).all(), (name, tag, r)

        content.fill_(0xA5); status.fill_(-1)
        verify(); check("verify")
        content.fill_(0xA5); status.fill_(-1)
        extract_then_proofs(); check("proofs")
        full_decode()
        torch.cuda.synchronize()
        assert int((dec_status != 0).sum()) == 0

        for _ in range(a.warmup):
            verify(); extract_then_proofs(); full_decode()
        t = {"verify_slices": [], "extract_then_verify_proofs": [], "extract_only": [], "full_bao_decode_batch": []}
        for _ in range(a.rounds):  # alternating
            t["verify_slices"].append(timed(verify))
            t["extract_then_verify_proofs"].append(timed(extract_then_proofs))
            t["extract_only"].append(timed(extract))
            t["full_bao_decode_batch"].append(timed(full_decode))

        # the per-request host call on a sample (each uploads and checks its whole stream)
        sample = np.linspace(0, nreq - 1, min(nreq, a.host_sample)).astype(int)
        rows = {int(s): enc[int(s), D.STREAM_OFFSET:D.STREAM_OFFSET + blen].cpu().numpy().tobytes()
                for s in set(rs[sample].tolist())}
        hh = hashes.cpu().numpy()
        host_ms = []
        for r in sample:
            s = int(rs[r])
            t0 = time.perf_counter()
            out = decoding.verify_slice(hh[s].tobytes(), rows[s], int(idx[r]), int(cnt[r]))
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert len(out) == clen[r]
        med = {k: statistics.median(v) for k, v in t.items()}
        per_req_host = statistics.median(host_ms)
        result["shapes"][name] = {
            "requests": int(nreq), "chunks_hashed": int(cnt.sum()), "proof_bytes": int(plen.sum()),
            "content_bytes": int(sum(clen)),
            **{k: stats(v) for k, v in t.items()},
            "host_verify_slice_per_request": {**stats(host_ms), "sample": int(sample.size)},
            "ratios": {
                "full_decode_over_verify_slices": round(med["full_bao_decode_batch"] / med["verify_slices"], 2),
                "full_decode_over_extract_then_verify_proofs":
                    round(med["full_bao_decode_batch"] / med["extract_then_verify_proofs"], 2),
                "host_calls_for_all_requests_over_verify_slices":
                    round(per_req_host * nreq / med["verify_slices"], 1),
            },
        }
        print(name, json.dumps(result["shapes"][name]["ratios"]), flush=True)

    s1 = result["shapes"]["1_one_slice_per_stream"]
    ok = s1["verify_slices"]["median_ms"] < s1["full_bao_decode_batch"]["median_ms"]
    result["shape1_verify_faster_than_full_decode"] = bool(ok)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"shape1_verify_faster_than_full_decode": bool(ok), "out": str(out)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
