#!/usr/bin/env python3
"""Slice audits planned on the device against the host-planned ones, on
audit_bench.py's set (GPU only; not bench.py): --streams resident bao streams
of 1 MiB of content in one buffer, random 1 KiB slices, one per stream and 16
per stream.

  planned_verify  chipp_verify_slices_dev (include/carbonado_hip_paudit.h): the
                  requests are device arrays, a kernel plans them, no upload
  host_verify     chipa_verify_slices_dev: the host plans and uploads a table
  planned_cycle   chipp_extract_slices_dev then chipp_verify_proofs_dev
  host_cycle      chipa_extract_slices_dev then chipa_verify_proofs_dev
  replay          one captured chipp_verify_slices_dev call, replayed

Before anything is timed every form's verdicts are checked and its content
compared with the streams' input, all of it.  A time is between two HIP events
around the call (no call synchronises); host_*_ms is the host clock around the
same call.  3 warm-ups, the forms alternating within one process for --reps
rounds; medians and min-max in ms, the GPU's clocks sampled meanwhile.  Prints
one JSON line (and writes it to --out) with the conditions the device plan was
built on: (a) at 16 slices per stream the planned median is below the
host-planned call's minimum, for verify and for the cycle; (b) at one slice per
stream the planned median is not above the host-planned maximum; (c) the host
time of the planned call at 16 slices per stream over its own at one, beside
the same ratio of the host-planned call (reported, not judged).

--dry needs no device: the capacity, the strides, the scratch sizes and the
launch counts of both request sets through the library's host-only calls."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

CONTENT = 1 << 20
SLICE = 1024
MAX_COUNT = 1
LAUNCHES = {"verify": 4, "extract": 2, "verify_proofs": 4}


def up16(x):
    return -(-x // 16) * 16


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    S, N = args.streams, CONTENT // 1024
    bound = L.chipp_proof_bound(N, MAX_COUNT)
    res = {"tool": "paudit_bench", "dry_run": True, "seed": args.seed, "streams": S, "content_bytes": CONTENT,
           "slice_bytes": SLICE, "table_bytes": L.chipq_stream_table_len(S), "root_table_bytes": L.chipp_root_table_len(S),
           "launches": LAUNCHES, "uploads_per_call": 0, "memsets_per_call": 0}
    for per in (1, 16):
        nreq = S * per
        res[f"audit_{per}"] = {
            "requests": nreq, "max_count": MAX_COUNT, "parent_slots": (bound - 8 - 1024 * MAX_COUNT) // 64,
            "content_stride": 1024 * MAX_COUNT, "proof_bound": bound, "proof_stride": up16(bound),
            "scratch_bytes": L.chipp_audit_scratch_len(N, nreq, MAX_COUNT),
            "host_planned_scratch_bytes": L.chipa_audit_scratch_len(S, nreq)}
    print(json.dumps(res))
    return 0


def time_forms(forms, reps):
    import torch
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms, host = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            f()
            host[k].append((time.perf_counter() - t0) * 1e3)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    r4 = lambda x: round(x, 4)  # noqa: E731
    return {k: {"median_ms": r4(statistics.median(v)), "min_ms": r4(min(v)), "max_ms": r4(max(v)),
                "host_median_ms": r4(statistics.median(host[k])), "host_min_ms": r4(min(host[k])),
                "host_max_ms": r4(max(host[k]))} for k, v in ms.items()}


class Set:
    """The resident streams of audit_bench.py and `per` random 1 KiB slices per stream, both ways."""

    def __init__(self, L, S, per, seed):
        import numpy as np
        import torch
        from carbonado_amd import device as D
        self.torch, self.D, self.np = torch, D, np
        n, N = CONTENT, CONTENT // 1024
        blen = L.chip_bao_encoded_len(n)
        pitch = -(-(D.STREAM_OFFSET + blen) // 256) * 256
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.inp = torch.randint(0, 256, (S, n), dtype=torch.uint8, device="cuda", generator=gen)
        enc = torch.zeros((S, pitch), dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
        D.bao_encode_batch(self.inp, n, enc, self.hashes, D.bao_scratch(n, S), out_offset=D.STREAM_OFFSET)
        torch.cuda.synchronize()
        self.flat = enc.view(-1)
        self.in_off = np.arange(S, dtype=np.uint64) * np.uint64(pitch) + np.uint64(D.STREAM_OFFSET)
        self.in_len = np.full(S, blen, dtype=np.uint64)
        rng = np.random.default_rng(seed + 1)
        nreq = self.nreq = S * per
        self.rs = np.repeat(np.arange(S), per).astype(np.uint32)
        self.idx = rng.integers(0, N, nreq).astype(np.uint64)
        self.cnt = np.ones(nreq, dtype=np.uint64)
        self.ns = np.full(nreq, n, dtype=np.uint64)
        # host-planned: the packed layout, one hash per request for the proofs
        poff, plen, coff, clen, ptotal, ctotal = D.slice_layout(self.ns, self.idx, self.cnt, 16)
        self.poff, self.plen, self.coff = (np.array(x, dtype=np.uint64) for x in (poff, plen, coff))
        assert clen == [SLICE] * nreq and ctotal == nreq * SLICE
        self.h_proofs = torch.empty(ptotal + 16, dtype=torch.uint8, device="cuda")
        self.h_content = torch.empty(ctotal + 16, dtype=torch.uint8, device="cuda")
        self.h_status = torch.empty(nreq, dtype=torch.int32, device="cuda")
        self.h_scratch = D.audit_scratch(S, nreq)
        self.req_hashes = self.hashes[torch.from_numpy(self.rs.astype(np.int64)).cuda()].contiguous()
        # planned: the tables, the requests on the device, slots
        t0 = time.perf_counter()
        self.table = D.stream_table(self.flat, self.in_off, self.in_len, self.hashes, [0] * S, [1024] * S)
        self.roots = D.root_table(np.full(S, n, dtype=np.uint64), self.hashes)
        torch.cuda.synchronize()
        self.tables_ms = (time.perf_counter() - t0) * 1e3
        dev = lambda x, dt: torch.from_numpy(x.astype(dt)).cuda()  # noqa: E731
        self.d_rs, self.d_idx, self.d_cnt = dev(self.rs, "int32"), dev(self.idx, "int64"), dev(self.cnt, "int64")
        self.cs, self.ps = 1024 * MAX_COUNT, up16(D.proof_bound(N, MAX_COUNT))
        self.content = torch.empty(nreq * self.cs, dtype=torch.uint8, device="cuda")
        self.proofs = torch.empty(nreq * self.ps, dtype=torch.uint8, device="cuda")
        self.clen = torch.empty(nreq, dtype=torch.int64, device="cuda")
        self.plen_d = torch.empty(nreq, dtype=torch.int64, device="cuda")
        self.status = torch.empty(nreq, dtype=torch.int32, device="cuda")
        self.scratch = D.planned_audit_scratch(self.table, nreq, MAX_COUNT)
        self.graph = None

    def planned_verify(self):
        self.D.verify_slices_planned(self.table, self.d_rs, self.d_idx, self.d_cnt, MAX_COUNT, self.content, self.cs,
                                     self.clen, self.status, self.scratch)

    def planned_cycle(self):
        D = self.D
        D.extract_slices_planned(self.table, self.d_rs, self.d_idx, self.d_cnt, MAX_COUNT, self.proofs, self.ps,
                                 self.plen_d, self.status, self.scratch)
        D.verify_slice_proofs_planned(self.roots, self.d_rs, self.d_idx, self.d_cnt, MAX_COUNT, self.proofs, self.ps,
                                      self.plen_d, self.content, self.cs, self.clen, self.status, self.scratch)

    def host_verify(self):
        self.D.verify_slices(self.flat, self.in_off, self.in_len, self.hashes, self.rs, self.idx, self.cnt,
                             self.h_content, self.coff, self.h_status, self.h_scratch)

    def host_cycle(self):
        D = self.D
        D.extract_slices(self.flat, self.in_off, self.in_len, self.rs, self.idx, self.cnt, self.h_proofs, self.poff,
                         self.plen, self.h_scratch)
        D.verify_slice_proofs(self.h_proofs, self.poff, self.plen, self.ns, self.req_hashes, self.idx, self.cnt,
                              self.h_content, self.coff, self.h_status, self.h_scratch)

    def capture(self):
        torch = self.torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            self.planned_verify()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.planned_verify()

    def replay(self):
        self.graph.replay()

    def check(self):
        """every form: all verdicts 0, every request's bytes those of the streams' input"""
        torch = self.torch
        at = self.d_idx * 1024
        want = self.inp[self.d_rs.to(torch.int64)[:, None], at[:, None] + torch.arange(SLICE, device="cuda")[None, :]]
        for name, f in (("planned_verify", self.planned_verify), ("planned_cycle", self.planned_cycle),
                        ("replay", self.replay)):
            self.content.fill_(0xA5); self.status.fill_(-1); self.clen.fill_(-1)
            f()
            torch.cuda.synchronize()
            assert int(self.status.count_nonzero()) == 0 and bool((self.clen == SLICE).all()), name
            assert torch.equal(self.content.view(self.nreq, self.cs)[:, :SLICE], want), name
        assert bool((self.plen_d == torch.from_numpy(self.plen.astype("int64")).cuda()).all())
        for name, f in (("host_verify", self.host_verify), ("host_cycle", self.host_cycle)):
            self.h_content.fill_(0xA5); self.h_status.fill_(-1)
            f()
            torch.cuda.synchronize()
            assert int(self.h_status.count_nonzero()) == 0, name
            assert torch.equal(self.h_content[:self.nreq * SLICE].view(self.nreq, SLICE), want), name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry", action="store_true", help="no device: sizes and launch counts only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paudit_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)
    import torch
    from bench import ClockSampler
    from carbonado_amd import _lib
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "paudit_bench", "seed": args.seed, "streams": args.streams, "content_bytes": CONTENT,
           "slice_bytes": SLICE, "reps": args.reps, "launches": LAUNCHES,
           "timing": "HIP events around each call, host_*_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    for per in (1, 16):
        s = Set(L, args.streams, per, args.seed + per)
        s.capture()
        s.check()
        r = {"requests": s.nreq, "max_count": MAX_COUNT, "content_stride": s.cs, "proof_stride": s.ps,
             "tables_ms": round(s.tables_ms, 4),
             **time_forms({"planned_verify": s.planned_verify, "host_verify": s.host_verify,
                           "planned_cycle": s.planned_cycle, "host_cycle": s.host_cycle, "replay": s.replay},
                          args.reps)}
        r["planned_verify_over_host_verify"] = round(r["planned_verify"]["median_ms"] / r["host_verify"]["median_ms"], 3)
        r["planned_cycle_over_host_cycle"] = round(r["planned_cycle"]["median_ms"] / r["host_cycle"]["median_ms"], 3)
        res[f"audit_{per}"] = r
        del s
        torch.cuda.empty_cache()
    res["clocks"] = clocks.stop()
    a1, a16 = res["audit_1"], res["audit_16"]
    res["a_planned_median_below_host_min_at_16"] = {
        k: a16[f"planned_{k}"]["median_ms"] < a16[f"host_{k}"]["min_ms"] for k in ("verify", "cycle")}
    res["b_planned_median_not_above_host_max_at_1"] = {
        k: a1[f"planned_{k}"]["median_ms"] <= a1[f"host_{k}"]["max_ms"] for k in ("verify", "cycle")}
    res["c_host_time_16_over_1"] = {
        k: round(a16[k]["host_median_ms"] / a1[k]["host_median_ms"], 2)
        for k in ("planned_verify", "host_verify", "planned_cycle", "host_cycle")}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
