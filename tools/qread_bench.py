#!/usr/bin/env python3
"""Ranged reads planned on the device against the host-planned ones, on
read_bench.py's set (GPU only; not bench.py): --streams streams of 1 MiB
objects at level 12 in one buffer, random 4 KiB object ranges, one per stream
and 16 per stream, intact and with 1 stream in 64 damaged inside its first
range.

  planned          chipq_read_ranges_dev (include/carbonado_hip_qread.h): the
                   requests are device arrays, a kernel plans them, no upload
  host             chipd_read_ranges_dev: the host plans and uploads a table
  planned_vouched  chipq_read_ranges_vouched_dev
  host_vouched     chipv_read_ranges_dev
  replay           one captured chipq_read_ranges_dev call, replayed
  stream_table     chipq_stream_table_dev, the once-per-set upload (timed apart)

Before anything is timed every form's bytes are compared with the clean
objects, all of them.  A time is between two HIP events around the call (no
call synchronises); host_*_ms is the host clock around the same call.  3
warm-ups, the forms alternating within one process for --reps rounds; medians
and min-max in ms, the GPU's clocks sampled meanwhile.  Prints one JSON line
(and writes it to --out) with the two conditions the device plan was built on:
at 16 ranges per stream its median is below the host-planned call's, and at
one range per stream it is not slower than that call by more than that call's
own min-max spread.

--dry needs no device: the capacity, the table and scratch sizes and the
launch geometry of both request sets through the library's host-only calls."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

OBJ = 1 << 20
RANGE = 4096
LAUNCHES = {"plan": 4, "read": 6, "vouched_read": 8}


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    S = args.streams
    C = OBJ // 4
    info = _lib.TableInfo(S, 8 * C // 1024, C, 0)
    res = {"tool": "qread_bench", "dry_run": True, "seed": args.seed, "streams": S, "object_bytes": OBJ - 41,
           "range_bytes": RANGE, "table_bytes": L.chipq_stream_table_len(S), "launches": LAUNCHES,
           "uploads_per_read": 0, "memsets_per_read": 0}
    for per in (1, 16):
        nreq = S * per
        slots = min(4, 1 + -(-(RANGE - 1) // C))
        res[f"read_{per}"] = {
            "requests": nreq, "max_len": RANGE, "content_stride": RANGE, "segment_slots": slots * nreq,
            "scratch_bytes": L.chipq_read_scratch_len(ctypes.byref(info), nreq, RANGE, 0),
            "vouched_scratch_bytes": L.chipq_read_scratch_len(ctypes.byref(info), nreq, RANGE, 1),
            "host_planned_scratch_bytes": L.chipd_read_scratch_len(nreq, slots * nreq),
            "scan_workgroups_per_array": -(-(slots * nreq + 1) // 1024)}
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


class Planned:
    """The device-planned side of a read_bench.Set: the stream table, the
    requests as device tensors, slots of RANGE bytes."""

    def __init__(self, s):
        import torch
        from carbonado_amd import device as D
        self.s, self.D, self.torch = s, D, torch
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.table = D.stream_table(s.buf, s.in_off, s.in_len, s.hashes, s.pad, s.cl)
        self.table_host_ms = (time.perf_counter() - t0) * 1e3
        b.record()
        b.synchronize()
        self.table_ms = a.elapsed_time(b)
        dev = lambda x, dt: torch.from_numpy(x.astype(dt)).cuda()  # noqa: E731
        self.rs, self.start, self.rlen = dev(s.rs, "int32"), dev(s.start, "int64"), dev(s.rlen, "int64")
        n = s.nreq
        self.content = torch.zeros(n * RANGE, dtype=torch.uint8, device="cuda")
        self.clen = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.status = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.used = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.vouch = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.scratch = D.planned_read_scratch(self.table, n, RANGE, vouched=True)
        # the host-planned vouched call, beside read_bench's unvouched one
        self.v_scratch = D.vread_scratch(n, s.nseg)
        self.v_vouch = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.graph = None

    def planned(self):
        self.D.read_ranges_planned(self.table, self.rs, self.start, self.rlen, RANGE, self.content, RANGE, self.clen,
                                   self.status, self.used, self.scratch)

    def planned_vouched(self):
        self.D.read_ranges_vouched_planned(self.table, self.rs, self.start, self.rlen, RANGE, self.content, RANGE,
                                           self.clen, self.status, self.used, self.vouch, self.scratch)

    def host_vouched(self):
        from read_bench import ptr, vp
        s = self.s
        rc = s.L.chipv_read_ranges_dev(vp(s.buf), ptr(s.in_off), ptr(s.in_len), vp(s.hashes), ptr(s.pad), ptr(s.cl),
                                       s.count, ptr(s.rs), ptr(s.start), ptr(s.rlen), s.nreq, vp(s.content), ptr(s.coff),
                                       ptr(s.clen), vp(s.status), vp(s.used), vp(self.v_vouch), 0, vp(self.v_scratch),
                                       self.v_scratch.numel(), None)
        assert rc == 0, rc

    def capture(self):
        torch = self.torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            self.planned()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.planned()

    def replay(self):
        self.graph.replay()

    def want(self):
        """[nreq, RANGE]: every request's bytes of the clean objects"""
        torch, s = self.torch, self.s
        at = self.rs.to(torch.int64) * s.pitch + self.start
        return s.inp[at[:, None] + torch.arange(RANGE, device="cuda")[None, :]]

    def check(self):
        torch, s = self.torch, self.s
        want = self.want()
        # rebuilt: every range that meets its stream's damaged chunk (the one under its first range's first byte)
        import numpy as np
        first, last = s.start.astype(np.int64) // 1024, (s.start.astype(np.int64) + RANGE - 1) // 1024
        bad = np.full(s.count, -1, dtype=np.int64)
        bad[s.damaged] = first[np.array(s.damaged, dtype=np.int64) * s.per]
        mine = np.repeat(bad, s.per)
        hurt = torch.from_numpy((first <= mine) & (mine <= last)).cuda()
        for name, f in (("planned", self.planned), ("planned_vouched", self.planned_vouched), ("replay", self.replay)):
            self.content.fill_(0xA5); self.status.fill_(-1); self.used.fill_(-1); self.clen.fill_(-1)
            f()
            torch.cuda.synchronize()
            assert int(self.status.count_nonzero()) == 0 and bool((self.clen == RANGE).all()), name
            assert torch.equal(self.content.view(s.nreq, RANGE), want), name
            rebuilt = self.used.bitwise_and(0xF0) != 0  # a parity shard: the range was rebuilt
            assert torch.equal(rebuilt, hurt), name
            if name == "planned_vouched":
                assert torch.equal(self.vouch != 0, hurt) and int((self.vouch & 6).count_nonzero()) == 0
        for name, f in (("host", s.read), ("host_vouched", self.host_vouched)):
            s.content.fill_(0xA5); s.status.fill_(-1)
            f()
            torch.cuda.synchronize()
            assert int(s.status.count_nonzero()) == 0 and (s.clen == RANGE).all(), name
            got = s.content[torch.from_numpy(s.coff.astype("int64")).cuda()[:, None] +
                            torch.arange(RANGE, device="cuda")[None, :]]
            assert torch.equal(got, want), name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry", action="store_true", help="no device: sizes and launch geometry only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "qread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)
    import torch
    from bench import ClockSampler
    from carbonado_amd import _lib
    from read_bench import Set
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "qread_bench", "level": 12, "seed": args.seed, "streams": args.streams, "object_bytes": OBJ - 41,
           "range_bytes": RANGE, "reps": args.reps, "launches": LAUNCHES,
           "timing": "HIP events around each call, host_*_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    for per in (1, 16):
        for every in (0, 64):
            s = Set(L, args.streams, per, every, args.seed + per + every)
            p = Planned(s)
            p.capture()
            p.check()
            r = {"requests": s.nreq, "segments": int(s.nseg), "damaged": len(s.damaged),
                 "stream_table": {"ms": round(p.table_ms, 4), "host_ms": round(p.table_host_ms, 4),
                                  "bytes": p.table.table.numel()},
                 **time_forms({"planned": p.planned, "host": s.read, "planned_vouched": p.planned_vouched,
                               "host_vouched": p.host_vouched, "replay": p.replay}, args.reps)}
            r["planned_over_host"] = round(r["planned"]["median_ms"] / r["host"]["median_ms"], 3)
            r["planned_vouched_over_host_vouched"] = round(r["planned_vouched"]["median_ms"] /
                                                           r["host_vouched"]["median_ms"], 3)
            res[f"read_{per}_" + ("damaged_1_in_64" if every else "intact")] = r
            del s, p
            torch.cuda.empty_cache()
    res["clocks"] = clocks.stop()
    res["planned_below_host_at_16"] = all(
        res[k]["planned"]["median_ms"] < res[k]["host"]["median_ms"] for k in res if k.startswith("read_16_"))
    res["planned_within_host_spread_at_1"] = all(
        res[k]["planned"]["median_ms"] - res[k]["host"]["median_ms"] <= res[k]["host"]["max_ms"] - res[k]["host"]["min_ms"]
        for k in res if k.startswith("read_1_"))
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
