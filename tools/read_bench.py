#!/usr/bin/env python3
"""Byte-range reads of device-resident level-12 (Zfec|Bao) streams: one
chipd_read_ranges_dev call (include/carbonado_hip_read.h) against what a caller
had before it (GPU only; not bench.py).

The set: --streams streams of 1 MiB objects in one buffer, one random 4 KiB
object range per stream (and, for the planner and upload cost, 16 per stream).

  intact    read            chipd_read_ranges_dev
            verify_windows  chipa_verify_slices_dev over the same chunk windows
                            of the primaries (one request per segment): the
                            same hashing, so the difference is the gated
                            fallback items and the byte-granular gather
            full_decode     chipx_decode_ragged_dev of all streams
  damaged   1 stream in 64 with a flipped bit in a primary chunk inside its
            range:
            read            the same call; the damaged ranges are rebuilt
            scrub_verify    chipr_scrub_ragged_dev into a second buffer, then
                            chipa_verify_slices_dev (repaired streams read
                            there): the sequence a caller had
  sixteen   read / verify_windows with 16 ranges per stream

Before anything is timed every form's bytes are compared with the clean
objects.  A time is between two HIP events around the call (the calls are not
synchronised; scrub synchronises itself); `host_ms` is the host clock around
the same call, that is planning, upload and enqueue.  3 warm-ups, the forms
alternating within one process for --reps rounds; medians and min-max in ms, the
GPU's clocks sampled meanwhile.  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import ClockSampler  # noqa: E402
from carbonado_amd import _lib  # noqa: E402
from carbonado_amd import device as D  # noqa: E402

LEVEL = 12
OBJ = 1 << 20
RANGE = 4096
SO = D.STREAM_OFFSET


def ptr(a):
    return a.ctypes.data_as(_lib.c_u64p if a.dtype == np.uint64 else _lib.c_u32p)


def vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def chunk_off(i, N):
    """Stream offset of chunk i of a bao stream of N full chunks (pre-order)."""
    off, lo, cnt = 8, 0, N
    while cnt > 1:
        off += 64
        left = 1 << ((cnt - 1).bit_length() - 1)
        if i < lo + left:
            cnt = left
        else:
            off += left * 1024 + 64 * (left - 1)
            lo, cnt = lo + left, cnt - left
    return off


class Set:
    """--streams objects of OBJ - 41 bytes encoded at level 12 into the first
    half of one buffer (each stream SO bytes into a row of 256-B multiple
    pitch; the second half takes scrub's output), `per` ranges per stream,
    every `every`-th stream (0: none) damaged inside its first range."""

    def __init__(self, L, count, per, every, seed):
        self.L, self.count, self.per = L, count, per
        sizes = [OBJ - 41] * count
        pitch = OBJ
        torch.manual_seed(seed)
        self.inp = torch.randint(0, 256, (count * pitch,), dtype=torch.uint8, device="cuda")
        in_off = [o * pitch for o in range(count)]
        self.off, self.len, self.half = D.ragged_layout(LEVEL, sizes, 256, SO)
        self.buf = torch.zeros(2 * self.half, dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((count, 32), dtype=torch.uint8, device="cuda")
        _, infos = D.encode_ragged(LEVEL, self.inp, in_off, sizes, self.buf, self.off, self.hashes,
                                   D.ragged_scratch(LEVEL, sizes))
        torch.cuda.synchronize()
        self.pad = np.array([i.padding_len for i in infos], dtype=np.uint32)
        self.cl = np.array([i.chunk_len for i in infos], dtype=np.uint32)
        C, spc = int(self.cl[0]), int(self.cl[0]) // 1024
        n_obj = 4 * C - int(self.pad[0])
        assert n_obj == sizes[0]
        rng = np.random.default_rng(seed)
        self.rs = np.repeat(np.arange(count, dtype=np.uint32), per)
        self.start = rng.integers(0, n_obj - RANGE, count * per).astype(np.uint64)
        self.rlen = np.full(count * per, RANGE, dtype=np.uint64)
        self.nreq = count * per
        self.in_off = np.array(self.off, dtype=np.uint64)
        self.in_len = np.array(self.len, dtype=np.uint64)
        # damage: a bit of the primary chunk holding the first range's first byte
        self.damaged = list(range(0, count, every)) if every else []
        if self.damaged:
            at = []
            for k, j in enumerate(self.damaged):
                x = int(self.start[j * per])
                at.append(self.off[j] + chunk_off(x // C * spc + x % C // 1024, 8 * spc) + 17 * k % 1024)
            self.buf[torch.tensor(at, dtype=torch.int64, device="cuda")] ^= 0x10
        # the read call
        coff, clen, ctotal, nseg = D.read_layout(self.cl, self.pad, self.rs, self.start, self.rlen, 16)
        self.coff = np.array(coff, dtype=np.uint64)
        self.clen = np.zeros(self.nreq, dtype=np.uint64)
        self.content = torch.zeros(ctotal + 16, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(self.nreq, dtype=torch.int32, device="cuda")
        self.used = torch.zeros(self.nreq, dtype=torch.int32, device="cuda")
        self.nseg = nseg
        self.scratch = D.read_scratch(self.nreq, nseg)
        # the same chunk windows as slice requests, one per segment
        seg_rs, idx, cnt, self.seg_of = [], [], [], []
        for r in range(self.nreq):
            x, end = int(self.start[r]), int(self.start[r]) + RANGE
            while x < end:
                p = x // C
                stop = min(end, (p + 1) * C)
                w0, w1 = (x - p * C) // 1024, -(-(stop - p * C) // 1024)
                seg_rs.append(self.rs[r]); idx.append(p * spc + w0); cnt.append(w1 - w0)
                self.seg_of.append((r, x - int(self.start[r]), (x - p * C) % 1024, stop - x))
                x = stop
        assert len(idx) == nseg
        self.v_rs = np.array(seg_rs, dtype=np.uint32)
        self.v_idx, self.v_cnt = np.array(idx, dtype=np.uint64), np.array(cnt, dtype=np.uint64)
        _, _, vcoff, _, _, vtotal = D.slice_layout(np.full(nseg, 8 * C, dtype=np.uint64), self.v_idx, self.v_cnt, 16)
        self.v_coff = np.array(vcoff, dtype=np.uint64)
        self.v_clen = np.zeros(nseg, dtype=np.uint64)
        self.v_content = torch.zeros(vtotal + 16, dtype=torch.uint8, device="cuda")
        self.v_status = torch.zeros(nseg, dtype=torch.int32, device="cuda")
        self.v_scratch = D.audit_scratch(count, nseg)
        # after a scrub into the second half, a repaired stream is read there
        self.v_in_off = self.in_off.copy()
        if self.damaged:
            self.v_in_off[self.damaged] += np.uint64(self.half)
        # the full decode
        self.d_off = np.arange(count, dtype=np.uint64) * np.uint64(pitch)
        self.d_len = np.zeros(count, dtype=np.uint64)
        self.d_out = torch.zeros(count * pitch, dtype=torch.uint8, device="cuda")
        self.d_status = torch.zeros(count, dtype=torch.int32, device="cuda")
        self.d_scratch = D.ragged_scratch(LEVEL, self.len, decode=True)
        # the scrub
        self.s_scratch_len = L.chipr_scrub_ragged_scratch_len(ptr(self.in_len), count, max(1, len(self.damaged)))
        self.s_scratch = torch.zeros(self.s_scratch_len, dtype=torch.uint8, device="cuda")
        self.s_status = np.zeros(count, dtype=np.int32)
        self.pitch, self.n_obj = pitch, n_obj

    def read(self):
        rc = self.L.chipd_read_ranges_dev(vp(self.buf), ptr(self.in_off), ptr(self.in_len), vp(self.hashes), ptr(self.pad),
                                          ptr(self.cl), self.count, ptr(self.rs), ptr(self.start), ptr(self.rlen),
                                          self.nreq, vp(self.content), ptr(self.coff), ptr(self.clen), vp(self.status),
                                          vp(self.used), vp(self.scratch), self.scratch.numel(), None)
        assert rc == 0, rc

    def _verify(self, in_off):
        rc = self.L.chipa_verify_slices_dev(vp(self.buf), ptr(in_off), ptr(self.in_len), vp(self.hashes), self.count,
                                            ptr(self.v_rs), ptr(self.v_idx), ptr(self.v_cnt), self.nseg,
                                            vp(self.v_content), ptr(self.v_coff), ptr(self.v_clen), vp(self.v_status),
                                            vp(self.v_scratch), None)
        assert rc == 0, rc

    def verify_windows(self):
        self._verify(self.in_off)

    def full_decode(self):
        rc = self.L.chipx_decode_ragged_dev(LEVEL, vp(self.buf), ptr(self.in_off), ptr(self.in_len), self.count,
                                            vp(self.hashes), ptr(self.pad), vp(self.d_out), ptr(self.d_off),
                                            ptr(self.d_len), vp(self.d_status), vp(self.d_scratch), None)
        assert rc == 0, rc

    def scrub_verify(self):
        rc = self.L.chipr_scrub_ragged_dev(vp(self.buf), ptr(self.in_off), ptr(self.in_len), self.count, vp(self.hashes),
                                           ptr(self.pad), ptr(self.cl), vp(self.buf, self.half), ptr(self.in_off),
                                           self.s_status.ctypes.data_as(ctypes.c_void_p), vp(self.s_scratch),
                                           self.s_scratch_len, None)
        assert rc == 0, rc
        self._verify(self.v_in_off)

    # ---- every form's bytes against the clean objects ------------------------------
    def _want(self, r):
        o = int(self.rs[r]) * self.pitch + int(self.start[r])
        return self.inp[o:o + RANGE]

    def check_read(self, sample):
        self.content.fill_(0xA5); self.status.fill_(-1); self.used.fill_(-1)
        self.read()
        torch.cuda.synchronize()
        assert int(self.status.count_nonzero()) == 0 and (self.clen == RANGE).all()
        used, hurt, rebuilt = self.used.cpu().numpy(), set(self.damaged), 0
        for r in range(self.nreq):  # copied from its own primaries, unless the damage is in its range
            p = int(self.start[r]) // int(self.cl[0])
            hit = r % self.per == 0 and r // self.per in hurt
            assert (int(used[r]) in (1 << p, 3 << p)) != hit, (r, int(used[r]))
            rebuilt += hit
        for r in sample:
            assert torch.equal(self.content[int(self.coff[r]):int(self.coff[r]) + RANGE], self._want(r)), ("read", r)
        return rebuilt

    def check_verify(self, sample_segs, fn):
        self.v_content.fill_(0xA5); self.v_status.fill_(-1)
        fn()
        torch.cuda.synchronize()
        assert int(self.v_status.count_nonzero()) == 0
        for g in sample_segs:
            r, at, skip, n = self.seg_of[g]
            o = int(self.v_coff[g]) + skip
            assert torch.equal(self.v_content[o:o + n], self._want(r)[at:at + n]), ("verify", g)

    def check_decode(self):
        self.d_out.fill_(0xA5); self.d_status.fill_(-1)
        self.full_decode()
        torch.cuda.synchronize()
        assert int(self.d_status.count_nonzero()) == 0 and (self.d_len == self.n_obj).all()
        got, want = self.d_out.view(self.count, self.pitch), self.inp.view(self.count, self.pitch)
        assert torch.equal(got[:, :self.n_obj], want[:, :self.n_obj])


def time_forms(forms, reps):
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
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "host_median_ms": round(statistics.median(host[k]), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "read_bench_mi355x.json"))
    args = ap.parse_args()
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "read_bench", "level": LEVEL, "seed": args.seed, "streams": args.streams, "object_bytes": OBJ - 41,
           "range_bytes": RANGE, "reps": args.reps,
           "timing": "HIP events around each call, host_median_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams

    s = Set(L, S, 1, 0, args.seed)
    sample = range(0, s.nreq, max(1, s.nreq // 256))
    assert s.check_read(sample) == 0
    s.check_verify(range(0, s.nseg, max(1, s.nseg // 256)), s.verify_windows)
    s.check_decode()
    r = res["intact"] = {"requests": s.nreq, "segments": int(s.nseg), "stream_GiB": round(sum(s.len) / (1 << 30), 3),
                         **time_forms({"read": s.read, "verify_windows": s.verify_windows,
                                       "full_decode": s.full_decode}, args.reps)}
    r["read_over_verify_windows"] = round(r["read"]["median_ms"] / r["verify_windows"]["median_ms"], 3)
    r["full_decode_over_read"] = round(r["full_decode"]["median_ms"] / r["read"]["median_ms"], 2)
    del s
    torch.cuda.empty_cache()

    s = Set(L, S, 1, 64, args.seed + 1)
    sample = sorted(set(range(0, s.nreq, max(1, s.nreq // 128))) | set(s.damaged))
    assert s.check_read(sample) == len(s.damaged)
    picked, hurt = set(sample), set(s.damaged)
    segs = [g for g, (rq, _, _, _) in enumerate(s.seg_of) if rq in picked]
    s.check_verify(segs, s.scrub_verify)
    assert [int(x) for x in s.s_status] == [0 if j in hurt else 12 for j in range(S)]
    r = res["damaged_1_in_64"] = {"requests": s.nreq, "damaged": len(s.damaged),
                                  **time_forms({"read": s.read, "scrub_verify": s.scrub_verify}, args.reps)}
    r["scrub_verify_over_read"] = round(r["scrub_verify"]["median_ms"] / r["read"]["median_ms"], 2)
    del s
    torch.cuda.empty_cache()

    s = Set(L, S, 16, 0, args.seed + 2)
    assert s.check_read(range(0, s.nreq, max(1, s.nreq // 256))) == 0
    s.check_verify(range(0, s.nseg, max(1, s.nseg // 256)), s.verify_windows)
    r = res["sixteen_per_stream"] = {"requests": s.nreq, "segments": int(s.nseg),
                                     **time_forms({"read": s.read, "verify_windows": s.verify_windows}, args.reps)}
    r["read_over_verify_windows"] = round(r["read"]["median_ms"] / r["verify_windows"]["median_ms"], 3)
    del s

    res["clocks"] = clocks.stop()
    res["intact_read_beats_full_decode"] = res["intact"]["full_decode_over_read"] > 1
    res["damaged_read_beats_scrub_verify"] = res["damaged_1_in_64"]["scrub_verify_over_read"] > 1
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
