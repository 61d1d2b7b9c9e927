#!/usr/bin/env python3
"""Scrubbing device-resident level-12 (Zfec|Bao) streams of mixed sizes: the
uniform entry point a caller has today against one ragged call
(include/carbonado_hip_repair.h).

Two sets of streams, each resident in one buffer:

  tails  the tails of --files files of a seeded random length in [1, 16] MiB
         cut into 1 MiB segments (tools/ragged_bench.py's archive), 1 in 4 of
         them with a flipped bit in one shard;
  equal  --equal streams of 1 MiB objects, 1 in 64 damaged.

Two forms over the same damaged streams and hashes:

  uniform  chip_scrub_batch_dev: one call per distinct size (tails), one call
           for the whole set (equal);
  ragged   one chipr_scrub_ragged_dev call, its scratch sized to repair the
           damaged streams in one pass.

Before anything is timed both forms' statuses are compared (0 for the damaged
streams, 12 for the others) and every repaired stream with the clean encoding.
Both calls are synchronous, so a time is the host clock around the call; 3
warm-ups, the forms alternating within one process for --reps rounds; medians
and min-max in ms, the GPU's clocks sampled meanwhile.  Prints one JSON line
(and writes it to --out).
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
SEG = 1 << 20
SO = D.STREAM_OFFSET


def u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])


def u32(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*[int(x) for x in xs])


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
    """Objects of `sizes` bytes encoded at level 12 into one buffer (each
    stream SO bytes into a row of 256-B multiple pitch), every `every`-th
    stream damaged in one shard, and the buffers both forms need."""

    def __init__(self, L, sizes, every, seed):
        self.L, self.sizes, self.count = L, list(sizes), len(sizes)
        in_off, cur = [], 0
        for n in self.sizes:
            in_off.append(cur)
            cur += (n + 255) // 256 * 256
        torch.manual_seed(seed)
        inp = torch.randint(0, 256, (cur + 256,), dtype=torch.uint8, device="cuda")
        self.off, self.len, total = D.ragged_layout(LEVEL, self.sizes, 256, SO)
        self.clean = torch.zeros(total, dtype=torch.uint8, device="cuda")
        self.hashes = torch.zeros((self.count, 32), dtype=torch.uint8, device="cuda")
        _, infos = D.encode_ragged(LEVEL, inp, in_off, self.sizes, self.clean, self.off, self.hashes,
                                   D.ragged_scratch(LEVEL, self.sizes))
        torch.cuda.synchronize()
        del inp
        self.pad = [i.padding_len for i in infos]
        self.cl = [i.chunk_len for i in infos]
        self.damaged = list(range(0, self.count, every))
        flips = []
        for k, j in enumerate(self.damaged):
            spc = self.cl[j] // 1024
            flips.append(self.off[j] + chunk_off((k % 8) * spc + k % spc, 8 * spc) + 17 * k % 1024)
        self.bad = self.clean.clone()
        at = torch.tensor(flips, dtype=torch.int64, device="cuda")
        self.bad[at] ^= 0x10
        self.out = torch.zeros_like(self.clean)
        self.want = np.full(self.count, 12, dtype=np.int32)
        self.want[self.damaged] = 0
        # the uniform form: one call per distinct size, the streams of a size at one stride
        self.groups = {}
        for j, ln in enumerate(self.len):  # one EncodeInfo per uniform call: same length and padding
            self.groups.setdefault((ln, self.pad[j]), []).append(j)
        self.uni = []
        for (ln, _), js in self.groups.items():
            stride = self.off[js[1]] - self.off[js[0]] if len(js) > 1 else ln
            rows = all(b == a + 1 and self.off[b] - self.off[a] == stride for a, b in zip(js, js[1:]))
            if rows:  # neighbours at one stride: a batch
                self.uni.append((js[0], len(js), ln, stride))
            else:     # two tails that happen to be equal, apart in the buffer: a call each
                self.uni += [(j, 1, ln, ln) for j in js]
        s_uni = max(L.chip_scrub_scratch_len(ln, cnt) for _, cnt, ln, _ in self.uni)
        s_rag = L.chipr_scrub_ragged_scratch_len(u64(self.len), self.count, len(self.damaged))
        self.scratch = torch.zeros(max(s_uni, s_rag), dtype=torch.uint8, device="cuda")
        self.rag_scratch_len = s_rag
        self.status = np.zeros(self.count, dtype=np.int32)
        self._off, self._len = u64(self.off), u64(self.len)
        self._pad, self._cl = u32(self.pad), u32(self.cl)
        self.stream_bytes = sum(self.len)
        self.damaged_bytes = sum(self.len[j] for j in self.damaged)

    def uniform(self):
        st = self.status.ctypes.data
        for j0, cnt, ln, stride in self.uni:
            rc = self.L.chip_scrub_batch_dev(vp(self.bad, self.off[j0]), stride, ln, cnt, vp(self.hashes, 32 * j0),
                                             self.pad[j0], self.cl[j0], vp(self.out, self.off[j0]), stride,
                                             ctypes.c_void_p(st + 4 * j0), vp(self.scratch), None)
            assert rc == 0, rc

    def ragged(self):
        rc = self.L.chipr_scrub_ragged_dev(vp(self.bad), self._off, self._len, self.count, vp(self.hashes), self._pad,
                                           self._cl, vp(self.out), self._off, self.status.ctypes.data_as(ctypes.c_void_p),
                                           vp(self.scratch), self.rag_scratch_len, None)
        assert rc == 0, rc

    def forms(self):
        return {"uniform": self.uniform, "ragged": self.ragged}

    def check(self):
        for name, f in self.forms().items():
            self.out.zero_()
            self.status[:] = -1
            f()
            torch.cuda.synchronize()
            assert np.array_equal(self.status, self.want), (name, "statuses")
            for j in self.damaged:
                a, b = self.off[j], self.off[j] + self.len[j]
                assert torch.equal(self.out[a:b], self.clean[a:b]), (name, j, "repaired stream differs")
            assert int(self.out.count_nonzero()) <= self.damaged_bytes, (name, "bytes outside the repaired ranges")


def time_forms(forms, reps):
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()  # synchronous: returns with the statuses on the host
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, v in ms.items():
        out[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return out


def measure(s, reps, res, name):
    s.check()
    res[name] = {"streams": s.count, "distinct_object_sizes": len(set(s.sizes)),
                 "distinct_stream_lengths": len(set(s.len)), "uniform_calls": len(s.uni),
                 "damaged": len(s.damaged), "stream_GiB": round(s.stream_bytes / (1 << 30), 3),
                 "damaged_MiB": round(s.damaged_bytes / (1 << 20), 2), "ragged_scratch_MiB":
                 round(s.rag_scratch_len / (1 << 20), 2), **time_forms(s.forms(), reps)}
    r = res[name]
    r["ragged_over_uniform"] = round(r["ragged"]["median_ms"] / r["uniform"]["median_ms"], 3)
    r["ragged_GiBps_streams"] = round(s.stream_bytes / (r["ragged"]["median_ms"] * 1e-3) / (1 << 30), 2)
    r["uniform_GiBps_streams"] = round(s.stream_bytes / (r["uniform"]["median_ms"] * 1e-3) / (1 << 30), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--equal", type=int, default=2048, help="streams of the equal-size set (0: skip it)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    rng = np.random.default_rng(args.seed)
    lengths = rng.integers(1 << 20, (16 << 20) + 1, args.files)
    tails = [int(x) % SEG for x in lengths if int(x) % SEG]
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "scrub_ragged_bench", "level": LEVEL, "seed": args.seed, "files": args.files, "reps": args.reps,
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    measure(Set(L, tails, 4, args.seed), args.reps, res, "tails")
    torch.cuda.empty_cache()
    if args.equal:
        measure(Set(L, [SEG] * args.equal, 64, args.seed + 1), args.reps, res, "equal")
    res["clocks"] = clocks.stop()
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
