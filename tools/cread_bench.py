#!/usr/bin/env python3
"""Plaintext byte-range reads of device-resident level-13 (Ecies|Zfec|Bao)
streams: chipc_read_ranges_dev with the keys in hand, chipc_stream_keys_dev,
and the two together (include/carbonado_hip_cread.h), against the hashing floor
and against the only way to plaintext before them (GPU only; not bench.py).
The sets and the box discipline are those of tools/vread_bench.py: --streams
streams whose envelopes have 1 MiB - 41 bytes (the objects of the other read
tools; the plaintexts are 97 bytes shorter) in one buffer, one random 4 KiB
plaintext range per stream, once intact and once with 1 stream in 64 damaged
inside its range.

  read_plain     chipc_read_ranges_dev, keys, nonces and key status in hand
  stream_keys    chipc_stream_keys_dev (waits once for the header bytes; one
                 key agreement per stream on the host)
  keys_and_read  the two together
  vread          chipv_read_ranges_dev of the same windows (envelope bytes
                 97 + start): the hashing floor, ciphertext out
  decode         chipe_decode_ragged_dev of the same streams: whole objects,
                 tags checked; a damaged stream fails it (status 5)

Before anything is timed the plaintext reads are compared with the objects,
and the damaged reads must come out status 0, vouch 1, all others vouch 0.
Timing as in read_bench.py: HIP events around each call, the forms alternating
within one process for --reps rounds after 3 warm-ups, medians and min-max in
ms (host_median_ms is the host clock around the same call; stream_keys waits
inside the call, so its two medians agree).  Prints one JSON line (and writes
it to --out).

--dry needs no device: it lays out the request set on the host
(chipc_read_layout, the scratch lengths) and prints the sizes."""
import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

LEVEL = 13
ENV = (1 << 20) - 41        # the envelope: the object of the level-12 read tools
PLAIN = ENV - 97
RANGE = 4096
SECRET = bytes(range(1, 33))
CASES = (("intact", 0, 0), ("damaged_1_in_64", 64, 1))  # name, every, seed +


def requests(count, seed):
    rng = np.random.default_rng(seed)
    rs = np.arange(count, dtype=np.uint32)
    start = rng.integers(0, PLAIN - RANGE, count).astype(np.uint64)
    return rs, start, np.full(count, RANGE, dtype=np.uint64)


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    count, C, pad = args.streams, (1 << 20) // 4, 41
    rs, start, rlen = requests(count, args.seed)
    cl, pd = np.full(count, C, dtype=np.uint32), np.full(count, pad, dtype=np.uint32)
    off, ln = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
    total, nseg = ctypes.c_uint64(), ctypes.c_uint64()
    p32, p64 = (lambda a: a.ctypes.data_as(_lib.c_u32p)), (lambda a: a.ctypes.data_as(_lib.c_u64p))
    rc = L.chipc_read_layout(p32(cl), p32(pd), count, p32(rs), p64(start), p64(rlen), count, 16, p64(off), p64(ln),
                             ctypes.byref(total), ctypes.byref(nseg))
    assert rc == 0 and (ln == RANGE).all() and total.value == RANGE * count
    res = {"tool": "cread_bench", "dry_run": True, "level": LEVEL, "seed": args.seed, "streams": count,
           "object_bytes": PLAIN, "range_bytes": RANGE, "reps": args.reps, "requests": count, "segments": nseg.value,
           "damaged_streams": len(range(0, count, 64)),
           "read_scratch_bytes": L.chipc_read_scratch_len(count, nseg.value, count),
           "vread_scratch_bytes": L.chipv_read_scratch_len(count, nseg.value),
           "keys_scratch_bytes": L.chipc_stream_keys_scratch_len(count),
           "launches": {"vouched_read": 8, "keystream": 2}}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dry", action="store_true", help="no device: lay the request set out on the host")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)

    import torch

    import read_bench as RB
    from bench import ClockSampler
    from carbonado_amd import _lib
    from carbonado_amd import device as D
    from oracle import oracle as O

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "cread_bench", "level": LEVEL, "seed": args.seed, "streams": args.streams, "object_bytes": PLAIN,
           "range_bytes": RANGE, "reps": args.reps,
           "timing": "HIP events around each call, host_median_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams
    pub = O.c_public_key(SECRET)
    sizes, pitch = [PLAIN] * S, 1 << 20
    in_off = [o * pitch for o in range(S)]
    off, slen, total = D.ragged_layout(12, [ENV] * S, 256)

    for name, every, ds in CASES:
        torch.manual_seed(args.seed + ds)
        inp = torch.randint(0, 256, (S * pitch,), dtype=torch.uint8, device="cuda")
        buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
        hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
        olen, infos = D.encode_ragged_ecies(LEVEL, pub, inp, in_off, sizes, buf, off, hashes,
                                            D.ecies_ragged_scratch(LEVEL, sizes))
        torch.cuda.synchronize()
        pad, cl = [i.padding_len for i in infos], [i.chunk_len for i in infos]
        C, spc = cl[0], cl[0] // 1024
        rs, start, rlen = requests(S, args.seed + ds)
        damaged = list(range(0, S, every)) if every else []
        if damaged:  # a bit of the primary chunk that holds the range's first byte
            at = []
            for k, j in enumerate(damaged):
                x = int(start[j]) + 97
                at.append(off[j] + RB.chunk_off(x // C * spc + x % C // 1024, 8 * spc) + 17 * k % 1024)
            buf[torch.tensor(at, dtype=torch.int64, device="cuda")] ^= 0x10
        coff, clen, ctotal, nseg = D.plain_read_layout(cl, pad, rs, start, rlen)
        content = torch.zeros(ctotal + 16, dtype=torch.uint8, device="cuda")
        vcontent = torch.zeros(ctotal + 16, dtype=torch.uint8, device="cuda")
        status, used, vouch = (torch.zeros(S, dtype=torch.int32, device="cuda") for _ in range(3))
        rscratch, vscratch = D.plain_read_scratch(S, nseg, S), D.vread_scratch(S, nseg)
        kscratch = D.stream_keys_scratch(S)
        vstart = start + np.uint64(97)
        d_out = torch.zeros(S * pitch, dtype=torch.uint8, device="cuda")
        d_status = torch.zeros(S, dtype=torch.int32, device="cuda")
        d_scratch = D.ecies_ragged_scratch(LEVEL, olen, decode=True)
        # the timed forms call the library as a store would: arrays converted once, no wrapper in between
        a64, a32 = (lambda x: np.ascontiguousarray(x, dtype=np.uint64)), (lambda x: np.ascontiguousarray(x, dtype=np.uint32))
        n_off, n_len, n_pad, n_cl, n_coff, n_clen = a64(off), a64(olen), a32(pad), a32(cl), a64(coff), a64(clen)
        ptr, vp = RB.ptr, RB.vp
        p8 = lambda a: a.ctypes.data_as(_lib.c_u8p)  # noqa: E731
        keys, ivs = np.zeros((S, 32), dtype=np.uint8), np.zeros((S, 16), dtype=np.uint8)
        kstat = np.zeros(S, dtype=np.uint32)

        def stream_keys():
            rc = L.chipc_stream_keys_dev(SECRET, 32, vp(buf), ptr(n_off), ptr(n_len), vp(hashes), ptr(n_pad), ptr(n_cl), S,
                                         p8(keys), p8(ivs), ptr(kstat), vp(kscratch), kscratch.numel(), None)
            assert rc == 0, rc

        def read_plain():
            rc = L.chipc_read_ranges_dev(p8(keys), p8(ivs), ptr(kstat), vp(buf), ptr(n_off), ptr(n_len), vp(hashes),
                                         ptr(n_pad), ptr(n_cl), S, ptr(rs), ptr(start), ptr(rlen), S, vp(content),
                                         ptr(n_coff), ptr(n_clen), vp(status), vp(used), vp(vouch), 0, vp(rscratch),
                                         rscratch.numel(), None)
            assert rc == 0, rc

        def keys_and_read():
            stream_keys()
            read_plain()

        def vread():
            rc = L.chipv_read_ranges_dev(vp(buf), ptr(n_off), ptr(n_len), vp(hashes), ptr(n_pad), ptr(n_cl), S, ptr(rs),
                                         ptr(vstart), ptr(rlen), S, vp(vcontent), ptr(n_coff), ptr(n_clen), vp(status),
                                         vp(used), vp(vouch), 0, vp(vscratch), vscratch.numel(), None)
            assert rc == 0, rc

        def decode():
            D.decode_ragged_ecies(LEVEL, SECRET, buf, off, olen, hashes, pad, d_out, in_off, d_status, d_scratch)

        # every plaintext read against the objects, the damaged ones rebuilt and vouched for
        stream_keys()
        assert not kstat.any()
        content.fill_(0xA5)
        read_plain()
        torch.cuda.synchronize()
        assert int(status.count_nonzero()) == 0
        assert vouch.cpu().tolist() == [1 if j in set(damaged) else 0 for j in range(S)]
        for r in sorted(set(range(0, S, max(1, S // 256))) | set(damaged)):
            o = r * pitch + int(start[r])
            assert torch.equal(content[coff[r]:coff[r] + RANGE], inp[o:o + RANGE]), ("read_plain", r)
        decode()
        torch.cuda.synchronize()
        failed = int(d_status.count_nonzero())
        assert failed == len(damaged)

        r = res[name] = {"requests": S, "segments": int(nseg), "damaged": len(damaged), "decode_failed_streams": failed,
                         **RB.time_forms({"read_plain": read_plain, "vread": vread, "stream_keys": stream_keys,
                                          "keys_and_read": keys_and_read, "decode": decode}, args.reps)}
        r["decode_over_read_plain"] = round(r["decode"]["median_ms"] / r["read_plain"]["median_ms"], 2)
        r["decode_over_keys_and_read"] = round(r["decode"]["median_ms"] / r["keys_and_read"]["median_ms"], 2)
        r["read_plain_over_vread"] = round(r["read_plain"]["median_ms"] / r["vread"]["median_ms"], 3)
        r["read_plain_minus_vread_ms"] = round(r["read_plain"]["median_ms"] - r["vread"]["median_ms"], 4)
        r["stream_keys_share_of_both"] = round(r["stream_keys"]["median_ms"] / r["keys_and_read"]["median_ms"], 3)
        del inp, buf, content, vcontent, d_out, d_scratch, rscratch, vscratch, kscratch
        torch.cuda.empty_cache()

    res["clocks"] = clocks.stop()
    res["read_plain_beats_decode"] = all(res[name]["decode_over_read_plain"] > 1 for name, _, _ in CASES)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
