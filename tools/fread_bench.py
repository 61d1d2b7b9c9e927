#!/usr/bin/env python3
"""Plaintext byte-range reads of device-resident level-14 (Snappy|Zfec|Bao) and
level-15 (Snappy|Ecies|Zfec|Bao) streams: chipf_read_ranges_dev with the frame
index in hand and chipf_frame_index_dev (include/carbonado_hip_fread.h), against
the only way to a plaintext byte before them, chips_decode_ragged_dev of the
whole streams, in the same run (GPU only; not bench.py).

Sets: --streams streams of 1 MiB objects at 14 and at 15, each on the two
corpora of tools/snap_bench.py (mix40: every chunk compressed, about 3:1;
random: every chunk stored raw; 8 distinct objects repeated over the set).
Requests: one random 4 KiB plaintext range per stream, and 16 per stream.

  read_1         chipf_read_ranges_dev, one range per stream, index and keys in hand
  read_16        the same with 16 ranges per stream
  frame_index    chipf_frame_index_dev (waits twice; a once-per-object cost)
  decode         chips_decode_ragged_dev of the same streams: the reference point

Before anything is timed the index must be proven for every stream and the
reads are compared with the objects.  Timing as in read_bench.py: HIP events
around each call, the forms alternating within one process for --reps rounds
after 3 warm-ups, medians and min-max in ms.  Prints one JSON line (and writes
it to --out); read_beats_decode says whether both reads beat the decode in
every cell.

--dry needs no device: it lays a request set over the index every random 1 MiB
object has (16 raw chunks) on the host and prints the sizes."""
import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

SEG = 1 << 20
RANGE = 4096
FRAME = 65536
SECRET = bytes(range(1, 33))
CORPORA = ("mix40", "random")
LAUNCHES = {"vouched_read": 8, "keystream": 2, "block": 1, "finish": 1, "walk": 1, "chain": 1}


def requests(count, per, seed):
    rng = np.random.default_rng(seed)
    rs = np.repeat(np.arange(count, dtype=np.uint32), per)
    start = rng.integers(0, SEG - RANGE, count * per).astype(np.uint64)
    return rs, start, np.full(count * per, RANGE, dtype=np.uint64)


def layout(L, fmt, cl, pad, frame_off, idx_off, nframes, plain, rs, start, rlen):
    """(content_off, content_len, content_total, nseg, stage_total, vseg) through the library, arrays as given"""
    from carbonado_amd import _lib
    p32, p64 = (lambda a: a.ctypes.data_as(_lib.c_u32p)), (lambda a: a.ctypes.data_as(_lib.c_u64p))
    nreq = rs.size
    off, ln = np.zeros(nreq, dtype=np.uint64), np.zeros(nreq, dtype=np.uint64)
    total, nseg, stage, vseg = (ctypes.c_uint64() for _ in range(4))
    rc = L.chipf_read_layout(fmt, p32(cl), p32(pad), None, p64(frame_off), p64(idx_off), p64(nframes), p64(plain),
                             cl.size, p32(rs), p64(start), p64(rlen), nreq, 16, p64(off), p64(ln), ctypes.byref(total),
                             ctypes.byref(nseg), ctypes.byref(stage), ctypes.byref(vseg))
    assert rc == 0, rc
    return off, ln, total.value, nseg.value, stage.value, vseg.value


def dry_run(args):
    from carbonado_amd import _lib
    L = _lib.lib()
    S = args.streams
    frames = SEG // FRAME
    flen = 10 + frames * (FRAME + 8)            # a random object's frame stream: 16 raw chunks
    pad, chunk = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.chip_calc_padding_len(flen, 4, ctypes.byref(pad), ctypes.byref(chunk)) == 0
    cl, pd = np.full(S, chunk.value, dtype=np.uint32), np.full(S, pad.value, dtype=np.uint32)
    one = np.array([10 + f * (FRAME + 8) for f in range(frames)] + [flen], dtype=np.uint64)
    frame_off = np.tile(one, S)
    idx_off = np.arange(S, dtype=np.uint64) * np.uint64(frames + 1)
    nframes, plain = np.full(S, frames, dtype=np.uint64), np.full(S, SEG, dtype=np.uint64)
    res = {"tool": "fread_bench", "dry_run": True, "seed": args.seed, "streams": S, "object_bytes": SEG,
           "range_bytes": RANGE, "reps": args.reps, "frames_per_stream": frames,
           "index_scratch_bytes": L.chipf_index_scratch_len(S, S * (frames + 1)), "launches": LAUNCHES}
    for per in (1, 16):
        rs, start, rlen = requests(S, per, args.seed)
        off, ln, total, nseg, stage, vseg = layout(L, 14, cl, pd, frame_off, idx_off, nframes, plain, rs, start, rlen)
        assert (ln == RANGE).all() and total == RANGE * S * per and S * per <= nseg <= 2 * S * per
        res[f"read_{per}"] = {"requests": S * per, "work_items": nseg, "staging_bytes": stage, "vread_segments": vseg,
                              "scratch_bytes": L.chipf_read_scratch_len(S * per, nseg, stage, vseg, S)}
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dry", action="store_true", help="no device: lay the request set out on the host")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fread_bench_mi355x.json"))
    args = ap.parse_args()
    if args.dry:
        return dry_run(args)

    import torch

    import read_bench as RB
    import snap_data as SD
    from bench import ClockSampler
    from carbonado_amd import _lib
    from carbonado_amd import device as D
    from carbonado_amd import encoding as E

    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "fread_bench", "seed": args.seed, "streams": args.streams, "object_bytes": SEG, "range_bytes": RANGE,
           "reps": args.reps, "launches": LAUNCHES,
           "timing": "HIP events around each call, host_median_ms = host clock around the same call; one box, one run",
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count}}
    clocks = ClockSampler(0)
    clocks.start()
    S = args.streams
    pub = E.public_key(SECRET)
    sizes, in_off = [SEG] * S, [o * SEG for o in range(S)]
    ptr, vp = RB.ptr, RB.vp
    p8 = lambda a: a.ctypes.data_as(_lib.c_u8p)  # noqa: E731
    a64, a32 = (lambda x: np.ascontiguousarray(x, dtype=np.uint64)), (lambda x: np.ascontiguousarray(x, dtype=np.uint32))
    beats = []

    for corpus in CORPORA:
        rng = np.random.default_rng(args.seed)
        rows = [np.frombuffer(SD.mix(SEG, 40, args.seed + i), dtype=np.uint8) if corpus == "mix40"
                else rng.integers(0, 256, SEG, dtype=np.uint8) for i in range(8)]
        host = torch.empty((S, SEG), dtype=torch.uint8)
        for o in range(S):
            host[o] = torch.from_numpy(rows[o % 8].copy())
        inp = host.cuda().view(-1)
        del host
        for fmt in (14, 15):
            off, cap, total = D.snap_encode_layout(fmt, sizes, 256)
            buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
            hashes = torch.zeros((S, 32), dtype=torch.uint8, device="cuda")
            olen, infos = D.encode_ragged_snap(fmt, inp, in_off, sizes, buf, off, hashes, D.snap_ragged_scratch(fmt, sizes),
                                               pubkey=pub if fmt == 15 else None)
            torch.cuda.synchronize()
            pad, cl = [i.padding_len for i in infos], [i.chunk_len for i in infos]
            keys = ivs = None
            if fmt == 15:
                keys, ivs, kstat = D.stream_keys(SECRET, buf, off, olen, hashes, pad, cl, D.stream_keys_scratch(S))
                assert not kstat.any()
            caps = SEG // FRAME + 1
            n_off, n_len, n_pad, n_cl = a64(off), a64(olen), a32(pad), a32(cl)
            idx_off, idx_cap = a64(np.arange(S) * caps), a64(np.full(S, caps))
            frame_off, nframes, plain = np.zeros(S * caps, dtype=np.uint64), np.zeros(S, dtype=np.uint64), \
                np.zeros(S, dtype=np.uint64)
            istat, ivouch = np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.uint32)
            iscratch = D.frame_index_scratch(S, S * caps)
            pk, pv = (p8(keys), p8(ivs)) if fmt == 15 else (None, None)

            def frame_index():
                rc = L.chipf_frame_index_dev(fmt, pk, pv, None, vp(buf), ptr(n_off), ptr(n_len), vp(hashes), ptr(n_pad),
                                             ptr(n_cl), S, ptr(frame_off), ptr(idx_off), ptr(idx_cap), ptr(nframes),
                                             ptr(istat), ptr(plain), ptr(ivouch), vp(iscratch), iscratch.numel(), None)
                assert rc == 0, rc

            frame_index()
            assert not istat.any() and not ivouch.any() and (plain == SEG).all() and (nframes == caps - 1).all()

            forms, sets = {}, {}
            for per in (1, 16):
                rs, start, rlen = requests(S, per, args.seed + per)
                coff, clen, ctotal, nseg, stage, vseg = layout(L, fmt, n_cl, n_pad, frame_off, idx_off, nframes, plain, rs,
                                                               start, rlen)
                content = torch.full((ctotal + 16,), 0xA5, dtype=torch.uint8, device="cuda")
                status, used, vouch = (torch.zeros(S * per, dtype=torch.int32, device="cuda") for _ in range(3))
                scratch = D.frame_read_scratch(S * per, nseg, stage, vseg, S)
                sets[per] = dict(rs=rs, start=start, rlen=rlen, coff=coff, clen=clen, content=content, status=status,
                                 used=used, vouch=vouch, scratch=scratch, nseg=nseg, stage=stage)

                def read(q=sets[per], n=S * per):
                    rc = L.chipf_read_ranges_dev(fmt, pk, pv, None, ptr(frame_off), ptr(idx_off), ptr(nframes), ptr(plain),
                                                 vp(buf), ptr(n_off), ptr(n_len), vp(hashes), ptr(n_pad), ptr(n_cl), S,
                                                 ptr(q["rs"]), ptr(q["start"]), ptr(q["rlen"]), n, vp(q["content"]),
                                                 ptr(q["coff"]), ptr(q["clen"]), vp(q["status"]), vp(q["used"]),
                                                 vp(q["vouch"]), 0, vp(q["scratch"]), q["scratch"].numel(), None)
                    assert rc == 0, rc

                forms[f"read_{per}"] = read
                read()
                torch.cuda.synchronize()
                assert int(status.count_nonzero()) == 0 and int(vouch.count_nonzero()) == 0
                for r in range(0, S * per, max(1, S * per // 256)):
                    o = int(rs[r]) * SEG + int(start[r])
                    assert torch.equal(content[int(coff[r]):int(coff[r]) + RANGE], inp[o:o + RANGE]), ("read", per, r)

            d_out = torch.zeros(S * SEG, dtype=torch.uint8, device="cuda")
            d_status = torch.zeros(S, dtype=torch.int32, device="cuda")
            d_got = torch.zeros(S, dtype=torch.int64, device="cuda")
            d_scratch = D.snap_ragged_scratch(fmt, olen, sizes)

            def decode():
                D.decode_ragged_snap(fmt, buf, off, olen, hashes, pad, d_out, in_off, sizes, d_got, d_status, d_scratch,
                                     secret_key=SECRET if fmt == 15 else None)

            decode()
            torch.cuda.synchronize()
            assert int(d_status.count_nonzero()) == 0 and torch.equal(d_out[:SEG], inp[:SEG])
            forms["frame_index"], forms["decode"] = frame_index, decode
            r = res[f"level{fmt}_{corpus}"] = {
                "stream_bytes": int(sum(olen)), "frame_stream_bytes": int(frame_off[caps - 1]),
                **{f"read_{per}_sizes": {"requests": S * per, "work_items": int(sets[per]["nseg"]),
                                         "staging_bytes": int(sets[per]["stage"]),
                                         "scratch_bytes": int(sets[per]["scratch"].numel())} for per in (1, 16)},
                **RB.time_forms(forms, args.reps)}
            for per in (1, 16):
                r[f"decode_over_read_{per}"] = round(r["decode"]["median_ms"] / r[f"read_{per}"]["median_ms"], 2)
                beats.append(r[f"decode_over_read_{per}"] > 1)
            r["frame_index_over_decode"] = round(r["frame_index"]["median_ms"] / r["decode"]["median_ms"], 2)
            del buf, d_out, d_scratch, iscratch, sets, forms
            torch.cuda.empty_cache()
        del inp
        torch.cuda.empty_cache()

    res["clocks"] = clocks.stop()
    res["read_beats_decode"] = all(beats)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
