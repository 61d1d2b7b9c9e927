#!/usr/bin/env python3
"""Mixed-size device-resident batches at level 12 (Zfec|Bao): what a caller
pays today against one ragged call (include/carbonado_hip_ext.h).

Archive mix: --files files of a seeded random length in [1, 16] MiB, each cut
into 1 MiB segments: the full segments plus one tail per file, all tails
different.  Three forms over the same buffers:

  A  one chip_encode_batch_dev call per distinct size (the uniform entry
     points: the full segments in one call, every tail a call of its own);
  B  one chipx_encode_ragged_dev call for everything;
  C  one uniform call for the full segments + one ragged call for the tails.

Also the tails alone (A, B), a uniform control (2048 x 1 MiB through the
uniform and through the ragged call: the price of raggedness against K13) and
the same three measurements for decode.  Every form's output is compared with
the CPU oracle on a sample of objects before anything is timed.  Times are HIP
events around work that ends in a synchronise, 3 warm-ups, the forms
alternating within one process for --reps rounds; medians and min-max in ms,
GiB/s of input over the median.  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from carbonado_amd import _lib  # noqa: E402
from carbonado_amd import device as D  # noqa: E402
from oracle import oracle as O  # noqa: E402

LEVEL = 12
SEG = 1 << 20
SO = D.STREAM_OFFSET


def u64(xs):
    return (ctypes.c_uint64 * max(len(xs), 1))(*[int(x) for x in xs])


def vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


class Mix:
    """`full` segments of 1 MiB (rows of one uniform batch) followed by the
    tails, in one input buffer, one encoded buffer and one decoded buffer."""

    def __init__(self, L, full, tails, rng):
        self.L, self.full, self.tails = L, full, list(tails)
        self.sizes = [SEG] * full + self.tails
        self.count = len(self.sizes)
        self.in_off, cur = [], 0
        for n in self.sizes:
            self.in_off.append(cur)
            cur += (n + 255) // 256 * 256
        torch.manual_seed(int(rng.integers(1 << 30)))
        self.inp = torch.randint(0, 256, (cur + 256,), dtype=torch.uint8, device="cuda")
        # the full segments at the fast offset of a uniform batch's rows; the tails 16-B aligned, which the
        # uniform entry points ask of objects small enough for their single-object kernels
        off1, len1, total1 = D.ragged_layout(LEVEL, self.sizes[:full], 256, SO)
        off2, len2, total2 = D.ragged_layout(LEVEL, self.tails, 256, 0)
        self.out_off, self.out_len, total = off1 + [total1 + o for o in off2], len1 + len2, total1 + total2
        self.enc = torch.zeros(total, dtype=torch.uint8, device="cuda")
        self.dec = torch.zeros_like(self.inp)
        self.hashes = torch.zeros((self.count, 32), dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(self.count, dtype=torch.int32, device="cuda")
        self.pads = [(-n) % 4096 for n in self.sizes]
        self.pitch = (SO + self.out_len[0] + 255) // 256 * 256 if full else 0
        s_uni = max([L.chip_encode_scratch_len(LEVEL, n, full if i == 0 else 1)
                     for i, n in enumerate([SEG] + self.tails)] +
                    [L.chip_decode_scratch_len(LEVEL, ln, full if i == 0 else 1)
                     for i, ln in enumerate([self.out_len[0] if full else 8] + self.out_len[full:])])
        s_rag = max(L.chipx_ragged_scratch_len(LEVEL, u64(self.sizes), self.count, 0),
                    L.chipx_ragged_scratch_len(LEVEL, u64(self.out_len), self.count, 1))
        self.scratch = torch.zeros(max(s_uni, s_rag), dtype=torch.uint8, device="cuda")
        self.in_bytes = sum(self.sizes)
        # ctypes arguments, built once: the loops below time the calls, not Python
        self._olen, self._info = ctypes.c_uint64(), _lib.EncodeInfoC()
        self._rag = {}
        for name, lo in (("all", 0), ("tails", full)):
            self._rag[name] = dict(n=self.count - lo, ioff=u64(self.in_off[lo:]), sizes=u64(self.sizes[lo:]),
                                   ooff=u64(self.out_off[lo:]), olen=u64(self.out_len[lo:]),
                                   lens=u64([0] * (self.count - lo)), pads=(ctypes.c_uint32 * max(self.count - lo, 1))(
                                       *self.pads[lo:]), lo=lo)

    # ---- encode
    def enc_uniform_full(self):
        if self.full:
            rc = self.L.chip_encode_batch_dev(LEVEL, vp(self.inp), SEG, SEG, self.full, vp(self.enc, SO), self.pitch,
                                              ctypes.byref(self._olen), vp(self.hashes), ctypes.byref(self._info),
                                              vp(self.scratch), None)
            assert rc == 0, rc

    def enc_uniform_tails(self):
        for i in range(self.full, self.count):
            rc = self.L.chip_encode_batch_dev(LEVEL, vp(self.inp, self.in_off[i]), 0, self.sizes[i], 1,
                                              vp(self.enc, self.out_off[i]), 0, ctypes.byref(self._olen),
                                              vp(self.hashes, 32 * i), ctypes.byref(self._info), vp(self.scratch), None)
            assert rc == 0, rc

    def enc_ragged(self, which):
        r = self._rag[which]
        rc = self.L.chipx_encode_ragged_dev(LEVEL, vp(self.inp), r["ioff"], r["sizes"], r["n"], vp(self.enc), r["ooff"],
                                            r["lens"], vp(self.hashes, 32 * r["lo"]), None, vp(self.scratch), None)
        assert rc == 0, rc

    # ---- decode
    def dec_uniform_full(self):
        if self.full:
            rc = self.L.chip_decode_batch_dev(LEVEL, vp(self.enc, SO), self.pitch, self.out_len[0], self.full,
                                              vp(self.hashes), 0, vp(self.dec), SEG, ctypes.byref(self._olen),
                                              vp(self.status), vp(self.scratch), None)
            assert rc == 0, rc

    def dec_uniform_tails(self):
        for i in range(self.full, self.count):
            rc = self.L.chip_decode_batch_dev(LEVEL, vp(self.enc, self.out_off[i]), 0, self.out_len[i], 1,
                                              vp(self.hashes, 32 * i), self.pads[i], vp(self.dec, self.in_off[i]), 0,
                                              ctypes.byref(self._olen), vp(self.status, 4 * i), vp(self.scratch), None)
            assert rc == 0, rc

    def dec_ragged(self, which):
        r = self._rag[which]
        rc = self.L.chipx_decode_ragged_dev(LEVEL, vp(self.enc), r["ooff"], r["olen"], r["n"],
                                            vp(self.hashes, 32 * r["lo"]), r["pads"], vp(self.dec), r["ioff"], r["lens"],
                                            vp(self.status, 4 * r["lo"]), vp(self.scratch), None)
        assert rc == 0, rc

    def forms(self, decode, tails_only=False):
        uf, ut, rg = ((self.dec_uniform_full, self.dec_uniform_tails, self.dec_ragged) if decode else
                      (self.enc_uniform_full, self.enc_uniform_tails, self.enc_ragged))
        if tails_only:
            return {"A": ut, "B": lambda: rg("tails")}
        return {"A": lambda: (uf(), ut()), "B": lambda: rg("all"), "C": lambda: (uf(), rg("tails"))}

    # ---- bit check against the oracle on a sample of objects
    def check(self, sample, forms_enc, forms_dec):
        want = {}
        for i in sample:
            data = self.inp[self.in_off[i]:self.in_off[i] + self.sizes[i]].cpu().numpy().tobytes()
            want[i] = (data,) + tuple(O.encode(data, LEVEL)[:2])
        for name, f in forms_enc.items():
            self.enc.zero_()
            self.hashes.zero_()
            f()
            torch.cuda.synchronize()
            for i in sample:
                got = self.enc[self.out_off[i]:self.out_off[i] + self.out_len[i]].cpu().numpy().tobytes()
                assert got == want[i][1] and self.hashes[i].cpu().numpy().tobytes() == want[i][2], ("encode", name, i)
        for name, f in forms_dec.items():
            self.dec.zero_()
            self.status.fill_(77)
            f()
            torch.cuda.synchronize()
            st = self.status.cpu().numpy()  # 77: an object this form does not touch (the tails-only forms)
            assert not st[st != 77].any() and not st[sample].any(), ("decode status", name)
            for i in sample:
                got = self.dec[self.in_off[i]:self.in_off[i] + self.sizes[i]].cpu().numpy().tobytes()
                assert got == want[i][0], ("decode", name, i)


def time_forms(forms, reps, in_bytes):
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for f in forms.values():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = ev(), ev()
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "GiBps_in": round(in_bytes / (med * 1e-3) / (1 << 30), 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--control", type=int, default=2048, help="objects of the uniform control (0: skip it)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--profile-form", choices=["A", "B", "C"], default="",
                    help="after the bit check only run this form of the archive mix --reps times, encode then "
                         "decode (for a kernel trace of one form in a run of its own)")
    args = ap.parse_args()
    L = _lib.lib()
    rc = L.chip_init(0)
    if rc != 0:
        raise SystemExit(f"no usable gfx950 device (status {rc})")
    rng = np.random.default_rng(args.seed)
    lengths = rng.integers(1 << 20, (16 << 20) + 1, args.files)
    full = int(sum(int(x) // SEG for x in lengths))
    tails = [int(x) % SEG for x in lengths if int(x) % SEG]
    prop = torch.cuda.get_device_properties(0)
    res = {"tool": "ragged_bench", "level": LEVEL, "seed": args.seed, "files": args.files, "reps": args.reps,
           "box": {"device": prop.name, "arch": prop.gcnArchName, "cus": prop.multi_processor_count},
           "full_segments": full, "tails": len(tails), "distinct_tails": len(set(tails))}
    mix = Mix(L, full, tails, rng)
    sample = sorted({0, full - 1, full, full + len(tails) // 2, mix.count - 1,
                     full + int(np.argmin(tails)), full + int(np.argmax(tails))})
    mix.check(sample, mix.forms(False), mix.forms(True))
    mix.check([i for i in sample if i >= full], mix.forms(False, True), mix.forms(True, True))
    res["checked_objects"] = len(sample)
    if args.profile_form:
        for decode in (False, True):
            f = mix.forms(decode)[args.profile_form]
            for _ in range(args.reps):
                f()
            torch.cuda.synchronize()
        print(json.dumps({**res, "profiled_form": args.profile_form}))
        return
    res["archive_in_GiB"] = round(mix.in_bytes / (1 << 30), 3)
    res["archive_encode"] = time_forms(mix.forms(False), args.reps, mix.in_bytes)
    res["archive_decode"] = time_forms(mix.forms(True), args.reps, mix.in_bytes)
    tail_bytes = sum(tails)
    res["tails_in_GiB"] = round(tail_bytes / (1 << 30), 3)
    res["tails_encode"] = time_forms(mix.forms(False, True), args.reps, tail_bytes)
    res["tails_decode"] = time_forms(mix.forms(True, True), args.reps, tail_bytes)
    del mix
    torch.cuda.empty_cache()
    if args.control:
        ctl = Mix(L, args.control, [], rng)
        f_enc = {"uniform": ctl.enc_uniform_full, "ragged": lambda: ctl.enc_ragged("all")}
        f_dec = {"uniform": ctl.dec_uniform_full, "ragged": lambda: ctl.dec_ragged("all")}
        ctl.check([0, args.control - 1], f_enc, f_dec)
        res["control_objects"] = args.control
        res["control_encode"] = time_forms(f_enc, args.reps, ctl.in_bytes)
        res["control_decode"] = time_forms(f_dec, args.reps, ctl.in_bytes)
    res["done"] = {
        "tails_encode_B_median_below_A_min": res["tails_encode"]["B"]["median_ms"] < res["tails_encode"]["A"]["min_ms"],
        "archive_encode_C_median_below_A_min":
            res["archive_encode"]["C"]["median_ms"] < res["archive_encode"]["A"]["min_ms"],
        "tails_decode_B_median_below_A_min": res["tails_decode"]["B"]["median_ms"] < res["tails_decode"]["A"]["min_ms"],
        "archive_decode_C_median_below_A_min":
            res["archive_decode"]["C"]["median_ms"] < res["archive_decode"]["A"]["min_ms"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
