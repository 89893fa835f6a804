#!/usr/bin/env python3
"""Rate of gtx_disc_realign_batch: 150-base reads against ~500-letter windows, 20 000 and 200 000 pairs, the median of five calls
after a warm-up, in pairs and in cell updates (read length x window length) per second.  For scale the 20 000 pairs also go
through a plain -O3, sanitizer-free build of the kernel's text over a sequential wave (tests/emu_realign) on one host core.
There is no other implementation to compare with: the reference's aligner (paw) is absent from its tree.
Writes profiles/realign_rate.json.  Usage: tools/realign_rate.py [--no-host]"""
import ctypes as C
import datetime
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphtyper_amd import lib as gtx  # noqa: E402


def make(n_pairs, seed=1):
    rng = random.Random(seed)
    n_windows, n_reads = 256, 4096
    windows = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(480, 521))) for _ in range(n_windows)]
    codes = np.zeros((n_reads, 160), np.uint8)
    lut = {"A": 1, "C": 2, "G": 4, "T": 8}
    home = []
    for i in range(n_reads):
        w = rng.randrange(n_windows)
        a = rng.randrange(60, len(windows[w]) - 220)
        r = list(windows[w][a:a + 160])
        for k in range(len(r)):
            if rng.random() < 0.01:
                r[k] = rng.choice("ACGT")
        if rng.random() < 0.5:  # an indel of the kind the windows are made for
            k = rng.randrange(20, 130)
            if rng.random() < 0.5:
                del r[k:k + rng.randrange(1, 8)]
            else:
                r[k:k] = [rng.choice("ACGT") for _ in range(rng.randrange(1, 8))]
        codes[i, :150] = [lut[c] for c in r[:150]]
        home.append(w)
    planes = gtx.planes_reference(codes, 80)
    lens = np.full(n_reads, 150, np.uint16)
    off = np.zeros(n_windows + 1, np.uint32)
    off[1:] = np.cumsum([len(w) for w in windows])
    seq = np.frombuffer("".join(windows).encode(), np.uint8).copy()
    pairs = np.zeros(n_pairs, gtx.REALIGN_PAIR)
    pairs["read"] = np.arange(n_pairs) % n_reads
    pairs["target"] = np.array(home, np.uint32)[pairs["read"]]
    cells = int((150 * (off[pairs["target"] + 1] - off[pairs["target"]]).astype(np.int64)).sum())
    return planes, 80, lens, seq, off, pairs, cells


def device_rate(n_pairs):
    import torch
    planes, stride, lens, seq, off, pairs, cells = make(n_pairs)
    L = gtx.lib()
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, 0, C.byref(h)))
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0") for a in (planes, lens, seq, off, pairs)]
    out = torch.zeros(n_pairs * gtx.REALIGN_RESULT.itemsize, dtype=torch.uint8, device="cuda:0")
    times = []
    for i in range(6):  # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gtx.disc_realign_batch(h, dev[0].data_ptr(), stride, dev[1].data_ptr(), len(lens), dev[2].data_ptr(), dev[3].data_ptr(), len(off) - 1,
                               dev[4].data_ptr(), n_pairs, out.data_ptr(), None)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res = out.cpu().numpy().view(gtx.REALIGN_RESULT)
    assert (res["status"] == 0).all()
    L.gtx_disc_destroy(h)
    t = statistics.median(times[1:])
    return {"pairs": n_pairs, "cells": cells, "seconds_median_of_5": t, "pairs_per_s": n_pairs / t, "cell_updates_per_s": cells / t}, res


def host_rate(n_pairs, device_results=None):
    planes, stride, lens, seq, off, pairs, cells = make(n_pairs)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "emu_realign_o3")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_realign"), "-s", "SAN=", "OPT=-O3", "OUT=" + exe])
        case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
        with open(case, "wb") as f:
            f.write(np.array([stride, len(lens), len(off) - 1, n_pairs, len(seq)], np.uint32).tobytes())
            f.write(planes.tobytes() + lens.tobytes() + b"\0\0" * (len(lens) & 1) + off.tobytes() + seq.tobytes() + b"\0" * (-len(seq) % 4) + pairs.tobytes())
        t = float(subprocess.run([exe, case, out], check=True, stdout=subprocess.PIPE).stdout.decode().split()[0])
        same = None if device_results is None else bool(np.fromfile(out, gtx.REALIGN_RESULT).tobytes() == device_results.tobytes())
    return {"pairs": n_pairs, "cells": cells, "seconds": t, "pairs_per_s": n_pairs / t, "cell_updates_per_s": cells / t,
            "what": "the kernel's text over a sequential wave, g++ -O3, one core", "results_equal_the_device": same}


def main():
    import torch
    result = {"device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "read_length": 150, "window_letters": "480..520",
              "runs": []}
    small = None
    for n in (20000, 200000):
        r, res = device_rate(n)
        result["runs"].append(r)
        small = res if n == 20000 else small
    if "--no-host" not in sys.argv:
        result["host_one_core"] = host_rate(20000, small)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "realign_rate.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
