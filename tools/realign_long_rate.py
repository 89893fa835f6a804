#!/usr/bin/env python3
"""Rate of the long realignment kernel beside the short one, in one run: gtx_disc_realign_batch on a default object at 256 x 712
(the short workload's window at 2 x 256 + 200), and on an object with gtx_disc_set_max_read_len(d, 1000) at 257 x 714, 512 x 1 224
and 1 000 x 2 200.  Every read is a piece of its window with substitutions and an indel.  Per shape: a warm-up call, then the median
of --repeats calls between host clocks around a device wait, in pairs and in cell updates (read length x window length) per second;
the result bytes of every repeat are the same.  The long figures hold the short kernel's launch too (it runs first and refuses the
pair).  The parent cannot run the long shapes, so the short kernel measured beside them is the yardstick: a first measurement, not
a bar.  Writes profiles/realign_long_rate.json.  Usage: tools/realign_long_rate.py [--repeats R] [--out FILE]"""
import argparse
import ctypes as C
import datetime
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphtyper_amd import lib as gtx  # noqa: E402

SHAPES = ((256, 712, 8192, False), (257, 714, 8192, True), (512, 1224, 4096, True), (1000, 2200, 2048, True))  # m, n, pairs, long mode
LUT = {"A": 1, "C": 2, "G": 4, "T": 8}


def make(m, n, n_pairs, seed=1):
    rng = random.Random(seed + m)
    n_windows, n_reads = 64, 512
    windows = ["".join(rng.choice("ACGT") for _ in range(n)) for _ in range(n_windows)]
    stride = (m + 31) // 32 * 16
    codes = np.zeros((n_reads, stride * 2), np.uint8)
    home = []
    for i in range(n_reads):
        w = rng.randrange(n_windows)
        a = rng.randrange(50, n - m - 60)
        r = list(windows[w][a:a + m + 10])
        for k in range(len(r)):
            if rng.random() < 0.01:
                r[k] = rng.choice("ACGT")
        k = rng.randrange(20, m - 20)
        if rng.random() < 0.5:
            del r[k:k + rng.randrange(1, 8)]
        else:
            r[k:k] = [rng.choice("ACGT") for _ in range(rng.randrange(1, 8))]
        codes[i, :m] = [LUT[c] for c in r[:m]]
        home.append(w)
    planes = gtx.planes_reference(codes, stride)
    lens = np.full(n_reads, m, np.uint16)
    off = (np.arange(n_windows + 1) * n).astype(np.uint32)
    seq = np.frombuffer("".join(windows).encode(), np.uint8).copy()
    pairs = np.zeros(n_pairs, gtx.REALIGN_PAIR)
    pairs["read"] = np.arange(n_pairs) % n_reads
    pairs["target"] = np.array(home, np.uint32)[pairs["read"]]
    return planes, stride, lens, seq, off, pairs


def device_rate(m, n, n_pairs, long_mode, repeats):
    import torch
    planes, stride, lens, seq, off, pairs = make(m, n, n_pairs)
    L = gtx.lib()
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGT", 4, 0, 0, C.byref(h)))
    if long_mode:
        gtx.disc_set_max_read_len(h, gtx.MAX_READ_LONG)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0") for a in (planes, lens, seq, off, pairs)]
    out = torch.zeros(n_pairs * gtx.REALIGN_RESULT.itemsize, dtype=torch.uint8, device="cuda:0")
    times, seen = [], set()
    for i in range(repeats + 1):  # the first call is the warm-up
        out.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gtx.disc_realign_batch(h, dev[0].data_ptr(), stride, dev[1].data_ptr(), len(lens), dev[2].data_ptr(), dev[3].data_ptr(), len(off) - 1,
                               dev[4].data_ptr(), n_pairs, out.data_ptr(), None)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        seen.add(out.cpu().numpy().tobytes())
    res = np.frombuffer(next(iter(seen)), gtx.REALIGN_RESULT)
    assert len(seen) == 1 and (res["status"] == 0).all() and (res["score"] > 0.75 * m).all()
    L.gtx_disc_destroy(h)
    t, cells = statistics.median(times[1:]), m * n * n_pairs
    return {"kernel": "long (behind the short one's launch)" if long_mode else "short", "read_bases": m, "window_letters": n, "pairs": n_pairs, "cells": cells,
            "seconds_median": t, "seconds_min": min(times[1:]), "seconds_max": max(times[1:]), "pairs_per_s": n_pairs / t, "cell_updates_per_s": cells / t,
            "results_equal_across_repeats": True}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign_long_rate.json"))
    a = ap.parse_args()
    result = {"tool": "tools/realign_long_rate.py", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "repeats": a.repeats,
              "runs": [device_rate(m, n, k, long_mode, a.repeats) for m, n, k, long_mode in SHAPES]}
    short = result["runs"][0]["cell_updates_per_s"]
    for r in result["runs"]:
        r["cell_rate_over_the_short_kernels"] = r["cell_updates_per_s"] / short
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
