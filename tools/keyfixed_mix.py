#!/usr/bin/env python3
"""Key mixes for the fixed-base keys: what per-key tables gain or cost on batches other than the
benchmark's.  Times fdgpu_ed25519_verify_txns_device on HBM-resident batches of single-signature 1232-byte
transactions with fdgpu_debug_opts_t.key_fixed on (0) and off (1), two contexts of one build interleaved
(on off off on ...), tools/keysplit_mix.py's way and with its batches.  Each row repeats one batch, so from its
second step on the on context finds every table in its key cache: the on column is a warm cache's
time; tools/keycache_mix.py has the cold one (key_cache off) and the batches that evict:

  exactK     every key at exactly K signatures (exact128: FD_FB_MIN, the row that confirms or moves the bound;
             more keys than FD_FB_CAP = 4,096 ask for tables then, and the surplus stays hot);
  half       half the signatures from 1,024 keys, half from keys of their own, interleaved by blocks of 4,096;
  exact8     every key at exactly 8 signatures: hot keys only, no tables -- must not lose;
  distinct   every key distinct -- must not lose.

usage: tools/keyfixed_mix.py [--txns N] [--reps R] [--steps S] [--batches exact128,half,exact8,distinct] [--out FILE]
Prints one JSON line per batch: per run the mean ms per step, the fixed-base and the repeated keys and signatures
the on context counted, medians, the off runs' spread and on - off.  Exits non-zero when exact8 or distinct loses
more than the off runs' spread, or any code is wrong.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import keysplit_mix  # noqa: E402


def make(synth, name, n):
    if name.startswith("exact"):
        k = int(name[5:])
        assert n % k == 0
        base = keysplit_mix.keys_parallel(synth, n // k, 98)
        return synth.make_batch(n, synth.LARGE_NOOP, seed=1235, threads=16,
                                key_arr=base[(np.arange(7 * n + 4) // 7) % (n // k)])
    return keysplit_mix.make(synth, name, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=4, help="interleaved runs per mode")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="exact128,half,exact8,distinct")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine, synth
    fa.load_library()
    n = a.txns
    stream = torch.cuda.Stream()                 # a stream of its own: stream 0 means "the context's" to the engine
    st = stream.cuda_stream
    eng = {}
    for name, mode in (("on", 0), ("off", 1)):
        engine.debug_set_opts(key_fixed=mode)
        try:
            eng[name] = fa.Engine(device=0, max_txn=n, max_sig=n)
        finally:
            engine.debug_reset_opts()
    lines, fail = [], []
    for bname in a.batches.split(","):
        payload, desc, expect, nsig = make(synth, bname, n)
        pd = torch.from_numpy(payload).cuda()
        dd = torch.from_numpy(desc.view(np.uint8)).cuda()
        to = torch.empty(n, dtype=torch.int8, device="cuda")

        def steps(e, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                e.verify_txns_device(pd.data_ptr(), dd.data_ptr(), n, nsig, to.data_ptr(), None, st)
            torch.cuda.synchronize()             # (the whole device: every stream's work is done)
            return (time.perf_counter() - t0) * 1e3 / k

        ok = True
        for e in eng.values():                   # warm-up (the de-duplication settles into its mode), and the codes
            steps(e, 3)
            ok = ok and bool((to.cpu().numpy() == expect).all())
        fixed, hot = eng["on"].fixed_count(), eng["on"].hot_count()
        runs = {name: [] for name in eng}
        for r in range(a.reps):
            for name in (("on", "off"), ("off", "on"))[r & 1]:
                runs[name].append(round(steps(eng[name], a.steps), 4))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = max(runs["off"]) - min(runs["off"])
        res = {"batch": bname, "txns": n, "sigs": nsig, "fixed_keys_sigs_on": fixed, "repeated_keys_sigs_on": hot,
               "results_ok": ok, "ms_per_step": runs, "median_ms": med, "off_spread_ms": round(spread, 4),
               "on_minus_off_median_ms": round(med["on"] - med["off"], 4),
               "within_off_spread": bool(med["on"] - med["off"] <= spread),
               "wins_by_more_than_off_spread": bool(med["off"] - med["on"] > spread)}
        if bname in ("exact8", "distinct") and not res["within_off_spread"]:
            fail.append(f"{bname} loses more than the spread between the off runs")
        if not ok:
            fail.append(f"{bname}: wrong codes")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del pd, dd, to
    for e in eng.values():
        e.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if fail:
        sys.exit("FAIL: " + "; ".join(fail))


if __name__ == "__main__":
    main()
