#!/usr/bin/env python3
"""Key mixes for the key cache: what keeping the fixed-base keys' tables from batch to batch gains or
costs.  Times fdgpu_ed25519_verify_txns_device on HBM-resident batches of single-signature 1232-byte transactions
with fdgpu_debug_opts_t.key_cache on (0) and off (1: every slot emptied ahead of each batch, so every key builds,
with the same kernels and launches), two contexts of one build interleaved (on off off on ...),
tools/keyfixed_mix.py's way and with its batches:

  flagship     the benchmark's shape: 1,024 signers, one batch repeated -- every key resident from the second on;
  exact128     every key at exactly 128 signatures, one batch repeated: twice as many keys as FD_FB_CAP = 4,096
               slots.  The residents are stamped before any claim, so the steady state must build nothing;
  exact128alt  the same shape, two batches of disjoint keys alternated: every batch misses and evicts, which is the
               off context's work plus the look-ups -- must not lose;
  exact8       every key at exactly 8 signatures: no candidate, only the index and an empty launch -- must not lose;
  distinct     every key distinct -- must not lose.

usage: tools/keycache_mix.py [--txns N] [--reps R] [--steps S] [--batches flagship,exact128,...] [--out FILE]
Prints one JSON line per row: per run the mean ms per step, the fixed-base keys and the cache's hits and builds
the on context counted in its last batch, medians, the off runs' spread and on - off.  Exits non-zero when a row
that must not lose is slower than off by more than the off runs' spread, when exact128 still builds in its steady
state, or when any code is wrong.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import keyfixed_mix  # noqa: E402
import keysplit_mix  # noqa: E402

MUST_NOT_LOSE = ("exact128alt", "exact8", "distinct")


def make(synth, name, n):
    """The row's batches, [(payload, desc, expect, nsig), ...]: a step takes them in turn"""
    if name == "flagship":
        return [synth.make_batch(n, synth.LARGE_NOOP, seed=1236, nkeys=1024, threads=16)]
    if name == "exact128alt":
        assert n % 128 == 0
        out = []
        for seed in (98, 198):       # (98: exact128's own keys)
            base = keysplit_mix.keys_parallel(synth, n // 128, seed)
            out.append(synth.make_batch(n, synth.LARGE_NOOP, seed=1235, threads=16,
                                        key_arr=base[(np.arange(7 * n + 4) // 7) % (n // 128)]))
        return out
    return [keyfixed_mix.make(synth, name, n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=4, help="interleaved runs per mode")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="flagship,exact128,exact128alt,exact8,distinct")
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
        engine.debug_set_opts(key_cache=mode)
        try:
            eng[name] = fa.Engine(device=0, max_txn=n, max_sig=n)
        finally:
            engine.debug_reset_opts()
    lines, fail = [], []
    for bname in a.batches.split(","):
        host = make(synth, bname, n)
        dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(d.view(np.uint8)).cuda(), ns) for p, d, _, ns in host]
        to = torch.empty(n, dtype=torch.int8, device="cuda")
        turn = {name: 0 for name in eng}         # each context goes on alternating where it stopped

        def steps(name, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                pd, dd, ns = dev[turn[name] % len(dev)]
                turn[name] += 1
                eng[name].verify_txns_device(pd.data_ptr(), dd.data_ptr(), n, ns, to.data_ptr(), None, st)
            torch.cuda.synchronize()             # (the whole device: every stream's work is done)
            return (time.perf_counter() - t0) * 1e3 / k

        ok = True
        for name in eng:                         # warm-up (the de-duplication settles into its mode), and the codes
            steps(name, 2)                       # of a batch that found its keys resident, for each of the row's batches
            for _ in dev:
                steps(name, 1)
                ok = ok and bool((to.cpu().numpy() == host[(turn[name] - 1) % len(dev)][2]).all())
        fixed, cache = eng["on"].fixed_count(), eng["on"].fcache_count()
        runs = {name: [] for name in eng}
        for r in range(a.reps):
            for name in (("on", "off"), ("off", "on"))[r & 1]:
                runs[name].append(round(steps(name, a.steps), 4))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = max(runs["off"]) - min(runs["off"])
        res = {"batch": bname, "txns": n, "fixed_keys_sigs_on": fixed, "hits_builds_on": cache,
               "hits_builds_off": eng["off"].fcache_count(),
               "results_ok": ok, "ms_per_step": runs, "median_ms": med, "off_spread_ms": round(spread, 4),
               "on_minus_off_median_ms": round(med["on"] - med["off"], 4),
               "within_off_spread": bool(med["on"] - med["off"] <= spread),
               "wins_by_more_than_off_spread": bool(med["off"] - med["on"] > spread)}
        if bname in MUST_NOT_LOSE and not res["within_off_spread"]:
            fail.append(f"{bname} loses more than the spread between the off runs")
        if bname == "exact128" and cache[1]:
            fail.append(f"exact128 still builds {cache[1]} keys in its steady state")
        if not ok:
            fail.append(f"{bname}: wrong codes")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del dev, to, host
    for e in eng.values():
        e.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if fail:
        sys.exit("FAIL: " + "; ".join(fail))


if __name__ == "__main__":
    main()
