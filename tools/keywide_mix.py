#!/usr/bin/env python3
"""Key mixes for the wide tables: what giving the first 1,024 full slots of a context tables over digits of
11, 11 and 10 bits gains or costs on batches other than the benchmark's.  Times fdgpu_ed25519_verify_txns_device on
HBM-resident batches of single-signature 1232-byte transactions with fdgpu_debug_opts_t.key_wide on (0) and off (1:
nothing allocated, the parent's kernels and launches), two contexts of one build per row, interleaved (on off off
on ...), tools/keyfull_mix.py's way and with its batches.  Each row repeats one batch:

  distinct       every key distinct: no fixed-base key -- must not lose;
  exact8         every key at exactly 8 signatures: hot keys only -- must not lose;
  exact128cold   every key at exactly 128 signatures with key_cache = 1 in both contexts: nothing is ever found
                 resident, so nothing is promoted and no wide table is built -- must not lose;
  exact128       the same batch with the cache on, on fresh contexts.  8,192 keys ask for 4,096 slots, of which the first
                 1,024 are wide; the first step claims, the next four promote 1,024 slots each, and each of those
                 steps builds the wide tables of the promoted slots below 1,024.  Reported: every one of the first eight
                 steps on its own (both contexts), the steady state after them, and how many steady steps pay the
                 builds back;
  half           half the signatures from 1,024 keys, half from keys of their own: likewise;
  flagship       the benchmark's shape, 1,024 signers: likewise.

usage: tools/keywide_mix.py [--txns N] [--reps R] [--steps S] [--batches distinct,exact8,...] [--out FILE]
Prints one JSON line per row.  Exits non-zero when a row that must not lose is slower than off by more than the off
runs' spread, or when any code is wrong.
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

MUST_NOT_LOSE = ("distinct", "exact8", "exact128cold")
FIRST = 8                            # steps timed one by one on the fresh contexts


def make(synth, name, n):
    if name == "flagship":
        return synth.make_batch(n, synth.LARGE_NOOP, seed=1236, nkeys=1024, threads=16)
    return keyfixed_mix.make(synth, "exact128" if name.startswith("exact128") else name, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=6, help="interleaved runs per mode")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="distinct,exact8,exact128cold,exact128,half,flagship")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine, synth
    fa.load_library()
    n = a.txns
    stream = torch.cuda.Stream()                 # a stream of its own: stream 0 means "the context's" to the engine
    st = stream.cuda_stream
    lines, fail = [], []
    for bname in a.batches.split(","):
        payload, desc, expect, nsig = make(synth, bname, n)
        pd = torch.from_numpy(payload).cuda()
        dd = torch.from_numpy(desc.view(np.uint8)).cuda()
        to = torch.empty(n, dtype=torch.int8, device="cuda")
        eng, mem = {}, {}
        for name, mode in (("on", 0), ("off", 1)):
            engine.debug_set_opts(key_wide=mode, key_cache=1 if bname == "exact128cold" else 0)
            free0 = torch.cuda.mem_get_info()[0]
            try:
                eng[name] = fa.Engine(device=0, max_txn=n, max_sig=n)
            finally:
                engine.debug_reset_opts()
            mem[name] = free0 - torch.cuda.mem_get_info()[0]          # the context's device allocation

        def steps(e, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                e.verify_txns_device(pd.data_ptr(), dd.data_ptr(), n, nsig, to.data_ptr(), None, st)
            torch.cuda.synchronize()             # (the whole device: every stream's work is done)
            return (time.perf_counter() - t0) * 1e3 / k

        ok = True
        first = {name: [] for name in eng}
        wide = []
        for k in range(FIRST):                   # the first steps one by one: the claims, then the promotions
            for name in (("on", "off"), ("off", "on"))[k & 1]:
                first[name].append(round(steps(eng[name], 1), 4))
                ok = ok and bool((to.cpu().numpy() == expect).all())
            wide.append(eng["on"].fwide_count())
        runs = {name: [] for name in eng}
        for r in range(a.reps):
            for name in (("on", "off"), ("off", "on"))[r & 1]:
                runs[name].append(round(steps(eng[name], a.steps), 4))
                ok = ok and bool((to.cpu().numpy() == expect).all())
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = max(runs["off"]) - min(runs["off"])
        # what the on context's first steps cost beyond the off context's, over what a steady step saves
        extra = sum(x - y for x, y in zip(first["on"][1:], first["off"][1:]) if x > y)
        gain = med["off"] - med["on"]
        res = {"batch": bname, "txns": n, "fixed_keys_sigs_on": eng["on"].fixed_count(),
               "full_keys_sigs_on": eng["on"].ffull_count(), "wide_keys_sigs_on": eng["on"].fwide_count(),
               "wide_keys_sigs_off": eng["off"].fwide_count(), "wide_keys_sigs_first_steps_on": wide,
               "context_device_bytes": mem,
               "results_ok": ok, "first_steps_ms": first, "ms_per_step": runs, "median_ms": med,
               "off_spread_ms": round(spread, 4), "on_minus_off_median_ms": round(-gain, 4),
               "first_steps_extra_ms": round(extra, 4),
               "steady_steps_that_pay_it_back": round(extra / gain, 2) if gain > 0 else None,
               "within_off_spread": bool(-gain <= spread), "wins_by_more_than_off_spread": bool(gain > spread)}
        if bname in MUST_NOT_LOSE and not res["within_off_spread"]:
            fail.append(f"{bname} loses more than the spread between the off runs")
        if not ok:
            fail.append(f"{bname}: wrong codes")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        for e in eng.values():
            e.close()
        del pd, dd, to, eng
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if fail:
        sys.exit("FAIL: " + "; ".join(fail))


if __name__ == "__main__":
    main()
