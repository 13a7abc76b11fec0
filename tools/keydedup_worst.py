#!/usr/bin/env python3
"""Worst case of the per-batch key de-duplication (DESIGN "One decode per distinct key"): a batch in which
the de-duplication saves nothing.  Times fdgpu_ed25519_verify_txns_device on an HBM-resident batch of
single-signature 1232-byte transactions in which every key is distinct, with fdgpu_debug_opts_t.key_dedup
on (0) and off (1), two contexts of one build interleaved (on off off on ...).  The all-distinct batch may
lose no more than the spread between the off runs themselves.

synth's signer index is (7 t + r) mod nkeys with r < 4, so nkeys equal to the signature count still repeats
keys (68 % distinct at 1M, and the de-duplication wins): only nkeys >= 7 n + 4, the default here, gives
every transaction a key of its own.  The default run checks that: the on context must have decoded as many
keys as there are signatures.  --nkeys K times any other batch.

usage: tools/keydedup_worst.py [--txns N] [--nkeys K] [--reps R] [--steps S] [--modes on,off] [--out FILE]
Prints one JSON line: per run the mean ms per step, the decodes the on context counted
(fdgpu_ed25519_key_count), the medians and spreads; the default run exits non-zero when on - off exceeds
the off runs' spread.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def keys_parallel(synth, n, seed, threads=16):
    """synth.keys in chunks on a thread pool (the C generator derives one key pair at a time)."""
    out = np.zeros((n, 128), np.uint8)
    edges = [n * i // threads for i in range(threads + 1)]

    def part(i):
        if edges[i + 1] > edges[i]:
            out[edges[i]:edges[i + 1]] = synth.keys(edges[i + 1] - edges[i], seed + 7919 * i)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(threads)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 20)
    ap.add_argument("--nkeys", type=int, default=0, help="0 = 7 txns + 4: every key distinct (the worst case)")
    ap.add_argument("--reps", type=int, default=4, help="interleaved runs per mode")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--modes", default="on,off", help="on,off (default), or one of them alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine, synth
    fa.load_library()
    n = a.txns
    nkeys = a.nkeys or 7 * n + 4
    payload, desc, expect, nsig = synth.make_batch(n, synth.LARGE_NOOP, seed=1234, threads=16,
                                                   key_arr=keys_parallel(synth, nkeys, 99))
    pd = torch.from_numpy(payload).cuda()
    dd = torch.from_numpy(desc.view(np.uint8)).cuda()
    to = torch.empty(n, dtype=torch.int8, device="cuda")
    stream = torch.cuda.Stream()                 # a stream of its own: stream 0 means "the context's" to the engine
    st = stream.cuda_stream
    eng = {}
    for name, mode in (("on", 0), ("off", 1)):
        if name not in a.modes.split(","):
            continue
        engine.debug_set_opts(key_dedup=mode)
        try:
            eng[name] = fa.Engine(device=0, max_txn=n, max_sig=nsig)
        finally:
            engine.debug_reset_opts()

    def steps(e, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            e.verify_txns_device(pd.data_ptr(), dd.data_ptr(), n, nsig, to.data_ptr(), None, st)
        torch.cuda.synchronize()                 # (the whole device: every stream's work is done)
        return (time.perf_counter() - t0) * 1e3 / k

    ok = True
    for e in eng.values():                       # warm-up, and the codes
        steps(e, 2)
        ok = ok and bool((to.cpu().numpy() == expect).all())
    decoded = eng["on"].key_count() if "on" in eng else None
    if not a.nkeys and decoded is not None:
        assert decoded == nsig, f"not the worst case: {decoded} keys decoded for {nsig} signatures"
    runs = {name: [] for name in eng}
    for r in range(a.reps):
        for name in (("on", "off"), ("off", "on"))[r & 1]:
            if name in eng:
                runs[name].append(round(steps(eng[name], a.steps), 4))
    for e in eng.values():
        e.close()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {"txns": n, "sigs": nsig, "nkeys": nkeys, "keys_decoded_on": decoded, "results_ok": ok, "ms_per_step": runs,
           "median_ms": med}
    if len(runs) == 2:
        res.update({"off_spread_ms": round(max(runs["off"]) - min(runs["off"]), 4),
                    "on_minus_off_median_ms": round(med["on"] - med["off"], 4),
                    "within_off_spread": bool(med["on"] - med["off"] <= max(runs["off"]) - min(runs["off"]))})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not a.nkeys and not res.get("within_off_spread", True):
        sys.exit("FAIL: the all-distinct batch loses more than the spread between the off runs")


if __name__ == "__main__":
    main()
