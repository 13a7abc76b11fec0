#!/usr/bin/env python3
"""Key mixes for the repeated-key walk: what the 64-doubling walk of hot signatures gains or
costs on batches other than the benchmark's.  Times fdgpu_ed25519_verify_txns_device on HBM-resident batches
of single-signature 1232-byte transactions with fdgpu_debug_opts_t.key_split on (0) and off (1), two
contexts of one build interleaved (on off off on ...), for three batches:

  distinct   every key distinct (nkeys = 7 n + 4: synth's signer index is (7 t + r) mod nkeys, r < 4): nothing is
             hot, and after its first batch the context only samples the keys -- the split may lose no more
             than the spread between the off runs;
  half       half the signatures from 1,024 keys, half from keys of their own, interleaved by blocks of 4,096;
  exact      every key at exactly FD_HOT_MIN = 8 signatures: the most high tables a batch can ask for.

usage: tools/keysplit_mix.py [--txns N] [--reps R] [--steps S] [--batches distinct,half,exact] [--modes on,off]
                             [--out FILE]
Prints one JSON line per batch: per run the mean ms per step, the hot keys and hot signatures the on context
counted (fdgpu_ed25519_hot_count), medians, the off runs' spread and on - off.  Exits non-zero when the
distinct batch loses more than the off runs' spread, or any code is wrong.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STRIDE = 1232
BLOCK = 4096


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


def make(synth, name, n):
    """(payload, desc, expect, nsig) of a named batch of n transactions."""
    if name == "distinct":
        return synth.make_batch(n, synth.LARGE_NOOP, seed=1234, threads=16, key_arr=keys_parallel(synth, 7 * n + 4, 99))
    if name == "exact":
        # synth's signer index is 7 t + r, r < 4: with 7 n + 4 table entries, entry i belongs to transaction i // 7
        # alone, so a table that repeats n / 8 keys gives transaction t the key t mod (n / 8), whatever r
        assert n % 8 == 0
        base = keys_parallel(synth, n // 8, 98)
        return synth.make_batch(n, synth.LARGE_NOOP, seed=1235, threads=16,
                                key_arr=base[(np.arange(7 * n + 4) // 7) % (n // 8)])
    if name == "half":
        h = n // 2
        pa, da, ea, na = synth.make_batch(h, synth.LARGE_NOOP, seed=1236, nkeys=1024, threads=16)
        pb, db, eb, nb = synth.make_batch(n - h, synth.LARGE_NOOP, seed=1237, threads=16,
                                          key_arr=keys_parallel(synth, 7 * (n - h) + 4, 97))
        assert na == h and nb == h and n % (2 * BLOCK) == 0
        # blocks of BLOCK transactions alternately from the two halves
        t = np.arange(n)
        from_b = ((t // BLOCK) & 1) == 1
        idx = (t // BLOCK >> 1) * BLOCK + t % BLOCK
        payload = np.zeros(n * STRIDE + 1024, np.uint8)
        rows = payload[: n * STRIDE].reshape(n, STRIDE)
        rows[~from_b] = pa[: h * STRIDE].reshape(h, STRIDE)[idx[~from_b]]
        rows[from_b] = pb[: h * STRIDE].reshape(h, STRIDE)[idx[from_b]]
        desc, expect = da[idx].copy(), ea[idx].copy()
        desc[from_b], expect[from_b] = db[idx[from_b]], eb[idx[from_b]]
        desc["payload_off"] = (t * STRIDE).astype(np.uint32)
        desc["sig_base"] = t.astype(np.uint32)
        return payload, desc, expect, n
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=4, help="interleaved runs per mode")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="distinct,half,exact")
    ap.add_argument("--modes", default="on,off", help="on,off (default), or one of them alone (for a kernel trace)")
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
        if name not in a.modes.split(","):
            continue
        engine.debug_set_opts(key_split=mode, key_fixed=1)   # (the fixed-base keys of DESIGN 16 off: tools/keyfixed_mix.py)
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
        hot = eng["on"].hot_count() if "on" in eng else None
        runs = {name: [] for name in eng}
        for r in range(a.reps):
            for name in (("on", "off"), ("off", "on"))[r & 1]:
                if name in eng:
                    runs[name].append(round(steps(eng[name], a.steps), 4))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        res = {"batch": bname, "txns": n, "sigs": nsig, "hot_keys_sigs_on": hot, "results_ok": ok, "ms_per_step": runs,
               "median_ms": med}
        if len(runs) == 2:
            spread = max(runs["off"]) - min(runs["off"])
            res.update({"off_spread_ms": round(spread, 4), "on_minus_off_median_ms": round(med["on"] - med["off"], 4),
                        "within_off_spread": bool(med["on"] - med["off"] <= spread)})
            if bname == "distinct" and not res["within_off_spread"]:
                fail.append("the all-distinct batch loses more than the spread between the off runs")
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
