#!/usr/bin/env python3
"""Key mixes for the pinned keys: what fdgpu_ed25519_set_pinned_keys gains where a batch holds a known key a
few dozen times, and what it costs where it cannot gain.  Times fdgpu_ed25519_verify_txns_device on HBM-resident
batches of single-signature 1232-byte transactions on two contexts of one build per row, one with 1,024 keys pinned
and one that never pinned, interleaved (pin nopin nopin pin ...), tools/keyfull_mix.py's way.  Each row repeats one
batch, after warm-up steps that let the context without pins claim and promote what it finds by itself:

  vote70      131,072 signatures, of every ten seven from the 1,024 pinned keys and three from keys of their own: a
              pinned key has about 90 signatures, below FD_FB_MIN, so without pins it is hot -- must win;
  vote70_1m   1,048,576 signatures of the same mix: here the 1,024 keys reach FD_FB_MIN by themselves, and the row
              shows what is left to win -- must win;
  distinct    131,072 signatures, every key distinct and none pinned, with 1,024 pins set: the cost of looking every
              representative up -- must not lose;
  flagship    bench.py's batch, 1,024 keys x 1,024 signatures, in the steady state: pinned against found by itself
              -- must not lose.

usage: tools/keypin_mix.py [--reps R] [--steps S] [--rows vote70,vote70_1m,distinct,flagship] [--modes pin,nopin]
                           [--out FILE]
Prints one JSON line per row.  Exits non-zero when a row that must win does not beat the unpinned median by more than
the unpinned runs' spread, when a row that must not lose is slower by more than that spread, or when any code is
wrong.
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

STRIDE = keysplit_mix.STRIDE
NPIN = 1024
SEED = 1234                          # bench.py's batch: synth.make_batch's default seed and its 1,024 signers
ROWS = {"vote70": 1 << 17, "vote70_1m": 1 << 20, "distinct": 1 << 17, "flagship": 1 << 20}
CTX = 1 << 20                        # every context's max_sig: 4,096 slots, a pin cap of 3,072
MUST_WIN = ("vote70", "vote70_1m")
WARM = 4


def make(synth, name, n, pool):
    """(payload, desc, expect, nsig) of a row's batch of n transactions; pool: the 1,024 signers that are pinned"""
    if name == "flagship":
        return synth.make_batch(n, synth.LARGE_NOOP, seed=SEED, threads=16, key_arr=pool)
    if name == "distinct":
        return synth.make_batch(n, synth.LARGE_NOOP, seed=1238, threads=16,
                                key_arr=keysplit_mix.keys_parallel(synth, 7 * n + 4, 96))
    t = np.arange(n)
    from_b = t % 10 >= 7             # of every ten transactions, seven by the pool and three by keys of their own
    na, nb = int((~from_b).sum()), int(from_b.sum())
    pa, da, ea, sa = synth.make_batch(na, synth.LARGE_NOOP, seed=1236, threads=16, key_arr=pool)
    pb, db, eb, sb = synth.make_batch(nb, synth.LARGE_NOOP, seed=1237, threads=16,
                                      key_arr=keysplit_mix.keys_parallel(synth, 7 * nb + 4, 97))
    assert sa == na and sb == nb
    idx = np.where(from_b, np.cumsum(from_b) - 1, np.cumsum(~from_b) - 1)
    payload = np.zeros(n * STRIDE + 1024, np.uint8)
    rows = payload[: n * STRIDE].reshape(n, STRIDE)
    rows[~from_b] = pa[: na * STRIDE].reshape(na, STRIDE)[idx[~from_b]]
    rows[from_b] = pb[: nb * STRIDE].reshape(nb, STRIDE)[idx[from_b]]
    desc, expect = np.zeros(n, da.dtype), np.zeros(n, ea.dtype)
    desc[~from_b], expect[~from_b] = da[idx[~from_b]], ea[idx[~from_b]]
    desc[from_b], expect[from_b] = db[idx[from_b]], eb[idx[from_b]]
    desc["payload_off"] = (t * STRIDE).astype(np.uint32)
    desc["sig_base"] = t.astype(np.uint32)
    return payload, desc, expect, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6, help="interleaved runs per context")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rows", default="vote70,vote70_1m,distinct,flagship")
    ap.add_argument("--modes", default="pin,nopin", help="pin,nopin (default), or one of them alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import synth
    fa.load_library()
    stream = torch.cuda.Stream()                 # a stream of its own: stream 0 means "the context's" to the engine
    st = stream.cuda_stream
    pool = synth.keys(NPIN, SEED ^ 0x5eed)
    pins = [synth.pubkey(pool, i) for i in range(NPIN)]
    lines, fail = [], []
    for row in a.rows.split(","):
        n = ROWS[row]
        payload, desc, expect, nsig = make(synth, row, n, pool)
        pd = torch.from_numpy(payload).cuda()
        dd = torch.from_numpy(desc.view(np.uint8)).cuda()
        to = torch.empty(n, dtype=torch.int8, device="cuda")
        # (contexts of a million signatures in every row: a context of 131,072 has 1,024 slots and pins 768 at most)
        eng = {name: fa.Engine(device=0, max_txn=CTX, max_sig=CTX) for name in a.modes.split(",")}
        pin_ms = 0.0
        if "pin" in eng:
            t0 = time.perf_counter()
            status = eng["pin"].set_pinned_keys(pins)
            pin_ms = (time.perf_counter() - t0) * 1e3
            assert (status == 0).all() and eng["pin"].pin_cap() >= NPIN

        def steps(e, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                e.verify_txns_device(pd.data_ptr(), dd.data_ptr(), n, nsig, to.data_ptr(), None, st)
            torch.cuda.synchronize()             # (the whole device: every stream's work is done)
            return (time.perf_counter() - t0) * 1e3 / k

        ok = True
        for k in range(WARM):
            for name in eng:
                steps(eng[name], 1)
                ok = ok and bool((to.cpu().numpy() == expect).all())
        runs = {name: [] for name in eng}
        for r in range(a.reps):
            for name in (list(eng), list(eng)[::-1])[r & 1]:
                runs[name].append(round(steps(eng[name], a.steps), 4))
                ok = ok and bool((to.cpu().numpy() == expect).all())
        med = {k: float(np.median(v)) for k, v in runs.items()}
        if len(eng) < 2:                         # one context alone: its steps, for a kernel trace
            print(json.dumps({"row": row, "txns": n, "results_ok": ok, "ms_per_step": runs, "median_ms": med}), flush=True)
            for e in eng.values():
                e.close()
            continue
        spread = max(runs["nopin"]) - min(runs["nopin"])
        gain = med["nopin"] - med["pin"]
        res = {"row": row, "txns": n, "set_pinned_keys_ms": round(pin_ms, 3),
               "counts_pin": {"pinned": eng["pin"].pinned_count(), "fixed": eng["pin"].fixed_count(),
                              "full": eng["pin"].ffull_count(), "hot": eng["pin"].hot_count(),
                              "hits_builds": eng["pin"].fcache_count(), "keys": eng["pin"].key_count()},
               "counts_nopin": {"pinned": eng["nopin"].pinned_count(), "fixed": eng["nopin"].fixed_count(),
                                "full": eng["nopin"].ffull_count(), "hot": eng["nopin"].hot_count(),
                                "hits_builds": eng["nopin"].fcache_count(), "keys": eng["nopin"].key_count()},
               "results_ok": ok, "ms_per_step": runs, "median_ms": med, "nopin_spread_ms": round(spread, 4),
               "pin_minus_nopin_median_ms": round(-gain, 4), "pin_over_nopin": round(med["pin"] / med["nopin"], 4),
               "within_nopin_spread": bool(-gain <= spread), "wins_by_more_than_nopin_spread": bool(gain > spread)}
        if row in MUST_WIN and not res["wins_by_more_than_nopin_spread"]:
            fail.append(f"{row} does not win by more than the spread between the unpinned runs")
        if row not in MUST_WIN and not res["within_nopin_spread"]:
            fail.append(f"{row} loses more than the spread between the unpinned runs")
        if not ok:
            fail.append(f"{row}: wrong codes")
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
