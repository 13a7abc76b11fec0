#!/usr/bin/env python3
"""What verifying signatures in place costs: 131,072 records with 1,167-byte messages by 1,024 keys --
bench.py's transactions (BASELINE configs[1]), a tenth of them invalid, at the batch size of DESIGN 19's row (a) --
named by per-signature descriptors over the transactions where they lie.  Four arms on one context, codes checked
in every run:

  a  fdgpu_ed25519_verify_many_host     three host pointer arrays, every byte copied by the host and uploaded
  b  fdgpu_ed25519_verify_sigs_host     the arena in a registered host region: packed by the GPU over PCIe
  c  fdgpu_ed25519_verify_sigs_device   the arena in HBM
  d  fdgpu_ed25519_verify_txns_device   the same records already packed in HBM: the floor

Each run is the mean of --steps calls between two device synchronisations on the host clock, after warm-up calls of
every arm; --runs runs per arm, the arms alternating (a b c d, d c b a, ...).  Reports medians and spreads, the pack
cost c - d against the bytes the pack kernels read and write at the 6.29 TB/s measured copy rate, and whether b's
slowest run beats a's fastest by more than three times a's spread.

usage: tools/sigs_ab.py [--runs R] [--steps S] [--arms a,b,c,d] [--n N] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/sigs/ab.json).  Exits non-zero on a wrong code or when
b does not beat a (with both arms run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29                      # MI355X measured float4 copy rate, TB/s
WARM = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--arms", default="a,b,c,d")
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--out", default=os.path.join("profiles", "sigs", "ab.json"))
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine, synth
    L = fa.load_library()
    n = a.n
    payload, tdesc, expect, nsig = synth.make_batch(n, synth.LARGE_NOOP, invalid_frac=0.1, threads=16)
    assert nsig == n
    off = tdesc["payload_off"].astype(np.int64)
    desc = np.zeros(n, engine.SIG_DESC_DTYPE)
    desc["sig_off"] = off + tdesc["signature_off"]
    desc["pub_off"] = off + tdesc["acct_addr_off"]
    desc["msg_off"] = off + tdesc["message_off"]
    desc["msg_sz"] = tdesc["payload_sz"].astype(np.int64) - tdesc["message_off"]
    msg_sz = int(desc["msg_sz"][0])
    assert (desc["msg_sz"] == msg_sz).all()
    msg_bytes = n * msg_sz
    stride = (96 + msg_sz + 7) // 8 * 8
    # the arena: the transactions, page-aligned, with the slack behind them; registered for arm b
    arena_sz = int(off[-1]) + int(tdesc["payload_sz"][-1])
    raw = np.zeros(arena_sz + engine.ARENA_SLACK + 8192, np.uint8)
    o = (-raw.ctypes.data) % 4096
    arena = raw[o:o + arena_sz + engine.ARENA_SLACK]
    arena[:arena_sz] = payload[:arena_sz]
    engine.host_register(arena)
    # arm a: pointers into a plain copy of the same bytes
    plain = payload.copy()
    base = plain.ctypes.data
    p_sig = (base + desc["sig_off"].astype(np.uint64)).astype(np.uint64)
    p_pub = (base + desc["pub_off"].astype(np.uint64)).astype(np.uint64)
    p_msg = (base + desc["msg_off"].astype(np.uint64)).astype(np.uint64)
    szs = desc["msg_sz"].astype(np.uint64)
    # arm d: the records as the pack kernel lays them out
    packed = np.zeros(n * stride + 1024, np.uint8)
    rows = packed[:n * stride].reshape(n, stride)
    ts = int(off[1] - off[0])                                 # (the generator's records: one stride, one shape)
    so, ao, mo = (int(tdesc[k][0]) for k in ("signature_off", "acct_addr_off", "message_off"))
    assert (off == np.arange(n) * ts).all() and all((tdesc[k] == tdesc[k][0]).all()
                                                    for k in ("signature_off", "acct_addr_off", "message_off"))
    src = plain[:n * ts].reshape(n, ts)
    rows[:, 0:64] = src[:, so:so + 64]
    rows[:, 64:96] = src[:, ao:ao + 32]
    rows[:, 96:96 + msg_sz] = src[:, mo:mo + msg_sz]
    pdesc = np.zeros(n, engine.DESC_DTYPE)
    pdesc["payload_off"] = np.arange(n, dtype=np.int64) * stride
    pdesc["sig_base"] = np.arange(n)
    pdesc["payload_sz"], pdesc["message_off"], pdesc["acct_addr_off"], pdesc["sig_cnt"] = 96 + msg_sz, 96, 64, 1

    eng = fa.Engine(device=0, max_txn=n, max_sig=n, max_payload=n * (stride + 8))
    eng.sigs_prepare(104 * n + msg_bytes)             # the bound the device form checks msg_bytes against
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d_arena = torch.from_numpy(arena).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    d_packed = torch.from_numpy(packed).cuda()
    d_pdesc = torch.from_numpy(pdesc.view(np.uint8)).cuda()
    d_out = torch.empty(n, dtype=torch.int8, device="cuda")
    h_out = np.zeros(n, np.int8)

    def call(arm):
        if arm == "a":
            rc = L.fdgpu_ed25519_verify_many_host(eng.ctx, p_msg.ctypes.data, szs.ctypes.data, p_sig.ctypes.data,
                                                  p_pub.ctypes.data, n, h_out.ctypes.data)
            assert rc == 0, engine.last_error()
        elif arm == "b":
            rc = L.fdgpu_ed25519_verify_sigs_host(eng.ctx, arena.ctypes.data, arena_sz, desc.ctypes.data, n,
                                                  h_out.ctypes.data)
            assert rc == 0, engine.last_error()
        elif arm == "c":
            eng.verify_sigs_device(d_arena.data_ptr(), arena_sz, d_desc.data_ptr(), n, msg_bytes, d_out.data_ptr(), st)
        else:
            eng.verify_txns_device(d_packed.data_ptr(), d_pdesc.data_ptr(), n, n, d_out.data_ptr(), None, st)

    def codes(arm):
        return h_out if arm in "ab" else d_out.cpu().numpy()

    def steps(arm, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            call(arm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    arms = a.arms.split(",")
    ok = True
    for _ in range(WARM):
        for arm in arms:
            h_out[:] = 7
            d_out.fill_(7)
            steps(arm, 1)
            ok = ok and bool((codes(arm) == expect).all())
    runs = {arm: [] for arm in arms}
    for r in range(a.runs):
        for arm in (arms, arms[::-1])[r & 1]:
            h_out[:] = 7
            d_out.fill_(7)
            runs[arm].append(round(steps(arm, a.steps), 4))
            ok = ok and bool((codes(arm) == expect).all())
    eng.close()
    engine.host_unregister(arena)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
    res = {"records": n, "msg_sz": msg_sz, "keys": 1024, "invalid": int((expect != 0).sum()), "steps": a.steps,
           "results_ok": ok, "ms_per_call": runs, "median_ms": med, "spread_ms": spread}
    fail = [] if ok else ["wrong codes"]
    if "a" in runs and "b" in runs:
        margin = min(runs["a"]) - max(runs["b"])
        res["a_fastest_minus_b_slowest_ms"] = round(margin, 4)
        res["b_beats_a_by_3_spreads"] = bool(margin > 3 * spread["a"])
        if not res["b_beats_a_by_3_spreads"]:
            fail.append("b does not beat a by more than three times a's spread")
    if "c" in runs and "d" in runs:
        # read: the three ranges and the descriptor twice (size, pack), the flags and offsets; written: the packed record,
        # its transaction descriptor, offset and flag
        moved = n * ((96 + msg_sz) + stride + 16 * 3 + 16 + 4 * 2 + 3)
        floor_ms = moved / (COPY_TBS * 1e12) * 1e3
        res["pack_ms"] = round(med["c"] - med["d"], 4)
        res["pack_bytes"] = moved
        res["pack_floor_ms_at_6.29TBs"] = round(floor_ms, 4)
        res["pack_over_floor"] = round((med["c"] - med["d"]) / floor_ms, 2)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if fail:
        sys.exit("FAIL: " + "; ".join(fail))


if __name__ == "__main__":
    main()
