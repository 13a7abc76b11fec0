#!/usr/bin/env python3
"""What a verdict on complete FEC sets costs through the whole tree against one proof walk per shred.
--sets complete sets (1,024 and 4,096 are the recorded sizes) of 32 data and 32 code shreds, proof depth 6, chained,
one leader, each shred 42 bytes behind a 64-byte boundary of an arena in HBM (32 distinct sets, repeated; every
eighth distinct set carries a broken signature).  Two arms on one context, codes and roots checked in every run:

  a  fdgpu_ed25519_verify_shreds_device    every shred's root from the proof it carries (STRICT_LEAF), the set's first
                                           shred keyed: 64 leaves and 384 merges a set
  b  fdgpu_ed25519_verify_fec_sets_device  the set's tree with CHECK_PROOFS and a key: 64 leaves and 63 merges

Each run is the mean of --steps calls between two device synchronisations on the host clock, after two warm-up calls
of each arm; --runs runs per arm, alternating a b / b a.  Reports medians, spreads and the SHA-256 compressions per
shred of both arms.  With --kernel-ms (fd_fec_tree_kernel's own time from a separate rocprofv3 --kernel-trace --stats
run) it also reports that.

usage: tools/fec_ab.py [--sets N] [--runs R] [--steps S] [--only a|b] [--kernel-ms T] [--out FILE]
Prints one JSON line and writes it to --out.  Exits non-zero on a wrong code or root.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARM = 2
DISTINCT = 32
DATA, CODE = 32, 32
STRIDE, LEAD = 1280, 42


def blocks(n_bytes):
    return (n_bytes + 9 + 63) >> 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--kernel-ms", type=float, default=0.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine
    from tests import fec_model as fm
    from tools.shreds_ab import signer
    sets, per = a.sets, DATA + CODE
    n = sets * per
    pub, sign = signer(b"fec_ab leader")
    m = min(DISTINCT, sets)
    rows = np.zeros((m * per, STRIDE), np.uint8)
    roots, full = [], []
    for i in range(m):
        shreds = fm.build_set(DATA, CODE, 1, 9000 + i, sign)
        roots.append(fm.tree([fm.leaf_hash(s) for s in shreds])[0])
        for j, s in enumerate(shreds):
            if i % 8 == 5:
                s = s[:35] + bytes([s[35] ^ 1]) + s[36:]           # a broken signature, the same in every member
            rows[i * per + j, LEAD:LEAD + len(s)] = np.frombuffer(s, np.uint8)
            full.append(len(s))
    arena_sz = n * STRIDE
    arena = np.zeros(arena_sz + engine.ARENA_SLACK, np.uint8)
    arena[:arena_sz].reshape(sets // m, m * per * STRIDE)[:] = rows.reshape(-1)
    idx = np.arange(n)
    sdesc = np.zeros(n, engine.SHRED_DESC_DTYPE)
    sdesc["off"] = idx * STRIDE + LEAD
    sdesc["sz"] = np.array(full, np.uint16)[idx % (m * per)]
    sdesc["key_idx"] = np.where(idx % per == 0, 0, engine.FDGPU_SHRED_NO_SIG)
    sdesc["sig_idx"] = idx // per
    sdesc["flags"] = engine.FDGPU_SHRED_STRICT_LEAF
    fdesc = np.zeros(sets, engine.FEC_DESC_DTYPE)
    fdesc["member0"] = np.arange(sets) * per
    fdesc["cnt"] = per
    fdesc["key_idx"] = 0
    fdesc["sig_idx"] = np.arange(sets)
    fdesc["flags"] = engine.FDGPU_FEC_CHECK_PROOFS
    member = np.zeros(n, engine.FEC_MEMBER_DTYPE)
    member["off"] = sdesc["off"]
    broken = (np.arange(sets) % m) % 8 == 5
    want_roots = np.frombuffer(b"".join(roots), np.uint8).reshape(m, 32)

    eng = fa.Engine(device=0, max_txn=max(sets, 64), max_sig=max(sets, 64))
    eng.shreds_prepare(n, 1)
    eng.fec_prepare(sets, n, 1)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d_arena = torch.from_numpy(arena).cuda()
    d_sdesc = torch.from_numpy(sdesc.view(np.uint8)).cuda()
    d_fdesc = torch.from_numpy(fdesc.view(np.uint8)).cuda()
    d_member = torch.from_numpy(member.view(np.uint8)).cuda()
    d_keys = torch.from_numpy(np.frombuffer(pub, np.uint8).copy()).cuda()
    d_out = torch.empty(n, dtype=torch.int8, device="cuda")
    d_root = torch.empty((n, 32), dtype=torch.uint8, device="cuda")

    def call(arm):
        if arm == "a":
            eng.verify_shreds_device(d_arena.data_ptr(), arena_sz, d_sdesc.data_ptr(), n, sets, d_keys.data_ptr(), 1,
                                     d_out.data_ptr(), d_root.data_ptr(), st)
        else:
            eng.verify_fec_sets_device(d_arena.data_ptr(), arena_sz, d_fdesc.data_ptr(), sets, d_member.data_ptr(), n, sets,
                                       d_keys.data_ptr(), 1, None, d_out.data_ptr(), d_root.data_ptr(), st)

    def good(arm):
        out = d_out.cpu().numpy()
        if arm == "a":
            first = out[::per]
            rest = np.delete(out, np.arange(0, n, per))
            r = d_root[:m * per].cpu().numpy().reshape(m, per, 32)
            return bool((first[~broken] == 0).all() and (first[broken] != 0).all() and not rest.any()
                        and (r == want_roots[:, None, :]).all())
        r = d_root[:sets].cpu().numpy().reshape(sets // m, m, 32)
        return bool((out[:sets][~broken] == 0).all() and (out[:sets][broken] != 0).all() and (r == want_roots[None]).all())

    def steps(arm, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            call(arm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    arms = [x for x in ("a", "b") if not a.only or x == a.only]
    ok = True
    for _ in range(WARM):
        for arm in arms:
            d_out.fill_(7)
            d_root.fill_(0x5A)
            steps(arm, 1)
            ok = ok and good(arm)
    runs = {arm: [] for arm in arms}
    for r in range(a.runs):
        for arm in (arms, arms[::-1])[r & 1]:
            d_out.fill_(7)
            d_root.fill_(0x5A)
            runs[arm].append(round(steps(arm, a.steps), 4))
            ok = ok and good(arm)
    eng.close()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
    # compressions: the leaf's blocks over 26 + ( moff - 64 ) bytes, two per merge
    leaf = (DATA * blocks(26 + 1203 - 120 - 64) + CODE * blocks(26 + 1228 - 120 - 64)) / per
    comp = {"a": leaf + 2 * 6, "b": leaf + 2 * (per - 1) / per}
    res = {"sets": sets, "shreds": n, "depth": 6, "broken_sets": int(broken.sum()), "steps": a.steps, "results_ok": ok,
           "ms_per_call": runs, "median_ms": med, "spread_ms": spread,
           "compressions_per_shred": {k: round(v, 3) for k, v in comp.items()}, "compressions_b_over_a": round(comp["b"] / comp["a"], 3)}
    if "a" in runs and "b" in runs:
        res["b_over_a"] = round(med["b"] / med["a"], 3)
    if a.kernel_ms:
        res["tree_kernel_ms"] = a.kernel_ms
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("FAIL: wrong codes or roots")


if __name__ == "__main__":
    main()
