#!/usr/bin/env python3
"""What deriving the Merkle roots of a batch of shreds costs.  --n built shreds (65,536 and 2,048 are the
recorded sizes) of proof depth 6, half data and half code, one leader key, one keyed shred per 32, each 42 bytes
behind a 64-byte boundary of an arena in HBM (2,048 distinct shreds, repeated).  Two arms on one context, codes
checked in every run:

  d  fdgpu_ed25519_verify_sigs_device    the parent's call over the same signatures with the roots already in HBM as
                                         32-byte messages: the floor
  c  fdgpu_ed25519_verify_shreds_device  the roots derived on the GPU

Each run is the mean of --steps calls between two device synchronisations on the host clock, after two warm-up calls
of each arm; --runs runs per arm, alternating c d / d c.  Reports medians and spreads, c - d as the cost of the roots,
and the least time the bytes fd_shred_root_kernel reads and writes take at the 6.29 TB/s measured copy rate.  With
--kernel-ms (fd_shred_root_kernel's own time from a separate rocprofv3 --kernel-trace --stats run) and
--valu-per-shred (its vector instructions per shred, counted in the ISA) it also reports that time as a multiple of
both bounds and names the larger.

usage: tools/shreds_ab.py [--n N] [--runs R] [--steps S] [--only c|d] [--kernel-ms T] [--valu-per-shred V] [--out FILE]
Prints one JSON line and writes it to --out.  Exits non-zero on a wrong code.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29                      # MI355X measured float4 copy rate, TB/s
VALU_PER_S = 256 * 4 * 2.4e9 / 2     # wave-instructions a second: 256 CUs x 4 SIMDs, one per 2 cycles at 2.4 GHz
WARM = 2
DISTINCT = 2048
STRIDE, LEAD = 1280, 42

# a textbook ed25519 signer, for the 64 distinct keyed shreds
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P


def _add(a, b):
    x1, y1, z1, t1 = a
    x2, y2, z2, t2 = b
    A, B, C, Dd = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P, t1 * 2 * D * t2 % P, z1 * 2 * z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return E * F % P, G * H % P, F * G % P, E * H % P


def _mul(s, p):
    q = (0, 1, 1, 0)
    while s:
        if s & 1:
            q = _add(q, p)
        p = _add(p, p)
        s >>= 1
    return q


def _enc(p):
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def _base():
    y = 4 * pow(5, P - 2, P) % P
    xx = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(xx, (P + 3) // 8, P)
    if (x * x - xx) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if x & 1:
        x = P - x
    return x, y, 1, x * y % P


def signer(seed: bytes):
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    B = _base()
    pub = _enc(_mul(a, B))

    def sign(msg: bytes) -> bytes:
        r = int.from_bytes(hashlib.sha512(h[32:] + msg).digest(), "little") % L
        R = _enc(_mul(r, B))
        k = int.from_bytes(hashlib.sha512(R + pub + msg).digest(), "little") % L
        return R + ((r + k * a) % L).to_bytes(32, "little")
    return pub, sign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--kernel-ms", type=float, default=0.0)
    ap.add_argument("--valu-per-shred", type=float, default=0.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import firedancer_amd as fa
    from firedancer_amd import engine
    from tests import shred_model as sm
    n = a.n
    assert n % 32 == 0
    pub, sign = signer(b"shreds_ab leader")
    m = min(DISTINCT, n)
    rows = np.zeros((m, STRIDE), np.uint8)
    roots, full = [], []
    for i in range(m):
        kind = (0x90, 0x60)[i & 1]                             # half data, half code
        keyed = i % 32 == 0
        s = bytearray(sm.build(kind, 6, 1 + i % 63, i, sign if keyed else (lambda r: bytes(64))))
        if keyed and i % 512 == 256:
            s[35] ^= 1                                         # a few broken signatures
        rows[i, LEAD:LEAD + len(s)] = np.frombuffer(bytes(s), np.uint8)
        roots.append(sm.outcome(bytes(s), len(s))[1])
        full.append(len(s))
    arena_sz = n * STRIDE
    arena = np.zeros(arena_sz + engine.ARENA_SLACK, np.uint8)
    arena[:arena_sz].reshape(n // m, m * STRIDE)[:] = rows.reshape(-1)
    idx = np.arange(n)
    desc = np.zeros(n, engine.SHRED_DESC_DTYPE)
    desc["off"] = idx * STRIDE + LEAD
    desc["sz"] = np.array(full, np.uint16)[idx % m]
    desc["key_idx"] = np.where(idx % 32 == 0, 0, engine.FDGPU_SHRED_NO_SIG)
    desc["sig_idx"] = idx // 32
    nsig = n // 32
    broken = (idx % 32 == 0) & ((idx % m) % 512 == 256)
    # arm d: the same signatures over the roots, sig | key | root every 128 bytes
    flat = np.zeros(nsig * 128 + engine.ARENA_SLACK, np.uint8)
    rec = flat[:nsig * 128].reshape(nsig, 128)
    src = (np.arange(nsig) * 32) % m
    rec[:, 0:64] = rows[src, LEAD:LEAD + 64]
    rec[:, 64:96] = np.frombuffer(pub, np.uint8)
    rec[:, 96:128] = np.frombuffer(b"".join(roots[i] for i in src), np.uint8).reshape(nsig, 32)
    sdesc = np.zeros(nsig, engine.SIG_DESC_DTYPE)
    sdesc["sig_off"] = np.arange(nsig) * 128
    sdesc["pub_off"] = sdesc["sig_off"] + 64
    sdesc["msg_off"] = sdesc["sig_off"] + 96
    sdesc["msg_sz"] = 32

    eng = fa.Engine(device=0, max_txn=max(nsig, 64), max_sig=max(nsig, 64))
    eng.shreds_prepare(n, 1)
    eng.sigs_prepare(136 * nsig)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    d_arena = torch.from_numpy(arena).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    d_keys = torch.from_numpy(np.frombuffer(pub, np.uint8).copy()).cuda()
    d_flat = torch.from_numpy(flat).cuda()
    d_sdesc = torch.from_numpy(sdesc.view(np.uint8)).cuda()
    d_out = torch.empty(n, dtype=torch.int8, device="cuda")
    d_root = torch.empty((n, 32), dtype=torch.uint8, device="cuda")

    def call(arm):
        if arm == "c":
            eng.verify_shreds_device(d_arena.data_ptr(), arena_sz, d_desc.data_ptr(), n, nsig, d_keys.data_ptr(), 1,
                                     d_out.data_ptr(), d_root.data_ptr(), st)
        else:
            eng.verify_sigs_device(d_flat.data_ptr(), nsig * 128, d_sdesc.data_ptr(), nsig, 32 * nsig, d_out.data_ptr(), st)

    def good(arm):
        out = d_out.cpu().numpy()
        if arm == "c":
            ok = (out[~broken] == 0).all() and (out[broken] != 0).all()
            r = d_root[:m].cpu().numpy()
            return bool(ok and r.tobytes() == b"".join(roots))
        sb = broken[::32]
        return bool((out[:nsig][~sb] == 0).all() and (out[:nsig][sb] != 0).all())

    def steps(arm, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            call(arm)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    arms = [x for x in ("c", "d") if not a.only or x == a.only]
    ok = True
    for _ in range(WARM):
        for arm in arms:
            d_out.fill_(7)
            steps(arm, 1)
            ok = ok and good(arm)
    runs = {arm: [] for arm in arms}
    for r in range(a.runs):
        for arm in (arms, arms[::-1])[r & 1]:
            d_out.fill_(7)
            runs[arm].append(round(steps(arm, a.steps), 4))
            ok = ok and good(arm)
    eng.close()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
    # fd_shred_root_kernel: the descriptor, the header fields' dwords, the hashed bytes from 26 in front of byte 64 on,
    # the proof; a keyed shred's signature and key; written: the root, the flag, a keyed shred's slot and descriptor
    moff = np.array(full, np.int64)[idx % m] - 120
    moved = int((16 + 28 + (moff - 38) + 120 + 32 + 1).sum()) + nsig * (64 + 32 + 128 + 16)
    floor_ms = moved / (COPY_TBS * 1e12) * 1e3
    res = {"shreds": n, "signatures": nsig, "depth": 6, "broken": int(broken.sum()), "steps": a.steps, "results_ok": ok,
           "ms_per_call": runs, "median_ms": med, "spread_ms": spread, "root_kernel_bytes": moved,
           "bytes_floor_ms_at_6.29TBs": round(floor_ms, 5)}
    if "c" in runs and "d" in runs:
        res["roots_ms"] = round(med["c"] - med["d"], 4)
    if a.kernel_ms:
        res["root_kernel_ms"] = a.kernel_ms
        res["kernel_over_bytes_floor"] = round(a.kernel_ms / floor_ms, 2)
        if a.valu_per_shred:
            valu_ms = (n / 64) * a.valu_per_shred / VALU_PER_S * 1e3
            res["valu_per_shred"] = a.valu_per_shred
            res["valu_floor_ms"] = round(valu_ms, 5)
            res["kernel_over_valu_floor"] = round(a.kernel_ms / valu_ms, 2)
            res["bound_by"] = "VALU issue" if valu_ms > floor_ms else "bytes"
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("FAIL: wrong codes")


if __name__ == "__main__":
    main()
