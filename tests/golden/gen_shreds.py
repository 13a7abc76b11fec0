#!/usr/bin/env python3
"""Generate tests/golden/shreds.npz from the REFERENCE shred code.  Run by hand in the build container only (needs
/root/reference and oracle/_ref); no test and no build step runs it.

Contents:

* ``shreds`` (186, 1228) / ``shred_sz``: the shreds of the reference's own fixtures
  src/disco/shred/fixtures/chained-5XDm....ar (122) and resigned-AmKF....ar (64), data files stored verbatim (a
  data shred's 1,203 bytes zero-padded), ``shred_key`` the index of each one's leader in ``keys``;
* ``keys`` (5, 32): the two leaders (from the archives' names), then a key that does not decode, a small-order key
  and a valid key that signed nothing here;
* cases ``c_base, c_off, c_len, c_bytes, c_sz, c_key``: shred c_base with c_len bytes of c_bytes written at c_off,
  handed over as c_sz bytes, checked against key c_key.  The first 186 cases are the originals;
* for every case, from the reference compiled from its own sources: ``c_parse`` (fd_shred_parse != NULL),
  ``c_merkle`` (fd_shred_merkle_root's return value on a fresh tree; 0 where it was not called: no parse, or a legacy
  variant, which src/disco/shred/fd_fec_resolver.c:360-363 rejects before it), ``c_root`` (32 bytes, zero where
  c_merkle is 0) and ``c_code`` (2, n): fd_ed25519_verify( root, 32, shred, key ) of the AVX-512 build and of the
  portable build (zero where c_merkle is 0).

The parse and root results come from a small driver of ours, compiled here with plain gcc in a temporary directory
against the reference's fd_shred.c, fd_bmtree.c and fd_sha256.c with the flags of oracle/Makefile's REF_NOARCH; the
verify codes from oracle/_ref's two builds.  Only data is written.
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.oracle import Reference, build  # noqa: E402

REF = "/root/reference/src"
ARCHIVES = ("chained-5XDmMEZpXM2GBXNjhgRCti4qLGeFQvx4RnzWeRgfupYk.ar", "resigned-AmKFVSAQ7DyhiW94pWfDexYDCSn8GB6SG2zbQqLhuufU.ar")
REC = 2048          # a driver record: u64 sz, then the bytes, zero-padded

DRIVER = r"""
#include "ballet/shred/fd_shred.h"
#include "ballet/bmtree/fd_bmtree.h"
#include <stdio.h>
#include <string.h>
/* stdin: records of 2048 bytes (u64 sz, the shred); stdout: 34 bytes a record: parsed, merkle ok, root */
int main( void ) {
  static uchar rec[ 2048 ] __attribute__((aligned(8)));
  static uchar mem[ 1<<20 ] __attribute__((aligned(128)));
  while( fread( rec, 1, 2048, stdin ) == 2048 ) {
    ulong sz; memcpy( &sz, rec, 8 );
    uchar out[ 34 ]; memset( out, 0, 34 );
    fd_shred_t const * s = fd_shred_parse( rec + 8, sz );
    if( s ) {
      out[0] = 1;
      if( s->variant != 0xa5 && s->variant != 0x5a ) {
        fd_bmtree_node_t root[1]; memset( root, 0, sizeof(root) );
        if( fd_shred_merkle_root( s, mem, root ) ) { out[1] = 1; memcpy( out + 2, root->hash, 32 ); }
      }
    }
    fwrite( out, 1, 34, stdout );
  }
  return 0;
}
"""

AL = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
P = 2**255 - 19
D = (-121665 * pow(121666, P - 2, P)) % P


def b58(s):
    n = 0
    for c in s:
        n = n * 58 + AL.index(c)
    return n.to_bytes(32, "big")


def decodes(y):
    xx = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(xx, (P + 3) // 8, P)
    return (x * x - xx) % P == 0 or (x * x + xx) % P == 0


def members(path):
    b = open(path, "rb").read()
    assert b[:8] == b"!<arch>\n"
    o, out = 8, []
    while o < len(b):
        sz = int(b[o + 48:o + 58])
        out.append(b[o + 60:o + 60 + sz])
        o += 60 + sz + (sz & 1)
    return out


def make_cases(shreds, key_of):
    """[(base, off, bytes, sz, key)]: the originals, then the mutants"""
    cases = [(i, 0, b"", len(s), key_of[i]) for i, s in enumerate(shreds)]
    picks = {}
    for i, s in enumerate(shreds):
        picks.setdefault(s[0x40], [])
        if len(picks[s[0x40]]) < 2 and (not picks[s[0x40]] or i - picks[s[0x40]][0] > 3):
            picks[s[0x40]].append(i)
    assert sorted(picks) == [0x65, 0x66, 0x76, 0x95, 0x96, 0xb6] and all(len(v) == 2 for v in picks.values())
    for variant, idxs in sorted(picks.items()):
        t, d = variant & 0xf0, variant & 0xf
        data = t in (0x80, 0x90, 0xb0)
        resigned = t in (0xb0, 0x70)
        full = 1203 if data else 1228
        moff = full - 20 * d - 64 * resigned
        for i in idxs:
            s, k = shreds[i], key_of[i]

            def mut(off, new, sz=full, key=k):
                cases.append((i, off, bytes(new), sz, key))

            def flip(off, bit=0x10):
                mut(off, [s[off] ^ bit])

            for off in (64, (64 + moff) // 2, moff - 1):                   # the Merkle-protected bytes
                flip(off)
            for lvl in range(d):                                            # every proof node
                flip(moff + 20 * lvl + (7 * lvl) % 20)
            flip(5), flip(40)                                               # R, S
            L = 2**252 + 27742317777372353535851937790883648493
            S = int.from_bytes(s[32:64], "little")
            if S + L < 2**256:
                mut(32, (S + L).to_bytes(32, "little"))                     # S + L
            flip(moff - 32 + 9, 0xff)                                       # the chained root (inside the leaf)
            if resigned:
                flip(full - 64 + 11, 0xff)                                  # the retransmitter's signature: not covered
            for nd in (d - 1, d + 1, 10, 11, 12, 13, 14, 15):
                mut(0x40, [t | nd])
            for v in (0xa5, 0x5a, 0x00):
                mut(0x40, [v])
            for sz in (0, 87, full - 1, full, full + 7):
                mut(0, b"", sz)
            for key in (1 - k, 2, 3, 4):                                    # the other leader, no decode, small order, unused
                mut(0, b"", full, key)
            u16 = lambda v: struct.pack("<H", v)
            u32 = lambda v: struct.pack("<I", v & 0xFFFFFFFF)
            if data:
                slot, idx = struct.unpack_from("<QI", s, 0x41)
                fec, = struct.unpack_from("<I", s, 0x4f)
                trailer = 20 * d + 32 + 64 * resigned
                for v in (87, 88, 1203 - trailer, 1204 - trailer):         # size
                    mut(0x56, u16(v))
                for v in (0x80, 0xBF, 0x40, 0xC0, 0x00):                    # flags
                    mut(0x55, [v])
                # parent_off against the slot: slot 10, 1, 0 and 2 with parent_off on each side
                for sl, po in ((10, 9), (10, 10), (10, 11), (10, 0), (1, 1), (1, 0), (0, 0), (0, 1), (2, 1), (2, 2),
                               (0x10000, 0xFFFF), (0xFFFF, 0xFFFF)):
                    mut(0x41, struct.pack("<Q", sl) + s[0x49:0x53] + u16(po))
                for v in (fec, fec - 1, fec + 511, fec + 512, fec + (1 << d) - 1, fec + (1 << d)):   # idx
                    mut(0x49, u32(v))
            else:
                idx, = struct.unpack_from("<I", s, 0x49)
                dc, cc, ci = struct.unpack_from("<HHH", s, 0x53)
                for v in (cc - 1, cc):                                      # code.idx against code_cnt
                    mut(0x57, u16(v))
                mut(0x49, u32(ci)), mut(0x49, u32(max(ci, 1) - 1))         # ... and against idx
                mut(0x53, u16(0)), mut(0x53, u16(1))                        # data_cnt
                mut(0x55, u16(0)), mut(0x55, u16(ci + 1))                   # code_cnt
                mut(0x53, u16(1) + u16(255) + u16(1)), mut(0x53, u16(1) + u16(256) + u16(1))
                mut(0x53, u16(0) + u16(256) + u16(1)), mut(0x53, u16(0) + u16(257) + u16(1))
                mut(0x53, u16(128) + u16(128) + u16(1)), mut(0x53, u16(129) + u16(128) + u16(1))
                mut(0x53, u16(1) + u16(255) + u16(254)), mut(0x49, u32(300) + s[0x4d:0x53] + u16(1) + u16(255) + u16(254))
    return cases


def apply(shreds, case, width):
    base, off, new, sz, _ = case
    b = bytearray(shreds[base].ljust(width, b"\0"))
    b[off:off + len(new)] = new
    return bytes(b)


def main() -> None:
    build(ref=True)
    shreds, key_of, keys = [], [], []
    for a, name in enumerate(ARCHIVES):
        ms = members(os.path.join(REF, "disco/shred/fixtures", name))
        shreds += ms
        key_of += [a] * len(ms)
        keys.append(b58(name.split("-")[1].split(".")[0]))
    assert len(shreds) == 186 and all(len(s) in (1203, 1228) for s in shreds)
    y = 2
    while decodes(y):
        y += 1
    keys.append(y.to_bytes(32, "little"))                       # no point has this y
    keys.append((P - 1).to_bytes(32, "little"))                 # (0, -1): order 2
    ref = {"avx512": Reference("avx512"), "portable": Reference("portable")}
    keys.append(ref["portable"].public_from_private(bytes(range(32))))
    cases = make_cases(shreds, key_of)

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "shred_driver.c")
        with open(src, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "shred_driver")
        flags = ["-std=c17", "-fwrapv", "-O3", "-fPIC", "-ffunction-sections", "-fdata-sections", "-DFD_HAS_BACKTRACE=0",
                 "-I" + REF, "-pthread", "-DFD_HAS_DOUBLE=1", "-DFD_HAS_ALLOCA=1"]      # oracle/Makefile REF_NOARCH
        subprocess.run(["gcc"] + flags + ["-w", "-Wl,--gc-sections", "-o", exe, src, REF + "/ballet/shred/fd_shred.c",
                        REF + "/ballet/bmtree/fd_bmtree.c", REF + "/ballet/sha256/fd_sha256.c"], check=True)
        inp = b"".join(struct.pack("<Q", c[3]) + apply(shreds, c, REC - 8) for c in cases)
        res = subprocess.run([exe], input=inp, capture_output=True, check=True).stdout
    assert len(res) == 34 * len(cases)
    res = np.frombuffer(res, np.uint8).reshape(-1, 34)
    n = len(cases)
    parse, merkle, root = res[:, 0].copy(), res[:, 1].copy(), res[:, 2:].copy()
    code = np.zeros((2, n), np.int8)
    for i, c in enumerate(cases):
        if merkle[i]:
            sig = apply(shreds, c, 1228)[:64]
            for s, v in enumerate(("avx512", "portable")):
                code[s, i] = ref[v].verify(root[i].tobytes(), sig, keys[c[4]])
    assert parse[:186].all() and merkle[:186].all() and not code[:, :186].any(), "an original does not verify"
    blen = max(len(c[2]) for c in cases)
    np.savez_compressed(
        os.path.join(HERE, "shreds.npz"),
        shreds=np.frombuffer(b"".join(s.ljust(1228, b"\0") for s in shreds), np.uint8).reshape(-1, 1228),
        shred_sz=np.array([len(s) for s in shreds], np.uint16), shred_key=np.array(key_of, np.uint16),
        keys=np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32),
        c_base=np.array([c[0] for c in cases], np.uint16), c_off=np.array([c[1] for c in cases], np.uint16),
        c_len=np.array([len(c[2]) for c in cases], np.uint16),
        c_bytes=np.frombuffer(b"".join(c[2].ljust(blen, b"\0") for c in cases), np.uint8).reshape(-1, blen),
        c_sz=np.array([c[3] for c in cases], np.uint16), c_key=np.array([c[4] for c in cases], np.uint16),
        c_parse=parse, c_merkle=merkle, c_root=root, c_code=code)
    m = slice(186, n)
    print(f"{n - 186} mutants: parse fails {int((parse[m] == 0).sum())}, merkle fails "
          f"{int(((parse[m] == 1) & (merkle[m] == 0)).sum())}, verify codes avx512 "
          f"{dict(zip(*np.unique(code[0, m][merkle[m] == 1], return_counts=True)))} portable "
          f"{dict(zip(*np.unique(code[1, m][merkle[m] == 1], return_counts=True)))}")


if __name__ == "__main__":
    main()
