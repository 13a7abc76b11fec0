#!/usr/bin/env python3
"""Generate tests/golden/fec_trees.npz from the REFERENCE tree code.  Run by hand in the build container only (needs
/root/reference); no test and no build step runs it.

For every leaf count n of tests/fec_model.py's SIZES one consistent set is built by fec_model.build_set from a recorded
(data_cnt, code_cnt, class, seed) and handed to a small driver of ours, compiled here with plain gcc in a temporary
directory against the reference's fd_bmtree.c, fd_sha256.c and fd_shred.c with the flags of oracle/Makefile's
REF_NOARCH.  The driver parses each shred (fd_shred_parse), hashes its leaf as the resolver and the shredder do
(fd_bmtree_hash_leaf over [64, fd_shred_merkle_off) with the long prefix), builds the tree (fd_bmtree_commit_init with
20-byte nodes, fd_bmtree_commit_append, fd_bmtree_commit_fini) and asks for every leaf's proof (fd_bmtree_get_proof).

Contents: ``n, data_cnt, code_cnt, cls, seed`` (one entry per set), ``depth`` (fd_bmtree_depth( n ) - 1), ``first``
(index of each set's leaf 0 in ``leaves``), ``leaves`` (sum n, 32), ``root`` (sets, 32) and ``proofs`` (sum n, 160):
leaf j's 20 * depth proof bytes, zero-padded.  Only data is written.
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
from tests import fec_model as fm  # noqa: E402

REF = "/root/reference/src"

DRIVER = r"""
#include "ballet/shred/fd_shred.h"
#include "ballet/bmtree/fd_bmtree.h"
#include <stdio.h>
#include <string.h>
/* stdin: sets: u64 n, then n records of 1232 bytes (u32 sz, the shred); stdout per set: u64 depth, n leaves of 32
   bytes, the root, n proofs of 160 bytes */
int main( void ) {
  static uchar rec[ 1232 ] __attribute__((aligned(8)));
  static uchar mem[ 1<<20 ] __attribute__((aligned(128)));
  static fd_bmtree_node_t leaf[ 256 ];
  ulong n;
  while( fread( &n, 8, 1, stdin ) == 1 ) {
    if( n < 1 || n > 256 ) return 2;
    for( ulong j=0; j<n; j++ ) {
      if( fread( rec, 1, 1232, stdin ) != 1232 ) return 3;
      uint sz; memcpy( &sz, rec, 4 );
      fd_shred_t const * s = fd_shred_parse( rec + 4, sz );
      if( !s ) return 4;
      memset( leaf + j, 0, sizeof(fd_bmtree_node_t) );
      fd_bmtree_hash_leaf( leaf + j, rec + 4 + sizeof(fd_ed25519_sig_t), fd_shred_merkle_off( s ) - sizeof(fd_ed25519_sig_t),
                           FD_BMTREE_LONG_PREFIX_SZ );
    }
    ulong depth = fd_bmtree_depth( n ) - 1UL;
    fd_bmtree_commit_t * t = fd_bmtree_commit_init( mem, FD_SHRED_MERKLE_NODE_SZ, FD_BMTREE_LONG_PREFIX_SZ, depth + 1UL );
    fd_bmtree_commit_append( t, leaf, n );
    uchar * root = fd_bmtree_commit_fini( t );
    fwrite( &depth, 8, 1, stdout );
    for( ulong j=0; j<n; j++ ) fwrite( leaf[j].hash, 1, 32, stdout );
    fwrite( root, 1, 32, stdout );
    for( ulong j=0; j<n; j++ ) {
      uchar p[ 160 ]; memset( p, 0, 160 );
      if( fd_bmtree_get_proof( t, p, j ) != (int)depth ) return 5;
      fwrite( p, 1, 160, stdout );
    }
  }
  return 0;
}
"""


def splits():
    """(n, data_cnt, code_cnt, cls, seed) per set: the splits move around the half, the classes take turns"""
    out = []
    for i, n in enumerate(fm.SIZES):
        data = 1 if n == 1 else max(1, min(n - 1, (n + 1) // 2 + (i % 3 - 1) * (n // 5)))
        out.append((n, data, n - data, i % 3, 4000 + 7 * i))
    return out


def main() -> None:
    sets = splits()
    inp = b""
    for n, dc, cc, cls, seed in sets:
        shreds = fm.build_set(dc, cc, cls, seed, lambda r: bytes(64))
        inp += struct.pack("<Q", n) + b"".join(struct.pack("<I", len(s)) + s.ljust(1228, b"\0") for s in shreds)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "fec_driver.c")
        with open(src, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "fec_driver")
        flags = ["-std=c17", "-fwrapv", "-O3", "-fPIC", "-ffunction-sections", "-fdata-sections", "-DFD_HAS_BACKTRACE=0",
                 "-I" + REF, "-pthread", "-DFD_HAS_DOUBLE=1", "-DFD_HAS_ALLOCA=1"]      # oracle/Makefile REF_NOARCH
        subprocess.run(["gcc"] + flags + ["-w", "-Wl,--gc-sections", "-o", exe, src, REF + "/ballet/shred/fd_shred.c",
                        REF + "/ballet/bmtree/fd_bmtree.c", REF + "/ballet/sha256/fd_sha256.c"], check=True)
        res = subprocess.run([exe], input=inp, capture_output=True, check=True).stdout
    o, depth, leaves, roots, proofs = 0, [], [], [], []
    for n, *_ in sets:
        depth.append(struct.unpack_from("<Q", res, o)[0])
        o += 8
        leaves.append(res[o:o + 32 * n])
        o += 32 * n
        roots.append(res[o:o + 32])
        o += 32
        proofs.append(res[o:o + 160 * n])
        o += 160 * n
    assert o == len(res)
    ns = np.array([s[0] for s in sets], np.uint16)
    np.savez_compressed(
        os.path.join(HERE, "fec_trees.npz"),
        n=ns, data_cnt=np.array([s[1] for s in sets], np.uint16), code_cnt=np.array([s[2] for s in sets], np.uint16),
        cls=np.array([s[3] for s in sets], np.uint8), seed=np.array([s[4] for s in sets], np.uint32),
        depth=np.array(depth, np.uint8), first=np.concatenate([[0], np.cumsum(ns.astype(np.int64))[:-1]]).astype(np.uint32),
        leaves=np.frombuffer(b"".join(leaves), np.uint8).reshape(-1, 32),
        root=np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32),
        proofs=np.frombuffer(b"".join(proofs), np.uint8).reshape(-1, 160))
    print(f"{len(sets)} sets, {int(ns.sum())} leaves, depths {sorted(set(depth))}, "
          f"{os.path.getsize(os.path.join(HERE, 'fec_trees.npz'))} bytes")


if __name__ == "__main__":
    main()
