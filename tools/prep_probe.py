#!/usr/bin/env python3
"""Latency-path batches for a kernel trace: runs REPS (default 20) HBM-resident batches of TXNS (default 2,800,
the paced leg's mean batch at 10M frags/s) single-signer 1232-byte transactions through the latency path, checks
the codes and prints what it ran.  Run it under a kernel trace to see the chain fd_prep_kernel -> walk ->
fd_reduce_kernel per batch.  QUAD_SHA=-1 puts the prep's hash role on one lane per signature
(fdgpu_debug_opts_t.quad_sha).  The prep's per-role wave times are recorded in profiles/r05/pp."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from firedancer_amd import Engine, synth  # noqa: E402

n = int(os.environ.get("TXNS", 2800))
if os.environ.get("QUAD_SHA"):
    from firedancer_amd import engine as _engine
    _engine.debug_set_opts(quad_sha=int(os.environ["QUAD_SHA"]))
reps = int(os.environ.get("REPS", 20))
payload, desc, expect, nsig = synth.make_batch(n, synth.LARGE_NOOP, seed=1234, threads=8)
pay_d = torch.from_numpy(payload).cuda()
desc_d = torch.from_numpy(desc.view(np.uint8)).cuda()
out_d = torch.empty(n, dtype=torch.int8, device="cuda")
eng = Engine(device=0, max_txn=n, max_sig=nsig)
st = torch.cuda.current_stream().cuda_stream
for it in range(reps):
    eng.verify_txns_device(pay_d.data_ptr(), desc_d.data_ptr(), n, nsig, out_d.data_ptr(), None, st)
    torch.cuda.synchronize()
assert (out_d.cpu().numpy() == expect).all()
print(json.dumps({"txns": n, "sigs": int(nsig), "reps": reps}))
