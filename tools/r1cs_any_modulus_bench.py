#!/usr/bin/env python3
"""The C5 shape (workloads.R1csSynthetic: 2^20 rows of 3 + 3 + 1 terms over 4096 base variables, random coefficients)
over fields of the any-modulus R1CS kernels (device/r1cs_generic_kernels.hpp), next to BN254 on the Montgomery row kernel
in the same process:

  tools/r1cs_any_modulus_bench.py [--fields z64,p256m2,p521,bn254] [--steps 5] [--warmup 1] [--out FILE]

Per field: the row check (HIP-event time of zkgpu_r1cs_check, r1cs_last_ms) with the satisfied / failed counts asserted
(every 97th lane is made to fail, as bench.py's c5 does), the witness generation (the assign launches of every dependency
level, host clock around them and a synchronize), and the check's algorithmic bytes: 7 gathered wire records per row and
lane (16 bytes per four words of a value), as a fraction of the 8 TB/s HBM peak.  Batches keep the wire table at or below
about 40 GB.  Kernel times per instantiation: run it under `rocprofv3 --kernel-trace --stats` in a pass of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# name -> (modulus, lanes)
FIELDS = {'z64': (2 ** 64, 1024), 'p256m2': (2 ** 256 - 2, 1024), 'p521': (2 ** 521 - 1, 448), 'bn254': (BN254_R, 1024)}
HBM_PEAK = 8.0e12   # bytes/s (spec; about 6.3e12 achievable)


def run(name, p, batch, M, n_base, steps, warmup, zk, workloads):
    t0 = time.time()
    wl = workloads.R1csSynthetic(M=M, n_base=n_base, p=p)
    ev = zk.Evaluator()
    ev.declare_inputs(0, wl.n_witness)
    ev.ingest_message(wl.base_relation())
    ev.finalize(retain_all=True)
    row_ptr, tv, tc, cb = wl.csr()
    ev.r1cs_load_csr(row_ptr, tv, tc, cb, wl.width, wl.M)
    w = wl.witnesses(batch)
    ev.set_inputs(None, w.tobytes(), batch)
    ev.replay()
    ev.synchronize()
    t1 = time.time()
    lo = 0
    for hi in wl.level_bounds:
        ev.r1cs_assign(lo, int(hi) - lo)
        lo = int(hi)
    ev.synchronize()
    assign_s = time.time() - t1
    zl = ev.r1cs_get_var(wl.last_z, batch)
    bad = 0
    for lane in range(batch):
        v = zl[lane]
        if lane % 97 == 0:
            v = (v + 1) % p
            bad += 1
        w[lane, wl.n_base] = np.frombuffer(int(v).to_bytes(wl.width, 'little'), dtype=np.uint8)
    ev.set_inputs(None, w.tobytes(), batch)
    ev.replay()
    ev.synchronize()
    ms = []
    for k in range(warmup + steps):
        ev.r1cs_check()
        ff, counts = ev.r1cs_results(batch)
        assert counts == (batch - bad, bad), (name, counts)
        if k >= warmup:
            ms.append(ev.r1cs_last_ms)
    nwords = wl.width // 4
    record = 16 * ((nwords + 3) // 4)
    alg_bytes = 7 * record * (M + 1) * batch
    check_ms = float(np.median(ms))
    return {'field': name, 'modulus_bits': p.bit_length(), 'representation': ev.field_representation(0),
            'rows': M + 1, 'batch': batch, 'levels': wl.n_levels, 'wire_table_GB': round(ev.table_bytes / 1e9, 2),
            'satisfied': counts[0], 'failed': counts[1],
            'check_ms_median': round(check_ms, 3), 'check_ms_all': [round(x, 3) for x in ms],
            'assign_all_levels_s': round(assign_s, 3), 'setup_s': round(t1 - t0, 2),
            'bytes_per_term': record, 'algorithmic_GB': round(alg_bytes / 1e9, 2),
            'algorithmic_TBps': round(alg_bytes / (check_ms * 1e-3) / 1e12, 3),
            'fraction_of_hbm_peak': round(alg_bytes / (check_ms * 1e-3) / HBM_PEAK, 4),
            'row_checks_per_s': round((M + 1) * batch / (check_ms * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fields', default='z64,p256m2,p521,bn254')
    ap.add_argument('--M', type=int, default=1 << 20)
    ap.add_argument('--n-base', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--batch-scale', type=float, default=1.0, help='multiply every batch (a quick rehearsal: 0.0625)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import __graft_entry__
    zk = __graft_entry__.ensure_built()
    from zkinterface_ir_amd import workloads
    results = []
    for name in args.fields.split(','):
        p, batch = FIELDS[name]
        batch = max(64, int(batch * args.batch_scale) // 64 * 64)
        r = run(name, p, batch, args.M, args.n_base, args.steps, args.warmup, zk, workloads)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
