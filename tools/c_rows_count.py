"""How many rows of C differ from the key's template for a voter of the benchmark's census, and how many non-zero signed 17-bit window digits those differences have:
what a pass without the transform pair of C (ZKC_C_ROWS, DESIGN.md "Constant folding") adds to its H jobs, against the 2.76 M VALU-busy cycles per SIMD the pair of C
costs a 64-proof pass (profiles/top_fold_kernel_valu_busy_table.json).  The census, the witnesses and the domain vectors come from the library (bench.py's census:
census.synthetic_census_flat, 8 192 voters; zkc_debug_stage 0 and zkc_debug_c_rows 1); the counting is numpy and Python integers on the host.  Prints one JSON object
(profiles/c_rows_count.json).  --voters N: the sample, evenly spaced over the census (default 64)."""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import census, setup

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RINV = pow(1 << 256, -1, R)
C_H, NW_H = 17, 15
CYCLES_PER_ADD = 19.277e6 / (64 * 2207128)          # VALU-busy cycles per SIMD and G1 addition of a 64-proof pass (top_fold_kernel_valu_busy_table.json)
PAIR_OF_C = 2.76e6                                   # a third of the three transform kernels' 8.29 M


def nz_digits(scalars):
    a = np.frombuffer(bytes(scalars), dtype='<u8').reshape(-1, 4)
    half, mask = np.uint64(1 << (C_H - 1)), np.uint64((1 << C_H) - 1)
    carry, cnt = np.zeros(len(a), dtype=np.uint64), 0
    for i in range(NW_H):
        li, sh = (C_H * i) >> 6, (C_H * i) & 63
        d = a[:, li] >> np.uint64(sh)
        if sh + C_H > 64 and li < 3:
            d = d | (a[:, li + 1] << np.uint64(64 - sh))
        d = (d & mask) + carry
        neg = d > half
        d = np.where(neg, np.uint64(1 << C_H) - d, d)
        carry = neg.astype(np.uint64)
        cnt += int(np.count_nonzero(d))
    return cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voters', type=int, default=64)
    ap.add_argument('--census', type=int, default=8192)
    ap.add_argument('--nlevels', type=int, default=160)
    args = ap.parse_args()
    nl = args.nlevels
    ctx = zkcensus_amd.Context(0)
    _, zp, _ = setup.ensure_test_artifacts(nl, ctx=ctx)
    pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read())
    n, nIn = pk.domain_size, ctx.n_inputs(nl)
    flat, _, _ = census.synthetic_census_flat(ctx, args.census, nl)
    pick = [i * (args.census // args.voters) for i in range(args.voters)]
    ws, st = ctx.witness([flat[32 * nIn * i:32 * nIn * (i + 1)] for i in pick], nl)
    assert st == [0] * len(pick)
    out = ctypes.create_string_buffer(96 * n)
    ctx._check(ctx._lib.zkc_debug_c_rows(pk._h, 1, 0, 0, out))
    tmpl = np.frombuffer(out.raw[64 * n:], dtype=np.uint8).reshape(n, 32)
    rows, digits = [], []
    for w in ws:
        d_w = torch.from_numpy(np.frombuffer(w, dtype=np.uint8).copy()).cuda()
        c = np.frombuffer(pk.debug_stage(d_w.data_ptr(), 0)[64 * n:], dtype=np.uint8).reshape(n, 32)
        idx = np.nonzero((c != tmpl).any(axis=1))[0]
        val = lambda a, i: int.from_bytes(a[i].tobytes(), 'little')
        diff = b''.join(((val(c, i) - val(tmpl, i)) * RINV % R).to_bytes(32, 'little') for i in idx)
        rows.append(len(idx)); digits.append(nz_digits(diff) if len(idx) else 0)
    mean_d = sum(digits) / len(digits)
    added = 64 * mean_d * CYCLES_PER_ADD
    print(json.dumps({
        'what': 'rows of C on the domain that differ from the template, and the non-zero signed 17-bit digits of the differences, per voter',
        'census_voters': args.census, 'nLevels': nl, 'sample': len(pick), 'domain': n,
        'rows_mean': sum(rows) / len(rows), 'rows_max': max(rows), 'rows_min': min(rows),
        'digits_mean': mean_d, 'digits_max': max(digits), 'digits_per_row_mean': mean_d / max(1e-9, sum(rows) / len(rows)),
        'predicted_M_cycles_per_simd_and_64_proof_pass': {'accumulation_added': round(added / 1e6, 3), 'pair_of_c_removed': round(PAIR_OF_C / 1e6, 3),
                                                            'balance': round((added - PAIR_OF_C) / 1e6, 3), 'cycles_per_addition': round(CYCLES_PER_ADD, 4)},
        'break_even_rows_at_this_digit_density': round(PAIR_OF_C / (64 * CYCLES_PER_ADD * (mean_d / max(1e-9, sum(rows) / len(rows))))),
    }, indent=1))
    pk.close(); ctx.close()


if __name__ == '__main__':
    main()
