#!/usr/bin/env python3
"""64-byte blocks of `vals` the band kernels load per system, counted from the program on the CPU — the traffic the interleaved
layout (cnl_options.batch_layout = 1) makes of it: a piece of eight elements that starts on a multiple of 8 is one block, any
other touches two; a block two pieces of ONE epoch touch is counted once (they are loaded together), a block two epochs touch twice
(the second load comes after the block has left the caches).  Today's program ("band") against its resident form ("bandr", csrc/band.h), and what the difference is per
launch of B problems.
  PYTHONPATH=. python tools/band_block_count.py [n] [ncon] [B]      (default: the headline, 10000 50 16384)"""
import json
import sys

import numpy as np

NPIECE, EW, BE_FP, BE_BP = 15, 44, 0, 15


def vals_block_loads(plan, prefix):
    """{"forward": blocks loaded, "backward": ..., "forward_distinct": distinct blocks touched, "backward_distinct": ...} per system,
    all parts together; None where the plan has no such program"""
    info = plan.array(f"{prefix}_info")
    if not info[0]:
        return None
    resident = prefix == "bandr"
    ebits = 23 if resident else 28
    out = {}
    for name, f in (("forward", BE_FP), ("backward", BE_BP)):
        loads, distinct = 0, 0
        for q in range(int(info[1])):
            every = []
            for pcs in plan.array(f"{prefix}_epochs{q}").reshape(-1, EW)[:, f: f + NPIECE]:
                base = (pcs[(pcs >= 0) & (pcs >> 28 == 0)] & ((1 << ebits) - 1)).astype(np.int64)
                every.append(np.union1d(base // 8, (base + 7) // 8))
                loads += len(every[-1])
            distinct += len(np.unique(np.concatenate(every)))
        out[name], out[name + "_distinct"] = loads, distinct
    return out


def main():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    n, p, B = (int(a) for a in (sys.argv[1:4] + ["10000", "50", "16384"][len(sys.argv) - 1:]))
    s = syn.band_structure(n, p)
    rows, cols = s.kkt_pattern()
    pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT))
    res = {k: vals_block_loads(pl, k) for k in ("band", "bandr")}
    out = {"pattern": [n, p], "batch": B, "blocks_per_system": res}
    if res["bandr"]:
        saved = sum(res["band"][k] - res["bandr"][k] for k in ("forward", "backward"))
        out["saved_bytes_per_system"] = 64 * saved
        out["saved_GB_per_launch"] = round(64 * saved * B / 1e9, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
