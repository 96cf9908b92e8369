#!/usr/bin/env python3
"""Newton systems/s (fp64) on a batch of constrained band NLS problems — BASELINE.json's metric.

One "step" = one `newton_system!` (KKT assembly + LDL^T + inertia + rho ladder + solve,
/root/reference/src/CaNNOLeS.jl:1008-1052) over a batch of independent problems that share the sparsity
pattern of BASELINE config 3 (n = nequ = 1e4, ncon = 50, band Jacobians), inputs already resident in HBM.
N > 1 GPUs: one process per GPU, every rank owns a contiguous shard of the problems
(cannoles.jl_amd/sharding.py), no collective on the data path; torch.distributed is used only for the
barrier and the max-over-ranks time.  Default: weak scaling, `--batch` problems per GPU.  `--strong --total T`
splits T problems over the ranks (BASELINE config 4: `--strong --total 256 --nvar 1000 --ncon 10`).
Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times `--steps` steps and prints the headline line (`value`, `ms_per_step`, ...).  Everything
else — the roofline and kernel timings, the CPU baseline and the parity guard against the oracle, the other batches, layouts
and configurations — runs with `--full`, which prints the long line and then a compact final line.  `--dump-outputs DIR` writes
what the last timed step computed (rank 0's shard: a fixed sample of the solutions, every problem's rho / rho_old / nfact /
success) as DIR/<name>.npy, so that two builds can be compared output for output on identical inputs.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus 8 --steps 20 --warmup 3
"""
import argparse
import collections
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec (MI355X_MICROARCH.md)
HBM_MEASURED_GBPS = 6290.0  # float4 copy rate measured on MI355X (same guide)
FP64_MFMA_SPEC_TFLOPS = 78.6       # datasheet fp64 matrix peak
FP64_MFMA_MEASURED_TFLOPS = 47.8   # v_mfma_f64_16x16x4_f64 loop, 4 waves/SIMD x 8 accumulators (profiles/r02_microbench.json)
CANONICAL_NNZL_CFG3 = 346209  # nnz(L) of the order "r, x natural, lambda" at n=1e4, p=50
CANONICAL_NNZL_CFG4 = 14529   # the same order at n=1e3, p=10 (BASELINE config 4 / 5)
PARITY_TOL = 1e-9   # bench.py FAILS (exit 3) when the timed kernel's solutions differ from the oracle's by more than this (relative, max norm)


def traffic_record(root, batch, workload, kernel):
    """newest profiles/r*_traffic.json whose batch, workload and kernel family match this run (HBM bytes per launch of the dominant
    kernel from separate rocprofv3 --pmc passes of the same command; tools/summarize_profiles.py writes it)"""
    import glob
    for path in sorted(glob.glob(os.path.join(root, "profiles", "r*_traffic.json")), reverse=True):
        try:
            tj = json.load(open(path))
        except Exception:
            continue
        if tj.get("batch") == batch and tj.get("workload") == list(workload) and kernel.split("_kernel")[0] in str(tj.get("kernel", "")):
            return tj, os.path.basename(path)
    return None, None


def band_batch(s, B, seed):
    """Vectorised generator of B problems of the cfg3 family (same distributions as
    synthetic.band_values; one RNG stream for the whole batch)."""
    rng = np.random.default_rng(seed)
    off = s.offsets()
    vals = np.zeros((B, s.nnzNS))
    r, c = np.asarray(s.hF[0]), np.asarray(s.hF[1])
    dg = r == c
    h = rng.uniform(-0.02, 0.02, (B, len(r)))
    h[:, dg] = rng.uniform(0.1, 1.0, (B, int(dg.sum())))
    vals[:, off[0]:off[1]] = h
    r, c = np.asarray(s.jF[0]), np.asarray(s.jF[1])
    dg = r == c
    j = rng.uniform(-0.5, 0.5, (B, len(r)))
    j[:, dg] = 2.0 + rng.uniform(0, 1, (B, int(dg.sum())))
    vals[:, off[2]:off[3]] = j
    if s.ncon > 0:
        lam = rng.normal(size=(B, s.ncon))
        b = rng.uniform(-0.1, 0.1, (B, s.nvar))
        blk = (np.arange(s.nvar) // s.meta["block"]).astype(int)
        vals[:, off[1]:off[2]] = -(lam[:, blk] * b)
        vals[:, off[3]:off[4]] = rng.uniform(-1, 1, (B, s.nnzjc))
        vals[:, off[5]:off[6]] = -0.1
    vals[:, off[4]:off[5]] = -1.0
    rhs = rng.normal(size=(B, s.N))
    return vals, rhs


def band_chunks(s, g0, nloc, chunk=512):
    """band_batch over problems [g0, g0 + nloc) of the job in chunks of `chunk` (seed 3000 + the chunk's first global problem),
    generated on host threads (numpy releases the GIL in the RNG and the array passes) and yielded in order as (b0, vals, rhs);
    at most a few chunks per thread are held at once"""
    starts = iter(range(0, nloc, chunk))
    nthr = max(1, min(16, len(os.sched_getaffinity(0)), -(-nloc // chunk)))
    with cf.ThreadPoolExecutor(nthr) as ex:
        pending = collections.deque()

        def submit():
            b0 = next(starts, None)
            if b0 is not None:
                pending.append((b0, ex.submit(band_batch, s, min(chunk, nloc - b0), 3000 + g0 + b0)))
        for _ in range(nthr + 2):
            submit()
        while pending:
            b0, fut = pending.popleft()
            vh, rh = fut.result()
            submit()
            yield b0, vh, rh


def dump_outputs(path, prob, nsample=128, seed=0):
    """what the last timed step left for the caller of cnl_newton_system_dev, as float64 .npy files: d of a fixed, seeded sample of
    the shard's problems and the rho slots of their `vals` (the step writes them when the problem climbs the ladder), and rho,
    rho_old, nfact, success of every problem"""
    torch, hipldl, s, B = prob.torch, prob.hipldl, prob.s, prob.B
    torch.cuda.synchronize()
    os.makedirs(path, exist_ok=True)
    pick = np.sort(np.random.default_rng(seed).choice(B, size=min(B, nsample), replace=False))
    sel = torch.from_numpy(pick).to(prob.d.device)
    slots = np.arange(s.nnzNS - s.nvar, s.nnzNS)
    if prob.L.config.get("batch_layout"):
        idx = hipldl.il_index(pick[:, None], slots[None, :], s.nnzNS)
        rho_slots = prob.vin[torch.from_numpy(idx).to(prob.d.device)]
    else:
        rho_slots = prob.vin[sel][:, s.nnzNS - s.nvar:]
    arrays = {"sample_problems": pick.astype(np.float64), "d": prob.d[sel].cpu().numpy(), "vals_rho_slots": rho_slots.cpu().numpy(),
              "rho": prob.rho.cpu().numpy(), "rho_old": prob.rho_old.cpu().numpy(),
              "nfact": prob.nfact.cpu().numpy().astype(np.float64), "success": prob.succ.cpu().numpy().astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def backward_error(s, rows, cols, vals, rhs, d):
    import scipy.sparse as sp
    Kl = sp.coo_matrix((vals, (rows - 1, cols - 1)), shape=(s.N, s.N)).tocsr()
    Ks = Kl + sp.tril(Kl, -1).T
    res = Ks @ d + rhs
    return float(np.abs(res).max() / (abs(Ks).sum(axis=1).max() * np.abs(d).max() + np.abs(rhs).max()))


def parse_options(hipldl, text):
    """--opt key=value[,key=value] -> cnl_options (None: the library's own choices)"""
    if not text:
        return None
    kw = {}
    for item in text.split(","):
        k, v = item.split("=", 1)
        kw[k] = v if k == "force_order" else int(v)
    return hipldl.Options(**kw)


class DeviceProblem:
    """device-resident buffers + handle for `B` problems of one pattern, and a timed loop over cnl_newton_system_dev"""

    def __init__(self, torch, hipldl, s, rows, cols, vals, rhs, B, device_index, stream, options=None):
        self.torch, self.hipldl, self.s, self.B = torch, hipldl, s, B
        dev = vals.device
        self.vals, self.rhs = vals, rhs
        self.d = torch.zeros((B, s.N), dtype=torch.float64, device=dev)
        self.rho_old = torch.zeros(B, dtype=torch.float64, device=dev)
        self.rho = torch.zeros(B, dtype=torch.float64, device=dev)
        self.nfact = torch.zeros(B, dtype=torch.int32, device=dev)
        self.succ = torch.zeros(B, dtype=torch.int32, device=dev)
        self.params = hipldl.default_params()
        self.L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, device=device_index, options=options)
        self.stream = stream
        # cnl_options.batch_layout = CNL_LAYOUT_INTERLEAVED: the kernel's `vals` is the interleaved array (what row f2 writes on such a
        # handle); the problem-major copy stays for the other blocks
        self.vin = self.vals
        if self.L.config.get("batch_layout"):
            self.vin = torch.empty(hipldl.layout_len(self.L, 0), dtype=torch.float64, device=dev)
            hipldl.interleave_dev(self.L, 0, self.vals.data_ptr(), self.vin.data_ptr(), 0)
            torch.cuda.synchronize()

    def step(self):
        self.rho_old.zero_()
        self.hipldl.newton_system_dev(self.L, self.vin.data_ptr(), self.rhs.data_ptr(), self.d.data_ptr(), self.rho_old.data_ptr(),
                                      self.rho.data_ptr(), self.nfact.data_ptr(), self.succ.data_ptr(), self.params, self.stream.cuda_stream)

    def timed(self, steps, warmup):
        """ms per step by HIP events on the launch stream"""
        torch = self.torch
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):
                self.step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for _ in range(steps):
                self.step()
            e1.record(self.stream)
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / max(steps, 1)

    def counts(self):
        return [self.B, int((self.succ == 1).sum().item())]

    def close(self):
        self.L.close()


def multi_front_end(torch, hipldl, s, rows, cols, devices, per_dev, steps, warmup, seed0=3000, total=None):
    """`steps` timed steps of cnl_multi_newton_system_dev + ONE cnl_multi_synchronize at the end, from one process: shard i's arrays live
    on devices[i].  Wall-clock (the devices have no common event timeline); every device is synchronised on both sides.
    Returns (seconds, problems, all_success, shards)."""
    ndev = len(devices)
    total = per_dev * ndev if total is None else total
    M = hipldl.MultiHIPLDLStruct(s.N, rows, cols, s.nvar, s.nequ, s.ncon, total, devices)
    T = []
    for (st, cnt, dv) in M.shards:
        dev = torch.device("cuda", dv)
        vals = torch.empty((cnt, s.nnzNS), dtype=torch.float64, device=dev)
        rhs = torch.empty((cnt, s.N), dtype=torch.float64, device=dev)
        for b0 in range(0, cnt, 512):
            nb = min(512, cnt - b0)
            vh, rh = band_batch(s, nb, seed=seed0 + st + b0)
            vals[b0:b0 + nb].copy_(torch.from_numpy(vh))
            rhs[b0:b0 + nb].copy_(torch.from_numpy(rh))
        T.append({"vals": vals, "rhs": rhs, "d": torch.zeros((cnt, s.N), dtype=torch.float64, device=dev),
                  "ro": torch.zeros(cnt, dtype=torch.float64, device=dev), "rho": torch.zeros(cnt, dtype=torch.float64, device=dev),
                  "nf": torch.zeros(cnt, dtype=torch.int32, device=dev), "ok": torch.zeros(cnt, dtype=torch.int32, device=dev)})
    p = hipldl.default_params()
    ptr = lambda k: [t[k].data_ptr() for t in T]   # noqa: E731
    args_ = (ptr("vals"), ptr("rhs"), ptr("d"), ptr("ro"), ptr("rho"), ptr("nf"), ptr("ok"))

    def sync_all():
        for (_, _, dv) in M.shards:
            torch.cuda.synchronize(dv)
    for _ in range(warmup):
        M.newton_system_dev(*args_, p)
    M.synchronize()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        M.newton_system_dev(*args_, p)     # enqueue only: every shard on its handle's own stream
    M.synchronize()
    dt = time.perf_counter() - t0
    ok = all(bool((t["ok"] == 1).all().item()) for t in T)
    shards = list(M.shards)
    M.close()
    return dt, total, ok, shards


def main_multi(args):
    """bench.py --multi: the whole job from ONE process (cnl_multi_*), all devices of the node (or --gpus of them)."""
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    ndev = min(max(1, args.gpus), torch.cuda.device_count())
    torch.zeros(1, device="cuda:0")
    s = syn.band_structure(args.n, args.ncon, name="cfg3")
    rows, cols = s.kkt_pattern()
    total = args.total if args.strong else args.batch * ndev
    dt, nprob, ok, shards = multi_front_end(torch, hipldl, s, rows, cols, list(range(ndev)), args.batch, args.steps, args.warmup, total=total)
    print(json.dumps({
        "metric": "Newton systems/sec (fp64), batched n=1e4 NLS; achieved HBM GB/s vs peak", "value": nprob * args.steps / dt, "unit": "systems/s",
        "n_gpus": ndev, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / max(args.steps, 1) * 1e3, "higher_is_better": True,
        "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"cfg3 band constrained NLS n={args.n} nequ={args.n} ncon={args.ncon}, {nprob} independent problems over {ndev} GPU(s), "
                               "one newton_system! per problem per step", "front_end": "ONE process: cnl_multi_newton_system_dev + cnl_multi_synchronize",
                   "shards": shards, "all_success": ok, "timer": "wall clock around the enqueue loop and the final cnl_multi_synchronize"}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("CNL_BENCH_BATCH", 16384)), help="problems per GPU (weak scaling); 16384 since round 5 (the band kernels hold that many at once), 8192 before — the line carries both")
    ap.add_argument("--strong", action="store_true", help="strong scaling: --total problems split over the ranks")
    ap.add_argument("--total", type=int, default=256, help="total problems with --strong")
    ap.add_argument("--nvar", "--n", dest="n", type=int, default=10000, help="variables = residuals per problem (spelled --nvar under torch.distributed.run, whose own options make --n ambiguous)")
    ap.add_argument("--ncon", type=int, default=50)
    ap.add_argument("--full", action="store_true", help="beside the headline: roofline and kernel timings, CPU baseline and parity guard against "
                                                        "the oracle, the other batches, layouts and configurations (long line + compact final line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (rank 0's shard) as DIR/<name>.npy")
    ap.add_argument("--cpu-sample", type=int, default=-1, help="with --full: problems timed on the CPU oracle (-1 auto, 0 off)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the small-batch, PCIe-inclusive, cfg2 and f1 blocks")
    ap.add_argument("--layout", choices=("interleaved", "problem-major"), default="interleaved",
                    help="layout of the device-resident `vals` of the headline handle: interleaved = cnl_options.batch_layout 1 (what row f2 writes on "
                         "such a handle; falls back to problem-major where the band kernels do not serve the handle), problem-major = the reference's "
                         "vector per problem; the line carries both")
    ap.add_argument("--opt", default="", help="cnl_options fields for the headline handle, key=value[,key=value] (measurement tools; default: the library's own choices)")
    ap.add_argument("--multi", action="store_true", help="ONE process drives --gpus devices through cnl_multi_newton_system_dev / cnl_multi_synchronize "
                                                         "(the second front end of DESIGN section 6) instead of one process per GPU")
    args = ap.parse_args()
    if args.multi:
        if args.dump_outputs:
            ap.error("--dump-outputs: the one-process-per-GPU path only (not --multi)")
        return main_multi(args)

    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, sharding, synthetic as syn

    rank, local_rank, world = sharding.env_rank()
    if world != args.gpus and rank == 0:
        print(f"warning: WORLD_SIZE={world} but --gpus {args.gpus}; using WORLD_SIZE", file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # CNL_BENCH_ONE_DEVICE=1 + CNL_DIST_BACKEND=gloo: several ranks on ONE GPU (dry run of the multi-process path on a
    # single-GPU box; RCCL refuses two ranks on one device, gloo carries the barrier and the reductions instead)
    if os.environ.get("CNL_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    backend = os.environ.get("CNL_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dist = sharding.init(backend)
    red_dev = torch.device("cuda", local_rank) if backend == "nccl" else "cpu"

    s = syn.band_structure(args.n, args.ncon, name="cfg3")
    rows, cols = s.kkt_pattern()
    total = args.total if args.strong else args.batch * world
    dev = torch.device("cuda", local_rank)
    stream = torch.cuda.Stream(device=dev)
    host_chunk = {}

    def make_executor(g0, g1):
        """this rank's shard: problems [g0, g1) of the job, generated on the host in chunks (bounded host memory) and uploaded;
        only the first chunk stays on the host, for the parity guard and the CPU-baseline sample.  Seeds follow the global
        problem number."""
        nloc = g1 - g0
        vals = torch.empty((nloc, s.nnzNS), dtype=torch.float64, device=dev)
        rhs = torch.empty((nloc, s.N), dtype=torch.float64, device=dev)
        for b0, vh, rh in band_chunks(s, g0, nloc):
            nb = len(vh)
            vals[b0:b0 + nb].copy_(torch.from_numpy(vh))
            rhs[b0:b0 + nb].copy_(torch.from_numpy(rh))
            if b0 == 0:
                host_chunk["vals"], host_chunk["rhs"] = vh, rh
        if args.layout == "interleaved":
            try:
                return DeviceProblem(torch, hipldl, s, rows, cols, vals, rhs, nloc, local_rank, stream,
                                     options=parse_options(hipldl, (args.opt + "," if args.opt else "") + "batch_layout=1"))
            except hipldl.CnlError:   # (the band kernels do not serve this shape / batch: the reference's layout)
                pass
        return DeviceProblem(torch, hipldl, s, rows, cols, vals, rhs, nloc, local_rank, stream, options=parse_options(hipldl, args.opt))

    # the per-rank driver shared with the CPU (gloo) test: shard, warm-up, barrier + synchronize on both sides of exactly
    # `steps` steps, max over ranks, job-wide counts
    with torch.cuda.stream(stream):
        elapsed, counts, prob, (g0, g1) = sharding.run_shard(total, make_executor, args.steps, args.warmup, dist,
                                                             sync=torch.cuda.synchronize, device=red_dev)
    B = g1 - g0
    vals_h, rhs_h = host_chunk.get("vals"), host_chunk.get("rhs")
    vals, rhs = (prob.vals, prob.rhs) if prob else (None, None)

    if rank != 0:
        if prob:
            prob.close()
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prob)
    if not args.full:
        return headline_only(args, prob, counts, elapsed, total, world, B, dist)

    LDLT = prob.L
    step_ms = prob.timed(min(10, max(2, args.steps)), 1)  # HIP events on the launch stream: the whole step of this rank
    # duration of the dominant kernel alone (the multifrontal kernel), HIP events inside the library on the launch
    # stream, over a few extra launches AFTER the timed region (timing mode synchronises every call)
    LDLT.set_timing(True)
    kms = []
    with torch.cuda.stream(stream):
        for _ in range(min(5, max(2, args.steps))):
            prob.step()
            kms.append(LDLT.last_kernel_ms())
    kern_ms = float(np.mean(kms))
    # the forward sweep alone (try_to_factorize: assembly + LDL^T + inertia, no solve), same timing mode: what is left of kern_ms
    # is the backward sweep (profiles/HISTORY.md 4a: the two sweeps are bound by different things)
    fwd_ms, solve_ms = None, None
    band = bool(LDLT.config.get("band"))
    try:
        if args.no_extras:   # (the profiling passes run with --no-extras: only full steps of the kernel in their statistics)
            raise RuntimeError("skipped")
        # the reference's own two-call sequence on the same handle (src/CaNNOLeS.jl:1023,1049): try_to_factorize = the forward sweep
        # (band handles: without the factor-record stores), solve_ldl! = (band handles) factorisation + both sweeps of a right-hand side
        fms, sms = [], []
        d_two = torch.zeros_like(prob.d)
        with torch.cuda.stream(stream):
            for _ in range(3):
                hipldl._check(hipldl.lib().cnl_factorize_dev(LDLT._h, prob.vin.data_ptr(), 2.220446049250313e-16, prob.succ.data_ptr(), stream.cuda_stream))
                torch.cuda.synchronize()
                fms.append(LDLT.last_kernel_ms())
                hipldl._check(hipldl.lib().cnl_solve_dev(LDLT._h, prob.rhs.data_ptr(), d_two.data_ptr(), stream.cuda_stream))
                torch.cuda.synchronize()
                sms.append(LDLT.last_kernel_ms())
            prob.step()   # leaves the handle and `succ` as the timed loop left them
            torch.cuda.synchronize()
        fwd_ms, solve_ms = float(np.mean(fms[1:])), float(np.mean(sms[1:]))
        two_call_equal = bool(torch.equal(d_two, prob.d))
        del d_two
    except Exception:
        fwd_ms = None
    LDLT.set_timing(False)

    ok = counts[1] == counts[0]
    nchk = min(B, 4)
    d_h = prob.d[:nchk].cpu().numpy()
    berr = max(backward_error(s, rows, cols, vals_h[b], rhs_h[b], d_h[b]) for b in range(nchk))

    info = LDLT.info
    headline = (args.n, args.ncon) == (10000, 50)
    # B_alg = 12 nnzNS + 24 N + 32 nnz(L*), nnz(L*) = min(fill of the build's own ordering WITHOUT the
    # explicit zeros of relaxed supernodes, canonical fill) — padding must not inflate the score
    nnzL_star = min(info["nnzL_exact"], CANONICAL_NNZL_CFG3) if headline else info["nnzL_exact"]
    b_alg = 12 * s.nnzNS + 24 * s.N + 32 * nnzL_star
    achieved = b_alg * B / (kern_ms * 1e-3) / 1e9
    traffic, traffic_src, traffic_raw = None, None, None
    kname = "band_newton_kernel" if band else "newton2_kernel"
    tj, tfile = traffic_record(ROOT, B, (args.n, args.ncon), kname)
    if tj:  # HBM bytes per launch of the dominant kernel from separate rocprofv3 PMC passes of this command
        traffic, traffic_raw = tj.get("hbm_bytes_per_launch"), tj.get("raw_sum_bytes")
        traffic_src = f"profiles/{tfile} (rocprofv3 --pmc passes of this command, not measured by this run)"
    # what the kernel itself has to move: the band kernels keep no L for the condensed rows (they re-read J in the
    # backward sweep) — per pivot 15 doubles read + 6 written forward, 13 read + 2 written backward; B_alg above is the CONTRACT figure
    #  and no bound on this kernel's traffic, so the fraction on the kernel's own bytes is printed beside it
    kernel_bytes = band_kernel_bytes(LDLT, s) if band else None
    out = headline_fields(args, LDLT, counts, elapsed, total, world, B)
    out["config"]["backward_error"] = berr
    out.update({
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                     "frac_of_measured_copy_rate": achieved / HBM_MEASURED_GBPS, "peak_measured_copy": HBM_MEASURED_GBPS,
                     "traffic": traffic, "traffic_source": traffic_src,
                     "measured_hbm_frac": (traffic / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if traffic else None,
                     "traffic_raw_counters": traffic_raw,
                     "kernel_bytes_per_system": kernel_bytes,
                     "frac_on_kernel_bytes": (kernel_bytes * B / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if kernel_bytes else None,
                     "traffic_over_kernel_bytes": (traffic / (kernel_bytes * B)) if (traffic and kernel_bytes) else None,
                     "bytes_per_system": b_alg, "nnzL_star": nnzL_star, "kernel_ms": kern_ms, "kernel": kname,
                     "units_per_launch": B,
                     "forward_sweep_ms": fwd_ms, "backward_sweep_ms": (kern_ms - fwd_ms) if fwd_ms else None,
                     "two_call_sequence": ({"try_to_factorize_ms": fwd_ms, "solve_ldl_ms": solve_ms, "total_over_newton_system": (fwd_ms + solve_ms) / kern_ms,
                                            "d_bit_equal_to_newton_system": two_call_equal,
                                            "note": "same handle, same kernel family (cnl_factorize_dev + cnl_solve_dev); band handles: the solve factorises again and sweeps in one launch"}
                                           if (fwd_ms and solve_ms) else None),
                     "kernel_is_whole_step": band or (bool(LDLT.config.get("lean")) and bool(LDLT.plan_array("brec")[7] & 256)),
                     "note": "since round 3 the lean kernel recovers the residual components in its backward sweep: no post-pass, kernel_ms == step_ms; "
                             "rounds 1-2 (and round 3 before that change) priced a kernel that left 1.2 ms of the step to a second kernel on the same algorithmic bytes "
                             "(their step_frac is the comparable figure)",
                     "step_ms": step_ms, "step_frac": b_alg * B / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS},
    })
    extras = (not args.no_extras) and world == 1 and not args.strong
    if extras:
        extra_blocks(out, torch, hipldl, syn, s, rows, cols, vals, rhs, vals_h, rhs_h, prob, B, dev, local_rank, stream, args)
    out["value_batch_per_gpu"] = B
    if _dig(out.get("small_batch"), ("B8192", "systems_per_s")) is not None:
        out["value_at_batch_8192"] = out["small_batch"]["B8192"]["systems_per_s"]   # rounds 1-4 quoted `value` at this batch
    if args.cpu_sample != 0 and world == 1:
        cpu_baseline(out, s, rows, cols, vals_h, rhs_h, prob, LDLT, args)
    # the long line first (every block, for profiles/), then a COMPACT FINAL LINE (<= 1.8 KB) with the mandated keys and one number
    # per configuration, so that a reader of the tail of this process's output has every config's figure
    # parity guard of the TIMED configuration: the solutions the timed kernel left in HBM against the oracle's
    # (max_rel_diff_vs_gpu of the cpu_baseline leg) and the backward errors of the first problems; a miss fails the bench
    perr = out.get("cpu_baseline", {}).get("max_rel_diff_vs_gpu")
    guard = {"all_success": bool(ok), "backward_error": berr, "backward_tol": 1e-12, "max_rel_diff_vs_oracle": perr, "oracle_tol": PARITY_TOL}
    guard["ok"] = bool(ok) and berr <= 1e-12 and (perr is None or perr <= PARITY_TOL)
    out["parity_guard"] = guard
    print(json.dumps(out))
    print(json.dumps(compact_line(out)))
    prob.close()
    if dist is not None:
        dist.destroy_process_group()
    if not guard["ok"]:
        print(f"bench.py: parity guard FAILED: {guard}", file=sys.stderr)
        sys.exit(3)


def headline_fields(args, LDLT, counts, elapsed, total, world, B):
    """the mandated keys and the workload / handle description: what a plain run prints, and the head of the --full line"""
    info = LDLT.info
    return {
        "metric": "Newton systems/sec (fp64), batched n=1e4 NLS; achieved HBM GB/s vs peak",
        "value": counts[0] * args.steps / elapsed, "unit": "systems/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / max(args.steps, 1) * 1e3, "higher_is_better": True, "scaling": "strong" if args.strong else "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"cfg3 band constrained NLS n={args.n} nequ={args.n} ncon={args.ncon}, "
                               + (f"{total} independent problems split over {world} GPU(s)" if args.strong else f"{B} independent problems per GPU")
                               + ", one newton_system! per problem per step",
                   "vals_layout": ("interleaved over groups of 32 problems (cnl_options.batch_layout = 1: what cnl_prepare_newton_system_dev writes on "
                                   "such a handle; rhs, d problem-major)" if LDLT.config.get("batch_layout") else "problem-major (the reference's vector per problem)"),
                   "batch_per_gpu": B, "total_problems": counts[0], "sharding": f"independent problems, {world} contiguous shard(s), no collective",
                   "ordering": info["order"], "nnzL_stored": info["nnzL"], "nnzL_exact": info["nnzL_exact"], "fronts": info["nsuper"],
                   "kernel": LDLT.config, "all_success": counts[1] == counts[0]},
    }


def headline_only(args, prob, counts, elapsed, total, world, B, dist):
    """a plain run: the headline line alone; fails (exit 3) when a problem of the timed batch did not succeed"""
    out = headline_fields(args, prob.L, counts, elapsed, total, world, B)
    out["value_batch_per_gpu"] = B
    out["value_vals_layout"] = "interleaved" if prob.L.config.get("batch_layout") else "problem-major"
    print(json.dumps(out))
    prob.close()
    if dist is not None:
        dist.destroy_process_group()
    if not out["config"]["all_success"]:
        print(f"bench.py: {counts[0] - counts[1]} of {counts[0]} problems did not succeed", file=sys.stderr)
        sys.exit(3)


def band_kernel_bytes(LDLT, s):
    """bytes one band_newton_kernel launch necessarily moves per system: every COO value and right-hand-side entry once in the forward
    sweep, the factor records written once and read once, the Jacobian / -I entries of the condensed rows and their right-hand sides
    a second time in the backward sweep, d written once"""
    bi = LDLT.plan_array("band_info")
    lsz = 0
    for q in range(int(bi[1])):
        lsz += int(LDLT.plan_array(f"band_part{q}")[3]) * 6   # factor events x BAND_LREC doubles
    nnzj = len(s.jF[0]) + len(s.jc[0])
    fwd = 8 * (s.nnzNS + s.N) + 8 * lsz
    bwd = 8 * lsz + 8 * (len(s.jF[0]) + 2 * s.nequ) + 8 * s.N
    del nnzj
    return fwd + bwd


def compact_line(out):
    """mandated keys + roofline + cpu_baseline (short) + `summary`: one figure per configuration of the long line"""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    c = {k: out[k] for k in keep}
    cfg = out["config"]
    c["config"] = {"workload": cfg["workload"], "batch_per_gpu": cfg["batch_per_gpu"], "kernel": "band" if cfg["kernel"].get("band") else cfg["kernel"].get("kernel"),
                   "all_success": cfg["all_success"], "backward_error": cfg["backward_error"]}
    r = out["roofline"]
    c["roofline"] = {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "bytes_per_system", "units_per_launch",
                                       "kernel_bytes_per_system", "frac_on_kernel_bytes", "traffic_over_kernel_bytes")}
    if "cpu_baseline" in out:
        b = out["cpu_baseline"]
        c["cpu_baseline"] = {k: b[k] for k in ("value", "unit", "cores", "kind", "sample") if k in b}
        if isinstance(c["cpu_baseline"].get("sample"), str):
            c["cpu_baseline"]["sample"] = c["cpu_baseline"]["sample"][:120]
    g = lambda blk, *path: _dig(out.get(blk), path)   # noqa: E731
    s = {
        "cfg3_B8192_ksys_s": _k(g("small_batch", "B8192", "systems_per_s")), "cfg3_B4096_ksys_s": _k(g("small_batch", "B4096", "systems_per_s")),
        "cfg3_B256_ksys_s": _k(g("small_batch", "B256", "systems_per_s")), "cfg3_B1_ms": g("small_batch", "B1", "ms_per_call"),
        "cfg2_B1_ms": g("cfg2_dense", "B1", "ms_per_system"), "cfg2_B1_frac": g("cfg2_dense", "B1", "frac_of_spec"),
        "cfg2_B8_frac": g("cfg2_dense", "B8", "frac_of_spec"), "cfg2_B32_frac": g("cfg2_dense", "B32", "frac_of_spec"),
        "cfg4_B256_ms": g("cfg4", "B256", "ms_per_call"), "cfg4_B256_frac": g("cfg4", "B256", "frac"), "cfg4_B32_ms": g("cfg4", "B32", "ms_per_call"),
        "cfg4_B4096_frac": g("cfg4", "B4096", "frac"), "cfg5_B256_ms": g("cfg5", "B256", "ms_per_call"), "cfg5_B256_frac": g("cfg5", "B256", "frac"),
        "f1_residual_vectors_ms": g("aux_f1", "residual_vectors", "ms"), "f1_residual_vectors_frac": g("aux_f1", "residual_vectors", "frac"),
        "f1_trial_point_frac": g("aux_f1", "trial_point", "frac"), "f2_prepare_frac": g("aux_f1", "f2_prepare", "frac"), "f2_prepare_interleaved_frac": g("aux_f1", "f2_prepare", "interleaved", "frac"),
        "f3_ms_per_step": g("aux_f3", "ms_per_step"), "two_call_over_newton": _dig(out.get("roofline"), ("two_call_sequence", "total_over_newton_system")),
        "pcie_inclusive_ksys_s": _k(g("pcie_inclusive", "systems_per_s")),
        "single_system_host_ms": g("call_pattern_single_system", "newton_system_ms"), "single_system_analysis_s": g("call_pattern_single_system", "analysis_s"), "multi_front_end_ratio": g("multi_front_end", "ratio_to_single_handle"),
    }
    c["summary"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items() if v is not None}
    if "parity_guard" in out:
        c["parity_guard"] = {k: out["parity_guard"][k] for k in ("ok", "max_rel_diff_vs_oracle", "backward_error")}
    # the default batch moved from 8192 (rounds 1-4) to 16384 in round 5 — say which batch `value` is measured on, and
    # carry the 8192-problem figure as a top-level key whenever this run measured it
    c["value_batch_per_gpu"] = cfg["batch_per_gpu"]
    c["value_vals_layout"] = "interleaved" if cfg["kernel"].get("batch_layout") else "problem-major"
    if g("problem_major_layout", "systems_per_s") is not None:
        c["value_problem_major_layout"] = g("problem_major_layout", "systems_per_s")   # rounds 1-5 quoted `value` on this layout
    b8 = g("small_batch", "B8192", "systems_per_s")
    if b8 is not None:
        c["value_at_batch_8192"] = b8
    return c


def _dig(d, path):
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def _k(v):
    return None if v is None else v / 1e3


def extra_blocks(out, torch, hipldl, syn, s, rows, cols, vals, rhs, vals_h, rhs_h, prob, B, dev, local_rank, stream, args):
    """Reported beside `value`, never part of it: small batches, the host-pointer (PCIe-inclusive) entry,
    BASELINE config 2 on the dense backend, and the vectors either side of the system (row f1)."""
    # ---- the headline batch on the reference's problem-major `vals` (what rounds 1-5 quoted) when `value` is on the interleaved layout
    twin = None
    if prob.L.config.get("batch_layout"):
        twin = DeviceProblem(torch, hipldl, s, rows, cols, vals, rhs, B, local_rank, stream, options=parse_options(hipldl, args.opt))
        ms = twin.timed(min(10, max(2, args.steps)), 2)
        same = bool(torch.equal(twin.d, prob.d)) if twin.L.config.get("band_nl") == prob.L.config.get("band_nl") else None
        r = out["roofline"]
        out["problem_major_layout"] = {"systems_per_s": B / (ms * 1e-3), "ms_per_step": ms, "kernel": twin.L.config,
                                       "frac": r["bytes_per_system"] * B / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                       "frac_on_kernel_bytes": (r["kernel_bytes_per_system"] * B / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if r.get("kernel_bytes_per_system") else None,
                                       "d_bit_equal_to_interleaved": same, "all_success": bool((twin.succ == 1).all().item()),
                                       "speedup_of_interleaved": (ms / out["roofline"]["step_ms"]) if out["roofline"]["step_ms"] else None}
        out["value_problem_major_layout"] = B / (ms * 1e-3)
    # ---- small batches of the same pattern: handles planned for latency (staged execution of the elimination tree)
    sb = {}
    # 4608: the chain's 4096 + a remainder of 512 on a handle of its own (cnl_options.split_tail); then two large parts (the
    # bidirectional chain), many large parts, and the bushy tree
    for bs in (8192, 4608, 4096, 1024, 256, 1):
        if bs > B:
            continue
        p2 = DeviceProblem(torch, hipldl, s, rows, cols, vals[:bs], rhs[:bs], bs, local_rank, stream)
        ms = p2.timed(20, 3)
        dh = p2.d[:1].cpu().numpy()
        sb[f"B{bs}"] = {"systems_per_s": bs / (ms * 1e-3), "ms_per_call": ms, "ordering": p2.L.info["order"], "kernel": p2.L.config["kernel"],
                        "fronts": p2.L.info["nsuper"], "all_success": bool((p2.succ == 1).all().item()),
                        "backward_error": backward_error(s, rows, cols, vals_h[0], rhs_h[0], dh[0])}
        if p2.L.config["tail"]:
            sb[f"B{bs}"]["remainder_handle"] = True
        p2.close()
    out["small_batch"] = sb
    # ---- PCIe-inclusive: cnl_newton_system with HOST pointers (what the Julia glue calls): H2D of vals/rhs, the step, D2H of d
    nb = min(len(vals_h), B)
    Lh = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=nb, device=local_rank)
    vv = vals_h[:nb].copy()
    dd = np.zeros((nb, s.N))
    ro = np.zeros(nb)
    hipldl.newton_system_(dd, s.nvar, s.nequ, s.ncon, rhs_h[:nb], vv, Lh, ro, prob.params)
    reps = 3
    tt = time.perf_counter()
    for _ in range(reps):
        hipldl.newton_system_(dd, s.nvar, s.nequ, s.ncon, rhs_h[:nb], vv, Lh, ro, prob.params)
    tw = (time.perf_counter() - tt) / reps
    bytes_sys = 8 * (s.nnzNS + 2 * s.N + s.nvar)
    out["pcie_inclusive"] = {"systems_per_s": nb / tw, "batch": nb, "ms_per_call": tw * 1e3, "bytes_per_system_over_pcie": bytes_sys,
                             "link_GBps": nb * bytes_sys / tw / 1e9, "entry": "cnl_newton_system (host pointers)"}
    Lh.close()
    # ---- BASELINE config 2: dense Jacobian n = 1000, nequ = 2000 on the dense backend (fp64 MFMA roofline)
    try:
        s2 = syn.dense_structure(1000, 2000)
        r2, c2 = s2.kkt_pattern()
        flop = 2000 * 1000 ** 2 + 1000 ** 3 / 3  # m n^2 + n^3 / 3
        c2blk = {"flop_per_system": flop, "peak_spec_TFLOPs": FP64_MFMA_SPEC_TFLOPS, "peak_measured_TFLOPs": FP64_MFMA_MEASURED_TFLOPS}
        gen8 = [syn.dense_values(s2, 2002 + b) for b in range(8)]
        for bs in (1, 8, 32):   # (32: the panel steps' latency is shared by more problems; 8 distinct problems, tiled)
            vh = np.stack([gen8[b % 8][0] for b in range(bs)])
            rh = np.stack([gen8[b % 8][1] for b in range(bs)])
            pv, pr = torch.from_numpy(vh).to(dev), torch.from_numpy(rh).to(dev)
            p3 = DeviceProblem(torch, hipldl, s2, r2, c2, pv, pr, bs, local_rank, stream)
            ms = p3.timed(20, 3)
            dh = p3.d[0].cpu().numpy()
            tf = flop * bs / (ms * 1e-3) / 1e12
            c2blk[f"B{bs}"] = {"ms_per_system": ms / bs, "TFLOPs": tf, "frac_of_spec": tf / FP64_MFMA_SPEC_TFLOPS,
                               "frac_of_measured_mfma": tf / FP64_MFMA_MEASURED_TFLOPS, "kernel": p3.L.config["kernel"],
                               "all_success": bool((p3.succ == 1).all().item()), "backward_error": backward_error(s2, r2, c2, vh[0], rh[0], dh)}
            p3.close()
            del pv, pr
        out["cfg2_dense"] = c2blk
    except Exception as e:  # reported figure, never a reason to fail the bench
        out["cfg2_dense"] = {"error": str(e)}
    # ---- SURVEY 8 row f1 (vectors either side of the system, device-resident), on the headline shapes; algorithmic bytes =
    # J_F and J_c values + r, lambda, F, c read + rhs written (resp. x, r, lambda, d read + xt, rt, lambdat, dlambda written)
    LDLT = (twin or prob).L   # (rows f1 / f4 read problem-major vals)
    sh = stream.cuda_stream
    rv = torch.randn((B, s.nequ), dtype=torch.float64, device=dev)
    lam = torch.randn((B, max(s.ncon, 1)), dtype=torch.float64, device=dev)
    Fx = torch.randn((B, s.nequ), dtype=torch.float64, device=dev)
    cx = torch.randn((B, max(s.ncon, 1)), dtype=torch.float64, device=dev)
    xv = torch.randn((B, s.nvar), dtype=torch.float64, device=dev)
    rhs2 = torch.empty_like(rhs)
    nrm = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    xt, rt, lt, dl = torch.empty_like(xv), torch.empty_like(rv), torch.empty_like(lam), torch.empty_like(lam)

    def timed(fn, reps=5):
        with torch.cuda.stream(stream):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_rv = timed(lambda: hipldl.residual_vectors_dev(LDLT, vals.data_ptr(), rv.data_ptr(), lam.data_ptr(), Fx.data_ptr(),
                                                      cx.data_ptr(), rhs2.data_ptr(), nrm.data_ptr(), sh))
    ms_tp = timed(lambda: hipldl.trial_point_dev(LDLT, xv.data_ptr(), rv.data_ptr(), lam.data_ptr(), prob.d.data_ptr(), 1e4,
                                                 xt.data_ptr(), rt.data_ptr(), lt.data_ptr(), dl.data_ptr(), sh))
    # row f2: the model's value arrays into the segments of a scratch copy of vals (the timed vals are left alone)
    nhF, nhc, njF, njc = len(s.hF[0]), len(s.hc[0]), len(s.jF[0]), len(s.jc[0])
    f2 = None
    try:
        Bp = min(B, 4096)   # (a second vals-sized array: kept small)
        mk = lambda n_: torch.randn((Bp, max(n_, 1)), dtype=torch.float64, device=dev)
        a_hF, a_hc, a_Jx, a_Jc = mk(nhF), mk(nhc), mk(njF), mk(njc)
        a_de = torch.full((Bp,), 1e-8, dtype=torch.float64, device=dev)
        v2 = torch.zeros((Bp, vals.shape[1]), dtype=torch.float64, device=dev)
        Lp = LDLT if Bp == B else hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=Bp)
        ms_p = timed(lambda: hipldl.prepare_newton_system_dev(Lp, nhF, nhc, njF, njc, a_hF.data_ptr(), a_hc.data_ptr() if s.ncon else 0, a_Jx.data_ptr(),
                                                              a_Jc.data_ptr() if s.ncon else 0, a_de.data_ptr() if s.ncon else 0, v2.data_ptr(), sh))
        by_p = 8 * (nhF + nhc + njF + njc + (vals.shape[1] - s.nequ))
        f2 = {"ms": ms_p, "batch": Bp, "bytes_per_system": by_p, "GBps": by_p * Bp / (ms_p * 1e-3) / 1e9, "frac": by_p * Bp / (ms_p * 1e-3) / 1e9 / HBM_PEAK_GBPS}
        if Lp is not LDLT:
            Lp.close()
        if prob.L.config.get("batch_layout"):   # the same pass writing `vals` interleaved (what the headline kernel reads)
            Li = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=Bp, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=1))
            v3 = torch.zeros(hipldl.layout_len(Li, 0), dtype=torch.float64, device=dev)
            ms_i = timed(lambda: hipldl.prepare_newton_system_dev(Li, nhF, nhc, njF, njc, a_hF.data_ptr(), a_hc.data_ptr() if s.ncon else 0, a_Jx.data_ptr(),
                                                                  a_Jc.data_ptr() if s.ncon else 0, a_de.data_ptr() if s.ncon else 0, v3.data_ptr(), sh))
            hipldl.deinterleave_dev(Li, 0, v3.data_ptr(), v2.data_ptr(), sh)   # (v2 holds the problem-major pass's output: compare through a copy)
            f2["interleaved"] = {"ms": ms_i, "GBps": by_p * Bp / (ms_i * 1e-3) / 1e9, "frac": by_p * Bp / (ms_i * 1e-3) / 1e9 / HBM_PEAK_GBPS}
            Li.close()
            del v3
        del a_hF, a_hc, a_Jx, a_Jc, v2
    except Exception as e:   # the extras never take the headline down
        f2 = {"error": str(e)}
    nnzj = len(s.jF[0]) + len(s.jc[0])
    by_rv = 8 * (nnzj + 2 * s.nequ + 2 * s.ncon + s.N)
    by_tp = 8 * (s.nvar + s.nequ + s.ncon + s.N + s.nvar + s.nequ + 2 * s.ncon)
    out["aux_f1"] = {"residual_vectors": {"ms": ms_rv, "bytes_per_system": by_rv, "GBps": by_rv * B / (ms_rv * 1e-3) / 1e9,
                                          "frac": by_rv * B / (ms_rv * 1e-3) / 1e9 / HBM_PEAK_GBPS},
                     "trial_point": {"ms": ms_tp, "bytes_per_system": by_tp, "GBps": by_tp * B / (ms_tp * 1e-3) / 1e9,
                                     "frac": by_tp * B / (ms_tp * 1e-3) / 1e9 / HBM_PEAK_GBPS},
                     "f2_prepare": f2}
    if twin is not None:
        twin.close()
        del twin
    # ---- BASELINE config 4 (n = nequ = 1000, ncon = 10; the config the 1/2/4/8 scaling is defined on) and config 5 (its
    # pattern with the rho ladder climbed to nfact = 6), each on its own algorithmic bytes
    try:
        out["cfg4"], out["cfg5"] = cfg45_blocks(torch, hipldl, syn, dev, local_rank, stream)
    except Exception as e:
        out["cfg4"] = {"error": str(e)}
    # ---- the second front end of DESIGN section 6: ONE process, cnl_multi_newton_system_dev + cnl_multi_synchronize (device list
    # [0] on a one-GPU box), same workload and batch as the headline: must match the single-handle rate
    try:
        dtm, npm, okm, shm = multi_front_end(torch, hipldl, s, rows, cols, [local_rank], B, min(10, max(2, args.steps)), 2)
        rate = npm * min(10, max(2, args.steps)) / dtm
        single = out.get("value_problem_major_layout") or out["value"]   # (the multi front end takes the reference's problem-major arrays)
        out["multi_front_end"] = {"entry": "cnl_multi_newton_system_dev + cnl_multi_synchronize, one process, devices [0]", "systems_per_s": rate,
                                  "ms_per_step": dtm / min(10, max(2, args.steps)) * 1e3, "ratio_to_single_handle": rate / single,
                                  "within_3_percent": abs(rate / single - 1.0) <= 0.03, "all_success": okm, "shards": shm,
                                  "timer": "wall clock (enqueue loop + final synchronize)"}
    except Exception as e:
        out["multi_front_end"] = {"error": str(e)}
    # ---- irregular sparsity whose fill makes fronts of order > 64 (the reference's own benchmark set is general sparsity,
    # docs/src/benchmark.md): batches of such systems run as 64 x 64 tiles on the dense machinery (MFMA trailing updates)
    try:
        out["irregular_sparse"] = irregular_block(torch, hipldl, syn, dev, local_rank, stream)
    except Exception as e:
        out["irregular_sparse"] = {"error": str(e)}
    # ---- the reference's literal call pattern: ONE system per call through host arrays (src/CaNNOLeS.jl:633), and the
    # two-call sequence try_to_factorize + solve_ldl! (src/solver_types.jl:69-98)
    try:
        out["call_pattern_single_system"] = call_pattern_block(torch, hipldl, s, rows, cols, vals_h, rhs_h, dev, local_rank, stream, prob.params)
    except Exception as e:
        out["call_pattern_single_system"] = {"error": str(e)}
    # ---- row f3: whole outer loops (src/CaNNOLeS.jl:418-864) of a closed-form family, device-resident and in lockstep
    from cannoles_jl_amd import device_loop as DL
    Bf = 2048
    fam = DL.BandQuadFamily(syn.band_structure(300, 4), Bf, seed=7, torch=torch, device=dev, curvature=1.5, start=1.0, noise=0.5)
    prm = hipldl.default_params()
    DL.solve_batch_device(fam, prm, device_index=local_rank)
    t0 = time.perf_counter()
    got = DL.solve_batch_device(fam, prm, device_index=local_rank)
    dt = time.perf_counter() - t0
    out["aux_f3"] = {"workload": "band family n=300 p=4 (cfg4 pattern), B=2048 complete solves in lockstep", "problems_per_s": Bf / dt,
                     "global_steps": got["steps"], "ms_per_step": 1e3 * got["loop_seconds"] / got["steps"],
                     "setup_seconds": dt - got["loop_seconds"], "note": "ms_per_step = the global steps alone; problems_per_s includes the symbolic analysis and the start-up evaluations", "newton_systems": int(got["nlinsolve"].sum()),
                     "factorisations": int(got["nfact"].sum()), "first_order": int(sum(st == "first_order" for st in got["status"]))}


def cfg45_blocks(torch, hipldl, syn, dev, local_rank, stream):
    s4 = syn.band_structure(1000, 10, name="cfg4")
    r4, c4 = s4.kkt_pattern()
    blk4 = {"workload": "BASELINE config 4 item: n = nequ = 1000, ncon = 10, band Jacobians"}
    # 32 / 64 / 128: what each of 8 / 4 / 2 GPUs holds under BASELINE config 4's strong scaling (--strong --total 256)
    for bs in (32, 64, 128, 256, 4096):
        vh, rh = band_batch(s4, bs, seed=4000)
        p4 = DeviceProblem(torch, hipldl, s4, r4, c4, torch.from_numpy(vh).to(dev), torch.from_numpy(rh).to(dev), bs, local_rank, stream)
        ms = p4.timed(30 if bs >= 256 else 60, 3)
        p4.L.set_timing(True)
        km = []
        with torch.cuda.stream(stream):
            for _ in range(4):
                p4.step()
                km.append(p4.L.last_kernel_ms())
        p4.L.set_timing(False)
        info = p4.L.info
        nnzl = min(info["nnzL_exact"], CANONICAL_NNZL_CFG4)
        b_alg = 12 * s4.nnzNS + 24 * s4.N + 32 * nnzl
        dh = p4.d[:1].cpu().numpy()
        gbps = b_alg * bs / (ms * 1e-3) / 1e9
        blk4[f"B{bs}"] = {"systems_per_s": bs / (ms * 1e-3), "ms_per_call": ms, "kernel_ms": float(np.mean(km[1:])), "bytes_per_system": b_alg,
                          "nnzL_star": nnzl, "achieved_GBps": gbps, "frac": gbps / HBM_PEAK_GBPS, "frac_of_measured_copy_rate": gbps / HBM_MEASURED_GBPS,
                          "working_set_MB": bs * 8 * (s4.nnzNS + 2 * s4.N + info["lsize"]) / 1e6,
                          "resident_in_infinity_cache": bs * 8 * (s4.nnzNS + 2 * s4.N + info["lsize"]) <= 256 << 20,
                          "ordering": info["order"], "fronts": info["nsuper"], "kernel": p4.L.config["kernel"],
                          "all_success": bool((p4.succ == 1).all().item()), "backward_error": backward_error(s4, r4, c4, vh[0], rh[0], dh[0])}
        p4.close()
    # BASELINE config 4 is a STRONG-scaling config (256 problems over 1/2/4/8 GPUs): the job's rate on G GPUs is 256 / (time of one
    # call on 256 / G problems) — predicted here from this GPU's own small-batch calls (no collective, no data exchange: the ranks
    # do not interact), so that the driver's SCALE record can be judged against a prediction
    if all(f"B{b}" in blk4 for b in (32, 64, 128, 256)):
        blk4["strong_scaling_prediction_total_256"] = {
            f"{g}_gpus": {"problems_per_gpu": 256 // g, "ms_per_step": blk4[f"B{256 // g}"]["ms_per_call"],
                          "systems_per_s": 256 / (blk4[f"B{256 // g}"]["ms_per_call"] * 1e-3),
                          "speedup_vs_1": blk4["B256"]["ms_per_call"] / blk4[f"B{256 // g}"]["ms_per_call"]} for g in (1, 2, 4, 8)}
        blk4["strong_scaling_prediction_total_256"]["note"] = ("latency-bound: a call on 32 problems costs most of what a call on 256 costs (the elimination tree's "
                                                               "critical path), so the curve is nearly flat — by construction of the config, not by a loss in the path")
    # config 5: the same pattern, every problem climbs the ladder to rho = 605.5 (fixture F3: nfact = 6)
    blk5 = {"workload": "BASELINE config 5: config 4's pattern, H_F = -10 on 10 % of the variables, |J| <= 1: nfact = 6 per system"}
    v8 = np.stack([syn.band_values(s4, 5000 + b, stress="ladder")[0] for b in range(8)])
    r8 = np.stack([syn.band_values(s4, 5000 + b, stress="ladder")[1] for b in range(8)])
    for bs in (256, 4096):
        vh, rh = np.tile(v8, (bs // 8, 1)), np.tile(r8, (bs // 8, 1))
        p5 = DeviceProblem(torch, hipldl, s4, r4, c4, torch.from_numpy(vh).to(dev), torch.from_numpy(rh).to(dev), bs, local_rank, stream)
        vals0 = p5.vals.clone()

        def step5():
            p5.vals.copy_(vals0)   # the ladder leaves its rho in the rho slots: restore them (device copy, inside the timed region)
            p5.step()
        with torch.cuda.stream(stream):
            for _ in range(2):
                step5()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(10):
                step5()
            e1.record(stream)
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        nf = p5.nfact.cpu().numpy()
        info = p5.L.info
        nnzl = min(info["nnzL_exact"], CANONICAL_NNZL_CFG4)
        nfm = float(nf.mean())
        b_alg = nfm * (12 * s4.nnzNS + 16 * nnzl) + 16 * nnzl + 24 * s4.N   # factor terms x nfact + the solve terms
        v_end = p5.vals[:1].cpu().numpy()
        dh = p5.d[:1].cpu().numpy()
        gbps = b_alg * bs / (ms * 1e-3) / 1e9
        blk5[f"B{bs}"] = {"systems_per_s": bs / (ms * 1e-3), "factorisations_per_s": bs * nfm / (ms * 1e-3), "ms_per_call": ms, "nfact_mean": nfm,
                          "nfact_min": int(nf.min()), "nfact_max": int(nf.max()), "bytes_per_system": b_alg, "achieved_GBps": gbps,
                          "frac": gbps / HBM_PEAK_GBPS, "kernel": p5.L.config["kernel"], "all_success": bool((p5.succ == 1).all().item()),
                          "rho_final": float(p5.rho[0].item()), "backward_error_with_final_rho": backward_error(s4, r4, c4, v_end[0], rh[0], dh[0]),
                          "note": "device-pointer call (asynchronous): the ladder runs on the device — staged handles climb it inside one fused launch per range "
                                  "of problem groups (every task of the elimination tree a wavefront, per-rung decision on the device; round 4), "
                                  "single-stream handles in their one launch; the timed step includes a device copy that restores the rho slots (0.1 MB per system)"}
        if bs == 256:
            # the same workload through the host-pointer call: the host drives the ladder, every rung a staged try_to_factorize
            # (PCIe transfers of vals / rhs / d included)
            try:
                dhost = np.zeros((bs, s4.N))
                hipldl.newton_system_(dhost, s4.nvar, s4.nequ, s4.ncon, rh, vh.copy(), p5.L, np.zeros(bs), p5.params)
                t0 = time.perf_counter()
                for _ in range(5):
                    outh = hipldl.newton_system_(dhost, s4.nvar, s4.nequ, s4.ncon, rh, vh.copy(), p5.L, np.zeros(bs), p5.params)
                mh = (time.perf_counter() - t0) / 5 * 1e3
                blk5[f"B{bs}"]["host_pointer_call"] = {"systems_per_s": bs / (mh * 1e-3), "ms_per_call": mh, "nfact_mean": float(np.mean(outh[4])),
                                                       "all_success": bool(np.all(outh[1])), "note": "PCIe-inclusive (24.6 MB go up through pageable memory); the ladder runs on the device inside the fused launch (round 3: driven from the host, 2.35 ms)"}
            except Exception as e:
                blk5[f"B{bs}"]["host_pointer_call"] = {"error": str(e)}
        p5.close()
    return blk4, blk5


def irregular_block(torch, hipldl, syn, dev, local_rank, stream):
    s5 = syn.random_structure(120, 130, 6, 0.03, 3)   # the parity tests' irregular family: condensed order 126, fronts up to 95
    r5, c5 = s5.kkt_pattern()
    v8, r8 = syn.batch_values(s5, 8, cfg=3, gen=syn.random_values)
    blk = {"workload": "random pattern n=120 nequ=130 ncon=6, density 0.03 (fronts of order up to 95)"}
    for bs in (640, 4096):
        vh, rh = np.tile(v8, (bs // 8, 1)), np.tile(r8, (bs // 8, 1))
        p5 = DeviceProblem(torch, hipldl, s5, r5, c5, torch.from_numpy(vh).to(dev), torch.from_numpy(rh).to(dev), bs, local_rank, stream)
        ms = p5.timed(20, 3)
        dh = p5.d[:1].cpu().numpy()
        blk[f"B{bs}"] = {"systems_per_s": bs / (ms * 1e-3), "ms_per_call": ms, "kernel": p5.L.config["kernel"], "fmax": p5.L.info["fmax"],
                         "all_success": bool((p5.succ == 1).all().item()), "backward_error": backward_error(s5, r5, c5, vh[0], rh[0], dh[0])}
        p5.close()
    return blk


def call_pattern_block(torch, hipldl, s, rows, cols, vals_h, rhs_h, dev, local_rank, stream, params):
    """One system per call, as `newton_system!` is called by the reference (host arrays), and the two-call sequence; wall-clock
    medians over repeated calls on one handle of batch 1."""
    L1 = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=1, device=local_rank)
    v1, r1 = vals_h[0].copy(), rhs_h[0].copy()
    d1 = np.zeros(s.N)

    def med(fn, reps=30):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts) * 1e3)

    res = {"entry": "host pointers, pageable numpy arrays, batch 1, cfg3 pattern"}
    # the one-time cost in front of the first call of a drop-in solver object (the reference: sparse + triu + ldl_analyze,
    # src/solver_types.jl:61-65): the host-side symbolic analysis cnl_create runs for this batch size (candidate orders on host threads)
    ta = []
    for _ in range(3):
        t0 = time.perf_counter()
        pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=1)
        ta.append(time.perf_counter() - t0)
        del pl
    res["analysis_s"] = float(np.median(ta))
    res["analysis_host_threads"] = min(16, os.cpu_count() or 1)
    res["newton_system_ms"] = med(lambda: hipldl.newton_system_(d1, s.nvar, s.nequ, s.ncon, r1, v1, L1, 0.0, params))
    res["try_to_factorize_ms"] = med(lambda: hipldl.try_to_factorize(L1, v1, s.nvar, s.nequ, s.ncon, params[0]))
    res["solve_ldl_ms"] = med(lambda: hipldl.solve_ldl_(r1, L1.factor, d1))
    res["two_call_total_ms"] = res["try_to_factorize_ms"] + res["solve_ldl_ms"]
    # the same call on a system that climbs the rho ladder (nfact = 6, BASELINE config 5's stress on this pattern): the host drives
    # the ladder, every rung a staged try_to_factorize (csrc/capi.cpp; the device ladder of the sequential launch: ~39 ms)
    try:
        from cannoles_jl_amd import synthetic as syn_
        vl, rl = syn_.batch_values(s, 1, cfg=5, stress="ladder")
        vl0 = vl[0].copy()
        outl = {}

        def ladder_call():
            outl["r"] = hipldl.newton_system_(d1, s.nvar, s.nequ, s.ncon, rl[0], vl0.copy(), L1, 0.0, params)
        res["newton_system_nfact6_ms"] = med(ladder_call, reps=10)
        res["nfact6_check"] = {"nfact": int(outl["r"][4]), "success": bool(outl["r"][1])}
    except Exception as e:
        res["newton_system_nfact6_ms"] = {"error": str(e)}
    # device-resident twins of the same three calls (HIP events)
    tv, tr = torch.from_numpy(v1[None].copy()).to(dev), torch.from_numpy(r1[None].copy()).to(dev)
    td = torch.zeros((1, s.N), dtype=torch.float64, device=dev)
    su = torch.zeros(1, dtype=torch.int32, device=dev)
    ro, rho = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    nf = torch.zeros(1, dtype=torch.int32, device=dev)
    sh = stream.cuda_stream

    def ev(fn, reps=40):
        with torch.cuda.stream(stream):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    lib = hipldl.lib()
    res["dev_newton_system_ms"] = ev(lambda: hipldl.newton_system_dev(L1, tv.data_ptr(), tr.data_ptr(), td.data_ptr(), ro.data_ptr(), rho.data_ptr(),
                                                                      nf.data_ptr(), su.data_ptr(), params, sh))
    res["dev_try_to_factorize_ms"] = ev(lambda: hipldl._check(lib.cnl_factorize_dev(L1._h, tv.data_ptr(), float(params[0]), su.data_ptr(), sh)))
    res["dev_solve_ldl_ms"] = ev(lambda: hipldl._check(lib.cnl_solve_dev(L1._h, tr.data_ptr(), td.data_ptr(), sh)))
    L1.close()
    return res


def oracle_split(O, s, rows, cols, perm64, vals_h, rhs_h, params, nsys):
    """assemble (set_vals!) / factorize + inertia / solve split of the restated reference path on one host core"""
    orc = O.Oracle(s.N, rows, cols, perm64)
    t_set = t_fac = t_sol = 0.0
    for b in range(nsys):
        t0 = time.perf_counter()
        orc.set_vals(vals_h[b])
        t1 = time.perf_counter()
        orc.try_to_factorize(vals_h[b], s.nvar, s.nequ, s.ncon, params[0])   # = set_vals! + ldl_factorize! + inertia
        t2 = time.perf_counter()
        orc.solve_ldl(rhs_h[b])
        t3 = time.perf_counter()
        t_set += t1 - t0
        t_fac += max(0.0, (t2 - t1) - (t1 - t0))
        t_sol += t3 - t2
    tot = t_set + t_fac + t_sol
    return {"systems": nsys, "systems_per_s": nsys / tot, "ms_per_system": 1e3 * tot / nsys, "assemble_ms": 1e3 * t_set / nsys,
            "factorize_ms": 1e3 * t_fac / nsys, "solve_ms": 1e3 * t_sol / nsys, "cores": 1, "nnzL": orc.nnzL}


def cpu_baseline(out, s, rows, cols, vals_h, rhs_h, prob, LDLT, args):
    """The oracle (restated LDLFactorizations path) on a bounded sample of the same workload, on the GPU box's host cores.
    A reported baseline, not the optimisation target."""
    from oracle import oracle as O
    params = prob.params
    # the oracle gets the product's own fill-reducing order (the fairest CPU baseline; the canonical r/x/lambda order of
    # SURVEY.md has 2.4x the fill)
    perm64 = LDLT.plan_array("perm").astype(np.int64)
    orc = O.Oracle(s.N, rows, cols, perm64)
    ncpu = args.cpu_sample
    if ncpu < 0:
        tt = time.perf_counter()
        O.newton_system_batch(orc, 1, s.nvar, s.nequ, s.ncon, rhs_h[:1], vals_h[:1].copy(), None, params)
        one = time.perf_counter() - tt
        ncpu = int(max(4, min(len(vals_h), 10.0 / max(one, 1e-4))))
    ncpu = min(ncpu, len(vals_h))
    tt = time.perf_counter()
    d0, ok0, _, _, nf0 = O.newton_system_batch(orc, ncpu, s.nvar, s.nequ, s.ncon, rhs_h[:ncpu], vals_h[:ncpu].copy(), None, params)
    tc = time.perf_counter() - tt
    dg = prob.d[:min(ncpu, 8)].cpu().numpy()
    perr = float(np.abs(dg - d0[:len(dg)]).max() / np.abs(d0[:len(dg)]).max())
    cb = {"value": ncpu / tc, "unit": "systems/s", "cores": 1, "kind": "port",
          "sample": f"first {ncpu} problems of rank 0's batch, oracle/cnl_oracle.c (restated LDLFactorizations up-looking LDL^T, scatter-map "
                    f"set_vals!, the product's own ordering, nnzL={orc.nnzL}), host has {os.cpu_count()} logical cores",
          "max_rel_diff_vs_gpu": perr}
    # the variant whose assembly mimics the reference's set_vals! literally: one binary search per entry in a CSC column
    # (/root/reference/src/solver_types.jl:53-59) — what the reference actually pays per factorisation
    try:
        orb = O.Oracle(s.N, rows, cols, perm64)
        orb.set_mode = 1
        nb = max(2, ncpu // 4)
        tt = time.perf_counter()
        O.newton_system_batch(orb, nb, s.nvar, s.nequ, s.ncon, rhs_h[:nb], vals_h[:nb].copy(), None, params)
        cb["set_vals_binary_search"] = {"value": nb / (time.perf_counter() - tt), "systems": nb, "cores": 1}
    except Exception as e:
        cb["set_vals_binary_search"] = {"error": str(e)}
    # the same port on ALL host cores, one problem per thread ("(ii) all host cores"); each thread owns an oracle
    # object, the ctypes calls release the GIL.  Bounded to a few seconds; `cores` above stays the contract's figure.
    try:
        import concurrent.futures as cf
        nthr = max(1, min(len(os.sched_getaffinity(0)), len(vals_h)))
        per = max(1, len(vals_h) // nthr)  # problems per thread (its slice of the first chunk)
        orcs = [O.Oracle(s.N, rows, cols, perm64) for _ in range(nthr)]
        deadline = time.perf_counter() + 4.0
        done = [0] * nthr

        def work(k):
            lo = k * per
            while time.perf_counter() < deadline:
                O.newton_system_batch(orcs[k], per, s.nvar, s.nequ, s.ncon, rhs_h[lo:lo + per], vals_h[lo:lo + per].copy(), None, params)
                done[k] += per

        tt = time.perf_counter()
        with cf.ThreadPoolExecutor(nthr) as ex:
            list(ex.map(work, range(nthr)))
        ta = time.perf_counter() - tt
        cb["all_cores"] = {"value": sum(done) / ta, "threads": nthr, "systems": sum(done)}
    except Exception as e:
        cb["all_cores"] = {"error": str(e)}
    # the assemble / factorize / solve split on the headline pattern, and the same for configs 4 and 2 with the
    # orderings the product chose for them (bounded samples; cfg2's restated up-looking factorisation takes seconds per system)
    try:
        import cannoles_jl_amd  # noqa: F401
        from cannoles_jl_amd import hipldl, synthetic as syn
        cb["split_cfg3"] = oracle_split(O, s, rows, cols, perm64, vals_h, rhs_h, params, min(8, len(vals_h)))
        if not args.no_extras:
            s4 = syn.band_structure(1000, 10)
            r4, c4 = s4.kkt_pattern()
            pl4 = hipldl.Plan(s4.N, r4, c4, s4.nvar, s4.nequ, s4.ncon, batch=256)
            v4, rh4 = band_batch(s4, 64, seed=4000)
            cb["cfg4"] = oracle_split(O, s4, r4, c4, pl4.array("perm").astype(np.int64), v4, rh4, params, 64)
            s2 = syn.dense_structure(1000, 2000)
            r2, c2 = s2.kkt_pattern()
            pl2 = hipldl.Plan(s2.N, r2, c2, s2.nvar, s2.nequ, s2.ncon, batch=1)
            v2, rh2 = syn.dense_values(s2, 2002)
            cb["cfg2"] = oracle_split(O, s2, r2, c2, pl2.array("perm").astype(np.int64), v2[None], rh2[None], params, 1)
        cb["note"] = ("all_cores / cores = %.1f x one core on %d logical cores: the host leg is memory-bound (every thread streams its own "
                      "factor through the shared memory system), not compute-bound" % (cb.get("all_cores", {}).get("value", 0) / cb["value"], os.cpu_count()))
    except Exception as e:
        cb["split_error"] = str(e)
    out["cpu_baseline"] = cb


if __name__ == "__main__":
    main()
