"""What vicgpu_prefetch_forcing_perturbed saves a perturbed-forcing ensemble, on a GPU:

    python tools/forcing_perturb_ab.py [--out profiles/forcing_perturb_ab.json] [--reps 3] [--members 16] [--columns 6250] [--merge]

The workload of tools/forcing_map_ab.py: 16 members x 6 250 columns -- the 100 000 cells x 25 HRUs of bench.py's cfg3 -- in
24-step hourly chunks, every member with its own factors at every step (domain.member_perturbations).
    side a  numpy builds the perturbed 100 000-wide raw table into pinned memory, member by member, then
            vicgpu_prefetch_forcing_raw + vicgpu_swap_forcing + vicgpu_synchronize
    side b  vicgpu_prefetch_forcing_perturbed on the 6 250-wide table with the same factors, then the same two calls
Per side, per repetition and as medians after a warm-up: the host wall time per chunk split into numpy and call, the bytes
uploaded, and the derivation kernels' device time (a second model under VICGPU_STATS, whose report on stderr is read back); then
24 steps from the same state on each side's chunk and whether the states are identical (they must be); then three chunks
streamed with prefetch(k + 1) issued before step(k), wall time per side.
--merge keeps what the output file already holds under other keys (the default-path A/B of tools/ab.sh)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from tools.forcing_map_ab import CHUNK, RAW_FROM

STD = {"VIC_RAW_PREC": 0.5, "VIC_RAW_SHORTWAVE": 0.2, "VIC_RAW_AIR_TEMP": 2.0, "VIC_RAW_LONGWAVE": 10.0}
NSTREAM = 3      # chunks of the streamed run


def stderr_of(fn):
    """What the library writes to file descriptor 2 while fn runs."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forcing_perturb_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("forcing_perturb_ab.py measures on a GPU: none is visible")
    import bench
    from vic_amd import domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol = cfg["opt"], args.members, args.columns
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    nsteps = CHUNK * NSTREAM
    f, _, dmy = domain.make_forcing(base, 0, nsteps, start_doy=cfg["start_doy"])
    D, _ = domain.tile_members(base, M)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    pert, _ = domain.member_perturbations(M, nsteps, float(opt.dt), STD, 24.0, seed=20261020)
    col_src = np.ascontiguousarray(np.tile(np.arange(ncol, dtype=np.int32), M))
    col_group = np.ascontiguousarray(np.repeat(np.arange(M, dtype=np.int32), ncol))
    os.environ.pop("VICGPU_STATS", None)
    model = Model(D)
    shared = model.pinned((nsteps, C["VIC_NRAW"], opt.dt, ncol))
    for name, src, scale in RAW_FROM:                # snow_step == 1 hour: the derivation gives the table back
        shared[:, C[name]] = f[:, C[src], :opt.NF] * scale
    wide = [model.pinned((CHUNK, C["VIC_NRAW"], opt.dt, D.ncell)) for _ in range(2)]      # side a's table, double-buffered for the streamed run

    def build_wide(buf, k):
        """numpy's side: chunk k of the shared table, expanded and perturbed member by member, straight into pinned memory."""
        s = slice(k * CHUNK, (k + 1) * CHUNK)
        x, p = shared[s], pert[s]
        for m in range(M):
            out = buf[..., m * ncol:(m + 1) * ncol]
            np.multiply(x, p[:, 0::2, None, m, None], out=out)
            out += p[:, 1::2, None, m, None]

    def prefetch(m, side, k, buf=0):
        """(numpy ms, call ms) of staging chunk k."""
        s = slice(k * CHUNK, (k + 1) * CHUNK)
        t0 = time.perf_counter()
        if side == "a":
            build_wide(wide[buf], k)
        t1 = time.perf_counter()
        if side == "a":
            m.prefetch_forcing_raw(wide[buf], dmy[s], min_wind_speed=0.0, plapse=True)
        else:
            m.prefetch_forcing_perturbed(shared[s], dmy[s], col_src, col_group, pert[s], min_wind_speed=0.0, plapse=True)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def chunk_leg(m, side):
        m.synchronize()
        tn, tc = prefetch(m, side, 0)
        t0 = time.perf_counter()
        m.swap_forcing(); m.synchronize()
        return tn, tc + (time.perf_counter() - t0) * 1e3

    def reset(m):
        m.set_state(sd0, si0)
        m.put_data_config(bench.OUT_STEP_RATIO)
        m.put_data_init()
        m.synchronize()

    def streamed(m, side):
        reset(m)
        t0 = time.perf_counter()
        prefetch(m, side, 0, 0); m.swap_forcing()
        for k in range(NSTREAM):
            if k + 1 < NSTREAM:
                prefetch(m, side, k + 1, (k + 1) % 2)
            m.dist_prec(0, CHUNK, sync=False)
            if k + 1 < NSTREAM:
                m.swap_forcing()
        m.synchronize()
        return (time.perf_counter() - t0) * 1e3

    nrep = max(args.reps, 3)
    res = {s: dict(numpy_ms=[], call_ms=[], streamed_ms=[]) for s in "ab"}
    for s in "ab":
        chunk_leg(model, s)                          # first touch: allocations, code objects
    for _ in range(nrep):
        for s in "ab":
            tn, tc = chunk_leg(model, s)
            res[s]["numpy_ms"].append(round(tn, 3)); res[s]["call_ms"].append(round(tc, 3))
    state = {}
    for s in "ab":                                   # 24 steps on each side's chunk from the same state
        reset(model)
        chunk_leg(model, s)
        model.dist_prec(0, CHUNK)
        state[s] = model.get_state()
    identical = bool(np.array_equal(state["a"][0], state["b"][0], equal_nan=True) and np.array_equal(state["a"][1], state["b"][1]))
    del state
    for s in "ab":
        streamed(model, s)
    for _ in range(nrep):
        for s in "ab":
            res[s]["streamed_ms"].append(round(streamed(model, s), 2))

    # the derivation kernels' device time: the library's own report under VICGPU_STATS, from a model of its own
    os.environ["VICGPU_STATS"] = "1"
    derive = {}

    def stats_run():
        m2 = Model(D)
        for s in "ab":
            for _ in range(nrep + 1):
                chunk_leg(m2, s)
        m2.close()
    try:
        log = stderr_of(stats_run)
    finally:
        os.environ.pop("VICGPU_STATS", None)
    ms = [float(x) for x in re.findall(r"forcing derive: .*?: ([0-9.]+) ms", log)]
    if len(ms) == 2 * (nrep + 1):
        derive = {"a": ms[1:nrep + 1], "b": ms[nrep + 2:]}
    model.close()                                    # the pinned tables are its

    raw_bytes = lambda width: CHUNK * C["VIC_NRAW"] * opt.dt * width * 8
    up = {"a": raw_bytes(D.ncell), "b": raw_bytes(ncol) + pert[:CHUNK].nbytes + col_src.nbytes + col_group.nbytes}
    for s in "ab":
        r = res[s]
        r["bytes_uploaded_per_chunk"] = int(up[s])
        r["derive_kernels_ms"] = derive.get(s)
        for k in ("numpy_ms", "call_ms", "streamed_ms"):
            r[k + "_median"] = float(np.median(r[k]))
        r["host_ms_per_chunk_median"] = round(r["numpy_ms_median"] + r["call_ms_median"], 3)
        r["derive_kernels_ms_median"] = float(np.median(r["derive_kernels_ms"])) if r["derive_kernels_ms"] else None
    a, b = res["a"], res["b"]
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), chunk_steps=CHUNK,
               streamed_chunks=NSTREAM, std=STD, tau_hours=24.0,
               a="numpy builds the perturbed ncell-wide raw table into pinned memory; vicgpu_prefetch_forcing_raw + swap + synchronize",
               b="vicgpu_prefetch_forcing_perturbed on the shared table with the same factors; swap + synchronize",
               same_state_after_24_steps=identical, side_a=a, side_b=b,
               b_over_a=dict(bytes_uploaded=round(up["b"] / up["a"], 4),
                             host_ms_per_chunk=round(b["host_ms_per_chunk_median"] / a["host_ms_per_chunk_median"], 4),
                             call_ms=round(b["call_ms_median"] / a["call_ms_median"], 4),
                             streamed_ms=round(b["streamed_ms_median"] / a["streamed_ms_median"], 4)))
    print(json.dumps(out), flush=True)
    doc = {}
    if args.merge and os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc["ensemble"] = out
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    if not identical:
        raise SystemExit("the two sides end in different states")


if __name__ == "__main__":
    main()
