"""What a forcing map (vicgpu_set_forcing_map) saves an ensemble, on a GPU:

    python tools/forcing_map_ab.py [--out profiles/forcing_map_ab.json] [--reps 3] [--members 16] [--columns 6250] [--merge]

A 16-member ensemble of 6 250 columns -- the 100 000 cells x 25 HRUs of bench.py's cfg3 -- runs on one Model, alternating
between the identity map with the hourly raw forcing replicated per cell (the baseline) and the member-major map of
domain.tile_members with the 6 250-wide table.  Reported for both, per repetition and as medians:
    forcing bytes of a one-day chunk (24 steps) in pinned host memory and in one device slot (raw + derived rows + flags)
    the wall time of vicgpu_prefetch_forcing_raw + vicgpu_swap_forcing for that chunk from pinned memory (transfer + derivation)
    ms_per_step: the wall time of the timed steps (put_data on, as in bench.py) over their number
and whether the two runs end in the same state, bit for bit (they must: the members read the same numbers either way).
--merge keeps what the output file already holds under other keys (the default-path A/B of tools/ab.sh)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CHUNK = 24      # steps of a one-day chunk
RAW_FROM = (("VIC_RAW_AIR_TEMP", "VIC_F_AIR_TEMP", 1.0), ("VIC_RAW_PREC", "VIC_F_PREC", 1.0), ("VIC_RAW_PRESSURE_KPA", "VIC_F_PRESSURE", 1e-3),
            ("VIC_RAW_VP_KPA", "VIC_F_VP", 1e-3), ("VIC_RAW_SHORTWAVE", "VIC_F_SHORTWAVE", 1.0), ("VIC_RAW_LONGWAVE", "VIC_F_LONGWAVE", 1.0),
            ("VIC_RAW_WIND", "VIC_F_WIND", 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forcing_map_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("forcing_map_ab.py measures on a GPU: none is visible")
    import bench
    from vic_amd import domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol = cfg["opt"], args.members, args.columns
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, _, dmy = domain.make_forcing(base, 0, CHUNK, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    for m in range(M):                               # a calibration ensemble: every member its own infiltration and baseflow shape
        s = slice(m * ncol, (m + 1) * ncol)
        D.cell_params[C["CP_B_INFILT"], s] *= 1.0 + 0.04 * m
        D.cell_params[C["CP_DS"], s] *= 1.0 + 0.03 * m
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    model = Model(D)
    raw = {"mapped": model.pinned((CHUNK, C["VIC_NRAW"], opt.dt, ncol)), "replicated": model.pinned((CHUNK, C["VIC_NRAW"], opt.dt, D.ncell))}
    for name, src, scale in RAW_FROM:                # snow_step == 1 hour: the derivation gives the table back
        raw["mapped"][:, C[name]] = f[:, C[src], :opt.NF] * scale
    raw["replicated"][...] = np.tile(raw["mapped"], (1, 1, 1, M))
    nsub = opt.NR + 1

    def forcing_bytes(width):
        host = CHUNK * C["VIC_NRAW"] * opt.dt * width * 8
        return dict(host_pinned=host, device_slot=host + CHUNK * C["VIC_NFORCE"] * nsub * width * 8 + CHUNK * nsub * D.ncell)

    def leg(kind, want_state=False):
        model.set_forcing_map(cell_col if kind == "mapped" else None, ncol if kind == "mapped" else None)
        model.set_state(sd0, si0)
        model.put_data_config(bench.OUT_STEP_RATIO)
        model.put_data_init()
        model.synchronize()
        t0 = time.perf_counter()
        model.prefetch_forcing_raw(raw[kind], dmy, min_wind_speed=0.0, plapse=True)
        model.swap_forcing()
        t_prefetch = time.perf_counter() - t0
        model.dist_prec(0, args.warmup)
        t0 = time.perf_counter()
        model.dist_prec(args.warmup, args.steps)
        t_steps = time.perf_counter() - t0
        return t_prefetch * 1e3, t_steps * 1e3 / args.steps, model.get_state() if want_state else None

    leg("replicated"); leg("mapped")                 # first touch of both widths: allocations, code objects
    res = {k: dict(prefetch_raw_ms=[], ms_per_step=[]) for k in ("replicated", "mapped")}
    state = {}
    nrep = max(args.reps, 3)
    for i in range(nrep):
        for kind in ("replicated", "mapped"):
            p, s, state[kind] = leg(kind, want_state=i == nrep - 1)      # the state tables are gigabytes: read once
            res[kind]["prefetch_raw_ms"].append(round(p, 3))
            res[kind]["ms_per_step"].append(round(s, 3))
    identical = bool(np.array_equal(state["replicated"][0], state["mapped"][0], equal_nan=True) and np.array_equal(state["replicated"][1], state["mapped"][1]))
    model.close()
    for kind, width in (("replicated", D.ncell), ("mapped", ncol)):
        r = res[kind]
        r["forcing_bytes_per_chunk"] = forcing_bytes(width)
        r["prefetch_raw_ms_median"] = float(np.median(r["prefetch_raw_ms"]))
        r["ms_per_step_median"] = float(np.median(r["ms_per_step"]))
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), chunk_steps=CHUNK,
               timed_steps=args.steps, warmup_steps=args.warmup, baseline="replicated", same_final_state=identical,
               replicated=res["replicated"], mapped=res["mapped"],
               mapped_over_replicated=dict(
                   host_bytes=round(res["mapped"]["forcing_bytes_per_chunk"]["host_pinned"] / res["replicated"]["forcing_bytes_per_chunk"]["host_pinned"], 4),
                   device_bytes=round(res["mapped"]["forcing_bytes_per_chunk"]["device_slot"] / res["replicated"]["forcing_bytes_per_chunk"]["device_slot"], 4),
                   prefetch_raw_ms=round(res["mapped"]["prefetch_raw_ms_median"] / res["replicated"]["prefetch_raw_ms_median"], 4),
                   ms_per_step=round(res["mapped"]["ms_per_step_median"] / res["replicated"]["ms_per_step_median"], 4)))
    print(json.dumps(out), flush=True)
    doc = {}
    if args.merge and os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc["ensemble"] = out
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    if not identical:
        raise SystemExit("the mapped and the replicated run end in different states")


if __name__ == "__main__":
    main()
