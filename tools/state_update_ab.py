"""What an analysis update costs an ensemble on the device, on a GPU, next to the only path there was before it:

    python tools/state_update_ab.py [--out profiles/state_update_ab.json] [--reps 3] [--members 16] [--columns 6250] [--merge]

The 16-member ensemble of tools/forcing_map_ab.py (6 250 columns, the 100 000 cells x 25 HRUs of bench.py's cfg3) on one Model,
in one process, after one step.  The analysis update reads SD_SNOW_SWQ and SD_MOIST0..2 of all HRUs, adds increments to them
and makes the node blocks consistent with the new moisture (VICGPU_DERIVE_CAP_MOIST | VICGPU_DERIVE_NODES over all HRUs).
Timed as wall time on the host, each after a warm-up, as medians over --reps repetitions with their spread:
    device_path   vicgpu_get_state_rows, vicgpu_update_state (ADD), vicgpu_derive_soil_state, vicgpu_synchronize; and its legs
    host_path     vicgpu_get_state, the same increments, the cap and distribute_node_moisture_properties of
                  vic_amd/init_state.py with numpy, vicgpu_set_state; and its legs
and how far the two paths' states are apart (the device functions against the numpy restatement).
--merge keeps what the output file already holds under other keys (the default-path A/B of tools/ab.sh).
Nothing is gated: the numbers are reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def spread(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)), all=[round(float(v), 3) for v in x])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_update_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("state_update_ab.py measures on a GPU: none is visible")
    import bench
    from vic_amd import abi, domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol = cfg["opt"], args.members, args.columns
    Nn = opt.Nnode
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, _, dmy = domain.make_forcing(base, 0, 2, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    sf = domain.make_snowflag(D, f, cell_col)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    cell = D.hru_iparams[C["HPI_CELL"]]
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"]], np.int32)
    mo = rows[1:]
    ic = np.array([C["SD_ICE0"] + l for l in range(3)], np.int32)
    node = {k: np.array([abi.sd_node(C[k], n, Nn) for n in range(Nn)], np.int32) for k in ("SDN_T", "SDN_MOIST", "SDN_ICE", "SDN_KAPPA", "SDN_CS")}
    mm = init_state._layer(D.cell_params, "CPL_MAX_MOIST", cell)
    rng = np.random.default_rng(1)
    # increments of a few percent; every tenth HRU is pushed above the maximum of layer 0
    inc = np.empty((4, D.nhru))
    inc[0] = 0.002 * rng.uniform(size=D.nhru)
    inc[1:] = 0.03 * mm * rng.uniform(-1.0, 1.0, size=(3, D.nhru))
    inc[1, ::10] = mm[0, ::10]
    what = C["VICGPU_DERIVE_CAP_MOIST"] | C["VICGPU_DERIVE_NODES"]
    nrep = max(args.reps, 3)

    model = Model(D)
    model.set_forcing_map(cell_col, ncol)
    model.set_state(sd0, si0)
    model.push_forcing(f, sf, dmy)
    model.dist_prec(0, 1)
    sd1, si1 = model.get_state()

    def clock(legs, fn):
        model.synchronize()
        t0 = time.perf_counter()
        r = fn()
        legs.append((time.perf_counter() - t0) * 1e3)
        return r

    def device_path(t):
        model.set_state(sd1, si1)
        clock(t["get_state_rows"], lambda: model.get_state_rows(rows))
        clock(t["update_state"], lambda: (model.update_state(rows, inc, mode=Model.ADD), model.synchronize()))
        clock(t["derive_soil_state"], lambda: (model.derive_soil_state(what), model.synchronize()))
        t["total"].append(t["get_state_rows"][-1] + t["update_state"][-1] + t["derive_soil_state"][-1])

    def host_path(t):
        model.set_state(sd1, si1)
        sd, si = clock(t["get_state"], model.get_state)

        def numpy_part():
            sd[rows] = sd[rows] + inc
            moist, ice = sd[mo], sd[ic]
            over = moist > mm
            with np.errstate(all="ignore"):
                ice = np.where(over, ice * (mm / moist), ice)
            moist = np.where(over, mm, moist)
            sd[mo], sd[ic] = moist, np.where(ice > moist, moist, ice)
            blocks = init_state.distribute_node_moisture_properties(opt, D.cell_params, cell, sd[node["SDN_T"]], moist)
            for k, b in zip(("SDN_MOIST", "SDN_ICE", "SDN_KAPPA", "SDN_CS"), blocks):
                sd[node[k]] = b
        clock(t["numpy"], numpy_part)
        clock(t["set_state"], lambda: model.set_state(sd, si))
        t["total"].append(t["get_state"][-1] + t["numpy"][-1] + t["set_state"][-1])

    td = {k: [] for k in ("get_state_rows", "update_state", "derive_soil_state", "total")}
    th = {k: [] for k in ("get_state", "numpy", "set_state", "total")}
    for r in range(nrep + 1):                             # the first round is a warm-up; the paths alternate
        device_path(td)
        sd_dev = model.get_state()[0] if r == nrep else None
        host_path(th)
    sd_host = model.get_state()[0]
    with np.errstate(all="ignore"):
        d = np.abs(sd_dev - sd_host) / np.maximum(1e-12, np.maximum(np.abs(sd_dev), np.abs(sd_host)))
    d = np.where(np.isnan(sd_dev) & np.isnan(sd_host), 0.0, d)
    apart = float(np.nanmax(d))
    capped = int((sd1[mo] + inc[1:] > mm).any(axis=0).sum())
    model.close()
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), reps=nrep,
               sd_rows=int(sd0.shape[0]), rows_updated=int(len(rows)), hrus_capped=capped, stage_budget_mb=int(os.environ.get("VICGPU_COPY_STAGE_MB", "256")),
               state_bytes_each_way=int(sd0.nbytes + si0.nbytes), listed_bytes_each_way=int(8 * len(rows) * D.nhru),
               device_path_wall_ms={k: spread(v[1:]) for k, v in td.items()},
               host_path_wall_ms={k: spread(v[1:]) for k, v in th.items()},
               device_over_host=round(float(np.median(td["total"][1:]) / np.median(th["total"][1:])), 5),
               paths_apart_rel=apart)
    print(json.dumps(out), flush=True)
    keep = {}
    if args.merge and os.path.exists(args.out):
        keep = json.load(open(args.out))
    keep.update(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(keep, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
