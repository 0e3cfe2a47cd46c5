"""What vicgpu_update_cell_params costs an ensemble, on a GPU, next to the only path there was before it:

    python tools/update_params_ab.py [--out profiles/update_params_ab.json] [--reps 3] [--members 16] [--columns 6250]

The 16-member ensemble of tools/forcing_map_ab.py (6 250 columns, the 100 000 cells x 25 HRUs of bench.py's cfg3) on one Model,
in one process, with a forcing map, a forcing chunk, put_data, a records configuration and one cell group per member in force.
Timed as wall time on the host, each after a warm-up call, as medians over --reps repetitions with their spread:
    dense_8 / dense_all     vicgpu_update_cell_params of all cells (no list), 8 rows / every row, plus vicgpu_synchronize
    listed_8 / listed_all   the same rows for the cells of one member
    set_domain_path         the same change the way it had to be made before: state and fluxes read back, vicgpu_set_domain with
                            the changed table, then forcing map, state, fluxes, forcing chunk, put_data, records and groups set
                            again (put_data's bookkeeping cannot be set: that path loses it)
    step_ms                 a vicgpu_step of one step plus vicgpu_synchronize from the same state (set again before every timed
                            step), without an update before it and right behind one that writes the values the table already
                            holds, so that both steps do the same work: the step is not slowed
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_params_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("update_params_ab.py measures on a GPU: none is visible")
    import bench
    from vic_amd import abi, domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol = cfg["opt"], args.members, args.columns
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, _, dmy = domain.make_forcing(base, 0, 2, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    sf = domain.make_snowflag(D, f, cell_col)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    names = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP"]
    group_off = np.arange(0, D.ncell + 1, ncol, dtype=np.int32)
    group_cell = np.arange(D.ncell, dtype=np.int32)
    nrep = max(args.reps, 3)
    ncp = D.cell_params.shape[0]
    rows8 = np.array([C["CP_B_INFILT"], C["CP_DS"], C["CP_DSMAX"], C["CP_WS"]] + [abi.cp_layer(C["CPL_KSAT"], l) for l in range(3)]
                     + [abi.cp_layer(C["CPL_EXPT"], 2)], np.int32)
    rows_all = np.arange(ncp, dtype=np.int32)
    member = (np.arange(ncol) + ncol).astype(np.int32)                  # the cells of member 1

    def establish(model, sd, si, fx):
        model.set_forcing_map(cell_col, ncol)
        model.set_state(sd, si)
        if fx is not None:
            model.set_fluxes(fx)
        model.push_forcing(f, sf, dmy)
        model.put_data_config(bench.OUT_STEP_RATIO)
        model.put_data_init()
        model.records_config(names, depth=2)
        model.records_set_groups(group_off, group_cell)
        model.synchronize()

    model = Model(D)
    establish(model, sd0, si0, None)

    def timed(fn):
        model.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def step():
        model.dist_prec(0, 1)

    def values(rows, cells, k):
        """the current rows with the soil rows of rows8 scaled: a new generation"""
        v = D.cell_params[rows] if cells is None else D.cell_params[np.ix_(rows, cells)]
        v = np.ascontiguousarray(v)
        v[np.isin(rows, rows8)] *= 1.0 + 1e-3 * k
        return v

    def update(rows, cells, k):
        v = values(rows, cells, k)
        return timed(lambda: (model.update_cell_params(rows, v, cells), model.synchronize()))

    def set_domain_path(k):
        cp = D.cell_params.copy()
        cp[rows8] *= 1.0 + 1e-3 * k

        def run():
            sd, si = model.get_state()
            fx = model.get_fluxes()
            D.cell_params = cp
            model.set_domain(D)
            establish(model, sd, si, fx)
        return timed(run)

    def step_from_start(with_update):
        model.set_state(sd0, si0)
        if with_update:
            model.update_cell_params(rows8, np.ascontiguousarray(D.cell_params[np.ix_(rows8, member)]), member)
        return timed(step)

    step(); step()                                        # warm-up: code objects, the pipeline's buffers
    t_step0, t_step1 = [], []
    for _ in range(nrep + 1):                             # the first pair is a warm-up
        t_step0.append(step_from_start(False))
        t_step1.append(step_from_start(True))
    t_step0, t_step1 = t_step0[1:], t_step1[1:]
    legs = dict(dense_8=(rows8, None), dense_all=(rows_all, None), listed_8=(rows8, member), listed_all=(rows_all, member))
    t = {k: [] for k in legs}
    t_path = []
    for k, (rows, cells) in legs.items():
        update(rows, cells, 0)                            # warm-up
    set_domain_path(0)
    step()
    # the legs alternate, so that the other work on the host falls on all of them alike
    for r in range(nrep):
        for k, (rows, cells) in legs.items():
            t[k].append(update(rows, cells, r + 1))
        t_path.append(set_domain_path(r + 1))
        step()
    held = bool(np.array_equal(model.get_cell_params(), D.cell_params))
    model.close()
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), reps=nrep,
               cp_rows=int(ncp), stage_budget_mb=int(os.environ.get("VICGPU_COPY_STAGE_MB", "256")),
               update_wall_ms={k: dict(rows=int(len(legs[k][0])), cells=int(D.ncell if legs[k][1] is None else len(legs[k][1])),
                                       bytes=int(8 * len(legs[k][0]) * (D.ncell if legs[k][1] is None else len(legs[k][1]))), **spread(t[k])) for k in legs},
               set_domain_path_wall_ms=dict(does="state and fluxes out, set_domain, forcing map, state, fluxes, forcing chunk, put_data, records, groups",
                                            **spread(t_path)),
               step_ms=dict(without_update=spread(t_step0), right_behind_an_update=spread(t_step1)),
               dense_all_over_set_domain_path=round(float(np.median(t["dense_all"]) / np.median(t_path)), 5),
               table_equals_host_copy=held)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if not held:
        raise SystemExit("the device table differs from the host copy after the updates")


if __name__ == "__main__":
    main()
