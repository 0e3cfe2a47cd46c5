"""What reducing the output records over cell groups on the device (vicgpu_records_set_groups) costs and saves, on a GPU:

    python tools/record_groups_ab.py [--out profiles/record_groups_ab.json] [--reps 3] [--members 16] [--columns 6250] [--merge]

A 16-member ensemble of 6 250 columns -- the 100 000 cells x 25 HRUs of bench.py's cfg3, members as cells over shared forcing
columns (domain.tile_members) -- runs vicgpu_run_records on one Model with R = 24, alternating between three legs:
    plain    no groups: a record is [nrow][ncell]
    basins   16 x 20 contiguous basin groups with area-like weights: a record is [nrow][320]
    grid     a grid of 2 x ncell nodes, every other node a cell, fill 1e20: a record is [nrow][2 ncell] (the lane-per-group kernel)
A leg starts from the same state on the same resident forcing chunk and runs `records` records.  Reported per leg: ms_per_step of
every repetition (host clock around vicgpu_run_records ... vicgpu_records_wait(-1), over the steps), the median, the reduce
kernel's own time for one record (the library's event pair, VICGPU_STATS) and the pinned bytes of a record.
The bound: a grouped leg's median is no further above the plain leg's median than the plain leg's max - min.
--merge keeps what the output file already holds under other keys (the default-path A/B of tools/ab.sh)."""
import argparse
import ctypes
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

OUT_VARS = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP", "OUT_PREC"]      # what bench.py's writer gets
R = 24
LEGS = ("plain", "basins", "grid")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_groups_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--basins", type=int, default=20)
    ap.add_argument("--records", type=int, default=2)
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("record_groups_ab.py measures on a GPU: none is visible")
    os.environ["VICGPU_STATS"] = "1"                 # the library times the reduction of a call's last record and says so on stderr
    import bench
    from vic_amd import domain, init_state
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol, nrec = cfg["opt"], args.members, args.columns, args.records
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, sf, dmy = domain.make_forcing(base, 0, R * nrec, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    ncell = int(D.ncell)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    sf = np.ascontiguousarray(np.tile(sf, (1, 1, M)))

    # the library's stderr lines, read back at the end
    log = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    saved_err = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        model = Model(D)
        lib, h = model.lib, model.h
        model.set_forcing_map(cell_col, ncol)
        model.push_forcing(f, sf, dmy)
        ids = model.var_ids(OUT_VARS)
        nrow = model._out_rows(ids)
        # basins: member m's columns cut into `basins` contiguous runs, weights like cell areas over the basin's area
        nb = args.basins
        off = [0]
        for m in range(M):
            for b in range(nb):
                off.append(m * ncol + (b + 1) * ncol // nb)
        basins_off = np.asarray(off, dtype=np.int32)
        basins_cell = np.arange(ncell, dtype=np.int32)
        area = 0.5 + np.random.default_rng(1).random(ncell)
        basins_w = np.concatenate([area[a:b] / area[a:b].sum() for a, b in zip(basins_off[:-1], basins_off[1:])])
        # grid: node 2 c is cell c, the odd nodes hold no cell
        grid_off = np.zeros(2 * ncell + 1, dtype=np.int32)
        grid_off[1:] = (np.arange(2 * ncell) // 2) + 1
        width = dict(plain=ncell, basins=M * nb, grid=2 * ncell)
        out = model.pinned((nrec * nrow * 2 * ncell,), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)

        def leg(kind):
            model.set_state(sd0, si0)
            model.put_data_config(R)
            model.put_data_init()
            model.records_config(OUT_VARS, depth=2)
            if kind == "basins":
                model.records_set_groups(basins_off, basins_cell, basins_w, fill=0.0)
            elif kind == "grid":
                model.records_set_groups(grid_off, basins_cell, None, fill=1e20)
            assert model.records_ncol() == width[kind]
            model.synchronize()
            t0 = time.perf_counter()
            model._chk(lib.vicgpu_run_records(h, 0, nrec, out.ctypes.data_as(fp), None))
            model._chk(lib.vicgpu_records_wait(h, -1))
            return (time.perf_counter() - t0) * 1e3 / (R * nrec)

        for kind in LEGS:                            # first touch: allocations, code objects
            leg(kind)
        # the legs agree on what they deliver: basin b of member m is the weighted sum of its cells, node 2c is cell c
        leg("plain")
        plain = out[:nrec * nrow * ncell].reshape(nrec, nrow, ncell).copy()
        leg("grid")
        grid = out[:nrec * nrow * 2 * ncell].reshape(nrec, nrow, 2 * ncell)
        assert np.array_equal(grid[..., 0::2] + np.float32(0.0), plain + np.float32(0.0), equal_nan=True) and (grid[..., 1::2] == np.float32(1e20)).all()
        leg("basins")
        basins = out[:nrec * nrow * M * nb].reshape(nrec, nrow, M * nb)
        want = np.add.reduceat(plain.astype(np.float64) * basins_w, basins_off[:-1], axis=2)
        assert np.allclose(basins, want, rtol=1e-5, atol=1e-6), "the basin sums are not the weighted sums of the plain records"
        ms = {k: [] for k in LEGS}
        for _ in range(max(args.reps, 3)):
            for kind in LEGS:
                ms[kind].append(round(leg(kind), 3))
        model.close()
    finally:
        sys.stderr.flush()
        os.dup2(saved_err, 2)
        os.close(saved_err)
    log.seek(0)
    text = log.read().decode(errors="replace")
    reduce_ms = {k: [] for k in LEGS}
    for m in re.finditer(r"records reduce: (\d+) groups, .*?: ([0-9.eE+-]+) ms", text):
        for kind in ("basins", "grid"):
            if int(m.group(1)) == width[kind]:
                reduce_ms[kind].append(float(m.group(2)))
    res = {}
    for kind in LEGS:
        res[kind] = dict(ms_per_step=ms[kind], ms_per_step_median=float(np.median(ms[kind])),
                         columns_per_record=width[kind], pinned_bytes_per_record=int(nrow * width[kind] * 4))
        if kind != "plain":
            v = reduce_ms[kind][-len(ms[kind]):]
            res[kind]["reduce_kernel_ms_per_record"] = v
            res[kind]["reduce_kernel_ms_per_record_median"] = float(np.median(v)) if v else None
    spread = max(ms["plain"]) - min(ms["plain"])
    bound = dict(rule="a grouped leg's median is no further above the plain leg's median than the plain leg's max - min",
                 plain_max_minus_min=round(spread, 3))
    for kind in ("basins", "grid"):
        over = res[kind]["ms_per_step_median"] - res["plain"]["ms_per_step_median"]
        bound[kind] = dict(median_minus_plain_median=round(over, 3), met=bool(over <= spread))
    doc_leg = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=ncell, nhru=int(D.nhru), out_step_ratio=R,
                   records_per_leg=nrec, rows_per_record=nrow, basins_per_member=nb, legs=res, bound=bound)
    print(json.dumps(doc_leg), flush=True)
    doc = {}
    if args.merge and os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc["records"] = doc_leg
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
