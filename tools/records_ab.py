"""Records per second of vicgpu_run_records against the loop it replaces (vicgpu_step + vicgpu_get_outputs(reset) +
vicgpu_get_cell_errors per record), same process, same Model, alternating, on a GPU:

    python tools/records_ab.py [--out profiles/records_ab.json] [--reps 3] [--cases NAME,...]

A repetition of either path starts from the same state on the same resident forcing chunk (48 steps) and runs it `passes`
times, so both do the same work; `passes` is chosen in the warm-up so that a repetition lasts about half a second.  The
clock is the host's, around work that ends in vicgpu_records_wait(-1) resp. vicgpu_synchronize.  The loop reads into
pageable arrays as the driver sketch of INTEGRATION.md does; run_records delivers into pinned tables allocated once.
A third figure, `records_paced`, waits for the records of every call before it makes the next one (a driver that hands each
chunk's records to its writer before it goes on): with QUICK_FLUX the plain form queues all passes before the first has run.
Reported per case: the rate of every repetition, the median of each path, the run-to-run spread ((max - min) / median) and
the ratio of the medians."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

OUT_VARS = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP", "OUT_PREC"]      # what bench.py's writer gets
CHUNK = 48
# name: (bench.config shape or None for the daily water balance, cells, out_step_ratio)
CASES = {
    "cfg2_10k_R24": ("cfg2", 10000, 24),
    "cfg2_10k_R1": ("cfg2", 10000, 1),
    "cfg2_100k_R24": ("cfg2", 100000, 24),
    "cfg2_100k_R1": ("cfg2", 100000, 1),
    "wb_daily_100k_R1": (None, 100000, 1),
    "cfg3_20k_R24": ("cfg3", 20000, 24),
}


def setup(shape, ncell):
    import bench
    from vic_amd import abi, domain, init_state
    if shape:
        cfg = bench.config(shape)
        opt, ntile, doy = cfg["opt"], cfg["ntile"], cfg["start_doy"]
    else:
        opt, ntile, doy = abi.default_options(FULL_ENERGY=0, dt=24, snow_step=3), 3, 60
    d = domain.make_domain(ncell, opt, ntile=ntile)
    f, sf, dmy = domain.make_forcing(d, 0, CHUNK, start_doy=doy)
    sd0, si0 = init_state.initial_state(d, f[0])
    return d, f, sf, dmy, sd0, si0


def run_case(name, reps):
    from vic_amd.api import Model
    shape, ncell, R = CASES[name]
    d, f, sf, dmy, sd0, si0 = setup(shape, ncell)
    m = Model(d)
    lib, h = m.lib, m.h
    nrec = CHUNK // R
    ids = m.var_ids(OUT_VARS)
    nrow = m._out_rows(ids)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    loop_out, loop_err = np.zeros((nrow, ncell), np.float32), np.zeros(ncell, np.int32)
    rec_out, rec_err = m.pinned((nrec, nrow, ncell), np.float32), m.pinned((nrec, ncell), np.int32)
    m.push_forcing(f, sf, dmy)

    def start():
        m.set_state(sd0, si0)
        m.put_data_config(R)
        m.put_data_init()
        m.records_config(OUT_VARS, depth=2)
        m.synchronize()

    def loop(passes):
        t0 = time.perf_counter()
        for _ in range(passes):
            for k in range(nrec):
                m._chk(lib.vicgpu_step(h, k * R, R))
                m._chk(lib.vicgpu_get_outputs(h, len(ids), ids.ctypes.data_as(ip), loop_out.ctypes.data_as(fp), 1))
                m._chk(lib.vicgpu_get_cell_errors(h, loop_err.ctypes.data_as(ip)))
        m._chk(lib.vicgpu_synchronize(h))
        return time.perf_counter() - t0

    def records(passes, paced=False):
        t0 = time.perf_counter()
        for _ in range(passes):
            m._chk(lib.vicgpu_run_records(h, 0, nrec, rec_out.ctypes.data_as(fp), rec_err.ctypes.data_as(ip)))
            if paced:
                m._chk(lib.vicgpu_records_wait(h, -1))
        m._chk(lib.vicgpu_records_wait(h, -1))
        return time.perf_counter() - t0

    # warm-up chunk: both paths once, which also sizes the repetitions and checks that they agree on the last record
    start(); t_loop = loop(1); want = loop_out.copy()
    start(); t_rec = records(1)
    assert np.array_equal(want, rec_out[-1], equal_nan=True), "the two paths disagree"
    passes = int(min(max(round(0.5 / max(min(t_loop, t_rec), 1e-6)), 1), 200))
    rate = {"loop": [], "records": [], "records_paced": []}
    for _ in range(reps):
        start(); rate["loop"].append(passes * nrec / loop(passes))
        start(); rate["records"].append(passes * nrec / records(passes))
        start(); rate["records_paced"].append(passes * nrec / records(passes, paced=True))
    m.close()
    res = dict(case=name, ncell=ncell, nhru=int(d.nhru), out_step_ratio=R, records_per_pass=nrec, passes=passes, rows_per_record=nrow)
    for k, v in rate.items():
        med = float(np.median(v))
        res[k] = dict(records_per_s=[round(x, 2) for x in v], median=round(med, 2), spread=round((max(v) - min(v)) / med, 4))
    res["records_over_loop"] = round(res["records"]["median"] / res["loop"]["median"], 4)
    res["records_paced_over_loop"] = round(res["records_paced"]["median"] / res["loop"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("records_ab.py measures on a GPU: none is visible")
    results = []
    for name in args.cases.split(","):
        r = run_case(name, max(args.reps, 3))
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(args.out, "w") as fh:      # after every case: a run that is cut short keeps what it measured
            json.dump(dict(device=torch.cuda.get_device_name(0), unit="output records per second, host clock", cases=results), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
