"""What vicgpu_copy_cells costs an ensemble, on a GPU, next to the host round trip it replaces:

    python tools/copy_cells_ab.py [--out profiles/copy_cells_ab.json] [--reps 5] [--members 16] [--columns 6250]

The 16-member ensemble of tools/forcing_map_ab.py (6 250 columns, the 100 000 cells x 25 HRUs of bench.py's cfg3) on one Model,
in one process.  Timed, each after a warm-up call, as medians over --reps repetitions with their spread (max - min):
    (a) the fan-out 0 -> 1 .. 15 (direct path)
    (b) a rotation of all members (staged path, the stage budget in force)
    (c) the host round trip that does (b): get_state + get_fluxes -> numpy.take -> set_state + set_fluxes
    (d) a plain device-to-device copy (torch Tensor.copy_) of as many bytes as (a) writes: the card's copy rate that day
(a) and (b) are wall times of the call plus vicgpu_synchronize -- host planning, the upload of the pair lists, the kernels -- and,
from a second Model under VICGPU_STATS, the kernels' own time between two device events (the line the library prints).  Rates
are bytes written into the tables over time; a copy reads as many bytes as it writes, the staged path moves them twice."""
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


def spread(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)), all=[round(float(v), 4) for v in x])


def capture_stderr(fn):
    """fn() with the process's stderr (the library prints there) sent to a file; its text."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_cells_ab.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("copy_cells_ab.py measures on a GPU: none is visible")
    import bench
    from vic_amd import abi, domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol = cfg["opt"], args.members, args.columns
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, _, _ = domain.make_forcing(base, 0, 1, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    member = D.hru_iparams[C["HPI_CELL"]] // ncol
    sd0[C["SD_MOIST0"]] *= 1.0 - 0.01 * member          # every member its own state
    j = np.arange(ncol, dtype=np.int32)
    fan = (np.concatenate([m * ncol + j for m in range(1, M)]), np.concatenate([j for _ in range(1, M)]))
    rot = (np.concatenate([((m + 1) % M) * ncol + j for m in range(M)]), np.concatenate([m * ncol + j for m in range(M)]))
    hpm = base.nhru
    lst = D.cell_hru_list.reshape(M, hpm)
    perm = np.arange(D.nhru)
    for m in range(M):
        perm[lst[(m + 1) % M]] = lst[m]                  # column h takes column perm[h]
    rows = abi.sd_nrow(opt.Nnode) * 8 + abi.si_nrow(opt.Nnode) * 4 + C["FX_NROW"] * 8          # bytes of an HRU's state columns
    bytes_fan, bytes_rot = rows * hpm * (M - 1), rows * hpm * M
    nrep = max(args.reps, 3)

    def timed(fn):
        model.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def device(pairs):
        model.copy_cells(*pairs)
        model.synchronize()

    def host():
        sd, si = model.get_state()
        fx = model.get_fluxes()
        model.set_state(np.take(sd, perm, axis=1), np.take(si, perm, axis=1))
        model.set_fluxes(np.take(fx, perm, axis=1))
        model.synchronize()

    model = Model(D)
    model.set_state(sd0, si0)
    stage_mb = int(os.environ.get("VICGPU_COPY_STAGE_MB", "256"))
    # the three legs alternate, so that the other work on the host falls on all of them alike
    t_fan, t_rot, t_host = [], [], []
    device(fan); device(rot); host()                 # warm-up: code objects, allocations, page faults of fresh host arrays
    for _ in range(nrep):
        t_fan.append(timed(lambda: device(fan)))
        t_rot.append(timed(lambda: device(rot)))
        t_host.append(timed(host))
    # results: the rotation on the device against numpy.take on the host, from the same state
    model.set_state(sd0, si0)
    device(rot)
    sd_dev, si_dev = model.get_state()
    same = bool(np.array_equal(sd_dev, np.take(sd0, perm, axis=1), equal_nan=True) and np.array_equal(si_dev, np.take(si0, perm, axis=1)))
    del sd_dev, si_dev
    model.close()

    # the kernels' own time: a second model that prints it (VICGPU_STATS is read when the domain is set)
    os.environ["VICGPU_STATS"] = "1"
    model = Model(D)
    os.environ.pop("VICGPU_STATS")
    model.set_state(sd0, si0)
    device(fan); device(rot)
    text = capture_stderr(lambda: [device(fan) for _ in range(nrep)] + [device(rot) for _ in range(nrep)])
    model.close()
    k_fan = [float(x) for x in re.findall(r"copy_cells: .* direct, .*: ([0-9.]+) ms on the device", text)]
    k_rot = [float(x) for x in re.findall(r"copy_cells: .* staged, .*: ([0-9.]+) ms on the device", text)]
    assert len(k_fan) == nrep and len(k_rot) == nrep, text

    # the yardstick: a device-to-device copy of as many bytes as the fan-out writes
    a = torch.empty(bytes_fan, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a); torch.cuda.synchronize()
    t_plain = []
    for _ in range(nrep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        t_plain.append(e0.elapsed_time(e1))
    gbs = lambda nbytes, ms: round(nbytes / (np.median(ms) * 1e-3) / 1e9, 1)
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), reps=nrep,
               bytes_per_hru_column=int(rows), stage_budget_mb=stage_mb,
               fanout=dict(path="direct", bytes_written=int(bytes_fan), wall_ms=spread(t_fan), kernel_ms=spread(k_fan),
                           wall_gb_per_s=gbs(bytes_fan, t_fan), kernel_gb_per_s=gbs(bytes_fan, k_fan)),
               rotation=dict(path="staged", bytes_written=int(bytes_rot), wall_ms=spread(t_rot), kernel_ms=spread(k_rot),
                             wall_gb_per_s=gbs(bytes_rot, t_rot), kernel_gb_per_s=gbs(bytes_rot, k_rot)),
               host_round_trip=dict(does="the rotation", bytes_written=int(bytes_rot), wall_ms=spread(t_host), wall_gb_per_s=gbs(bytes_rot, t_host)),
               plain_device_copy=dict(bytes_written=int(bytes_fan), kernel_ms=spread(t_plain), gb_per_s=gbs(bytes_fan, t_plain)),
               rotation_over_host_round_trip=round(float(np.median(t_rot) / np.median(t_host)), 5),
               rotation_equals_numpy_take=same)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if not same:
        raise SystemExit("the rotation on the device differs from numpy.take on the host")


if __name__ == "__main__":
    main()
