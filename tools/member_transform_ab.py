"""What the analysis of a localised ensemble filter costs with the transform solved and applied on the device, on a GPU, next
to the only path there was before it:

    python tools/member_transform_ab.py [--out profiles/member_transform_ab.json] [--reps 3] [--members 16] [--columns 6250] [--obs 8]

The 16-member ensemble of tools/mix_cells_ab.py (6 250 columns, the 100 000 cells x 25 HRUs of bench.py's cfg3) on one Model, in
one process, after one step; every base column its own transform from --obs observations (the members' snow water equivalent
and top-layer moisture of the column, perturbed), on SD_SNOW_SWQ and SD_MOIST0..2.  Timed as wall time on the host, each after a
warm-up, as medians over --reps repetitions with their spread:
    device_path   vicgpu_member_transform_solve, vicgpu_member_transform_apply, vicgpu_synchronize
    host_path     the same formulas in numpy (batched eigh over the columns), domain.member_transform (the term lists),
                  vicgpu_mix_cells: what the parent commit offers; its three legs apart
and, from the library's VICGPU_STATS lines, the solve kernel's and the apply's own time on the device, the bytes each path
uploads, how far the two transforms are apart and whether the two states agree bit for bit when both paths apply the device's T.
Nothing is gated: the numbers are reported."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mix_cells_ab import Stderr, spread


def host_transform(M, hx, yobs, rinv, rho):
    """The formulas of include/vicgpu.h for hx [ncol][nobs][M], yobs and rinv [ncol][nobs], rho [ncol]: T [ncol][M][M]."""
    ybar = hx.sum(axis=2) / M
    Y = hx - ybar[:, :, None]
    d = yobs - ybar
    RY = rinv[:, :, None] * Y
    A = np.einsum("jpa,jpb->jab", RY, Y) + ((M - 1) / rho)[:, None, None] * np.eye(M)
    g = np.einsum("jpa,jp->ja", RY, d)
    lam, U = np.linalg.eigh(A)
    wbar = np.einsum("jai,ji->ja", U, np.einsum("jai,ja->ji", U, g) / lam)
    Wa = (U * np.sqrt((M - 1) / lam)[:, None, :]) @ U.transpose(0, 2, 1)
    W = Wa + wbar[:, :, None]
    return W + ((1.0 - W.sum(axis=1)) / M)[:, None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_transform_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--obs", type=int, default=8)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("member_transform_ab.py measures on a GPU: none is visible")
    os.environ["VICGPU_STATS"] = "1"
    import bench
    from vic_amd import domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model

    cfg = bench.config("cfg3")
    opt, M, ncol, nobs = cfg["opt"], args.members, args.columns, args.obs
    base = domain.make_domain(ncol, opt, ntile=cfg["ntile"])
    f, _, dmy = domain.make_forcing(base, 0, 2, start_doy=cfg["start_doy"])
    D, cell_col = domain.tile_members(base, M)
    sf = domain.make_snowflag(D, f, cell_col)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(np.tile(f[0], (1, 1, M))))
    member = D.hru_iparams[C["HPI_CELL"]] // ncol
    for r in ("SD_MOIST0", "SD_MOIST1", "SD_MOIST2"):
        sd0[C[r]] *= 1.0 - 0.01 * member
    sd0[C["SD_SNOW_SWQ"]] += 0.001 * member
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"]], np.int32)
    nrep = max(args.reps, 3)

    model = Model(D)
    model.set_forcing_map(cell_col, ncol)
    model.set_state(sd0, si0)
    model.push_forcing(f, sf, dmy)
    model.dist_prec(0, 1)
    sd1, si1 = model.get_state()
    # H x: the cell sums of the top-layer moisture and of the snow water equivalent, alternating, each with noise of its own
    rng = np.random.default_rng(2)
    cell = D.hru_iparams[C["HPI_CELL"]]
    two = np.stack([np.bincount(cell, weights=sd1[C[r]], minlength=D.ncell).reshape(M, ncol).T for r in ("SD_MOIST0", "SD_SNOW_SWQ")])       # [2][ncol][M]
    hx = np.ascontiguousarray(np.stack([two[p % 2] * (1.0 + 0.02 * rng.normal(size=(ncol, M))) for p in range(nobs)], axis=1))              # [ncol][nobs][M]
    yobs = hx.mean(axis=2) * (1.0 + 0.05 * rng.normal(size=(ncol, nobs)))
    rinv = rng.uniform(0.2, 1.0, size=(ncol, nobs)) / np.maximum(hx.var(axis=2), 1e-12)
    rho = np.full(ncol, 1.05)
    off = (np.arange(ncol + 1) * nobs).astype(np.int32)
    flat = (off, hx.reshape(-1, M), yobs.reshape(-1), rinv.reshape(-1), rho)

    def clock(legs, fn):
        model.synchronize()
        t0 = time.perf_counter()
        r = fn()
        legs.append((time.perf_counter() - t0) * 1e3)
        return r

    td = {k: [] for k in ("solve", "apply", "total", "solve_kernel", "apply_kernels")}
    th = {k: [] for k in ("numpy_transform", "member_transform_lists", "mix_cells", "total", "mix_kernels")}
    keep = {}
    for r in range(nrep + 1):                                 # the first round is a warm-up; the paths alternate
        model.set_state(sd1, si1)
        with Stderr() as err:
            keep["info"] = clock(td["solve"], lambda: model.member_transform_solve(M, *flat))
            clock(td["apply"], lambda: (model.member_transform_apply(rows), model.synchronize()))
        td["total"].append(td["solve"][-1] + td["apply"][-1])
        m = re.search(r"member_transform_solve: .*?: ([0-9.]+) ms", err.text)
        if m:
            td["solve_kernel"].append(float(m.group(1)))
        m = re.search(r"member_transform_apply: .*?(\d+) passes, (\d+) bytes written: ([0-9.]+) ms", err.text)
        if m:
            td["apply_kernels"].append(float(m.group(3)))
        if r == nrep:
            keep["T_dev"], keep["sd_dev"] = model.member_transform_get(), model.get_state()[0]
        model.set_state(sd1, si1)
        T = clock(th["numpy_transform"], lambda: host_transform(M, hx, yobs, rinv, rho))
        lists = clock(th["member_transform_lists"], lambda: domain.member_transform(M, ncol, T))
        with Stderr() as err:
            clock(th["mix_cells"], lambda: (model.mix_cells(rows, *lists), model.synchronize()))
        th["total"].append(sum(th[k][-1] for k in ("numpy_transform", "member_transform_lists", "mix_cells")))
        m = re.search(r"mix_cells: .*?(\d+) passes, (\d+) bytes written: ([0-9.]+) ms", err.text)
        if m:
            th["mix_kernels"].append(float(m.group(3)))
        if r == nrep:
            keep["T_host"], keep["sd_host"], keep["lists"] = T, model.get_state()[0], lists
    # both paths with the device's transform: the states must agree bit for bit
    model.set_state(sd1, si1)
    model.mix_cells(rows, *domain.member_transform(M, ncol, keep["T_dev"]))
    twin = model.get_state()[0]
    model.close()
    a, b = keep["sd_dev"][rows], twin[rows]
    nan = np.isnan(a) & np.isnan(b)
    bitwise = bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]))
    with np.errstate(all="ignore"):
        d = np.abs(keep["sd_dev"][rows] - keep["sd_host"][rows]) / np.maximum(1e-12, np.abs(keep["sd_host"][rows]))
    info, lists = keep["info"], keep["lists"]
    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, observations_per_column=nobs, ncell=int(D.ncell), nhru=int(D.nhru), rows=int(len(rows)),
               reps=nrep, sweeps=dict(min=int(info.min()), max=int(info.max()), mean=round(float(info.mean()), 2), not_converged=int((info < 0).sum())),
               device_path_wall_ms={k: spread(v[1:]) for k, v in td.items() if len(v) > 1},
               host_path_wall_ms={k: spread(v[1:]) for k, v in th.items() if len(v) > 1},
               device_over_host=round(float(np.median(td["total"][1:]) / np.median(th["total"][1:])), 5),
               bytes_uploaded_device_path=int(sum(x.nbytes for x in flat) + rows.nbytes),
               bytes_uploaded_host_path=int(sum(x.nbytes for x in lists) + rows.nbytes), weight_array_bytes=int(keep["T_dev"].nbytes),
               transforms_apart_abs=float(np.abs(keep["T_dev"] - keep["T_host"]).max()), states_apart_rel=float(np.nanmax(d)),
               apply_equals_mix_cells_bitwise=bitwise)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
