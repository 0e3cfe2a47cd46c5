"""What an ensemble transform costs on the device, on a GPU, next to the only path there was before it:

    python tools/mix_cells_ab.py [--out profiles/mix_cells_ab.json] [--reps 3] [--members 16] [--columns 6250] [--merge]

The 16-member ensemble of tools/state_update_ab.py (6 250 columns, the 100 000 cells x 25 HRUs of bench.py's cfg3) on one Model,
in one process, after one step.  A dense members x members transform (every analysis member a convex combination of the
forecast members, so the state stays physical) on
    case 1   SD_SNOW_SWQ, SD_MOIST0..2
    case 2   the same four rows and the SDN_T block
followed by VICGPU_DERIVE_CAP_MOIST | VICGPU_DERIVE_NODES over all HRUs.  Timed as wall time on the host, each after a warm-up,
as medians over --reps repetitions with their spread:
    device_path   vicgpu_mix_cells, vicgpu_derive_soil_state, vicgpu_synchronize; and its legs
    host_path     vicgpu_get_state_rows, numpy (einsum over the members per column), vicgpu_update_state (SET), the same
                  derive; and its legs: what the parent commit offers
and, from the library's VICGPU_STATS line, the mix's own time on the device (the gather-multiply-add kernel and the scatter
of every pass), the bytes it must read and write, the resulting GB/s, and how far the two paths' states are apart.
--merge keeps what the output file already holds under other keys (the default-path A/B of tools/ab.sh).
Nothing is gated: the numbers are reported."""
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
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)), all=[round(float(v), 3) for v in x])


class Stderr:
    """What the library writes to file descriptor 2 inside the block (the VICGPU_STATS lines), also passed on."""

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.tmp = tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        sys.stderr.write(self.text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_cells_ab.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--columns", type=int, default=6250)
    ap.add_argument("--merge", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mix_cells_ab.py measures on a GPU: none is visible")
    os.environ["VICGPU_STATS"] = "1"
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
    # the members start apart: drier soil and more snow with the member index
    member = D.hru_iparams[C["HPI_CELL"]] // ncol
    for r in ("SD_MOIST0", "SD_MOIST1", "SD_MOIST2"):
        sd0[C[r]] *= 1.0 - 0.01 * member
    sd0[C["SD_SNOW_SWQ"]] += 0.001 * member
    four = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"]], np.int32)
    cases = {"four_rows": four, "four_rows_and_node_T": np.concatenate([four, [abi.sd_node(C["SDN_T"], n, Nn) for n in range(Nn)]]).astype(np.int32)}
    rng = np.random.default_rng(1)
    W = rng.uniform(0.1, 1.0, size=(M, M))
    W /= W.sum(axis=0, keepdims=True)
    t0 = time.perf_counter()
    lists = domain.member_transform(M, ncol, W)
    lists_ms = (time.perf_counter() - t0) * 1e3
    what = C["VICGPU_DERIVE_CAP_MOIST"] | C["VICGPU_DERIVE_NODES"]
    nrep = max(args.reps, 3)
    # member m's HRUs in the base's order: hru_of[m][k] pairs by position across the members
    hru_of = np.stack([np.concatenate([D.cell_hru_list[D.cell_hru_offset[c]:D.cell_hru_offset[c + 1]] for c in range(m * ncol, (m + 1) * ncol)]) for m in range(M)])

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

    out = dict(device=torch.cuda.get_device_name(0), members=M, columns=ncol, ncell=int(D.ncell), nhru=int(D.nhru), reps=nrep, sd_rows=int(sd0.shape[0]),
               destinations=int(len(lists[0])), terms=int(len(lists[2])), member_transform_lists_ms=round(lists_ms, 3),
               term_list_bytes=int(lists[1].nbytes + lists[2].nbytes + lists[3].nbytes), stage_budget_mb=int(os.environ.get("VICGPU_COPY_STAGE_MB", "256")), cases={})
    for name, rows in cases.items():
        def device_path(t):
            model.set_state(sd1, si1)
            with Stderr() as err:
                clock(t["mix_cells"], lambda: (model.mix_cells(rows, *lists), model.synchronize()))
            clock(t["derive_soil_state"], lambda: (model.derive_soil_state(what), model.synchronize()))
            t["total"].append(t["mix_cells"][-1] + t["derive_soil_state"][-1])
            m = re.search(r"mix_cells: .*?(\d+) passes, (\d+) bytes written: ([0-9.]+) ms", err.text)
            if m:
                t["kernels"].append(float(m.group(3)))
                t["passes"], t["written"] = int(m.group(1)), int(m.group(2))

        def host_path(t):
            model.set_state(sd1, si1)
            v = clock(t["get_state_rows"], lambda: model.get_state_rows(rows))

            def numpy_part():
                x = v[:, hru_of]                                  # [row][m'][k]
                a = np.einsum("pm,rpk->rmk", W, x)                # x_a[m] = sum over m' of W[m', m] * x_f[m']
                v[:, hru_of] = a
            clock(t["numpy"], numpy_part)
            clock(t["update_state"], lambda: (model.update_state(rows, v), model.synchronize()))
            clock(t["derive_soil_state"], lambda: (model.derive_soil_state(what), model.synchronize()))
            t["total"].append(sum(t[k][-1] for k in ("get_state_rows", "numpy", "update_state", "derive_soil_state")))

        td = {k: [] for k in ("mix_cells", "derive_soil_state", "total", "kernels")}
        th = {k: [] for k in ("get_state_rows", "numpy", "update_state", "derive_soil_state", "total")}
        for r in range(nrep + 1):                             # the first round is a warm-up; the paths alternate
            device_path(td)
            sd_dev = model.get_state()[0] if r == nrep else None
            host_path(th)
        sd_host = model.get_state()[0]
        with np.errstate(all="ignore"):
            d = np.abs(sd_dev - sd_host) / np.maximum(1e-12, np.maximum(np.abs(sd_dev), np.abs(sd_host)))
        d = np.where(np.isnan(sd_dev) & np.isnan(sd_host), 0.0, d)
        nrow = len(rows)
        # the kernel reads every source word once per destination that lists it and writes the stage; the scatter reads the
        # stage and writes the table; the indices: three words per lane and row tile, two index words and a weight per term
        read_sources = 8 * nrow * D.nhru * M
        stage_traffic = 3 * 8 * nrow * D.nhru
        must_move = 8 * nrow * D.nhru * 2                     # every listed word read once and written once
        kernel_ms = float(np.median(td["kernels"][1:])) if len(td["kernels"]) > 1 else None
        out["cases"][name] = dict(
            rows=int(nrow), passes=td.get("passes"), bytes_written=td.get("written"),
            device_path_wall_ms={k: spread(v[1:]) for k, v in td.items() if k not in ("passes", "written") and len(v) > 1},
            host_path_wall_ms={k: spread(v[1:]) for k, v in th.items()},
            device_over_host=round(float(np.median(td["total"][1:]) / np.median(th["total"][1:])), 5),
            kernels_ms=kernel_ms, bytes_source_reads=int(read_sources), bytes_stage_and_scatter=int(stage_traffic), bytes_minimum=int(must_move),
            gb_per_s_moved=None if not kernel_ms else round((read_sources + stage_traffic) / kernel_ms / 1e6, 1),
            gb_per_s_useful=None if not kernel_ms else round(must_move / kernel_ms / 1e6, 1),
            paths_apart_rel=float(np.nanmax(d)))
    model.close()
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
