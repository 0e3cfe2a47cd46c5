"""Output records reduced over cell groups (vicgpu_records_set_groups, include/vicgpu_out.h) against the contract the header
states, restated here in numpy.  Run by tests/test_record_groups.py with VICGPU_LIB pointing at the unsanitized host build
(SAN=none tools/hostemu/build.sh); tests/test_record_groups_gpu.py imports run() and the group builders for the GPU.
    python tools/hostemu/check_record_groups.py run <case> [<case> ...]
        one Model runs vicgpu_run_records with groups set, a second one from the same state runs the plain vicgpu_run_records;
        the plain float records go through contract() and the grouped output must equal that bit for bit.  cell_err records,
        state, fluxes, balance, accumulators and cell outputs equal the plain run's and the aggregates are zero; a second call
        follows the first; with the groups removed again a third call delivers the plain [nrow][ncell] records.  Before that,
        the inputs are checked: a left-to-right sum of the same terms must differ from the contract's order in the float
        result of at least one element, or the case would prove nothing about the order.
    python tools/hostemu/check_record_groups.py errors
        every error and lifetime return the header lists, the refusal of a group shard included
    python tools/hostemu/check_record_groups.py refusals
        vicgpu_records_set_groups under a runtime that refuses its n-th allocation, for every n: VICGPU_ERR_HIP, nothing left
        behind and the groups in force kept"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, VicGpuError, load_library

# out of table order, every aggregation type and element kind (as tools/hostemu/check_records.py)
OUT = ["OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SURF_TEMP", "OUT_SOIL_MOIST", "OUT_AERO_RESIST", "OUT_SWE"]
BIG = 1.0e12 / 3.0           # the weight of a cancelling pair: what is left of the small terms shows the order in the float result


# ------------------------------------------------------------------------------------------------ the contract, in numpy
def _terms(v, cells, weights):
    """t_i = w_i * (double)v[..][cell_i]: float64 products, one rounding each; v is float32 [..][ncell]."""
    return [np.float64(w) * v[..., int(c)].astype(np.float64) for c, w in zip(cells, weights)]


def _contract_sum(t):
    """The order of the header: lane l of 64 is assigned t_l and adds t_{l+64}, t_{l+128}, ...; a lane without a member holds
    +0.0; then p_l = p_l + p_{l+s} for l < s, s = 32 .. 1; the value is p_0.  Explicit loops; every + is one float64 addition
    (elementwise over the leading axes, which are independent records and rows)."""
    zero = np.zeros_like(t[0])
    p = []
    for l in range(64):
        if l < len(t):
            acc = t[l]
            for i in range(l + 64, len(t), 64):
                acc = acc + t[i]
            p.append(acc)
        else:
            p.append(zero)
    s = 32
    while s >= 1:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s //= 2
    return p[0]


def _left_to_right_sum(t):
    acc = t[0]
    for x in t[1:]:
        acc = acc + x
    return acc


def reduce_records(v, off, cells, weights, fill, order=_contract_sum):
    """float32 [..][ncell] -> float32 [..][ngroup]"""
    ng = len(off) - 1
    w = np.ones(len(cells)) if weights is None else weights
    out = np.empty(v.shape[:-1] + (ng,), dtype=np.float32)
    for g in range(ng):
        a, b = int(off[g]), int(off[g + 1])
        if a == b:
            out[..., g] = np.float32(fill)
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                out[..., g] = order(_terms(v, cells[a:b], w[a:b])).astype(np.float32)
    return out


def contract(v, off, cells, weights, fill):
    return reduce_records(v, off, cells, weights, fill, _contract_sum)


def same_bits(a, b):
    """uint32 views equal, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ groups
def pack(groups):
    """[(cells, weights)] -> (offsets, cells, weights)"""
    off = np.zeros(len(groups) + 1, dtype=np.int32)
    for g, (c, _) in enumerate(groups):
        off[g + 1] = off[g] + len(c)
    cells = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in groups]) if off[-1] else np.zeros(0, np.int32)
    w = np.concatenate([np.asarray(x, dtype=np.float64) for _, x in groups]) if off[-1] else np.zeros(0)
    return off, cells, w


def _weights(n, rng):
    return rng.choice([1.0 / 3.0, 0.1, 0.7, 1.0 / 7.0], size=n)


def mixed_groups(ncell, sizes, seed=5):
    """Groups over `ncell` cells with non-dyadic weights: one of each size in `sizes` (the first in scrambled order over all the
    cells when it is ncell), an empty one, two that share cells, and one in which a cell repeats: a cancelling pair
    (+BIG, -BIG on one cell) in front of more than 64 small terms, so that the order of the additions shows in the float."""
    rng = np.random.default_rng(seed)
    groups = []
    for n in sizes:
        c = rng.permutation(ncell)[:n]
        groups.append((c, _weights(n, rng)))
    groups.append((np.zeros(0, np.int32), np.zeros(0)))
    a = rng.permutation(ncell)[:min(40, ncell)]
    groups.append((a, _weights(len(a), rng)))
    b = np.concatenate([a[len(a) // 2:], rng.permutation(ncell)[:7]])          # shares half of a's cells
    groups.append((b[rng.permutation(len(b))], _weights(len(b), rng)))
    rest = rng.integers(0, ncell, size=min(68, 2 * ncell))
    c0 = int(rest[0])
    groups.append((np.concatenate([[c0, c0], rest]), np.concatenate([[BIG, -BIG], _weights(len(rest), rng)])))
    return pack(groups)


def grid_groups(ncell, nnode, seed=9):
    """The writer's grid: nnode nodes, the cells scattered over them, one member of weight 1 (no weights passed) or none."""
    rng = np.random.default_rng(seed)
    node = np.sort(rng.permutation(nnode)[:ncell])
    off = np.zeros(nnode + 1, dtype=np.int32)
    has = np.zeros(nnode, dtype=np.int32)
    has[node] = 1
    off[1:] = np.cumsum(has)
    return off, np.arange(ncell, dtype=np.int32), None


def span_groups(ncell, lo, hi):
    """All cells, the cells [lo, hi) (across a chunk boundary), and a cancelling pair in front of every cell."""
    rng = np.random.default_rng(3)
    allc = np.arange(ncell)
    groups = [(allc, _weights(ncell, rng)), (np.arange(lo, hi), _weights(hi - lo, rng)),
              (np.concatenate([[lo, lo], allc]), np.concatenate([[BIG, -BIG], _weights(ncell, rng)]))]
    return pack(groups)


# name: options, cells, tiles, start day, R, records, depths, steps before the first record, VICGPU_CHUNKS values, groups, fill
CASES = {
    "quickflux": (dict(FULL_ENERGY=1, Nband=3), 130, 2, 80, 3, 4, (1, 2), 1, (None,), lambda n: mixed_groups(n, (130, 65, 64, 1)), -9.0),
    "grid": (dict(FULL_ENERGY=1, Nband=3), 130, 2, 80, 3, 2, (2,), 0, (None,), lambda n: grid_groups(n, 150), 1e20),
    "frozen_chunks": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 330, 2, 3, (1, 2), 0, ("2",),
                      lambda n: span_groups(n, 1, 4), 0.5),
}


def _tables(m):
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["balance"] = m.get_balance()
    r["accum"] = m.get_accum()
    r["cell_out"] = m.get_cell_outputs()
    r["agg_after"] = m.get_output_data(OUT, aggregated=True)
    return r


def _start(d, f, sf, dmy, sd0, si0, R, pre, depth):
    m = Model(d)
    m.set_state(sd0, si0)
    m.put_data_config(R)
    m.put_data_init()
    m.push_forcing(f, sf, dmy)
    if pre:
        m.dist_prec(0, pre)          # record 0 includes what the aggregates held
    m.records_config(OUT, depth=depth)
    return m


def _records(m, f, sf, dmy, pre, nrec, push):
    if push:
        m.push_forcing(f, sf, dmy)
    rec = m.run_records(pre, nrec, errors=True)
    rec.wait(0)
    rec.wait()
    out, err = rec.out.copy(), rec.errors.copy()
    del rec
    return out, err


def run(name, spec, log=print):
    """Problems of one case (an empty list: none).  Results must not depend on depth or on the cell chunks."""
    kw, ncell, ntile, doy, R, nrec, depths, pre, chunk_list, make_groups, fill = spec
    opt = abi.default_options(**kw)
    d = domain.make_domain(ncell, opt, ntile=ntile)
    nsteps = pre + R * nrec
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=doy)
    sd0, si0 = init_state.initial_state(d, f[0])
    off, cells, w = make_groups(ncell)
    ng, nnz = len(off) - 1, int(off[-1])
    bad = []
    os.environ.pop("VICGPU_CHUNKS", None)
    # the plain run: three calls (the records, one more record of a fresh chunk, and one more again)
    if chunk_list[0]:
        os.environ["VICGPU_CHUNKS"] = chunk_list[0]
    a = _start(d, f, sf, dmy, sd0, si0, R, pre, 2)
    plain1, err1 = _records(a, f, sf, dmy, pre, nrec, False)
    want = _tables(a)
    plain2, err2 = _records(a, f, sf, dmy, pre, 1, True)
    plain3, err3 = _records(a, f, sf, dmy, pre, 1, True)
    a.close()
    if not (np.isfinite(plain1).all() and plain1.any()):
        bad.append("the plain records are not finite or all zero")
    want1, want2 = contract(plain1, off, cells, w, fill), contract(plain2, off, cells, w, fill)
    # the inputs must tell the contract's order from a left-to-right sum
    multi = bool((np.diff(off) > 1).any())
    if multi:
        ltr = reduce_records(plain1, off, cells, w, fill, _left_to_right_sum)
        differ = int(np.sum(ltr.view(np.uint32) != want1.view(np.uint32)))
        log("record groups %s: a left-to-right sum differs from the contract's order in %d of %d elements" % (name, differ, want1.size), flush=True)
        if differ == 0:
            return ["the inputs do not tell the summation orders apart"]
    first = None
    for chunks in chunk_list:
        for depth in depths:
            if chunks:
                os.environ["VICGPU_CHUNKS"] = chunks
            b = _start(d, f, sf, dmy, sd0, si0, R, pre, depth)
            b.records_set_groups(off, cells, w, fill)
            shape_ok = b.records_get_groups() == (ng, nnz) and b.records_ncol() == ng
            got1, gerr1 = _records(b, f, sf, dmy, pre, nrec, False)
            got = _tables(b)
            got2, gerr2 = _records(b, f, sf, dmy, pre, 1, True)
            b.records_set_groups(None, None)
            removed = b.records_get_groups() == (0, 0) and b.records_ncol() == ncell
            got3, gerr3 = _records(b, f, sf, dmy, pre, 1, True)
            b.close()
            diff = [k for k in want if not np.array_equal(want[k], got[k], equal_nan=True)]
            if not same_bits(got1, want1):
                diff.append("grouped records (%d elements)" % int(np.sum(got1.view(np.uint32) != want1.view(np.uint32))))
            if not same_bits(got2, want2):
                diff.append("grouped records of the second call")
            if not same_bits(got3, plain3):
                diff.append("plain records after the groups were removed")
            if not (np.array_equal(gerr1, err1) and np.array_equal(gerr2, err2) and np.array_equal(gerr3, err3)):
                diff.append("cell_err records")
            if got["agg_after"].any():
                diff.append("aggregates not zero")
            if not shape_ok or not removed:
                diff.append("records_get_groups / records_ncol")
            if first is None:
                first = got1
            elif not same_bits(first, got1):
                diff.append("results depend on depth or chunks")
            log("record groups %s chunks %s depth %d: %d records of %d rows x %d groups (%d members) from %d cells, differing: %s"
                % (name, chunks or "default", depth, nrec, want1.shape[1], ng, nnz, ncell, diff or "none"), flush=True)
            bad += ["%s chunks %s depth %d: %s" % (name, chunks, depth, x) for x in diff]
    os.environ.pop("VICGPU_CHUNKS", None)
    return bad


# ------------------------------------------------------------------------------------------------ error and lifetime returns
def errors():
    lib = load_library()
    ARG, STATE, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    fp, ip, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    checks = []

    def want(what, got, code):
        checks.append((what, got, code))

    i32 = lambda x: np.asarray(x, dtype=np.int32)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    ng, nz = ctypes.c_int(-1), ctypes.c_int(-1)

    def setg(h, off, cell, w=None, fill=0.0):
        n = len(off) - 1 if off is not None else 0
        return lib.vicgpu_records_set_groups(h, n, off.ctypes.data_as(ip) if off is not None else None,
                                             cell.ctypes.data_as(ip) if cell is not None else None,
                                             w.ctypes.data_as(dp) if w is not None else None, fill)

    def getg(h):
        rc = lib.vicgpu_records_get_groups(h, ctypes.byref(ng), ctypes.byref(nz))
        return rc if rc else (ng.value, nz.value)

    off, cell = i32([0, 2, 2, 3]), i32([0, 6, 3])
    want("set_groups(NULL)", setg(None, off, cell), ARG)
    want("get_groups(NULL)", lib.vicgpu_records_get_groups(None, ctypes.byref(ng), ctypes.byref(nz)), ARG)
    want("records_ncol(NULL)", lib.vicgpu_records_ncol(None), ARG)

    os.environ.pop("VICGPU_CHUNKS", None)
    opt = abi.default_options(FULL_ENERGY=1, Nband=3)
    d = domain.make_domain(7, opt, ntile=2)
    R, nrec = 2, 2
    f, sf, dmy = domain.make_forcing(d, 0, R * nrec, start_doy=80)
    sd0, si0 = init_state.initial_state(d, f[0])
    m = Model(d)
    m.set_state(sd0, si0)
    ids = m.var_ids(OUT)
    nrow = m._out_rows(ids)
    cfg = lambda depth: lib.vicgpu_records_config(m.h, len(ids), ids.ctypes.data_as(ip), depth)
    want("set_groups before put_data_config", setg(m.h, off, cell), STATE)
    m.put_data_config(R)
    m.put_data_init()
    want("set_groups before records_config", setg(m.h, off, cell), STATE)
    want("get_groups before records_config", getg(m.h), STATE)
    want("records_ncol before records_config", lib.vicgpu_records_ncol(m.h), STATE)
    want("records_config", cfg(2), OK)
    want("get_groups when none is set", getg(m.h), (0, 0))
    want("records_ncol without groups", lib.vicgpu_records_ncol(m.h), d.ncell)
    want("get_groups with a null result", lib.vicgpu_records_get_groups(m.h, None, ctypes.byref(nz)), ARG)
    want("ngroup < 0", lib.vicgpu_records_set_groups(m.h, -1, None, None, None, 0.0), ARG)
    want("offsets NULL", lib.vicgpu_records_set_groups(m.h, 3, None, cell.ctypes.data_as(ip), None, 0.0), ARG)
    want("cells NULL", lib.vicgpu_records_set_groups(m.h, 3, off.ctypes.data_as(ip), None, None, 0.0), ARG)
    want("group_off[0] != 0", setg(m.h, i32([1, 2, 2, 3]), cell), ARG)
    want("decreasing offsets", setg(m.h, i32([0, 2, 1, 3]), cell), ARG)
    want("cell == ncell", setg(m.h, off, i32([0, 7, 3])), ARG)
    want("negative cell", setg(m.h, off, i32([0, -1, 3])), ARG)
    want("NaN weight", setg(m.h, off, cell, f64([1, np.nan, 1])), ARG)
    want("infinite weight", setg(m.h, off, cell, f64([1, 1, np.inf])), ARG)
    want("get_groups after refused calls", getg(m.h), (0, 0))
    want("set_groups", setg(m.h, off, cell, f64([0.5, 0.25, 2.0]), -1.0), OK)
    want("get_groups", getg(m.h), (3, 3))
    want("records_ncol with groups", lib.vicgpu_records_ncol(m.h), 3)
    want("a refused call keeps the groups in force", (setg(m.h, off, i32([0, 7, 3])), getg(m.h)), (ARG, (3, 3)))
    # a grouped run, then every way the groups go
    m.push_forcing(f, sf, dmy)
    out = m.pinned((nrec, nrow, 3), np.float32)
    err = m.pinned((nrec, d.ncell), np.int32)
    run = lambda: lib.vicgpu_run_records(m.h, 0, nrec, out.ctypes.data_as(fp), err.ctypes.data_as(ip))
    want("run_records with groups", run(), OK)
    want("records_wait(-1)", lib.vicgpu_records_wait(m.h, -1), OK)
    want("all-empty groups", setg(m.h, i32([0, 0, 0]), i32([]), None, -3.0), OK)
    want("records_wait after set_groups", lib.vicgpu_records_wait(m.h, -1), STATE)
    want("get_groups of empty groups", getg(m.h), (2, 0))
    want("run_records with empty groups", run(), OK)
    want("records_wait(0)", lib.vicgpu_records_wait(m.h, 0), OK)
    want("synchronize", lib.vicgpu_synchronize(m.h), OK)
    want("empty groups hold the fill value", bool((out.ravel()[:nrec * nrow * 2] == -3.0).all()), True)
    want("ngroup 0 removes", lib.vicgpu_records_set_groups(m.h, 0, None, None, None, 0.0), OK)
    want("get_groups after removal", getg(m.h), (0, 0))
    want("set_groups again", setg(m.h, off, cell), OK)
    want("records_config drops the groups", (cfg(1), getg(m.h)), (OK, (0, 0)))
    want("set_groups again (2)", setg(m.h, off, cell), OK)
    want("nvar 0 drops the groups", (lib.vicgpu_records_config(m.h, 0, None, 0), getg(m.h), setg(m.h, off, cell)), (OK, STATE, STATE))
    want("records_config (3)", (cfg(2), setg(m.h, off, cell), getg(m.h)), (OK, OK, (3, 3)))
    m.put_data_config(R)
    want("put_data_config drops the groups", (getg(m.h), lib.vicgpu_records_ncol(m.h)), (STATE, STATE))
    want("records_config (4)", (cfg(2), getg(m.h), setg(m.h, off, cell)), (OK, (0, 0), OK))
    m.set_domain(d)
    want("set_domain drops the groups", getg(m.h), STATE)
    m.close()

    # a context with groups set, driven as a shard of a device group
    g = Group(d, devices=[0, 0])
    g.set_state(sd0, si0)
    g.put_data_config(R)
    g.put_data_init()
    g.push_forcing(f, sf, dmy)
    g.records_config(OUT, depth=2)
    ctx = g.shard_ctx(1)
    want("set_groups on a shard's context", setg(ctx, i32([0, 1]), i32([0])), OK)
    gout, gerr = g.pinned((nrec, nrow, d.ncell), np.float32), g.pinned((nrec, d.ncell), np.int32)
    grun = lambda: lib.vicgpu_group_run_records(g.h, 0, nrec, gout.ctypes.data_as(fp), gerr.ctypes.data_as(ip))
    want("group_run_records with a grouped shard", grun(), STATE)
    want("groups removed from the shard", lib.vicgpu_records_set_groups(ctx, 0, None, None, None, 0.0), OK)
    want("group_run_records again", (grun(), lib.vicgpu_group_records_wait(g.h, -1)), (OK, OK))
    try:
        g.records_set_groups(off, cell)
        want("Group.records_set_groups raises", False, True)
    except VicGpuError:
        want("Group.records_set_groups raises", True, True)
    g.close()
    failed = [(w, g_, c) for w, g_, c in checks if g_ != c]
    for w, g_, c in failed:
        print("record groups return: %s gave %s, want %s" % (w, g_, c), flush=True)
    print("record groups errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return 1 if failed else 0


def refusals():
    """vicgpu_records_set_groups with the n-th allocation refused, n = 1, 2, ...: VICGPU_ERR_HIP, the count of live runtime
    objects where it was and the groups in force as they were, until the call gets through."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    live0 = lib.hostemu_live_objects()
    os.environ["VICGPU_CHUNKS"] = "2"
    opt = abi.default_options(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0)
    d = domain.make_domain(5, opt, ntile=2)
    f, sf, dmy = domain.make_forcing(d, 0, 2, start_doy=330)
    sd0, si0 = init_state.initial_state(d, f[0])
    depth = 3
    m = _start(d, f, sf, dmy, sd0, si0, 1, 0, depth)
    m.records_set_groups([0, 2], [0, 4], [0.5, 0.25], fill=7.0)          # the groups in force
    off, cell, w = np.asarray([0, 1, 3, 3], np.int32), np.asarray([1, 2, 3], np.int32), np.asarray([0.1, 0.2, 0.3])
    bad = []
    before = lib.hostemu_live_objects()
    for n in range(1, 50):
        lib.hostemu_refuse_alloc(n)
        rc = lib.vicgpu_records_set_groups(m.h, 3, off.ctypes.data_as(ip), cell.ctypes.data_as(ip), w.ctypes.data_as(dp), 0.0)
        lib.hostemu_refuse_alloc(0)
        if rc == 0:
            break
        if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or m.records_get_groups() != (1, 2):
            bad.append("allocation %d refused: code %d, %d objects more, groups %s" % (n, rc, lib.hostemu_live_objects() - before, m.records_get_groups()))
    if n != 3 + depth + 1:           # offsets, cells, weights and one table per slot were refused once each
        bad.append("%d refusals" % (n - 1))
    if m.records_get_groups() != (3, 3) or lib.hostemu_live_objects() != before:
        bad.append("after the call that got through: groups %s, %d objects more" % (m.records_get_groups(), lib.hostemu_live_objects() - before))
    # the groups that were kept through the refusals still worked: checked by running the new ones and the removal
    rec = m.run_records(0, 2, errors=True)
    rec.wait()
    if rec.out.shape[2] != 3 or not np.isfinite(rec.out).all():
        bad.append("the run after the refusals")
    del rec
    before = lib.hostemu_live_objects()          # with the events of the run
    m.records_set_groups(None, None)
    if lib.hostemu_live_objects() != before - (3 + depth):
        bad.append("%d objects left by the removal" % (lib.hostemu_live_objects() - before + 3 + depth))
    m.close()
    left = lib.hostemu_live_objects() - live0
    if left:
        bad.append("%d objects left after close" % left)
    print("record groups refusals: %d refused; problems: %s" % (n - 1, bad or "none"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        rc = 0
        for n in sys.argv[2:]:
            problems = run(n, CASES[n])
            print("record groups %s: problems: %s" % (n, problems or "none"), flush=True)
            rc = rc or (1 if problems else 0)
        sys.exit(rc)
    sys.exit({"errors": errors, "refusals": refusals}[sys.argv[1]]())
