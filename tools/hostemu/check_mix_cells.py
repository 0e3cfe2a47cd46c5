"""Model state combined linearly across cells on the device (vicgpu_mix_cells, include/vicgpu.h) against numpy written in the
contract's order: per destination acc = w0 * x[src0], then acc = acc + w_t * x[src_t], vectorised over destinations of equal
term count, in float64.  Every comparison is bit for bit, NaNs by position.  Run by tests/test_mix_cells.py with VICGPU_LIB
pointing at the unsanitized host build (SAN=none tools/hostemu/build.sh); tests/test_mix_cells_gpu.py imports the functions for
the GPU.
    python tools/hostemu/check_mix_cells.py dense         a random 4 x 4 member transform, 11 rows, two staging budgets
    python tools/hostemu/check_mix_cells.py percolumn     a 3-D W: every base column its own transform
    python tools/hostemu/check_mix_cells.py irregular     shuffled destinations, 1 / 2 / 3 / 65 terms, self and mutual terms
    python tools/hostemu/check_mix_cells.py special       -0.0, a denormal, +-inf, NaN; weights 0, -1, 1e-300; weight 1 = copy_cells
    python tools/hostemu/check_mix_cells.py untouched     what a call must leave alone; a retired destination
    python tools/hostemu/check_mix_cells.py midrun        FROZEN_SOIL as one chunk and as two, right behind a two-step vicgpu_step
    python tools/hostemu/check_mix_cells.py errors        every error return, each leaving every table as it was
    python tools/hostemu/check_mix_cells.py refusals      the n-th allocation refused, for every n
    python tools/hostemu/check_mix_cells.py large         4 members x 2 000 cells x 6 HRUs, 12 rows, then a derive
Each prints "mix cells <name>: problems: none" (or the list) and exits with 1 when there are any."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import check_copy_cells as cc
import check_state_update as su
import check_update_params as cu
from vic_amd import abi, domain
from vic_amd.abi import C
from vic_amd.api import Model, VicGpuError, load_library

same, differing = cc.same, cc.differing
model, clone = cu.model, cu.clone
CAP, NODES = C["VICGPU_DERIVE_CAP_MOIST"], C["VICGPU_DERIVE_NODES"]


def same_nan(a, b):
    """bit for bit, NaNs by position"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def hrus_by_position(D, cells, counts):
    """The first counts[i] HRUs of cells[i], in cell_hru_list order, concatenated."""
    off = D.cell_hru_offset.astype(np.int64)
    start = np.repeat(off[cells], counts)
    within = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
    return D.cell_hru_list[start + within]


def np_mix(D, sd, rows, dst, term_off, term_cell, term_weight):
    """The SD table after the call, from the table before it: the contract's order, every product and every sum one float64
    operation."""
    rows, dst, term_off, term_cell = (np.asarray(x, dtype=np.int64) for x in (rows, dst, term_off, term_cell))
    term_weight = np.asarray(term_weight, dtype=np.float64)
    out = sd.copy()
    x = sd[rows]
    nterm = np.diff(term_off)
    per_cell = np.diff(D.cell_hru_offset.astype(np.int64))
    with np.errstate(all="ignore"):
        for k in np.unique(nterm):
            sel = np.flatnonzero(nterm == k)
            nh = per_cell[dst[sel]]
            hd = hrus_by_position(D, dst[sel], nh)
            acc = None
            for q in range(int(k)):
                t = term_off[sel] + q
                hs = hrus_by_position(D, term_cell[t], nh)
                w = np.repeat(term_weight[t], nh)
                prod = w[None, :] * x[:, hs]
                acc = prod if acc is None else acc + prod
            out[np.ix_(rows, hd)] = acc
    return out


def started(E, stage_mb=None, steps=1):
    m = cc.start(model(E, clone(E.D), stage_mb=stage_mb), E)
    if steps:
        m.dist_prec(0, steps, sync=False)
    return m


def compare(m, D, rows, lists, bad, what):
    """One call on model m against np_mix of the state before it; returns the state after."""
    before = m.get_state()[0]
    m.mix_cells(rows, *lists)
    got = m.get_state()[0]
    want = np_mix(D, before, rows, *lists)
    if not same_nan(want, got):
        with np.errstate(all="ignore"):
            n = int((~((want == got) | (np.isnan(want) & np.isnan(got)))).sum())
        bad.append("%s: %d words differ from numpy" % (what, n))
    if same_nan(before, got):
        bad.append("%s: the call changed nothing" % what)
    return got


def mix_rows(D):
    """11 distinct SD rows, out of order: two row tiles, the second ragged"""
    Nn = D.opt.Nnode
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST2"], C["SD_MOIST0"], abi.sd_node(C["SDN_T"], 1, Nn), C["SD_GLAC_CUM_MASS_BALANCE"], C["SD_WDEW"],
                     abi.sd_node(C["SDN_CS"], Nn - 1, Nn), C["SD_MOIST1"], C["SD_SNOW_DEPTH"], C["SD_ICE1"], C["SD_TSURF"]], np.int32)
    assert len(set(rows.tolist())) == 11
    return rows


# ------------------------------------------------------------------------------------------------ 1. dense, 2. per column
def check_dense(log=print):
    E = cc.quickflux()
    D = E.D
    rows = mix_rows(D)
    rng = np.random.default_rng(21)
    W = rng.normal(size=(E.M, E.M))
    lists = domain.member_transform(E.M, E.ncol, W)
    bad, kept = [], []
    if D.nhru != 924 or D.ncell != 140 or len(rows) != 11:
        bad.append("the case: %d cells, %d HRUs, %d rows" % (D.ncell, D.nhru, len(rows)))
    named = set(rows.tolist())
    if not {C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"], abi.sd_node(C["SDN_T"], 1, D.opt.Nnode)} <= named:
        bad.append("the case: the rows")
    for stage in (None, "0"):
        m = started(E, stage)
        kept.append(compare(m, D, rows, lists, bad, "stage %s" % (stage or "default")))
        m.close()
    if not same_nan(kept[0], kept[1]):
        bad.append("one row per pass gives other bits than the default budget")
    log("mix cells dense: %d destinations x %d terms, %d rows, %d HRUs, differing: %s" % (len(lists[0]), E.M, len(rows), D.nhru, bad or "none"), flush=True)
    return bad


def check_percolumn(log=print):
    E = cc.quickflux()
    D = E.D
    rows = mix_rows(D)
    rng = np.random.default_rng(22)
    W = rng.normal(size=(E.ncol, E.M, E.M))
    lists = domain.member_transform(E.M, E.ncol, W)
    bad = []
    w = lists[3].reshape(E.M, E.ncol, E.M)
    if len(np.unique(w)) != w.size:
        bad.append("the case: weights repeat")
    m = started(E)
    compare(m, D, rows, lists, bad, "3-D W")
    m.close()
    log("mix cells percolumn: %d destinations, differing: %s" % (len(lists[0]), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 3. irregular terms
def irregular_lists(E):
    """(dst, term_off, term_cell, term_weight): destinations in shuffled order with 1, 2, 3 and 65 terms."""
    rng = np.random.default_rng(23)
    cell = lambda m, j: m * E.ncol + j
    nine = [c for c in range(E.ncol) if c % 5 == 0]
    D = {}
    D[cell(1, 3)] = [(cell(0, 3), 0.7)]
    D[cell(2, 4)] = [(cell(2, 4), 0.5), (cell(0, 4), 0.5)]                                     # a term of itself
    D[cell(3, 6)] = [(cell(0, 6), 0.25), (cell(1, 6), 1.5), (cell(0, 6), -0.75)]                # a source twice
    D[cell(0, 7)] = [(cell(q % E.M, 7), float(w)) for q, w in enumerate(rng.normal(size=65) / 8)]
    D[cell(1, 8)] = [(cell(2, 8), 0.25), (cell(1, 8), 0.75)]                                   # terms of each other
    D[cell(2, 8)] = [(cell(1, 8), 2.0), (cell(2, 8), -1.0)]
    D[cell(1, nine[0])] = [(cell(1, nine[1]), 0.3), (cell(1, nine[0]), 0.7)]                   # two nine-HRU cells of one member
    D[cell(1, nine[1])] = [(cell(1, nine[0]), 1.0)]
    for j in range(11, 35):                                                                    # and enough for several waves
        k = 1 + j % 3
        D[cell(j % E.M, j)] = [(cell((j + q) % E.M, j), float(rng.normal())) for q in range(k)]
    order = rng.permutation(len(D))
    dst = np.array(list(D), np.int32)[order]
    off, tc, tw = [0], [], []
    for d in dst:
        tc += [c for c, _ in D[int(d)]]
        tw += [w for _, w in D[int(d)]]
        off.append(len(tc))
    return dst, np.array(off, np.int32), np.array(tc, np.int32), np.array(tw)


def check_irregular(log=print):
    E = cc.quickflux()
    D = E.D
    rows = mix_rows(D)
    lists = irregular_lists(E)
    dst, off = lists[0], lists[1]
    bad = []
    counts = set(np.diff(off).tolist())
    nh = int(np.diff(D.cell_hru_offset)[dst].sum())
    if counts != {1, 2, 3, 65} or (np.diff(dst) > 0).all() or nh <= 128 or nh % 64 == 0:
        bad.append("the case: term counts %s, %d destination HRUs" % (sorted(counts), nh))
    m = started(E)
    compare(m, D, rows, lists, bad, "irregular")
    m.close()
    log("mix cells irregular: %d destinations, %d HRUs, %d terms, differing: %s" % (len(dst), nh, off[-1], bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 4. special values
def check_special(log=print):
    E = cc.quickflux()
    D = E.D
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"], C["SD_GLAC_CUM_MASS_BALANCE"]], np.int32)
    j = np.arange(E.ncol)
    cells = lambda m: (m * E.ncol + j).astype(np.int32)
    bad = []

    def planted():
        m = started(E)
        sd, si = m.get_state()
        h0 = cu.hrus_of(D, cells(0))
        for k, v in enumerate((-0.0, 5e-324, np.inf, -np.inf, np.nan)):
            sd[rows[k % 4], h0[k::5]] = v
        sd[C["SD_MOIST1"], cu.hrus_of(D, cells(3))[::4]] = np.inf                    # 1e-300 * inf; 0 * inf comes from member 0
        m.set_state(sd, si)
        return m, sd

    # member 1 <- 0 * m0 - 1 * m2 + 1e-300 * m3; member 2 <- 1 * m0
    dst = np.concatenate([cells(1), cells(2)])
    tc = np.concatenate([np.stack([cells(0), cells(2), cells(3)], axis=1).reshape(-1), cells(0)]).astype(np.int32)
    tw = np.concatenate([np.tile([0.0, -1.0, 1e-300], E.ncol), np.ones(E.ncol)])
    off = np.concatenate([3 * np.arange(E.ncol), 3 * E.ncol + np.arange(E.ncol + 1)]).astype(np.int32)
    m, sd = planted()
    got = compare(m, D, rows, (dst, off, tc, tw), bad, "special values")
    m.close()
    h1, h0 = cu.hrus_of(D, cells(1)), cu.hrus_of(D, cells(0))
    if not np.isnan(got[np.ix_(rows[:4], h1)][np.isnan(sd[np.ix_(rows[:4], h0)]) | np.isinf(sd[np.ix_(rows[:4], h0)])]).all():
        bad.append("0 * NaN or 0 * inf did not give NaN")
    if not np.isnan(sd[C["SD_GLAC_CUM_MASS_BALANCE"]]).any():
        bad.append("the case: SD_GLAC_CUM_MASS_BALANCE holds no NaN")
    # a single term of weight 1.0 against vicgpu_copy_cells(VICGPU_COPY_STATE)
    a, _ = planted()
    b, sd = planted()
    one = np.arange(E.ncol + 1, dtype=np.int32)
    a.mix_cells(rows, cells(2), one, cells(0), np.ones(E.ncol))
    b.copy_cells(cells(2), cells(0), Model.STATE)
    sa, sb = a.get_state()[0], b.get_state()[0]
    a.close(); b.close()
    if not same(sa[rows], sb[rows]):
        bad.append("a single term of weight 1.0 differs from copy_cells on the listed rows")
    if not same(sa[:, h0], sd[:, h0]):
        bad.append("the source changed")
    h2 = cu.hrus_of(D, cells(2))
    if not same(sa[np.ix_(rows, h2)], sd[np.ix_(rows, h0)]) or not np.signbit(sa[np.ix_(rows, h2)][sd[np.ix_(rows, h0)] == 0]).any():
        bad.append("weight 1.0 does not reproduce the source (or no -0.0 in it)")
    rest = np.setdiff1d(np.arange(sa.shape[0]), rows)
    if not same(sa[rest], sd[rest]):
        bad.append("unlisted rows changed")
    log("mix cells special: %d destinations, differing: %s" % (len(dst), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 5. untouched
def check_untouched(log=print):
    """A mid-run mix with put_data, records, cell groups, a forcing map and a retire mask in force; a retired destination."""
    E = cc.quickflux()
    D = E.D
    m = cc.start(model(E, clone(D)), E)
    m.records_config(cc.OUT, depth=2)
    m.records_set_groups(np.arange(0, D.ncell + 1, E.ncol, dtype=np.int32), np.arange(D.ncell, dtype=np.int32))
    m.set_retire_on_error(C["VICGPU_CELLERR_REFERENCE"])
    retired = 2 * E.ncol + 3
    valid = np.ones(D.ncell, np.int32); valid[retired] = 0
    m.dist_prec(0, 2)
    m.set_cell_valid(valid)

    def snapshot():
        t = su.full_tables(m)
        t["forcing"], t["snowflag"] = m.get_forcing(3)
        t["map"] = m.get_forcing_map()[1]
        return t, (m.lib.vicgpu_records_nrow(m.h), m.records_ncol(), m.records_get_groups(), m.get_forcing_map()[0])

    t0, cfg0 = snapshot()
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"]], np.int32)
    cols = np.array([3, 0, 7, 20, 34, 11], np.int32)
    W = np.array([[0.4, 0.1, 0.2, 0.3], [0.3, 0.6, 0.1, 0.2], [0.2, 0.2, 0.5, 0.1], [0.1, 0.1, 0.2, 0.4]])      # columns sum to 1
    lists = domain.member_transform(E.M, E.ncol, W, cols)
    m.mix_cells(rows, *lists)
    t1, cfg1 = snapshot()
    bad = [k + " changed" for k in differing(t0, t1) if k != "sd"]
    if cfg0 != cfg1:
        bad.append("the configuration changed: %s -> %s" % (cfg0, cfg1))
    want = np_mix(D, t0["sd"], rows, *lists)
    if not same_nan(want, t1["sd"]):
        bad.append("SD differs from numpy (unlisted rows and columns included)")
    hd = cu.hrus_of(D, lists[0])
    rest = np.setdiff1d(np.arange(D.nhru), hd)
    other = np.setdiff1d(np.arange(t0["sd"].shape[0]), rows)
    if not same(t0["sd"][:, rest], t1["sd"][:, rest]) or not same(t0["sd"][other], t1["sd"][other]):
        bad.append("unlisted SD rows or columns changed")
    hr = cu.hrus_of(D, [retired])
    if retired not in lists[0].tolist() or same(t0["sd"][np.ix_(rows, hr)], t1["sd"][np.ix_(rows, hr)]):
        bad.append("the retired destination did not take its values")
    if t1["valid"][retired] != 0:
        bad.append("the retired destination is valid again")
    rec = m.run_records(2, 1)
    rec.wait()
    if rec.out.shape[-1] != E.M or not np.isfinite(rec.out).all() or not rec.out.any():
        bad.append("the record after the mix")
    del rec
    m.close()
    log("mix cells untouched: %d destinations, differing: %s" % (len(lists[0]), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 6. mid-run
def check_midrun(log=print, chunks="2"):
    """The frozen pair of check_copy_cells.check_frozen: steps, mix_cells, steps with no synchronize in between, against the
    same run in which the host does get_state -> numpy -> set_state at that point.  State, fluxes and records."""
    os.environ["VICGPU_CHUNKS"] = chunks
    try:
        E = cc.ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 2, 2 + 2 * cc.R, 330, glacier=True)
        D = E.D
        Nn = D.opt.Nnode
        rows = np.array([C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"], C["SD_SNOW_SWQ"]] + [abi.sd_node(C["SDN_T"], n, Nn) for n in (1, 2, 3)], np.int32)
        W = np.array([[0.7, 0.4], [0.3, 0.6]])
        lists = domain.member_transform(E.M, E.ncol, W)
        a, b, n = cc.model(E), cc.model(E), cc.model(E)
        a.dist_prec(0, 2, sync=False)
        a.mix_cells(rows, *lists)
        ra = cc.run_records(a, 2, 2)
        b.dist_prec(0, 2)
        b.synchronize()
        sd, si = b.get_state()
        mixed = np_mix(D, sd, rows, *lists)
        b.set_state(mixed, si)
        rb = cc.run_records(b, 2, 2)
        n.dist_prec(0, 2)
        rn = cc.run_records(n, 2, 2)
        ta, tb, tn = (cc.tables(x) for x in (a, b, n))
        for x in (a, b, n):
            x.close()
        bad = ["after the steps: " + k for k in differing(tb, ta)]
        if not same(ra, rb):
            bad.append("the records after the mix")
        if same(tb["sd"], tn["sd"]) or same(rb, rn) or not np.isfinite(rb).all() or not np.isfinite(tb["cell_out"]).all():
            bad.append("the run with the mix does not differ from the run without, or is not finite")
        if same(mixed, sd) or not D.hru_iparams[C["HPI_IS_GLACIER"]].any():
            bad.append("the case: nothing to mix, or no glacier HRU")
    finally:
        os.environ.pop("VICGPU_CHUNKS", None)
    log("mix cells midrun (chunks %s): %d destinations, differing: %s" % (chunks, len(lists[0]), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 7. errors and refusals
def error_returns(log=print):
    """Every VICGPU_ERR_ARG / VICGPU_ERR_STATE return of the header, each followed by a comparison of all tables; then the call
    that follows works.  All of them are refused on the host before any launch."""
    lib = load_library()
    ARG, ST, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    NONE = object()
    checks = []

    def call(h, rows, dst, off, tc, tw, nrow=None, ndst=None):
        arrs = [None if x is None else i32(x) for x in (rows, dst, off, tc)]
        w = None if tw is None else np.asarray(tw, dtype=np.float64)
        nrow = (len(arrs[0]) if arrs[0] is not None else 0) if nrow is None else nrow
        ndst = (len(arrs[1]) if arrs[1] is not None else 0) if ndst is None else ndst
        P = lambda a: a.ctypes.data_as(ip) if a is not None else None
        return lib.vicgpu_mix_cells(h, nrow, P(arrs[0]), ndst, P(arrs[1]), P(arrs[2]), P(arrs[3]), w.ctypes.data_as(dp) if w is not None else None)

    E = cc.quickflux()
    D = E.D
    nc, nsd = D.ncell, abi.sd_nrow(D.opt.Nnode)
    odd = E.ncol + 3                 # member 1, base cell 3: its second HRU gets another vegetation class
    D.hru_iparams[C["HPI_VEG_CLASS"], D.cell_hru_list[D.cell_hru_offset[odd] + 1]] += 1
    R, A, B = [C["SD_MOIST0"], C["SD_SNOW_SWQ"]], 36, 1          # cells 36 and 1: member 1 and member 0 of base cell 1
    good = dict(rows=R, dst=[A, B], off=[0, 2, 3], tc=[A, B, A], tw=[0.5, 0.5, 1.0])

    def with_(**kw):
        d = dict(good); d.update(kw)
        return d["rows"], d["dst"], d["off"], d["tc"], d["tw"]

    checks.append(("null handle", call(None, *with_()), ARG))
    checks.append(("null handle, nothing to do", call(None, [], [], [0], [], []), ARG))
    fresh = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(fresh)) == 0
    checks.append(("no domain", call(fresh, *with_()), ST))
    checks.append(("no domain, nothing to do", call(fresh, [], [], [0], [], []), ST))
    checks.append(("no domain, nrow < 0", call(fresh, *with_(), nrow=-1), ARG))
    lib.vicgpu_destroy(fresh)
    m = cc.start(Model(D), E)
    m.dist_prec(0, 1)
    t0 = su.full_tables(m)
    inf, nan = float("inf"), float("nan")
    cases = [
        ("nrow < 0", lambda: call(m.h, *with_(), nrow=-1)),
        ("ndst < 0", lambda: call(m.h, *with_(), ndst=-1)),
        ("null rows", lambda: call(m.h, *with_(rows=None), nrow=2)),
        ("null dst_cell", lambda: call(m.h, *with_(dst=None), ndst=2)),
        ("null term_off", lambda: call(m.h, *with_(off=None))),
        ("null term_cell", lambda: call(m.h, *with_(tc=None))),
        ("null term_weight", lambda: call(m.h, *with_(tw=None))),
        ("row == nrows", lambda: call(m.h, *with_(rows=[0, nsd]))),
        ("row < 0", lambda: call(m.h, *with_(rows=[-1]))),
        ("a row listed twice", lambda: call(m.h, *with_(rows=[2, 1, 2]))),
        ("dst == ncell", lambda: call(m.h, *with_(dst=[A, nc]))),
        ("dst < 0", lambda: call(m.h, *with_(dst=[-1, B]))),
        ("a destination listed twice", lambda: call(m.h, *with_(dst=[A, A]))),
        ("term_off[0] != 0", lambda: call(m.h, *with_(off=[1, 2, 3]))),
        ("decreasing offsets", lambda: call(m.h, *with_(off=[0, 2, 1]))),
        ("the first destination has no term", lambda: call(m.h, *with_(off=[0, 0, 3]))),
        ("the last destination has no term", lambda: call(m.h, *with_(off=[0, 3, 3]))),
        ("term cell == ncell", lambda: call(m.h, *with_(tc=[A, nc, A]))),
        ("term cell < 0", lambda: call(m.h, *with_(tc=[A, B, -1]))),
        ("a NaN weight", lambda: call(m.h, *with_(tw=[0.5, nan, 1.0]))),
        ("an infinite weight", lambda: call(m.h, *with_(tw=[0.5, 0.5, inf]))),
        ("a negative infinite weight", lambda: call(m.h, *with_(tw=[-inf, 0.5, 1.0]))),
        ("HRU counts differ (a 9-HRU and a 6-HRU cell)", lambda: call(m.h, *with_(dst=[0, B], tc=[0, 1, A]))),
        ("vegetation class differs at one position", lambda: call(m.h, *with_(dst=[3, B], tc=[3, odd, A]))),
        ("... in the last term of the last destination", lambda: call(m.h, *with_(dst=[A, odd], tc=[A, B, 3 + 2 * E.ncol]))),
        ("... as the destination", lambda: call(m.h, *with_(dst=[odd, B], tc=[odd, 3, A]))),
    ]
    for w, f in cases:
        checks.append((w, f(), ARG))
        checks.append((w + ": tables", differing(t0, su.full_tables(m)) or "unchanged", "unchanged"))
    for w, f in [("nrow == 0", lambda: call(m.h, *with_(rows=[]))), ("ndst == 0", lambda: call(m.h, R, [], [0], [], [])),
                 ("nrow == 0, null lists", lambda: call(m.h, None, None, None, None, None)),
                 ("ndst == 0, null lists", lambda: call(m.h, R, None, None, None, None)),
                 ("nrow == 0, lists that would be refused", lambda: call(m.h, [], [A, A], [0, 0, 0], [], []))]:
        checks.append((w, f(), OK))
    checks.append(("tables after the no-ops", differing(t0, su.full_tables(m)) or "unchanged", "unchanged"))
    for w, args, words in [("an incompatible pair", with_(dst=[3, B], tc=[3, odd, A]), ("destination 0", "term 1", "vegetation")),
                           ("a weight", with_(tw=[0.5, 0.5, nan]), ("destination 1", "term 2", "finite")),
                           ("a row", with_(rows=[1, 1]), ("listed twice",))]:
        try:
            m.mix_cells(*args)
            checks.append(("Model.mix_cells raises for " + w, False, True))
        except VicGpuError as e:
            checks.append(("Model.mix_cells names %s: %s" % (w, e), all(x in str(e) for x in words), True))
    # the call that follows works, and the odd cell may be mixed with itself
    checks.append(("the call that follows", call(m.h, *with_()), OK))
    checks.append(("the odd cell with itself", call(m.h, R, [odd], [0, 2], [odd, odd], [0.5, 0.25]), OK))
    t1 = su.full_tables(m)
    want = np_mix(D, np_mix(D, t0["sd"], *with_()), R, [odd], [0, 2], [odd, odd], [0.5, 0.25])
    checks.append(("... changed SD alone", differing(t0, t1), ["sd"]))
    checks.append(("... as numpy does", same_nan(want, t1["sd"]), True))
    m.close()
    failed = [(w, got, want) for w, got, want in checks if got != want]
    for w, got, want in failed:
        log("mix cells return: %s gave %s, want %s" % (w, got, want), flush=True)
    log("mix cells errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return ["%s gave %s" % (w, got) for w, got, _ in failed], len(checks)


def check_refusals(log=print):
    """vicgpu_mix_cells under a runtime that refuses its n-th allocation, n = 1, 2, ...: VICGPU_ERR_HIP, no live runtime object
    added and every table as it was, until the call gets through -- which leaves no object behind either."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    E = cc.quickflux()
    rows = np.array([C["SD_MOIST0"], C["SD_MOIST1"], C["SD_SNOW_SWQ"]], np.int32)
    dst, off, tc, tw = domain.member_transform(E.M, E.ncol, np.random.default_rng(4).normal(size=(E.M, E.M)))
    P = lambda a: a.ctypes.data_as(ip)
    bad = []
    m = started(E)
    t0 = su.full_tables(m)
    before = lib.hostemu_live_objects()
    for n in range(1, 20):
        lib.hostemu_refuse_alloc(n)
        rc = lib.vicgpu_mix_cells(m.h, len(rows), P(rows), len(dst), P(dst), P(off), P(tc), tw.ctypes.data_as(dp))
        lib.hostemu_refuse_alloc(0)
        if rc == 0:
            break
        if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or differing(t0, su.full_tables(m)):
            bad.append("allocation %d refused: code %d, %d objects more, changed %s" % (n, rc, lib.hostemu_live_objects() - before, differing(t0, su.full_tables(m))))
    if lib.hostemu_live_objects() != before:
        bad.append("%d objects left by the call that got through" % (lib.hostemu_live_objects() - before))
    if differing(t0, su.full_tables(m)) != ["sd"]:
        bad.append("the call that got through changed %s" % differing(t0, su.full_tables(m)))
    m.close()
    if n - 1 != 3:                                           # the lists, the weights and the stage
        bad.append("%d refusals" % (n - 1))
    log("mix cells refusals: %d refused; problems: %s" % (n - 1, bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 8. a larger case
def check_large(log=print, stage_mb=None):
    """4 members x 2 000 cells x 6 HRUs (QUICK_FLUX): a dense 4 x 4 transform on 12 rows of all 48 000 HRUs, then a derive over
    all of them."""
    E = cc.ensemble(dict(FULL_ENERGY=1, Nband=3), 2000, 4, 2, 1, 80)
    D = E.D
    Nn = D.opt.Nnode
    rows = np.concatenate([su.layer_rows("SD_MOIST"), su.layer_rows("SD_ICE"), [C["SD_SNOW_SWQ"], C["SD_SNOW_DEPTH"], C["SD_WDEW"], C["SD_TSURF"], C["SD_SNOW_SURF_TEMP"]],
                           [abi.sd_node(C["SDN_T"], 0, Nn)]]).astype(np.int32)
    W = np.random.default_rng(8).uniform(0.1, 1.0, size=(E.M, E.M))
    W /= W.sum(axis=0, keepdims=True)                        # every analysis member a convex combination
    lists = domain.member_transform(E.M, E.ncol, W)
    m = su.begin(model(E, clone(D), stage_mb), E)
    bad = []
    if len(rows) != 12 or D.nhru != 48000 or len(lists[0]) != 8000:
        bad.append("the case: %d rows, %d HRUs, %d destinations" % (len(rows), D.nhru, len(lists[0])))
    compare(m, D, rows, lists, bad, "large")
    try:
        m.derive_soil_state(CAP | NODES)
    except VicGpuError as e:
        bad.append("derive_soil_state: %s" % e)
    sd = m.get_state()[0]
    m.close()
    if not np.isfinite(sd[su.node_rows(Nn)]).all():
        bad.append("the node blocks after the derive are not finite")
    log("mix cells large (stage %s MB): %d rows x %d HRUs, differing: %s" % (stage_mb or "default", len(rows), D.nhru, bad or "none"), flush=True)
    return bad


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "errors":
        problems, _ = error_returns()
    else:
        both_chunkings = lambda: check_midrun(chunks="1") + check_midrun(chunks="2")
        problems = {"dense": check_dense, "percolumn": check_percolumn, "irregular": check_irregular, "special": check_special, "untouched": check_untouched,
                    "midrun": both_chunkings, "refusals": check_refusals, "large": check_large}[cmd]()
    print("mix cells %s: problems: %s" % (cmd, problems or "none"), flush=True)
    sys.exit(1 if problems else 0)
