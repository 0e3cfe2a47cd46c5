"""The device's root finders (vic_math.hpp Brent and BrentLean) pinned to the reference's RootBrent::root_brent
(root_brent.c:97-337) evaluation by evaluation, on the battery of tests/brent_cases.py.

tests/golden/brent_traces.npz holds the reference's run of every case (tests/golden/make_golden_brent.py).  On the CPU: the
battery covers every path of root_brent.c, regenerates the fixture's inputs, and the reference (when present), the oracle
and the Python transcription each reproduce the fixture bit for bit; functions with a known root end within 2 tol of it;
the host build of the device code replays the fixture bit for bit (tests/test_hostemu_sanitizers.py::
test_brent_battery_clean).  On the GPU: vicgpu_debug_root_brent replays every case
(Brent bit for bit in several lane arrangements, BrentLean up to its documented difference).
"""
import os

import numpy as np
import pytest

from tests import brent_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return bc.load_fixture()


@pytest.fixture(scope="module")
def battery(fixture):
    return bc.fixture_battery(fixture)


# ------------------------------------------------------------------------------------------------ CPU
def test_battery_covers_every_path(battery):
    """The battery cannot thin out quietly: a minimum count per path of root_brent.c and per class of case."""
    cases, runs = battery
    cnt = bc.count_labels(runs, cases)
    least = {
        # bracket and expansion
        "bracketed": 300, "expand_1": 50, "expand_2": 40, "expand_3": 30, "expand_4": 20, "expand_5": 10, "expand_fail": 50,
        "equal_bounds": 20,
        # ERROR paths
        "err_a": 40, "err_b": 40, "err_both": 20, "search0_1": 10, "search0_2": 5, "search0_many": 5, "search0_exhausted": 2,
        "exp_one_fail_up": 10, "exp_one_fail_down": 10, "search1": 40, "search1_halving": 20, "search1_exhausted": 2,
        "main_err_first": 10, "main_err_late": 10,
        # main loop
        "stop_m": 300, "stop_m_eq": 10, "stop_fb0": 50, "step_tol": 300, "step_tol_eq": 5, "secant": 300, "iqi": 200,
        "accept": 300, "reject_t1": 20, "reject_t2": 20, "reject_t1_only": 1, "swap": 300, "swap_tie": 50, "bisect_fa": 50,
        "bisect_fa_tie": 50, "bisect_e": 20, "tol_rel": 100,
        # sign tests at the edge of the number range
        "zero_at_end": 30, "underflow_product": 10, "subnormal_main": 20,
        # classes
        "cls:err_minus999_number": 10, "cls:trace_surf": 150, "cls:trace_node": 150, "cls:script_long": 2,
        "cls:script_step_tol_eq": 5, "cls:script_m_eq_tol": 10,
    }
    short = {k: (cnt.get(k, 0), v) for k, v in least.items() if cnt.get(k, 0) < v}
    assert not short, short
    assert 1500 <= len(cases) <= 2500
    # the traces are what their names say: surface-type brackets (ground surface +-1 K or (T0 - 1, 0), snow pack and
    # glacier +-5 K, canopy) are wider than a node's T0 +- 0.25 K, and every node trace has a node's bracket
    w = {cls: np.array([c.upper - c.lower for c in cases if c.cls == cls]) for cls in ("trace_surf", "trace_node")}
    assert w["trace_surf"].min() > 0.6, w["trace_surf"].min()
    assert np.abs(w["trace_node"] - 0.5).max() < 1e-12
    assert max(R.nmain for R in runs) >= 200
    assert sum(len(R.fs) > 1000 for R in runs) >= 2                 # the searches run to MAXITER


def test_fixture_is_current(fixture, battery):
    """Regenerating the battery gives the fixture's inputs bit for bit (and the transcription its outputs)."""
    cases, runs = battery
    p = bc.pack(cases, runs)
    for k in ("bounds", "off", "fs", "xs", "result", "failed", "cls", "trace_src"):
        assert p[k].shape == fixture[k].shape and (bc.same_bits(p[k], fixture[k]) if p[k].dtype == np.float64
                                                   else np.array_equal(p[k], fixture[k])), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "brent_traces.npz")) < 300 * 1000


def test_traces_rerecorded(oracle_lib, fixture):
    """The fixture's traces are what the oracle's model runs solve: re-recorded, every trace of the runs that take seconds
    (all but the 50-node one) has the same kind, bounds and values bit for bit."""
    src = fixture["trace_src"]
    n = 0
    for r, (name, nsteps) in enumerate(bc.TRACE_RUNS):
        if name == "deep_spikes_n50":
            continue
        solves = {s[0]: s for s in bc.record_solves(name, nsteps)}
        for i in np.flatnonzero(src[:, 0] == r):
            solve, kind, lo, hi, _, _, xs, fs = solves[int(src[i, 1])]
            o0, o1 = fixture["off"][i], fixture["off"][i + 1]
            assert fixture["cls"][i] == "trace_" + kind, (name, i)
            assert bc.same_bits(fixture["bounds"][i], [lo, hi]) and bc.same_bits(fixture["fs"][o0:o1], fs), (name, i)
            assert bc.same_bits(fixture["xs"][o0:o1], xs), (name, i)
            n += 1
    assert n >= 200, n


def _each(fixture, battery, run):
    """run(case) -> (result, xs, fs) against the fixture, bit for bit."""
    cases, runs = battery
    bad = []
    for i, c in enumerate(cases):
        o0, o1 = fixture["off"][i], fixture["off"][i + 1]
        r, xs, fs = run(c)
        if not (bc.same_bits(xs, fixture["xs"][o0:o1]) and bc.same_bits(fs, fixture["fs"][o0:o1])
                and bc.same_bits(r, fixture["result"][i])):
            bad.append("case %d (%s) [%r, %r]" % (i, c.cls, c.lower, c.upper))
    assert not bad, "\n".join(bad[:20])


def test_transcription_equals_fixture(fixture, battery):
    _each(fixture, battery, lambda c: (lambda R: (R.result, R.xs, R.fs))(bc.transcribe(c.lower, c.upper, c.make())))


def test_oracle_equals_fixture(oracle_lib, fixture, battery):
    """orc_root_brent, and orc_root_brent_tol with the node tolerances for the node traces."""
    def run(c):
        if c.cls == "trace_node":
            return oracle_lib.oracle_root_brent(c.lower, c.upper, c.make(), bc.MACHEPS, bc.TTOL)
        return oracle_lib.oracle_root_brent(c.lower, c.upper, c.make())
    _each(fixture, battery, run)


def test_reference_equals_fixture(fixture, battery, ref_available):
    """The reference itself, live, where it is present; its error string is set exactly on failure."""
    from oracle import pyref
    if not pyref.have_ref("plain"):
        pytest.skip("reference harness not built")
    fails = []

    def run(c):
        r, xs, fs, err = pyref.ref_root_brent(c.lower, c.upper, c.make())
        fails.append(bool(err))
        return r, xs, fs
    _each(fixture, battery, run)
    assert np.array_equal(np.array(fails), fixture["failed"])


def test_known_roots(battery):
    """Functions with a known root r: a successful result lies within 2 tol(r) of it (Brent's own guarantee; of the
    nearest one where there are several)."""
    cases, runs = battery
    bad, n = [], 0
    for c, R in zip(cases, runs):
        if c.mp_root is None or R.failed:
            continue
        n += 1
        r = min(c.mp_root, key=lambda v: abs(R.result - v)) if isinstance(c.mp_root, tuple) else c.mp_root
        tol = 2 * bc.MACHEPS * abs(r) + bc.TTOL
        if not abs(R.result - r) <= 2 * tol:
            bad.append("%s [%r, %r]: %r vs root %r" % (c.cls, c.lower, c.upper, R.result, c.mp_root))
    assert n >= 500 and not bad, (n, bad[:20])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    from tests import node_cases as nc
    return nc.hook_model()


def _replay(model, g, idx, mode=0):
    from vic_amd.abi import C
    b, f, off = bc.gather(g, idx)
    return model.debug_root_brent(C["VICGPU_BRENT_LEAN"] if mode else C["VICGPU_BRENT_FULL"], b, f, off)


@pytest.mark.gpu
def test_brent_replay(model, fixture, battery):
    """Every case, natural order: every abscissa, the count, no overrun, result, failure and counters bit for bit."""
    cases, runs = battery
    n = len(runs)
    xreq, out = _replay(model, fixture, list(range(n)))
    bad = bc.check_full(fixture, runs, xreq, out)
    longest = int(np.argmax(np.diff(fixture["off"])))
    print("brent replay: %d cases, %d evaluations, longest %d (%s), longest main loop %d" % (
        n, int(fixture["off"][-1]), int(np.diff(fixture["off"])[longest]), fixture["cls"][longest], max(R.nmain for R in runs)))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_brent_lane_independence(model, fixture, battery):
    """A seeded permutation, each case alone, and each case in a wave whose other 63 lanes replay the longest case."""
    cases, runs = battery
    n = len(runs)
    perm = list(np.random.default_rng(5).permutation(n))
    xreq, out = _replay(model, fixture, perm)
    bad = bc.check_full(fixture, runs, xreq, out, perm)
    longest = int(np.argmax(np.diff(fixture["off"])))
    for i in range(n):
        xreq, out = _replay(model, fixture, [i])
        bad += bc.check_full(fixture, runs, xreq, out, [i])
        idx = [longest] * 64
        idx[i % 64] = i
        xreq, out = _replay(model, fixture, idx)
        bad += bc.check_full(fixture, runs, xreq, out, idx)
        if len(bad) > 20:
            break
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_brent_lean_replay(model, fixture, battery):
    """BrentLean on the ERROR-free cases: the reference's abscissae up to the first divergence, which is an interpolation
    step a few ulp off or a near-tie of the reference's acceptance test; without one, the same count and result."""
    cases, runs = battery
    idx = bc.lean_cases(fixture)
    assert len(idx) >= 1000
    xreq, out = _replay(model, fixture, idx, mode=1)
    bad, div = bc.check_lean(fixture, runs, xreq, out, idx)
    print("brent lean: %d cases, %d diverge (%d in an accepted step, %d at a near-tie), largest step difference %.3e "
          "(bound %.0e): %s" % (len(idx), len(div), sum(d[2] == "step" for d in div), sum(d[2] == "tie" for d in div),
                               max([d[3] for d in div] or [0.0]), bc.LEAN_STEP_REL,
                               ", ".join("%s@%d" % (fixture["cls"][i], k) for i, k, _, _ in div[:20])))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_brent_lean_reads_minus999_as_number(model, fixture):
    """The documented difference: a residual of exactly -999.0 is ERROR for Brent (a bisection search toward the valid
    end) and a number for BrentLean (fa * fb >= 0: both ends move out by TSTEP)."""
    idx = [i for i in range(len(fixture["cls"])) if fixture["cls"][i] == "err_minus999_number"]
    assert idx
    for i in idx:
        lo, hi = fixture["bounds"][i]
        xf, of = _replay(model, fixture, [i])
        xl, ol = _replay(model, fixture, [i], mode=1)
        assert fixture["fs"][fixture["off"][i]] == bc.ERROR
        assert xf[2] == 0.5 * (lo + hi) and xl[2] == lo - bc.TSTEP, (i, xf[:3], xl[:3])
