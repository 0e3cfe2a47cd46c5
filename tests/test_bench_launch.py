"""bench.py's own launcher (CPU test): `python bench.py --gpus N` with no WORLD_SIZE in the environment must start N
ranks itself -- one process per GPU through torch.distributed.run -- before it touches the GPU; a rank count that does
not match --gpus is an error, never a silent 1-GPU run.  `--launch-check` makes the ranks rendezvous over gloo and
report instead of benchmarking, so the test needs no GPU.  Also: --steps is honoured exactly, --dump-outputs writes
finite, bounded, repeatable files (on a stand-in model here, on a real one in the GPU test), and a plain run leaves the
measurements that take runs of their own to --full (GPU test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                              "TORCHELASTIC_RUN_ID")}
    return env


def test_gpus_2_starts_two_ranks():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout                    # rank 0 prints ONE line
    r = json.loads(lines[0])
    assert r["gpus_requested"] == 2 and r["ranks_seen"] == 2
    assert len(set(r["pids"])) == 2 and os.getpid() not in r["pids"]


def test_rank_count_mismatch_is_an_error():
    env = dict(_env(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE 1" in p.stderr


def test_steps_must_be_honoured_exactly():
    """--steps is the number of timed steps: a count the workload cannot time exactly is refused, never rounded."""
    for extra in (["--steps", "0"], ["--config", "cfg5", "--steps", "30"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, env=_env(), cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode != 0 and "--steps" in p.stderr, (extra, p.stderr[-2000:])


class _FakeModel:
    """What bench.dump_outputs reads of a Model, on the host, larger than the dump's sample sizes."""

    def __init__(self, ncell, nhru):
        from types import SimpleNamespace
        self.dom = SimpleNamespace(ncell=ncell, nhru=nhru)

    def get_state(self):
        sd = np.arange(108 * self.dom.nhru, dtype=np.float64).reshape(108, -1)
        sd[34] = np.nan                      # a marker row (no glacier accumulation window open)
        sd[35, ::3] = np.nan
        return sd, np.ones((37, self.dom.nhru), dtype=np.int32)

    def get_output_data(self, names, aggregated=False):
        return np.arange(9 * self.dom.ncell, dtype=np.float64).reshape(9, -1)

    def get_accum(self):
        return np.ones((10, self.dom.ncell))

    def get_cell_errors(self):
        return np.zeros(self.dom.ncell, dtype=np.int32)


def test_dump_outputs_is_bounded_and_repeatable(tmp_path):
    """--dump-outputs: finite float32 / float64 .npy files, at most 64 MB in all, the same sample of cells and HRUs every run."""
    sys.path.insert(0, ROOT)
    import bench
    m = _FakeModel(ncell=300000, nhru=50000)
    assert m.dom.ncell > bench.DUMP_MAX_CELLS and m.dom.nhru > bench.DUMP_MAX_HRUS
    table = np.arange(9 * 300000, dtype=np.float32).reshape(9, -1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, table)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "output_table.npy" in names and "state_double.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
        assert np.isfinite(a).all(), n
    assert total <= 64 << 20
    # the NaN markers of the state are kept as a mask beside the finite values
    hrus = np.load(tmp_path / "a" / "hrus.npy").astype(np.int64)
    want = m.get_state()[0][:, hrus]
    defined = np.load(tmp_path / "a" / "state_double_defined.npy")
    assert np.array_equal(defined == 1, ~np.isnan(want))
    assert np.array_equal(np.load(tmp_path / "a" / "state_double.npy")[defined == 1], want[~np.isnan(want)])
    assert "output_table_defined.npy" not in names           # arrays without markers are written as they are
    cols = np.load(tmp_path / "a" / "output_table_cells.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "output_table.npy"), table[:, cols])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ["cfg3", "cfg4"])
def test_dump_outputs_of_a_model_are_finite(cfg_name, tmp_path):
    """bench.dump_outputs on a small model of the bench workload after a few steps: every file finite, the state's NaN
    markers (SD_GLAC_CUM_MASS_BALANCE outside a glacier's accumulation window) exactly where get_state has them."""
    sys.path.insert(0, ROOT)
    import bench
    from vic_amd import domain, init_state
    from vic_amd.abi import C
    from vic_amd.api import Model
    cfg = bench.config(cfg_name)
    d = domain.make_domain(64, cfg["opt"], ntile=cfg["ntile"], glacier_top_band=cfg.get("glacier", False))
    f, sf, dmy = domain.make_forcing(d, 0, 3, start_doy=cfg["start_doy"])
    sd0, si0 = init_state.initial_state(d, f[0])
    if cfg.get("glacier"):
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    m = Model(d)
    try:
        m.set_state(sd0, si0); m.set_write_fluxes(False); m.put_data_config(bench.OUT_STEP_RATIO); m.put_data_init()
        m.push_forcing(f, sf, dmy)
        m.dist_prec(0, 3)
        table = m.get_outputs(bench.OUT_VARS, reset=False)
        bench.dump_outputs(str(tmp_path), m, table)
        sd, _ = m.get_state()
    finally:
        m.close()
    for n in os.listdir(tmp_path):
        a = np.load(tmp_path / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert np.array_equal(np.load(tmp_path / "state_double_defined.npy") == 1, ~np.isnan(sd))
    assert np.array_equal(np.load(tmp_path / "output_table.npy"), table)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,steps,warmup", [("cfg3", 6, 1), ("cfg5", 24, 6)])
def test_plain_run_leaves_the_extra_legs_to_full(cfg_name, steps, warmup):
    """A plain run prints the headline line with the extra legs' figures null; --full measures them after the timed region
    (the CPU baseline, host time only, is left out here).  Small domains via --ncell."""
    def run(*extra):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", cfg_name, "--ncell", "2000",
                            "--steps", str(steps), "--warmup", str(warmup)] + list(extra), env=_env(), cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])
    plain = run()
    full = run("--full", "--no-cpu-baseline")
    for r in (plain, full):
        assert r["metric"] == "cell-timesteps/s" and r["unit"] == "cell-timesteps/s" and r["higher_is_better"] is True
        assert r["dtype"] == "f64" and r["steps"] == steps and r["value"] > 0 and r["ms_per_step"] > 0
        assert r["config"]["cells_with_error_flags"] == 0
    assert plain["config"]["full"] is False and full["config"]["full"] is True
    if cfg_name == "cfg3":
        legs = ("strict_replay_ms_per_step", "compat_ms_per_step", "streamed_raw_forcing_ms_per_step")
        assert plain["cpu_baseline"]["value"] is None and plain["cpu_baseline"]["sample"].startswith("not measured")
    else:
        legs = ("resident_forcing_ms_per_step", "chunk_upload_and_derive_ms_per_step", "state_save_ms")
        assert plain["config"]["streamed_state_equals_resident"] is None
        assert full["config"]["streamed_state_equals_resident"] is True and full["config"]["state_record_bytes"] > 0
    for k in legs:
        assert plain["config"][k] is None and full["config"][k] > 0, k
