"""bench.py with vicgpu_set_retire_on_error(VICGPU_CELLERR_REFERENCE) on every Model it makes (tools/ab.sh, MASK_LINE=1): no
cell of the benchmark fails, so the run measures what the validity table costs when it is in use -- one int row per wave in
the HRU kernels, one word per cell in the cell-level kernels.  Same arguments and same JSON line as bench.py."""
import os
import runpy
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: before the library, as in bench.py)
from vic_amd import api  # noqa: E402
from vic_amd.abi import C  # noqa: E402

_init = api.Model.__init__


def _init_with_mask(self, *args, **kw):
    _init(self, *args, **kw)
    self.set_retire_on_error(C["VICGPU_CELLERR_REFERENCE"])


api.Model.__init__ = _init_with_mask
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
