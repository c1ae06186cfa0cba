"""usage: bench_with_clip.py MAX_NORM [bench.py arguments] : bench.py as it stands, with engine.get_optimizer handing out its
optimizer with max_grad_norm = MAX_NORM (bench.py itself has the option off) - the step time with the gradient-norm clip."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buctd_amd import engine  # noqa: E402

max_norm = float(sys.argv[1])
plain = engine.get_optimizer
engine.get_optimizer = lambda cfg, model, max_grad_norm=None: plain(cfg, model, max_grad_norm=max_norm)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
