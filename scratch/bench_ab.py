"""bench.py with engine switches set from the command line (A/B on one box):
   python scratch/bench_ab.py <spec> [bench.py arguments]      spec: comma list of  off | on | parts=N | nofuse | nobranch | serial"""
import os, sys, runpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buctd_amd import ops
for tok in sys.argv[1].split(","):
    if tok == "off":
        ops.set_group_branches(False)
    elif tok.startswith("parts="):
        ops.set_group_parts(int(tok[6:]))
    elif tok == "nofuse":
        ops.conv_bn_group_ok = lambda xs, layers: False
    elif tok == "nobranch":
        ops.group_branches_ok = lambda xs, chains: False
    elif tok == "serial":           # no branch streams, no weight-gradient stream: every kernel on the compute stream
        ops.set_stream_forks(False, False)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
