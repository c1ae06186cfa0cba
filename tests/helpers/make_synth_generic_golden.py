"""Writes tests/golden/pose_synthesis_generic.npz: what the REFERENCE's generic pose synthesis (synthesize_pose with a
DATASET.DATASET other than coco / crowdpose, i.e. synthesize_pose_fish) produces on the scenes of
tests/helpers/synth_generic_ref.py, as per-joint class counts.  Run where the reference checkout is, from the
repository root; it is not needed to run the tests:

    python -m tests.helpers.make_synth_generic_golden /path/to/reference [runs]

The reference's lib/dataset/pose_synthesis.py (pure numpy / random) is imported from the path, the way
oracle/make_golden.py:pose_synthesis_case does it.  Per scene it is run `runs` (1500) times beside the table-driven CPU
twin; both outputs are classified geometrically (good, jitter, inversion, swap, miss, dropped) and the two frequency
tables must agree within sampling noise before anything is written.  Only counts and scene parameters are stored."""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import synth_generic_ref as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_synthesis_generic.npz")


class _C(dict):
    __getattr__ = dict.__getitem__


def main(ref_root, runs=1500):
    spec = importlib.util.spec_from_file_location("ref_pose_synthesis", os.path.join(ref_root, "lib/dataset/pose_synthesis.py"))
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    rec = {"runs": np.int64(runs), "scenes": np.array(G.SCENES, dtype=np.int64)}
    worst = 0.0
    for i, (K, n_ann, ov, n_near, seed) in enumerate(G.SCENES):
        cfg = _C(MODEL=_C(NUM_JOINTS=K), DATASET=_C(DATASET="fish"))
        joints, est, near, area = G.make_scene(K, n_ann, n_near, seed)
        T = G.generic_tables(K)
        np.random.seed(11 + i)
        random.seed(11 + i)
        ref_out, twin_out = np.zeros((runs, K, 3)), np.zeros((runs, K, 3))
        for it in range(runs):
            ref_out[it] = ps.synthesize_pose(cfg, joints.copy(), est.copy(), near.copy(), area, ov)
            twin_out[it] = G.synthesize_pose(T, joints, est, near, area, ov, seed=1000 + it)
        assert not ref_out[:, :, 2].any() and not twin_out[:, :, 2].any(), "visibility column convention"
        ref = G.class_counts(ref_out, joints, est, near, area)
        twin = G.class_counts(twin_out, joints, est, near, area)
        fr, fo = ref / runs, twin / runs
        tol = 4.0 * np.sqrt(np.maximum(fr * (1 - fr), 1e-3) * 2 / runs) + 0.004
        bad = np.abs(fr - fo) > tol
        assert not bad.any(), f"scene {i}: class frequencies differ from the reference at {np.argwhere(bad).tolist()}:\n" \
                              f"{fr[bad]} vs {fo[bad]}"
        gap = float(np.abs(fr - fo).max())
        pooled = float(np.abs(fr.mean(0) - fo.mean(0)).max())
        worst = max(worst, gap)
        rec[f"scene{i}_ref_counts"] = ref.astype(np.int64)
        print(f"  scene {i} (K {K}, {n_ann} annotated, num_overlap {ov}, {n_near} neighbours): {runs} runs, max per-joint "
              f"class-frequency gap to the reference {gap:.4f}, pooled over the joints {pooled:.4f}")
        print("    reference, pooled over the joints: " + ", ".join(f"{n} {v:.4f}" for n, v in zip(G.CLASSES, fr.mean(0))))
        print("    twin,      pooled over the joints: " + ", ".join(f"{n} {v:.4f}" for n, v in zip(G.CLASSES, fo.mean(0))))
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); largest per-joint gap {worst:.4f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1500)
